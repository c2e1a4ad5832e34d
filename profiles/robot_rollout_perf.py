#!/usr/bin/env python3
"""Multi-cycle robot rollouts (salp_robot_vec_rollout / salp_robot_vec_rollout_policy) against the host loop they replace,
and the rollout kernel's service period M (csrc/salp_robot_kernels.h).  On the GPU box.
    python profiles/robot_rollout_perf.py [--envs 4096,262144] [--horizon 16] [--rounds 5] [--window 0.5] [--out FILE]
    python profiles/robot_rollout_perf.py --sampled [--envs 4096] ...      the sampled rollout against its deterministic twin

Rows: env count x action mix (Box-wide: coast 0-10 s; short: coast <= 1 s) x loop (open: recorded actions; closed: a linear
and a 64 x 64 tanh policy).  Forms of a row, each on an env of its own (same seed):
    step loop     the path without this feature: H `step` calls on the recorded actions; closed loop: `sac.Actor` forward
                  (deterministic) + `step`, H times.  The cycle-length schedule stays at its default (on from 32768 envs).
    M = 0         the rollout kernel, synchronised form (a wavefront's lanes go cycle by cycle)
    M = 32, 128, 512   a lane whose cycle has ended waits at most M Euler iterations for its next one
Method: device events around `calls` back-to-back calls, `calls` chosen so that a window lasts `--window` seconds; every
form is warmed up first; the forms of a row are ALTERNATED inside each of `--rounds` rounds, and a row reports the median
over the rounds and the spread (max - min) / median of each form's identical repeats.  Closed-loop envs are reset before every
window so that every form starts its episodes from rest; the policies' output layers are scaled up so that their actions
spread over the Box (the mean and the largest cycle length of a row are printed).  M is read by the library at create
(SALP_ROBOT_ROLLOUT_M), which is how one process holds all four.

--sampled: salp_robot_vec_rollout_policy_sampled against salp_robot_vec_rollout_policy at the library's default M, same
method (alternated rounds, envs reset before every window).  Forms of a row, each on an env of its own (same seed), all
with `want_actions=False`:
    mean              the deterministic rollout on the Gaussian policy's handle
    sampled, sd -> 0  the sampled rollout with every log-std bias at -25 (clamped to -20: a standard deviation of 2e-9), so
                      that the actions, the cycle lengths and the simulator's work are the mean run's and the difference is
                      what sampling itself costs: two Philox blocks, three Box-Muller draws, the log-std head, the
                      log-probability and the logp store
    sampled, ls = -1  log-std biases of -1: other actions, so other cycle lengths (printed) — what a learner would run

--evaluate [--envs 4096] [--parent-lib LIB.so] [--launches 25] [--episode-cycles 500] [--episode-launches 5]:
salp_robot_vec_evaluate_policy (include/salp_robot_evaluate.h).  One GPU process; every launch is timed on its own with
device events, the forms alternated, each env reset before each launch; a row reports the median, the spread
(max - min) / median and the interquartile range / median.
    row 1   the 64 x 64 policy, Box-wide coast: `rollout_policy(..., want_actions=False)["reward"].sum(0)` — on the library
            given by --parent-lib, a build of the commit before the evaluation calls — against `evaluate_policy`; the row
            also says whether the records were, bit for bit, `summarize_robot_rollout` of the per-step blocks
    row 2   the population of examples/evaluate_robot_policy.py (64 linear policies x 64 robots) for 500 cycles:
            `evaluate_policy` with and without `first_episode`, and the Euler steps each simulated"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

PERIODS = (0, 32, 128, 512)
MIXES = {"box": 1.0, "short": 0.1}          # upper end of the coast component


def make_env(n, period=None):
    from underwater_swimmer_rl_amd.robot_env import SalpRobotVectorEnv
    if period is None:
        os.environ.pop("SALP_ROBOT_ROLLOUT_M", None)
    else:
        os.environ["SALP_ROBOT_ROLLOUT_M"] = str(period)
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=3)
    os.environ.pop("SALP_ROBOT_ROLLOUT_M", None)
    return env


def actor_for(hidden, coast_hi, seed, obs):
    """A `sac.Actor` on the Box [0, 1] x [0, coast_hi] x [-1, 1] whose deterministic actions spread over it: the output
    layer is scaled so that its pre-activations have a standard deviation of 1.2 on the observations `obs`."""
    import torch
    from underwater_swimmer_rl_amd.sac import Actor
    torch.manual_seed(seed)
    actor = Actor(6, 3, hidden, act_low=np.array([0.0, 0.0, -1.0]), act_high=np.array([1.0, coast_hi, 1.0])).to("cuda:0")
    with torch.no_grad():
        actor.mu.bias.zero_()
        actor.mu.weight.mul_(1.2 / actor.mu(actor.body(obs)).std())
    return actor.eval()


def timed(run, calls):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(calls):
        run()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / calls


def measure(forms, rounds, window, before=None):
    """forms: name -> callable.  Returns name -> (median ms, spread, calls per window)."""
    import torch
    calls = {}
    for name, run in forms.items():           # warm-up of every form, and the calls that fill a window
        run()
        torch.cuda.synchronize()
        if before:
            before(name)
        ms = timed(run, 2)
        calls[name] = max(2, min(200, int(round(window * 1e3 / ms))))
    samples = {name: [] for name in forms}
    for _ in range(rounds):
        for name, run in forms.items():       # alternated
            if before:
                before(name)
            samples[name].append(timed(run, calls[name]))
    return {name: (float(np.median(v)), float((max(v) - min(v)) / np.median(v)), calls[name]) for name, v in samples.items()}


def sampled_rows(args):
    """The rows of --sampled (see the top of the file)."""
    import torch
    from underwater_swimmer_rl_amd.policy import GaussianPolicy
    H, rows = args.horizon, []
    for n in (int(x) for x in args.envs.split(",")):
        envs = {k: make_env(n) for k in ("mean", "sampled, sd -> 0", "sampled, ls = -1")}
        for mix, coast_hi in MIXES.items():
            for label, hidden in (("linear", ()), ("64x64", (64, 64))):
                actor = actor_for(hidden, coast_hi, 5, envs["mean"].reset()[0])
                handles, forms = {}, {}
                for k, env in envs.items():
                    with torch.no_grad():
                        actor.log_std.weight.zero_()
                        actor.log_std.bias.fill_(-1.0 if k.endswith("-1") else -25.0)
                    handles[k] = env.make_policy(GaussianPolicy.from_actor(actor))
                    forms[k] = (lambda e, h, s: lambda: e.rollout_policy(h, H, want_actions=False, sample=s))(env, handles[k], k != "mean")
                cycles = {}
                for k, env in envs.items():
                    env.reset()
                    inner = env.rollout_policy(handles[k], H, sample=k != "mean")["inner_steps"].float()
                    cycles[k] = (float(inner.mean()), int(inner.max()))
                row = dict(envs=n, mix=mix, loop=f"closed {label}", horizon=H, cycle_steps=cycles,
                           forms=measure(forms, args.rounds, args.window, before=lambda name: envs[name].reset()))
                f = row["forms"]
                row["sampled_over_mean"] = f["sampled, sd -> 0"][0] / f["mean"][0]
                rows.append(row)
                print(json.dumps(row), flush=True)
                for h in handles.values():
                    h.close()
        for e in envs.values():
            e.close()
    print("\n| envs | mix | policy | mean | sampled, sd -> 0 | ratio | sampled, ls = -1 (mean / max Euler steps per cycle) | largest spread |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f, c = r["forms"], r["cycle_steps"]["sampled, ls = -1"]
        print(f"| {r['envs']} | {r['mix']} | {r['loop']} | {f['mean'][0]:.2f} | {f['sampled, sd -> 0'][0]:.2f} | {r['sampled_over_mean']:.3f} | "
              f"{f['sampled, ls = -1'][0]:.2f} ({c[0]:.0f} / {c[1]}) | {100 * max(v[1] for v in f.values()):.1f} % |")
    print("(ms per call of H = %d env steps; median of %d alternated rounds)" % (H, args.rounds))
    return rows


def per_launch(forms, launches, before):
    """forms: name -> callable; every launch timed on its own (device events), the forms alternated, `before(name)` ahead
    of each.  Returns name -> (median ms, (max - min) / median, interquartile range / median, launches)."""
    import torch
    for name, run in forms.items():
        before(name)
        run()
    torch.cuda.synchronize()
    samples = {name: [] for name in forms}
    for _ in range(launches):
        for name, run in forms.items():
            before(name)
            samples[name].append(timed(run, 1))
    out = {}
    for name, v in samples.items():
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        out[name] = (float(med), float((max(v) - min(v)) / med), float((q3 - q1) / med), launches)
    return out


def evaluate_rows(args):
    """The rows of --evaluate (see the top of the file)."""
    import torch
    from underwater_swimmer_rl_amd import _capi
    from underwater_swimmer_rl_amd.policy import MLPPolicy, summarize_robot_rollout
    H, rows = args.horizon, []

    def env_on(n, lib=None):
        """An env on the library at `lib` (an older build: a library without the evaluation calls loads too)."""
        if lib is None:
            return make_env(n)
        own, _capi._lib = _capi._lib, _capi.load_library(lib)
        try:
            return make_env(n)
        finally:
            _capi._lib = own

    # (a) rollout_policy + reward.sum(0) against (b) evaluate_policy: 64 x 64 policy, same start, every launch timed alone
    for n in (int(x) for x in args.envs.split(",")):
        a_env, b_env = env_on(n, args.parent_lib), env_on(n)
        a_env.reset()          # (the two envs see the same sequence of resets: the same targets, the same work)
        policy = MLPPolicy.from_actor(actor_for((64, 64), 1.0, 5, b_env.reset()[0]))
        a_h, b_h = a_env.make_policy(policy), b_env.make_policy(policy)
        forms = {"rollout_policy + reward.sum(0)": lambda: a_env.rollout_policy(a_h, H, want_actions=False)["reward"].sum(0),
                 "evaluate_policy": lambda: b_env.evaluate_policy(b_h, H)}
        envs_of = dict(zip(forms, (a_env, b_env)))
        a_env.reset(), b_env.reset()
        want = a_env.rollout_policy(a_h, H, want_actions=False)
        got = b_env.evaluate_policy(b_h, H)
        fold = summarize_robot_rollout(*(want[k].cpu().numpy() for k in ("reward", "terminated", "truncated", "inner_steps")))
        same = got["record"].cpu().numpy().tobytes() == fold.tobytes()
        row = dict(envs=n, horizon=H, policy="64x64", per_step_library=args.parent_lib or "this build",
                   euler_steps=int(got["euler_steps"].sum()), same_records=same,
                   forms=per_launch(forms, args.launches, before=lambda name: envs_of[name].reset()))
        f = row["forms"]
        row["evaluate_over_rollout"] = f["evaluate_policy"][0] / f["rollout_policy + reward.sum(0)"][0]
        rows.append(row)
        print(json.dumps(row), flush=True)
        for e in (a_env, b_env):
            e.close()
    if args.episode_launches < 1:
        return rows
    # whole episodes: the population of examples/evaluate_robot_policy.py, 500 cycles, with and without the stop
    P, E, T = 64, 64, args.episode_cycles
    scale, shift = np.array([0.5, 0.05, 1.0], np.float32), np.array([0.5, 0.05, 0.0], np.float32)
    theta = np.random.default_rng(0).standard_normal((P, 3, 7)).astype(np.float32)
    population = MLPPolicy([(theta[..., :6], theta[..., 6])], np.tile(scale, (P, 1)), np.tile(shift, (P, 1)), "clip")
    envs_of = {"evaluate_policy": make_env(P * E), "evaluate_policy, first_episode": make_env(P * E)}      # the same episodes
    forms = {name: (lambda e, h, stop: lambda: e.evaluate_policy(h, T, first_episode=stop))(e, e.make_policy(population), "first" in name)
             for name, e in envs_of.items()}
    steps = {}
    for name, run in forms.items():
        envs_of[name].reset()
        v = run()
        steps[name] = dict(euler_steps=int(v["euler_steps"].sum()), finished=float((v["first_end"] != 0).float().mean()),
                           reached=float((v["first_end"] == 1).float().mean()), mean_first_length=float(v["first_length"].float().mean()))
    row = dict(envs=P * E, horizon=T, policy="64 linear policies x 64 robots", totals=steps,
               forms=per_launch(forms, args.episode_launches, before=lambda name: envs_of[name].reset()))
    f = row["forms"]
    row["stop_over_full"] = f["evaluate_policy, first_episode"][0] / f["evaluate_policy"][0]
    rows.append(row)
    print(json.dumps(row), flush=True)
    for e in envs_of.values():
        e.close()
    return rows


def main():
    import torch
    from underwater_swimmer_rl_amd.policy import MLPPolicy
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluate", action="store_true", help="evaluate_policy against rollout_policy + reward.sum(0), and the first-episode stop")
    ap.add_argument("--parent-lib", default=None, help="--evaluate: the library the per-step form runs on (default: this build)")
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--episode-cycles", type=int, default=500)
    ap.add_argument("--episode-launches", type=int, default=5)
    ap.add_argument("--envs", default="4096,262144")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sampled", action="store_true", help="the sampled rollout against its deterministic twin")
    args = ap.parse_args()
    H = args.horizon
    rows = []
    if args.sampled:
        rows = sampled_rows(args)
    if args.evaluate:
        rows = evaluate_rows(args)          # (no table below: the rows are the report)
    own_rows = args.sampled or args.evaluate
    for n in (() if own_rows else (int(x) for x in args.envs.split(","))):
        base = make_env(n)
        rolls = {m: make_env(n, m) for m in PERIODS}
        for mix, coast_hi in MIXES.items():
            rng = np.random.default_rng(7)
            acts = torch.as_tensor(np.stack([rng.uniform(0, 1, (H, n)), rng.uniform(0, coast_hi, (H, n)), rng.uniform(-1, 1, (H, n))],
                                            axis=2).astype(np.float32), device="cuda:0")

            def step_loop():
                for t in range(H):
                    base.step(acts[t])
            forms = {"step loop": step_loop}
            for m, env in rolls.items():
                forms[f"M={m}"] = (lambda e: lambda: e.rollout(acts))(env)
            inner = rolls[0].rollout(acts)["inner_steps"].float()
            row = dict(envs=n, mix=mix, loop="open", horizon=H, mean_cycle_steps=float(inner.mean()), max_cycle_steps=int(inner.max()),
                       forms=measure(forms, args.rounds, args.window))
            rows.append(row)
            print(json.dumps(row), flush=True)
            for label, hidden in (("linear", ()), ("64x64", (64, 64))):
                actor = actor_for(hidden, coast_hi, 5, base.reset()[0])
                policy = MLPPolicy.from_actor(actor)
                handles = {m: env.make_policy(policy) for m, env in rolls.items()}

                def actor_loop():
                    with torch.no_grad():
                        obs = base.observe()
                        for t in range(H):
                            a, _ = actor(obs, deterministic=True, with_logprob=False)
                            obs = base.step(a)[0]
                forms = {"step loop": actor_loop}
                for m, env in rolls.items():
                    forms[f"M={m}"] = (lambda e, h: lambda: e.rollout_policy(h, H, want_actions=False))(env, handles[m])
                envs_of = {"step loop": base, **{f"M={m}": e for m, e in rolls.items()}}
                rolls[0].reset()
                inner = rolls[0].rollout_policy(handles[0], H)["inner_steps"].float()
                row = dict(envs=n, mix=mix, loop=f"closed {label}", horizon=H, mean_cycle_steps=float(inner.mean()),
                           max_cycle_steps=int(inner.max()),
                           forms=measure(forms, args.rounds, args.window, before=lambda name: envs_of[name].reset()))
                rows.append(row)
                print(json.dumps(row), flush=True)
                for h in handles.values():
                    h.close()
        for e in (base, *rolls.values()):
            e.close()
    if not own_rows:
        print("\n| envs | mix | loop | mean / max Euler steps per cycle | " + " | ".join(["step loop"] + [f"M = {m}" for m in PERIODS]) + " | largest spread |")
        print("|---|---|---|---|" + "---|" * (len(PERIODS) + 2))
    for r in ([] if own_rows else rows):
        f = r["forms"]
        cells = [f"{f[k][0]:.2f}" for k in ["step loop"] + [f"M={m}" for m in PERIODS]]
        print(f"| {r['envs']} | {r['mix']} | {r['loop']} | {r['mean_cycle_steps']:.0f} / {r['max_cycle_steps']} | " + " | ".join(cells) +
              f" | {100 * max(v[1] for v in f.values()):.1f} % |")
    if not own_rows:
        print("(ms per call of H = %d env steps; median of %d alternated rounds)" % (H, args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
