#!/usr/bin/env python3
"""Interleaved A/B timing of several builds of libsalp_hip.so in ONE process (same device, same
data), as cdna_hip_programming.md §5.4 rule 24 asks.  usage:
    python profiles/ab_bench.py name1=path1.so name2=path2.so ... [--rounds 6] [--launches 5]
Prints per-variant median / min kernel ms (HIP events) for the bench workload.
Variant-name suffixes pick the entry point: "+gen" / "+gennoout" device-generated actions; "+packed" / "+packedfinal"
salp_vec_rollout_packed (records of obs_dim + 4 / 2 obs_dim + 4 words); "+step" salp_vec_step with info (and final_obs
with --final-obs), which needs --chunk 1 — with --chunk 1 "+packed" is salp_vec_step_packed's launch.  --calls N times N
consecutive calls as one sample (a 10-us step launch is below what one event pair resolves).
"+policy": salp_vec_rollout_policy with the 24 -> 32 -> 32 -> A actor (sac.Actor, seed 0) evaluated in the kernel; it writes
the actions it takes into the shared action block, so with --launches 1 and the "+policy" variant listed FIRST a plain
variant behind it replays exactly those actions from the same state (the price of the policy block alone).
"+evaluate": salp_vec_evaluate_policy with the same policy as "+policy" (one 32-byte summary record per env, no per-step
output); pair it against "+policy" of the PARENT commit's library: `par+policy=parent.so new+evaluate=libsalp_hip.so`.
"+policypacked" / "+policypackedfinal": salp_vec_rollout_policy_packed with the same policy (records of obs_dim + 4 /
2 obs_dim + 4 words, the actions into the shared block like "+policy"); pair it against "+policy" of the same library, and
for scale "+packed" against a plain variant: the closed-loop ratio should lie near the open-loop one.
--policy linear | mlp32 | mlp64 picks the policy of both: the 25-parameter linear clip rule (the pursuit rule), or the
24 -> 32 -> 32 -> A / 24 -> 64 -> 64 -> A actor.
"+actorgraph": the same actor in torch around salp_vec_step, `SalpVectorEnv.capture_policy_steps(n_steps = chunk)` replayed
— the best closed-loop path without the in-kernel policy (runs the installed library whatever path is given)."""
import ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi

def main():
    variants, rounds, launches, n, H, preset = [], 6, 5, 262144, 250, "single_food_long_horizon"
    want_fin = False
    calls = 1
    overrides = {}
    policy_kind = "mlp32"
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--rounds": rounds = int(next(it))
        elif a == "--launches": launches = int(next(it))
        elif a == "--envs": n = int(next(it))
        elif a == "--chunk": H = int(next(it))
        elif a == "--preset": preset = next(it)
        elif a == "--set":                           # --set width=801 (a SalpSnakeEnv keyword on top of the preset)
            k, v = next(it).split("=", 1); overrides[k] = (int(v) if v.lstrip("-").isdigit() else (v == "true") if v in ("true", "false") else float(v))
        elif a == "--calls": calls = int(next(it))
        elif a == "--policy": policy_kind = next(it)
        elif a == "--final-obs": want_fin = True      # the non-FULL output signature (terminal observations written)
        else:
            k, v = a.split("=", 1); variants.append((k, os.path.abspath(v)))
    # a variant name ending in "+gen" runs the device-generated-action mode (act = NULL, actions
    # written to act_out); "+gennoout" the same without act_out
    cfg = pkg.load_env_config(preset, **overrides)
    dev = torch.device("cuda", 0)
    act = torch.rand((H, n, cfg.act_dim), device=dev) * 2 - 1
    obs = torch.empty((H, n, cfg.obs_dim), device=dev)
    rew = torch.empty((H, n), device=dev)
    term = torch.empty((H, n), dtype=torch.uint8, device=dev)
    trunc = torch.empty((H, n), dtype=torch.uint8, device=dev)
    fin = torch.empty((H, n, cfg.obs_dim), device=dev) if want_fin else None
    info = torch.empty((H, n, _capi.INFO_COLS), dtype=torch.int32, device=dev)
    rec = torch.empty((H, n, 2 * cfg.obs_dim + _capi.REC_EXTRA_COLS), device=dev)      # either record width
    handles = {}
    for name, path in variants:
        lib = _capi.load_library(path)
        c = cfg.to_c(); h = ctypes.c_void_p()
        _capi.check(lib, lib.salp_vec_create(ctypes.byref(c), n, 0, 0, 0, ctypes.byref(h)), "create")
        handles[name] = (lib, h, c)
    policies, graphs, envs = {}, {}, []
    eval_rec = torch.zeros((n, _capi.EVAL_WORDS), dtype=torch.int32, device=dev)
    if any("+policy" in name or "+actorgraph" in name or "+evaluate" in name for name, _ in variants):
        from underwater_swimmer_rl_amd.policy import MLPPolicy, pursuit_policy
        from underwater_swimmer_rl_amd.sac import Actor
        torch.manual_seed(0)
        low, high = (None, None) if cfg.forced_breathing else ([0.0, -1.0], [1.0, 1.0])
        width = {"mlp32": 32, "mlp64": 64, "linear": 32}[policy_kind]
        actor = Actor(cfg.obs_dim, cfg.act_dim, hidden=(width, width), act_low=low, act_high=high).to(dev)
        mlp = pursuit_policy(3.0, cfg.obs_dim) if policy_kind == "linear" else MLPPolicy.from_actor(actor)
        w = mlp.pack()
        for name, _ in variants:
            if "+policy" in name or "+evaluate" in name:
                lib, h, _ = handles[name]
                d, ph = mlp.desc(), ctypes.c_void_p()
                _capi.check(lib, lib.salp_policy_create(h, ctypes.byref(d), w.ctypes.data_as(ctypes.c_void_p), 0, None, ctypes.byref(ph)), "policy_create")
                policies[name] = ph
            if "+actorgraph" in name:
                env = pkg.SalpVectorEnv(cfg, num_envs=n, seed=0)
                env.reset()
                with torch.no_grad():
                    graphs[name] = env.capture_policy_steps(lambda o: actor(o, deterministic=True, with_logprob=False)[0], n_steps=H,
                                                            want_final_observation=False)
                envs.append(env)
    def launch(name):
        lib, h, _ = handles[name]
        vp = ctypes.c_void_p
        st = vp(torch.cuda.current_stream().cuda_stream)
        if "+actorgraph" in name:
            graphs[name].replay()
            return
        if "+evaluate" in name:
            _capi.check(lib, lib.salp_vec_evaluate_policy(h, policies[name], H, vp(eval_rec.data_ptr()), _capi.SALP_DEVICE_PTRS, st), "evaluate_policy")
            return
        if "+policypacked" in name:
            flags = _capi.SALP_DEVICE_PTRS | (_capi.REC_FINAL_OBS if name.endswith("+policypackedfinal") else 0)
            _capi.check(lib, lib.salp_vec_rollout_policy_packed(h, policies[name], H, vp(rec.data_ptr()), vp(act.data_ptr()), flags, st), "rollout_policy_packed")
            return
        if "+policy" in name:
            _capi.check(lib, lib.salp_vec_rollout_policy(h, policies[name], H, vp(obs.data_ptr()), vp(rew.data_ptr()), vp(term.data_ptr()),
                        vp(trunc.data_ptr()), vp(act.data_ptr()), _capi.SALP_DEVICE_PTRS, st), "rollout_policy")
            return
        if "+packed" in name:
            flags = _capi.SALP_DEVICE_PTRS | (_capi.REC_FINAL_OBS if name.endswith("+packedfinal") else 0)
            _capi.check(lib, lib.salp_vec_rollout_packed(h, vp(act.data_ptr()), H, vp(rec.data_ptr()), None, flags, st), "rollout_packed")
            return
        if name.endswith("+step"):
            assert H == 1, "+step needs --chunk 1"
            _capi.check(lib, lib.salp_vec_step(h, vp(act.data_ptr()), vp(obs.data_ptr()), vp(rew.data_ptr()), vp(term.data_ptr()),
                        vp(trunc.data_ptr()), vp(fin.data_ptr()) if fin is not None else None, vp(info.data_ptr()), 1, st), "step")
            return
        a_in = None if "+gen" in name else vp(act.data_ptr())
        a_out = vp(act.data_ptr()) if name.endswith("+gen") else None
        _capi.check(lib, lib.salp_vec_rollout(h, a_in, H, vp(obs.data_ptr()), vp(rew.data_ptr()),
                    vp(term.data_ptr()), vp(trunc.data_ptr()), vp(fin.data_ptr()) if fin is not None else None, a_out, 1, vp(torch.cuda.current_stream().cuda_stream)), "rollout")
    times = {name: [] for name, _ in variants}
    warm = int(os.environ.get("AB_WARM", "8"))   # advance every variant to the same (desynchronised) phase mix
    for name, _ in variants:
        for _ in range(warm): launch(name)
    torch.cuda.synchronize()
    for r in range(rounds):
        for name, _ in variants:
            for _ in range(launches):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(calls): launch(name)
                e.record(); e.synchronize()
                times[name].append(s.elapsed_time(e))
    # every variant simulates the same trajectory (same seed, warm-up and launch count), so launch i of one variant and
    # launch i of another do the same work: the MEAN over all launches, and the mean of the per-launch ratios to the
    # first variant, compare like with like even though launches differ from each other (event rates drift)
    base = times[variants[0][0]]
    out = {name: {"median_ms": statistics.median(t), "mean_ms": statistics.fmean(t), "min_ms": min(t), "max_ms": max(t), "n": len(t),
                  "paired_ratio_to_first": statistics.fmean(a / b for a, b in zip(t, base))} for name, t in times.items()}
    if os.environ.get("AB_DUMP") == "1":   # every launch time in order (e.g. with AB_WARM=0: the phase mix desynchronising)
        for name, t in times.items():
            out[name]["all_ms"] = [round(x, 4) for x in t]
    print(json.dumps(out, indent=1))

if __name__ == "__main__":
    main()
