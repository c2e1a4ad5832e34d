"""Sampled actions inside the robot's multi-cycle rollout kernel (salp_robot_vec_rollout_policy_sampled,
include/salp_robot_sampled.h): every action and log-probability against `GaussianPolicy.reference` within
`GaussianPolicy.error_bound`, the noise step, the simulator against a twin that replays the actions, the mean path,
continuation, populations, the pointer forms, hipGraph capture, refusals and `sac.collect_in_kernel` on a robot env.

The shapes are those of tests/test_gpu_robot_rollout.py: 357 envs (two workgroups, the last wavefront ragged) and 7 env
steps, 256 envs for populations, max_cycles = 2 where episodes must end.  The comparisons with a twin env use that file's
`assert_same_run` and its tolerances (flags, Euler-step counts and the final-observation mask identical; float32 outputs
within 2^-22 and the fp64 state within 1e-11, relative to max(1, |x|)) and print whether the results were bit-identical.
The policies are the cases of tests/robot_sampled_cases.py, whose CPU guard is tests/test_robot_sampled_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import robot_sampled_cases as cases
import test_gpu_robot_rollout as rr
from underwater_swimmer_rl_amd._capi import SalpLib
from underwater_swimmer_rl_amd.policy import GaussianPolicy
from underwater_swimmer_rl_amd.robot_env import R_RNG, SalpRobotVectorEnv

pytestmark = pytest.mark.gpu

N, H, SEED = cases.N, cases.H, cases.SEED
INVALID = -1
SENTINEL = 0xA5C3F00D
OUT_KEYS = ("obs", "reward", "terminated", "truncated", "inner_steps", "_final_observation", "actions", "logp")
host, kept = rr.host, rr.kept
assert (rr.N, rr.H, rr.SEED) == (N, H, SEED)


def make_env(n=N, output="numpy", **kw):
    return SalpRobotVectorEnv(n, device="cuda:0", seed=SEED, output=output, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b, keys=OUT_KEYS):
    return [k for k in keys if not np.array_equal(bits(a[k]), bits(b[k]))]


def assert_is_the_definition(policy, seen, out, n0, label="", env_base=0):
    """Every action and log-probability within `error_bound(seen, z)` of `reference(seen, z)`, z the noise of (env, n0 + t);
    no NaN.  Prints and returns the worst ratios."""
    Hh, n = out["actions"].shape[:2]
    z = cases.case_noise(policy, n, n0, Hh, SEED, env_base)
    (wa, wl), (ea, el) = policy.reference(seen, z), policy.error_bound(seen, z)
    assert not np.isnan(out["actions"]).any() and not np.isnan(out["logp"]).any(), label
    ra = np.abs(out["actions"].astype(np.float64) - wa) / ea
    rl = np.abs(out["logp"].astype(np.float64) - wl) / el
    print(f"{label}: worst ratio to the bound: action {ra.max():.3f}, logp {rl.max():.3f} "
          f"(bounds up to {ea.max():.3g}, {el.max():.3g})")
    assert ra.max() <= 1.0, (label, float(ra.max()))
    assert rl.max() <= 1.0, (label, float(rl.max()))
    return float(ra.max()), float(rl.max())


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One sampled rollout of a case from a fresh env and noise step 0: computed once, shared, read-only."""
    policy = cases.case_policy(name)
    env = make_env()
    entry = host(env.observe())
    handle = env.make_policy(policy)
    out = kept(env.rollout_policy(handle, H, sample=True))
    state, step = env.get_state(), handle.noise_step
    env.close()
    seen = cases.rows_seen(entry, out["obs"])
    for a in (entry, seen, state, *[v for v in out.values() if v is not None]):
        a.setflags(write=False)
    return dict(policy=policy, entry=entry, seen=seen, out=out, state=state, noise_step=step)


# ---------------------------------------------------------------- 5. definition
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_sampled_action_and_logp_is_the_definition(name):
    r = device_run(name)
    out = r["out"]
    assert set(out) == {"obs", "reward", "terminated", "truncated", "final_observation", "_final_observation", "inner_steps",
                        "actions", "logp"}
    assert out["actions"].shape == (H, N, 3) and out["logp"].shape == (H, N) and out["logp"].dtype == np.float32
    assert r["noise_step"] == H
    assert_is_the_definition(r["policy"], r["seen"], out, 0, label=name)
    lo, hi = cases.SHIFT - cases.SCALE, cases.SHIFT + cases.SCALE
    assert np.all(out["actions"] >= lo) and np.all(out["actions"] <= hi)
    assert np.ptp(out["inner_steps"][:, :64]) > 50, "cycle lengths must differ inside a wavefront"


# ---------------------------------------------------------------- 6. noise step applied
@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_noise_step_was_applied(name):
    r = device_run(name)
    clamped = list(cases.floor_clamped_components(r["policy"]))
    assert clamped == ([1] if name == cases.CLAMPED else []), "only the intended case has floor-clamped components"
    share = cases.off_by_one_share(r["policy"], r["seen"], r["out"]["actions"])
    print(f"{name}: share of entries more than {cases.OFF_BY_ONE_BOUNDS:g} bounds from the noise of n + 1: {share:.3f}")
    assert share > cases.OFF_BY_ONE_SHARE


# ---------------------------------------------------------------- 7. simulator untouched
@pytest.mark.parametrize("name", list(cases.CASES))
def test_simulator_untouched(name):
    r = device_run(name)
    twin = make_env()
    replay = kept(twin.rollout(r["out"]["actions"]))
    state = twin.get_state()
    rr.assert_same_run(r["out"], replay, r["state"], state, f"sampled {name} against rollout(actions taken)")
    assert np.array_equal(r["state"][R_RNG], state[R_RNG]), "the env's own draw counter was consumed"
    twin.close()


def test_endings_in_mixed_wavefronts_and_the_action_after_an_autoreset():
    """max_cycles = 2, one step, then every third env reset: the two cohorts are truncated on alternating steps, so every
    wavefront mixes finished and unfinished lanes on every step.  The action after an autoreset is the definition on the
    new episode's first row (obs[t] of the ending step), at that env's own step index."""
    policy = cases.case_policy("mlp32x16")
    rng = np.random.default_rng(1)
    first = rr.schedule_mix(rng, 5, N)[0]
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    env, twin = make_env(max_cycles=2), make_env(max_cycles=2)
    for e in (env, twin):
        e.step(first)
        e.reset(mask=mask)
    entry = host(env.observe())
    out = kept(env.rollout_policy(policy, H, sample=True))
    done = out["_final_observation"]
    print("finishers per step:", done.sum(axis=1).tolist())
    assert np.array_equal(done, out["truncated"] | out["terminated"]) and out["truncated"].sum() > N
    for t in range(H):
        for w in range(0, N, 64):
            assert 0 < done[t, w:w + 64].sum() < min(64, N - w), (t, w)
    seen = cases.rows_seen(entry, out["obs"])
    assert_is_the_definition(policy, seen, out, 0, label="max_cycles = 2")
    after = done[:-1]          # actions of step t + 1 that follow an ending on step t
    z = cases.case_noise(policy)
    (wa, _), (ea, _) = policy.reference(seen, z), policy.error_bound(seen, z)
    assert after.sum() > N and np.all(np.abs(out["actions"][1:][after] - wa[1:][after]) <= ea[1:][after])
    replay = kept(twin.rollout(out["actions"]))
    state, state_twin = env.get_state(), twin.get_state()
    rr.assert_same_run(out, replay, state, state_twin, "sampled, max_cycles = 2")
    assert np.array_equal(state[R_RNG], state_twin[R_RNG]) and state[R_RNG].min() >= 2, "autoresets draw from the env's own counter alone"
    for e in (env, twin):
        e.close()


# ---------------------------------------------------------------- 8. mean path
def test_the_deterministic_call_runs_the_mean_and_leaves_the_noise_step():
    policy = cases.case_policy("mlp32x16")
    a, b = make_env(max_cycles=3), make_env(max_cycles=3)
    handle = a.make_policy(policy)
    assert handle.gaussian and handle.words == policy.words == policy.mean_policy().words + 3 * 16 + 3
    handle.set_noise_step(5)
    got = kept(a.rollout_policy(handle, H))
    want = kept(b.rollout_policy(policy.mean_policy(), H))
    assert "logp" not in got and handle.noise_step == 5
    keys = tuple(k for k in OUT_KEYS if k != "logp")
    assert same_bits(got, want, keys) == []
    done = want["_final_observation"]
    assert done.any() and np.array_equal(bits(got["final_observation"][done]), bits(want["final_observation"][done]))
    assert np.array_equal(a.get_state(), b.get_state())
    for e in (a, b):
        e.close()


# ---------------------------------------------------------------- 9. continuation
def test_a_second_call_continues_the_noise():
    policy = cases.case_policy("mlp16")
    env = make_env()
    handle = env.make_policy(policy)
    entry = host(env.observe())
    first = kept(env.rollout_policy(handle, 3, sample=True))
    assert handle.noise_step == 3
    second = kept(env.rollout_policy(handle, 4, sample=True))
    assert handle.noise_step == 7
    assert_is_the_definition(policy, cases.rows_seen(entry, first["obs"]), first, 0, label="steps 0..2 at n0 = 0")
    assert_is_the_definition(policy, cases.rows_seen(first["obs"][-1], second["obs"]), second, 3, label="steps 3..6 at n0 = 3")
    # ... and not at n0 = 0 again (off_by_one_share looks at n0 + 1: 2^32 - 1 + 1 is step 0 in the low 32 bits)
    seen2 = cases.rows_seen(first["obs"][-1], second["obs"])
    assert cases.off_by_one_share(policy, seen2, second["actions"], n0=2 ** 32 - 1) > cases.OFF_BY_ONE_SHARE
    env.close()
    fresh = make_env()
    again = fresh.make_policy(policy)
    again.set_noise_step(1234567)
    again.set_noise_step(0)
    rerun = kept(fresh.rollout_policy(again, 3, sample=True))
    assert same_bits(rerun, first) == [] and again.noise_step == 3
    # the 64-bit word is kept whole; the draw takes its low 32 bits
    again.set_noise_step(2 ** 40 + 3)
    assert again.noise_step == 2 ** 40 + 3
    cont = kept(fresh.rollout_policy(again, 4, sample=True))
    assert again.noise_step == 2 ** 40 + 7
    assert same_bits(cont, second) == []
    fresh.close()


# ---------------------------------------------------------------- 10. population
def test_population_halves_equal_the_single_policies():
    n = 256
    c = cases.CASES["mlp16"]
    ps = [cases.robot_gaussian_policy((16,), 41, c["gain"], c["out_gain"], (-1.0, -2.0, -3.0)),
          cases.robot_gaussian_policy((16,), 42, c["gain"], 4.0, (-0.5, -1.0, -1.5))]
    both = make_env(n)
    out = kept(both.rollout_policy(GaussianPolicy.stack(ps), H, sample=True))
    state = both.get_state()
    refs = []
    for k, p in enumerate(ps):
        alone = make_env(n)
        ref = kept(alone.rollout_policy(p, H, sample=True))
        half = slice(128 * k, 128 * (k + 1))
        for key in OUT_KEYS:
            assert np.array_equal(bits(out[key][:, half]), bits(ref[key][:, half])), (k, key)
        assert np.array_equal(state[:, half], alone.get_state()[:, half]), k
        refs.append(ref)
        alone.close()
    assert np.abs(refs[0]["actions"] - refs[1]["actions"]).mean() > 0.05
    assert np.abs(refs[0]["logp"] - refs[1]["logp"]).mean() > 0.5
    three = GaussianPolicy.stack(ps + [ps[0]])
    with pytest.raises(ValueError):
        both.make_policy(three)
    assert both.L.salp_robot_policy_words_gaussian(both._h, ctypes.byref(three.desc())) == INVALID
    both.close()


# ---------------------------------------------------------------- 11. pointer forms, guard words, nullable outputs
@pytest.mark.parametrize("with_actions,with_logp", [(True, True), (False, True), (True, False)], ids=["all", "act_out NULL", "logp_out NULL"])
def test_pointer_forms_guard_words_and_null_outputs(with_actions, with_logp):
    import torch
    policy = cases.case_policy("mlp32x16")
    ref = make_env(max_cycles=2)
    ref._rollout_outputs(H)[4][...] = np.uint32(SENTINEL).view(np.float32)      # final_obs goes in as well as out
    want = kept(ref.rollout_policy(policy, H, sample=True))
    want["final_obs"] = want["final_observation"]
    want_state = ref.get_state()
    ref.close()

    env = make_env(output="torch", max_cycles=2)
    handle = env.make_policy(policy)
    G = 64

    def block(shape, dtype):
        rows = int(np.prod(shape))
        b = torch.empty(rows + G, dtype=dtype, device="cuda:0")
        if dtype == torch.uint8:
            b.fill_(0xA5)
        else:
            b.view(torch.int32).fill_(int(np.uint32(SENTINEL).view(np.int32)))
        return b, rows
    bl = dict(obs=block((H, N, 6), torch.float32), reward=block((H, N), torch.float32), terminated=block((H, N), torch.uint8),
              truncated=block((H, N), torch.uint8), final_obs=block((H, N, 6), torch.float32),
              inner_steps=block((H, N), torch.int32), actions=block((H, N, 3), torch.float32), logp=block((H, N), torch.float32))
    torch.cuda.synchronize()
    p = SalpLib._ptr
    rc = env.L.salp_robot_vec_rollout_policy_sampled(
        env._h, handle._p, H, *[p(bl[k][0]) for k in ("obs", "reward", "terminated", "truncated", "final_obs", "inner_steps")],
        p(bl["actions"][0]) if with_actions else None, p(bl["logp"][0]) if with_logp else None, 1, env._stream)
    assert rc == 0, env.L.salp_robot_last_error()
    torch.cuda.synchronize()
    assert handle.noise_step == H
    for k, (b, rows) in bl.items():
        got = b.cpu().numpy()
        guard = got[rows:]
        assert (guard == 0xA5).all() if got.dtype == np.uint8 else (guard.view(np.uint32) == SENTINEL).all(), f"{k}: guard words written"
        if (k == "actions" and not with_actions) or (k == "logp" and not with_logp):
            assert (got.view(np.uint32) == SENTINEL).all(), f"{k} == NULL, yet the block was written"
            continue
        w = want[k].reshape(-1)
        w = w.astype(np.uint8) if w.dtype == bool else w
        assert np.array_equal(bits(got[:rows]), bits(w)), f"{k} differs from the host-pointer run"
    assert np.array_equal(env.get_state(), want_state)
    done = want["_final_observation"]
    assert done.any() and not done.all()
    env.close()


# ---------------------------------------------------------------- 12. hipGraph
def test_graph_capture_draws_fresh_noise_and_takes_new_weights():
    import torch
    c = cases.CASES["mlp32x16"]
    p1 = cases.case_policy("mlp32x16")
    p2 = cases.robot_gaussian_policy(c["hidden"], 52, c["gain"], c["out_gain"], (-0.5, -1.0, -2.0))
    w1, w2 = (torch.from_numpy(q.pack()).to("cuda:0") for q in (p1, p2))
    env = make_env(output="torch")
    handle = env.make_policy(p1, weights=w1)
    env.rollout_policy(handle, H, sample=True)           # warm-up: buffers, lazy kernel load
    handle.set_noise_step(0)
    torch.cuda.synchronize()
    assert handle.noise_step == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.rollout_policy(handle, H, sample=True)
    torch.cuda.synchronize()
    assert handle.noise_step == 0, "capture must not execute"
    runs = []
    for rep, pol in enumerate((p1, p2)):
        if rep == 1:
            handle.update(w2)                              # stream-ordered, nothing allocated, no re-capture
        entry = host(env.observe())
        g.replay()
        torch.cuda.synchronize()
        got = {k: host(out[k]) for k in ("obs", "actions", "logp")}
        assert handle.noise_step == (rep + 1) * H          # advanced on the device, by the replay itself
        seen = cases.rows_seen(entry, got["obs"])
        assert_is_the_definition(pol, seen, got, rep * H, label=f"replay {rep}")
        runs.append((seen, got))
    seen, got = runs[1]      # the second replay ran the new weights, not the old ones
    z = cases.case_noise(p1, N, H, H)
    assert (np.abs(got["actions"] - p1.reference(seen, z)[0]) > 100 * p1.error_bound(seen, z)[0]).mean() > 0.5
    assert not np.array_equal(runs[0][1]["actions"], got["actions"])
    assert handle.noise_step == 2 * H
    env.close()


# ---------------------------------------------------------------- 13. refusals
def test_refusals_launch_nothing():
    env, other = make_env(), make_env(64)
    L = env.L
    policy = cases.case_policy("mlp16")
    handle, foreign, plain = env.make_policy(policy), other.make_policy(policy), env.make_policy(policy.mean_policy())
    handle.set_noise_step(41)
    obs, rew, logp = np.empty((H, N, 6), np.float32), np.empty((H, N), np.float32), np.full((H, N), 7.0, np.float32)
    p = SalpLib._ptr
    before = env.get_state()
    call = lambda h, pol, hz, flags, o=obs: L.salp_robot_vec_rollout_policy_sampled(h, pol, hz, p(o), p(rew), None, None, None, None,
                                                                                     None, p(logp), flags, None)
    refused = {
        "NULL handle": lambda: call(None, handle._p, H, 0), "NULL policy": lambda: call(env._h, None, H, 0),
        "horizon 0": lambda: call(env._h, handle._p, 0, 0), "negative horizon": lambda: call(env._h, handle._p, -3, 0),
        "horizon above the cap": lambda: call(env._h, handle._p, 1025, 0),
        "unknown flag bits": lambda: call(env._h, handle._p, H, 4),
        "unknown flag bits next to the known one": lambda: call(env._h, handle._p, H, 3),
        "no main output": lambda: L.salp_robot_vec_rollout_policy_sampled(env._h, handle._p, H, None, None, None, None, p(obs), None,
                                                                          None, p(logp), 0, None),
        "a policy of another handle": lambda: call(env._h, foreign._p, H, 0),
        "a policy that is not Gaussian": lambda: call(env._h, plain._p, H, 0),
    }
    for what, f in refused.items():
        assert f() == INVALID, (what, L.salp_robot_last_error())
        assert handle.noise_step == 41, what
        assert np.array_equal(env.get_state(), before), what
    assert np.all(logp == 7.0)
    # the noise step of a policy that has none; NULL arguments
    n = ctypes.c_uint64(99)
    assert L.salp_robot_policy_noise_step(plain._p, ctypes.byref(n)) == INVALID and n.value == 99
    assert L.salp_robot_policy_set_noise_step(plain._p, 3, None) == INVALID
    assert L.salp_robot_policy_noise_step(None, ctypes.byref(n)) == INVALID and L.salp_robot_policy_noise_step(handle._p, None) == INVALID
    assert L.salp_robot_policy_set_noise_step(None, 3, None) == INVALID
    with pytest.raises(ValueError):
        env.rollout_policy(plain, H, sample=True)
    with pytest.raises(ValueError):
        env.rollout_policy(policy.mean_policy(), H, sample=True)
    # descriptors: a Gaussian policy squashes with tanh; the other ranges are those of salp_robot_policy_create
    out = ctypes.c_void_p()
    w = np.zeros(8192, np.float32)
    assert L.salp_robot_policy_words_gaussian(env._h, ctypes.byref(policy.desc())) == policy.words
    bad = []
    for change in (dict(out_activation=1), dict(n_policies=2), dict(n_policies=0), dict(n_hidden=3), dict(struct_size=8)):
        d = policy.desc()
        for k, v in change.items():
            setattr(d, k, v)
        bad.append(d)
    d = policy.desc()
    d.hidden[0] = 24
    bad.append(d)
    for d in bad:
        assert L.salp_robot_policy_words_gaussian(env._h, ctypes.byref(d)) == INVALID
        assert L.salp_robot_policy_create_gaussian(env._h, ctypes.byref(d), p(w), 0, None, ctypes.byref(out)) == INVALID and not out.value
    assert L.salp_robot_policy_words_gaussian(None, ctypes.byref(policy.desc())) == INVALID
    assert L.salp_robot_policy_create_gaussian(env._h, ctypes.byref(policy.desc()), None, 0, None, ctypes.byref(out)) == INVALID
    assert L.salp_robot_policy_create_gaussian(env._h, ctypes.byref(policy.desc()), p(w), 2, None, ctypes.byref(out)) == INVALID
    with pytest.raises(ValueError):
        env.make_policy(cases.sc.gaussian_policy(24, 3, (16,), 5, 1.0, 1.0, (-1.0, -1.0, -1.0)))
    assert np.array_equal(env.get_state(), before) and handle.noise_step == 41
    # the handle still works
    good = kept(env.rollout_policy(handle, 2, sample=True))
    assert not np.isnan(good["logp"]).any() and handle.noise_step == 43
    env.close()
    other.close()


# ---------------------------------------------------------------- 14. the learner hook
def test_collect_in_kernel_on_a_robot_env():
    import torch
    from underwater_swimmer_rl_amd import sac
    n, HC = 256, 4
    torch.manual_seed(0)
    low, high = np.array([0.0, 0.0, -1.0], np.float32), np.array([1.0, 0.3, 1.0], np.float32)      # coast up to 3 s
    agent = sac.SAC(6, 3, sac.SACConfig(hidden_sizes=(32, 32)), device="cuda:0", act_low=low, act_high=high)
    with torch.no_grad():
        agent.actor.log_std.bias.fill_(-1.0)
    pol = GaussianPolicy.from_actor(agent.actor)

    def fresh():
        env = make_env(n, output="torch", max_cycles=2)
        env.step(torch.full((n, 3), 0.5, device="cuda:0"))
        env.reset(mask=torch.as_tensor((np.arange(n) % 3 == 0).astype(np.uint8), device="cuda:0"))
        return env
    twin = fresh()
    first = twin.observe().clone()
    handle_t = twin.make_policy(pol)
    out = twin.rollout_policy(handle_t, HC, sample=True)
    seen = torch.cat([first[None], out["obs"][:-1]])
    assert_is_the_definition(pol, seen.cpu().numpy(), dict(actions=host(out["actions"]), logp=host(out["logp"])), 0, label="collect twin")
    done = out["_final_observation"]
    assert 0 < int(done.sum()) < HC * n and int(out["truncated"].sum()) > n
    # collect_in_kernel: all H x N transitions, truncated ones with their terminal row
    env = fresh()
    buf = sac.DeviceReplayBuffer(2 * HC * n, 6, 3, torch.device("cuda:0"))
    handle = sac.collect_in_kernel(env, agent, buf, HC)
    assert buf.size == HC * n and handle.gaussian and handle.noise_step == HC
    flat = lambda t: t.reshape((HC * n,) + tuple(t.shape[2:]))
    k = buf.size
    assert torch.equal(buf.obs[:k], flat(seen)) and torch.equal(buf.act[:k], flat(out["actions"]))
    assert torch.equal(buf.rew[:k], flat(out["reward"])) and torch.equal(buf.term[:k], flat(out["terminated"]).float())
    nxt, d = buf.next_obs[:k], flat(done)
    assert torch.equal(nxt[d], flat(out["final_observation"])[d]), "next_obs of an ended episode is its terminal row"
    assert torch.equal(nxt[~d], flat(out["obs"])[~d]), "next_obs elsewhere is obs[t]"
    assert not torch.equal(nxt[d], flat(out["obs"])[d]) and not torch.isnan(nxt).any()
    again = sac.collect_in_kernel(env, agent, buf, 2, handle=handle)
    assert again is handle and handle.noise_step == HC + 2 and buf.size == (HC + 2) * n
    env.close()
    twin.close()
