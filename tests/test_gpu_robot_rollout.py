"""Multi-cycle rollouts of the HEAD simulator in one launch (salp_robot_vec_rollout, salp_robot_vec_rollout_policy,
include/salp_robot_rollout.h): against the loop of `step` calls, against the policy's restated arithmetic
(`policy_matrix.py_forward`), and against the C oracle.

Unless a test says otherwise: 357 envs (two workgroups, the last wavefront ragged) and 7 env steps.

Tolerances of the comparisons with the step loop (`assert_same_run`): flags, Euler-step counts and the final-observation
mask identical; the fp64 state within 1e-11 and the float32 outputs within 2^-22, both relative to max(1, |x|).
include/salp_robot.h (trajectory comparison) states that the lanes of a wavefront couple only through the wave-uniform exact sin / cos and sqrt
fallbacks, by < 1e-12 relative per cycle — and which lanes step together is what differs between a rollout and the step
loop; times at most 8 cycles and rounded up that is 1e-11, and a float32 cast of such a value moves by at most one unit in
the last place.  Each comparison also reports (prints) whether the outputs were in fact bit-identical.

Episode endings at small horizons are compared device against device here (max_cycles = 2 or 3); the oracle comparison
uses the default configuration (truncation after 500 cycles)."""
import ctypes
import time

import numpy as np
import pytest

import policy_cases
import robot_oracle_lib as rol
from policy_matrix import py_forward
from support import rel
from underwater_swimmer_rl_amd._capi import SalpLib
from underwater_swimmer_rl_amd.policy import MLPPolicy
from underwater_swimmer_rl_amd.robot_env import SalpRobotVectorEnv

pytestmark = pytest.mark.gpu

N, H, SEED = 357, 7, 11
INVALID = -1
F32_TOL, F64_TOL = 2.0 ** -22, 1e-11
SCALE, SHIFT = np.array([0.5, 0.075, 1.0], np.float32), np.array([0.5, 0.075, 0.0], np.float32)
SENTINEL = np.uint32(0xA5C3F00D).view(np.float32)
FLOAT_KEYS = ("obs", "reward")
EXACT_KEYS = ("terminated", "truncated", "inner_steps", "_final_observation")


def make_env(n=N, output="numpy", **kw):
    return SalpRobotVectorEnv(n, device="cuda:0", seed=SEED, output=output, **kw)


def host(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.array(x, copy=True)


def kept(out):
    """A rollout's dict as host copies (the blocks are the env's own buffers)."""
    return {k: (None if v is None else host(v)) for k, v in out.items()}


def run_steps(env, actions):
    """The loop of `step` calls, stacked like a rollout's dict."""
    rows = {k: [] for k in ("obs", "reward", "terminated", "truncated", "final_observation", "_final_observation", "inner_steps")}
    for a in actions:
        obs, rew, term, trunc, info = env.step(a)
        for k, v in (("obs", obs), ("reward", rew), ("terminated", term), ("truncated", trunc),
                     ("final_observation", info["final_observation"]), ("_final_observation", info["_final_observation"]),
                     ("inner_steps", info["inner_steps"])):
            rows[k].append(host(v))
    return {k: np.stack(v) for k, v in rows.items()}


def close_enough(a, b, tol):
    """NaNs in the same places, everything else within `tol` relative to max(1, |x|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= tol * np.maximum(1.0, np.abs(b[ok]))))


def assert_same_run(got, want, state_got, state_want, what):
    """`got` against `want` (two dicts of a rollout) and the two final states, with the tolerances at the top of the file.
    Returns (and prints) whether everything was bit-identical."""
    for k in EXACT_KEYS:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    done = want["_final_observation"]
    pairs = [(k, got[k], want[k]) for k in FLOAT_KEYS] + [("final_observation", got["final_observation"][done], want["final_observation"][done])]
    for k, a, b in pairs:
        assert close_enough(a, b, F32_TOL), f"{what}: {k} differs by {rel(a, b)}"
    assert close_enough(state_got, state_want, F64_TOL), f"{what}: state differs by {rel(state_got, state_want)}"
    identical = all(np.array_equal(a, b, equal_nan=True) for _, a, b in pairs) and np.array_equal(state_got, state_want, equal_nan=True)
    print(f"{what}: bit-identical = {identical}; obs rel {rel(got['obs'], want['obs']):.3g}, state rel {rel(state_got, state_want):.3g}")
    return identical


def schedule_mix(rng, steps, n):
    """The actions of test_cycle_length_schedule_does_not_change_results: components in [-0.2, 1.2], coast up to 0.3, a few
    NaN rows."""
    a = np.stack([rng.uniform(-0.2, 1.2, (steps, n)), rng.uniform(0, 0.3, (steps, n)), rng.uniform(-1, 1, (steps, n))], axis=2).astype(np.float32)
    a[2, :7, 0] = np.nan
    a[4, 100:103] = np.nan
    return a


def robot_policy(hidden, out="clip", seed=31, gain=1.5, out_gain=2.0):
    p = policy_cases.random_policy(6, 3, hidden, out, seed, gain, out_gain)
    return MLPPolicy(p.layers, SCALE[None], SHIFT[None], out)


def rows_seen(entry, obs):
    """The row each action saw: the entry observation, then obs[t - 1]."""
    return np.concatenate([entry[None], obs[:-1]])


# ---------------------------------------------------------------- 1. open loop equals the step loop
def staggered_pair():
    """Two envs of one seed with max_cycles = 3, one step, then the envs with i % 3 == 0 reset: endings fall on different
    steps in different lanes."""
    rng = np.random.default_rng(1)
    envs = [make_env(max_cycles=3) for _ in range(2)]
    first = schedule_mix(rng, 5, N)[0]
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    for e in envs:
        e.step(first)
        e.reset(mask=mask)
    return envs, schedule_mix(rng, H, N)


def test_open_loop_equals_the_step_loop():
    """`rollout(actions)` against seven `step` calls from the staggered start.  With max_cycles = 3, one step and the reset
    of every third env, the two cohorts are truncated on steps 1, 4 and on steps 2, 5 of the rollout (238 and 119 envs);
    no episode can end on steps 0, 3 and 6, so what is asserted is that endings fall on at least two different steps and
    that finished and unfinished lanes mix on each of them.  Measured on an MI355X: bit-identical."""
    (a, b), actions = staggered_pair()
    got = kept(a.rollout(actions))
    want = run_steps(b, actions)
    finished = want["_final_observation"]
    print("finishers per step:", finished.sum(axis=1).tolist())
    # episodes end by truncation on their third cycle: the two cohorts end on different steps, never all lanes at once
    ending_steps = np.flatnonzero(finished.any(axis=1))
    assert len(ending_steps) >= 2, "endings must fall on at least two different steps"
    assert all(0 < finished[t].sum() < N for t in ending_steps), "finished and unfinished lanes must mix"
    assert_same_run(got, want, a.get_state(), b.get_state(), "open loop")
    for e in (a, b):
        e.close()


# ---------------------------------------------------------------- 2. lane independence edges
def edge_actions():
    rng = np.random.default_rng(2)
    a = np.stack([rng.uniform(0, 1, (H, N)), rng.uniform(0, 0.3, (H, N)), rng.uniform(-1, 1, (H, N))], axis=2).astype(np.float32)
    a[:, 0:64] = (0.0, 0.0, 0.5)                # wavefront 0: zero-length cycles on every step ...
    a[:, 8:16, 0] = np.nan                      # ... and lanes that run no Euler step for other reasons
    a[:, 16:24, 0] = -np.inf
    a[:, 24:32, 1] = -np.inf
    a[:, 64:128] = (0.0, 0.0, -0.25)            # wavefront 1: one full-length lane among zero-length ones
    a[:, 77] = (1.0, 1.0, 0.0)
    a[:, 128:192, 1] = rng.uniform(0, 1, (H, 64)).astype(np.float32)      # wavefront 2: coast over the whole [0, 1]
    return a


def test_lanes_of_a_wavefront_are_independent():
    import torch
    a, b = make_env(), make_env()
    actions = edge_actions()
    t0 = time.time()
    got = kept(a.rollout(actions))
    torch.cuda.synchronize()
    assert time.time() - t0 < 5.0
    inner = got["inner_steps"]
    assert inner.max() <= 1461
    assert np.all(inner[:, 0:64] == 0), "zero-length and non-finite cycles run no Euler step"
    assert np.all(inner[:, 77] >= 1449) and np.all(np.delete(inner[:, 64:128], 13, axis=1) == 0)
    assert inner[:, 128:192].min() < 300 and inner[:, 128:192].max() > 1000
    want = run_steps(b, actions)
    assert_same_run(got, want, a.get_state(), b.get_state(), "edges")
    for e in (a, b):
        e.close()


# ---------------------------------------------------------------- 3. / 4. actions are the policy of the row; the closed loop replayed
@pytest.mark.parametrize("hidden", [(), (16,), (32, 16), (64, 64)], ids=lambda h: "x".join(map(str, h)) or "linear")
def test_actions_are_the_policy_of_the_row(hidden):
    env, twin = make_env(), make_env()
    policy = robot_policy(hidden)
    entry = host(env.observe())
    assert np.array_equal(entry, host(twin.reset(mask=np.zeros(N, np.uint8))[0])), "the entry row is what reset with a zero mask returns"
    out = kept(env.rollout_policy(policy, H))
    seen = rows_seen(entry, out["obs"])
    _, want = py_forward(policy, policy.pack(), seen)
    assert np.array_equal(out["actions"].view(np.uint32), want.view(np.uint32)), \
        f"actions differ from py_forward in {int((out['actions'] != want).sum())} words"
    lo, hi = SHIFT - SCALE, SHIFT + SCALE
    assert np.all(out["actions"] >= lo) and np.all(out["actions"] <= hi)
    assert out["actions"][..., 0].std() > 0.05, "the policy must not sit on the clamp"
    assert out["inner_steps"].max() <= 601 and np.ptp(out["inner_steps"][:, :64]) > 50, "cycle lengths must differ inside a wavefront"
    # 4. the same actions through seven `step` calls on a twin
    replay = run_steps(twin, out["actions"])
    assert_same_run(out, replay, env.get_state(), twin.get_state(), f"closed loop {hidden}")
    for e in (env, twin):
        e.close()


def test_closed_loop_replayed_across_episode_endings():
    env, twin = make_env(max_cycles=2), make_env(max_cycles=2)
    policy = robot_policy((32, 16))
    entry = host(env.observe())
    out = kept(env.rollout_policy(policy, H))
    assert out["truncated"][1::2].all() and not out["truncated"][0::2].any(), "every episode ends on its second cycle"
    # after an autoreset the policy sees the first row of the new episode
    _, want = py_forward(policy, policy.pack(), rows_seen(entry, out["obs"]))
    assert np.array_equal(out["actions"].view(np.uint32), want.view(np.uint32))
    replay = run_steps(twin, out["actions"])
    assert_same_run(out, replay, env.get_state(), twin.get_state(), "closed loop, max_cycles = 2")
    for e in (env, twin):
        e.close()


def test_tanh_policy_is_within_its_error_bound():
    env = make_env()
    policy = robot_policy((32, 16), out="tanh")
    entry = host(env.observe())
    out = kept(env.rollout_policy(policy, H))
    seen = rows_seen(entry, out["obs"])
    err = np.abs(out["actions"].astype(np.float64) - policy.reference(seen))
    bound = policy.error_bound(seen)
    assert np.all(err <= bound), float((err / bound).max())
    assert bound.max() < 1e-4
    env.close()


# ---------------------------------------------------------------- 5. against the oracle
def test_closed_loop_matches_the_oracle():
    steps = 5
    env = make_env()
    orc = rol.RobotOracleVec(N, seed=SEED)
    policy = robot_policy((32, 16))
    assert rel(host(env.observe()), orc.reset(np.zeros(N, np.uint8))) <= 1e-6
    out = kept(env.rollout_policy(policy, steps))
    for t in range(steps):
        ref = orc.step(out["actions"][t])
        assert np.array_equal(out["inner_steps"][t], ref["inner_steps"]), t
        assert np.array_equal(out["terminated"][t], ref["terminated"].astype(bool)), t
        assert np.array_equal(out["truncated"][t], ref["truncated"].astype(bool)), t
        assert rel(out["obs"][t], ref["obs"]) <= 1e-6 and rel(out["reward"][t], ref["reward"]) <= 1e-5, t
    assert rel(env.get_state(), orc.get_state()) <= 1e-6
    env.close()
    orc.close()


# ---------------------------------------------------------------- 6. population
def test_population_halves_equal_the_single_policies():
    n = 256
    ps = [robot_policy((16,), seed=41), robot_policy((16,), seed=42, out_gain=4.0)]
    both = make_env(n)
    out = kept(both.rollout_policy(MLPPolicy.stack(ps), H))
    state = both.get_state()
    refs = []
    for k, p in enumerate(ps):
        alone = make_env(n)
        ref = kept(alone.rollout_policy(p, H))
        half = slice(128 * k, 128 * (k + 1))
        for key in FLOAT_KEYS + EXACT_KEYS + ("actions",):
            assert np.array_equal(out[key][:, half], ref[key][:, half]), (k, key)
        assert np.array_equal(state[:, half], alone.get_state()[:, half]), k
        refs.append(ref)
        alone.close()
    # the two policies are clearly different: on the same envs their actions are far apart
    assert np.abs(refs[0]["actions"] - refs[1]["actions"]).mean() > 0.05
    # a P that n does not allow
    three = MLPPolicy.stack(ps + [robot_policy((16,), seed=43)])
    with pytest.raises(ValueError):
        both.make_policy(three)
    assert both.L.salp_robot_policy_words(both._h, ctypes.byref(three.desc())) == INVALID
    p = ctypes.c_void_p()
    assert both.L.salp_robot_policy_create(both._h, ctypes.byref(three.desc()), SalpLib._ptr(three.pack()), 0, None, ctypes.byref(p)) == INVALID
    assert not p.value
    both.close()


# ---------------------------------------------------------------- 7. determinism, host and device pointers
def test_runs_are_deterministic_and_pointer_forms_agree():
    policy = robot_policy((32, 16))
    runs = []
    for output in ("numpy", "numpy", "torch"):
        env = make_env(output=output, max_cycles=2)
        bufs = env._rollout_outputs(H)          # the blocks the next rollout writes: final_obs goes in as well as out
        bufs[4][...] = float(SENTINEL)
        out = kept(env.rollout_policy(policy, H))
        runs.append((out, env.get_state()))
        env.close()
    (a, sa), (b, sb), (c, sc) = runs
    for other, so, what in ((b, sb, "second run"), (c, sc, "device pointers")):
        for key in a:
            assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint8), np.ascontiguousarray(other[key]).view(np.uint8)), (what, key)
        assert np.array_equal(sa, so), what
    done = a["_final_observation"]
    fin = a["final_observation"].view(np.uint32)
    assert done.any() and not done.all()
    assert np.all(fin[~done] == 0xA5C3F00D), "final_obs rows of running episodes were written"
    assert not np.any(fin[done] == 0xA5C3F00D), "final_obs rows of ended episodes were not written"


# ---------------------------------------------------------------- 8. continuation
def test_a_second_call_continues_the_first():
    env = make_env()
    policy = robot_policy((16,))
    first = kept(env.rollout_policy(policy, 3))
    second = kept(env.rollout_policy(policy, 2))
    _, want = py_forward(policy, policy.pack(), first["obs"][-1:])
    assert np.array_equal(second["actions"][0].view(np.uint32), want[0].view(np.uint32))
    env.close()
    # open loop: 3 + 4 steps against 7
    (a, b), actions = staggered_pair()
    p1 = kept(a.rollout(actions[:3]))
    p2 = kept(a.rollout(actions[3:]))
    parts = {k: np.concatenate([p1[k], p2[k]]) for k in p1}
    whole = kept(b.rollout(actions))
    assert_same_run(parts, whole, a.get_state(), b.get_state(), "3 + 4 steps against 7")
    for e in (a, b):
        e.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_launch_nothing():
    env, other = make_env(), make_env(64)
    L = env.L
    policy = robot_policy((16,))
    handle, foreign = env.make_policy(policy), other.make_policy(policy)
    act = np.zeros((H, N, 3), np.float32)
    obs, rew = np.empty((H, N, 6), np.float32), np.empty((H, N), np.float32)
    p = SalpLib._ptr
    before = env.get_state()
    rollout = lambda h, a, hz, flags, o=obs: L.salp_robot_vec_rollout(h, p(a), hz, p(o), p(rew), None, None, None, None, flags, None)
    closed = lambda h, pol, hz, flags, o=obs: L.salp_robot_vec_rollout_policy(h, pol, hz, p(o), p(rew), None, None, None, None, None, flags, None)
    cases = {
        "NULL handle": rollout(None, act, H, 0), "NULL act": rollout(env._h, None, H, 0),
        "horizon 0": rollout(env._h, act, 0, 0), "horizon above the cap": rollout(env._h, act, 1025, 0),
        "unknown flag bits": rollout(env._h, act, H, 2),
        "no main output": L.salp_robot_vec_rollout(env._h, p(act), H, None, None, None, None, p(obs), None, 0, None),
        "policy: NULL handle": closed(None, handle._p, H, 0), "NULL policy": closed(env._h, None, H, 0),
        "policy: horizon 0": closed(env._h, handle._p, 0, 0), "policy: horizon above the cap": closed(env._h, handle._p, 1025, 0),
        "policy: unknown flag bits": closed(env._h, handle._p, H, 4),
        "policy: no main output": L.salp_robot_vec_rollout_policy(env._h, handle._p, H, None, None, None, None, p(obs), None, None, 0, None),
        "a policy of another handle": closed(env._h, foreign._p, H, 0),
    }
    for what, rc in cases.items():
        assert rc == INVALID, (what, rc, L.salp_robot_last_error())
    # a descriptor outside the ranges; a P that n does not allow; NULL weights
    d = policy.desc()
    d.hidden[0] = 24
    out = ctypes.c_void_p()
    assert L.salp_robot_policy_words(env._h, ctypes.byref(d)) == INVALID
    assert L.salp_robot_policy_create(env._h, ctypes.byref(d), p(policy.pack()), 0, None, ctypes.byref(out)) == INVALID
    d = policy.desc()
    d.n_policies = 2                      # 357 envs
    assert L.salp_robot_policy_words(env._h, ctypes.byref(d)) == INVALID
    assert L.salp_robot_policy_words(None, ctypes.byref(policy.desc())) == INVALID
    assert L.salp_robot_policy_create(env._h, ctypes.byref(policy.desc()), None, 0, None, ctypes.byref(out)) == INVALID
    assert L.salp_robot_policy_update(handle._p, None, 0, None) == INVALID
    assert L.salp_robot_policy_words(env._h, ctypes.byref(policy.desc())) == policy.words
    assert np.array_equal(env.get_state(), before), "a refused call changed the state"
    with pytest.raises(ValueError):
        env.make_policy(policy_cases.random_policy(24, 3, (16,), "clip", 5, 1.0, 1.0))
    env.close()
    other.close()


# ---------------------------------------------------------------- 10. capture
def test_rollout_policy_is_capturable():
    import torch
    steps = 3
    p1, p2 = robot_policy((32, 16), seed=51), robot_policy((32, 16), seed=52)
    w1, w2 = (torch.from_numpy(q.pack()).to("cuda:0") for q in (p1, p2))
    keys = ("obs", "reward", "terminated", "truncated", "inner_steps", "actions")

    def prepared():
        env = make_env(output="torch")
        handle = env.make_policy(p1, weights=w1)
        env.rollout_policy(handle, steps)            # warm-up: buffers, lazy kernel load
        torch.cuda.synchronize()
        return env, handle

    env, handle = prepared()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.rollout_policy(handle, steps)
    got = []
    g.replay()
    got.append({k: host(out[k]) for k in keys})
    handle.update(w2)
    g.replay()
    got.append({k: host(out[k]) for k in keys})
    torch.cuda.synchronize()
    state = env.get_state()

    twin, twin_handle = prepared()
    want = [{k: host(v) for k, v in twin.rollout_policy(twin_handle, steps).items() if k in keys}]
    twin_handle.update(w2)
    want.append({k: host(v) for k, v in twin.rollout_policy(twin_handle, steps).items() if k in keys})
    for r, (a, b) in enumerate(zip(got, want)):
        for k in keys:
            assert np.array_equal(a[k], b[k]), (r, k)
    assert not np.array_equal(got[0]["actions"], got[1]["actions"])
    assert np.array_equal(state, twin.get_state())
    env.close()
    twin.close()
