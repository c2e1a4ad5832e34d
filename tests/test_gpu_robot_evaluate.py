"""Policy evaluation on the HEAD simulator (salp_robot_vec_evaluate_policy, _sampled; include/salp_robot_evaluate.h): one
summary record per robot instead of per-step blocks.  The reference of every test is a TWIN — a second env of the same
seed and config driven through `rollout_policy` — folded by `policy.summarize_robot_rollout`, the numpy statement of the
record (tests/test_robot_evaluate_summary.py).

Unless a test says otherwise: 357 envs (two workgroups, the last wavefront ragged) and 7 env steps, as
tests/test_gpu_robot_rollout.py; every test is a few thousand Euler iterations.

Same chunking and no stop: the record must equal the twin's fold as 48 bytes per robot (the kernel is the rollout kernel
with another output signature: the same service schedule, the same arithmetic).  Where the chunking differs (3 + 4 against
7) or lanes stop (first_episode), which lanes of a wavefront step together differs, so the integer fields must be identical
and the two float64 sums within H * 2^-22 * max(1, max |reward|): include/salp_robot_rollout.h's per-output contract, which
`assert_same_run` of tests/test_gpu_robot_rollout.py applies to each float32 reward (2^-22 relative to max(1, |x|)), summed
over the H rewards of a record.  Each such comparison prints whether the sums were in fact bit-identical."""
import ctypes

import numpy as np
import pytest

import robot_sampled_cases as cases
from test_gpu_robot_rollout import H, INVALID, N, host, kept, make_env, robot_policy, schedule_mix
from underwater_swimmer_rl_amd._capi import SalpLib
from underwater_swimmer_rl_amd.policy import (REVAL_EPISODES, REVAL_FIRST_END, REVAL_FIRST_LENGTH, REVAL_WORDS, MLPPolicy,
                                              robot_evaluation_views, summarize_robot_rollout)
from underwater_swimmer_rl_amd.robot_env import R_CYCLE, R_POS, R_RNG, R_TIME

pytestmark = pytest.mark.gpu

WAVE = 64
SENTINEL = np.int32(0x5AC3F00D)
INT_WORDS = slice(4, REVAL_WORDS)          # every word behind the two float64 sums
FIELDS = ("return_sum", "first_return", "euler_steps", "first_length", "first_end", "episodes", "reached", "first_euler_steps")


def staggered(count, output="numpy", n=N):
    """`count` envs of one seed with max_cycles = 3 in the staggered start of tests/test_gpu_robot_rollout.py: one open-loop
    step, then the envs with i % 3 == 0 reset, so that episodes end on different steps in different lanes."""
    first = schedule_mix(np.random.default_rng(1), 5, n)[0]
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    envs = [make_env(n, output=output, max_cycles=3) for _ in range(count)]
    for e in envs:
        e.step(first)
        e.reset(mask=mask)
    return envs


def fold(out, record=None, first_episode=False):
    return summarize_robot_rollout(out["reward"], out["terminated"], out["truncated"], out["inner_steps"], record=record,
                                   first_episode=first_episode)


def same_bytes(a, b):
    return np.ascontiguousarray(host(a)).tobytes() == np.ascontiguousarray(host(b)).tobytes()


def differing(got, want):
    """The names of the fields in which two record blocks differ."""
    g, w = robot_evaluation_views(np.ascontiguousarray(host(got))), robot_evaluation_views(np.ascontiguousarray(host(want)))
    return [k for k in FIELDS if not np.array_equal(g[k].view(np.int64 if g[k].dtype.itemsize == 8 else np.int32),
                                                    w[k].view(np.int64 if w[k].dtype.itemsize == 8 else np.int32))]


def assert_same_sums(got, want, rewards, steps, what):
    """Integer fields identical; the float64 sums within steps * 2^-22 * max(1, max |reward|) (top of the file)."""
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(host(want))
    assert np.array_equal(got[:, INT_WORDS], want[:, INT_WORDS]), f"{what}: integer fields differ: {differing(got, want)}"
    tol = steps * 2.0 ** -22 * max(1.0, float(np.abs(rewards).max()))
    g, w = robot_evaluation_views(got), robot_evaluation_views(want)
    worst = max(float(np.abs(g[k] - w[k]).max()) for k in ("return_sum", "first_return"))
    print(f"{what}: float64 sums bit-identical = {same_bytes(got[:, :4], want[:, :4])}; max |diff| {worst:.3g}, bound {tol:.3g}")
    assert worst <= tol, f"{what}: float64 sums differ by {worst}, bound {tol}"


def mixed_wavefront(flag_row, n=N):
    """Does some whole wavefront hold both lanes with the flag and lanes without it?"""
    full = flag_row[:n // WAVE * WAVE].reshape(-1, WAVE).sum(axis=1)
    return bool(np.any((full > 0) & (full < WAVE)))


# ---------------------------------------------------------------- 1. the record equals the twin, bit for bit
@pytest.mark.parametrize("hidden", [(), (32, 16)], ids=lambda h: "x".join(map(str, h)) or "linear")
def test_record_equals_the_twin(hidden):
    import torch
    env, twin = staggered(2, output="torch")
    policy = robot_policy(hidden)
    block = torch.full((N + 1, REVAL_WORDS), int(SENTINEL), dtype=torch.int32, device="cuda:0")
    got = env.evaluate_policy(policy, H, out=block[:N])
    out = kept(twin.rollout_policy(policy, H))
    finished = out["_final_observation"]
    ending_steps = np.flatnonzero(finished.any(axis=1))
    print("finishers per step:", finished.sum(axis=1).tolist())
    assert len(ending_steps) >= 2, "endings must fall on at least two different steps"
    assert all(mixed_wavefront(finished[t]) for t in ending_steps), "finished and unfinished lanes must share a wavefront"
    assert np.ptp(out["inner_steps"][:, :WAVE]) > 50, "cycle lengths must differ inside a wavefront"
    want = fold(out)
    rec = host(block)
    assert same_bytes(rec[:N], want), f"record differs from the twin's summary in {differing(rec[:N], want)}"
    assert np.all(rec[N] == SENTINEL), "the row behind the last robot was written"
    assert got["record"].data_ptr() == block.data_ptr() and same_bytes(got["return_sum"], robot_evaluation_views(want)["return_sum"])
    assert not rec[:N, REVAL_WORDS - 1].any()
    assert np.array_equal(env.get_state(), twin.get_state()), "the final states differ"
    for e in (env, twin):
        e.close()


# ---------------------------------------------------------------- 2. targets reached
def origin_env(n):
    """Every target is exactly the origin, where a robot starts: x_min = y_min = 0 and both spans are 0."""
    return make_env(n, width=100, height=100, tank_margin=50.0, max_cycles=3)


def constant_policy(action):
    return MLPPolicy.linear(np.zeros((3, 6), np.float32), np.asarray(action, np.float32), out="clip")


def test_targets_reached_and_missed_by_wavefront():
    """Wavefront 0 takes (0.02, 0, 0): 9 Euler steps, and it is still within 0.01 of the target: terminated on every step.
    Wavefront 1 takes (1, 0, 0.5): 451 Euler steps away from the target, never terminated, truncated on every third cycle."""
    n = 128
    policy = MLPPolicy.stack([constant_policy((0.02, 0.0, 0.0)), constant_policy((1.0, 0.0, 0.5))])
    env, twin = origin_env(n), origin_env(n)
    v = env.evaluate_policy(policy, H)
    expect = {0: dict(reached=7, episodes=7, first_end=1, first_length=1, euler_steps=63, first_euler_steps=9),
              1: dict(reached=0, episodes=2, first_end=2, first_length=3, euler_steps=7 * 451, first_euler_steps=3 * 451)}
    for w, fields in expect.items():
        for k, x in fields.items():
            assert np.all(host(v[k])[WAVE * w:WAVE * (w + 1)] == x), (w, k, host(v[k])[WAVE * w:WAVE * (w + 1)][:4], x)
    out = kept(twin.rollout_policy(policy, H))
    assert same_bytes(v["record"], fold(out)), differing(v["record"], fold(out))
    assert np.array_equal(env.get_state(), twin.get_state())
    for e in (env, twin):
        e.close()


def test_terminating_and_moving_lanes_in_one_wavefront():
    """One open-loop step, (0, 0, 0) on even lanes and (1, 0, 0.5) on odd ones, then a0 = clip(0.02 + 20 obs[0]): the even
    lanes sit on the target and terminate on every step, the odd ones swim, are truncated and only then sit on it."""
    n = 128
    first = np.zeros((n, 3), np.float32)
    first[1::2] = (1.0, 0.0, 0.5)
    W = np.zeros((3, 6), np.float32)
    W[0, 0] = 20.0
    policy = MLPPolicy.linear(W, np.array([0.02, 0.0, 0.0], np.float32), out="clip")
    env, twin = origin_env(n), origin_env(n)
    for e in (env, twin):
        e.step(first)
    v = env.evaluate_policy(policy, H)
    out = kept(twin.rollout_policy(policy, H))
    term, inner = out["terminated"][:, :WAVE], out["inner_steps"][:, :WAVE]
    assert term[:, 0::2].all(), "the even lanes terminate on every step"
    assert any(term[t].any() and (inner[t][~term[t]] > 100).any() for t in range(H)), "terminating and moving lanes must mix"
    assert out["truncated"][:, :WAVE].any() and len(np.unique(host(v["first_end"])[:WAVE])) == 2
    assert same_bytes(v["record"], fold(out)), differing(v["record"], fold(out))
    assert np.array_equal(env.get_state(), twin.get_state())
    for e in (env, twin):
        e.close()


# ---------------------------------------------------------------- 3. sampled actions
def test_sampled_record_equals_the_twin():
    env, twin, mean = staggered(3)
    policy = cases.case_policy("mlp32x16")
    handles = [e.make_policy(policy) for e in (env, twin)]
    for h in handles:
        h.set_noise_step(1000)
    v = env.evaluate_policy(handles[0], H, sample=True)
    out = kept(twin.rollout_policy(handles[1], H, sample=True))
    assert out["_final_observation"].any() and out["actions"].std(axis=1).min() > 0, "sampled actions differ between lanes"
    assert same_bytes(v["record"], fold(out)), differing(v["record"], fold(out))
    assert handles[0].noise_step == 1000 + H and handles[1].noise_step == 1000 + H
    assert np.array_equal(env.get_state(), twin.get_state())
    # the mean of the same policy is another run: the noise entered
    assert not same_bytes(mean.evaluate_policy(policy, H)["return_sum"], v["return_sum"])
    for e in (env, twin, mean):
        e.close()


# ---------------------------------------------------------------- 4. continuation
def test_a_cut_run_continues_its_records():
    env, twin, whole = staggered(3)
    policy = robot_policy((32, 16))
    first = env.evaluate_policy(policy, 3)
    assert (host(first["first_end"]) != 0).any(), "the second call must meet frozen FIRST_* fields"
    v = env.evaluate_policy(policy, 4, accumulate=True)
    assert v["record"] is first["record"], "without `out` the env continues its own block"
    a, b = kept(twin.rollout_policy(policy, 3)), kept(twin.rollout_policy(policy, 4))
    want = fold(b, record=fold(a))
    assert same_bytes(v["record"], want), f"3 + 4 steps differ from the twin's 3 + 4 in {differing(v['record'], want)}"
    assert np.array_equal(env.get_state(), twin.get_state())
    # against one call of 7: lanes resynchronise at the call boundary
    one = whole.evaluate_policy(policy, H)
    assert_same_sums(v["record"], one["record"], np.concatenate([a["reward"], b["reward"]]), H, "3 + 4 against 7")
    # without the flag the records are overwritten
    again = env.evaluate_policy(policy, 2)
    assert again["record"] is v["record"] and np.all(host(again["first_length"]) <= 2)
    for e in (env, twin, whole):
        e.close()


# ---------------------------------------------------------------- 5. stop at the end of the first episode
def test_first_episode_stop():
    env, twin, cut = staggered(3)
    policy = robot_policy((32, 16))
    start = twin.get_state()
    out = kept(twin.rollout_policy(policy, H))
    want = fold(out, first_episode=True)
    assert (robot_evaluation_views(fold(out))["episodes"] > 1).any(), "the unstopped twin runs on into second episodes"
    v = env.evaluate_policy(policy, H, first_episode=True)
    assert_same_sums(v["record"], want, out["reward"], H, "first episode, one call")
    g = {k: host(v[k]) for k in FIELDS}
    assert same_bytes(g["return_sum"], g["first_return"]) and np.array_equal(g["euler_steps"], g["first_euler_steps"])
    assert np.array_equal(g["episodes"], g["first_end"] != 0) and np.array_equal(g["reached"], g["first_end"] == 1)
    assert g["euler_steps"].sum() < robot_evaluation_views(fold(out))["euler_steps"].sum(), "stopping must save Euler steps"
    # a stopped robot sits at the start of its next episode, its draw counter one further
    stopped = g["first_end"] != 0
    assert stopped.all(), "with max_cycles = 3 every first episode ends within 7 steps"
    state = env.get_state()
    assert not state[R_POS:R_POS + 3].any() and not state[R_TIME].any() and not state[R_CYCLE].any()
    assert np.array_equal(state[R_RNG], start[R_RNG] + 1), "one reset draw since the start, the one that ended the first episode"
    # cut in two: after 2 steps one cohort has stopped, the other has not; the continued call steps only the latter
    first = cut.evaluate_policy(policy, 2, first_episode=True)
    rec2, state2 = host(first["record"]), cut.get_state()
    done = rec2[:, REVAL_FIRST_END] != 0
    assert done.any() and not done.all() and mixed_wavefront(done)
    assert not state2[R_POS:R_POS + 3, done].any() and not state2[R_CYCLE, done].any()
    assert np.array_equal(state2[R_RNG, done], start[R_RNG, done] + 1) and np.array_equal(state2[R_RNG, ~done], start[R_RNG, ~done])
    v2 = cut.evaluate_policy(policy, 5, accumulate=True, first_episode=True)
    rec7, state7 = host(v2["record"]), cut.get_state()
    assert same_bytes(rec7[done], rec2[done]), "the record of a stopped robot changed"
    assert same_bytes(state7[:, done], state2[:, done]), "the state rows of a stopped robot changed"
    assert np.all(rec7[~done, REVAL_FIRST_END] != 0) and not same_bytes(state7[:, ~done], state2[:, ~done])
    assert_same_sums(rec7, want, out["reward"], H, "first episode, 2 + 5 steps")
    # everything has stopped: one more continued call runs nothing at all
    v3 = cut.evaluate_policy(policy, 3, accumulate=True, first_episode=True)
    assert same_bytes(v3["record"], rec7) and same_bytes(cut.get_state(), state7)
    for e in (env, twin, cut):
        e.close()


# ---------------------------------------------------------------- 6. pointer forms and determinism
def test_runs_are_deterministic_and_pointer_forms_agree():
    import torch
    policy = robot_policy((32, 16))
    rng = np.random.default_rng(6)
    pre = summarize_robot_rollout(rng.normal(size=(4, N)).astype(np.float32), rng.random((4, N)) < 0.2, rng.random((4, N)) < 0.2,
                                  rng.integers(0, 1461, (4, N)))
    runs = []
    for output in ("numpy", "numpy", "torch"):
        (env,) = staggered(1, output=output)
        fresh = host(env.evaluate_policy(policy, 3)["record"])
        block = pre.copy() if output == "numpy" else torch.from_numpy(pre.copy()).to("cuda:0")
        v = env.evaluate_policy(policy, 4, out=block, accumulate=True)
        assert v["record"] is block
        runs.append((fresh, host(block), env.get_state()))
        env.close()
    for other, what in ((runs[1], "second run"), (runs[2], "device pointers")):
        for a, b, part in zip(runs[0], other, ("fresh record", "continued record", "state")):
            assert same_bytes(a, b), (what, part)
    # the pre-filled records were continued, not overwritten
    assert np.all(runs[0][1][:, REVAL_EPISODES] >= pre[:, REVAL_EPISODES]) and np.any(runs[0][1][:, REVAL_EPISODES] > pre[:, REVAL_EPISODES])
    assert np.all(robot_evaluation_views(runs[0][1])["euler_steps"] > robot_evaluation_views(pre)["euler_steps"])
    frozen = pre[:, REVAL_FIRST_END] != 0
    assert frozen.any() and same_bytes(runs[0][1][frozen][:, [2, 3, 6, 7, 10]], pre[frozen][:, [2, 3, 6, 7, 10]]), "FIRST_* must stay frozen"


# ---------------------------------------------------------------- 7. capture
def test_evaluate_policy_is_capturable():
    import torch
    steps = 3
    p1, p2 = robot_policy((32, 16), seed=51), robot_policy((32, 16), seed=52)
    w1, w2 = (torch.from_numpy(q.pack()).to("cuda:0") for q in (p1, p2))

    def prepared():
        (env,) = staggered(1, output="torch")
        handle = env.make_policy(p1, weights=w1)
        rec = torch.zeros((N, REVAL_WORDS), dtype=torch.int32, device="cuda:0")
        env.evaluate_policy(handle, steps, out=rec, accumulate=True)            # warm-up: lazy kernel load
        torch.cuda.synchronize()
        rec.zero_()
        return env, handle, rec

    env, handle, rec = prepared()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.evaluate_policy(handle, steps, out=rec, accumulate=True)
    assert not host(rec).any(), "capture must not execute"
    g.replay()
    after_one = host(rec)
    handle.update(w2)
    g.replay()
    torch.cuda.synchronize()

    twin, twin_handle, twin_rec = prepared()
    twin.evaluate_policy(twin_handle, steps, out=twin_rec, accumulate=True)
    assert same_bytes(after_one, twin_rec), "the first replay differs from the eager call"
    twin_handle.update(w2)
    twin.evaluate_policy(twin_handle, steps, out=twin_rec, accumulate=True)
    assert same_bytes(rec, twin_rec), differing(rec, twin_rec)
    assert np.all(host(rec)[:, REVAL_FIRST_LENGTH] >= 1) and not same_bytes(rec, after_one)
    assert np.array_equal(env.get_state(), twin.get_state())
    env.close()
    twin.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_launch_nothing():
    import torch
    env, other, tiny = make_env(), make_env(64), make_env(64, dt=1e-9)
    L, p = env.L, SalpLib._ptr
    plain = robot_policy((16,))
    gauss = cases.case_policy("mlp16")
    handle, foreign, on_tiny = env.make_policy(plain), other.make_policy(plain), tiny.make_policy(plain)
    ghandle, gforeign = env.make_policy(gauss), other.make_policy(gauss)
    ghandle.set_noise_step(41)
    rec = np.full((N, REVAL_WORDS), int(SENTINEL), np.int32)
    dev = torch.full((N + 1, REVAL_WORDS), int(SENTINEL), dtype=torch.int32, device="cuda:0")
    before = env.get_state()
    det, smp = L.salp_robot_vec_evaluate_policy, L.salp_robot_vec_evaluate_policy_sampled
    cases_ = {}
    for name, f, pol, bad_pol in (("evaluate", det, handle, foreign), ("sampled", smp, ghandle, gforeign)):
        cases_.update({
            f"{name}: NULL handle": f(None, pol._p, H, p(rec), 0, None),
            f"{name}: NULL policy": f(env._h, None, H, p(rec), 0, None),
            f"{name}: NULL rec": f(env._h, pol._p, H, None, 0, None),
            f"{name}: horizon 0": f(env._h, pol._p, 0, p(rec), 0, None),
            f"{name}: horizon above the cap": f(env._h, pol._p, 1025, p(rec), 0, None),
            f"{name}: flag bit 2": f(env._h, pol._p, H, p(rec), 2, None),
            f"{name}: flag bit 16": f(env._h, pol._p, H, p(rec), 4 | 8 | 16, None),
            f"{name}: misaligned device rec": f(env._h, pol._p, H, dev.data_ptr() + 8, 1, None),
            f"{name}: a policy of another handle": f(env._h, bad_pol._p, H, p(rec), 0, None),
        })
    cases_["sampled: a policy that is not Gaussian"] = smp(env._h, handle._p, H, p(rec), 0, None)
    tiny_rec = np.zeros((64, REVAL_WORDS), np.int32)
    cases_["a dt the history calls refuse"] = det(tiny._h, on_tiny._p, H, p(tiny_rec), 0, None)
    for what, rc in cases_.items():
        assert rc == INVALID, (what, rc, L.salp_robot_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), before), "a refused call changed the state"
    assert np.all(rec == SENTINEL) and np.all(host(dev) == SENTINEL) and not tiny_rec.any(), "a refused call wrote a record"
    assert ghandle.noise_step == 41, "a refused call moved the noise step"
    with pytest.raises(ValueError):
        env.evaluate_policy(handle, H, sample=True)
    with pytest.raises(ValueError):
        env.evaluate_policy(plain, H, out=np.zeros((N, 8), np.int32))
    assert np.array_equal(env.get_state(), before) and ghandle.noise_step == 41
    # and the same arguments, put right, are accepted
    assert smp(env._h, ghandle._p, H, p(rec), 0, None) == 0 and ghandle.noise_step == 41 + H
    assert not np.any(rec[:, REVAL_WORDS - 1]) and np.all(rec[:, REVAL_FIRST_LENGTH] >= 1)
    for e in (env, other, tiny):
        e.close()
