"""Cycle history of the HEAD simulator on the GPU (salp_robot_step_record_kernel through salp_robot_vec_step_history,
include/salp_robot.h): against the reference's own histories, bit-identical step results with and without recording,
consistency with the observations at 65536 robots under the longest-cycle-first schedule, no stray writes, argument
checks, and hipGraph capture."""
import ctypes
import json
import os

import numpy as np
import pytest

from underwater_swimmer_rl_amd.robot_env import H_COUNT, H_STATE, SalpRobotVectorEnv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "history_robot_cycles.npz")
SENTINEL = -12345.0


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_history_matches_reference(output):
    z = np.load(GOLD, allow_pickle=False)
    o = z["offsets"]
    seen = 0
    for k, _ in enumerate(z["case_names"]):
        meta = json.loads(str(z[f"c{k}_meta"]))
        act = z[f"c{k}_actions"]
        T, n, _ = act.shape
        env = SalpRobotVectorEnv(n, device="cuda:0", seed=meta["seed"], env_index_base=meta["env_index_base"], output=output)
        env.record_history(None, stride=1)
        for t in range(T):
            obs, rew, term, trunc, info = env.step(act[t])
            assert info["cycle_history_envs"] == (0, n)
            hist, hlen = _np(info["cycle_history"]), _np(info["cycle_history_len"])
            for j in np.flatnonzero((z["rec_case"] == k) & (z["rec_step"] == t)):
                i = int(z["rec_env"][j])
                ref = z["history"][o[j]:o[j + 1]]
                assert hlen[i] == len(ref) == z["rec_inner_steps"][j] + 1, (k, t, i)
                got = hist[i, :hlen[i]].astype(np.float64)
                assert np.array_equal(got[:, H_STATE], ref[:, H_STATE]), (k, t, i)
                err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
                assert err.max() <= 1e-6, (k, t, i, float(err.max()), np.unravel_index(err.argmax(), err.shape))
                d = env.history_of(i)
                assert d["position_history"].shape == (hlen[i], 3) and d["state_history"].dtype == np.int64
                assert np.array_equal(d["length_history"], got[:, 12])
                seen += 1
        env.close()
    assert seen == len(z["rec_case"])


def _actions(rng, n, coast=0.3, lo=-0.2, hi=1.2):
    return np.stack([rng.uniform(lo, hi, n), rng.uniform(0, coast, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)


@pytest.mark.parametrize("schedule", ["0", "1"])
def test_recording_changes_nothing(schedule, monkeypatch):
    monkeypatch.setenv("SALP_ROBOT_SCHEDULE", schedule)
    n, seed, T = 5000, 9, 5
    rng = np.random.default_rng(4)
    acts = [_actions(rng, n) for _ in range(T)]
    acts[1][:300, 1] = 3.0                       # 30 s asked: cut at 14.6 s, some envs leave the 5 m radius
    runs = []
    for mode in (None, (None, 1), (slice(1000, 2300), 7)):
        env = SalpRobotVectorEnv(n, device="cuda:0", seed=seed)
        if mode:
            env.record_history(mode[0], stride=mode[1])
        rec = []
        for a in acts:
            obs, rew, term, trunc, info = env.step(a)
            done = _np(term | trunc)
            rec.append([_np(x).copy() for x in (obs, rew, term, trunc, info["inner_steps"])] +
                       [_np(info["final_observation"])[done].copy()])
        rec.append([env.get_state()])
        runs.append(rec)
        env.close()
    assert any(r[5].size for r in runs[0][:-1])
    for other in runs[1:]:
        for r0, r1 in zip(runs[0], other):
            for x0, x1 in zip(r0, r1):
                assert np.array_equal(x0, x1, equal_nan=True)


def test_history_consistency_at_scale():
    """65536 robots (schedule on): a recorded range across wavefront and block edges."""
    import torch
    n, seed, T, s = 65536, 21, 4, 5
    begin, count = 3 * 256 - 37, 2 * 256 + 101
    envs = [SalpRobotVectorEnv(n, device="cuda:0", seed=seed) for _ in range(2)]
    envs[0].record_history(slice(begin, begin + count), stride=1)
    envs[1].record_history(slice(begin, begin + count), stride=s)
    rng = np.random.default_rng(8)
    prev_last = None
    for t in range(T):
        a = _actions(rng, n, coast=0.1, lo=0.0, hi=1.0)
        if t == 2:
            a[begin:begin + 40, 1] = 3.0
        outs = [e.step(a) for e in envs]
        torch.cuda.synchronize()
        obs, _, term, trunc, info = outs[0]
        h1, l1 = _np(info["cycle_history"]), _np(info["cycle_history_len"])
        hs, ls = _np(outs[1][4]["cycle_history"]), _np(outs[1][4]["cycle_history_len"])
        inner = _np(info["inner_steps"])[begin:begin + count]
        done = _np(term | trunc)[begin:begin + count]
        ref_obs = np.where(done[:, None], _np(info["final_observation"])[begin:begin + count], _np(obs)[begin:begin + count])
        assert np.array_equal(l1, inner + 1)
        last = h1[np.arange(count), l1 - 1]
        assert np.array_equal(last[:, [3, 4, 8, 11]], ref_obs[:, 2:6])
        if prev_last is not None:
            keep = ~prev_done
            assert np.array_equal(h1[keep, 0, :12], prev_last[keep, :12])
        for j in range(count):
            idx = list(range(0, inner[j] + 1, s))
            if idx[-1] != inner[j]:
                idx.append(inner[j])
            assert ls[j] == len(idx)
            assert np.array_equal(hs[j, :ls[j]], h1[j, idx]), j
        prev_last, prev_done = last.copy(), done.copy()
    for e in envs:
        e.close()


def _raw_step(env, a, begin, count, stride, cap, hist_ptr, len_ptr, flags, stream=None):
    p = env._p
    return env.L.salp_robot_vec_step_history(env._h, p(a), p(env._obs), p(env._rew), p(env._term), p(env._trunc), p(env._fin),
                                             p(env._inner), begin, count, stride, cap, hist_ptr, len_ptr, flags, stream)


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_history_writes_stay_in_place(output):
    """Buffers filled with a sentinel: samples past history_len and rows around the recorded range are never written."""
    import torch
    n, begin, count, stride = 700, 129, 300, 3
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=2, output=output)
    cap = env.history_capacity(stride)
    rng = np.random.default_rng(1)
    for _ in range(2):
        a = _actions(rng, n, coast=0.2, lo=0.0, hi=1.0)
        if output == "torch":
            buf = torch.full((count + 2, cap, H_COUNT), SENTINEL, device="cuda:0")
            lens = torch.full((count + 2,), -7, dtype=torch.int32, device="cuda:0")
            at = torch.as_tensor(a, device="cuda:0")
            rc = _raw_step(env, at, begin, count, stride, cap, ctypes.c_void_p(buf[1].data_ptr()),
                           ctypes.c_void_p(lens[1].data_ptr()), 1, env._stream)
            torch.cuda.synchronize()
        else:
            buf = np.full((count + 2, cap, H_COUNT), SENTINEL, np.float32)
            lens = np.full((count + 2,), -7, np.int32)
            rc = _raw_step(env, a, begin, count, stride, cap, ctypes.c_void_p(buf[1:].ctypes.data),
                           ctypes.c_void_p(lens[1:].ctypes.data), 0)
        assert rc == 0
        buf, lens, inner = _np(buf), _np(lens), _np(env._inner)[begin:begin + count]
        assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL) and lens[0] == -7 and lens[-1] == -7
        L = lens[1:-1]
        assert np.array_equal(L, (inner + stride - 1) // stride + 1)
        # device pointers: nothing past history_len is written; host pointers: rows come back up to the longest
        # record of the call (include/salp_robot.h), nothing past it
        end = L if output == "torch" else np.full_like(L, L.max())
        for j in range(count):
            assert np.all(buf[1 + j, end[j]:] == SENTINEL) and not np.any(buf[1 + j, :L[j]] == SENTINEL)
    env.close()


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_empty_history_range_is_the_plain_step(output):
    """hist_count == 0 (history NULL) is salp_robot_vec_step: same outputs and state, bit for bit."""
    n, T = 900, 3
    envs = [SalpRobotVectorEnv(n, device="cuda:0", seed=17, output=output) for _ in range(2)]
    rng = np.random.default_rng(3)
    for _ in range(T):
        a = _actions(rng, n)
        for e in envs:
            e._fin[:] = 0
        envs[0].step(a)
        a1 = a
        if output == "torch":
            import torch
            a1 = torch.as_tensor(a, device="cuda:0")
        assert _raw_step(envs[1], a1, 0, 0, 1, 0, None, None, envs[1]._flags, envs[1]._stream) == 0
        for name in ("_obs", "_rew", "_term", "_trunc", "_fin", "_inner"):
            assert np.array_equal(_np(getattr(envs[0], name)), _np(getattr(envs[1], name))), name
    assert np.array_equal(envs[0].get_state(), envs[1].get_state())
    for e in envs:
        e.close()


def test_tiny_dt_is_refused_by_the_history_calls():
    """A dt whose longest cycle exceeds 2^24 Euler steps: capacity -1 and a clean -1 from the step, no launch."""
    env = SalpRobotVectorEnv(64, device="cuda:0", seed=1, output="numpy", dt=1e-9)
    assert env.L.salp_robot_vec_history_capacity(env._h, 1) == -1
    with pytest.raises(ValueError):
        env.record_history(None)
    buf = np.zeros((64, 4, H_COUNT), np.float32)
    a = np.zeros((64, 3), np.float32)
    assert _raw_step(env, a, 0, 64, 1, 4, ctypes.c_void_p(buf.ctypes.data), None, 0) == -1
    assert b"dt" in env.L.salp_robot_last_error()
    env.close()


def test_capacity_of_the_built_library_is_the_host_twin():
    """The library that runs on the GPU counts what tests/test_robot_params_host.py checks on the host: handles and
    capacities only, no step (a step at dt = 8e-7 is millions of Euler steps)."""
    import robot_params_host_lib as rp
    for dt in (0.01, 0.005, 0.02, 8e-7):
        env = SalpRobotVectorEnv(64, device="cuda:0", seed=1, output="numpy", dt=dt)
        steps = rp.max_steps(dt)
        assert (steps == -1) == (dt == 8e-7)
        for s in (1, 4, 10):
            assert env.L.salp_robot_vec_history_capacity(env._h, s) == rp.history_capacity(steps, s), (dt, s)
        env.close()


def test_rejected_arguments_launch_nothing():
    import torch
    n = 512
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=3)
    cap = env.history_capacity(1)
    assert cap == 1462 and env.history_capacity(10) == 148 and env.L.salp_robot_vec_history_capacity(env._h, 0) == -1
    buf = torch.zeros((n, cap, H_COUNT), device="cuda:0")
    lens = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    a = torch.full((n, 3), 0.5, device="cuda:0")
    env._obs.fill_(SENTINEL)
    state0 = env.get_state()
    hp, lp = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(lens.data_ptr())
    for begin, count, stride, c, h in ((0, 10, 0, cap, hp), (-1, 10, 1, cap, hp), (500, 13, 1, cap, hp), (0, n + 1, 1, cap, hp),
                                       (0, 10, 1, cap - 1, hp), (0, 10, 4, env.history_capacity(4) - 1, hp), (0, 10, 1, cap, None)):
        assert _raw_step(env, a, begin, count, stride, c, h, lp, 1, env._stream) == -1, (begin, count, stride, c)
        assert env.L.salp_robot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(env._obs == SENTINEL) and not buf.any() and not lens.any()
    assert np.array_equal(env.get_state(), state0)
    env.close()


def test_recorded_step_in_a_graph_matches_eager():
    import torch
    n, seed = 3000, 13
    a = torch.as_tensor(_actions(np.random.default_rng(6), n, coast=0.2, lo=0.0, hi=1.0), device="cuda:0")
    eager, graphed = (SalpRobotVectorEnv(n, device="cuda:0", seed=seed) for _ in range(2))
    for e in (eager, graphed):
        e.record_history(slice(1000, 1700), stride=2)
    static_a = a.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step(static_a)
    g.replay()
    obs_e, rew_e, _, _, info_e = eager.step(a)
    torch.cuda.synchronize()
    info_g = {"cycle_history": graphed._hist[4], "cycle_history_len": graphed._hist[5]}
    assert torch.equal(graphed._obs, obs_e) and torch.equal(graphed._rew, rew_e)
    L = info_e["cycle_history_len"]
    assert torch.equal(info_g["cycle_history_len"], L)
    he, hg = info_e["cycle_history"].cpu().numpy(), info_g["cycle_history"].cpu().numpy()
    for j, lj in enumerate(L.cpu().numpy()):
        assert np.array_equal(he[j, :lj], hg[j, :lj])
    assert np.array_equal(eager.get_state(), graphed.get_state())
    del g
    eager.close(); graphed.close()
