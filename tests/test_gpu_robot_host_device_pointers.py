"""Host pointers equal device pointers, bit for bit, across the C ABI of include/salp_robot.h: reset (mask, NULL mask, the
all-zero mask of observe), step, step_history, trajectory and get_state.  The host-pointer forms go through staged() of
csrc/salp_host.h; this is the robot twin of test_gpu_host_device_pointers.py.

Two SalpRobotVectorEnv of one seed, one with numpy arrays and one with device tensors, get the same raw ABI calls; every
output starts out as a sentinel and must come back equal.  100 envs (one workgroup: a full and a partial wavefront) and
321 (two workgroups, the last one partial); max_cycles = 2, so every episode is truncated on its second step and final_obs
— an output that is also an input: rows of episodes that did not end must come back as they went in — really gets
written.  Actions lie in the action Box with a coast of at most 0.3 (3 s), so a cycle is a few hundred Euler steps."""
import numpy as np
import pytest

from underwater_swimmer_rl_amd._capi import SalpLib
from underwater_swimmer_rl_amd.robot_compare import PER_ROBOT_ACTIONS, robot_params
from underwater_swimmer_rl_amd.robot_env import H_COUNT, R_COUNT, SalpRobotVectorEnv

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float32): np.uint32(0xA5C3F00D).view(np.float32), np.dtype(np.uint8): 0xA5,
            np.dtype(np.int32): -1515982835, np.dtype(np.float64): -7.25}
SCALE = np.array([0.06, 10.0, np.pi / 2])     # Box action -> contraction (m), coast time (s), nozzle yaw (rad)


class Pair:
    """The same ABI call on both handles: `out(...)` / `given(...)` make a host array and a device tensor of equal
    contents, `call` runs the function on each handle with its own set (and SALP_DEVICE_PTRS on the device side),
    `check` compares every array made since the last check."""

    def __init__(self, n):
        import torch
        self.torch = torch
        self.host = SalpRobotVectorEnv(n, device="cuda:0", seed=11, output="numpy", max_cycles=2)
        self.dev = SalpRobotVectorEnv(n, device="cuda:0", seed=11, output="torch", max_cycles=2)
        self.made = []

    def given(self, a, name="input"):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.copy()).to("cuda:0")
        self.made.append((name, a, t))
        return (a, t)

    def out(self, name, shape, dtype):
        return self.given(np.full(shape, SENTINEL[np.dtype(dtype)], dtype), name)

    def call(self, function, *args, flags=0):
        for side, env in enumerate((self.host, self.dev)):
            rc = getattr(env.L, function)(env._h, *[SalpLib._ptr(a[side]) if isinstance(a, tuple) else a for a in args],
                                          flags | side, env._stream)
            assert rc == 0, (function, side, env.L.salp_robot_last_error())
        self.torch.cuda.synchronize()

    def check(self, what):
        for name, a, t in self.made:
            got = t.cpu().numpy()
            assert np.array_equal(a.view(np.uint8), got.view(np.uint8)), f"{what}: {name} differs between host and device pointers"
        self.made = []

    def close(self):
        self.host.close()
        self.dev.close()


def _actions(rng, n):
    return np.stack([rng.uniform(0, 1, n), rng.uniform(0, 0.3, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", [100, 321])
def test_host_pointers_equal_device_pointers(n):
    p = Pair(n)
    rng = np.random.default_rng(5)
    f32, u8, i32, f64 = np.float32, np.uint8, np.int32, np.float64
    obs = lambda: p.out("obs", (n, 6), f32)
    outputs = lambda: [obs(), p.out("reward", (n,), f32), p.out("terminated", (n,), u8), p.out("truncated", (n,), u8),
                       p.out("final_obs", (n, 6), f32), p.out("inner_steps", (n,), i32)]

    def final_obs_rows(o, what):
        """Rows of episodes that did not end hold the sentinel on both sides; returns the number that ended."""
        ended = (o[2][0] | o[3][0]).astype(bool)
        for side in (0, 1):
            fin = o[4][side] if side == 0 else o[4][side].cpu().numpy()
            assert np.all(fin[~ended].view(np.uint32) == 0xA5C3F00D), f"{what}: final_obs rows of running episodes were written"
            assert not np.any(fin[ended].view(np.uint32) == 0xA5C3F00D), f"{what}: final_obs rows of ended episodes were not written"
        return int(ended.sum())

    p.call("salp_robot_vec_reset", p.given((rng.uniform(size=n) < 0.5).astype(u8), "mask"), obs())
    p.check("reset(mask, obs)")
    p.call("salp_robot_vec_reset", None, obs())
    p.check("reset(NULL, obs)")
    p.call("salp_robot_vec_reset", p.given(np.zeros(n, u8), "mask"), obs())
    p.check("observe (all-zero mask)")

    finished = 0
    for t in range(3):       # every output; final_obs goes in as well as out
        o = outputs()
        p.call("salp_robot_vec_step", p.given(_actions(rng, n), "act"), *o)
        finished += final_obs_rows(o, f"step {t}")
        p.check(f"step {t}")
    assert finished > 0, "no episode ended: final_obs was never written"
    p.call("salp_robot_vec_step", p.given(_actions(rng, n), "act"), obs(), None, None, None, None, None)
    p.check("step(obs only)")
    o = outputs()
    p.call("salp_robot_vec_step", p.given(_actions(rng, n), "act"), None, *o[1:])
    p.check("step(obs = NULL)")

    begin, count, stride = 37, 50, 3
    cap = p.host.history_capacity(stride)
    for with_len in (True, False):
        o = outputs()
        hist = p.given(np.full((count, cap, H_COUNT), SENTINEL[np.dtype(f32)], f32), "history")
        p.made.pop()                                   # compared row by row below, each up to its own length
        hlen = p.out("history_len", (count,), i32) if with_len else None
        p.call("salp_robot_vec_step_history", p.given(_actions(rng, n), "act"), *o, begin, count, stride, cap, hist, hlen)
        L = (o[5][0][begin:begin + count] + stride - 1) // stride + 1          # samples of env begin + j: inner steps / stride + 1
        if with_len:
            assert np.array_equal(hlen[0], L), "history_len is not ceil(inner_steps / stride) + 1"
        hh, hd = hist[0], hist[1].cpu().numpy()
        for j in range(count):
            assert np.array_equal(hh[j, :L[j]].view(np.uint8), hd[j, :L[j]].view(np.uint8)), f"history row {j} differs between host and device pointers"
            assert not np.any(hh[j, :L[j], 0].view(np.uint32) == 0xA5C3F00D), f"history row {j} was not written up to its length"
        assert np.all(hh[:, L.max():].view(np.uint32) == 0xA5C3F00D), "the host history was written past the longest record"
        final_obs_rows(o, "step_history")
        p.check(f"step_history(history_len {'given' if with_len else 'NULL'})")

    T = 3
    shared = rng.uniform([0, 0, -1], [1, 0.3, 1], (T, 3)) * SCALE
    p.call("salp_robot_vec_trajectory", None, p.given(shared, "actions"), T, p.given(rng.normal(0, 0.1, (T, 6)), "expected"),
           p.out("states", (T, n, 6), f64), p.out("metrics", (n, 5), f64), p.out("inner_steps", (T, n), i32))
    p.check("trajectory(shared actions, expected, states, metrics, inner_steps)")
    table = robot_params(n, "cpu").numpy() * rng.uniform(0.9, 1.1, (12, n))
    per = rng.uniform([0, 0, -1], [1, 0.3, 1], (T, n, 3)) * SCALE
    p.call("salp_robot_vec_trajectory", p.given(table, "params"), p.given(per, "actions"), T, None,
           p.out("states", (T, n, 6), f64), None, None, flags=PER_ROBOT_ACTIONS)
    p.check("trajectory(per-robot actions, parameter table, states)")

    # get_state: the host-pointer form into the arrays and the device-pointer form into the tensors, on each handle
    snaps = [p.out("state", (R_COUNT, n), f64) for _ in range(2)]
    for env, (a, t) in zip((p.host, p.dev), snaps):
        assert env.L.salp_robot_vec_get_state(env._h, SalpLib._ptr(a), 0, None) == 0
        assert env.L.salp_robot_vec_get_state(env._h, SalpLib._ptr(t), 1, p.dev._stream) == 0
    p.torch.cuda.synchronize()
    p.check("get_state with host and with device pointers")
    assert np.array_equal(snaps[0][0].view(np.uint8), snaps[1][0].view(np.uint8)), "the final states of the two handles differ"
    assert not np.any(snaps[0][0] == SENTINEL[np.dtype(f64)])
    p.close()
