"""The robot rollout calls (salp_robot_vec_rollout, salp_robot_vec_rollout_policy) — the parts that need no GPU:
what check_rollout_args() of csrc/salp_robot_params.h refuses, the iteration bound of the kernel's loop, and the device
block of a 6 -> 3 policy through the host layout functions of csrc/salp_policy.h, which salp_robot.hip calls with these
dimensions (tests/robot_rollout_host_lib.py, tests/policy_host_lib.py)."""
import numpy as np
import pytest

import policy_host_lib as ph
import robot_rollout_host_lib as rr

INVALID = -1                    # SALP_ERR_INVALID (include/salp_vec.h)
STEPS = 1461                    # robot_max_steps(0.01)
SHAPES = ((), (16,), (64,), (32, 16), (16, 48), (64, 64))


def test_constants():
    assert rr.max_cycles() == 1024
    assert rr.max_steps(0.01) == STEPS
    periods, shipped = rr.periods()
    assert periods == (0, 32, 128, 512) and shipped in periods
    assert all(m == 0 or (m & (m - 1)) == 0 for m in periods)       # the kernel tests iter & (M - 1)


def test_accepted_calls():
    for H in (1, 7, 1024):
        assert rr.check_rollout(STEPS, H) == (0, "")
        assert rr.check_rollout(STEPS, H, flags=1) == (0, "")


@pytest.mark.parametrize("kwargs, text", [
    (dict(horizon=0), "horizon must be in [1, 1024]"),
    (dict(horizon=-3), "horizon must be in [1, 1024]"),
    (dict(horizon=1025), "horizon must be in [1, 1024]"),
    (dict(horizon=4, flags=2), "unknown flag bits"),
    (dict(horizon=4, flags=0x80000001), "unknown flag bits"),
    (dict(horizon=4, source=False), "act / policy is NULL"),
    (dict(horizon=4, main_output=False), "one of obs, reward, terminated, truncated is required"),
    (dict(horizon=4, max_steps=-1), "dt is too small (more than 2^24 Euler steps per cycle)"),
])
def test_refusals(kwargs, text):
    assert rr.check_rollout(**{"max_steps": STEPS, **kwargs}) == (INVALID, text)


def test_a_short_message_buffer_is_not_overrun():
    rc, msg = rr.check_rollout(STEPS, 0, msg_size=8)
    assert rc == INVALID and msg == "horizon"


@pytest.mark.parametrize("period", [0, 32, 128, 512])
def test_the_iteration_bound_covers_the_longest_run(period):
    """A lane's cycle runs at most max_steps Euler iterations and waits at most `period` iterations for its service point
    (period 0: a round of the wavefront lasts at most max_steps iterations); the kernel counts one iteration per Euler step
    and at least one per round.  The bound must exceed H cycles of that plus the closing service point, and stay far from
    overflow at the largest horizon and the smallest dt the calls accept."""
    for H in (1, 7, 1024):
        worst = H * (STEPS + period + 1) + period + 1
        assert worst <= rr.max_iters(H, STEPS, period) <= 2 * worst
    assert rr.max_iters(1024, 1 << 24, 512) < 1 << 40


# ---- the device block of a 6 -> 3 policy (obs_dim 6, act_dim 3, kmax 3 as salp_robot.hip passes them)
@pytest.mark.parametrize("hidden", SHAPES, ids=lambda h: "x".join(map(str, h)) or "linear")
def test_the_block_holds_every_public_word_exactly_once(hidden):
    d = ph.desc_of(hidden, out=1)
    rc, words, why = ph.check(d, obs_dim=6, act_dim=3, kmax=3, n_envs=357)
    assert rc == 0, why
    widths = (6,) + tuple(hidden) + (3,)
    assert words == sum(widths[k + 1] * (widths[k] + 1) for k in range(len(widths) - 1)) + 2 * 3
    m = ph.block_map(d, obs_dim=6, act_dim=3)
    assert len(m) % 16 == 0
    used = m[m >= 0]
    assert np.array_equal(np.sort(used), np.arange(words)), "a public word is missing from the block or held twice"
    # what policy_eval_impl<6, 3> of csrc/salp_policy.h reads: per hidden chunk of the first layer 16 biases, then 16 weights per input
    off = 0
    if hidden:
        h0, Wp, bp = hidden[0], 0, hidden[0] * 6
        for c in range(h0 // 16):
            assert np.array_equal(m[off:off + 16], bp + 16 * c + np.arange(16))
            for i in range(6):
                assert np.array_equal(m[off + 16 * (1 + i):off + 16 * (2 + i)], Wp + (16 * c + np.arange(16)) * 6 + i)
            off += 16 * 7
    if len(hidden) == 2:
        off += (hidden[1] // 16) * 16 * (hidden[0] + 1)
    # the tail: b_last[3], scale[3], shift[3] in the first nine words of one 16-word group, the rest zero
    last_in = widths[-2]
    pub_last = words - 6 - 3 - 3 * last_in
    tail = m[off:off + 16]
    assert np.array_equal(tail[:3], pub_last + 3 * last_in + np.arange(3))            # b_last
    assert np.array_equal(tail[3:9], words - 6 + np.arange(6)) and np.all(tail[9:] == -1)
    # the last layer: one row per action, padded to a multiple of 16 words
    rs = (last_in + 15) // 16 * 16
    assert len(m) == off + 16 + 3 * rs
    for a in range(3):
        row = m[off + 16 + a * rs:off + 16 + (a + 1) * rs]
        assert np.array_equal(row[:last_in], pub_last + a * last_in + np.arange(last_in)) and np.all(row[last_in:] == -1)


def test_populations_need_whole_wavefronts():
    d = ph.desc_of((16,), out=1, P=2)
    assert ph.check(d, obs_dim=6, act_dim=3, kmax=3, n_envs=256)[0] == 0
    for n in (357, 192, 255):                  # odd, 96 per policy, odd
        rc, _, why = ph.check(d, obs_dim=6, act_dim=3, kmax=3, n_envs=n)
        assert rc == INVALID and "n_policies > 1" in why
    hd = ph.header(d, len(ph.block_map(d, obs_dim=6, act_dim=3)), 256)
    s = ph.header_slots()
    assert hd[s["GROUP"]] == 128 and hd[s["COUNT"]] == 2 and hd[s["STRIDE"]] == len(ph.block_map(d, obs_dim=6, act_dim=3))
