"""`policy.summarize_robot_rollout` and `policy.robot_evaluation_views` on hand-made arrays: the numpy statement of the
record salp_robot_vec_evaluate_policy leaves (include/salp_robot_evaluate.h), which tests/test_gpu_robot_evaluate.py holds
the kernel to.  No GPU needed."""
import numpy as np
import pytest

from underwater_swimmer_rl_amd.policy import (REVAL_FIRST_END, REVAL_WORDS, robot_evaluation_views, summarize_robot_rollout)


def flags(rows):
    return np.array(rows, np.uint8)


def test_the_sum_is_sequential_float64_not_float32():
    """1 + 2^-30 + 2^-30 ...: every float32 partial sum stays 1, the float64 sum does not; and a column whose float64 sum
    depends on the order (2^60, 1, -2^60) is added in step order."""
    small = np.float32(2.0 ** -30)
    reward = np.array([[1.0, 2.0 ** 60], [small, 1.0], [small, -(2.0 ** 60)], [small, 0.0]], np.float32)
    zeros = np.zeros((4, 2), np.uint8)
    v = robot_evaluation_views(summarize_robot_rollout(reward, zeros, zeros, np.full((4, 2), 5, np.int32)))
    acc32 = np.float32(0)
    for x in reward[:, 0]:
        acc32 = np.float32(acc32 + x)
    assert float(acc32) == 1.0 and v["return_sum"][0] == 1.0 + 3 * 2.0 ** -30 != float(acc32)
    assert v["return_sum"][1] == 0.0, "(2^60 + 1) - 2^60 in step order is 0 in float64; any other order gives 1"
    assert np.array_equal(v["first_return"], v["return_sum"]) and np.array_equal(v["euler_steps"], [20, 20])
    assert np.array_equal(v["first_length"], [4, 4]) and not v["first_end"].any() and not v["episodes"].any()
    with pytest.raises(ValueError):
        summarize_robot_rollout(reward.astype(np.float64), zeros, zeros, zeros)


def test_terminated_wins_and_first_fields_freeze():
    reward = np.array([[1, 1, 1], [2, 2, 2], [4, 4, 4], [8, 8, 8]], np.float32)
    term = flags([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 1, 0]])
    trunc = flags([[0, 0, 0], [1, 1, 0], [0, 0, 0], [0, 1, 0]])
    inner = np.array([[10, 10, 10], [20, 20, 20], [30, 30, 30], [40, 40, 40]], np.int32)
    v = robot_evaluation_views(summarize_robot_rollout(reward, term, trunc, inner))
    assert np.array_equal(v["first_end"], [1, 2, 0]), "both flags on one step: terminated wins"
    assert np.array_equal(v["first_length"], [2, 2, 4]) and np.array_equal(v["first_return"], [3.0, 3.0, 15.0])
    assert np.array_equal(v["first_euler_steps"], [30, 30, 100])
    assert np.array_equal(v["return_sum"], [15.0, 15.0, 15.0]) and np.array_equal(v["euler_steps"], [100, 100, 100])
    assert np.array_equal(v["episodes"], [2, 2, 0]) and np.array_equal(v["reached"], [2, 1, 0])
    assert v["euler_steps"].dtype == np.int64 and v["return_sum"].dtype == np.float64 and v["first_end"].dtype == np.int32
    assert not v["record"][:, REVAL_WORDS - 1].any()


def test_three_plus_four_steps_continue_to_seven_bit_for_bit():
    rng = np.random.default_rng(3)
    H, N = 7, 40
    reward = (rng.normal(size=(H, N)) * 10.0 ** rng.integers(-6, 6, (H, N))).astype(np.float32)
    term = (rng.random((H, N)) < 0.15).astype(np.uint8)
    trunc = (rng.random((H, N)) < 0.15).astype(np.uint8)
    inner = rng.integers(0, 1461, (H, N)).astype(np.int32)
    for first_episode in (False, True):
        whole = summarize_robot_rollout(reward, term, trunc, inner, first_episode=first_episode)
        part = summarize_robot_rollout(reward[:3], term[:3], trunc[:3], inner[:3], first_episode=first_episode)
        kept = part.copy()
        both = summarize_robot_rollout(reward[3:], term[3:], trunc[3:], inner[3:], record=part, first_episode=first_episode)
        assert np.array_equal(part, kept), "`record` is not modified"
        assert both.tobytes() == whole.tobytes()
    fresh = summarize_robot_rollout(reward, term, trunc, inner, record=np.zeros((N, REVAL_WORDS), np.int32))
    assert fresh.tobytes() == summarize_robot_rollout(reward, term, trunc, inner).tobytes(), "an all-zero record is a fresh one"
    # the float64 sums are those of a host loop over the float32 values
    v = robot_evaluation_views(whole)
    for i in range(N):
        acc, n = 0.0, 0
        for t in range(H):
            acc += float(reward[t, i])
            n += int(inner[t, i])
            if term[t, i] or trunc[t, i]:
                break
        assert v["return_sum"][i] == acc and v["euler_steps"][i] == n


def test_first_episode_ignores_the_steps_after_the_first_ending():
    rng = np.random.default_rng(4)
    H, N = 9, 64
    reward = rng.normal(size=(H, N)).astype(np.float32)
    term = (rng.random((H, N)) < 0.1).astype(np.uint8)
    trunc = (rng.random((H, N)) < 0.1).astype(np.uint8)
    inner = rng.integers(0, 1461, (H, N)).astype(np.int32)
    full = robot_evaluation_views(summarize_robot_rollout(reward, term, trunc, inner))
    v = robot_evaluation_views(summarize_robot_rollout(reward, term, trunc, inner, first_episode=True))
    assert (v["first_end"] != 0).any() and (v["first_end"] == 0).any() and (full["episodes"] > 1).any()
    assert np.array_equal(v["return_sum"].view(np.int64), v["first_return"].view(np.int64))
    assert np.array_equal(v["euler_steps"], v["first_euler_steps"])
    assert np.array_equal(v["episodes"], (v["first_end"] != 0).astype(np.int32))
    assert np.array_equal(v["reached"], (v["first_end"] == 1).astype(np.int32))
    for k in ("first_return", "first_length", "first_end", "first_euler_steps"):
        assert np.array_equal(v[k], full[k]), k
    # a record that arrives finished is returned unchanged
    done = v["record"][v["first_end"] != 0]
    again = summarize_robot_rollout(reward[:, :len(done)], term[:, :len(done)], trunc[:, :len(done)], inner[:, :len(done)],
                                    record=done, first_episode=True)
    assert again.tobytes() == done.tobytes()


def test_views_alias_the_block_and_refuse_other_blocks():
    rec = np.zeros((5, REVAL_WORDS), np.int32)
    v = robot_evaluation_views(rec)
    assert v["record"] is rec
    v["return_sum"][2] = 1.5
    v["euler_steps"][3] = (1 << 40) + 7
    v["first_end"][4] = 2
    assert rec[2, :2].view(np.float64)[0] == 1.5 and rec[3, 4:6].view(np.int64)[0] == (1 << 40) + 7 and rec[4, REVAL_FIRST_END] == 2
    assert all(np.shares_memory(x, rec) for x in v.values())
    assert set(v) == {"record", "return_sum", "first_return", "euler_steps", "first_length", "first_end", "episodes", "reached",
                      "first_euler_steps"}
    for bad in (np.zeros((5, 8), np.int32), np.zeros((5, REVAL_WORDS), np.int64), np.zeros((5, REVAL_WORDS), np.float32),
                np.zeros(5 * REVAL_WORDS, np.int32), np.zeros((5, 2 * REVAL_WORDS), np.int32)[:, ::2],
                np.zeros((REVAL_WORDS, 5), np.int32).T):
        with pytest.raises(ValueError):
            robot_evaluation_views(bad)
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, REVAL_WORDS), dtype=torch.int32)
    tv = robot_evaluation_views(t)
    tv["first_return"][1] = 2.5
    assert t[1, 2:4].numpy().view(np.float64)[0] == 2.5 and tv["euler_steps"].dtype == torch.int64
    with pytest.raises(ValueError):
        robot_evaluation_views(torch.zeros((3, 8), dtype=torch.int32))
