"""The per-env summary record of salp_vec_evaluate_policy on the CPU: `policy.summarize_rollout` (the numpy statement of
the record that tests/test_gpu_policy_evaluate.py compares the kernel with) on hand-made arrays, the guard of the GPU
cases (on the oracle's closed-loop runs of tests/policy_cases.py every case must end episodes both ways, more than once,
capture food and have first episode ends on both sides of the accumulation cut), and the header against `_capi`."""
import os
import re

import numpy as np
import pytest

import evaluate_cases as ec
import policy_cases as cases
from underwater_swimmer_rl_amd import _capi, policy
from underwater_swimmer_rl_amd.policy import evaluation_views, summarize_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_made():
    """Six steps, five envs: 0 finishes at step 0 (terminated); 1 never finishes; 2 is terminated AND truncated in step 2;
    3 is truncated in step 1 and terminated in step 4 (a second episode); 4 never finishes and has rewards whose float32
    running sum loses what the float64 one keeps."""
    H, N = 6, 5
    rew = np.array([[1.5, -0.1, -0.1, -0.1, 1e8],
                    [-0.1, -0.1, -0.1, 2.25, 1.0],
                    [-0.1, -0.1, -50.0, -0.1, 1.0],
                    [10.0, -0.1, -0.1, -0.1, 1.0],
                    [-0.1, -0.1, -0.1, -50.0, -1e8],
                    [-0.1, 0.9, -0.1, -0.1, 0.1]], np.float32)
    term, trunc, cap = np.zeros((H, N), np.uint8), np.zeros((H, N), np.uint8), np.zeros((H, N), bool)
    term[0, 0] = 1
    term[2, 2] = trunc[2, 2] = 1
    trunc[1, 3] = 1
    term[4, 3] = 1
    cap[3, 0] = cap[5, 1] = cap[1, 3] = True
    return rew, term, trunc, cap


def _seq64(column, upto=None):
    acc = 0.0
    for r in column[:upto]:
        acc += float(r)               # float(np.float32) is exact; Python adds in float64
    return acc


def test_summarize_rollout_on_hand_made_arrays():
    rew, term, trunc, cap = _hand_made()
    rec = summarize_rollout(rew, term, trunc, cap)
    assert rec.dtype == np.int32 and rec.shape == (5, 8)
    v = evaluation_views(rec)
    assert v["return_sum"].dtype == np.float64 and v["first_return"].dtype == np.float64 and v["food"].dtype == np.int32
    assert v["first_length"].tolist() == [1, 6, 3, 2, 6]
    assert v["first_end"].tolist() == [1, 0, 1, 2, 0]          # env 2: terminated wins over truncated
    assert v["episodes"].tolist() == [1, 0, 1, 2, 0]
    assert v["food"].tolist() == [1, 1, 0, 1, 0]
    for i in range(5):
        assert v["return_sum"][i] == _seq64(rew[:, i])
        assert v["first_return"][i] == _seq64(rew[:, i], int(v["first_length"][i]))
    assert v["first_return"][0] == 1.5 and v["first_return"][1] == v["return_sum"][1]
    # env 4: the float32 running sum drops the three 1.0 behind 1e8, the float64 sum of the float32 values keeps them
    acc32 = np.float32(0)
    for r in rew[:, 4]:
        acc32 = np.float32(acc32 + r)
    assert float(acc32) == float(np.float32(0.1)) and v["return_sum"][4] == 3.0 + float(np.float32(0.1))
    assert v["return_sum"][4] != float(acc32)
    # the views alias the block
    assert np.shares_memory(v["return_sum"], rec) and v["record"] is rec


@pytest.mark.parametrize("cut", [1, 2, 3, 5])
def test_accumulation_over_a_split_equals_one_pass(cut):
    rew, term, trunc, cap = _hand_made()
    whole = summarize_rollout(rew, term, trunc, cap)
    first = summarize_rollout(rew[:cut], term[:cut], trunc[:cut], cap[:cut])
    kept = first.copy()
    both = summarize_rollout(rew[cut:], term[cut:], trunc[cut:], cap[cut:], record=first)
    assert np.array_equal(both, whole) and np.array_equal(first, kept)      # bit for bit; the input record is not modified
    # an all-zero record is a fresh one
    assert np.array_equal(summarize_rollout(rew, term, trunc, cap, record=np.zeros((5, 8), np.int32)), whole)
    # without the capture flags the food count stays where it was
    assert (evaluation_views(summarize_rollout(rew, term, trunc))["food"] == 0).all()


def test_argument_checks():
    rew, term, trunc, cap = _hand_made()
    with pytest.raises(ValueError):
        summarize_rollout(rew.astype(np.float64), term, trunc)
    with pytest.raises(ValueError):
        evaluation_views(np.zeros((5, 8), np.int64))
    with pytest.raises(ValueError):
        evaluation_views(np.zeros((5, 7), np.int32))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_closed_loop_cases_exercise_every_field_on_the_oracle(name):
    cfg, pol, f64, i32, obs_in, actions, outs = cases.oracle_closed_loop(name)
    cap = ec.captures_from_info(outs["info"], outs["terminated"], outs["truncated"], start_count=i32[_capi.I_FOOD_COLLECTED])
    rec = summarize_rollout(np.zeros(outs["terminated"].shape, np.float32), outs["terminated"], outs["truncated"], cap)
    ec.assert_not_vacuous(name, rec)
    v = evaluation_views(rec)
    done = (outs["terminated"] | outs["truncated"]).astype(bool)
    assert np.array_equal(v["episodes"], done.sum(0)) and int(v["food"].sum()) == int(cap.sum())
    assert np.array_equal(v["first_length"], np.where(done.any(0), done.argmax(0) + 1, cases.H))


def _enum_values(text):
    """name -> value of every enumerator of the header's anonymous / named enums (comments stripped; `= N` or the one before + 1)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    values = {}
    for body in re.findall(r"enum\s*\w*\s*\{(.*?)\}", text, flags=re.S):
        nxt = 0
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            m = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\w+))?", item)
            assert m, item
            if m.group(2) is not None:
                tok = m.group(2).rstrip("uU")
                nxt = int(tok, 0) if re.fullmatch(r"-?(0x)?[0-9a-fA-F]+", tok) else values[tok]
            values[m.group(1)] = nxt
            nxt += 1
    return values


def test_header_declares_the_entry_point_and_capi_holds_its_values():
    with open(os.path.join(ROOT, "include", "salp_vec.h")) as f:
        text = f.read()
    assert re.search(r"int\s+salp_vec_evaluate_policy\(salp_vec_t\*\s*h,\s*const salp_policy_t\*\s*pol,\s*int32_t\s+horizon,\s*void\*\s*rec,"
                     r"\s*uint32_t\s+flags,\s*void\*\s*stream\);", text)
    e = _enum_values(text)
    assert e["SALP_DEVICE_PTRS"] == 1 and e["SALP_REC_FINAL_OBS"] == 2        # the parser reads the enums it knows
    want = dict(SALP_EVAL_ACCUMULATE=4, SALP_EVAL_RETURN=0, SALP_EVAL_FIRST_RETURN=2, SALP_EVAL_FIRST_LENGTH=4, SALP_EVAL_FIRST_END=5,
                SALP_EVAL_EPISODES=6, SALP_EVAL_FOOD=7, SALP_EVAL_WORDS=8)
    for k, val in want.items():
        assert e[k] == val, k
        assert getattr(_capi, k[len("SALP_"):]) == val, k
        if k != "SALP_EVAL_ACCUMULATE":
            assert getattr(policy, k[len("SALP_"):]) == val, k
    assert "salp_vec_evaluate_policy" in _capi.EXPORTS
    assert _capi.EVAL_ACCUMULATE & (_capi.SALP_DEVICE_PTRS | _capi.REC_FINAL_OBS) == 0
