"""The shared test helpers (tests/support.py, tests/gpu_support.py, the closed-loop driver of tests/policy_cases.py) held to
what the GPU suite relies on.  No GPU: importing gpu_support binds `_capi` without loading the library."""
from types import SimpleNamespace

import numpy as np
import pytest

import golden_util
import parity_cases as pc
import policy_cases
import sampled_cases
import support
from gpu_support import OBS_TOL, REW_TOL, STATE_TOL, assert_state_parity
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.policy import EVAL_FIRST_LENGTH, EVAL_WORDS, evaluation_views

CFG = SimpleNamespace(max_observed_food=3, num_food_items=2)      # angle columns 4, 13, 17, 21 of 24


def test_tolerances_keep_their_values():
    assert (OBS_TOL, REW_TOL, STATE_TOL) == (1e-5, 1e-5, 1e-9)


def test_obs_diff_wraps_angle_columns_only():
    assert support.angle_cols(CFG) == [4, 13, 17, 21]
    a, b = np.zeros((2, 24), np.float32), np.zeros((2, 24), np.float32)
    a[0, 4], b[0, 4] = 0.999, -0.999          # an angle column: the same heading but for 0.002
    a[1, 5], b[1, 5] = 0.999, -0.999          # any other column: far apart
    d = support.obs_diff(CFG, a, b)
    assert d[0, 4] == pytest.approx(0.002, abs=1e-6) and d[1, 5] == pytest.approx(1.998, abs=1e-6)
    assert np.count_nonzero(d) == 2


def test_obs_diff_is_strict_about_nan_and_golden_util_is_not():
    a, b = np.zeros((2, 24), np.float32), np.zeros((2, 24), np.float32)
    a[1, 7] = np.nan
    d = support.obs_diff(CFG, a, b)
    assert np.isnan(d[1, 7]) and np.isnan(d.max()) and not d.max() <= OBS_TOL
    assert golden_util.obs_diff(CFG, a, b).max() == 0.0      # the fixtures' NaN rows count as equal there, on purpose


def _state(n=4):
    f64 = np.arange((_capi.F_FOOD0 + 2 * CFG.num_food_items) * n, dtype=np.float64).reshape(-1, n)
    f64[_capi.F_FOOD0, 1] = f64[_capi.F_FOOD0 + CFG.num_food_items, 1] = np.nan       # env 1: its first food is gone
    return f64, np.arange(_capi.I_COUNT * n, dtype=np.int32).reshape(-1, n)


def test_same_state():
    f64, i32 = _state()
    assert support.same_state((f64, i32), (f64.copy(), i32.copy()))
    g = f64.copy()
    g[2, 3] = np.nextafter(g[2, 3], np.inf)
    assert not support.same_state((f64, i32), (g, i32))
    j = i32.copy()
    j[5, 0] += 1
    assert not support.same_state((f64, i32), (f64, j))


def test_bits_of_a_strided_view():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = support.bits(a[:, ::2])
    assert b.dtype == np.uint32 and b.shape == (3, 2) and np.array_equal(b, a.view(np.uint32)[:, ::2])
    assert support.bits(np.float32([-0.0]))[0] == 0x80000000 != support.bits(np.float32([0.0]))[0]


def test_fields_diff_names_the_field_and_the_env():
    fields = ("return_sum", "first_return", "first_length", "first_end", "episodes", "food")
    rec = np.arange(4 * EVAL_WORDS, dtype=np.int32).reshape(4, EVAL_WORDS)
    assert support.fields_diff(rec, rec.copy(), evaluation_views, fields) == ""
    other = rec.copy()
    other[2, EVAL_FIRST_LENGTH] += 5
    assert support.fields_diff(rec, other, evaluation_views, fields) == \
        f"first_length: 1 envs, first env 2: {rec[2, EVAL_FIRST_LENGTH]!r} != {other[2, EVAL_FIRST_LENGTH]!r}"


class _Dev:
    """What assert_state_parity needs of a handle: n_envs and a get_state that fills the caller's arrays."""

    def __init__(self, f64, i32):
        self.f64, self.i32, self.n_envs = f64, i32, f64.shape[1]

    def get_state(self, f64, i32, stream):
        f64[:], i32[:] = self.f64, self.i32


def test_assert_state_parity():
    f64, i32 = _state()
    dev = _Dev(f64, i32)
    assert_state_parity(CFG, dev, (f64.copy(), i32.copy()))
    assert_state_parity(CFG, dev, SimpleNamespace(get_state=lambda: (f64.copy(), i32.copy())), "an oracle")
    nan_moved = f64.copy()
    nan_moved[_capi.F_FOOD0, 1], nan_moved[_capi.F_FOOD0, 2] = 0.0, np.nan
    with pytest.raises(AssertionError, match="None-pattern"):
        assert_state_parity(CFG, dev, (nan_moved, i32))
    j = i32.copy()
    j[3, 2] += 1
    with pytest.raises(AssertionError, match=r"integer state differs in rows \[3\]"):
        assert_state_parity(CFG, dev, (f64, j))
    off = f64.copy()
    off[0, 1] += 2e-9           # row 0 holds 0 .. 3: the sum is exact to 2^-52
    with pytest.raises(AssertionError, match="fp64 state diff"):
        assert_state_parity(CFG, dev, (off, i32))
    off[0, 1] = f64[0, 1] + 5e-10
    assert_state_parity(CFG, dev, (off, i32))
    assert 5e-10 < STATE_TOL < 2e-9


@pytest.mark.parametrize("cases", [policy_cases, sampled_cases], ids=["deterministic", "sampled"])
def test_closed_loop_runs_feed_each_row_to_the_next_action(cases):
    r = cases.oracle_closed_loop("one_food_mlp32")
    obs_in, actions, outs = r[4:7] if cases is policy_cases else (r[5], r[6], r[8])
    assert obs_in.shape == outs["obs"].shape and actions.shape[:2] == obs_in.shape[:2] and actions.dtype == np.float32
    assert np.array_equal(support.bits(obs_in[1:]), support.bits(outs["obs"][:-1]))
    assert not any(a.flags.writeable for a in (obs_in, actions, *outs.values()))


def test_drive_oracle_on_two_envs():
    cfg = policy_cases.case_cfg("one_food_mlp32")
    orc = pc.ol.OracleVec(cfg, 2, seed=pc.ENV_SEED)
    first = orc.observe()
    obs_in, actions, outs, kept = policy_cases.drive_oracle(orc, 5, lambda t, o: (np.full((2, cfg.act_dim), 0.1 * t, np.float32), t))
    orc.close()
    assert kept == [0, 1, 2, 3, 4] and np.array_equal(actions[:, 0, 0], np.float32(0.1) * np.arange(5, dtype=np.float32))
    assert np.array_equal(support.bits(obs_in[0]), support.bits(first))
    assert np.array_equal(support.bits(obs_in[1:]), support.bits(outs["obs"][:-1]))
    assert set(outs) == {"obs", "terminated", "truncated", "info"} and outs["info"].shape == (5, 2, 3)
