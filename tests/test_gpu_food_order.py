"""GPU food-ordering tests: every selection network of csrc/salp_food_reg.h and the packed-key pass of salp_food_lds.h
against the CPU oracle on the tied food sets of tests/food_order_cases.py — near ties at every rank up to K / K + 1 in
every ordered pair of slots, exact ties of two to four foods, squared distances one ulp apart that share a distance,
ties next to empty slots, in mixed wavefronts.  The expected order is the reference's stable fp64 sort (the oracle; its
numpy model and the counts of what each case exercises are pinned on the CPU by tests/test_food_order_recipe.py).

Three device paths see each state: salp_vec_observe (the reset / observe kernel's serial fp64 sort), two salp_vec_step
calls with final_obs and info, and a fused rollout of 16 zero-action steps (the resting swimmers' order cache).  A swapped
pair moves an observation column by >= 1e-2 and, with K = 0, the reward by >= 1e-2: a thousand times the tolerances."""
import numpy as np
import pytest

import food_order_cases as fc
from gpu_support import OBS_TOL, REW_TOL, assert_parity, assert_state_parity, run_device, started
from support import obs_diff

pytestmark = pytest.mark.gpu


def first_bad_env(cfg, got, ref):
    """The first env whose observation or reward is outside the tolerances in a [..., n] block pair, or None."""
    d = obs_diff(cfg, got["obs"], ref["obs"]).max(axis=-1)
    rd = np.abs(got["reward"].astype(np.float64) - ref["reward64"]) / np.maximum(1.0, np.abs(ref["reward64"]))
    bad = ~(d <= OBS_TOL) | ~(rd <= REW_TOL)
    bad = bad.reshape(-1, bad.shape[-1]).any(axis=0)
    return int(np.argmax(bad)) if bad.any() else None


def compare(name, cfg, meta, got, ref, what):
    """assert_parity with the project's tolerances; a failure names the case, family, rank and slots of the first bad env."""
    try:
        return assert_parity(cfg, got, ref, f"{name}: {what}")
    except AssertionError as err:
        i = first_bad_env(cfg, got, ref)
        raise AssertionError(f"{err}; first bad env: {fc.describe_env(name, meta, i) if i is not None else 'flags only'}") from None


@pytest.mark.parametrize("name", list(fc.CASES))
def test_tied_food_order_matches_oracle(name):
    cfg, orc, f64, i32, meta = fc.start_oracle(name, threads=4)
    n, kernel = fc.N_ENVS, fc.CASES[name][1]
    dev = started(cfg, n, f64, i32, seed=fc.ENV_SEED)
    # observe(): the reset / observe kernel
    obs = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs, 0)
    zero = np.zeros(n)
    compare(name, cfg, meta, dict(obs=obs, reward=zero.astype(np.float32), terminated=zero, truncated=zero),
            dict(obs=orc.observe(), reward64=zero, terminated=zero, truncated=zero), "observe()")
    # two acting steps with every output
    act = np.zeros((fc.STEP_CALLS + fc.ROLLOUT_STEPS, n, cfg.act_dim), np.float32)
    S = fc.STEP_CALLS
    ref = orc.rollout(act[:S], want_final=True)
    got = dict(obs=np.empty((S, n, cfg.obs_dim), np.float32), reward=np.empty((S, n), np.float32),
               terminated=np.empty((S, n), np.uint8), truncated=np.empty((S, n), np.uint8))
    fin = np.full((S, n, cfg.obs_dim), np.nan, np.float32)
    info = np.empty((S, n, 3), np.int32)
    for t in range(S):
        dev.step(act[t], got["obs"][t], got["reward"][t], got["terminated"][t], got["truncated"][t], fin[t], info[t], 0)
        ll = dev.last_launch()
        assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == kernel, (name, ll)
    dmax, rmax = compare(name, cfg, meta, got, ref, "salp_vec_step")
    assert np.array_equal(info, ref["info"]), f"{name}: info differs"
    assert not ref["terminated"].any() and not ref["truncated"].any() and np.isnan(fin).all(), f"{name}: an episode ended"
    # the fused rollout
    got, _ = run_device(cfg, n, act[S:], dev=dev)
    ref = orc.rollout(act[S:])
    d2, r2 = compare(name, cfg, meta, got, ref, "fused rollout")
    ll = dev.last_launch()
    assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == kernel, (name, ll)
    assert ll["envs_unpredicated"] == n and ll["envs_predicated"] == 0
    assert_state_parity(cfg, dev, orc, name)
    print(f"{name}: kernel {kernel}, max obs diff {max(dmax, d2):.3g}, max rel reward diff {max(rmax, r2):.3g}, "
          f"families {np.bincount(meta['family'], minlength=4).tolist()}")
    dev.close()
    orc.close()
