"""CPU guard of the GPU food-ordering tests' recipe (tests/food_order_cases.py), in the manner of test_parity_recipe.py: the
oracle and the numpy model of the reference's order pin each other over the shared case table, the generated geometry
holds through the run the GPU tests make, and what each case exercises — envs the fp32 keys alone would mis-order, envs
inside the kernel's tolerance, gaps on both sides of it, shared distances, every slot arrangement — is counted ON THE
MODELS and held above committed floors at every tie rank, so that editing a seed or the recipe on a machine without a GPU
cannot quietly take the ties away."""
import numpy as np
import pytest

import food_order_cases as fc
import oracle_lib as ol
from support import obs_diff

MODEL_TOL = 1e-6      # numpy against libm in fp64, both rounded to float32; a swapped pair moves a column by >= 1e-2


@pytest.mark.parametrize("name", list(fc.CASES))
def test_recipe_ties_foods_on_the_oracle(name):
    cfg, orc, f64, i32, meta = fc.start_oracle(name)
    n, F, K, R = fc.N_ENVS, cfg.num_food_items, int(cfg.max_observed_food), fc.tie_ranks(cfg)
    # the numpy model of the reference's order predicts the oracle's food columns and padding in every env
    obs = orc.observe()
    want = np.concatenate([obs[:, :10], fc.predicted_food_columns(f64, cfg)], axis=1)
    d = obs_diff(cfg, obs, want)
    bad = int(np.argmax(d.max(axis=1)))
    assert d.max() <= MODEL_TOL, f"oracle and numpy model differ by {d.max()}: {fc.describe_env(name, meta, bad)}"
    order = fc.reference_order(f64, cfg)
    shown_live = np.minimum(meta["live"], K)
    padded = obs[:, 10: 10 + 4 * K].reshape(n, K, 4)
    is_pad = (padded == np.array([0.0, 0.0, 1.0, 0.0], np.float32)).all(axis=2)
    assert np.array_equal(is_pad, np.arange(K)[None, :] >= shown_live[:, None]), "padding does not follow the live count"
    assert np.array_equal((order >= 0).sum(axis=1), meta["live"])
    # the geometry holds through the GPU tests' run: nothing moves, nothing ends, nothing is captured
    H = fc.STEP_CALLS + fc.ROLLOUT_STEPS
    ref = orc.rollout(np.zeros((H, n, cfg.act_dim), np.float32), want_final=True)
    after, i_after = orc.get_state()
    assert np.array_equal(after[ol.F_X], f64[ol.F_X]) and np.array_equal(after[ol.F_Y], f64[ol.F_Y]), "a swimmer moved"
    assert np.array_equal(after[ol.F_FOOD0:], f64[ol.F_FOOD0:], equal_nan=True), "a food changed"
    assert not ref["terminated"].any() and not ref["truncated"].any()
    assert np.array_equal(i_after[ol.I_STEPS_SINCE_FOOD], np.full(n, H)) and np.isnan(ref["final_obs"]).all()
    same = ref["obs"].copy()         # the breathing columns go on; the food columns stay what the model predicts
    same[:, :, 10:] = want[None, :, 10:]
    dd = obs_diff(cfg, ref["obs"], same)
    assert dd.max() <= MODEL_TOL, "the food columns change during the run"
    # what the case exercises, from the models; never from a device
    ev = fc.exercise_counts(f64, cfg, meta)
    fam = np.bincount(meta["family"], minlength=4).tolist()
    print(f"{name}: {ev}, families {dict(zip(fc.FAMILIES, fam))}, shared-distance draws moved to near ties {meta['shared_moved']}, "
          f"near-tie arrangements {len(fc.arrangements(meta))}, live counts {sorted(set(meta['live'].tolist()))}")
    assert ev["escaped"] == 0, f"{name}: {ev['escaped']} envs mis-ordered by the fp32 keys lie OUTSIDE tie_tolerance: the tolerance is too small"
    assert name in fc.FLOORS, f"{name}: no floors committed"
    for k in ("wrong", "inside", "window", "shared"):
        floor = fc.FLOORS[name][k]
        assert len(floor) == R and all(v >= max(f, 1) for v, f in zip(ev[k], floor)), \
            f"{name}: {k} per rank {ev[k]} on the models, floors {floor}: the case no longer tests that"
    # full enumeration: every (rank, ordered slot pair) in a near tie; every live count; the tie at the last shown rank
    assert fc.arrangements(meta) == {(r, i, j) for r in range(1, R + 1) for (i, j) in fc.slot_pairs(F)}
    assert len(fc.arrangements(meta, fc.EXACT)) >= min(R * F * (F - 1), 800) and len(fc.arrangements(meta, fc.SHARED)) >= min(R * F * (F - 1), 400) // 2
    assert set(meta["live"].tolist()) == set(range(1, F + 1))
    near, Ks = meta["family"] == fc.NEAR, fc.shown(cfg)
    if Ks + 1 <= F:
        assert (near & meta["empties"] & (meta["live"] == Ks + 1) & (meta["rank"] == Ks)).any(), "no tie K / K + 1 with K + 1 live foods"
    if 2 <= Ks <= F:
        assert (near & (meta["live"] == Ks) & (meta["rank"] == Ks - 1)).any(), "no tie K - 1 / K with K live foods"
    assert (meta["size"][meta["family"] == fc.EXACT].max() == min(4, F)) and (meta["family"] == fc.SINGLE).sum() >= 16
    # wavefronts are mixed: each holds full food sets and empty slots, and every family
    wave = np.arange(n) // 64
    for w in (0, n // 64 - 1):
        m = wave == w
        assert 0 < meta["empties"][m].sum() < 64 and len(set(meta["family"][m].tolist())) >= 3
    orc.close()
