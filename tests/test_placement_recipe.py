"""CPU guard of the GPU placement tests' recipe (tests/placement_cases.py): the oracle alone, over the shared case table
and run shape, must reach what tests/test_gpu_food_placement.py exists to compare — foods placed by the forced draw at
reset, in in-rollout resets and at respawn, valid draws found in a later 64-draw batch, wavefronts in which some lanes
respawn (limit 50) while others are reset (limit 100) — and must show that a rejection limit one off would be seen.  The
figures come from the oracle's placement counters (oracle/salp_oracle.h), which change no output."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
import placement_cases as plc

PAIRS = [pytest.param(k, r, id=f"{plc.case_id(k)}-{r}") for k, r in plc.pairs()]


def test_case_table_names_every_kernel_class():
    named = set(pc.EXPECT_KERNEL.values())
    import golden_util
    named |= set(golden_util.RT_KERNEL.values())
    assert set(plc.CASES) == named and len(plc.CASES) == 12
    cfgs = {k: plc.case_cfg(k, plc.regimes_for(k)[0]) for k in plc.CASES}
    slots = lambda c: ((1 if c.num_food_items <= 1 else 4 if c.num_food_items <= 4 else 8 if c.num_food_items <= 8 else
                        12 if c.num_food_items <= 12 else 16) if c.max_observed_food == 3 else (12 if c.num_food_items <= 12 else 16))
    for k, c in cfgs.items():
        assert slots(c) == k[0] and (3 if c.max_observed_food == 3 else 8) == k[1], (k, c)
    fewer = sorted((c.num_food_items, k[0]) for k, c in cfgs.items() if c.num_food_items < k[0])
    assert fewer == [(5, 8), (9, 12), (14, 16)]          # and 1..4 foods in 4 slots where the count is drawn:
    assert [k for k, c in cfgs.items() if c.random_food_count] == [(4, 3, 0)]
    assert set(plc.MIXED_DISTANCE) == {k for k in plc.CASES if k[2] == 0} and set(plc.FLOORS) == set(plc.pairs())
    assert len(plc.pairs()) == 2 * 7 + 5
    assert set(plc.STEP_KERNELS) <= set(plc.CASES)
    # the run shape: whole wavefronts for the unpredicated kernel (more than one workgroup) plus a ragged remainder
    assert plc.N_UNPREDICATED % plc.WAVE == 0 and plc.N_UNPREDICATED > plc.BLOCK and 0 < plc.N_PREDICATED < plc.WAVE
    assert plc.N_ENVS % plc.WAVE != 0 and plc.HORIZON == 40 and plc.BUDGET == 6
    # and the one batch that the library itself splits: just beyond n H = 2^22, ragged
    assert (plc.SPLIT_ENVS - 1) * plc.HORIZON <= 1 << 22 < plc.SPLIT_ENVS * plc.HORIZON and plc.SPLIT_ENVS % plc.WAVE != 0
    assert (plc.SPLIT_KERNEL, plc.SPLIT_REGIME) in plc.pairs()


@pytest.mark.parametrize("kernel,regime", PAIRS)
def test_the_distance_decides_between_literal_and_runtime_constants(kernel, regime):
    """Why the literal classes have no `forced` and no `mixed` regime: min_food_distance is one of the literal constants, so
    the handle of a literal-class spec at any other distance is a handle of the run-time class (is_std() on the host, what
    salp_vec_create consults).  And every case of the table runs the class it is keyed by."""
    import params_host_lib as ph
    cfg = plc.case_cfg(kernel, regime)
    # (the generic-K classes report literal constants 0 whatever is_std() says; their cases are off the literals anyway)
    assert ph.Params(cfg.to_c()).is_std() == bool(kernel[2]), (kernel, regime)
    if kernel[2]:
        assert cfg.min_food_distance == plc.LITERAL_DISTANCE
        for d in (plc.FORCED_DISTANCE, 200.0, 80.0 + 2.0 ** -40):
            other = pc.make_cfg(dict(plc.CASES[kernel], max_steps_without_food=plc.BUDGET, min_food_distance=d))
            assert not ph.Params(other.to_c()).is_std(), d


def test_counters_change_no_output_and_count_masked_resets():
    """The counters are bookkeeping: a clear in the middle changes nothing, and a masked reset counts its envs' foods only."""
    cfg = plc.case_cfg((12, 3, 0), "mixed")
    a, b = (ol.OracleVec(cfg, 100, seed=3) for _ in range(2))
    act = pc.make_actions(cfg, 30, 100, seed=1)
    assert (a.placement_counters()[ol.PC_RESET_PLACED] == 12).all()
    b.clear_placement_counters()
    assert not b.placement_counters().any()
    ra, rb = a.rollout(act, want_final=True), b.rollout(act, want_final=True)
    for k in ("obs", "reward64", "terminated", "truncated", "final_obs", "info"):
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    before = a.placement_counters()
    mask = plc.reset_mask(100)
    a.reset(mask)
    b.reset(mask)
    grown = a.placement_counters() - before
    assert np.array_equal(grown[ol.PC_RESET_PLACED], 12 * mask.astype(np.int64))
    assert (grown[ol.PC_RESET_FORCED] <= grown[ol.PC_RESET_PLACED]).all() and not grown[ol.PC_RESPAWN_PLACED].any()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y, equal_nan=True)
    with pytest.raises(ValueError):
        a.set_placement_limits(-1, 50)
    a.close()
    b.close()


def differing_envs(cfg, run, other):
    """Envs whose final food rows or draw counter differ between two runs of the recipe (after the rollout)."""
    F = cfg.num_food_items
    fa, fb = (r["state1"][0][ol.F_FOOD0: ol.F_FOOD0 + 2 * F] for r in (run, other))
    food = ~((fa == fb) | (np.isnan(fa) & np.isnan(fb))).all(axis=0)
    return food | (run["state1"][1][ol.I_RNG_COUNTER] != other["state1"][1][ol.I_RNG_COUNTER])


@pytest.mark.parametrize("kernel,regime", PAIRS)
def test_recipe_reaches_the_forced_draw_on_the_oracle(kernel, regime):
    run = plc.run_oracle(kernel, regime)
    cfg, ref, n = run["cfg"], run["ref"], plc.N_ENVS
    ev = plc.placement_events(run)
    print(f"{plc.case_id(kernel)} {regime} (min_food_distance {cfg.min_food_distance:g}): {ev}")
    floors = plc.floors_for(kernel, regime)
    assert regime == "literal" or all(floors[k] >= v for k, v in plc.MIN_FLOORS.items())
    for k, v in floors.items():
        assert ev[k] >= v, f"{k} = {ev[k]} on the oracle, below the floor {v}: the case no longer tests that ({ev})"
    assert ev["twice"] == n, f"{n - ev['twice']} envs do not finish twice"
    # every food placed is counted, by the route it took: at create, in the rollout's resets, at the masked reset
    nf0, nf2 = plc.foods_present(cfg, run["state0"]), plc.foods_present(cfg, run["state2"])
    assert ev["initial_placed"] == int(nf0.sum()) and ev["masked_reset_placed"] == int(nf2[run["mask"] != 0].sum())
    assert ev["respawn_placed"] == ev["respawns"] and ev["rollout_reset_placed"] > 0
    near = plc.near_food_lanes(n) & ~(ref["terminated"][0] | ref["truncated"][0]).astype(bool)
    assert (ref["info"][0, near, pc.INFO_STEPS_SINCE_FOOD] == 0).all(), "the injected near food is captured on the first step"
    drawn_count = 1 if cfg.random_food_count else 0
    if regime == "forced":
        for part in ("initial", "rollout_reset", "masked_reset"):
            assert ev[f"{part}_forced"] == ev[f"{part}_placed"] > 0, (part, ev)
        assert ev["respawn_forced"] == ev["respawn_placed"] and ev["max_valid_rejections"] == 0
        assert np.array_equal(run["state0"][1][ol.I_RNG_COUNTER], (plc.RESET_LIMIT + 1) * nf0 + drawn_count), "draws of a reset"
        # the draws of the whole run: every reset 101 nf (+ the count's), every respawn 51, one jitter draw per thrust step;
        # so the counter after the masked reset of an env exceeds the one before it by exactly 101 nf (+ 1)
        m = run["mask"] != 0
        grown = run["state2"][1][ol.I_RNG_COUNTER] - run["state1"][1][ol.I_RNG_COUNTER]
        assert np.array_equal(grown[m], (plc.RESET_LIMIT + 1) * nf2[m] + drawn_count) and not grown[~m].any()
    elif regime == "literal":       # the class's own 80 px: the forced draw is out of reach (tests/placement_cases.py)
        assert ev["reset_forced"] == 0 and ev["respawn_forced"] == 0
        return
    else:
        for part in ("initial", "rollout_reset", "masked_reset"):
            share = ev[f"{part}_forced"] / ev[f"{part}_placed"]
            assert 0.10 <= share <= 0.90, f"{part}: {share:.3f} of the foods of a reset are forced ({ev})"
        assert ev["respawn_forced"] >= 1 and ev["respawn_placed"] - ev["respawn_forced"] >= 1, ev
        if cfg.num_food_items >= 5:
            assert ev["max_valid_rejections"] >= plc.WAVE, f"no valid draw behind a whole batch of rejections ({ev})"
    # sensitivity: a limit one off, either way, must change what the GPU comparison looks at
    for limits in ((plc.RESET_LIMIT - 1, plc.RESPAWN_LIMIT - 1), (plc.RESET_LIMIT + 1, plc.RESPAWN_LIMIT + 1)):
        off = differing_envs(cfg, run, plc.run_oracle(kernel, regime, limits=limits))
        print(f"    limits {limits}: {int(off.sum())} of {n} envs end with other foods or draw counters")
        assert off.sum() >= (n // 2 if regime == "forced" else 1), (limits, int(off.sum()))
    # and each limit alone
    for limits in ((plc.RESET_LIMIT - 1, plc.RESPAWN_LIMIT), (plc.RESET_LIMIT, plc.RESPAWN_LIMIT + 1)):
        assert differing_envs(cfg, run, plc.run_oracle(kernel, regime, limits=limits)).any(), limits


def test_crowded_tank_reaches_the_forced_respawn_of_the_literal_sixteen_slot_class():
    """The one forced draw a literal-constant class can be brought to (tests/placement_cases.py CROWDED_*): respawns behind 50
    rejections in <16, 3, literal>, several of them in the whole wavefronts the unpredicated (HALF) kernel runs, next to
    lanes that are reset in the same step; and a respawn limit one off changes the foods or draw counters compared."""
    import params_host_lib as ph
    run = plc.run_crowded()
    cfg, n, fl = run["cfg"], plc.CROWDED_ENVS, plc.CROWDED_FLOORS
    assert ph.Params(cfg.to_c()).is_std() and cfg.num_food_items == 16 and cfg.max_observed_food == 3
    assert abs(plc.crowded_open_share() - plc.CROWDED_OPEN) < 0.002
    assert plc.CROWDED_UNPREDICATED % plc.WAVE == 0 and n % plc.WAVE != 0 and n * plc.CROWDED_HORIZON <= 1 << 22
    ev, head = plc.crowded_events(run), plc.crowded_events(run, 0, plc.CROWDED_UNPREDICATED)
    print(f"crowded: {ev}; first {plc.CROWDED_UNPREDICATED} envs: {head}")
    assert ev["respawn_forced"] >= fl["respawn_forced"] and head["respawn_forced"] >= fl["respawn_forced_unpredicated"]
    assert ev["respawn_placed"] - ev["respawn_forced"] >= fl["respawn_valid"]
    assert ev["resets"] >= fl["resets"] and ev["both_limits"] >= fl["both_limits"] >= plc.MIN_FLOORS["both_limits"]
    assert ev["reset_forced"] == 0          # a reset at 80 px stays out of reach
    capture = ~plc.crowded_truncating_lanes(n)
    assert (run["ref"]["info"][0, capture, pc.INFO_STEPS_SINCE_FOOD] == 0).all() and run["ref"]["truncated"][0, ~capture].all()
    forced_envs = (run["placed1"] - run["placed0"])[ol.PC_RESPAWN_FORCED] > 0
    # A forced respawn consumes 51 draws.  One limit less: 50, in every such env.  One more: the 51st draw is judged, and only
    # where it happens to be valid (CROWDED_OPEN of the time) does the env end as before; elsewhere it consumes 52.
    for limits, share in (((plc.RESET_LIMIT, plc.RESPAWN_LIMIT - 1), 1.0), ((plc.RESET_LIMIT, plc.RESPAWN_LIMIT + 1), 0.5)):
        off = differing_envs(cfg, run, plc.run_crowded(limits=limits))
        print(f"    limits {limits}: {int(off.sum())} envs end with other foods or draw counters, {int(off[forced_envs].sum())} of the {int(forced_envs.sum())} forced")
        assert off[forced_envs].sum() >= share * forced_envs.sum(), limits


def test_default_distance_would_leave_the_forced_draw_untested():
    """What the regimes are for: at the specs' own min_food_distance no food of the whole table is placed by the forced draw."""
    forced = 0
    for kernel in plc.CASES:
        cfg = pc.make_cfg(dict(plc.CASES[kernel], max_steps_without_food=plc.BUDGET))
        orc = ol.OracleVec(cfg, plc.N_ENVS, seed=plc.ENV_SEED)
        orc.rollout(pc.make_actions(cfg, plc.HORIZON, plc.N_ENVS, seed=plc.ACTION_SEED))
        c = orc.placement_counters()
        forced += int(c[ol.PC_RESET_FORCED].sum() + c[ol.PC_RESPAWN_FORCED].sum())
        orc.close()
    assert forced == 0
