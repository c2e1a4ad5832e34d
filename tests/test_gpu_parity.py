"""GPU parity tests: the HIP path (through the C ABI of include/salp_vec.h) against the CPU oracle
on the same seeded inputs.  Run on the MI355X box with `pytest -m gpu`.

Tolerances (north_star: "within 1e-5 fp32"):
  * terminated / truncated / info integers: identical;
  * observation: max |diff| <= 1e-5 (columns holding an angle/pi are compared on the circle,
    i.e. modulo 2, because -1 and +1 are the same heading — snake:403-407 wraps to [-pi, pi]);
  * reward: |diff| <= 1e-5 * max(1, |reward|);
  * fp64 state snapshot: |diff| <= 1e-9 (only device sin/cos and d^2-vs-sqrt predicates differ).
The helpers and the tolerances live in tests/gpu_support.py; they are imported by name because the soak scripts reach
them through this module.
"""
import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
from gpu_support import (OBS_TOL, REW_TOL, assert_final_obs, assert_parity, assert_state_parity, device_state,   # noqa: F401
                         run_device, start_pair)
from parity_cases import CASES, EXPECT_KERNEL, make_actions, make_cfg   # noqa: F401  (the soak scripts reach them through this module)
from support import obs_diff
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpLib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_parity(name):
    """Every case ends episodes in mixed wavefronts, by wall contact and by truncation (and captures food where it has any):
    the start state of tests/parity_cases.py, injected into device and oracle alike.  The event counts are taken from the
    ORACLE's output and held above floors (also on the CPU: tests/test_parity_recipe.py), so the terminal branch of the
    kernel the case names — autoreset, final_obs store, post-reset observation — is always compared."""
    cfg = pc.case_cfg(name)
    n, H, seed = pc.N_ENVS, pc.HORIZON, pc.ENV_SEED
    act = make_actions(cfg, H, n, seed=pc.ACTION_SEED)
    dev, orc = start_pair(cfg, n, seed)
    assert_state_parity(cfg, dev, orc, f"{name}: start state")
    got, _ = run_device(cfg, n, act, want_final=True, dev=dev)
    ref = orc.rollout(act, want_final=True)
    ev = pc.count_events(ref)
    pc.assert_event_floors(name, ev)
    dmax, rmax = assert_parity(cfg, got, ref, name)
    fmax = assert_final_obs(cfg, got["final_obs"], ref, name)
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert_state_parity(cfg, dev, orc, name)
    if name == "no_respawn_F3":     # lanes that run with fewer live foods than K, and terminations by completion
        assert pc.steps_left_short_of_foods(cfg, ref) >= pc.NO_RESPAWN_SHORT_STEPS_FLOOR
        assert (ref["terminated"].astype(bool) & (ref["info"][..., pc.INFO_COLLISION] == 0)).sum() > 0
    st = dev.stats()
    assert st["env_steps"] == n * H
    assert st["episodes"] == int(done.sum())
    assert st["terminated"] == int(ref["terminated"].sum()) and st["truncated"] == int(ref["truncated"].sum())
    assert st["collisions"] == int(ref["info"][..., pc.INFO_COLLISION].sum()) and st["food_collected"] == ev["captures"]
    ll = dev.last_launch()      # 2048 envs = 32 whole wavefronts: the unpredicated kernel, non-FULL signature (final_obs)
    assert ll["envs_unpredicated"] == n and ll["envs_predicated"] == 0
    assert ll["full_signature"] == (2 if ll["observed_capacity"] == 3 else 0)    # main outputs + final_obs + info
    assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (ll["full_signature"], -1)
    assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == EXPECT_KERNEL[name], ll
    print(f"{name}: max obs diff {dmax:.3g}, final_obs {fmax:.3g}, max rel reward diff {rmax:.3g}, episodes {st['episodes']}, "
          f"wall terminations {ev['wall']}, truncations {ev['truncated']}, captures {ev['captures']}, mixed wavefront-steps "
          f"{ev['mixed_wave_steps']}, kernel {EXPECT_KERNEL[name]} signature {ll['full_signature']}")
    dev.close()
    orc.close()


@pytest.mark.parametrize("name", list(pc.STEP_CASES))
def test_step_acting_path_matches_oracle(name):
    """salp_vec_step with every output (final_obs and info included) — what SAC's acting loop calls — on 64 whole wavefronts
    of sac_gail, and its ragged twin (4096 + 37 envs: a step call of that size runs ONE predicated launch, which exists for
    the every-store-tested signature only).  Every step's observation, reward, flags, info and the final_obs rows of the
    finished envs against the oracle, then the state; wall terminations, truncations and captures all occur (floors on the
    oracle's output, also in tests/test_parity_recipe.py); last_launch names the kernel after every step."""
    cfg, orc, f64, i32, act = pc.step_case(name)
    H, n = act.shape[:2]
    ref = orc.rollout(act, want_final=True)
    pc.assert_step_floors(name, pc.count_events(ref))
    dev = SalpLib(cfg, n, device_id=0, seed=pc.STEP_ENV_SEED)
    dev.set_state(f64, i32, 0)
    obs = np.empty((n, cfg.obs_dim), np.float32)
    rew = np.empty(n, np.float32)
    term = np.empty(n, np.uint8)
    trunc = np.empty(n, np.uint8)
    info = np.empty((n, 3), np.int32)
    fin = np.empty((n, cfg.obs_dim), np.float32)
    ragged = n % 64 != 0
    want = (dict(envs_unpredicated=0, envs_predicated=n, full_signature=0, signature_unpredicated=-1, signature_predicated=0)
            if ragged else
            dict(envs_unpredicated=n, envs_predicated=0, full_signature=2, signature_unpredicated=2, signature_predicated=-1))
    dmax = rmax = fmax = 0.0
    for t in range(H):
        fin.fill(np.nan)
        dev.step(act[t], obs, rew, term, trunc, fin, info, 0)
        assert np.array_equal(term, ref["terminated"][t]) and np.array_equal(trunc, ref["truncated"][t]), f"flags differ at step {t}"
        assert np.array_equal(info, ref["info"][t]), f"info differs at step {t}"
        dmax = max(dmax, float(obs_diff(cfg, obs, ref["obs"][t]).max()))
        r64 = ref["reward64"][t]
        rmax = max(rmax, float((np.abs(rew - r64) / np.maximum(1.0, np.abs(r64))).max()))
        done = (term | trunc).astype(bool)
        assert np.array_equal(np.isnan(fin[:, 0]), ~done), f"final_obs rows at step {t}"
        if done.any():
            fmax = max(fmax, float(obs_diff(cfg, fin[done], ref["final_obs"][t][done]).max()))
        assert dmax <= OBS_TOL and rmax <= REW_TOL and fmax <= OBS_TOL, f"step {t}: obs {dmax}, reward {rmax}, final_obs {fmax}"
        ll = dev.last_launch()
        assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == (12, 3, 1)
        assert {k: ll[k] for k in want} == want, ll
    assert_state_parity(cfg, dev, orc, f"step path {name}")
    print(f"step path {name}: max obs diff {dmax:.3g}, final_obs {fmax:.3g}, reward {rmax:.3g}, {pc.count_events(ref)}")
    dev.close()
    orc.close()


def test_split_launch_with_final_obs_matches_oracle():
    """One rollout call split into the unpredicated launch (64 whole wavefronts, terminal-observation signature) and the
    predicated launch over the last 37 envs (every store tested): n H > 2^22 env-steps, with the injected start state, so both
    halves end episodes.  last_launch reports each half's own signature."""
    cfg = pkg.load_env_config("sac_gail", max_steps_without_food=300)
    n, H, seed = 4096 + 37, 1020, 13
    dev, orc = start_pair(cfg, n, seed, threads=4)
    act = make_actions(cfg, H, n, seed=14)
    got, _ = run_device(cfg, n, act, want_final=True, dev=dev)
    ref = orc.rollout(act, want_final=True)
    ev_tail = pc.count_events({k: ref[k][:, 4096:] for k in ("terminated", "truncated", "info")})     # the predicated half
    assert ev_tail["wall"] > 0 and ev_tail["truncated"] > 0 and ev_tail["captures"] > 0, ev_tail
    assert_parity(cfg, got, ref, "split launch")
    assert_final_obs(cfg, got["final_obs"], ref, "split launch")
    assert_state_parity(cfg, dev, orc, "split launch")
    ll = dev.last_launch()
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (4096, 37), ll
    assert (ll["full_signature"], ll["signature_unpredicated"], ll["signature_predicated"]) == (2, 2, 0), ll
    dev.close()
    orc.close()


@pytest.mark.parametrize("foods,slots", [(3, 4), (5, 8), (12, 12), (16, 16)])
def test_multi_food_full_signature_main_launch(foods, slots):
    """The FULL-signature unpredicated kernels (what bench.py and salp_vec_rollout without final_obs run) of every
    multi-food slot count, with captures, respawns and truncation resets inside whole wavefronts."""
    cfg = pkg.load_env_config("sac_gail", num_food_items=foods, max_steps_without_food=120)
    n, H, seed = 1024, 400, 31 + foods
    act = make_actions(cfg, H, n, seed=foods)
    got, dev = run_device(cfg, n, act, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    ref = orc.rollout(act)
    assert_parity(cfg, got, ref, f"F{foods} full signature")
    assert_state_parity(cfg, dev, orc, f"F{foods} full signature")
    ll = dev.last_launch()
    assert ll["food_slots"] == slots and ll["observed_capacity"] == 3 and ll["literal_constants"] == 1
    assert ll["full_signature"] == 1 and ll["envs_unpredicated"] == n and ll["envs_predicated"] == 0
    assert dev.stats()["truncated"] > 100
    dev.close()


def test_config2_4096x256_single_food():
    """BASELINE.json configs[1]: N_envs=4096 single_food, 256-step rollout, fp32 diff <= 1e-5."""
    cfg = pkg.load_env_config("single_food")
    n, H = 4096, 256
    act = make_actions(cfg, H, n, seed=0)
    got, dev = run_device(cfg, n, act, seed=0)
    ref = ol.OracleVec(cfg, n, seed=0).rollout(act)
    dmax, rmax = assert_parity(cfg, got, ref, "config2")
    print(f"config2: max obs diff {dmax:.3g}, max rel reward diff {rmax:.3g}")
    dev.close()


def test_long_rollout_wall_and_food_events():
    """2000 steps: many wall terminations, food captures + respawns, the rounding-escape case."""
    cfg = pkg.load_env_config("single_food_long_horizon")
    n, H = 512, 2000
    act = make_actions(cfg, H, n, seed=9)
    got, dev = run_device(cfg, n, act, seed=5)
    orc = ol.OracleVec(cfg, n, seed=5)
    ref = orc.rollout(act)
    assert ref["terminated"].sum() > 100
    assert_parity(cfg, got, ref, "long")
    assert_state_parity(cfg, dev, orc, "long")
    dev.close()


def test_step_equals_rollout_and_info():
    cfg = pkg.load_env_config("sac_gail")
    n, H, seed = 777, 300, 21   # ragged: not a multiple of 64
    act = make_actions(cfg, H, n, seed=4)
    got, dev_r = run_device(cfg, n, act, seed=seed)
    dev_s = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    ref = orc.rollout(act)
    obs = np.empty((n, cfg.obs_dim), np.float32)
    rew = np.empty(n, np.float32)
    term = np.empty(n, np.uint8)
    trunc = np.empty(n, np.uint8)
    info = np.empty((n, 3), np.int32)
    for t in range(H):
        dev_s.step(act[t], obs, rew, term, trunc, None, info, 0)
        assert np.array_equal(obs, got["obs"][t]) and np.array_equal(rew, got["reward"][t])
        assert np.array_equal(term, got["terminated"][t]) and np.array_equal(trunc, got["truncated"][t])
        assert np.array_equal(info, ref["info"][t]), f"info differs at step {t}"
    # 777 envs: one predicated launch each; the rollout ran the main-only kernel, the step (info) the every-store-tested one
    lr, ls = dev_r.last_launch(), dev_s.last_launch()
    assert (lr["envs_unpredicated"], lr["envs_predicated"], ls["envs_unpredicated"], ls["envs_predicated"]) == (0, n, 0, n)
    assert (lr["full_signature"], lr["signature_unpredicated"], lr["signature_predicated"]) == (1, -1, 1), lr
    assert (ls["full_signature"], ls["signature_unpredicated"], ls["signature_predicated"]) == (0, -1, 0), ls
    dev_r.close()
    dev_s.close()


def test_reset_observation_and_mask():
    cfg = pkg.load_env_config("sac_gail")
    n, seed = 1000, 3
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    obs = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs, 0)
    assert obs_diff(cfg, obs, orc.observe()).max() <= OBS_TOL
    act = make_actions(cfg, 50, n, seed=1)
    run_device(cfg, n, act, dev=dev)
    orc.rollout(act)
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    dev.reset(mask, obs, 0)
    ref = orc.reset(mask)
    assert obs_diff(cfg, obs, ref).max() <= OBS_TOL
    assert_state_parity(cfg, dev, orc, "masked reset")
    dev.close()


@pytest.mark.parametrize("n,preset,over", [(640, "single_food", {}), (700, "sac_gail", {}),
                                            (333, "single_food", dict(forced_breathing=False))])
def test_device_generated_actions_match_oracle_stream(n, preset, over):
    """act == NULL: in-kernel generation (FULL signature), full and ragged wavefronts, 1 and 2 actions."""
    cfg = pkg.load_env_config(preset, **over)
    H, seed = 203, 99
    got, dev = run_device(cfg, n, None, horizon=H, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    ref = orc.rollout(None, horizon=H)
    assert np.array_equal(got["actions"], ref["actions"])
    assert got["actions"][..., -1].min() >= -1.0 and got["actions"][..., -1].max() < 1.0
    assert_parity(cfg, got, ref, "device actions")
    # second launch continues the action stream at global step H
    got2, _ = run_device(cfg, n, None, horizon=50, dev=dev)
    ref2 = orc.rollout(None, horizon=50)
    assert np.array_equal(got2["actions"], ref2["actions"])
    assert_parity(cfg, got2, ref2, "device actions, 2nd launch")
    dev.close()


def test_set_state_injection_eval_style():
    """eval/collect_navigation_data.py:76-89: overwrite pose, velocity, heading and the food."""
    cfg = pkg.load_env_config("single_food", respawn_food=False, max_steps_without_food=3000)
    n, seed = 256, 1
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    f64, i32 = device_state(dev, cfg)
    rng = np.random.default_rng(2)
    f64[_capi.F_X] = 150.0
    f64[_capi.F_Y] = 300.0
    f64[_capi.F_VX] = 0.0
    f64[_capi.F_VY] = 0.0
    f64[_capi.F_THETA] = rng.uniform(-np.pi, np.pi, n)
    f64[_capi.F_OMEGA] = 0.0
    f64[_capi.F_FOOD0] = 650.0
    f64[_capi.F_FOOD0 + 1] = 300.0
    i32[_capi.I_STEPS_SINCE_FOOD] = 0
    dev.set_state(f64, i32, 0)
    fo, io_ = orc.get_state()
    fo[:] = f64
    fo[_capi.F_ELLIPSE_A] = 30.0
    fo[_capi.F_ELLIPSE_B] = 30.0
    orc.set_state(fo, i32)
    obs = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs, 0)
    assert obs_diff(cfg, obs, orc.observe()).max() <= OBS_TOL
    act = make_actions(cfg, 600, n, seed=8, scale=0.3)
    got, _ = run_device(cfg, n, act, dev=dev)
    ref = orc.rollout(act)
    assert_parity(cfg, got, ref, "injected")
    assert_state_parity(cfg, dev, orc, "injected")
    dev.close()


# ---- injected-state edges: snapshots the reference's attribute pokes can produce and a plain reset never does -----------
# Each runs a literal-constant kernel and one that reads its constants (they differ exactly here), on four whole wavefronts,
# with the injected lanes mixed among untouched ones.  Either the device matches the oracle within the contract or
# salp_vec_set_state refuses the snapshot (include/salp_vec.h, "Ranges accepted by salp_vec_set_state").
EDGE_N = 256


def edge_pair(cfg, seed, edit, n=EDGE_N):
    """Device and oracle after `edit(f64, i32)` on the post-reset snapshot.  The oracle takes the ellipse rows as given
    (salp_oracle.c set_state) while the device derives them, so an edit that changes water or the breathing integers also
    writes the ellipse the reference's formulas (legacy:184-259) give for that state."""
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    f64, i32 = orc.get_state()
    edit(f64, i32)
    dev.set_state(f64, i32, 0)
    orc.set_state(f64, i32)
    return dev, orc


def compare_edge(cfg, dev, orc, act, label, kernel):
    n = dev.n_envs
    obs = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs, 0)
    d0 = obs_diff(cfg, obs, orc.observe())
    assert d0.max() <= OBS_TOL, f"{label}: observe() diff {d0.max()} at {np.unravel_index(d0.argmax(), d0.shape)}"
    got, _ = run_device(cfg, n, act, want_final=True, dev=dev)
    ref = orc.rollout(act, want_final=True)
    assert_parity(cfg, got, ref, label)
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert np.array_equal(np.isnan(got["final_obs"][..., 0]), ~done)
    if done.any():
        assert obs_diff(cfg, got["final_obs"][done], ref["final_obs"][done]).max() <= OBS_TOL, f"{label}: final_obs"
    assert_state_parity(cfg, dev, orc, label)
    ll = dev.last_launch()
    assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == kernel and ll["envs_predicated"] == 0, ll
    return got, ref


def refused(dev, f64, i32, word):
    """set_state refuses the snapshot with SALP_ERR_INVALID and a message naming the quantity; nothing is written."""
    before = device_state(dev, dev.cfg)
    with pytest.raises(_capi.SalpError, match=word) as e:
        dev.set_state(f64, i32, 0)
    assert "(-1)" in str(e.value)
    after = device_state(dev, dev.cfg)
    assert np.array_equal(before[0], after[0], equal_nan=True) and np.array_equal(before[1], after[1])


WATER_CONFIGS = {      # forced and free breathing, each with literal constants and with constants read at run time
    "literal_forced": (dict(preset="single_food"), (1, 3, 1)),
    "literal_free_F12": (dict(preset="sac_gail", forced_breathing=False), (12, 3, 1)),
    "runtime_forced_F3": (dict(preset="sac_gail", num_food_items=3, width=900, tank_margin=40.0), (4, 3, 0)),
    # exhale_duration = 250: the longest released breath, int(250 max(water, 0.3)), must still fit the packed word's 8 bits
    "runtime_free_exhale250": (dict(preset="single_food", forced_breathing=False, exhale_duration=250, base_radius=26.0), (1, 3, 0)),
}


@pytest.mark.parametrize("name", list(WATER_CONFIGS))
def test_injected_water_level_in_range_matches_oracle(name):
    """`env.water_volume = w; env.breathing_phase = 'inhaling'; env.breathing_timer = t` (legacy:184-259) with w anywhere in
    [0, 1], not only the t / inhale_duration a run produces: timer at and below inhale_duration, so forced breathing releases on
    the first step and free breathing releases where the action says so.  The released breath's ellipse comes from w; the
    swimmer starts inside the wall's reach moving into it, so the radius of that very step decides the clamped position
    (terminal observation, columns 0 and 6)."""
    spec, kernel = WATER_CONFIGS[name]
    cfg = make_cfg(spec)
    rng = np.random.default_rng(31)
    lanes = np.nonzero(np.arange(EDGE_N) % 3 == 0)[0]
    water = rng.choice([0.0, 0.04, 0.05, 0.050000000000000044, 0.3, 0.62, 1.0 - 2.0 ** -53, 1.0], lanes.size)
    timer = rng.choice([cfg.inhale_duration, cfg.inhale_duration - 1, cfg.inhale_duration // 2, 3], lanes.size)
    R = cfg.base_radius

    def edit(f64, i32):
        i32[ol.I_PHASE, lanes], i32[ol.I_TIMER, lanes], i32[ol.I_SHAPE_HOLD, lanes] = 1, timer, 0
        f64[ol.F_WATER, lanes] = water
        f64[ol.F_ELLIPSE_A, lanes] = R * 1.3 + (R * 1.1 - R * 1.3) * water       # legacy:212-213 at progress = water
        f64[ol.F_ELLIPSE_B, lanes] = R * 0.8 + (R * 1.1 - R * 0.8) * water
        f64[ol.F_X, lanes], f64[ol.F_VX, lanes] = cfg.tank_margin + R, -1.0        # nearer than any radius: clamped to margin + r

    dev, orc = edge_pair(cfg, 3, edit)
    act = make_actions(cfg, 40, EDGE_N, seed=32)
    if not cfg.forced_breathing:       # half of the injected lanes release at once, the others keep inhaling for a while
        act[:6, lanes[::2], 0] = 0.0
        act[:6, lanes[1::2], 0] = 1.0
    got, ref = compare_edge(cfg, dev, orc, act, f"water {name}", kernel)
    # the wall was met on that very step (x is clamped to margin + r; `x - r <= margin` can miss by a rounding, snake:219-230)
    assert (ref["terminated"][0, lanes] & ref["info"][0, lanes, pc.INFO_COLLISION]).mean() > 0.5
    dev.close()
    orc.close()


@pytest.mark.parametrize("name", ["literal_forced", "runtime_free_exhale250"])
@pytest.mark.parametrize("water", [1.0 + 1e-9, 1.2, 2.5, -0.1, float("nan")])
def test_injected_water_level_out_of_range_is_refused(name, water):
    """`env.water_volume = 1.2` and the like.  The reference would go on (2.5 at exhale_duration 150 gives a 375-step breath,
    ellipse_b > ellipse_a for one step); the packed breathing word keeps 8 bits of the length and the literal-constant
    kernels take ellipse_a for the radius, so set_state refuses a level outside [0, 1] instead of diverging."""
    cfg = make_cfg(WATER_CONFIGS[name][0])
    dev = SalpLib(cfg, EDGE_N, device_id=0, seed=3)
    f64, i32 = device_state(dev, cfg)
    i32[_capi.I_PHASE, 70], i32[_capi.I_TIMER, 70], i32[_capi.I_SHAPE_HOLD, 70] = 1, 60, 0
    f64[_capi.F_WATER, 70] = water
    refused(dev, f64, i32, "water")
    f64[_capi.F_WATER, 70] = 1.0           # the same snapshot with the level in range is taken
    dev.set_state(f64, i32, 0)
    assert device_state(dev, cfg)[0][_capi.F_WATER, 70] == 1.0
    dev.close()


def test_breathing_integers_out_of_range_are_refused():
    """The packed breathing word keeps 2 + 8 + 8 + 3 bits: values beyond them were silently truncated."""
    cfg = pkg.load_env_config("single_food")
    dev = SalpLib(cfg, EDGE_N, device_id=0, seed=3)
    for row, bad in ((_capi.I_EXHALE_DUR, 375), (_capi.I_TIMER, 256), (_capi.I_PHASE, 3), (_capi.I_SHAPE_HOLD, 8), (_capi.I_TIMER, -1)):
        f64, i32 = device_state(dev, cfg)
        i32[row, 129] = bad
        refused(dev, f64, i32, "exhale duration")
    dev.close()


HEADING_CONFIGS = {
    "literal_F1": (dict(preset="single_food"), (1, 3, 1)),
    "runtime_F1": (dict(preset="single_food", width=900, height=700, tank_margin=40.0), (1, 3, 0)),
    "literal_F12": (dict(preset="sac_gail", proximity_reward_weight=1.0), (12, 3, 1)),
    "runtime_F16": (dict(preset="sac_gail", num_food_items=16, width=900, height=650), (16, 3, 0)),
    "generic_F9_K5": (dict(preset="sac_gail", num_food_items=9, max_observed_food=5), (12, 8, 0)),
}


@pytest.mark.parametrize("name", list(HEADING_CONFIGS))
def test_injected_heading_far_outside_the_circle_matches_oracle(name):
    """`env.robot_angle = 70.0` (eval/collect_navigation_data.py:80 pokes the heading; nothing keeps it in [-pi, pi]), with and
    without angular velocity.  observe() before any step reports theta / pi unwrapped, as the reference would; the first step
    wraps it by repeated subtraction (legacy:329-332) — up to 16 turns here, where the kernels used to stop after 9 and
    leave the heading outside the circle."""
    spec, kernel = HEADING_CONFIGS[name]
    cfg = make_cfg(spec)
    rng = np.random.default_rng(41)
    lanes = np.nonzero(np.arange(EDGE_N) % 3 == 1)[0]
    theta = rng.choice([3.5, -3.5, 20.0, -20.0, 57.0, -57.0, 70.0, -70.0, 100.0, -100.0], lanes.size)
    omega = rng.choice([0.0, 0.0, 0.3, -0.3, 2.0, -7.0], lanes.size)

    def edit(f64, i32):
        f64[ol.F_THETA, lanes], f64[ol.F_OMEGA, lanes] = theta, omega

    dev, orc = edge_pair(cfg, 5, edit)
    compare_edge(cfg, dev, orc, make_actions(cfg, 30, EDGE_N, seed=42), f"heading {name}", kernel)
    f_end, _ = orc.get_state()
    assert np.abs(f_end[ol.F_THETA]).max() <= np.pi
    dev.close()
    orc.close()


@pytest.mark.parametrize("row,value", [(_capi.F_THETA, 1e3), (_capi.F_THETA, -1e3), (_capi.F_THETA, 100.001), (_capi.F_OMEGA, -250.0),
                                       (_capi.F_THETA, float("inf")), (_capi.F_OMEGA, float("nan"))])
def test_injected_heading_beyond_the_documented_range_is_refused(row, value):
    """theta = 1e3 is 318.3 in the observation, where fp32 no longer resolves 1e-5, and 159 turns of the wrapping loop: refused
    (|theta|, |omega| <= SALP_SET_STATE_MAX_ANGLE = 100)."""
    cfg = pkg.load_env_config("single_food")
    dev = SalpLib(cfg, EDGE_N, device_id=0, seed=5)
    f64, i32 = device_state(dev, cfg)
    f64[row, 200] = value
    refused(dev, f64, i32, "theta")
    dev.close()


NEAR_FOOD_CONFIGS = {
    "literal_F12": (dict(preset="sac_gail", proximity_reward_weight=5.0), (12, 3, 1)),
    "runtime_F12": (dict(preset="sac_gail", proximity_reward_weight=5.0, width=900), (12, 3, 0)),
    "literal_F8": (dict(preset="sac_gail", num_food_items=8, proximity_reward_weight=5.0), (8, 3, 1)),
    "literal_F16": (dict(preset="sac_gail", num_food_items=16, proximity_reward_weight=5.0), (16, 3, 1)),
    "generic_F9_K5": (dict(preset="sac_gail", num_food_items=9, max_observed_food=5, proximity_reward_weight=5.0), (12, 8, 0)),
    "generic_F14_K5": (dict(preset="sac_gail", num_food_items=14, max_observed_food=5, proximity_reward_weight=5.0), (16, 8, 0)),
}


@pytest.mark.parametrize("name", list(NEAR_FOOD_CONFIGS))
def test_several_foods_next_to_the_swimmer_keep_every_observed_entry(name):
    """`env.food_positions[k] = robot_pos + tiny` for three and four slots (the fallback placement of snake:120-131 can do the
    same to two).  The capture loop takes the lowest slot inside the radius, one per step, so after the first step two (lanes
    0 mod 3) or three (lanes 1 mod 3) foods within 2 px are alive in the SAME observation: entries 0, 1 and 2 each need offsets
    from the exact positions — with fp32 positions (roundings of ~3e-5 px) a bearing at 0.45 px is off by up to ~1e-4 rad."""
    spec, kernel = NEAR_FOOD_CONFIGS[name]
    cfg = make_cfg(spec)
    F = cfg.num_food_items
    rng = np.random.default_rng(51)
    idx = np.arange(EDGE_N)
    variants = ((idx % 3 == 0, ((2, 1.8), (5, 0.3), (7, 0.45))),                 # slot 2 goes first: 0.3 and 0.45 px stay
                (idx % 3 == 1, ((1, 2.0), (2, 0.6), (5, 0.3), (7, 0.45))))      # slot 1 goes first: three stay

    def edit(f64, i32):
        for mask, foods in variants:
            m = np.nonzero(mask)[0]
            f64[ol.F_X, m] += rng.uniform(-30.0, 30.0, m.size)      # off the tank centre, which fp32 holds exactly
            f64[ol.F_Y, m] += rng.uniform(-30.0, 30.0, m.size)
            for slot, d in foods:
                ang = rng.uniform(-np.pi, np.pi, m.size)
                f64[ol.F_FOOD0 + slot, m] = f64[ol.F_X, m] + d * np.cos(ang)
                f64[ol.F_FOOD0 + F + slot, m] = f64[ol.F_Y, m] + d * np.sin(ang)

    dev, orc = edge_pair(cfg, 21, edit)
    act = np.zeros((5, EDGE_N, cfg.act_dim), np.float32)
    got, ref = compare_edge(cfg, dev, orc, act, f"near foods {name}", kernel)
    # the state the case is about was reached: after step 0 entries 0 and 1 (and 2) are within 2 px (distance / diagonal)
    diag = float(np.hypot(cfg.width, cfg.height))
    two, three = variants[0][0], variants[1][0]
    assert (ref["obs"][0, two][:, 10 + 4 * 1 + 2] * diag < 2.0).all() and (ref["obs"][0, three][:, 10 + 4 * 2 + 2] * diag < 2.05).all()
    assert (ref["info"][:3, two | three, pc.INFO_STEPS_SINCE_FOOD] == 0).all()      # a capture on each of the first three steps
    d = obs_diff(cfg, got["obs"], ref["obs"])
    for e in range(3):      # entries 0, 1, 2 and the reward, spelled out (compare_edge has asserted the whole row already)
        assert d[..., 10 + 4 * e: 14 + 4 * e].max() <= OBS_TOL, f"near foods {name}: entry {e} diff {d[..., 10 + 4 * e: 14 + 4 * e].max()}"
    rd = np.abs(got["reward"] - ref["reward64"]) / np.maximum(1.0, np.abs(ref["reward64"]))
    assert rd.max() <= REW_TOL, f"near foods {name}: reward diff {rd.max()}"
    dev.close()
    orc.close()


FEW_FOOD_CONFIGS = {       # (spec, kernel, live foods kept in the injected lanes; None = the config itself has fewer than K)
    "F2_K3_literal": (dict(preset="sac_gail", num_food_items=2, respawn_food=False), (4, 3, 1), None),
    "F2_K3_runtime": (dict(preset="sac_gail", num_food_items=2, respawn_food=False, width=900), (4, 3, 0), None),
    "F5_two_live_literal": (dict(preset="sac_gail", num_food_items=5, respawn_food=False), (8, 3, 1), 2),
    "F5_two_live_runtime": (dict(preset="sac_gail", num_food_items=5, respawn_food=False, tank_margin=40.0), (8, 3, 0), 2),
    "F12_one_live_literal": (dict(preset="sac_gail", num_food_items=12, respawn_food=False), (12, 3, 1), 1),
    "F12_one_live_runtime": (dict(preset="sac_gail", num_food_items=12, respawn_food=False, base_radius=28.0), (12, 3, 0), 1),
}


@pytest.mark.parametrize("name", list(FEW_FOOD_CONFIGS))
def test_fewer_live_foods_than_observed_entries_from_the_first_step(name):
    """`env.food_positions[k] = None` (snake:215) for all but one or two slots, nothing respawning: the selection has missing
    entries (index -1, padded observation) on every one of 400 steps, in lanes next to lanes with a full set."""
    spec, kernel, keep = FEW_FOOD_CONFIGS[name]
    cfg = make_cfg(spec)
    F = cfg.num_food_items
    lanes = np.nonzero(np.arange(EDGE_N) % 2 == 0)[0]

    def edit(f64, i32):
        if keep is not None:       # the survivors sit in the LAST slots: every lower slot is empty
            f64[ol.F_FOOD0: ol.F_FOOD0 + F - keep, lanes] = np.nan
            f64[ol.F_FOOD0 + F: ol.F_FOOD0 + 2 * F - keep, lanes] = np.nan

    dev, orc = edge_pair(cfg, 61, edit)
    got, ref = compare_edge(cfg, dev, orc, make_actions(cfg, 400, EDGE_N, seed=62), f"few foods {name}", kernel)
    short = (ref["obs"][..., 10 + 4 * 2 + 2] == 1.0) & (ref["obs"][..., 10 + 4 * 2] == 0.0)      # third entry padded (snake:412)
    assert short[:, lanes].mean() > 0.9, short[:, lanes].mean()
    dev.close()
    orc.close()


def test_out_of_range_and_nan_actions():
    """Actions are not clipped by the reference (legacy:125-135); NaN ends up at +max nozzle."""
    cfg = pkg.load_env_config("single_food")
    n, H = 128, 120
    act = make_actions(cfg, H, n, seed=6, scale=3.0)
    act[5::17, 3::7, 0] = np.nan
    got, dev = run_device(cfg, n, act, seed=2)
    orc = ol.OracleVec(cfg, n, seed=2)
    ref = orc.rollout(act)
    assert np.array_equal(got["terminated"], ref["terminated"])
    ok = ~np.isnan(ref["obs"]).any(axis=-1)
    assert obs_diff(cfg, got["obs"][ok], ref["obs"][ok]).max() <= OBS_TOL
    assert np.array_equal(np.isnan(got["obs"]), np.isnan(ref["obs"]))
    dev.close()


def test_sharding_is_trajectory_invariant():
    """env i's trajectory depends on its GLOBAL index only (multi-GPU sharding by env index)."""
    cfg = pkg.load_env_config("sac_gail")
    n, H, seed = 512, 150, 17
    act = make_actions(cfg, H, n, seed=12)
    full, d0 = run_device(cfg, n, act, seed=seed)
    lo, d1 = run_device(cfg, n // 2, np.ascontiguousarray(act[:, : n // 2]), seed=seed, base=0)
    hi, d2 = run_device(cfg, n // 2, np.ascontiguousarray(act[:, n // 2:]), seed=seed, base=n // 2)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert np.array_equal(full[k][:, : n // 2], lo[k]) and np.array_equal(full[k][:, n // 2:], hi[k]), k
    for d in (d0, d1, d2):
        d.close()


@pytest.mark.parametrize("foods", [1, 5, 12, 16])
def test_partial_output_signatures_match_oracle(foods):
    """Callers may leave any output NULL (include/salp_vec.h): the kernels compiled for that case test every store.  Two
    such signatures per slot count in the unpredicated launch (2048 envs) — no reward / truncated, and reward + flags
    without observations (with terminal observations) — against the oracle, and the state after both."""
    cfg = make_cfg(dict(preset="sac_gail", num_food_items=foods, max_steps_without_food=60))
    n, H, seed = 2048, 200, 5
    act = make_actions(cfg, 2 * H, n, seed=9)
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    ref1 = orc.rollout(act[:H], want_final=True)
    ref2 = orc.rollout(act[H:], want_final=True)
    obs = np.empty((H, n, cfg.obs_dim), np.float32)
    term = np.empty((H, n), np.uint8)
    dev.rollout(np.ascontiguousarray(act[:H]), H, obs, None, term, None, None, None, 0)
    ll = dev.last_launch()
    assert ll["full_signature"] == 0 and ll["envs_unpredicated"] == n and ll["food_slots"] >= foods
    assert np.array_equal(term, ref1["terminated"])
    assert obs_diff(cfg, obs, ref1["obs"]).max() <= OBS_TOL
    rew = np.empty((H, n), np.float32)
    trunc = np.empty((H, n), np.uint8)
    fin = np.full((H, n, cfg.obs_dim), np.nan, np.float32)
    dev.rollout(np.ascontiguousarray(act[H:]), H, None, rew, term, trunc, fin, None, 0)
    assert dev.last_launch()["full_signature"] == 0
    assert np.array_equal(term, ref2["terminated"]) and np.array_equal(trunc, ref2["truncated"])
    r = ref2["reward"]
    assert (np.abs(rew - r) / np.maximum(1.0, np.abs(r))).max() <= REW_TOL
    done = (ref2["terminated"] | ref2["truncated"]).astype(bool)
    assert done.any() and np.array_equal(np.isnan(fin[..., 0]), ~done)
    assert obs_diff(cfg, fin[done], ref2["final_obs"][done]).max() <= OBS_TOL
    assert_state_parity(cfg, dev, orc, f"partial_F{foods}")
    dev.close()
    orc.close()


@pytest.mark.parametrize("foods,tank,min_wg,max_vgprs", [
    (1, False, 4, 128), (3, False, 4, 128), (5, False, 4, 128), (8, False, 4, 128), (12, False, 3, 168), (16, False, 3, 168),
    (5, True, 4, 128), (8, True, 4, 128), (1, True, 4, 128), (12, True, 3, 168), (16, True, 2, 256)])
def test_kernel_occupancy_matches_the_design(foods, tank, min_wg, max_vgprs):
    """DESIGN.md section 3.1's occupancy table as the runtime reports it for the kernels actually launched (no timing):
    workgroups of 256 threads resident per CU (= wavefronts per SIMD), VGPRs, no scratch — for the main-only signature and
    for the one with terminal observations, literal constants and an 801-wide tank.  (Two signatures of the 4- / 8-slot kernels
    once sat at 129 VGPRs — three per SIMD, 22 % slower — without any test noticing.)"""
    cfg = make_cfg(dict(preset="sac_gail", num_food_items=foods, **(dict(width=801) if tank else {})))
    n, H = 2048, 4
    act = make_actions(cfg, H, n, seed=1)
    dev = SalpLib(cfg, n, device_id=0, seed=3)
    for want_final in (False, True):
        run_device(cfg, n, act, dev=dev, want_final=want_final)
        ll, res = dev.last_launch(), dev.last_kernel_resources()
        assert ll["literal_constants"] == (0 if tank else 1) and ll["full_signature"] == (2 if want_final else 1)
        assert res["workgroups_per_cu"] >= min_wg, (ll, res)
        assert res["vgprs"] <= max_vgprs and res["scratch_bytes"] <= (32 if tank else 0), (ll, res)   # (801-wide, 12 slots: 2 registers)
    dev.close()


def test_food_next_to_the_swimmer_keeps_the_reward_exact():
    """A fallback placement (snake:120-131, :270-276) can leave a food next to the swimmer; with two foods inside the capture
    radius the one in the later slot survives a step, and the shaped reward w cos(bearing) is then taken on an offset of a
    fraction of a pixel.  In fp32 (roundings of both positions, ~6e-5 px) the bearing of a food 0.7 px away was off by
    1.7e-5 rad, the reward of w = 5 by 8e-5 (tests/soak_main_kernels.py case 92); the nearest food's offsets now come from the
    exact positions when it is that close.  Injected: 12 foods, two of them 0.4 and 0.9 px from the resting swimmer."""
    cfg = make_cfg(dict(preset="sac_gail", proximity_reward_weight=5.0))
    n, H = 128, 3
    dev = SalpLib(cfg, n, device_id=0, seed=21)
    orc = ol.OracleVec(cfg, n, seed=21)
    f64, i32 = device_state(dev, cfg)
    rng = np.random.default_rng(4)
    ang = rng.uniform(-np.pi, np.pi, size=(2, n))
    F = cfg.num_food_items
    for j, (slot, d) in enumerate(((7, 0.4), (3, 0.9))):     # the nearer one sits in the LATER slot: it survives the first step
        f64[_capi.F_FOOD0 + slot] = f64[_capi.F_X] + d * np.cos(ang[j])
        f64[_capi.F_FOOD0 + F + slot] = f64[_capi.F_Y] + d * np.sin(ang[j])
    dev.set_state(f64, i32, 0)
    orc.set_state(f64, i32)
    act = np.zeros((H, n, cfg.act_dim), np.float32)
    got, _ = run_device(cfg, n, act, dev=dev)
    ref = orc.rollout(act)
    assert ref["reward"][0].max() > 10 and ref["reward"][1].max() > 10      # a capture in each of the first two steps
    assert_parity(cfg, got, ref, "near food")
    r = ref["reward"]
    assert (np.abs(got["reward"] - r) / np.maximum(1.0, np.abs(r))).max() <= 3e-6
    dev.close()
    orc.close()


def test_properties_full_size_262144():
    """BASELINE.json configs[2] size, checked through size-independent properties: bounded
    observations, breathing period 273 in forced mode, |nozzle| <= 1, positions inside the tank,
    env-step accounting, and agreement with the oracle on a strided sample of 256 envs."""
    cfg = pkg.load_env_config("single_food_long_horizon")
    n, H, seed = 262144, 300, 0
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    obs = np.empty((H, n, cfg.obs_dim), np.float32)
    term = np.empty((H, n), np.uint8)
    aout = np.empty((H, n, 1), np.float32)
    dev.rollout(None, H, obs, None, term, None, None, aout, 0)
    assert np.isfinite(obs).all()
    assert obs[..., 0].min() >= (50 + 24) / 800 - 1e-6 and obs[..., 0].max() <= (750 - 24) / 800 + 1e-6
    assert obs[..., 1].min() >= (50 + 24) / 600 - 1e-6 and obs[..., 1].max() <= (550 - 24) / 600 + 1e-6
    assert np.abs(obs[..., 9]).max() <= 1.0 + 1e-6
    assert obs[..., 8].min() >= 0.0 and obs[..., 8].max() <= 1.0
    assert np.abs(obs[..., 4]).max() <= 1.0 + 1e-6
    alive = term[:284].sum(axis=0) == 0                     # envs that did not reset in the first cycle
    assert alive.sum() > n // 2
    assert np.array_equal(obs[0, alive, 6], obs[273, alive, 6])   # body size repeats with period 273
    assert np.array_equal(obs[10, alive, 7], obs[283, alive, 7])
    assert dev.stats()["env_steps"] == n * H
    idx = np.arange(0, n, n // 256)[:256]
    for j, i in enumerate(idx[:64]):
        orc = ol.OracleVec(cfg, 1, seed=seed, env_index_base=int(i))
        ref = orc.rollout(np.ascontiguousarray(aout[:, i:i + 1]))
        assert np.array_equal(term[:, i], ref["terminated"][:, 0])
        assert obs_diff(cfg, obs[:, i], ref["obs"][:, 0]).max() <= OBS_TOL
    dev.close()


def test_create_rejects_bad_arguments():
    lib = _capi.load_library()
    cfg = pkg.load_env_config("single_food")
    with pytest.raises(_capi.SalpError):
        SalpLib(cfg, 0)
    with pytest.raises(_capi.SalpError):
        SalpLib(cfg, 16, device_id=99)
    c = cfg.to_c()
    c.struct_size = 8
    import ctypes
    h = ctypes.c_void_p()
    assert lib.salp_vec_create(ctypes.byref(c), 16, 0, 0, 0, ctypes.byref(h)) == -1
    assert b"struct_size" in lib.salp_last_error()


def _random_cfg(rng):
    """A random but valid environment: food slots 0..16, observed foods 0..8, every flag, non-default tank,
    radii, drag, thrust and durations (the generic <16, 8> instantiation and the LDS food path), or the
    reference's constants with random flags (the STD instantiations)."""
    std = rng.random() < 0.4
    kw = dict(num_food_items=int(rng.integers(0, 17)), max_observed_food=int(rng.integers(0, 9)) if not std else 3,
              forced_breathing=bool(rng.random() < 0.6), random_food_count=bool(rng.random() < 0.3),
              respawn_food=bool(rng.random() < 0.7), proximity_reward_weight=float(rng.choice([0.0, 0.5, 5.0])),
              efficiency_bonus=float(rng.choice([0.0, 1.0])), max_steps_without_food=int(rng.integers(20, 400)),
              food_reward=float(rng.uniform(1, 20)), collision_penalty=float(-rng.uniform(1, 60)),
              time_penalty=float(-rng.uniform(0, 0.5)))
    if not std:
        kw.update(width=int(rng.integers(500, 1200)), height=int(rng.integers(450, 900)),
                  tank_margin=float(rng.uniform(20, 60)), base_radius=float(rng.uniform(18, 34)),
                  max_thrust_force=float(rng.uniform(60, 160)), drag_coefficient=float(rng.uniform(0.95, 0.995)),
                  angular_drag=float(rng.uniform(0.9, 0.99)), max_nozzle_angle=float(rng.uniform(0.6, 1.3)),
                  nozzle_response_rate=float(rng.uniform(0.02, 0.2)), food_radius=float(rng.uniform(8, 25)),
                  min_food_distance=float(rng.uniform(40, 110)))
        if rng.random() < 0.5:      # other breathing timings than the legacy 120 / 150 / 60
            kw.update(inhale_duration=int(rng.integers(10, 200)), exhale_duration=int(rng.integers(20, 250)),
                      rest_duration=int(rng.integers(0, 120)))
    return pkg.SalpSnakeConfig(**kw)


@pytest.mark.parametrize("case", range(24))
def test_random_configuration_parity(case):
    rng = np.random.default_rng(1000 + case)
    cfg = _random_cfg(rng)
    # 20 cases of 777 envs: a small ragged batch (n H <= 2^22) runs ONE predicated launch over the whole range
    # (launch_rollout), so these exercise the RAGGED = true kernels only, with final_obs (non-FULL signature).
    # Cases 5, 11, 17, 23: 16449 envs x 260 steps (n H > 2^22) split into the unpredicated main launch over 257 whole
    # wavefronts plus a one-env predicated launch, FULL signature.
    big = case % 6 == 5
    n, H, seed = (16449 if big else 777), 260, int(rng.integers(0, 2 ** 31))
    act = make_actions(cfg, H, n, seed=case, scale=1.2)            # a little outside the Box too
    got, dev = run_device(cfg, n, act, seed=seed, want_final=not big)
    orc = ol.OracleVec(cfg, n, seed=seed, threads=8 if big else 1)
    ref = orc.rollout(act, want_final=not big)
    assert_parity(cfg, got, ref, f"random case {case}: {cfg}")
    assert_state_parity(cfg, dev, orc, f"random case {case}")
    ll = dev.last_launch()
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == ((16448, 1) if big else (0, 777)), ll
    if not big:
        done = (ref["terminated"] | ref["truncated"]).astype(bool)
        if done.any():
            assert obs_diff(cfg, got["final_obs"][done], ref["final_obs"][done]).max() <= OBS_TOL
    dev.close()
    orc.close()


@pytest.mark.parametrize("foods", [4, 12, 16])
def test_near_tie_food_order_matches_oracle_across_scales(foods):
    """The order of the observed foods when two of them are ALMOST equally far — relative distance gaps from 1e-16 to
    1e-4, at distances 60..200 px — must be the reference's (stable sort on the fp64 distance,
    snake:382).  The fp32 ordering pass (csrc/salp_food_reg.h) may only decide where its error bound separates the keys
    and must fall back to the exact order otherwise (4, 12 and 16 slots).  A wrong
    bound would show as two swapped food blocks (bearing columns differ by O(1)).  4096 resting swimmers (zero velocity:
    the geometry holds for the whole rollout), observe() and 20 fused steps."""
    cfg = pkg.load_env_config("sac_gail", num_food_items=foods, proximity_reward_weight=1.0)
    n, H, seed = 4096, 20, 77
    dev = SalpLib(cfg, n, device_id=0, seed=seed)
    orc = ol.OracleVec(cfg, n, seed=seed, threads=8)
    f64, i32 = device_state(dev, cfg)
    rng = np.random.default_rng(5)
    x = rng.uniform(380, 420, n); y = rng.uniform(280, 320, n)
    f64[_capi.F_X], f64[_capi.F_Y] = x, y
    f64[_capi.F_VX] = f64[_capi.F_VY] = f64[_capi.F_OMEGA] = 0.0
    f64[_capi.F_THETA] = rng.uniform(-3, 3, n)
    F = foods
    # every food far away first, all distinct
    for k in range(F):
        ang = rng.uniform(0, 2 * np.pi, n)
        rad = rng.uniform(215, 235, n) + 0.37 * k
        f64[_capi.F_FOOD0 + k] = x + rad * np.cos(ang)
        f64[_capi.F_FOOD0 + F + k] = y + 0.85 * rad * np.sin(ang)
    # two (sometimes three) slots, in random slot order, at nearly the same distance d in [45, 200]
    d = rng.uniform(60, 200, n)                       # outside the capture radius (<= 54 px)
    gap = 10.0 ** rng.uniform(-16, -4, n) * rng.choice([-1.0, 1.0], n)
    slots = np.argsort(rng.random((n, F)), axis=1)[:, :3]
    angs = rng.uniform(0, 2 * np.pi, (n, 3))
    dist = np.stack([d, d * (1.0 + gap), np.where(rng.random(n) < 0.3, d * (1.0 - 0.5 * gap), d + 60.0)], axis=1)
    for j in range(3):
        f64[_capi.F_FOOD0 + slots[:, j], np.arange(n)] = x + dist[:, j] * np.cos(angs[:, j])
        f64[_capi.F_FOOD0 + F + slots[:, j], np.arange(n)] = y + dist[:, j] * np.sin(angs[:, j])
    i32[_capi.I_STEPS_SINCE_FOOD] = 0
    dev.set_state(f64, i32, 0)
    fo, _ = orc.get_state()
    fo[:] = f64
    fo[_capi.F_ELLIPSE_A] = 30.0
    fo[_capi.F_ELLIPSE_B] = 30.0
    orc.set_state(fo, i32)
    obs = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs, 0)
    d0 = obs_diff(cfg, obs, orc.observe())
    assert d0.max() <= OBS_TOL, f"observe(): {d0.max()} at {np.unravel_index(d0.argmax(), d0.shape)}"
    act = np.zeros((H, n, 1), np.float32)
    got, _ = run_device(cfg, n, act, dev=dev)
    ref = orc.rollout(act)
    assert_parity(cfg, got, ref, f"near ties, {foods} foods")
    assert dev.last_launch()["food_slots"] == {4: 4, 12: 12, 16: 16}[foods]
    dev.close()
    orc.close()
