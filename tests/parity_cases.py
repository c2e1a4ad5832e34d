"""The rollout-parity case table, its actions and its start state, shared by the GPU parity tests
(tests/test_gpu_parity.py) and their CPU guard (tests/test_parity_recipe.py).  Needs numpy, the package's
configuration and the oracle binding only — no GPU library.

Why a start state: from a plain reset 17 of the 20 cases finish no episode in 384 steps and none ever meets a wall, so the
kernels' terminal branch (autoreset, `final_obs` store, post-reset observation, `info` of a lane that ends while its
neighbours go on) was compared with nothing.  `inject_start_state` makes every case end episodes, both ways, in mixed
wavefronts; `count_events` measures that ON THE ORACLE'S OUTPUT and `FLOORS` / `MIN_FLOORS` keep it from going dead again.
"""
import numpy as np

import oracle_lib as ol
import underwater_swimmer_rl_amd as pkg

N_ENVS, HORIZON, ENV_SEED, ACTION_SEED, START_SEED = 2048, 384, 11, 3, 7
DEFAULT_BUDGET = 150        # max_steps_without_food of a case that does not set its own
WAVE = 64

CASES = {
    "single_food": dict(preset="single_food"),
    "long_horizon": dict(preset="single_food_long_horizon"),
    "sac_gail_F12": dict(preset="sac_gail"),
    "free_breathing": dict(preset="single_food", forced_breathing=False),
    "no_respawn_F3": dict(preset="sac_gail", num_food_items=3, respawn_food=False),
    "random_count_F5": dict(preset="sac_gail", num_food_items=5, random_food_count=True),
    "class_default_F5": dict(preset="sac_gail", num_food_items=5),          # the 8-slot register-food instantiation
    "F8_all_slots": dict(preset="sac_gail", num_food_items=8, max_steps_without_food=150),
    # K = 3 with non-default constants: the per-slot-count instantiations that read their constants from the launch parameters
    "other_tank_F1": dict(preset="single_food", width=900, height=700, tank_margin=40.0),
    "other_physics_F12": dict(preset="sac_gail", drag_coefficient=0.97, max_thrust_force=120.0, base_radius=26.0,
                              inhale_duration=100, exhale_duration=130, nozzle_response_rate=0.08),
    "other_tank_F5_free": dict(preset="sac_gail", num_food_items=5, width=1000, forced_breathing=False, min_food_distance=60.0),
    "K2_generic": dict(preset="sac_gail", num_food_items=6, max_observed_food=2, proximity_reward_weight=2.0),
    "K0_no_food_obs": dict(preset="single_food", max_observed_food=0),
    "F0_empty": dict(preset="single_food", num_food_items=0),
    "short_timeout": dict(preset="single_food", max_steps_without_food=40),
    # the unpredicated (main-launch) forms of the instantiations that only ran predicated before round 3:
    "F16_sixteen_slots": dict(preset="sac_gail", num_food_items=16, max_steps_without_food=200),        # <16, 3, STD>
    "F16_sixteen_slots_other_tank": dict(preset="sac_gail", num_food_items=16, width=900, height=650),  # <16, 3, !STD>
    "F14_K5_generic_lds": dict(preset="sac_gail", num_food_items=14, max_observed_food=5),              # <16, 8>: generic, foods in LDS
    "F9_K5_generic_reg": dict(preset="sac_gail", num_food_items=9, max_observed_food=5),                # <12, 8>: generic, foods in VGPRs
    "F3_other_tank": dict(preset="sac_gail", num_food_items=3, width=900, tank_margin=40.0),            # <4, 3, !STD>
}
# (food slots, observed capacity, literal constants) of the kernel each case must run (salp_vec_last_launch);
# the generic instantiations (observed capacity 8) always read their constants from the launch parameters
EXPECT_KERNEL = {
    "single_food": (1, 3, 1), "long_horizon": (1, 3, 1), "sac_gail_F12": (12, 3, 1), "free_breathing": (1, 3, 1),
    "no_respawn_F3": (4, 3, 1), "random_count_F5": (8, 3, 1), "class_default_F5": (8, 3, 1), "F8_all_slots": (8, 3, 1),
    "other_tank_F1": (1, 3, 0), "other_physics_F12": (12, 3, 0), "other_tank_F5_free": (8, 3, 0), "K2_generic": (12, 8, 0),
    "K0_no_food_obs": (12, 8, 0), "F0_empty": (1, 3, 1), "short_timeout": (1, 3, 1),
    "F16_sixteen_slots": (16, 3, 1), "F16_sixteen_slots_other_tank": (16, 3, 0), "F14_K5_generic_lds": (16, 8, 0),
    "F9_K5_generic_reg": (12, 8, 0), "F3_other_tank": (4, 3, 0),
}

INFO_FOOD_COLLECTED, INFO_STEPS_SINCE_FOOD, INFO_COLLISION = 0, 1, 2


def make_cfg(spec):
    spec = dict(spec)
    return pkg.load_env_config(spec.pop("preset"), **spec)


def case_cfg(name, budget=DEFAULT_BUDGET):
    """The case's configuration with its event budget; `budget=None` leaves the preset's own max_steps_without_food."""
    spec = dict(CASES[name])
    if budget is not None:
        spec.setdefault("max_steps_without_food", budget)
    return make_cfg(spec)


def make_actions(cfg, H, n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    act = rng.uniform(-scale, scale, size=(H, n, cfg.act_dim)).astype(np.float32)
    if not cfg.forced_breathing:  # inhale control in [0,1], held for random stretches
        hold = rng.uniform(0, 1, size=(H // 16 + 1, n)).repeat(16, axis=0)[:H]
        act[..., 0] = hold.astype(np.float32)
    return act


def wall_lanes(n):
    """Every 4th env: 16 of the 64 lanes of every wavefront head for a wall, the other 48 go on."""
    return np.arange(n) % 4 == 1


def completion_lanes(n):
    """Every 8th env (none of them a wall lane): lanes that collect all their foods when nothing respawns."""
    return np.arange(n) % 8 == 3


def inject_start_state(cfg, f64, i32, seed=START_SEED, ssf_low=0):
    """Edits a post-reset snapshot (get_state rows, include/salp_vec.h) in place; the caller hands the same arrays to the
    device's and the oracle's set_state.  Stands for the reference's attribute pokes `env.robot_pos`, `env.robot_velocity`,
    `env.steps_since_food`, `env.food_positions` (eval/collect_navigation_data.py:76-89).
      * wall lanes: 5-120 px (body edge at its widest, 1.3 R, to the wall) inside one of the four walls, 0.5-3 px/step towards it;
      * every env: steps_since_food uniform in [ssf_low, max_steps_without_food), so truncations spread over steps and lanes;
      * respawn_food=False with >= 3 foods: completion lanes get their first three foods 3, 6 and 9 px away — one capture per step
        (the capture loop stops at its first hit), so with F = 3 they terminate by completion on their third step and pass
        through "fewer live foods than K" on the way."""
    n = f64.shape[1]
    rng = np.random.default_rng(seed)
    lanes = np.nonzero(wall_lanes(n))[0]
    side = rng.integers(0, 4, lanes.size)
    gap = rng.uniform(5.0, 120.0, lanes.size) + 1.3 * cfg.base_radius
    speed = rng.uniform(0.5, 3.0, lanes.size)
    lo, hi_x, hi_y = cfg.tank_margin, cfg.width - cfg.tank_margin, cfg.height - cfg.tank_margin
    x, y, vx, vy = f64[ol.F_X], f64[ol.F_Y], f64[ol.F_VX], f64[ol.F_VY]
    for s, (pos, vel, where, sign) in enumerate(((x, vx, lo, 1.0), (x, vx, hi_x, -1.0), (y, vy, lo, 1.0), (y, vy, hi_y, -1.0))):
        m = lanes[side == s]
        pos[m] = where + sign * gap[side == s]
        vel[m] = -sign * speed[side == s]
    i32[ol.I_STEPS_SINCE_FOOD] = rng.integers(ssf_low, cfg.max_steps_without_food, n)
    F = cfg.num_food_items
    if not cfg.respawn_food and F >= 3:
        m = np.nonzero(completion_lanes(n))[0]
        ang = rng.uniform(-np.pi, np.pi, (3, m.size))
        for k, d in enumerate((3.0, 6.0, 9.0)):
            f64[ol.F_FOOD0 + k, m] = x[m] + d * np.cos(ang[k])
            f64[ol.F_FOOD0 + F + k, m] = y[m] + d * np.sin(ang[k])
    return f64, i32


def start_oracle(cfg, n, seed, start_seed=START_SEED, ssf_low=0, threads=1):
    """An oracle in the injected start state, and the snapshot that put it there (for the device's set_state)."""
    orc = ol.OracleVec(cfg, n, seed=seed, threads=threads)
    f64, i32 = orc.get_state()
    inject_start_state(cfg, f64, i32, seed=start_seed, ssf_low=ssf_low)
    orc.set_state(f64, i32)
    return orc, f64, i32


def count_events(ref):
    """Event counts of an oracle rollout ([H, n] outputs with `info`)."""
    term, trunc, info = ref["terminated"].astype(bool), ref["truncated"].astype(bool), ref["info"]
    done = term | trunc
    wall = term & (info[..., INFO_COLLISION] != 0)
    H, n = done.shape
    per_wave = done[:, : n // WAVE * WAVE].reshape(H, n // WAVE, WAVE).sum(axis=2)
    return dict(
        wall=int(wall.sum()), wall_steps=int(wall.any(axis=1).sum()), truncated=int(trunc.sum()),
        captures=int((info[..., INFO_STEPS_SINCE_FOOD] == 0).sum()),      # the counter is zero after a step only if it collected
        completed=int((term & ~wall).sum()),
        mixed_wave_steps=int(((per_wave > 0) & (per_wave < WAVE)).sum()), # (step, wavefront) pairs: some lanes finish, not all
        twice=int((done.sum(axis=0) >= 2).sum()))


def steps_left_short_of_foods(cfg, ref):
    """respawn_food=False only: env-steps after which the episode goes on with fewer live foods than K (every capture
    takes one food away for the rest of the episode), i.e. steps the kernels then run with missing observed entries."""
    assert not cfg.respawn_food
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    live = cfg.num_food_items - ref["info"][..., INFO_FOOD_COLLECTED]
    return int(((live < cfg.max_observed_food) & ~done).sum())


NO_RESPAWN_SHORT_STEPS_FLOOR = 3600      # no_respawn_F3: half of the 7200 such env-steps the oracle shows

# No case may fall below these, whatever FLOORS says (ISSUE: the conditions of the recipe).
MIN_FLOORS = dict(wall=50, truncated=1000, mixed_wave_steps=1000, captures=10)
# Per case: about half of what the recipe gives on the oracle (tests/test_parity_recipe.py prints the figures).
FLOORS = {
    "single_food": dict(wall=100, truncated=2500, captures=15, mixed_wave_steps=2100, twice=1000),
    "long_horizon": dict(wall=100, truncated=2500, captures=15, mixed_wave_steps=2100, twice=1000),
    "sac_gail_F12": dict(wall=120, truncated=2400, captures=120, mixed_wave_steps=2000, twice=1000),
    "free_breathing": dict(wall=110, truncated=2500, captures=17, mixed_wave_steps=2100, twice=1000),
    "no_respawn_F3": dict(wall=100, truncated=2400, captures=410, mixed_wave_steps=1900, twice=1000),
    "random_count_F5": dict(wall=100, truncated=2500, captures=27, mixed_wave_steps=2100, twice=1000),
    "class_default_F5": dict(wall=110, truncated=2500, captures=53, mixed_wave_steps=2100, twice=1000),
    "F8_all_slots": dict(wall=120, truncated=2400, captures=88, mixed_wave_steps=2100, twice=1000),
    "other_tank_F1": dict(wall=100, truncated=2500, captures=13, mixed_wave_steps=2100, twice=1000),
    "other_physics_F12": dict(wall=89, truncated=2400, captures=140, mixed_wave_steps=2000, twice=1000),
    "other_tank_F5_free": dict(wall=120, truncated=2400, captures=86, mixed_wave_steps=2100, twice=1000),
    "K2_generic": dict(wall=110, truncated=2500, captures=65, mixed_wave_steps=2100, twice=1000),
    "K0_no_food_obs": dict(wall=100, truncated=2500, captures=15, mixed_wave_steps=2100, twice=1000),
    "F0_empty": dict(wall=100, truncated=2500, captures=0, mixed_wave_steps=2100, twice=1000),
    "short_timeout": dict(wall=50, truncated=9500, captures=15, mixed_wave_steps=4800, twice=1000),
    "F16_sixteen_slots": dict(wall=150, truncated=1600, captures=340, mixed_wave_steps=1500, twice=770),
    "F16_sixteen_slots_other_tank": dict(wall=120, truncated=2400, captures=130, mixed_wave_steps=2000, twice=1000),
    "F14_K5_generic_lds": dict(wall=130, truncated=2400, captures=150, mixed_wave_steps=2000, twice=1000),
    "F9_K5_generic_reg": dict(wall=120, truncated=2400, captures=100, mixed_wave_steps=2100, twice=1000),
    "F3_other_tank": dict(wall=100, truncated=2500, captures=30, mixed_wave_steps=2100, twice=1000),
}


def floors_for(name):
    f = dict(MIN_FLOORS)
    f.update(FLOORS.get(name, {}))
    if CASES[name].get("num_food_items", 1) == 0:
        f["captures"] = 0
    return f


def assert_event_floors(name, ev):
    for k, v in floors_for(name).items():
        assert ev[k] >= v, f"{name}: {k} = {ev[k]} on the oracle, below the floor {v}: the case no longer tests that event ({ev})"
    assert ev["twice"] > 0, f"{name}: no env finishes twice ({ev})"
    if name == "no_respawn_F3":
        assert ev["completed"] > 0, f"{name}: no termination by completion ({ev})"


# ---- the acting path (salp_vec_step with final_obs + info), tests/test_gpu_parity.py::test_step_acting_path_*
STEP_PRESET, STEP_ENV_SEED, STEP_ACTION_SEED = "sac_gail", 21, 4
STEP_CASES = {"whole_wavefronts": dict(n=4096, steps=400), "ragged": dict(n=4096 + 37, steps=150)}
STEP_FLOORS = {     # about half of the oracle's figures
    "whole_wavefronts": dict(wall=320, truncated=1400, captures=710, mixed_wave_steps=1600),
    "ragged": dict(wall=250, truncated=1600, captures=250, mixed_wave_steps=1500),
}


def step_case(name):
    """cfg, oracle in its start state, the snapshot, actions.  sac_gail keeps its budget of 1500 steps without food; the
    counters start in its last `steps` steps, so truncations fall on every step of the run."""
    c = STEP_CASES[name]
    cfg = pkg.load_env_config(STEP_PRESET)
    orc, f64, i32 = start_oracle(cfg, c["n"], STEP_ENV_SEED, ssf_low=cfg.max_steps_without_food - c["steps"], threads=4)
    return cfg, orc, f64, i32, make_actions(cfg, c["steps"], c["n"], seed=STEP_ACTION_SEED)


def assert_step_floors(name, ev):
    for k in ("wall", "truncated", "captures", "mixed_wave_steps"):
        assert ev[k] > STEP_FLOORS.get(name, {}).get(k, 0), f"step case {name}: {k} = {ev[k]} on the oracle ({ev})"
