"""The forced-placement case table, its run shape and its event counts, shared by the GPU placement tests
(tests/test_gpu_food_placement.py) and their CPU guard (tests/test_placement_recipe.py).  Needs numpy, the package's
configuration and the oracle binding only — no GPU library.

Food placement is a rejection sampler with a deterministic escape: after `limit` rejected draws (100 at reset, snake:92-131;
50 at respawn, snake:232-276) the next draw is taken whatever it is.  At the presets' min_food_distance of 80 px that
escape all but never runs, so the device's three statements of it (place_food, place_food_coop, place_food_coop_reg: the
forced index, `attempts` carried over a 64-draw batch, the draw count written back) were compared with nothing.  Two
regimes make it run in every kernel class that reads its constants from the launch parameters (literal constants 0):
  * forced: min_food_distance = 2000 px, beyond every tank diagonal of the table: every draw is rejected, every food is the
    unconditional draw, a reset consumes exactly 101 nf draws (one more where the food count is drawn), a respawn 51;
  * mixed: a distance per case (MIXED_DISTANCE) at which, ON THE ORACLE, 10 % .. 90 % of the foods of a reset are forced,
    respawns end both ways, and (5 foods and more) valid draws are found behind 64 and more rejections, i.e. in a later batch.
The five classes with literal constants cannot be given either: min_food_distance is one of the literals (csrc/salp_params.h
SALP_STD_CONSTS, min_food_dist2 = 6400), so a handle with any other distance IS a handle of the run-time class
(is_std(), asserted on the host by the guard).  At 80 px a reset never reaches its limit (at most 15 foods and the tank
centre reject a draw, 100 times in a row), and a respawn with 12 slots or fewer does not either (12 discs cover at most 77 %
of the 670 x 470 px draw box).  What IS in reach is the forced respawn of <16, 3, literal>: 15 live foods and the swimmer
on a covering layout, injected through set_state — the crowded case below (CROWDED_*).  Besides it the literal classes
run the common recipe in a third regime, `literal`, at their own 80 px: in-rollout resets and respawns, food rows and draw
counters compared as strictly, and NO forced draw (the guard asserts that there is none, so nobody takes the regime for
more); its captures fall on the first step only, so it has next to no wavefront with both limits either.
The counts come from the oracle's placement counters (oracle/salp_oracle.h) and from `info`; FLOORS keeps them alive.

Run shape: HORIZON 40 steps, max_steps_without_food 6, the start state of parity_cases.inject_start_state (staggered
truncations, wall lanes), and in every 5th env slot 0's food 3 px from the swimmer: step 1 captures and respawns.
N_UNPREDICATED + N_PREDICATED envs: the whole wavefronts a split launch gives to the unpredicated kernel (two workgroups,
the second one partly filled) and the ragged remainder it gives to the predicated one.  The library splits a ragged batch
only when n H > 2^22 (salp_vec.hip launch_rollout: 104858 envs at this horizon), so the GPU tests run the two parts as two
handles over the env ranges [0, N_UNPREDICATED) and [N_UNPREDICATED, N) of ONE oracle run, and the whole range once more as
the single predicated launch the library itself chooses at this size.  One case (SPLIT_KERNEL) also runs at SPLIT_ENVS, the
smallest ragged batch the library does split at this horizon: one call, both parts, every env's foods and counters."""
import numpy as np

import oracle_lib as ol
import parity_cases as pc

BLOCK, WAVE = 256, pc.WAVE                   # threads of a workgroup (csrc/salp_rollout_traits.h kBlock), lanes of a wavefront
N_UNPREDICATED = BLOCK + WAVE                # 320: five whole wavefronts, two workgroups
N_PREDICATED = 22                            # the ragged remainder: one partial wavefront
N_ENVS = N_UNPREDICATED + N_PREDICATED       # 342, no multiple of 64
HORIZON, BUDGET, ENV_SEED, ACTION_SEED = 40, 6, 23, 5
NEAR_FOOD_EVERY, NEAR_FOOD_PX = 5, 3.0
RESET_LIMIT, RESPAWN_LIMIT = 100, 50         # snake:99, snake:239
FORCED_DISTANCE = 2000.0
LITERAL_DISTANCE = 80.0                     # StdConsts::min_food_dist2 = 6400

# One entry per kernel class, keyed by what salp_vec_last_launch reports: (food slots, observed capacity, literal
# constants).  The specs are those of parity_cases.CASES (respawn kept on: the respawn sampler is half of the subject).
CASES = {
    (1, 3, 1): dict(pc.CASES["single_food"]),
    (1, 3, 0): dict(pc.CASES["other_tank_F1"]),
    (4, 3, 1): dict(pc.CASES["no_respawn_F3"], num_food_items=4, respawn_food=True),
    (4, 3, 0): dict(pc.CASES["F3_other_tank"], num_food_items=4, random_food_count=True),     # 1..4 foods per episode in 4 slots
    (8, 3, 1): dict(pc.CASES["F8_all_slots"]),
    (8, 3, 0): dict(pc.CASES["other_tank_F5_free"]),                # 5 foods in 8 slots, free breathing
    (12, 3, 1): dict(pc.CASES["sac_gail_F12"]),
    (12, 3, 0): dict(pc.CASES["other_physics_F12"]),
    (16, 3, 1): dict(pc.CASES["F16_sixteen_slots"]),
    (16, 3, 0): dict(pc.CASES["F16_sixteen_slots_other_tank"]),
    (12, 8, 0): dict(pc.CASES["F9_K5_generic_reg"]),                # 9 foods in 12 slots, foods in VGPRs
    (16, 8, 0): dict(pc.CASES["F14_K5_generic_lds"]),               # 14 foods in 16 slots, foods in LDS
}
# the real split launch: the smallest n, no multiple of 64, with n HORIZON > 2^22 (salp_vec.hip launch_rollout)
SPLIT_ENVS = (1 << 22) // HORIZON + 1        # 104858 = 1638 whole wavefronts + 26 envs
SPLIT_KERNEL, SPLIT_REGIME = (4, 3, 0), "mixed"      # register foods, the food count drawn per episode, forced and valid draws
STEP_KERNELS = ((12, 3, 1), (12, 3, 0), (16, 8, 0), (1, 3, 0))                  # these also run the 40 steps through salp_vec_step

# min_food_distance of the mixed regime, px: adjusted until the guard's conditions hold on the oracle (the figures are in FLOORS)
MIXED_DISTANCE = {
    (1, 3, 0): 480.0, (4, 3, 0): 440.0, (8, 3, 0): 330.0, (12, 3, 0): 200.0, (16, 3, 0): 200.0, (12, 8, 0): 220.0, (16, 8, 0): 190.0,
}

# No case may fall below these, whatever FLOORS says.
MIN_FLOORS = dict(resets=50, respawns=10, both_limits=20, respawn_forced=1)
# Per case and regime: about half of what the recipe gives on the oracle (tests/test_placement_recipe.py prints the figures).
# resets: episodes ended (and reset) inside the rollout; respawns: captures; both_limits: both_limits(); respawn_forced: the
# oracle's count of respawns placed by the forced draw.
# The oracle's figures the floors were taken from (342 envs x 40 steps; reset foods: create + in-rollout resets + the masked
# reset; longest valid run: the most rejections that preceded a VALID acceptance; both limits: both_limits()):
#   F1_K3_literal  literal    80 px  reset foods forced     0 /  2344   respawns forced    0 /   70   longest valid run  2   resets 1888   both limits   0
#   F1_K3_runtime  forced   2000 px  reset foods forced  2332 /  2332   respawns forced  116 /  116   longest valid run  0   resets 1876   both limits  39
#   F1_K3_runtime  mixed     480 px  reset foods forced  1991 /  2336   respawns forced   84 /  105   longest valid run 99   resets 1880   both limits  28
#   F4_K3_literal  literal    80 px  reset foods forced     0 /  9352   respawns forced    0 /   80   longest valid run  5   resets 1882   both limits   2
#   F4_K3_runtime  forced   2000 px  reset foods forced  5708 /  5708   respawns forced  224 /  224   longest valid run  0   resets 1859   both limits  97
#   F4_K3_runtime  mixed     440 px  reset foods forced  3524 /  5780   respawns forced  120 /  150   longest valid run 99   resets 1874   both limits  56
#   F8_K3_literal  literal    80 px  reset foods forced     0 / 18656   respawns forced    0 /   93   longest valid run  8   resets 1876   both limits   5
#   F8_K3_runtime  forced   2000 px  reset foods forced 11505 / 11505   respawns forced  331 /  331   longest valid run  0   resets 1845   both limits 139
#   F8_K3_runtime  mixed     330 px  reset foods forced  3825 / 11660   respawns forced  111 /  150   longest valid run 99   resets 1876   both limits  65
#   F12_K3_literal literal    80 px  reset foods forced     0 / 27936   respawns forced    0 /  103   longest valid run 15   resets 1872   both limits   5
#   F12_K3_runtime forced   2000 px  reset foods forced 27120 / 27120   respawns forced  706 /  706   longest valid run  0   resets 1804   both limits 199
#   F12_K3_runtime mixed     200 px  reset foods forced 12239 / 27612   respawns forced  316 /  344   longest valid run 99   resets 1845   both limits 141
#   F16_K3_literal literal    80 px  reset foods forced     0 / 37168   respawns forced    0 /  111   longest valid run 23   resets 1867   both limits   7
#   F16_K3_runtime forced   2000 px  reset foods forced 35808 / 35808   respawns forced  864 /  864   longest valid run  0   resets 1782   both limits 212
#   F16_K3_runtime mixed     200 px  reset foods forced 17544 / 36352   respawns forced  474 /  498   longest valid run 99   resets 1816   both limits 173
#   F12_K8_runtime forced   2000 px  reset foods forced 20367 / 20367   respawns forced  634 /  634   longest valid run  0   resets 1807   both limits 196
#   F12_K8_runtime mixed     220 px  reset foods forced  7559 / 20817   respawns forced  227 /  270   longest valid run 99   resets 1857   both limits 118
#   F16_K8_runtime forced   2000 px  reset foods forced 31108 / 31108   respawns forced  953 /  953   longest valid run  0   resets 1766   both limits 211
#   F16_K8_runtime mixed     190 px  reset foods forced 15269 / 31864   respawns forced  480 /  502   longest valid run 99   resets 1820   both limits 182
FLOORS = {
    ((1, 3, 1), "literal"): dict(resets=940, respawns=35, both_limits=0, respawn_forced=0),
    ((1, 3, 0), "forced"): dict(resets=930, respawns=58, both_limits=20, respawn_forced=58),
    ((1, 3, 0), "mixed"): dict(resets=940, respawns=52, both_limits=20, respawn_forced=42),
    ((4, 3, 1), "literal"): dict(resets=940, respawns=40, both_limits=1, respawn_forced=0),
    ((4, 3, 0), "forced"): dict(resets=920, respawns=110, both_limits=48, respawn_forced=110),
    ((4, 3, 0), "mixed"): dict(resets=930, respawns=75, both_limits=28, respawn_forced=60),
    ((8, 3, 1), "literal"): dict(resets=930, respawns=46, both_limits=2, respawn_forced=0),
    ((8, 3, 0), "forced"): dict(resets=920, respawns=160, both_limits=69, respawn_forced=160),
    ((8, 3, 0), "mixed"): dict(resets=930, respawns=75, both_limits=32, respawn_forced=55),
    ((12, 3, 1), "literal"): dict(resets=930, respawns=51, both_limits=2, respawn_forced=0),
    ((12, 3, 0), "forced"): dict(resets=900, respawns=350, both_limits=99, respawn_forced=350),
    ((12, 3, 0), "mixed"): dict(resets=920, respawns=170, both_limits=70, respawn_forced=150),
    ((16, 3, 1), "literal"): dict(resets=930, respawns=55, both_limits=3, respawn_forced=0),
    ((16, 3, 0), "forced"): dict(resets=890, respawns=430, both_limits=100, respawn_forced=430),
    ((16, 3, 0), "mixed"): dict(resets=900, respawns=240, both_limits=86, respawn_forced=230),
    ((12, 8, 0), "forced"): dict(resets=900, respawns=310, both_limits=98, respawn_forced=310),
    ((12, 8, 0), "mixed"): dict(resets=920, respawns=130, both_limits=59, respawn_forced=110),
    ((16, 8, 0), "forced"): dict(resets=880, respawns=470, both_limits=100, respawn_forced=470),
    ((16, 8, 0), "mixed"): dict(resets=910, respawns=250, both_limits=91, respawn_forced=240),
}


def pairs():
    return [(k, r) for k in CASES for r in regimes_for(k)]


def case_id(kernel):
    return "F%d_K%d_%s" % (kernel[0], kernel[1], "literal" if kernel[2] else "runtime")


def regimes_for(kernel):
    return ("forced", "mixed") if kernel[2] == 0 else ("literal",)


def case_cfg(kernel, regime):
    assert regime in regimes_for(kernel), (kernel, regime)
    distance = dict(forced=FORCED_DISTANCE, mixed=MIXED_DISTANCE.get(kernel), literal=LITERAL_DISTANCE)[regime]
    cfg = pc.make_cfg(dict(CASES[kernel], max_steps_without_food=BUDGET, min_food_distance=distance))
    assert FORCED_DISTANCE > np.hypot(cfg.width, cfg.height) and cfg.respawn_food
    return cfg


def near_food_lanes(n):
    return np.arange(n) % NEAR_FOOD_EVERY == 0


def inject_start_state(cfg, f64, i32):
    """parity_cases.inject_start_state, then slot 0's food of every 5th env 3 px from the swimmer (bearing by env index)."""
    pc.inject_start_state(cfg, f64, i32)
    m = np.nonzero(near_food_lanes(f64.shape[1]))[0]
    ang = 0.7 * m
    f64[ol.F_FOOD0, m] = f64[ol.F_X, m] + NEAR_FOOD_PX * np.cos(ang)
    f64[ol.F_FOOD0 + cfg.num_food_items, m] = f64[ol.F_Y, m] + NEAR_FOOD_PX * np.sin(ang)
    return f64, i32


def reset_mask(n):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


def both_limits(cfg, ref):
    """(step, wavefront) pairs in which some lanes respawn a food (limit 50) and go on while others finish and are reset in
    the kernel (limit 100); wavefronts of 64 envs by index, the last one partial."""
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    respawn = (ref["info"][..., pc.INFO_STEPS_SINCE_FOOD] == 0) & bool(cfg.respawn_food) & ~done
    H, n = done.shape
    pad = -n % WAVE
    per_wave = lambda a: np.pad(a, ((0, 0), (0, pad))).reshape(H, -1, WAVE).any(axis=2)
    return int((per_wave(done) & per_wave(respawn)).sum())


def run_oracle(kernel, regime, limits=None, n=N_ENVS, threads=1, outputs=True):
    """The whole recipe on the oracle.  Returns a dict: cfg; `state0`, `obs0`, `placed0` after create (the initial reset);
    `f64`, `i32` the injected start state; `act`; `ref` the rollout (with final_obs and info); `state1`, `placed1` after
    it; `mask`, `obs2`, `state2`, `placed2` after the masked reset that follows.  `placed*` are placement counters
    (cumulative).  `limits`: other rejection limits than (100, 50) from the start state on — the guard's sensitivity runs.
    `outputs=False`: states and counters only, `ref` holds no per-step array (a large batch; oracle_range gives samples)."""
    cfg = case_cfg(kernel, regime)
    orc = ol.OracleVec(cfg, n, seed=ENV_SEED, threads=threads)
    out = dict(cfg=cfg, state0=orc.get_state(), obs0=orc.observe(), placed0=orc.placement_counters())
    f64, i32 = (a.copy() for a in out["state0"])
    inject_start_state(cfg, f64, i32)
    orc.set_state(f64, i32)
    if limits is not None:
        orc.set_placement_limits(*limits)
    act = pc.make_actions(cfg, HORIZON, n, seed=ACTION_SEED)
    out.update(f64=f64, i32=i32, act=act, ref=orc.rollout(act, want_final=True) if outputs else orc.rollout(act, light=True))
    out.update(state1=orc.get_state(), placed1=orc.placement_counters(), mask=reset_mask(n))
    out["obs2"] = orc.reset(out["mask"])
    out.update(state2=orc.get_state(), placed2=orc.placement_counters())
    orc.close()
    return out


# ---- the crowded tank: the forced RESPAWN of the 16-slot literal class ------------------------------------------------------
# After a capture with 16 foods there are 15 live foods and the swimmer: 16 discs of 80 px, 321.7k px^2, against a draw box of
# 670 x 470 = 314.9k px^2.  A snapshot may hold any layout (set_state), so the foods of slots 1..15 and the swimmer sit on a
# covering layout (found by hill climbing; it leaves CROWDED_OPEN of the box open), slot 0's food 3 px from the swimmer: the
# first step captures it and respawns with a rejection probability of 1 - CROWDED_OPEN per draw, so that about
# (1 - CROWDED_OPEN)^50 of the respawns end in the forced draw — in <16, 3, literal>, whose unpredicated form is the HALF tile
# variant.  Every 4th env captures nothing and starts on its last step without food: it is truncated and reset (limit 100) in
# the step in which its wavefront's other lanes respawn (limit 50).
CROWDED_KERNEL = (16, 3, 1)
CROWDED_LAYOUT = (      # [0]: the swimmer; [1..15]: the foods of slots 1..15 (px)
    (143.0, 134.7), (343.0, 119.3), (503.3, 118.4), (662.7, 135.3), (118.5, 274.8), (270.5, 227.5), (426.9, 243.0), (577.9, 240.4),
    (216.7, 358.8), (367.1, 354.8), (523.1, 370.9), (674.8, 322.9), (127.2, 459.7), (283.1, 478.6), (442.5, 480.3), (651.2, 466.8))
CROWDED_OPEN = 0.093    # crowded_open_share(): 0.907^50 = 0.8 % of the respawns are forced
CROWDED_UNPREDICATED = 4096                  # 64 whole wavefronts
CROWDED_ENVS = CROWDED_UNPREDICATED + N_PREDICATED
CROWDED_HORIZON = 3
CROWDED_TRUNCATE_EVERY = 4
# the oracle shows 27 forced of 3088 respawns (all 27 among the first 4096 envs), valid draws behind up to 49 rejections, 1030
# in-rollout resets and 65 (step, wavefront) pairs with both limits; the floors are about half
CROWDED_FLOORS = dict(respawn_forced=13, respawn_forced_unpredicated=13, respawn_valid=1500, resets=500, both_limits=32)


def crowded_truncating_lanes(n):
    return np.arange(n) % CROWDED_TRUNCATE_EVERY == 1


def crowded_open_share(step=2.0):
    """The share of the draw box farther than min_food_distance from every point of the layout (a grid of `step` px)."""
    cfg = case_cfg(CROWDED_KERNEL, "literal")
    lo = cfg.tank_margin + cfg.food_radius
    gx, gy = np.meshgrid(np.arange(lo, cfg.width - lo, step), np.arange(lo, cfg.height - lo, step))
    p = np.asarray(CROWDED_LAYOUT)
    d2 = (gx[..., None] - p[:, 0]) ** 2 + (gy[..., None] - p[:, 1]) ** 2
    return float((d2 >= cfg.min_food_distance ** 2).all(axis=-1).mean())


def run_crowded(n=CROWDED_ENVS, limits=None, threads=1):
    """The crowded recipe on the oracle; the keys of run_oracle() up to `placed1`."""
    cfg = case_cfg(CROWDED_KERNEL, "literal")
    F = cfg.num_food_items
    orc = ol.OracleVec(cfg, n, seed=ENV_SEED, threads=threads)
    out = dict(cfg=cfg, state0=orc.get_state(), placed0=orc.placement_counters())
    f64, i32 = (a.copy() for a in out["state0"])
    p = np.asarray(CROWDED_LAYOUT)
    f64[ol.F_X], f64[ol.F_Y] = p[0]
    for k in range(1, F):
        f64[ol.F_FOOD0 + k], f64[ol.F_FOOD0 + F + k] = p[k]
    trunc = crowded_truncating_lanes(n)
    ang = 0.7 * np.arange(n)
    # slot 0: 3 px from the swimmer; in the truncating lanes out of its reach, next to slot 1's food
    f64[ol.F_FOOD0] = np.where(trunc, p[1, 0] + 1.0, p[0, 0] + NEAR_FOOD_PX * np.cos(ang))
    f64[ol.F_FOOD0 + F] = np.where(trunc, p[1, 1] + 1.0, p[0, 1] + NEAR_FOOD_PX * np.sin(ang))
    i32[ol.I_STEPS_SINCE_FOOD] = np.where(trunc, cfg.max_steps_without_food, 0)
    orc.set_state(f64, i32)
    if limits is not None:
        orc.set_placement_limits(*limits)
    act = pc.make_actions(cfg, CROWDED_HORIZON, n, seed=ACTION_SEED)
    out.update(f64=f64, i32=i32, act=act, ref=orc.rollout(act, want_final=True))
    out.update(state1=orc.get_state(), placed1=orc.placement_counters())
    orc.close()
    return out


def crowded_events(run, lo=0, hi=None):
    """Respawns of the envs [lo, hi) by the way they ended, and the (step, wavefront) pairs with both limits."""
    grown = (run["placed1"] - run["placed0"])[:, lo:hi]
    ref = {k: run["ref"][k][:, lo:hi] for k in ("terminated", "truncated", "info")}
    return dict(respawn_placed=int(grown[ol.PC_RESPAWN_PLACED].sum()), respawn_forced=int(grown[ol.PC_RESPAWN_FORCED].sum()),
                reset_placed=int(grown[ol.PC_RESET_PLACED].sum()), reset_forced=int(grown[ol.PC_RESET_FORCED].sum()),
                resets=int((ref["terminated"] | ref["truncated"]).sum()), both_limits=both_limits(run["cfg"], ref))


def oracle_range(run, lo, hi):
    """The rollout outputs (with final_obs and info) of the envs [lo, hi) of a run, from an oracle of those envs alone: env
    i's trajectory depends on its global index, its start state and its actions only."""
    orc = ol.OracleVec(run["cfg"], hi - lo, seed=ENV_SEED, env_index_base=lo)
    orc.set_state(np.ascontiguousarray(run["f64"][:, lo:hi]), np.ascontiguousarray(run["i32"][:, lo:hi]))
    ref = orc.rollout(np.ascontiguousarray(run["act"][:, lo:hi]), want_final=True)
    f64, i32 = orc.get_state()
    assert np.array_equal(f64, run["state1"][0][:, lo:hi], equal_nan=True) and np.array_equal(i32, run["state1"][1][:, lo:hi])
    orc.close()
    return ref


def foods_present(cfg, state):
    """Foods per env of a snapshot (the NaN slots are empty)."""
    F = cfg.num_food_items
    return (~np.isnan(state[0][ol.F_FOOD0: ol.F_FOOD0 + F])).sum(axis=0)


def placement_events(run):
    """What the guard asserts, from the oracle's counters and outputs of run_oracle()."""
    cfg, ref = run["cfg"], run["ref"]
    ev = pc.count_events(ref)
    p0, p1, p2 = (run[k].sum(axis=1) for k in ("placed0", "placed1", "placed2"))
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    return dict(
        resets=int(done.sum()), respawns=ev["captures"] if cfg.respawn_food else 0, both_limits=both_limits(cfg, ref),
        twice=ev["twice"], wall=ev["wall"], truncated=ev["truncated"],
        reset_placed=int(p2[ol.PC_RESET_PLACED]), reset_forced=int(p2[ol.PC_RESET_FORCED]),
        initial_placed=int(p0[ol.PC_RESET_PLACED]), initial_forced=int(p0[ol.PC_RESET_FORCED]),
        rollout_reset_placed=int((p1 - p0)[ol.PC_RESET_PLACED]), rollout_reset_forced=int((p1 - p0)[ol.PC_RESET_FORCED]),
        masked_reset_placed=int((p2 - p1)[ol.PC_RESET_PLACED]), masked_reset_forced=int((p2 - p1)[ol.PC_RESET_FORCED]),
        respawn_placed=int(p2[ol.PC_RESPAWN_PLACED]), respawn_forced=int(p2[ol.PC_RESPAWN_FORCED]),
        max_valid_rejections=int(run["placed2"][ol.PC_MAX_VALID_REJECTIONS].max()))


def floors_for(kernel, regime):
    f = dict(MIN_FLOORS)
    if regime == "literal":      # no forced draw, and captures on the first step only: no floor on either
        f.update(both_limits=0, respawn_forced=0)
    f.update(FLOORS.get((kernel, regime), {}))
    return f
