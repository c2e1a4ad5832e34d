"""The shape x kernel matrix of the in-kernel GAUSSIAN policy, shared by tests/test_gpu_gaussian_matrix.py,
tests/test_gpu_robot_gaussian_matrix.py and their CPU guard tests/test_gaussian_matrix.py.  Needs numpy, the package's
configuration, `policy.GaussianPolicy` and the oracle bindings — no GPU library.  It follows tests/policy_matrix.py:
configurations and injected start states of tests/parity_cases.py, H = 64 compared steps behind one call of horizon 1,
128 envs (100 where the launch is predicated).

What the matrix is for: the log-std head that the device block lays out behind the mean head, and the noise draw of the
sampled kernels — every policy shape the ABI accepts (21) with one and with two action components, the shapes with
h0 != h1 in every one of the twenty K = 3 handle classes (two free-breathing multi-food classes among them that no policy
test ran), populations, the robot's 6 -> 3 policies — compared with `oracle_lib.policy_forward_gaussian`: the two heads
restated in C from the public layout, IEEE arithmetic only.  Behind the heads the kernel is held to `GaussianPolicy.sampling_stage`: the definition
evaluated from the restated heads, with the bound of the sampling arithmetic alone.

Weights are DENSE seeded normal draws, the log-std head included, all values of one policy distinct and non-zero.  The
log-std gain and biases keep every unclamped component's log_std inside (-20, 2) — in about [-4, 0.5] — and moving from
row to row; the clamp entries put exactly one component's bias beyond a clamp.  Seeds and gains were picked on the oracle
until every entry passes the guard: `PICKED` and `ROBOT_PICKED` below.
"""
import functools

import numpy as np

import oracle_lib as ol
import parity_cases as pc
import policy_matrix as pm
import robot_oracle_lib as rol
import robot_sampled_cases as rsc
import sampled_cases as sc
from policy_cases import drive_oracle
from underwater_swimmer_rl_amd.policy import LOG_STD_MAX, LOG_STD_MIN, GaussianPolicy, MLPPolicy

H = pm.H                            # compared steps per snake entry
UPDATE_STEPS = pm.UPDATE_STEPS
WAVE = pm.WAVE
KEY = pc.ENV_SEED                   # the snake handles' seed: the key of the noise stream
BASE = 2 ** 32 + 320                # env_index_base of the env-base runs: both counter words of the global index are used
MUTANT_ROWS, MUTANT_STEP_STRIDE = pm.MUTANT_ROWS, pm.MUTANT_STEP_STRIDE
NOT_BLIND = 0.25                    # of the visited rows, per action component, must be out of tanh saturation
LS_AIM = (-4.5, 1.0)                # where an unclamped log_std must stay (the aim is [-4, 0.5]; the hard limits are the clamps)
LS_MOVES = 0.1                      # ... and its standard deviation over the visited rows is at least this
CLAMP_MARGIN = 1.0                  # a clamped component's raw head is beyond its clamp by at least this on every row

# ------------------------------------------------------------------------------------------------ snake entries
# handle classes that tests/parity_cases.py does not have: name -> configuration, (slots, capacity, literal).  The first two
# are the free-breathing multi-food classes that no policy test ran; with the other seven every one of the twenty
# K = 3 handle classes (1, 4, 8, 12, 16 slots x literal / run-time constants x forced / free breathing) is in the matrix
EXTRA_CASES = {
    "free_F12": dict(preset="sac_gail", forced_breathing=False),
    "free_F16_other_tank": dict(preset="sac_gail", num_food_items=16, forced_breathing=False, width=900),
    "other_tank_F5": dict(preset="sac_gail", num_food_items=5, width=900),
    "free_other_tank_F1": dict(preset="single_food", forced_breathing=False, width=900),
    "free_F3": dict(preset="sac_gail", num_food_items=3, forced_breathing=False),
    "free_F3_other_tank": dict(preset="sac_gail", num_food_items=3, forced_breathing=False, width=900),
    "free_F5": dict(preset="sac_gail", num_food_items=5, forced_breathing=False),
    "free_F12_other_tank": dict(preset="sac_gail", forced_breathing=False, width=900),
    "free_F16": dict(preset="sac_gail", num_food_items=16, forced_breathing=False),
}
EXTRA_KERNEL = {"free_F12": (12, 3, 1), "free_F16_other_tank": (16, 3, 0), "other_tank_F5": (8, 3, 0), "free_other_tank_F1": (1, 3, 0),
                "free_F3": (4, 3, 1), "free_F3_other_tank": (4, 3, 0), "free_F5": (8, 3, 1), "free_F12_other_tank": (12, 3, 0),
                "free_F16": (16, 3, 1)}
FAMILY_SHAPES = ((128, (64, 64)), (128, (16, 64)), (100, (48, 32)))
POPULATIONS = tuple(p[:4] for p in pm.POPULATIONS)          # parity case, P, n, hidden
SEED0 = 9000
DEFAULTS = dict(gain=1.5, out_gain=1.5, ls_gain=0.5)
B_LS = {1: (-1.75,), 2: (-1.25, -2.25), 3: (-1.0, -1.75, -2.5)}     # the log-std biases of an entry without a clamp
CLAMP_HI, CLAMP_LO = 8.0, -28.0                                   # the bias of a component clamped by design
# name -> (component, bias): the clamp entries; exactly one component beyond a clamp, the others lively
SNAKE_CLAMPS = {"free_breathing-32x48-n128": (0, CLAMP_HI), "free_breathing-48x16-n128": (1, CLAMP_LO)}
# entries that are run once more with env_index_base = BASE: one per action width, one multi-food
BASE_ENTRIES = ("single_food-32x32-n128", "free_breathing-16x48-n128", "sac_gail_F12-64x64-n128")
WRAP_ENTRY, ROBOT_WRAP_ENTRY = "single_food-48x32-n128", "robot-16x64-n128"
# the comparison can fail: these entries are run with a mutant's WEIGHTS uploaded to the unchanged kernel
UPLOADED_MUTANTS = (("free_breathing-64x64-n128", "ls_chunk3_dropped"), ("free_breathing-32x16-n128", "ls_row1_takes_row0"),
                    ("other_tank_F5_free-16x64-n128", "ls_rows_at_stride_h0"))
# what was picked on the oracle: name -> (seed, hidden gain, mean gain, log-std gain).  The log-std gain is the one that
# gives the head a standard deviation of 0.1 .. 0.45 over the visited rows, two significant digits
PICKED = {
    "free_other_tank_F1-64x64-n128": (11680, 0.5, 1.0, 10.0),
    "other_tank_F5-64x64-n128": (9477, 0.7, 0.7, 3.1),
    "other_tank_F5-16x64-n128": (9278, 0.7, 0.7, 3.1),
    "other_tank_F5-48x32-n100": (9079, 0.7, 0.7, 4.2),
    "free_other_tank_F1-16x64-n128": (9281, 0.7, 0.7, 3.6),
    "free_other_tank_F1-48x32-n100": (9082, 0.7, 0.7, 3.2),
    "free_F3-64x64-n128": (9683, 0.5, 1.0, 7.9),
    "free_F3-16x64-n128": (9084, 0.7, 0.7, 4.2),
    "free_F3-48x32-n100": (9085, 0.7, 0.7, 2.4),
    "free_F3_other_tank-64x64-n128": (9086, 0.7, 0.7, 3.1),
    "free_F3_other_tank-16x64-n128": (9087, 0.7, 0.7, 3.0),
    "free_F3_other_tank-48x32-n100": (9288, 0.7, 0.7, 2.1),
    "free_F5-64x64-n128": (9289, 0.5, 0.5, 4.5),
    "free_F5-16x64-n128": (9090, 0.7, 0.7, 14.0),
    "free_F5-48x32-n100": (9091, 0.35, 1.0, 12.0),
    "free_F12_other_tank-64x64-n128": (9292, 0.35, 1.0, 17.0),
    "free_F12_other_tank-16x64-n128": (9093, 0.7, 0.7, 6.8),
    "free_F12_other_tank-48x32-n100": (9094, 0.7, 0.7, 5.8),
    "free_F16-64x64-n128": (9295, 0.7, 0.7, 2.9),
    "free_F16-16x64-n128": (9096, 0.7, 0.7, 2.2),
    "free_F16-48x32-n100": (9097, 0.7, 0.7, 2.9),
    "free_breathing-64x48-n128": (10640, 0.7, 0.7, 5.1),
    "single_food-48x32-n100": (10842, 0.7, 0.7, 3.8),
    "free_breathing-48x32-n100": (11643, 0.7, 0.7, 5.2),
    "single_food-linear-n128": (9000, 1.0, 1.0, 2.6),
    "single_food-16-n128": (9001, 1.0, 1.0, 6.8),
    "single_food-32-n128": (9202, 1.0, 1.0, 2.5),
    "single_food-48-n128": (9203, 0.7, 0.7, 2.4),
    "single_food-64-n128": (9004, 0.5, 0.5, 4.7),
    "single_food-16x16-n128": (9005, 1.0, 1.0, 3.9),
    "single_food-16x32-n128": (9006, 1.0, 1.0, 1.7),
    "single_food-16x48-n128": (9007, 0.7, 0.7, 10.0),
    "single_food-16x64-n128": (9008, 0.7, 0.7, 2.6),
    "single_food-32x16-n128": (9009, 1.0, 1.0, 3.3),
    "single_food-32x32-n128": (9010, 1.0, 1.0, 6.2),
    "single_food-32x48-n128": (9011, 0.7, 0.7, 6.8),
    "single_food-32x64-n128": (9412, 0.7, 0.7, 5.2),
    "single_food-48x16-n128": (9013, 0.7, 0.7, 10.0),
    "single_food-48x32-n128": (9014, 0.35, 1.0, 27.0),
    "single_food-48x48-n128": (9015, 0.7, 0.7, 4.0),
    "single_food-48x64-n128": (9016, 0.5, 1.0, 7.6),
    "single_food-64x16-n128": (9017, 0.7, 0.7, 4.0),
    "single_food-64x32-n128": (9018, 0.7, 0.7, 4.0),
    "single_food-64x48-n128": (9819, 0.7, 0.7, 3.2),
    "single_food-64x64-n128": (9020, 0.7, 0.7, 3.2),
    "free_breathing-linear-n128": (9021, 1.0, 1.0, 2.7),
    "free_breathing-16-n128": (9022, 1.0, 1.0, 3.7),
    "free_breathing-32-n128": (9023, 1.0, 1.0, 2.6),
    "free_breathing-48-n128": (9024, 0.7, 0.7, 5.6),
    "free_breathing-64-n128": (9025, 0.7, 0.7, 4.0),
    "free_breathing-16x16-n128": (9026, 0.7, 1.0, 3.3),
    "free_breathing-16x32-n128": (9227, 1.0, 1.0, 2.0),
    "free_breathing-16x48-n128": (9028, 0.7, 0.7, 5.5),
    "free_breathing-16x64-n128": (10029, 0.5, 0.5, 11.0),
    "free_breathing-32x16-n128": (9030, 1.0, 1.0, 6.7),
    "free_breathing-32x32-n128": (10431, 0.7, 1.0, 4.7),
    "free_breathing-32x48-n128": (10432, 0.35, 1.0, 14.0),
    "free_breathing-32x64-n128": (9233, 0.7, 0.7, 3.9),
    "free_breathing-48x16-n128": (10234, 0.7, 0.7, 5.1),
    "free_breathing-48x32-n128": (10435, 0.7, 0.7, 3.4),
    "free_breathing-48x48-n128": (9036, 0.7, 0.7, 3.5),
    "free_breathing-48x64-n128": (9037, 0.7, 0.7, 2.3),
    "free_breathing-64x16-n128": (9238, 0.7, 0.7, 2.6),
    "free_breathing-64x32-n128": (9839, 0.5, 1.0, 15.0),
    "free_breathing-64x64-n128": (9241, 0.5, 0.5, 11.0),
    "sac_gail_F12-64x64-n128": (9242, 0.35, 1.0, 18.0),
    "sac_gail_F12-16x64-n128": (9043, 0.7, 0.7, 4.3),
    "sac_gail_F12-48x32-n100": (9044, 0.7, 0.7, 2.8),
    "other_physics_F12-64x64-n128": (9045, 0.7, 0.7, 3.5),
    "other_physics_F12-16x64-n128": (9046, 0.7, 0.7, 6.1),
    "other_physics_F12-48x32-n100": (9047, 0.7, 0.7, 9.4),
    "no_respawn_F3-64x64-n128": (9048, 0.7, 0.7, 2.8),
    "no_respawn_F3-16x64-n128": (9049, 0.7, 0.7, 3.0),
    "no_respawn_F3-48x32-n100": (9050, 0.7, 0.7, 6.2),
    "F3_other_tank-64x64-n128": (9451, 0.7, 0.7, 2.0),
    "F3_other_tank-16x64-n128": (9052, 0.7, 0.7, 4.0),
    "F3_other_tank-48x32-n100": (9253, 0.7, 0.7, 8.9),
    "class_default_F5-64x64-n128": (10054, 0.7, 0.7, 2.8),
    "class_default_F5-16x64-n128": (9055, 0.7, 0.7, 4.8),
    "class_default_F5-48x32-n100": (9256, 0.7, 0.7, 4.1),
    "other_tank_F5_free-64x64-n128": (9857, 0.5, 0.5, 7.6),
    "other_tank_F5_free-16x64-n128": (9058, 0.7, 0.7, 3.3),
    "other_tank_F5_free-48x32-n100": (9059, 0.7, 0.7, 3.7),
    "F16_sixteen_slots-64x64-n128": (9060, 0.5, 1.0, 12.0),
    "F16_sixteen_slots-16x64-n128": (9061, 0.7, 0.7, 6.3),
    "F16_sixteen_slots-48x32-n100": (9462, 0.7, 0.7, 3.3),
    "F16_sixteen_slots_other_tank-64x64-n128": (9063, 0.5, 1.0, 6.2),
    "F16_sixteen_slots_other_tank-16x64-n128": (9064, 0.7, 0.7, 8.0),
    "F16_sixteen_slots_other_tank-48x32-n100": (9065, 0.7, 0.7, 3.8),
    "other_tank_F1-64x64-n128": (9666, 0.7, 0.7, 2.3),
    "other_tank_F1-16x64-n128": (9067, 0.7, 0.7, 5.3),
    "other_tank_F1-48x32-n100": (9068, 0.7, 0.7, 8.4),
    "free_F12-64x64-n128": (9869, 0.7, 0.7, 1.8),
    "free_F12-16x64-n128": (9270, 0.7, 0.7, 3.1),
    "free_F12-48x32-n100": (9471, 0.7, 0.7, 3.4),
    "free_F16_other_tank-64x64-n128": (9072, 0.7, 0.7, 3.0),
    "free_F16_other_tank-16x64-n128": (9073, 0.7, 0.7, 2.2),
    "free_F16_other_tank-48x32-n100": (9074, 0.5, 1.0, 6.0),
    "sac_gail_F12-48x32-n192-P3": (9075, 0.7, 0.7, 1.5),
    "free_breathing-16x64-n128-P2": (9276, 0.7, 0.7, 3.2),
    "single_food-linear-n256-P4": (9077, 1.0, 1.0, 1.6),
    "free_breathing-32x48-n128-clamp0hi": (9478, 0.7, 0.7, 4.7),
    "free_breathing-48x16-n128-clamp1lo": (9279, 0.7, 0.7, 13.0),
}


def case_spec(case):
    return pc.CASES[case] if case in pc.CASES else EXTRA_CASES[case]


def case_cfg(case):
    spec = dict(case_spec(case))
    spec.setdefault("max_steps_without_food", pc.DEFAULT_BUDGET)
    return pc.make_cfg(spec)


def case_kernel(case):
    slots, cap, literal = pc.EXPECT_KERNEL[case] if case in pc.EXPECT_KERNEL else EXTRA_KERNEL[case]
    assert cap == 3
    return slots, literal


def _name(case, hidden, n, P=1, clamp=None):
    s = f"{case}-{'x'.join(map(str, hidden)) or 'linear'}-n{n}" + (f"-P{P}" if P > 1 else "")
    return s + (f"-clamp{clamp[0]}{'hi' if clamp[1] > 0 else 'lo'}" if clamp else "")


def _entries():
    rows = [("single_food", 128, hidden, 1, None) for hidden in pm.SHAPES]          # all 21 shapes, one component
    rows += [("free_breathing", 128, hidden, 1, None) for hidden in pm.SHAPES]      # all 21 shapes, two components
    rows += [(case, 100, (48, 32), 1, None) for case in ("single_food", "free_breathing")]      # their predicated launch
    for case in pm.FAMILY_CASES + tuple(EXTRA_CASES):
        rows += [(case, n, hidden, 1, None) for n, hidden in FAMILY_SHAPES]
    rows += [(case, n, hidden, P, None) for case, P, n, hidden in POPULATIONS]
    for base, clamp in SNAKE_CLAMPS.items():
        case, shape, n = base.split("-")
        rows.append((case, int(n[1:]), tuple(int(v) for v in shape.split("x")), 1, clamp))
    table = {}
    for i, (case, n, hidden, P, clamp) in enumerate(rows):
        name = _name(case, hidden, n, P, clamp)
        seed, gain, out_gain, ls_gain = PICKED.get(name, (SEED0 + i, DEFAULTS["gain"], DEFAULTS["out_gain"], DEFAULTS["ls_gain"]))
        A = case_cfg(case).act_dim
        b_ls = list(B_LS[A])
        if clamp:
            b_ls[clamp[0]] = clamp[1]
        assert name not in table
        table[name] = dict(case=case, n=n, hidden=tuple(hidden), P=P, seed=seed, gain=gain, out_gain=out_gain, ls_gain=ls_gain,
                           b_ls=tuple(b_ls), clamped=(clamp[0],) if clamp else (), kernel=case_kernel(case), predicated=n % WAVE != 0)
    return table


# ------------------------------------------------------------------------------------------------ robot entries (6 -> 3)
ROBOT_H, ROBOT_MAX_CYCLES, ROBOT_SEED = 7, 3, rsc.SEED
ROBOT_SHAPES = ((), (16,), (64,), (16, 64), (48, 32), (64, 64))
ROBOT_CLAMP = ("robot-64-n128", (1, CLAMP_LO))
ROBOT_CLIP_SHAPES = ((), (16, 64), (48, 32))               # deterministic `clip` policies: bit for bit with the restatement
ROBOT_DEFAULTS = dict(gain=0.25, out_gain=1.0, ls_gain=0.3)
ROBOT_SEED0 = 9500
ROBOT_PICKED = {
    "robot-linear-n128-clip": (9508, 0.25, 2.0, 0.3),      # (the clip entries have no log-std head: their last figure is unused)
    "robot-16x64-n128-clip": (9709, 2.0, 2.0, 0.3),
    "robot-48x32-n100-clip": (9510, 1.0, 4.0, 0.3),
    "robot-linear-n128": (9500, 0.25, 1.0, 0.13),
    "robot-16-n128": (9701, 0.1, 1.0, 3.9),
    "robot-64-n128": (9502, 0.25, 1.0, 2.2),
    "robot-16x64-n128": (9503, 0.25, 1.0, 14.0),
    "robot-48x32-n100": (9504, 0.25, 1.0, 7.5),
    "robot-64x64-n128": (9505, 0.25, 1.0, 5.0),
    "robot-16x64-n128-P2": (9706, 0.25, 1.0, 4.3),
    "robot-64-n128-clamp1lo": (9507, 0.25, 1.0, 0.99),
}


def _robot_entries():
    rows = [(hidden, 100 if hidden == (48, 32) else 128, 1, None, "gaussian") for hidden in ROBOT_SHAPES]
    rows.append(((16, 64), 128, 2, None, "gaussian"))
    rows.append(((64,), 128, 1, ROBOT_CLAMP[1], "gaussian"))
    rows += [(hidden, 100 if hidden == (48, 32) else 128, 1, None, "clip") for hidden in ROBOT_CLIP_SHAPES]
    table = {}
    for i, (hidden, n, P, clamp, kind) in enumerate(rows):
        name = _name("robot", hidden, n, P, clamp) + ("-clip" if kind == "clip" else "")
        d = ROBOT_DEFAULTS
        seed, gain, out_gain, ls_gain = ROBOT_PICKED.get(name, (ROBOT_SEED0 + i, d["gain"], d["out_gain"], d["ls_gain"]))
        b_ls = list(B_LS[3])
        if clamp:
            b_ls[clamp[0]] = clamp[1]
        table[name] = dict(case="robot", n=n, hidden=tuple(hidden), P=P, seed=seed, gain=gain, out_gain=out_gain, ls_gain=ls_gain,
                           b_ls=tuple(b_ls), clamped=(clamp[0],) if clamp else (), kind=kind, predicated=n % WAVE != 0)
    return table


ENTRIES = _entries()
ROBOT_ENTRIES = _robot_entries()
ROBOT_GAUSSIAN = [k for k, e in ROBOT_ENTRIES.items() if e["kind"] == "gaussian"]
ROBOT_CLIP = [k for k, e in ROBOT_ENTRIES.items() if e["kind"] == "clip"]
ALL = {**ENTRIES, **ROBOT_ENTRIES}
assert all(k in ENTRIES for k in PICKED) and all(k in ROBOT_ENTRIES for k in ROBOT_PICKED)
assert all(k in ENTRIES for k in BASE_ENTRIES + (WRAP_ENTRY,)) and ROBOT_WRAP_ENTRY in ROBOT_ENTRIES
assert all(k in ENTRIES for k, _ in UPLOADED_MUTANTS)


# ------------------------------------------------------------------------------------------------ policies
def dense_gaussian(obs_dim, act_dim, hidden, seed, gain, out_gain, ls_gain, b_ls, scale, shift):
    """One Gaussian policy with dense weights, as `policy_matrix.dense_policy` draws them: N(0, 1) * gain / sqrt(fan_in)
    (`out_gain` for the mean head, `ls_gain` for the log-std head), biases N(0, 1) * 0.1; the log-std biases are `b_ls`.
    A value that occurs twice in the policy is drawn again until all are distinct and non-zero."""
    rng = np.random.default_rng(seed)
    widths = (obs_dim,) + tuple(hidden) + (act_dim,)
    sigma = []
    for li in range(len(widths) - 1):
        d, h = widths[li], widths[li + 1]
        g = out_gain if li == len(hidden) else gain
        sigma += [np.full(h * d, g / np.sqrt(d)), np.full(h, 0.1)]
    d = widths[-2]
    sigma.append(np.full(act_dim * d, ls_gain / np.sqrt(d)))
    sigma = np.concatenate(sigma)
    fixed = np.concatenate([np.asarray(b_ls, np.float32), np.asarray(scale, np.float32), np.asarray(shift, np.float32)])
    assert np.unique(fixed[:act_dim]).size == act_dim and (fixed[:act_dim] != 0).all()     # (the robot's Box has a shift of 0)
    flat = (rng.standard_normal(sigma.size) * sigma).astype(np.float32)
    while True:
        _, first = np.unique(flat, return_index=True)
        again = np.ones(flat.size, bool)
        again[first] = False
        again |= (flat == 0) | np.isin(flat, fixed)
        if not again.any():
            break
        flat[again] = (rng.standard_normal(int(again.sum())) * sigma[again]).astype(np.float32)
    layers, o = [], 0
    for li in range(len(widths) - 1):
        d, h = widths[li], widths[li + 1]
        layers.append((flat[o:o + h * d].reshape(h, d), flat[o + h * d:o + h * d + h]))
        o += h * d + h
    d = widths[-2]
    W_ls = flat[o:o + act_dim * d].reshape(act_dim, d)
    return GaussianPolicy.from_layers(layers, (W_ls, np.asarray(b_ls, np.float32)), np.asarray(scale, np.float32), np.asarray(shift, np.float32))


def is_robot(name):
    return name in ROBOT_ENTRIES


def entry_cfg(name):
    return case_cfg(ENTRIES[name]["case"])


def entry_policies(name, generation=0):
    """The entry's P policies; `generation=1`: the second weight set of the same shape (for policy_update)."""
    e = ALL[name]
    if is_robot(name):
        od, ad, scale, shift = 6, 3, rsc.SCALE, rsc.SHIFT
    else:
        cfg = entry_cfg(name)
        od, ad, scale, shift = cfg.obs_dim, cfg.act_dim, pm.SCALE[cfg.act_dim], pm.SHIFT[cfg.act_dim]
    ps = [dense_gaussian(od, ad, e["hidden"], e["seed"] + 100000 * generation + 1000 * k, e["gain"], e["out_gain"], e["ls_gain"],
                         tuple(b + 0.125 * k + 0.0625 * generation for b in e["b_ls"]), scale, shift) for k in range(e["P"])]
    if e.get("kind") == "clip":      # the robot's deterministic entries: the same body and mean head behind a clamp to [-1, 1]
        ps = [MLPPolicy(p.layers, p.scale, p.shift, "clip") for p in ps]
    return ps


def entry_policy(name, generation=0):
    ps = entry_policies(name, generation)
    return ps[0] if len(ps) == 1 else type(ps[0]).stack(ps)


def key_of(name):
    """The seed of the entry's handles: the key of its noise stream."""
    return ROBOT_SEED if is_robot(name) else KEY


def local_index_share(policy, seen, actions, n0, key):
    """Share of the action entries (components at the lower clamp aside) that lie more than `sampled_cases.OFF_BY_ONE_BOUNDS`
    bounds from the definition evaluated with the noise of the LOCAL env index 0 .. n - 1."""
    Hh, n = actions.shape[:2]
    z_wrong = noise(policy, n, n0, Hh, key, 0)
    want, _ = policy.reference(seen, z_wrong)
    bound, _ = policy.error_bound(seen, z_wrong)
    keep = np.setdiff1d(np.arange(policy.act_dim), sc.floor_clamped_components(policy))
    far = np.abs(np.asarray(actions, np.float64) - want) > sc.OFF_BY_ONE_BOUNDS * bound
    return float(far[..., keep].mean())


def noise(policy, n, n0, horizon, key, base=0):
    """z float64 [horizon, n, act_dim]: step t of a call that starts at noise step n0 draws the blocks of (base + env, n0 + t)."""
    return sc.case_noise(policy, n, n0, horizon, key, base)


# ------------------------------------------------------------------------------------------------ the restatement and the stage
def restated(policy, seen):
    """The two heads of the restatement on the rows `seen` [..., N, obs_dim]: m, r float32 — with no subnormal on the way."""
    m, r, sub = ol.policy_forward_gaussian(policy, seen)
    assert sub == 0, f"{sub} subnormal intermediates"
    return m, r


def stage(policy, m, r, z):
    """`GaussianPolicy.sampling_stage` as a dict: a, lp (float64 values from the given heads), ea, el (the stage bounds)."""
    a, lp, ea, el = policy.sampling_stage(m, r, z)
    return dict(a=a, lp=lp, ea=ea, el=el)


def assert_is_the_stage(label, policy, seen, out, z):
    """Actions and logp of `out` within the stage bound of the restated heads on `seen` under the noise z, and within
    `error_bound` of the float64 reference.  Prints and returns the four largest error / bound ratios."""
    assert not np.isnan(out["actions"]).any() and not np.isnan(out["logp"]).any()
    m, r = restated(policy, seen)
    s = stage(policy, m, r, z)
    a, lp = out["actions"].astype(np.float64), out["logp"].astype(np.float64)
    sa, sl = np.abs(a - s["a"]) / s["ea"], np.abs(lp - s["lp"]) / s["el"]
    (wa, wl), (ea, el) = policy.reference(seen, z), policy.error_bound(seen, z)
    fa, fl = np.abs(a - wa) / ea, np.abs(lp - wl) / el
    print(f"{label}: error / stage bound: action {sa.max():.4f}, logp {sl.max():.4f} (bounds up to {s['ea'].max():.3g}, {s['el'].max():.3g}); "
          f"error / error_bound: action {fa.max():.4f}, logp {fl.max():.4f} (bounds up to {ea.max():.3g}, {el.max():.3g})")
    ia, il = np.unravel_index(sa.argmax(), sa.shape), np.unravel_index(sl.argmax(), sl.shape)
    assert (sa <= 1.0).all(), (f"{label}: {int((sa > 1).sum())} actions outside the stage bound, worst ratio {sa.max()} at {ia}: "
                               f"m {m[ia]!r}, r {r[ia]!r}, z {z[ia]!r}, got {out['actions'][ia]!r}, want {s['a'][ia]!r}")
    assert (sl <= 1.0).all(), (f"{label}: {int((sl > 1).sum())} logp outside the stage bound, worst ratio {sl.max()} at {il}: "
                               f"m {m[il]!r}, r {r[il]!r}, z {z[il]!r}, got {out['logp'][il]!r}, want {s['lp'][il]!r}")
    assert (fa <= 1.0).all() and (fl <= 1.0).all(), f"{label}: outside error_bound, worst ratios {fa.max()}, {fl.max()}"
    return float(sa.max()), float(sl.max()), float(fa.max()), float(fl.max())


def outside(got_a, got_lp, s):
    """Rows [...] whose action (any component) or log-probability is outside the stage bound of `s`."""
    return (np.abs(np.asarray(got_a, np.float64) - s["a"]) > s["ea"]).any(axis=-1) | (np.abs(np.asarray(got_lp, np.float64) - s["lp"]) > s["el"])


def certainly_outside(s0, s1):
    """Rows on which a correct fp32 evaluation of `s1` (anywhere within ITS stage bound) is outside the stage bound of `s0`."""
    return ((np.abs(s1["a"] - s0["a"]) > s0["ea"] + s1["ea"]).any(axis=-1)) | (np.abs(s1["lp"] - s0["lp"]) > s0["el"] + s1["el"])


# ------------------------------------------------------------------------------------------------ start states and oracle runs
def start_snapshot(name, base=0, n=None):
    """cfg and the injected start state of a snake entry (`n`: another env count), its envs at global indices base .."""
    e, cfg = ENTRIES[name], entry_cfg(name)
    orc = ol.OracleVec(cfg, n or e["n"], seed=KEY, env_index_base=base)
    f64, i32 = orc.get_state()
    orc.close()
    pc.inject_start_state(cfg, f64, i32)
    return e, cfg, f64, i32


@functools.lru_cache(maxsize=None)
def oracle_closed_loop(name, base=0):
    """The oracle stepped closed-loop under `reference(obs, z)` rounded to float32 from the injected start state and noise
    step 0: computed once, shared, read-only."""
    e, cfg, f64, i32 = start_snapshot(name, base)
    policy, n = entry_policy(name), e["n"]
    z = noise(policy, n, 0, H, KEY, base)
    orc = ol.OracleVec(cfg, n, seed=KEY, env_index_base=base)
    orc.set_state(f64, i32)

    def act(t, o):
        a, lp = policy.reference(o, z[t])
        return a.astype(np.float32), lp
    obs_in, actions, outs, logp = drive_oracle(orc, H, act)
    orc.close()
    return _closed(e, cfg, policy, z, obs_in, actions, np.array(logp), outs)


def _closed(e, cfg, policy, z, obs_in, actions, logp, outs):
    m, r, sub = ol.policy_forward_gaussian(policy, obs_in)
    for arr in (z, obs_in, actions, logp, m, r, *outs.values()):
        arr.setflags(write=False)
    return dict(e=e, cfg=cfg, policy=policy, z=z, obs_in=obs_in, actions=actions, logp=logp, outs=outs, m=m, r=r, subnormals=sub)


def robot_first_action(n, first=0):
    """The one step every robot entry takes before its compared run: contraction 0.5, coast 0.75 s, yaw by env (`first`:
    the position of this handle's env 0 in a larger batch, for shards)."""
    a = np.empty((n, 3), np.float32)
    a[:, 0], a[:, 1], a[:, 2] = 0.5, 0.075, (np.arange(first, first + n) % 7 - 3) / 4.0
    return a


def robot_reset_mask(n, first=0):
    """Every third robot is reset behind that step: with max_cycles = 3 the two cohorts are truncated on different steps, so
    every wavefront mixes finished and unfinished lanes."""
    return (np.arange(first, first + n) % 3 == 0).astype(np.uint8)


def robot_oracle_cfg():
    c = rol.default_robot_config()
    c.max_cycles = ROBOT_MAX_CYCLES
    return c


@functools.lru_cache(maxsize=None)
def robot_closed_loop(name, base=0):
    """The robot oracle (max_cycles = 3) after the staggering step and masked reset, stepped closed-loop under
    `reference(obs, z)` rounded to float32 from noise step 0: computed once, shared, read-only."""
    e, policy = ROBOT_ENTRIES[name], entry_policy(name)
    n = e["n"]
    z = noise(policy, n, 0, ROBOT_H, ROBOT_SEED, base)
    orc = rol.RobotOracleVec(n, seed=ROBOT_SEED, env_index_base=base, cfg=robot_oracle_cfg())
    orc.reset(np.zeros(n, np.uint8))
    orc.step(robot_first_action(n))
    o = orc.reset(robot_reset_mask(n))
    obs_in, actions, logp = np.empty((ROBOT_H, n, 6), np.float32), np.empty((ROBOT_H, n, 3), np.float32), np.empty((ROBOT_H, n))
    outs = dict(obs=np.empty((ROBOT_H, n, 6), np.float32), terminated=np.empty((ROBOT_H, n), np.uint8),
                truncated=np.empty((ROBOT_H, n), np.uint8), inner_steps=np.empty((ROBOT_H, n), np.int32))
    for t in range(ROBOT_H):
        obs_in[t] = o
        a, logp[t] = policy.reference(o, z[t])
        actions[t] = a.astype(np.float32)
        s = orc.step(actions[t])
        for k in outs:
            outs[k][t] = s[k]
        o = s["obs"]
    orc.close()
    return _closed(e, None, policy, z, obs_in, actions, logp, outs)


@functools.lru_cache(maxsize=None)
def robot_clip_closed_loop(name):
    """A deterministic `clip` entry on the robot oracle, stepped under the C restatement `oracle_lib.policy_forward`."""
    e, policy = ROBOT_ENTRIES[name], entry_policy(name)
    n = e["n"]
    orc = rol.RobotOracleVec(n, seed=ROBOT_SEED, cfg=robot_oracle_cfg())
    orc.reset(np.zeros(n, np.uint8))
    orc.step(robot_first_action(n))
    o = orc.reset(robot_reset_mask(n))
    obs_in, u, sub = np.empty((ROBOT_H, n, 6), np.float32), np.empty((ROBOT_H, n, 3), np.float32), 0
    done = np.empty((ROBOT_H, n), np.uint8)
    for t in range(ROBOT_H):
        obs_in[t] = o
        u[t], a, s_ = ol.policy_forward(policy, o)
        sub += s_
        s = orc.step(a)
        o, done[t] = s["obs"], s["terminated"] | s["truncated"]
    orc.close()
    return dict(e=e, policy=policy, obs_in=obs_in, u=u, subnormals=sub, outs=dict(terminated=done, truncated=np.zeros_like(done)))


def closed_loop(name, base=0):
    return robot_closed_loop(name, base) if is_robot(name) else oracle_closed_loop(name, base)


def mixed_wave_steps(outs):
    """(step, wavefront) pairs in which some lanes finish and others do not."""
    done = (outs["terminated"] | outs["truncated"]).astype(bool)
    Hh, n = done.shape
    w = n // WAVE * WAVE
    per_wave = done[:, :w].reshape(Hh, -1, WAVE).sum(axis=2)
    return int(done.sum()), int(((per_wave > 0) & (per_wave < WAVE)).sum())


def ceilings(name):
    """(action bound ceiling, logp bound ceiling) of the entry: the project's, of the respective cases module."""
    mod, A = (rsc, 3) if is_robot(name) else (sc, entry_cfg(name).act_dim)
    return mod.BOUND_CEILING, A * mod.LOGP_BOUND_CEILING_PER_COMPONENT


# ------------------------------------------------------------------------------------------------ the guard's mutants
def gaussian_layout(policy):
    """Offsets in the public Gaussian words of one policy: W_mu, b_mu, W_ls, b_ls, and (A, in) of the heads."""
    o, d = 0, policy.obs_dim
    for h in policy.hidden:
        o += h * d + h
        d = h
    A = policy.act_dim
    return dict(W_mu=o, b_mu=o + A * d, W_ls=o + A * d + A, b_ls=o + 2 * A * d + A, A=A, d=d)


def weight_mutants(policy):
    """name -> (public Gaussian weights [P, words] with the LOG-STD head re-indexed the way a wrong device map or a wrong
    stride in the kernel would read it, the action components the mutant touches); only those that apply to the shape."""
    w0 = policy.pack()
    L = gaussian_layout(policy)
    A, d, Wm, bm, Wl, bl = L["A"], L["d"], L["W_mu"], L["b_mu"], L["W_ls"], L["b_ls"]
    words, hid = policy.words, policy.hidden
    every = tuple(range(A))
    out = {}

    def mutant(name, touches=every):
        w = w0.copy()
        out[name] = (w, tuple(touches))
        return w

    def columns(which):
        return np.array([Wl + j * d + i for j in range(A) for i in which])
    for c in range((d + 15) // 16):                     # each chunk of 16 inputs never reaches the log-std head
        mutant(f"ls_chunk{c}_dropped")[:, columns(range(16 * c, min(16 * c + 16, d)))] = 0.0
    swaps = [("ls_two_weights_swapped_within_16", 1, 2)] + ([("ls_two_weights_swapped_16_apart", 2, 18)] if d > 16 else [])
    for label, i, k in swaps:                           # in every row, so that no clamp hides it
        m = mutant(label)
        m[:, columns([i])], m[:, columns([k])] = w0[:, columns([k])], w0[:, columns([i])]
    for k in range(1, A):
        mutant(f"ls_row{k}_takes_row{k - 1}", (k,))[:, Wl + k * d:Wl + (k + 1) * d] = w0[:, Wl + (k - 1) * d:Wl + k * d]
        mutant(f"b_ls{k}_takes_b_ls{k - 1}", (k,))[:, bl + k] = w0[:, bl + k - 1]
    mutant("ls_head_takes_W_mu")[:, Wl:Wl + A * d] = w0[:, Wm:Wm + A * d]
    mutant("ls_head_takes_b_mu")[:, bl:bl + A] = w0[:, bm:bm + A]
    if len(hid) == 2 and hid[0] != hid[1] and A >= 2:   # rows read at stride h0 instead of h1
        j, i = np.meshgrid(np.arange(A), np.arange(d), indexing="ij")
        mutant("ls_rows_at_stride_h0", range(1, A))[:, (Wl + j * d + i).ravel()] = w0[:, ((Wl + j * hid[0] + i) % words).ravel()]
    if policy.n_policies > 1:                           # policy k takes policy k - 1's log-std head alone
        m = mutant("policy_k_takes_policy_k_minus_1_ls_head")
        m[:, Wl:Wl + A * d], m[:, bl:bl + A] = np.roll(w0[:, Wl:Wl + A * d], 1, axis=0), np.roll(w0[:, bl:bl + A], 1, axis=0)
    return out


def noise_mutants(policy, n, n0, horizon, key, base=0):
    """name -> (z [horizon, n, A] of a wrong noise definition, the components it touches); only those that apply."""
    A = policy.act_dim
    z = noise(policy, n, n0, horizon, key, base)
    out = {"noise_step_plus_1": (noise(policy, n, n0 + 1, horizon, key, base), tuple(range(A)))}
    if A >= 2:                                          # component 1 from words (0, 1): component 0's draw
        zz = z.copy()
        zz[..., 1] = z[..., 0]
        out["component1_from_words_0_1"] = (zz, (1,))
    if A == 3:                                          # component 2 from the first two words of the stream-3 block
        zz = z.copy()
        zz[..., 2] = z[..., 0]
        out["component2_from_stream_3"] = (zz, (2,))
    if base:
        out["local_env_index"] = (noise(policy, n, n0, horizon, key, 0), tuple(range(A)))
    return out


def mutant_rows(name, base=0):
    """label -> (rows of those tried on which the mutant is certainly outside the stage bound, exempt): every 4th step's rows
    of the oracle's closed loop (all of the robot's 7 steps).  A mutant is exempt only where every component it touches is
    one the entry clamps by design."""
    r = closed_loop(name, base)
    policy, e = r["policy"], r["e"]
    stride = 1 if is_robot(name) else MUTANT_STEP_STRIDE
    seen, z, m, rr = r["obs_in"][::stride], r["z"][::stride], r["m"][::stride], r["r"][::stride]
    s0 = stage(policy, m, rr, z)
    shown = {}
    for label, (w, touches) in weight_mutants(policy).items():
        assert w.shape == policy.pack().shape and not np.array_equal(w, policy.pack()), label
        mm, rm, _ = ol.policy_forward_gaussian(policy, seen, weights=w)
        assert np.array_equal(mm, m), f"{label} is a mutant of the log-std head alone"
        shown[label] = (int(certainly_outside(s0, stage(policy, mm, rm, z)).sum()), set(touches) <= set(e["clamped"]))
    Hh = r["z"].shape[0]
    for label, (zz, touches) in noise_mutants(policy, e["n"], 0, Hh, ROBOT_SEED if is_robot(name) else KEY, base).items():
        shown[label] = (int(certainly_outside(s0, stage(policy, m, rr, zz[::stride])).sum()), set(touches) <= set(e["clamped"]))
    return shown, seen.shape[0] * seen.shape[1]


def expected_mutants(name, base=0):
    e = ALL[name]
    A = 3 if is_robot(name) else entry_cfg(name).act_dim
    hid = e["hidden"]
    d = hid[-1] if hid else (6 if is_robot(name) else 24)
    want = {f"ls_chunk{c}_dropped" for c in range((d + 15) // 16)}
    want |= {"ls_two_weights_swapped_within_16", "ls_head_takes_W_mu", "ls_head_takes_b_mu", "noise_step_plus_1"}
    if d > 16:
        want.add("ls_two_weights_swapped_16_apart")
    for k in range(1, A):
        want |= {f"ls_row{k}_takes_row{k - 1}", f"b_ls{k}_takes_b_ls{k - 1}"}
    if len(hid) == 2 and hid[0] != hid[1] and A >= 2:
        want.add("ls_rows_at_stride_h0")
    if e["P"] > 1:
        want.add("policy_k_takes_policy_k_minus_1_ls_head")
    if A >= 2:
        want.add("component1_from_words_0_1")
    if A == 3:
        want.add("component2_from_stream_3")
    if base:
        want.add("local_env_index")
    return want


def guard(name, base=0):
    """Everything the CPU guard asserts of one Gaussian entry, measured on the oracle: (figures, list of failures)."""
    r = closed_loop(name, base)
    e, policy, z, obs_in = r["e"], r["policy"], r["z"], r["obs_in"]
    A = policy.act_dim
    fails = []
    ends, mixed = mixed_wave_steps(r["outs"])
    if ends < 1 or mixed < 1:
        fails.append(f"episodes: {ends} endings, {mixed} mixed wavefront-steps")
    if r["subnormals"]:
        fails.append(f"{r['subnormals']} subnormals")
    ea, el = policy.error_bound(obs_in, z)
    cap_a, cap_l = ceilings(name)
    if not (ea.max() < cap_a and el.max() < cap_l):
        fails.append(f"error_bound {ea.max():.3g} (ceiling {cap_a}), logp {el.max():.3g} (ceiling {cap_l})")
    s = stage(policy, r["m"], r["r"], z)
    if not ((s["ea"] <= ea).all() and (s["el"] <= el).all()):
        fails.append("a stage bound above error_bound")
    ra, rl = policy.reference(obs_in, z)            # the restated heads give the float64 definition, within its forward bound
    if not ((np.abs(s["a"] - ra) <= ea).all() and (np.abs(s["lp"] - rl) <= el).all()):
        fails.append("the restated heads are not the float64 reference within error_bound")
    m64, r64 = r["m"].astype(np.float64), r["r"].astype(np.float64)
    u = m64 + np.exp(np.clip(r64, LOG_STD_MIN, LOG_STD_MAX)) * z
    open_ = (np.abs(np.tanh(u)) < 0.999).reshape(-1, A).mean(axis=0)
    if not (open_ >= NOT_BLIND).all():
        fails.append(f"unsaturated share {np.round(open_, 3).tolist()}")
    ls = r64.reshape(-1, A)
    lively = [k for k in range(A) if k not in e["clamped"]]
    for k in lively:
        if not (LOG_STD_MIN < ls[:, k].min() and ls[:, k].max() < LOG_STD_MAX and LS_AIM[0] < ls[:, k].min()
                and ls[:, k].max() < LS_AIM[1] and ls[:, k].std() >= LS_MOVES):
            fails.append(f"log_std[{k}] in [{ls[:, k].min():.3g}, {ls[:, k].max():.3g}], std {ls[:, k].std():.3g}")
    for k in e["clamped"]:
        b = e["b_ls"][k]
        beyond = ls[:, k].min() > LOG_STD_MAX + CLAMP_MARGIN if b > 0 else ls[:, k].max() < LOG_STD_MIN - CLAMP_MARGIN
        if not beyond:
            fails.append(f"clamped log_std[{k}] in [{ls[:, k].min():.3g}, {ls[:, k].max():.3g}]")
    shown, tried = mutant_rows(name, base)
    if set(shown) != expected_mutants(name, base):
        fails.append(f"mutants {sorted(set(shown) ^ expected_mutants(name, base))}")
    low = {k: v for k, (v, exempt) in shown.items() if v < MUTANT_ROWS and not exempt}
    if low:
        fails.append(f"mutants below {MUTANT_ROWS} rows: {low}")
    figures = dict(endings=ends, mixed=mixed, bound=float(ea.max()), logp_bound=float(el.max()), stage=float(s["ea"].max()),
                   logp_stage=float(s["el"].max()), unsaturated=np.round(open_, 3).tolist(),
                   ls=[(round(float(ls[:, k].min()), 2), round(float(ls[:, k].max()), 2)) for k in range(A)],
                   tried=tried, mutants={k: (f"{v} (exempt)" if ex else v) for k, (v, ex) in shown.items()})
    return figures, fails
