"""What the robot library derives or refuses on the host, checked without a GPU.  csrc/salp_robot_params.h writes the
constants of the breathing cycle once, lists the physical parameters once (SALP_ROBOT_PHYS) and holds every function that
salp_robot_vec_create, salp_robot_vec_step_history and salp_robot_vec_trajectory run before they launch; it compiles as
plain C++ (tests/robot_params_host.cpp).  A wrong robot_max_steps or history_capacity is an out-of-bounds history write on
the device, so the expectations here are written from the reference's formulas as oracle/salp_robot_oracle.c states them
(env_reset, env_step), not taken from the code under test."""
import ctypes
import glob
import math
import os
import re

import numpy as np
import pytest

import robot_params_host_lib as rp
from underwater_swimmer_rl_amd.robot_compare import ROBOT_PARAM_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc")
SALP_OK, SALP_ERR_INVALID = 0, -1
TINY = 5e-324      # the smallest positive double
T_MAX = 14.6       # the cycle-length cut of include/salp_robot.h, s
MAX_STEPS = 1461   # Euler steps of the longest cycle at dt = 0.01


@pytest.fixture(scope="module")
def default():
    return rp.default_config()


# ---- defaults and constants
def test_default_config_is_the_documented_one(default):
    """Every field has the value written beside it in include/salp_robot.h."""
    from underwater_swimmer_rl_amd._capi import CRobotConfig
    assert default.struct_size == ctypes.sizeof(CRobotConfig) == rp.config_sizeof()
    assert default.reserved0 == 0
    want = dict(width=900, height=700, tank_margin=50.0, dry_mass=1.0, init_length=0.3, init_width=0.15, max_contraction=0.06,
                density=1000.0, dt=0.01, drag_coefficient_min=0.4, drag_coefficient_max=1.0, nozzle_length1=0.05,
                nozzle_length2=0.05, nozzle_length3=0.05, nozzle_area=0.00016, nozzle_mass=1.0, nozzle_gamma=math.pi / 4,
                max_cycles=500)
    assert set(want) | {"struct_size", "reserved0"} == {f for f, _ in CRobotConfig._fields_}
    for name, v in want.items():
        assert getattr(default, name) == v, name        # == on floats: bit for bit (no field is NaN or -0.0)


def test_constants_have_the_reference_values():
    """_rescale_action (salp_robot_env.py:129-137) and set_control's rates (robot.py:767, 776), as the literals fold."""
    c = rp.constants()
    assert c == dict(kPi=math.pi, kActContraction=0.06, kActCoast=10.0, kActYaw=math.pi / 2, kContractRate=0.06 / 3,
                     kReleaseRate=0.06 / 1.5, kMaxCycleTime=T_MAX, kSchedBins=256.0, kMaxHistorySteps=float(2 ** 24))


def test_the_literals_are_written_once():
    """The cut is defined in one place, the ABI file holds no device code, and no kernel compares SALP_RP_ rows by hand."""
    hits = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            hits += [(os.path.basename(path), line.strip()) for line in f if "14.6" in line]
    assert hits == [("salp_robot_params.h", "constexpr double kMaxCycleTime = 14.6;")], hits
    with open(os.path.join(CSRC, "salp_robot.hip")) as f:
        abi = f.read()
    assert "__global__" not in abi and "__device__" not in abi
    with open(os.path.join(CSRC, "salp_robot_kernels.h")) as f:
        kernels = f.read()
    assert not re.search(r"SALP_RP_\w+\s*==", kernels) and "SALP_ROBOT_PHYS(SALP_ROBOT_PHYS_LOAD)" in kernels


# ---- the list of physical parameters
def test_the_list_is_the_public_parameter_table():
    rows = rp.phys_list()
    fields = [f for f, _, _, _ in rows]
    assert tuple(fields) == ROBOT_PARAM_NAMES      # tests/test_robot_trajectory.py ties these to the SALP_RP_* enum
    assert [r for _, r, _, _ in rows] == ["SALP_RP_" + f.upper() for f in fields]
    assert [v for _, _, v, _ in rows] == list(range(len(rows)))
    members = [m for _, _, _, m in rows]
    assert len(set(members)) == len(members)
    for absent in ("nozzle_length3", "dt", "tank_margin", "width", "height", "max_cycles"):
        assert absent not in fields and absent not in members


# ---- make_robot_params
@pytest.mark.parametrize("w,h,m", [(900, 700, 50.0), (901, 701, 49.5), (2, 2, 0.0), (400, 300, 250.0)])
def test_the_target_range_is_the_reference_formula(default, w, h, m):
    """oracle env_reset: x_min = (-(double)width / 2 + margin) / 200, x_max = ((double)width / 2 - margin) / 200, and the
    draw is x_min + (x_max - x_min) * u.  (400, 300, 250) gives negative spans, which create does not refuse."""
    _, d = rp.make_params(rp.changed(default, width=w, height=h, tank_margin=m))
    x_min, y_min = (-(w / 2) + m) / 200, (-(h / 2) + m) / 200
    assert d["x_min"] == x_min and d["x_span"] == ((w / 2) - m) / 200 - x_min
    assert d["y_min"] == y_min and d["y_span"] == ((h / 2) - m) / 200 - y_min
    if m == 250.0:
        assert d["x_span"] < 0 and d["y_span"] < 0


def test_seed_base_count_and_pitch(default):
    _, d = rp.make_params(default, n_envs=64, seed=0x0123456789ABCDEF, base=77)
    assert (d["seed_lo"], d["seed_hi"], d["env_base"], d["n"]) == (0x89ABCDEF, 0x01234567, 77, 64)
    assert [rp.make_params(default, n_envs=n)[1]["pitch"] for n in (1, 64, 65)] == [64, 64, 128]
    assert [rp.make_params(default, n_envs=n)[1]["n"] for n in (1, 64, 65)] == [1, 64, 65]


def test_every_listed_field_reaches_its_member(default):
    values = {name: 1 + k / 16 for k, name in enumerate(ROBOT_PARAM_NAMES)}      # exact in binary, all different
    listed, d = rp.make_params(rp.changed(default, dt=0.0078125, max_cycles=321, nozzle_length3=9.0, **values))
    assert listed.tolist() == [values[name] for name in ROBOT_PARAM_NAMES]
    assert d["dt"] == 0.0078125 and d["max_cycles"] == 321


# ---- check_robot_create
def test_create_accepts_the_default_and_the_edges_it_always_accepted(default):
    assert rp.check_create(default) == (SALP_OK, "")
    assert rp.check_create(default, n_envs=1) == (SALP_OK, "")
    for fields in (dict(dt=TINY), dict(init_width=TINY), dict(nozzle_area=TINY), dict(density=-1000.0),
                   dict(max_contraction=default.init_length * 2), dict(dt=math.inf)):
        assert rp.check_create(rp.changed(default, **fields)) == (SALP_OK, ""), fields


def test_create_refusals(default):
    size = "salp_robot_config_t.struct_size mismatch"
    rng = "n_envs / env_index_base out of range"
    pos = "dt, init_width, nozzle_area must be positive"
    assert rp.check_create(None) == (SALP_ERR_INVALID, size)
    for off in (4, -4):
        assert rp.check_create(rp.changed(default, struct_size=default.struct_size + off)) == (SALP_ERR_INVALID, size)
    for n, base in ((0, 0), (-1, 0), (64, -1)):
        assert rp.check_create(default, n_envs=n, base=base) == (SALP_ERR_INVALID, rng), (n, base)
    for fields in (dict(dt=0.0), dict(dt=-0.01), dict(dt=math.nan), dict(init_width=0.0), dict(nozzle_area=0.0),
                   dict(init_width=math.nan), dict(nozzle_area=-TINY)):
        assert rp.check_create(rp.changed(default, **fields)) == (SALP_ERR_INVALID, pos), fields
    # the parent's order: the struct, then the counts, then the config's values
    assert rp.check_create(rp.changed(default, struct_size=0, dt=0.0), n_envs=0)[1] == size
    assert rp.check_create(rp.changed(default, dt=0.0), n_envs=0)[1] == rng


# ---- robot_max_steps, history_capacity
def _count(dt):
    """The cycle body's own loop for a cycle of the cut's length: fp64 accumulation of dt (oracle env_step)."""
    t, k = 0.0, 0
    while t < T_MAX:
        t += dt
        k += 1
    return k


@pytest.mark.parametrize("dt", [0.01, 0.005, 0.02, 0.003, 0.1, 1e-4, 14.6, 20.0, math.inf])
def test_max_steps_is_the_accumulated_count(dt):
    want = _count(dt)
    assert rp.max_steps(dt) == want
    if dt == 0.01:
        assert want == MAX_STEPS
    if dt >= T_MAX:
        assert want == 1


def test_max_steps_refuses_what_it_cannot_count():
    assert T_MAX / 8e-7 > 2 ** 24 > T_MAX / 9e-7
    for dt in (8e-7, 1e-9, TINY, math.nan, -0.01, -math.inf):
        assert rp.max_steps(dt) == -1, dt
    k = rp.max_steps(9e-7)      # 16.2 million steps: counted in C only
    assert T_MAX / 9e-7 <= k <= T_MAX / 9e-7 + 2


def test_history_capacity():
    """ceil(T / stride) + 1 samples: sample 0, one every `stride` steps, and the last step when T % stride != 0."""
    assert [rp.history_capacity(MAX_STEPS, s) for s in (1, 4, 10)] == [1462, 367, 148]
    for s in (1, 2, 3, 7, 1460):
        assert rp.history_capacity(MAX_STEPS, s) == len(set(range(0, MAX_STEPS, s)) | {MAX_STEPS})
    for s in (MAX_STEPS, MAX_STEPS + 1, 2 ** 31 - 1):
        assert rp.history_capacity(MAX_STEPS, s) == 2
    for s in (1, 4, 2 ** 31 - 1):
        assert rp.history_capacity(-1, s) == -1


# ---- check_history_args
N = 512
CAP = 1462
RANGE_MSG = "history env range [hist_begin, hist_begin + hist_count) is outside [0, n_envs)"


def _hist(begin=0, count=10, stride=1, capacity=CAP, steps=MAX_STEPS, **kw):
    return rp.check_history(N, steps, begin, count, stride, capacity, **kw)


def test_history_refusals_have_the_messages_of_the_abi():
    assert _hist(stride=0) == (SALP_ERR_INVALID, "history stride must be >= 1", False)
    assert _hist(stride=-3) == (SALP_ERR_INVALID, "history stride must be >= 1", False)
    for begin, count in ((-1, 10), (500, 13), (0, N + 1), (0, -1), (N + 1, 0), (2 ** 62, 2 ** 62)):
        assert _hist(begin, count) == (SALP_ERR_INVALID, RANGE_MSG, False), (begin, count)
    assert _hist(capacity=CAP - 1) == \
        (SALP_ERR_INVALID, "history capacity 1461 is below salp_robot_vec_history_capacity = 1462", False)
    assert _hist(stride=4, capacity=366) == \
        (SALP_ERR_INVALID, "history capacity 366 is below salp_robot_vec_history_capacity = 367", False)
    assert _hist(capacity=-5)[1] == "history capacity -5 is below salp_robot_vec_history_capacity = 1462"
    assert _hist(history=0) == (SALP_ERR_INVALID, "history is NULL while hist_count > 0", False)
    for addr in (0x1004, 0x1008, 0x100F):
        assert _hist(history=addr, flags=1) == (SALP_ERR_INVALID, "device history must be 16-byte aligned", False)
    assert _hist(steps=-1) == \
        (SALP_ERR_INVALID, "dt is too small to record a history (more than 2^24 Euler steps per cycle)", False)


def test_history_accepts_the_last_value_inside_each_range():
    ok = (SALP_OK, "", False)
    assert _hist() == ok and _hist(stride=2 ** 31 - 1, capacity=2) == ok
    for begin, count in ((0, N), (500, 12), (N - 1, 1), (0, 1)):
        assert _hist(begin, count) == ok, (begin, count)
    assert _hist(stride=4, capacity=367) == ok and _hist(capacity=2 ** 31 - 1) == ok
    assert _hist(history=0x1008, flags=0) == ok          # host pointers need no alignment
    assert _hist(history=0x1010, flags=1) == ok


def test_an_empty_history_range_is_the_plain_step():
    """hist_count == 0 is salp_robot_vec_step: nothing after the range is looked at, the stride and the range still are."""
    plain = (SALP_OK, "", True)
    assert _hist(0, 0, capacity=0, history=0) == plain and _hist(N, 0, capacity=0, history=0, steps=-1) == plain
    assert _hist(0, 0, stride=0)[1] == "history stride must be >= 1"
    assert _hist(N + 1, 0)[1] == RANGE_MSG


def test_history_refusals_come_in_the_order_of_the_abi():
    assert _hist(-1, 10, stride=0, steps=-1)[1] == "history stride must be >= 1"
    assert _hist(-1, 10, steps=-1, capacity=0, history=0)[1] == RANGE_MSG
    assert _hist(steps=-1, capacity=0, history=0)[1].startswith("dt is too small")
    assert _hist(capacity=0, history=0)[1].startswith("history capacity 0 ")
    assert _hist(history=0, flags=1)[1] == "history is NULL while hist_count > 0"


def test_a_short_message_buffer_truncates():
    rc, msg, _ = _hist(capacity=CAP - 1, msg_size=40)
    assert rc == SALP_ERR_INVALID and msg == "history capacity 1461 is below salp_robot_vec_history_capacity = 1462"[:39]
    assert rp.check_trajectory(MAX_STEPS, 0, msg_size=12) == (SALP_ERR_INVALID, "cycles must")


# ---- check_trajectory_args
def test_trajectory_refusals_have_the_messages_of_the_abi():
    top = rp.max_trajectory_cycles()
    assert top == 1024
    for cycles in (0, -2, top + 1, -2 ** 31):
        assert rp.check_trajectory(MAX_STEPS, cycles) == (SALP_ERR_INVALID, "cycles must be in [1, 1024]"), cycles
    for flags in (1 | 4, 4, 1 << 31, 0xFFFFFFFC):
        assert rp.check_trajectory(MAX_STEPS, 8, flags) == (SALP_ERR_INVALID, "unknown flag bits"), flags
    assert rp.check_trajectory(MAX_STEPS, 8, metrics=True) == (SALP_ERR_INVALID, "metrics need expected states")
    assert rp.check_trajectory(-1, 8) == (SALP_ERR_INVALID, "dt is too small (more than 2^24 Euler steps per cycle)")
    # the parent's order
    assert rp.check_trajectory(-1, 0, 4, metrics=True)[1] == "cycles must be in [1, 1024]"
    assert rp.check_trajectory(-1, 8, 4, metrics=True)[1] == "unknown flag bits"
    assert rp.check_trajectory(-1, 8, 0, metrics=True)[1] == "metrics need expected states"


def test_trajectory_accepts_the_last_value_inside_each_range():
    for cycles in (1, 1024):
        for flags in (0, 1, 2, 3):
            assert rp.check_trajectory(MAX_STEPS, cycles, flags) == (SALP_OK, ""), (cycles, flags)
    assert rp.check_trajectory(0, 8, expected=True, metrics=True) == (SALP_OK, "")
    assert rp.check_trajectory(MAX_STEPS, 8, expected=True) == (SALP_OK, "")


# ---- schedule_bin
def _bins_by_formula(act):
    """schedule_bin's own formula in numpy fp64 (no contraction): truncation of b, 0 for b <= 0 or NaN, 255 from 255 up."""
    a0, a1 = act[:, 0].astype(np.float64), act[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        total = (a0 * 0.06) * (3.0 / 0.06 + 1.5 / 0.06) + a1 * 10.0
        b = total * (255 / 14.6)
        inside = (b > 0.0) & (b < 255.0)
        return np.where(inside, np.trunc(np.where(inside, b, 0.0)), np.where(b >= 255.0, 255.0, 0.0)).astype(np.int32), total


@pytest.fixture(scope="module")
def box_actions():
    rng = np.random.default_rng(2026)
    act = rng.uniform([0.0, 0.0, -1.0], [1.0, 1.0, 1.0], (100_000, 3)).astype(np.float32)
    act[:8, :2] = [(0, 0), (1, 1), (1, 0), (0, 1), (0.5, 0.5), (1e-30, 0), (0, 1e-30), (1, 0.999)]
    return act


def test_schedule_bin_is_its_formula_bit_for_bit(box_actions):
    got = rp.schedule_bins(box_actions)
    want, _ = _bins_by_formula(box_actions)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() <= 255 and len(np.unique(got)) > 250     # the Box fills the bins up to 14.5 s


def test_schedule_bin_follows_the_cycle_length_the_kernel_computes(box_actions):
    """set_control (oracle env_step): T = c / (0.06 / 3) + c / (0.06 / 1.5) + coast with c = a0 * 0.06, coast = a1 * 10.
    The schedule computes the same length with one product instead of two quotients, so a value next to a bin edge may
    land in the neighbouring bin — never further."""
    c = box_actions[:, 0].astype(np.float64) * 0.06
    T = c / (0.06 / 3) + c / (0.06 / 1.5) + box_actions[:, 1].astype(np.float64) * 10.0
    want = np.clip(np.floor(T * 255 / 14.6), 0, 255).astype(np.int32)
    got = rp.schedule_bins(box_actions)
    assert np.abs(got - want).max() <= 1
    assert np.mean(got == want) > 0.999


def test_schedule_bin_edges():
    inf, nan = np.inf, np.nan
    zero = [(nan, 0.5), (0.5, nan), (nan, nan), (inf, -inf), (-inf, inf), (0.0, 0.0), (-0.0, 0.0), (-1.0, 0.0), (0.0, -1.0),
            (0.5, -0.25), (-inf, 0.0), (1.0, -1.0)]
    top = [(1.0, 1.0101),(1.0, 1.5), (0.0, 1.46), (4.0, 0.0), (inf, 0.0), (0.0, inf), (inf, inf), (3e38, 3e38), (1e9, 0.0)]
    for pairs, want in ((zero, 0), (top, 255)):
        act = np.array([(a, b, 0.0) for a, b in pairs], np.float32)
        got = rp.schedule_bins(act)
        _, total = _bins_by_formula(act)
        assert np.all((total >= T_MAX) if want else ~(total > 0.0)), total       # the cases are what their group says
        assert np.array_equal(got, np.full(len(pairs), want, np.int32)), (got, pairs)
    # out of the Box on both sides: still its formula, always a valid bin
    rng = np.random.default_rng(7)
    act = rng.uniform(-2.0, 3.0, (20_000, 3)).astype(np.float32)
    got = rp.schedule_bins(act)
    assert np.array_equal(got, _bins_by_formula(act)[0]) and got.min() == 0 and got.max() == 255
