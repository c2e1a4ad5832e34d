"""The literal-constant kernels are chosen by is_std(DevParams), and a configuration they are chosen for must derive every
literal exactly: a constant that differs in the last bit simulates another tank with no error.  csrc/salp_params.h writes
the constants once (SALP_STD_CONSTS) and generates StdConsts and is_std() from that list; its host functions compile as
plain C++ (tests/params_host.cpp), so what salp_vec_create runs before it touches a GPU is checked here without one."""
import ctypes
import glob
import math
import os
import re

import numpy as np
import pytest

import params_host_lib as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SALP_OK, SALP_ERR_INVALID = 0, -1

# config fields that feed a listed constant, with the constants each one reaches (make_params)
INT_FIELDS = {"width": ("W", "half_W", "wall_hi_x", "food_xspan", "inv_W", "inv_diag", "tie_c0"),
              "height": ("H", "half_H", "wall_hi_y", "food_yspan", "inv_H", "inv_diag"),
              "inhale_duration": ("inhale_dur", "cycle_len"), "exhale_duration": ("exhale_dur", "exhale_dur_d", "cycle_len"),
              "rest_duration": ("cycle_len",)}
DOUBLE_FIELDS = {"tank_margin": ("margin", "wall_hi_x", "wall_hi_y", "food_xlo", "food_ylo", "food_xspan", "food_yspan"),
                 "base_radius": ("R", "a_rest", "b_rest", "ab_full", "da_inh", "db_inh", "da_exh", "db_exh", "inv_R"),
                 "max_thrust_force": ("thrust_force",), "drag_coefficient": ("drag",), "angular_drag": ("ang_drag",),
                 "max_nozzle_angle": ("max_nozzle", "inv_max_nozzle"), "nozzle_response_rate": ("nozzle_rate",),
                 "food_radius": ("food_radius", "food_xlo", "food_ylo", "food_xspan", "food_yspan"),
                 "min_food_distance": ("min_food_dist2",)}
# fields that no listed constant depends on: kernels read them from the launch parameters in every instantiation
UNLISTED = {"food_reward": 11.0, "collision_penalty": -7.0, "time_penalty": -0.3, "efficiency_bonus": 0.0,
            "proximity_reward_weight": 5.0, "num_food_items": 12, "max_observed_food": 5, "max_steps_without_food": 900,
            "forced_breathing": 0, "random_food_count": 1, "respawn_food": 0, "no_autoreset": 1}


@pytest.fixture(scope="module")
def default():
    return ph.default_config()


@pytest.fixture(scope="module")
def rows():
    return ph.std_consts()


def test_default_config_is_the_documented_one(default):
    from underwater_swimmer_rl_amd.config import CConfig, SalpSnakeConfig
    want = SalpSnakeConfig().to_c()
    assert default.struct_size == ctypes.sizeof(CConfig)
    assert bytes(default) == bytes(want)


def test_defaults_derive_the_literals(default, rows):
    P = ph.Params(default)
    assert P.is_std()
    for i, (typ, name, text, literal) in enumerate(rows):
        # the exported value is the literal as written (a number or a quotient of two), in the row's own precision
        if typ == "float":
            written = float(np.float32(text.rstrip("f")))
        else:
            num, *den = [float(t) for t in text.split("/")]
            written = num / den[0] if den else num
        assert literal == written, (name, text, literal)
        assert P.value(i) == literal, (name, text, P.value(i), literal)   # exact: fp64, fp32 and int as stored


def _perturbed(default, field, value):
    c = ph.changed(default, **{field: value})
    assert ph.validate(c)[0] == SALP_OK, (field, value)
    return ph.Params(c)


def _constants_moved(P, rows):
    return {name for i, (_, name, _, literal) in enumerate(rows) if P.value(i) != literal}


@pytest.mark.parametrize("field", sorted(INT_FIELDS))
def test_an_integer_field_one_step_off_leaves_the_standard_class(default, rows, field):
    P = _perturbed(default, field, getattr(default, field) + 1)
    assert not P.is_std()
    moved = _constants_moved(P, rows)
    assert moved and moved <= set(INT_FIELDS[field]), moved


@pytest.mark.parametrize("toward", [-math.inf, math.inf])
@pytest.mark.parametrize("field", sorted(DOUBLE_FIELDS))
def test_a_double_field_one_ulp_off_leaves_the_standard_class(default, rows, field, toward):
    """No exception is needed: every one of these fields reaches at least one constant that does not round back to its
    literal after a change of one ulp in either direction (most are copied; min_food_distance is squared: one ulp of 80,
    1.4e-14, moves the square by 2.3e-12, 2.5 ulp of 6400)."""
    v = math.nextafter(getattr(default, field), toward)
    assert v != getattr(default, field)
    P = _perturbed(default, field, v)
    assert not P.is_std()
    moved = _constants_moved(P, rows)
    assert moved and moved <= set(DOUBLE_FIELDS[field]), moved


@pytest.mark.parametrize("field", sorted(UNLISTED))
def test_an_unlisted_field_stays_in_the_standard_class(default, rows, field):
    assert getattr(default, field) != UNLISTED[field]
    P = _perturbed(default, field, UNLISTED[field])
    assert P.is_std() and not _constants_moved(P, rows)


def test_every_field_of_the_config_is_in_one_of_the_three_groups():
    from underwater_swimmer_rl_amd.config import CConfig
    assert {n for n, _ in CConfig._fields_} - {"struct_size"} == set(INT_FIELDS) | set(DOUBLE_FIELDS) | set(UNLISTED)


def test_the_list_is_complete(rows):
    """What the hand-written is_std() never had: StdConsts as the compiler sees it holds exactly the names of the list that
    is_std() is generated from, and every constant a kernel reads through CV() is one of them."""
    names = [name for _, name, _, _ in rows]
    assert len(set(names)) == len(names)
    assert ph.std_members_after_preprocessing() == names
    used = set()
    csrc = os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")):
        with open(path) as f:
            used |= set(re.findall(r"\bCV\((\w+)\)", f.read()))
    used.discard("name")                       # the macro's own definition and its comment
    assert len(used) > 20 and used <= set(names), sorted(used - set(names))
    with open(os.path.join(csrc, "salp_params.h")) as f:
        src = f.read()
    assert "struct StdConsts {\n#define SALP_STD_MEMBER" in src and "return true SALP_STD_CONSTS(SALP_STD_EQUAL);" in src


def test_validate_accepts_the_default_and_refuses_null_and_a_foreign_struct(default):
    assert ph.validate(default) == (SALP_OK, "")
    assert ph.validate(None) == (SALP_ERR_INVALID, "config is NULL")
    assert ph.validate(ph.changed(default, struct_size=default.struct_size + 4)) == \
        (SALP_ERR_INVALID, "salp_config_t.struct_size mismatch (ABI version skew)")


TINY = 5e-324      # the smallest positive double
RANGES = [   # field, first values outside, last values inside, message
    ("width", [0, -1], [1], "width/height must be positive"),
    ("height", [0, -1], [1], "width/height must be positive"),
    ("num_food_items", [-1, 17], [0, 16], "num_food_items must be in [0, SALP_MAX_FOOD]"),
    ("max_observed_food", [-1, 9], [0, 8], "max_observed_food must be in [0, SALP_MAX_OBSERVED_FOOD]"),
    ("inhale_duration", [0, 256], [1, 255], "inhale_duration in [1,255], exhale_duration in [4,254] required"),
    ("exhale_duration", [3, 255], [4, 254], "inhale_duration in [1,255], exhale_duration in [4,254] required"),
    ("rest_duration", [-1], [0], "rest_duration must be >= 0"),
    ("base_radius", [0.0, -TINY, math.nan], [TINY], "base_radius and max_nozzle_angle must be positive"),
    ("max_nozzle_angle", [0.0, -TINY, math.nan], [TINY], "base_radius and max_nozzle_angle must be positive"),
]


@pytest.mark.parametrize("field,outside,inside,message", RANGES, ids=[r[0] for r in RANGES])
def test_validate_refuses_each_range_at_its_first_value_outside(default, field, outside, inside, message):
    for v in outside:
        assert ph.validate(ph.changed(default, **{field: v})) == (SALP_ERR_INVALID, message), (field, v)
    for v in inside:
        assert ph.validate(ph.changed(default, **{field: v})) == (SALP_OK, ""), (field, v)
