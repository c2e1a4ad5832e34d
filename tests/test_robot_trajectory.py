"""Trajectory comparison of the HEAD simulator (salp_robot_vec_trajectory, include/salp_robot.h) — the parts that need
no GPU: the C ABI is declared and exported, the parameter and metric enums match the Python names, the parameter
helpers, and the reference's own comparisons (tests/golden/trajectory_robot_params.npz,
gen_robot_trajectory_golden.py) are consistent with themselves and with the C oracle run with each candidate's config.
The GPU side is tests/test_gpu_robot_trajectory.py."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import robot_oracle_lib as rol
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.robot_compare import (MAX_TRAJECTORY_CYCLES, METRIC_NAMES, PER_ROBOT_ACTIONS,
                                                     ROBOT_PARAM_NAMES, params_from_robot, robot_params)
from underwater_swimmer_rl_amd.robot_env import ROBOT_EXPORTS, CRobotConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "trajectory_robot_params.npz")
NAME = "salp_robot_vec_trajectory"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "salp_robot.h")).read(), flags=re.S)


def _enum(prefix, count):
    body = re.search(r"enum\s*\{([^}]*" + prefix + count + r"[^}]*)\}", _header()).group(1)
    return {k: int(v) for k, v in re.findall(prefix + r"([A-Z_0-9]+)\s*=\s*(\d+)", body)}


def test_trajectory_abi_is_declared_and_exported():
    src = _header()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert NAME in ROBOT_EXPORTS
    assert hasattr(_capi.load_library(), NAME)
    assert _enum("SALP_ROBOT_", "PER_ROBOT_ACTIONS") == {"PER_ROBOT_ACTIONS": PER_ROBOT_ACTIONS}
    assert _enum("SALP_ROBOT_", "MAX_TRAJECTORY_CYCLES") == {"MAX_TRAJECTORY_CYCLES": MAX_TRAJECTORY_CYCLES}


def test_parameter_and_metric_enums_match_python():
    rp = _enum("SALP_RP_", "COUNT")
    assert rp.pop("COUNT") == len(ROBOT_PARAM_NAMES) == 12
    assert [k.lower() for k, _ in sorted(rp.items(), key=lambda kv: kv[1])] == list(ROBOT_PARAM_NAMES)
    assert sorted(rp.values()) == list(range(12))
    rm = _enum("SALP_RM_", "COUNT")
    assert rm.pop("COUNT") == len(METRIC_NAMES) == 5
    assert [k.lower() for k, _ in sorted(rm.items(), key=lambda kv: kv[1])] == list(METRIC_NAMES)
    fields = {f for f, _ in CRobotConfig._fields_}
    assert set(ROBOT_PARAM_NAMES) <= fields and "nozzle_length3" not in ROBOT_PARAM_NAMES


def test_robot_params_defaults_overrides_and_errors():
    L = _capi.load_library()
    cfg = CRobotConfig()
    L.salp_robot_config_default.argtypes = [ctypes.POINTER(CRobotConfig)]
    assert L.salp_robot_config_default(ctypes.byref(cfg)) == 0
    t = robot_params(5, "cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (12, 5)
    for j, name in enumerate(ROBOT_PARAM_NAMES):
        assert torch.all(t[j] == getattr(cfg, name)), name
    t = robot_params(4, "cpu", dry_mass=[1.0, 2.0, 3.0, 4.0], nozzle_area=2e-4, density=np.float64(990.0))
    assert t[0].tolist() == [1.0, 2.0, 3.0, 4.0] and torch.all(t[9] == 2e-4) and torch.all(t[4] == 990.0)
    assert torch.all(t[1] == cfg.init_length)
    with pytest.raises(TypeError):
        robot_params(4, "cpu", nozzle_length3=0.1)
    with pytest.raises(TypeError):
        robot_params(4, "cpu", drymass=1.0)
    with pytest.raises(ValueError):
        robot_params(4, "cpu", dry_mass=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        robot_params(4, "cpu", dry_mass=np.ones((4, 1)))
    with pytest.raises(ValueError):
        robot_params(0, "cpu")


def test_params_from_robot_reads_a_reference_robot():
    nozzle = SimpleNamespace(length1=0.06, length2=0.04, length3=0.01, area=2e-4, mass=0.8, gamma=0.7)
    robot = SimpleNamespace(dry_mass=1.3, init_length=0.31, init_width=0.14, max_contraction=0.05, density=1025,
                            _drag_coefficents=[0.35, 1.1], nozzle=nozzle, dt=0.01)
    p = params_from_robot(robot)
    assert p == dict(dry_mass=1.3, init_length=0.31, init_width=0.14, max_contraction=0.05, density=1025.0,
                     drag_coefficient_min=0.35, drag_coefficient_max=1.1, nozzle_length1=0.06, nozzle_length2=0.04,
                     nozzle_area=2e-4, nozzle_mass=0.8, nozzle_gamma=0.7)
    t = robot_params(3, "cpu", **p)
    assert t[:, 2].tolist() == [p[k] for k in ROBOT_PARAM_NAMES]


def _parts(z):
    yield "shared", z["actions_shared"], z["expected_shared"]
    yield "per", z["actions_per"], z["expected_per"]


def test_fixture_is_self_consistent():
    """The package's error and metric formulas (the torch code of compare_actions_with_states and the kernel's metric
    definitions) applied to the fixture's actual / expected states reproduce the reference's stored values."""
    z = np.load(GOLD, allow_pickle=False)
    assert list(z["param_names"]) == list(ROBOT_PARAM_NAMES)
    P = z["params"]
    assert P.shape == (12, 8) and all((P[j] != P[j, 0]).any() for j in range(12))
    assert np.array_equal(P[:, 0], robot_params(1, "cpu").numpy()[:, 0])
    scale = np.array([0.06, 10.0, np.pi / 2])
    assert np.array_equal(z["actions_shared"], z["a_shared"].astype(np.float64) * scale)
    assert np.array_equal(z["actions_per"], z["a_per"].astype(np.float64) * scale)
    a = z["a_shared"]
    assert (a[:, 0] == 0).any() and (a[:, :2] == 1).all(axis=1).any() and (a[:, 1] == 0).any() and (a[:, 1] >= 0.3).any()
    assert (a[:, 2] == 1).any() and (a[:, 2] == -1).any()
    assert z["shared_inner_steps"].max() == 1451 and (z["shared_inner_steps"] == 0).any()
    for part, acts, expected in _parts(z):
        actual = torch.as_tensor(z[f"{part}_actual_states"])
        x = torch.as_tensor(expected)
        err = actual - x
        assert torch.equal(err, torch.as_tensor(z[f"{part}_errors"]))
        for key, got in (("position_errors", torch.linalg.vector_norm(err[..., 0:2], dim=-1)),
                         ("velocity_errors", torch.linalg.vector_norm(err[..., 2:4], dim=-1)),
                         ("angle_errors", err[..., 4].abs())):
            np.testing.assert_allclose(got.numpy(), z[f"{part}_{key}"], rtol=1e-14, atol=0)
        pe = z[f"{part}_position_errors"]
        # the kernel's metric definitions: fp64 sums in cycle order / T, max
        for key, per in (("position_error", pe), ("velocity_error", z[f"{part}_velocity_errors"]),
                         ("angle_error", z[f"{part}_angle_errors"]), ("angular_velocity_error", np.abs(z[f"{part}_errors"][..., 5]))):
            s = np.zeros(per.shape[0])
            for t in range(per.shape[1]):
                s = s + per[:, t]
            np.testing.assert_allclose(s / per.shape[1], z[f"{part}_{key}"], rtol=1e-13, atol=0)
        assert np.array_equal(pe.max(axis=1), z[f"{part}_max_position_error"])
        assert z[f"{part}_inner_steps"].dtype == np.int32 and z[f"{part}_inner_steps"].shape == actual.shape[:2]
    k = int(z["true_candidate"])
    assert np.argmin(z["shared_position_error"]) == k


def _oracle_cfg(col):
    c = rol.default_robot_config()
    for j, name in enumerate(ROBOT_PARAM_NAMES):
        setattr(c, name, float(col[j]))
    return c


def test_fixture_matches_the_oracle_per_candidate():
    """Each reference trajectory equals the C oracle's, created with that candidate's config and stepping the stored
    float32 actions as env actions, up to the robot's first env termination (target reached or lost, max_cycles)."""
    z = np.load(GOLD, allow_pickle=False)
    runs = [(z["params"][:, k], z["a_shared"], z["shared_actual_states"][k], z["shared_inner_steps"][k])
            for k in range(z["params"].shape[1])]
    runs += [(z["params"][:, 0], z["a_per"][m], z["per_actual_states"][m], z["per_inner_steps"][m])
             for m in range(z["a_per"].shape[0])]
    checked = 0
    for col, a, ref, steps in runs:
        orc = rol.RobotOracleVec(1, seed=3, cfg=_oracle_cfg(col))
        orc.reset(np.zeros(1, np.uint8))
        for t in range(len(a)):
            out = orc.step(a[t][None])
            assert out["inner_steps"][0] == steps[t], t
            if out["terminated"][0] or out["truncated"][0]:
                break
            s = orc.get_state()[:, 0]
            got = np.array([s[rol.R_POS], s[rol.R_POS + 1], s[rol.R_VEL], s[rol.R_VEL + 1], s[rol.R_EULER + 2], s[rol.R_OMEGA + 2]])
            assert np.max(np.abs(got - ref[t]) / np.maximum(1.0, np.abs(ref[t]))) <= 1e-6, (t, got, ref[t])
            checked += 1
        orc.close()
    assert checked >= 100
