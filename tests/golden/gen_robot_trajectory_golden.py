#!/usr/bin/env python3
"""Golden trajectory comparisons for the HEAD simulator (salp_robot_vec_trajectory, include/salp_robot.h), generated
by running the REFERENCE's own robot.py + compare_trajectories.py (compare_actions_with_states) in the build container
(tests/golden/robot_harness.py).
    python tests/golden/gen_robot_trajectory_golden.py
Writes trajectory_robot_params.npz (the name keeps it out of the robot_*.npz step vectors).  Every action is
float64(float32 a) * (0.06, 10, pi/2), with `a` stored too, so that the C oracle can replay it as env actions.
  param_names [12]                              SALP_RP_* order
  shared part: K candidate robots, one shared action sequence of T cycles
    params f64 [12, K]                          candidate k's parameters (column 0 is the default robot)
    a_shared f32 [T, 3], actions_shared f64 [T, 3]
    true_candidate i64, expected_shared f64 [T, 6]   that candidate's reference trajectory plus seeded noise
    shared_<key>                                compare_actions_with_states(actions_shared, expected_shared, robot_k)
                                                per candidate along axis 0 (actual_states, errors, position_errors,
                                                velocity_errors, angle_errors [K, T, ...]; position_error,
                                                velocity_error, angle_error, max_position_error [K])
    shared_angular_velocity_error f64 [K]       mean |d yaw rate|
    shared_inner_steps i32 [K, T]               Euler steps of each cycle (len(position_history) - 1)
  per-robot part: M action sequences on the default robot
    a_per f32 [M, T2, 3], actions_per f64 [M, T2, 3], expected_per f64 [T2, 6], per_<key> as above over M"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import robot_harness as rb  # noqa: E402

PARAM_NAMES = ("dry_mass", "init_length", "init_width", "max_contraction", "density", "drag_coefficient_min",
               "drag_coefficient_max", "nozzle_length1", "nozzle_length2", "nozzle_area", "nozzle_mass", "nozzle_gamma")
DEFAULT = dict(dry_mass=1.0, init_length=0.3, init_width=0.15, max_contraction=0.06, density=1000.0,
               drag_coefficient_min=0.4, drag_coefficient_max=1.0, nozzle_length1=0.05, nozzle_length2=0.05,
               nozzle_area=0.00016, nozzle_mass=1.0, nozzle_gamma=np.pi / 4)
SCALE = np.array([0.06, 10.0, np.pi / 2])
KEYS = ("actual_states", "errors", "position_errors", "velocity_errors", "angle_errors", "position_error",
        "velocity_error", "angle_error", "max_position_error")


def load_compare():
    robot_mod, _, _ = rb.load()      # puts the reference's environments directory on sys.path (robot.py)
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("compare_trajectories_ref", os.path.join(rb.ENV_DIR, "compare_trajectories.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return robot_mod, mod


def make_robot(robot_mod, p):
    """Robot(...) / Nozzle(...) / set_environment / _drag_coefficents of the candidate, as a user of the reference
    builds it (compare_trajectories.py:40-45)."""
    nozzle = robot_mod.Nozzle(length1=p["nozzle_length1"], length2=p["nozzle_length2"], length3=0.05,
                              area=p["nozzle_area"], mass=p["nozzle_mass"])
    nozzle.gamma = p["nozzle_gamma"]
    robot = robot_mod.Robot(dry_mass=p["dry_mass"], init_length=p["init_length"], init_width=p["init_width"],
                            max_contraction=p["max_contraction"], nozzle=nozzle)
    robot.set_environment(density=p["density"])
    robot._drag_coefficents = [p["drag_coefficient_min"], p["drag_coefficient_max"]]
    robot.nozzle.set_angles(angle1=0.0, angle2=0.0)
    return robot


class _CountingRobot:
    """Records len(position_history) - 1 after every step_through_cycle of the wrapped robot."""

    def __init__(self, robot):
        self.__dict__["_r"], self.__dict__["steps"] = robot, []

    def step_through_cycle(self):
        self._r.step_through_cycle()
        self.steps.append(len(self._r.position_history) - 1)

    def __getattr__(self, name):
        return getattr(self._r, name)

    def __setattr__(self, name, value):
        setattr(self._r, name, value)


def run(cmp_mod, robot, actions, expected):
    r = _CountingRobot(robot)
    out = cmp_mod.compare_actions_with_states(actions, expected, robot=r, verbose=False)
    out["angular_velocity_error"] = float(np.mean(np.abs(out["errors"][:, 5])))
    out["inner_steps"] = np.array(r.steps, np.int32)
    return out


def stack(outs, prefix):
    d = {f"{prefix}_{k}": np.array([o[k] for o in outs], np.float64) for k in KEYS + ("angular_velocity_error",)}
    d[f"{prefix}_inner_steps"] = np.stack([o["inner_steps"] for o in outs]).astype(np.int32)
    return d


def main():
    robot_mod, cmp_mod = load_compare()
    # candidates: together they move every row away from its default; 0 is the default robot
    changes = [{},
               dict(dry_mass=1.3, density=1025.0),
               dict(init_length=0.33, init_width=0.14, max_contraction=0.05),
               dict(drag_coefficient_min=0.3, drag_coefficient_max=1.2),
               dict(nozzle_length1=0.06, nozzle_length2=0.04, nozzle_area=0.0002),
               dict(nozzle_mass=0.8, nozzle_gamma=np.pi / 5),
               dict(dry_mass=0.9, init_width=0.16, drag_coefficient_max=0.9, nozzle_area=0.00013),
               dict(init_length=0.28, max_contraction=0.07, density=990.0, nozzle_mass=1.2, nozzle_gamma=0.9,
                    drag_coefficient_min=0.45)]
    cands = [dict(DEFAULT, **c) for c in changes]
    params = np.array([[c[k] for c in cands] for k in PARAM_NAMES], np.float64)
    assert all((params[j] != params[j, 0]).any() for j in range(len(PARAM_NAMES)))

    # shared actions: contraction 0, the Box maximum, coast 0 and several seconds, yaw +-pi/2
    a = np.array([[0.8, 0.05, 0.0], [1.0, 0.0, 1.0], [0.0, 0.1, 0.3], [1.0, 1.0, -1.0], [0.5, 0.0, -1.0],
                  [0.0, 0.0, 0.5], [0.7, 0.4, 0.25], [1.0, 0.02, 1.0], [0.3, 0.3, -0.6], [0.9, 0.0, 0.0],
                  [0.6, 0.05, -0.2], [1.0, 0.15, 0.7], [0.2, 0.6, 1.0], [1.0, 0.0, -0.4], [0.45, 0.1, 0.9],
                  [0.75, 0.25, -1.0]], np.float32)
    acts = a.astype(np.float64) * SCALE
    true_k = 6
    truth = run(cmp_mod, make_robot(robot_mod, cands[true_k]), acts, np.zeros((len(a), 6)))["actual_states"]
    rng = np.random.default_rng(2024)
    expected = truth + rng.normal(0.0, 1.0, truth.shape) * np.array([0.01, 0.01, 0.005, 0.005, 0.02, 0.01])
    outs = [run(cmp_mod, make_robot(robot_mod, c), acts, expected) for c in cands]

    # per-robot actions on the default robot, in the style of compare_action_combinations (:287-321)
    T2 = 8
    combos = [(1.0, 0.1, 0.0), (0.5, 0.1, 0.0), (1.0, 0.05, 0.0), (1.0, 0.1, 1.0 / 3), (1.0, 0.1, -1.0 / 3)]
    a_per = np.stack([np.tile(np.array(c, np.float32), (T2, 1)) for c in combos] +
                     [np.stack([rng.uniform(0, 1, T2), rng.uniform(0, 0.3, T2), rng.uniform(-1, 1, T2)], 1).astype(np.float32)])
    acts_per = a_per.astype(np.float64) * SCALE
    ref0 = run(cmp_mod, make_robot(robot_mod, DEFAULT), acts_per[3], np.zeros((T2, 6)))["actual_states"]
    expected_per = ref0 + rng.normal(0.0, 1.0, ref0.shape) * 0.01
    outs_per = [run(cmp_mod, make_robot(robot_mod, DEFAULT), acts_per[m], expected_per) for m in range(len(a_per))]

    out = dict(param_names=np.array(PARAM_NAMES), params=params, a_shared=a, actions_shared=acts,
               true_candidate=np.int64(true_k), expected_shared=expected, a_per=a_per, actions_per=acts_per,
               expected_per=expected_per)
    out.update(stack(outs, "shared"))
    out.update(stack(outs_per, "per"))
    path = os.path.join(HERE, "trajectory_robot_params.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cands)} candidates x {len(a)} cycles, {len(a_per)} sequences x {T2} cycles, "
          f"{int(out['shared_inner_steps'].sum() + out['per_inner_steps'].sum())} Euler steps, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if not rb.available():
        raise SystemExit("reference not found: run in the build container")
    main()
