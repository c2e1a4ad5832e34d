"""Trajectory comparison on the GPU (salp_robot_trajectory_kernel through salp_robot_vec_trajectory and
robot_compare.compare_actions_with_states): against the reference's own comparisons, robots of different candidates in
one wavefront, random parameter sets against the C oracle, the same physics as the env step, the default-parameter
path, independence from the env state, metrics, argument checks and hipGraph capture."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

import robot_oracle_lib as rol
from robot_math_cases import random_robot_params
from underwater_swimmer_rl_amd.robot_compare import ROBOT_PARAM_NAMES, compare_actions_with_states, robot_params
from underwater_swimmer_rl_amd.robot_env import R_EULER, R_OMEGA, R_POS, R_VEL, SalpRobotVectorEnv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_robot_params.npz")
SCALE = np.array([0.06, 10.0, np.pi / 2])
KEYS = ("position_error", "velocity_error", "angle_error", "max_position_error", "angular_velocity_error")
SENTINEL = -12345.0


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _ptr(x):
    if x is None:
        return None
    return ctypes.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else ctypes.c_void_p(x.ctypes.data)


def _raw(env, params, actions, cycles, expected, states, metrics, inner, flags, stream=None):
    return env.L.salp_robot_vec_trajectory(env._h, _ptr(params), _ptr(actions), int(cycles), _ptr(expected), _ptr(states),
                                           _ptr(metrics), _ptr(inner), flags, stream)


def _run_host(n, params, actions, T, expected, per_robot=False):
    """Host pointers (numpy), the staged path."""
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=1, output="numpy")
    st = np.full((T, n, 6), SENTINEL)
    met = np.full((n, 5), SENTINEL) if expected is not None else None
    inner = np.full((T, n), -7, np.int32)
    rc = _raw(env, None if params is None else np.ascontiguousarray(params, np.float64), np.ascontiguousarray(actions, np.float64),
              T, None if expected is None else np.ascontiguousarray(expected), st, met, inner, 2 if per_robot else 0)
    assert rc == 0, env.L.salp_robot_last_error()
    env.close()
    return dict(states=st, metrics=met, inner=inner)


def _scaled(a):
    return a.astype(np.float64) * SCALE


def test_reference_parity_host_and_device_pointers():
    z = np.load(GOLD, allow_pickle=False)
    for part, params, acts, expected in (("shared", z["params"], z["actions_shared"], z["expected_shared"]),
                                         ("per", None, z["actions_per"], z["expected_per"])):
        per_robot = acts.ndim == 3
        n = acts.shape[0] if per_robot else params.shape[1]
        T = acts.shape[1] if per_robot else acts.shape[0]
        out = compare_actions_with_states(acts, expected, params)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert got["actual_states"].shape == (n, T, 6)
        assert _rel(got["actual_states"], z[f"{part}_actual_states"]) <= 1e-6, part
        assert np.array_equal(got["inner_steps"], z[f"{part}_inner_steps"]), part
        for k in ("errors", "position_errors", "velocity_errors", "angle_errors") + KEYS:
            assert _rel(got[k], z[f"{part}_{k}"]) <= 1e-6, (part, k)
        host = _run_host(n, params, np.transpose(acts, (1, 0, 2)) if per_robot else acts, T, expected, per_robot)
        assert np.array_equal(host["states"], np.transpose(got["actual_states"], (1, 0, 2)))
        assert np.array_equal(host["inner"], got["inner_steps"].T)
        assert np.array_equal(host["metrics"], np.stack([got[k] for k in KEYS], axis=1))


def test_mixed_wavefronts_match_their_candidate():
    z = np.load(GOLD, allow_pickle=False)
    K = z["params"].shape[1]
    n = 4096
    idx = np.arange(n) % K
    out = compare_actions_with_states(z["actions_shared"], z["expected_shared"], z["params"][:, idx])
    st = out["actual_states"].cpu().numpy()
    met = np.stack([out[k].cpu().numpy() for k in KEYS], axis=1)
    inner = out["inner_steps"].cpu().numpy()
    for k in range(K):
        rows = idx == k
        assert np.all(st[rows] == st[k]) and np.all(met[rows] == met[k]) and np.all(inner[rows] == inner[k]), k
        assert _rel(st[k], z["shared_actual_states"][k]) <= 1e-6, k
        assert _rel(met[k], np.array([z[f"shared_{m}"][k] for m in KEYS])) <= 1e-6, k


def _oracle_states(col, a):
    c = rol.default_robot_config()
    for j, name in enumerate(ROBOT_PARAM_NAMES):
        setattr(c, name, float(col[j]))
    orc = rol.RobotOracleVec(1, seed=5, cfg=c)
    orc.reset(np.zeros(1, np.uint8))
    rows, steps = [], []
    for t in range(len(a)):
        out = orc.step(a[t][None])
        steps.append(int(out["inner_steps"][0]))
        if out["terminated"][0] or out["truncated"][0]:
            break
        s = orc.get_state()[:, 0]
        rows.append([s[R_POS], s[R_POS + 1], s[R_VEL], s[R_VEL + 1], s[R_EULER + 2], s[R_OMEGA + 2]])
    orc.close()
    return np.array(rows), steps


def test_random_parameters_at_scale_against_the_oracle():
    """65536 robots with random parameters; 160 sampled ones against (a) a device env created with that robot's config
    (the same physics with the parameters as kernel constants), to 1e-6 over all six cycles, and (b) the C oracle, to
    1e-6 on the first cycle.  Later cycles are not held to the oracle: in this box some robots spin at several rad/s
    and their roll / pitch grow from the last-bit difference of host and device libm in the nozzle IK (DESIGN.md 8f-4,
    long-run agreement) until the trajectories part; the device env of the same config parts from the oracle the same
    way.  Against the one-robot env the seed is the wave-uniform exact sin / cos fallback (< 1e-12 per cycle; one
    spinning robot takes it for its whole wavefront).  The worst differences are printed."""
    rng = np.random.default_rng(11)
    n, T = 65536, 6
    P = random_robot_params(rng, n)
    a = np.stack([rng.uniform(0, 1, T), rng.uniform(0, 0.2, T), rng.uniform(-1, 1, T)], 1).astype(np.float32)
    out = compare_actions_with_states(_scaled(a), None, P)
    st, inner = out["actual_states"].cpu().numpy(), out["inner_steps"].cpu().numpy()
    assert np.all(np.isfinite(st))
    checked, worst_env, worst_orc = 0, 0.0, 0.0
    for i in rng.choice(n, 160, replace=False):
        ref, steps = _oracle_states(P[:, i], a)
        assert list(inner[i, :len(steps)]) == steps, i
        env = SalpRobotVectorEnv(1, device="cuda:0", seed=5, output="numpy",
                                 **{name: float(P[j, i]) for j, name in enumerate(ROBOT_PARAM_NAMES)})
        rows = []
        for t in range(len(ref)):
            env.step(a[t][None])
            s = env.get_state()[:, 0]
            rows.append([s[R_POS], s[R_POS + 1], s[R_VEL], s[R_VEL + 1], s[R_EULER + 2], s[R_OMEGA + 2]])
        env.close()
        if len(ref):
            worst_env = max(worst_env, _rel(st[i, :len(ref)], np.array(rows)))
            assert _rel(st[i, 0], ref[0]) <= 1e-6, i
            worst_orc = max(worst_orc, _rel(st[i, :len(ref)], ref))
            checked += len(ref)
    print(f"160 random robots: worst relative difference to the device env {worst_env:.3g}, to the oracle {worst_orc:.3g}")
    assert worst_env <= 1e-6
    assert checked >= 400


def test_same_physics_as_the_env_step():
    """params NULL, shared actions: bit-identical to the env's state after each step, up to each robot's first done."""
    n, T = 3000, 8
    rng = np.random.default_rng(2)
    a = np.stack([rng.uniform(0, 1, T), rng.uniform(0, 0.3, T), rng.uniform(-1, 1, T)], 1).astype(np.float32)
    a[2] = (1.0, 1.0, -1.0)
    out = compare_actions_with_states(_scaled(a), None, None, num_robots=n)
    st, inner = out["actual_states"].cpu().numpy(), out["inner_steps"].cpu().numpy()
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=4, output="numpy")
    alive = np.ones(n, bool)
    for t in range(T):
        _, _, term, trunc, info = env.step(np.tile(a[t], (n, 1)))
        assert np.array_equal(info["inner_steps"][alive], inner[alive, t])
        alive &= ~(term | trunc)
        s = env.get_state()
        ref = np.stack([s[R_POS], s[R_POS + 1], s[R_VEL], s[R_VEL + 1], s[R_EULER + 2], s[R_OMEGA + 2]], 1)
        assert np.array_equal(st[alive, t], ref[alive]), t
    assert alive.any()
    env.close()


def test_default_parameters_equal_an_explicit_table():
    rng = np.random.default_rng(3)
    n, T = 1000, 5
    acts = _scaled(np.stack([rng.uniform(0, 1, (n, T)), rng.uniform(0, 0.3, (n, T)), rng.uniform(-1, 1, (n, T))], 2).astype(np.float32))
    x = rng.normal(0, 0.1, (T, 6))
    a = compare_actions_with_states(acts, x, None)
    b = compare_actions_with_states(acts, x, robot_params(n, "cuda:0"))
    for k in ("actual_states", "inner_steps") + KEYS:
        assert torch.equal(a[k], b[k]), k


def test_the_call_leaves_the_env_alone():
    n = 1500
    rng = np.random.default_rng(7)
    envs = [SalpRobotVectorEnv(n, device="cuda:0", seed=8) for _ in range(2)]
    a0 = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    for e in envs:
        e.step(a0)
    s0 = envs[0].get_state()
    acts = torch.as_tensor(_scaled(rng.uniform(0, 1, (6, 3)).astype(np.float32)), device="cuda:0")
    P = torch.as_tensor(random_robot_params(rng, n), device="cuda:0")
    st = torch.empty((6, n, 6), dtype=torch.float64, device="cuda:0")
    e0 = envs[0]
    assert _raw(e0, P, acts, 6, None, st, None, None, 1, e0._stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(e0.get_state(), s0)
    a1 = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    outs = [[x.clone() for x in e.step(a1)[:4]] for e in envs]
    for x0, x1 in zip(*outs):
        assert torch.equal(x0, x1)
    assert np.array_equal(envs[0].get_state(), envs[1].get_state())
    for e in envs:
        e.close()


def test_metrics():
    rng = np.random.default_rng(9)
    n, T = 2000, 7
    acts = _scaled(np.stack([rng.uniform(0, 1, T), rng.uniform(0, 0.3, T), rng.uniform(-1, 1, T)], 1).astype(np.float32))
    P = random_robot_params(rng, n)
    x = rng.normal(0, 0.2, (T, 6))
    full = compare_actions_with_states(acts, x, P)
    only = compare_actions_with_states(acts, x, P, metrics_only=True)
    assert "actual_states" not in only and "inner_steps" not in only
    for k in KEYS:
        assert torch.equal(full[k], only[k]), k
    checks = (("position_error", full["position_errors"].mean(1)), ("velocity_error", full["velocity_errors"].mean(1)),
              ("angle_error", full["angle_errors"].mean(1)), ("max_position_error", full["position_errors"].max(1).values),
              ("angular_velocity_error", full["errors"][..., 5].abs().mean(1)))
    for k, ref in checks:
        assert torch.all(torch.abs(full[k] - ref) <= 1e-12 * ref.abs()), k
    xn = x.copy()
    xn[3, 0] = np.nan
    nan = compare_actions_with_states(acts, xn, P, metrics_only=True)
    assert torch.all(torch.isnan(nan["position_error"])) and torch.all(torch.isnan(nan["max_position_error"]))
    assert torch.all(torch.isfinite(nan["velocity_error"])) and torch.equal(nan["velocity_error"], full["velocity_error"])


def test_system_identification_sanity():
    z = np.load(GOLD, allow_pickle=False)
    acts = z["actions_shared"]
    first = compare_actions_with_states(acts, None, z["params"])
    for k in (0, 3, 6):
        out = compare_actions_with_states(acts, first["actual_states"][k], z["params"], metrics_only=True)
        for m in KEYS:
            assert out[m][k].item() == 0.0, (k, m)
        assert int(out["position_error"].argmin()) == k and int(torch.count_nonzero(out["position_error"] == 0)) == 1


def test_bad_parameters_stay_in_their_lane():
    rng = np.random.default_rng(12)
    n, T = 256, 4
    P = random_robot_params(rng, n)
    acts = _scaled(np.array([[1.0, 0.1, 0.3], [0.5, 0.0, -1.0], [0.2, 0.2, 1.0], [1.0, 1.0, 0.0]], np.float32))
    clean = compare_actions_with_states(acts, None, P)["actual_states"].cpu().numpy()
    bad = P.copy()
    j = {name: i for i, name in enumerate(ROBOT_PARAM_NAMES)}
    bad[j["dry_mass"], 3] = np.nan
    bad[j["nozzle_area"], 10] = 0.0
    bad[j["init_width"], 40] = -0.15
    t0 = time.monotonic()
    got = compare_actions_with_states(acts, None, bad)["actual_states"].cpu().numpy()
    assert time.monotonic() - t0 < 5.0
    good = np.setdiff1d(np.arange(n), [3, 10, 40])
    assert _rel(got[good], clean[good]) <= 1e-9
    assert not np.all(np.isfinite(got[3]))


def test_rejected_arguments_launch_nothing():
    n, T = 300, 3
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=1)
    acts = torch.full((T, 3), 0.02, dtype=torch.float64, device="cuda:0")
    x = torch.zeros((T, 6), dtype=torch.float64, device="cuda:0")
    st = torch.full((1025, n, 6), SENTINEL, dtype=torch.float64, device="cuda:0")
    met = torch.full((n, 5), SENTINEL, dtype=torch.float64, device="cuda:0")
    inner = torch.full((1025, n), -7, dtype=torch.int32, device="cuda:0")
    L, h, s = env.L, env._h, env._stream
    # NULL handle, NULL actions, cycles outside [1, 1024], unknown flag bits, metrics without expected
    cases = [(None, acts, T, x, 1), (h, None, T, x, 1), (h, acts, 0, x, 1), (h, acts, -2, x, 1), (h, acts, 1025, x, 1),
             (h, acts, T, x, 1 | 4), (h, acts, T, x, 1 << 31), (h, acts, T, None, 1)]
    for hh, a, c, xx, f in cases:
        rc = L.salp_robot_vec_trajectory(hh, None, _ptr(a), c, _ptr(xx), _ptr(st), _ptr(met), _ptr(inner), f, s)
        assert rc == -1, (c, f)
        assert L.salp_robot_last_error().decode()
    tiny = SalpRobotVectorEnv(64, device="cuda:0", seed=1, dt=1e-9)
    assert _raw(tiny, None, acts, T, x, st, met, inner, 1, tiny._stream) == -1
    assert b"dt" in tiny.L.salp_robot_last_error()
    torch.cuda.synchronize()
    assert torch.all(st == SENTINEL) and torch.all(met == SENTINEL) and torch.all(inner == -7)
    # the cap itself is accepted
    one = SalpRobotVectorEnv(1, device="cuda:0", seed=1)
    a1 = torch.zeros((1024, 3), dtype=torch.float64, device="cuda:0")
    assert _raw(one, None, a1, 1024, None, st, None, None, 1, one._stream) == 0
    torch.cuda.synchronize()
    for e in (env, tiny, one):
        e.close()


def test_graph_replay_matches_eager():
    rng = np.random.default_rng(13)
    n, T = 3000, 5
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=2)
    acts = torch.as_tensor(_scaled(rng.uniform(0, 1, (T, 3)).astype(np.float32)), device="cuda:0")
    x = torch.as_tensor(rng.normal(0, 0.1, (T, 6)), device="cuda:0")
    P = torch.as_tensor(random_robot_params(rng, n), device="cuda:0")
    st = torch.empty((T, n, 6), dtype=torch.float64, device="cuda:0")
    met = torch.empty((n, 5), dtype=torch.float64, device="cuda:0")
    inner = torch.empty((T, n), dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = env.L.salp_robot_vec_trajectory(env._h, _ptr(P), _ptr(acts), T, _ptr(x), _ptr(st), _ptr(met), _ptr(inner), 1,
                                                 ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    P.copy_(torch.as_tensor(random_robot_params(rng, n), device="cuda:0"))
    g.replay()
    torch.cuda.synchronize()
    eager = compare_actions_with_states(acts, x, P.clone())
    assert torch.equal(st.transpose(0, 1), eager["actual_states"]) and torch.equal(inner.T, eager["inner_steps"])
    assert torch.equal(met, torch.stack([eager[k] for k in KEYS], 1))
    del g
    env.close()
