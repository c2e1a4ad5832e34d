"""HEAD-simulator oracle (oracle/salp_robot_oracle.c) against vectors produced by the reference's own
robot.py + salp_robot_env.py (tests/golden/gen_robot_golden.py).  The reference's 3x3 products go
through numpy/BLAS whose summation order is unspecified, so the pin is a tolerance: flags and
inner-step counts identical; observations / rewards / fp64 end state within 1e-6 (relative to
max(1, |x|)) — the measured deviation is ~1e-8 after thousands of Euler steps."""
import glob
import json
import os

import numpy as np
import pytest

import robot_oracle_lib as rol
from support import rel

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robot_*.npz")))
TOL = 1e-6
TANK_KEYS = ("width", "height", "tank_margin")


def test_fixtures_present():
    assert len(GOLD) == 6


def robot_config(meta):
    """The oracle's configuration for a vector: the reference's own, with the tank the vector's `meta` names (if any)."""
    cfg = rol.default_robot_config()
    for k in TANK_KEYS:
        if k in meta:
            setattr(cfg, k, meta[k])
    return cfg


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_robot_oracle_matches_reference_vectors(path):
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    act = z["actions"]
    T, n, _ = act.shape
    orc = rol.RobotOracleVec(n, seed=meta["seed"], env_index_base=meta["env_index_base"], cfg=robot_config(meta))
    assert rel(orc.reset(np.zeros(n, np.uint8)), z["reset_obs"]) <= TOL
    for t in range(T):
        out = orc.step(act[t])
        assert np.array_equal(out["terminated"], z["terminated"][t]) and np.array_equal(out["truncated"], z["truncated"][t]), t
        assert np.array_equal(out["inner_steps"], z["inner_steps"][t]), t
        assert rel(out["obs"], z["obs"][t]) <= TOL and rel(out["reward"], z["reward"][t]) <= TOL, t
        done = (z["terminated"][t] | z["truncated"][t]).astype(bool)
        assert np.array_equal(~np.isnan(out["final_obs"][:, 0]), done)
        if done.any():
            assert rel(out["final_obs"][done], z["final_obs"][t][done]) <= TOL
    assert rel(orc.get_state(), z["end_state"]) <= TOL
    orc.close()


def test_other_tank_vectors_hold_their_events():
    """What the three vectors off the reference's 900x700 tank were made for, from the stored arrays."""
    z = {os.path.basename(p)[6:-4]: np.load(p, allow_pickle=False) for p in GOLD}
    metas = {k: json.loads(str(v["meta"])) for k, v in z.items()}
    assert [metas[k].get(t) for k in ("target_reached", "small_tank", "wide_tank") for t in TANK_KEYS] == \
        [100, 100, 50, 300, 260, 35, 2400, 1800, 20]
    assert not any(t in metas[k] for k in ("cycles", "max_cycles", "out_of_bounds") for t in TANK_KEYS)
    r = z["target_reached"]
    term, inner = r["terminated"].astype(bool), r["inner_steps"]
    assert r["actions"].shape[:2] == (12, 4) and term.sum() >= 20
    assert (r["end_state"][rol.R_TARGET:rol.R_TARGET + 2] == 0.0).all()                # every target is the origin
    assert (term[:, 0::2].any(axis=1) & (~term[:, 1::2] & (inner[:, 1::2] > 100)).any(axis=1)).any()
    assert (r["reward"][term] > 9.0).all()                                             # the +10 of reaching the target
    for name, reach in (("small_tank", (0.575, 0.475)), ("wide_tank", (5.9, 4.4))):
        s = z[name]
        assert s["actions"].shape[:2] == (40, 4)
        tx, ty = np.abs(s["end_state"][rol.R_TARGET]), np.abs(s["end_state"][rol.R_TARGET + 1])
        assert (tx <= reach[0] + 1e-6).all() and (ty <= reach[1] + 1e-6).all(), name
    w = z["wide_tank"]
    assert w["truncated"].sum() >= 1 and w["actions"].shape[0] < 500                   # 40 cycles, not 500: distance > 5 m
    gone = w["final_obs"][w["truncated"].astype(bool)]
    assert (np.hypot(gone[:, 0], gone[:, 1]) > 5.0).all()                              # obs 0-1: position minus target
    assert np.hypot(*w["end_state"][rol.R_TARGET:rol.R_TARGET + 2]).max() > 2.9        # a target the default tank cannot place


def test_cycle_structure():
    """One env step is a whole cycle: (contraction/0.02 + contraction/0.04 + coast) / 0.01 Euler steps."""
    orc = rol.RobotOracleVec(3, seed=1)
    a = np.array([[0.5, 0.1, 0.0], [0.0, 0.0, 0.3], [1.0, 1.0, -1.0]], np.float32)
    out = orc.step(a)
    expect = [(0.03 / 0.02 + 0.03 / 0.04 + 1.0) / 0.01, 0.0, (0.06 / 0.02 + 0.06 / 0.04 + 10.0) / 0.01]
    assert abs(out["inner_steps"][0] - expect[0]) <= 1 and out["inner_steps"][1] == 0 and abs(out["inner_steps"][2] - expect[2]) <= 1
    s = orc.get_state()
    assert s[rol.R_CYCLE].tolist() == [1.0, 1.0, 1.0]
    assert s[rol.R_POS + 2].max() < 1e-6          # planar motion: z stays ~0
    orc.close()
