"""Cycle history of the HEAD simulator (salp_robot_vec_step_history, include/salp_robot.h) — the parts that need no
GPU: the C ABI is declared and exported, the channel enum matches the Python constants, and the reference's own
histories (tests/golden/history_robot_cycles.npz, gen_robot_history_golden.py) are consistent with themselves and
with the C oracle's end-of-cycle state.  The GPU side is tests/test_gpu_robot_history.py."""
import json
import os
import re

import numpy as np

import robot_oracle_lib as rol
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.robot_env import (H_COUNT, H_EULER, H_LENGTH, H_NOZZLE_YAW, H_OMEGA, H_POS, H_STATE, H_VEL,
                                                 H_WIDTH, HISTORY_CHANNELS, ROBOT_EXPORTS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "history_robot_cycles.npz")
NEW = ("salp_robot_vec_history_capacity", "salp_robot_vec_step_history")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "salp_robot.h")).read(), flags=re.S)


def test_history_abi_is_declared_and_exported():
    src = _header()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in ROBOT_EXPORTS
        assert hasattr(_capi.load_library(), name), name


def test_channel_enum_matches_python():
    body = re.search(r"enum\s*\{([^}]*SALP_H_COUNT[^}]*)\}", _header()).group(1)
    enum = {k: int(v) for k, v in re.findall(r"SALP_H_([A-Z_]+)\s*=\s*(\d+)", body)}
    assert enum == dict(POS=H_POS, VEL=H_VEL, EULER=H_EULER, OMEGA=H_OMEGA, LENGTH=H_LENGTH, WIDTH=H_WIDTH, STATE=H_STATE,
                        NOZZLE_YAW=H_NOZZLE_YAW, COUNT=H_COUNT)
    assert H_COUNT == 16 and sorted(c for c, _ in HISTORY_CHANNELS.values()) == [0, 3, 6, 9, 12, 13, 14, 15]


def _records(z):
    o = z["offsets"]
    for j in range(len(z["rec_case"])):
        yield j, z["history"][o[j]:o[j + 1]]


def test_fixture_is_self_consistent():
    z = np.load(GOLD, allow_pickle=False)
    assert z["history"].shape[1] == H_COUNT and z["history"].dtype == np.float64
    assert z["rec_truncated"].any() and (z["rec_inner_steps"] == 0).any() and z["rec_inner_steps"].max() > 1000
    fresh = 0
    for j, h in _records(z):
        k, t, i = int(z["rec_case"][j]), int(z["rec_step"][j]), int(z["rec_env"][j])
        act = z[f"c{k}_actions"][t, i].astype(np.float64)
        assert len(h) == z["rec_inner_steps"][j] + 1
        assert set(np.unique(h[:, H_STATE])) <= {0.0, 1.0, 2.0, 3.0}
        assert np.all(h[:, H_NOZZLE_YAW] == act[2] * (np.pi / 2))
        ended_before = t > 0 and any(z["rec_case"][m] == k and z["rec_step"][m] == t - 1 and z["rec_env"][m] == i and
                                     (z["rec_terminated"][m] or z["rec_truncated"][m]) for m in range(len(z["rec_case"])))
        if t == 0 or ended_before:                    # the first cycle of an episode starts from the reset pose
            fresh += 1
            assert np.all(h[0, H_POS:H_OMEGA + 3] == 0.0)
            assert h[0, H_STATE] == 3 and h[0, H_LENGTH] == 0.3 and h[0, H_WIDTH] == 0.15
    assert fresh >= 5


def test_fixture_last_samples_match_the_oracle():
    """The last sample of a cycle is the state the env step ends on: for cycles that do not end the episode it equals
    the C oracle's fp64 state after that step (position, body velocity, Euler angles, angular velocity)."""
    z = np.load(GOLD, allow_pickle=False)
    recs = {(int(z["rec_case"][j]), int(z["rec_step"][j]), int(z["rec_env"][j])): (j, h) for j, h in _records(z)}
    checked = 0
    for k, _ in enumerate(z["case_names"]):
        meta = json.loads(str(z[f"c{k}_meta"]))
        act = z[f"c{k}_actions"]
        T, n, _ = act.shape
        orc = rol.RobotOracleVec(n, seed=meta["seed"], env_index_base=meta["env_index_base"])
        orc.reset(np.zeros(n, np.uint8))
        for t in range(T):
            out = orc.step(act[t])
            want = [(i, recs[(k, t, i)]) for i in range(n) if (k, t, i) in recs]
            if not want:
                continue
            s = orc.get_state()
            for i, (j, h) in want:
                assert out["inner_steps"][i] == z["rec_inner_steps"][j]
                assert bool(out["truncated"][i]) == bool(z["rec_truncated"][j])
                if out["terminated"][i] or out["truncated"][i]:
                    continue
                last = h[-1]
                for row, ch in ((rol.R_POS, H_POS), (rol.R_VEL, H_VEL), (rol.R_EULER, H_EULER), (rol.R_OMEGA, H_OMEGA)):
                    ref = s[row:row + 3, i]
                    assert np.max(np.abs(last[ch:ch + 3] - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-6, (k, t, i, ch)
                checked += 1
        orc.close()
    assert checked >= 15
