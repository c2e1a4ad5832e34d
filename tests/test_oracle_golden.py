"""The CPU oracle (oracle/salp_oracle.c) against the golden vectors produced by the REFERENCE's own
Python implementation (tests/golden/gen_golden.py).  Bit-for-bit: f32 observations, fp64 rewards,
flags, info integers and the fp64 / integer end state."""
import numpy as np
import pytest

import oracle_lib as ol
from golden_util import fixture_names, load_fixture

NAMES = fixture_names()


def test_fixtures_present():
    assert len(NAMES) >= 20, NAMES
    assert sum(n.startswith("rt_") for n in NAMES) == 6, NAMES      # the vectors off the reference's default constants


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_vectors(name):
    z, meta, cfg = load_fixture(name)
    act = z["actions"]
    H, n, _ = act.shape
    orc = ol.OracleVec(cfg, n, seed=meta["seed"], env_index_base=meta["env_index_base"])
    if "inject_f64" in z.files:
        orc.set_state(z["inject_f64"], z["inject_i32"])
    assert np.array_equal(orc.observe(), z["reset_obs"]), "reset observation"
    if "food_schedule" in z.files:      # base_num_food_items pokes: roll out segment by segment
        cuts = [0] + [int(t) for t, _ in z["food_schedule"]] + [H]
        ks = [None] + [int(k) for _, k in z["food_schedule"]]
        parts = []
        for a, b, k in zip(cuts[:-1], cuts[1:], ks):
            if k is not None:
                orc.set_base_num_food(k)
            if b > a:
                parts.append(orc.rollout(np.ascontiguousarray(act[a:b]), want_final=True))
        out = {key: np.concatenate([p[key] for p in parts]) for key in ("terminated", "truncated", "info", "reward64", "obs", "final_obs")}
    else:
        out = orc.rollout(act, want_final=True)
    assert np.array_equal(out["terminated"], z["terminated"])
    assert np.array_equal(out["truncated"], z["truncated"])
    assert np.array_equal(out["info"], z["info"])
    assert np.array_equal(out["reward64"], z["reward"]), np.abs(out["reward64"] - z["reward"]).max()
    assert np.array_equal(out["obs"], z["obs"], equal_nan=True)
    assert np.array_equal(out["final_obs"], z["final_obs"], equal_nan=True)
    f64, i32 = orc.get_state()
    assert np.array_equal(i32, z["end_i32"]), np.nonzero(i32 != z["end_i32"])
    assert np.array_equal(f64, z["end_f64"], equal_nan=True)


def test_philox_known_answers():
    """Random123 kat_vectors for philox4x32-10."""
    assert ol.philox((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert ol.philox((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert ol.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_breathing_cycle_properties():
    """forced-breathing period 273 = 1 rest + 121 inhaling + 151 exhaling steps,
    61 thrust steps per cycle (exhale timer 15..75), |nozzle| <= pi/3, position inside the tank."""
    import underwater_swimmer_rl_amd as pkg
    cfg = pkg.load_env_config("single_food")
    orc = ol.OracleVec(cfg, 4, seed=3)
    act = np.random.default_rng(0).uniform(-1, 1, size=(600, 4, 1)).astype(np.float32)
    rng_before = orc.get_state()[1][ol.I_RNG_COUNTER].copy()
    out = orc.rollout(act)
    obs = out["obs"]
    phase = obs[:, 0, 7]
    assert (phase[:273] == 0.0).sum() == 1 and (phase[:273] == 0.5).sum() == 121 and (phase[:273] == 1.0).sum() == 151
    assert np.array_equal(obs[:273, :, 6], obs[273:546, :, 6])
    assert obs[0, 0, 6] == np.float32(1.3) and obs[121, 0, 6] == np.float32(1.1)
    assert np.abs(obs[..., 9]).max() <= 1.0
    # 61 jitter draws per cycle and env (no other draw happens without food / reset events)
    orc2 = ol.OracleVec(cfg, 4, seed=3)
    orc2.rollout(act[:273])
    assert np.all(orc2.get_state()[1][ol.I_RNG_COUNTER] - rng_before == 61)
