"""Cross-check of the CPU oracle against the reference's Python implementation on longer randomized runs than the
other committed vectors: the reference's outputs are recorded in tests/golden/crosscheck_*.npz and its
configs/*.yaml in tests/golden/ref_configs/ (both made by tests/golden/gen_crosscheck_golden.py)."""
import glob
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import underwater_swimmer_rl_amd as pkg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(preset, over):
    for path in sorted(glob.glob(os.path.join(GOLDEN, "crosscheck_*.npz"))):
        z = np.load(path, allow_pickle=False)
        case = json.loads(str(z["case_json"]))
        if case["preset"] == preset and case["overrides"] == over:
            return {k: z[k] for k in z.files}, case
    raise FileNotFoundError(f"no crosscheck fixture for {preset} {over}")


@pytest.mark.parametrize("preset,over", [
    ("single_food", {}), ("single_food_long_horizon", {}), ("sac_gail", {}),
    ("single_food", dict(forced_breathing=False)),
    ("sac_gail", dict(num_food_items=4, random_food_count=True, max_steps_without_food=80)),
])
def test_bit_exact_against_reference(preset, over):
    z, case = load_case(preset, over)
    cfg = pkg.load_env_config(preset, **over)
    n, T, seed = 3, 2500, 4321
    assert (case["n"], case["T"], case["seed"]) == (n, T, seed)
    orc = ol.OracleVec(cfg, n, seed=seed)
    assert np.array_equal(orc.observe(), z["reset_obs"])
    act = z["actions"]
    assert act.shape == (T, n, cfg.act_dim)
    out = orc.rollout(act, want_final=True)
    final = {(int(t), int(i)): k for k, (t, i) in enumerate(z["done_tn"])}
    ref_term, ref_trunc = z["terminated"].astype(bool), z["truncated"].astype(bool)
    assert len(final) == int(np.count_nonzero(ref_term | ref_trunc))
    for t in range(T):
        for i in range(n):
            assert z["reward"][t, i] == out["reward64"][t, i], (t, i)
            term, trunc = ref_term[t, i], ref_trunc[t, i]
            assert term == bool(out["terminated"][t, i]) and trunc == bool(out["truncated"][t, i]), (t, i)
            if term or trunc:
                assert np.array_equal(z["final_obs"][final[(t, i)]], out["final_obs"][t, i])
            assert np.array_equal(z["obs"][t, i], out["obs"][t, i]), (t, i)


def test_presets_match_reference_yaml():
    """config.PRESETS restates configs/*.yaml `environment.params`."""
    for name in ("single_food", "single_food_long_horizon", "sac_gail", "defaults"):
        a = pkg.load_env_config(name)
        b = pkg.load_env_config(os.path.join(GOLDEN, "ref_configs", f"{name}.yaml"))
        assert a == b, name
