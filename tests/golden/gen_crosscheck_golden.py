#!/usr/bin/env python3
"""Generates tests/golden/crosscheck_<case>.npz: long randomized runs of the reference's own SalpSnakeEnv
(tests/golden/ref_harness.py), recorded so that tests/test_oracle_vs_reference.py can hold the CPU oracle to them
bit for bit without the reference on the machine.  Also copies the reference's configs/<preset>.yaml files (settings
only) to tests/golden/ref_configs/.  Run in the build container:  python tests/golden/gen_crosscheck_golden.py

Each fixture holds inputs and expected outputs only (no reference source):
  case_json     preset, overrides, n, T, seed, action seed
  actions       f32 [T, n, act_dim]
  reset_obs     [n, obs_dim]          observation of the first reset(), as the reference returned it
  obs           [T, n, obs_dim]       returned observation (post-autoreset on finished steps)
  reward        f64 [T, n]
  terminated, truncated  u8 [T, n]
  done_tn       i32 [M, 2]            (t, env) of every finished step
  final_obs     [M, obs_dim]          the terminal observation of each finished step
Autoreset is emulated the way a VectorEnv drives the reference: when step() reports terminated or truncated,
reset() is called and its observation replaces the returned one.
"""
from __future__ import annotations

import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402
import underwater_swimmer_rl_amd as pkg  # noqa: E402

# (file suffix, preset, overrides) -- the cases of tests/test_oracle_vs_reference.py::test_bit_exact_against_reference
CASES = [
    ("single_food", "single_food", {}),
    ("single_food_long_horizon", "single_food_long_horizon", {}),
    ("sac_gail", "sac_gail", {}),
    ("single_food_free_breathing", "single_food", dict(forced_breathing=False)),
    ("sac_gail_random_count", "sac_gail", dict(num_food_items=4, random_food_count=True, max_steps_without_food=80)),
]
N, T, SEED, ACT_SEED = 3, 2500, 4321, 11
CONFIGS = ("single_food", "single_food_long_horizon", "sac_gail", "defaults")


def actions(cfg):
    rng = np.random.default_rng(ACT_SEED)
    act = rng.uniform(-1, 1, size=(T, N, cfg.act_dim)).astype(np.float32)
    if not cfg.forced_breathing:
        act[..., 0] = rng.uniform(0, 1, size=(T // 25 + 1, N)).repeat(25, axis=0)[:T]
    return act


def run_case(name, preset, over):
    cfg = pkg.load_env_config(preset, **over)
    act = actions(cfg)
    refs = [rh.ReferenceEnv(SEED, i, **cfg.env_kwargs()) for i in range(N)]
    reset_obs = np.stack([r.reset() for r in refs])
    obs = np.empty((T, N) + reset_obs.shape[1:], reset_obs.dtype)
    reward = np.empty((T, N), np.float64)
    term = np.zeros((T, N), np.uint8)
    trunc = np.zeros((T, N), np.uint8)
    done_tn, final_obs = [], []
    for t in range(T):
        for i, r in enumerate(refs):
            o, rew, te, tr, _ = r.step(act[t, i])
            reward[t, i] = rew
            term[t, i], trunc[t, i] = bool(te), bool(tr)
            if te or tr:
                done_tn.append((t, i))
                final_obs.append(np.asarray(o))
                o = r.reset()
            obs[t, i] = o
    path = os.path.join(HERE, f"crosscheck_{name}.npz")
    np.savez_compressed(
        path, case_json=json.dumps(dict(preset=preset, overrides=over, n=N, T=T, seed=SEED, action_seed=ACT_SEED)),
        actions=act, reset_obs=reset_obs, obs=obs, reward=reward, terminated=term, truncated=trunc,
        done_tn=np.asarray(done_tn, np.int32).reshape(-1, 2),
        final_obs=np.asarray(final_obs, obs.dtype).reshape(-1, obs.shape[-1]))
    print(f"{path}: {os.path.getsize(path)} bytes, {len(done_tn)} finished steps")


def main():
    if not rh.reference_available():
        raise SystemExit(f"reference not found under {rh.REFERENCE_ROOT}: run in the build container")
    os.makedirs(os.path.join(HERE, "ref_configs"), exist_ok=True)
    for name in CONFIGS:
        shutil.copyfile(os.path.join(rh.REFERENCE_ROOT, "configs", f"{name}.yaml"),
                        os.path.join(HERE, "ref_configs", f"{name}.yaml"))
    for case in CASES:
        run_case(*case)


if __name__ == "__main__":
    main()
