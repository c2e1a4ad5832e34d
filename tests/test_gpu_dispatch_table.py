"""Which rollout kernel each call launches, pinned against a recorded table (tests/test_gpu_dispatch_table.json).

`salp_vec_last_launch` and `salp_vec_last_launch_signatures` report the kernel the dispatch picked: food slots, observed
capacity, literal constants, breathing, output signature, action source, the env counts of the unpredicated and of the
predicated launch, and each launch's own signature.  The table was recorded by this file (`python
tests/test_gpu_dispatch_table.py --record FILE`) at the commit before the rollout kernels moved into units of their own and
the dispatch began to return the signature it picked; every row must stay as it was.

Rows: every handle class (1, 4, 8, 12 and 16 food slots with K = 3, literal and run-time constants, forced and free
breathing; K = 2 with 5 and with 14 foods) x every call kind the class supports x three env counts, H = 2, device pointers:
  164      two whole wavefronts and 36 more envs.  With H = 2 this is a small ragged batch (n_envs x H <= 2^22), which the
           library runs as ONE predicated launch over all 164 envs: the recorded rows say 0 / 164, not 128 / 36.
  100      the single predicated launch of a batch below two wavefronts.
  2^21+36  the smallest batch that H = 2 splits in two (n_envs x H > 2^22): an unpredicated launch over 2^21 envs and a
           predicated one over the last 36.  Here both launches are asserted to have been issued, with both signatures
           (salp_vec_step is one step: 2^21 + 36 <= 2^22, one predicated launch again).
"""
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import parity_cases as pc
import sampled_cases as sc
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpLib

pytestmark = pytest.mark.gpu

TABLE = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
H = 2
DEV = _capi.SALP_DEVICE_PTRS
SPLIT = (1 << 21) + 36
ENV_COUNTS = (164, 100, SPLIT)
KEYS = ("food_slots", "observed_capacity", "literal_constants", "forced", "full_signature", "actions_in_kernel",
        "envs_unpredicated", "envs_predicated", "signature_unpredicated", "signature_predicated")


def handle_classes():
    out = {}
    for breathing in ("forced", "free"):
        forced = breathing == "forced"
        for slots, foods in ((1, 1), (4, 3), (8, 5), (12, 12), (16, 16)):
            preset = "single_food" if foods == 1 else "sac_gail"
            out[f"F{slots}_literal_{breathing}"] = dict(preset=preset, num_food_items=foods, forced_breathing=forced)
            out[f"F{slots}_other_tank_{breathing}"] = dict(preset=preset, num_food_items=foods, forced_breathing=forced, width=900)
        for foods in (5, 14):
            out[f"K2_F{foods}_{breathing}"] = dict(preset="sac_gail", num_food_items=foods, max_observed_food=2, forced_breathing=forced)
    return out


CLASSES = handle_classes()
CALLS_ANY = ("step", "rollout", "rollout_final_obs", "rollout_no_reward", "rollout_generated", "packed", "packed_tail")
CALLS_K3 = ("policy", "policy_sampled", "evaluate", "evaluate_sampled")


def call_kinds(cfg):
    return CALLS_ANY + (CALLS_K3 if cfg.max_observed_food == 3 else ())


def rows_of(name):
    """{"<class>/<n_envs>/<call>": [the ten values of KEYS]} of one handle class, from the GPU."""
    import torch
    cfg = pc.make_cfg(CLASSES[name])
    rows = {}
    for n in ENV_COUNTS:
        dev = SalpLib(cfg, n, device_id=0, seed=3)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
        act, act_out = f32(H, n, cfg.act_dim), f32(H, n, cfg.act_dim)
        obs, fin, rew, logp = f32(H, n, cfg.obs_dim), f32(H, n, cfg.obs_dim), f32(H, n), f32(H, n)
        term, trunc = u8(H, n), u8(H, n)
        info = torch.zeros((n, _capi.INFO_COLS), dtype=torch.int32, device="cuda:0")
        rec, rec_tail = f32(H, n, dev.record_width(False)), f32(H, n, dev.record_width(True))
        summary = torch.zeros((n, _capi.EVAL_WORDS), dtype=torch.int32, device="cuda:0")
        ph = None
        if cfg.max_observed_food == 3:
            ph = dev.policy_create(sc.gaussian_policy(cfg.obs_dim, cfg.act_dim, (16,), 7, 1.0, 1.0, (-1.0,) * cfg.act_dim,
                                                      free_breathing=not cfg.forced_breathing))
        run = {
            "step": lambda: dev.step(act[0], obs[0], rew[0], term[0], trunc[0], fin[0], info, DEV),
            "rollout": lambda: dev.rollout(act, H, obs, rew, term, trunc, None, None, DEV),
            "rollout_final_obs": lambda: dev.rollout(act, H, obs, rew, term, trunc, fin, None, DEV),
            "rollout_no_reward": lambda: dev.rollout(act, H, obs, None, term, trunc, None, None, DEV),
            "rollout_generated": lambda: dev.rollout(None, H, obs, rew, term, trunc, None, act_out, DEV),
            "packed": lambda: dev.rollout_packed(act, H, rec, None, DEV),
            "packed_tail": lambda: dev.rollout_packed(act, H, rec_tail, None, DEV | _capi.REC_FINAL_OBS),
            "policy": lambda: dev.rollout_policy(ph, H, obs, rew, term, trunc, act_out, DEV),
            "policy_sampled": lambda: dev.rollout_policy_sampled(ph, H, obs, rew, term, trunc, act_out, logp, DEV),
            "evaluate": lambda: dev.evaluate_policy(ph, H, summary, DEV),
            "evaluate_sampled": lambda: dev.evaluate_policy_sampled(ph, H, summary, DEV),
        }
        for kind in call_kinds(cfg):
            run[kind]()
            launch = dev.last_launch()
            rows[f"{name}/{n}/{kind}"] = [launch[k] for k in KEYS]
        torch.cuda.synchronize()
        dev.close()
    return rows


def expected_keys():
    return {f"{name}/{n}/{kind}" for name, spec in CLASSES.items() for n in ENV_COUNTS for kind in call_kinds(pc.make_cfg(spec))}


def test_the_table_covers_every_combination():
    with open(TABLE) as f:
        table = json.load(f)
    assert set(table) == expected_keys()
    assert len(CLASSES) == 24 and len(table) == 3 * (20 * 11 + 4 * 7)


@pytest.mark.parametrize("name", list(CLASSES))
def test_every_call_launches_the_recorded_kernel(name):
    with open(TABLE) as f:
        table = json.load(f)
    rows = rows_of(name)
    wrong = {k: (v, table.get(k)) for k, v in rows.items() if table.get(k) != v}
    assert not wrong, f"(now, recorded) by {KEYS}: {wrong}"
    for k, v in rows.items():
        row = dict(zip(KEYS, v))
        n, kind = int(k.split("/")[1]), k.split("/")[2]
        if n * (1 if kind == "step" else H) > 1 << 22:      # both launches were issued, each with a signature of its own
            assert (row["envs_unpredicated"], row["envs_predicated"]) == (n // 64 * 64, n % 64) == (1 << 21, 36), k
            assert row["signature_unpredicated"] >= 0 and row["signature_predicated"] >= 0, k
            assert row["full_signature"] == row["signature_unpredicated"], k
        else:               # a small ragged batch: one predicated launch over all of it
            assert (row["envs_unpredicated"], row["envs_predicated"]) == (0, n), k
            assert row["signature_unpredicated"] == -1 and row["full_signature"] == row["signature_predicated"] >= 0, k
    assert sum(v[6] > 0 and v[7] > 0 for v in rows.values()) == len(rows) // 3 - 1      # every call kind but the one-step call


if __name__ == "__main__":
    assert sys.argv[1] == "--record", __doc__
    table = {}
    for name in CLASSES:
        table.update(rows_of(name))
    assert set(table) == expected_keys()
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in sorted(table.items())) + "\n}\n")
    print(f"{len(table)} rows -> {sys.argv[2]}")
