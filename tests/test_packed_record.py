"""The packed transition record without a GPU: the layout helpers (records.py) on oracle rollouts, the binding's constants
against the header, the sharded step's packed fast path under gloo, and the packed LDS tile against the bank model."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle_lib as ol
import parity_cases as pc
from support import free_port
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi, records
from underwater_swimmer_rl_amd.records import pack_record, record_width, unpack_record
from underwater_swimmer_rl_amd.sharded import ShardedSalpVectorEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_rollout(K, n=64, H=200):
    cfg = pkg.load_env_config("sac_gail", max_observed_food=K, max_steps_without_food=40)
    act = np.random.default_rng(K).uniform(-1, 1, size=(H, n, cfg.act_dim)).astype(np.float32)
    orc, _, _ = pc.start_oracle(cfg, n, 3)       # the parity recipe's start state: wall contacts as well as truncations
    ref = orc.rollout(act, want_final=True)
    orc.close()
    return cfg, ref


@pytest.mark.parametrize("K,width,width_final", [(0, 16, 28), (3, 28, 52), (8, 48, 92)])
@pytest.mark.parametrize("as_torch", [False, True])
def test_pack_unpack_round_trip(K, width, width_final, as_torch):
    cfg, ref = oracle_rollout(K)
    D = cfg.obs_dim
    assert (record_width(D, False), record_width(D, True)) == (width, width_final)
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert done.any() and ref["info"][..., 2].any(), "the rollout must finish episodes, some by collision"
    for fin in (None, ref["final_obs"]):
        rec = pack_record(ref["obs"], ref["reward"], ref["terminated"], ref["truncated"], ref["info"], fin)
        assert rec.dtype == np.float32 and rec.shape == done.shape + (width if fin is None else width_final,)
        # the layout, word by word
        words = rec.view(np.uint32)
        assert np.array_equal(words[..., D + 1], ref["terminated"].astype(np.uint32) | (ref["truncated"].astype(np.uint32) << 8)
                              | ((ref["info"][..., 2] != 0).astype(np.uint32) << 16))
        assert np.array_equal(rec.view(np.int32)[..., D + 2], ref["info"][..., 0])
        assert np.array_equal(rec.view(np.int32)[..., D + 3], ref["info"][..., 1])
        block = torch.from_numpy(rec) if as_torch else rec
        u = unpack_record(block, D)
        host = {k: (v.numpy() if as_torch and v is not None else v) for k, v in u.items()}
        if as_torch:
            lo, hi = block.data_ptr(), block.data_ptr() + block.numel() * 4
            assert all(lo <= v.data_ptr() < hi for v in u.values() if v is not None)
            assert u["terminated"].dtype == u["truncated"].dtype == torch.bool and u["collision"].dtype == torch.uint8
            assert u["food_collected"].dtype == u["steps_since_food"].dtype == torch.int32
        else:
            assert all(np.shares_memory(v, rec) for v in u.values() if v is not None)
            assert u["terminated"].dtype == u["truncated"].dtype == np.bool_ and u["collision"].dtype == np.uint8
            assert u["food_collected"].dtype == u["steps_since_food"].dtype == np.int32
        assert np.array_equal(host["obs"], ref["obs"]) and np.array_equal(host["reward"], ref["reward"])
        assert np.array_equal(host["terminated"], ref["terminated"].astype(bool))
        assert np.array_equal(host["truncated"], ref["truncated"].astype(bool))
        assert np.array_equal(host["collision"], ref["info"][..., 2])
        assert np.array_equal(host["food_collected"], ref["info"][..., 0])
        assert np.array_equal(host["steps_since_food"], ref["info"][..., 1])
        if fin is None:
            assert host["final_observation"] is None
        else:
            assert np.array_equal(host["final_observation"], fin, equal_nan=True)
        # a view: writing through it changes the block
        u["food_collected"][0, 0] = 77
        assert rec.view(np.int32)[0, 0, D + 2] == 77
    with pytest.raises(ValueError):
        unpack_record(np.zeros((4, width + 1), np.float32), D)


def test_binding_constants_equal_the_header():
    with open(os.path.join(ROOT, "include", "salp_vec.h")) as f:
        header = f.read()
    m = re.search(r"enum \{ (SALP_REC_REWARD = 0[^}]*) \};", header)
    names = [x.split("=")[0].strip() for x in m.group(1).split(",")]
    assert names == ["SALP_REC_REWARD", "SALP_REC_FLAGS", "SALP_REC_FOOD_COLLECTED", "SALP_REC_STEPS_SINCE_FOOD", "SALP_REC_EXTRA_COLS"]
    for i, name in enumerate(names):
        assert getattr(_capi, name[len("SALP_"):]) == i and getattr(records, name[len("SALP_"):]) == i
    assert int(re.search(r"SALP_REC_FINAL_OBS = (\d+)u", header).group(1)) == _capi.REC_FINAL_OBS == 2
    assert int(re.search(r"SALP_DEVICE_PTRS = (\d+)u", header).group(1)) == _capi.SALP_DEVICE_PTRS
    for fn in ("salp_vec_record_width", "salp_vec_step_packed", "salp_vec_rollout_packed"):
        assert fn in _capi.EXPORTS and re.search(r"\bint " + fn + r"\(", header)
    assert pkg.unpack_record is unpack_record and pkg.pack_record is pack_record and pkg.record_width is record_width


# ---- the sharded step's packed fast path under gloo
class PlainEngine:
    """The oracle with the HIP engine's `step` (the engine of tests/test_sharded_gloo.py): no `step_packed`."""

    def __init__(self, cfg, n, seed, base):
        self.o = ol.OracleVec(cfg, n, seed=seed, env_index_base=base)

    def reset(self, seed=None, options=None):
        return self.o.reset(), {}

    def _out(self, actions):
        out = self.o.step(np.asarray(actions, np.float32), want_final=True)
        done = (out["terminated"] | out["truncated"]).astype(bool)
        out["final_obs"] = np.where(done[:, None], out["final_obs"], 0.0).astype(np.float32)   # unfinished rows: unspecified
        return out, done

    def step(self, actions):
        out, done = self._out(actions)
        info = {"food_collected": out["info"][:, 0], "steps_since_food": out["info"][:, 1], "collision": out["info"][:, 2],
                "final_observation": out["final_obs"], "_final_observation": done}
        return out["obs"], out["reward"], out["terminated"].astype(bool), out["truncated"].astype(bool), info

    def close(self):
        self.o.close()


class PackedEngine(PlainEngine):
    """The same engine offering `step_packed`, built with pack_record."""

    def step_packed(self, actions, want_final_observation=True):
        out, _ = self._out(actions)
        return pack_record(out["obs"], out["reward"], out["terminated"], out["truncated"], out["info"],
                           out["final_obs"] if want_final_observation else None)


def _worker(rank, world, port, tmp):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = pkg.load_env_config("sac_gail", max_steps_without_food=40)
        N, H, seed = 64, 120, 5
        act = np.random.default_rng(0).uniform(-1, 1, size=(H, N, 1)).astype(np.float32)
        plain = ShardedSalpVectorEnv(cfg, N, seed=seed, engine_factory=lambda c, n, s, b: PlainEngine(c, n, s, b))
        packed = ShardedSalpVectorEnv(cfg, N, seed=seed, engine_factory=lambda c, n, s, b: PackedEngine(c, n, s, b))
        narrow = ShardedSalpVectorEnv(cfg, N, seed=seed, engine_factory=lambda c, n, s, b: PackedEngine(c, n, s, b),
                                      gather_final_observation=False)
        finished = 0
        lo, hi = rank * (N // world), (rank + 1) * (N // world)
        for t in range(H):
            a = torch.from_numpy(act[t])
            o1, r1, te1, tr1, i1 = plain.step(a)
            o2, r2, te2, tr2, i2 = packed.step(a)
            o3, r3, te3, tr3, i3 = narrow.step(a)
            for x, y, z in ((o1, o2, o3), (r1, r2, r3), (te1, te2, te3), (tr1, tr2, tr3)):
                assert x.dtype == y.dtype == z.dtype and x.shape == y.shape and torch.equal(x, y) and torch.equal(x, z), t
            assert set(i1) == set(i2) and set(i3) == set(i1) - {"final_observation", "_final_observation"}
            for k in ("food_collected", "steps_since_food", "collision", "_final_observation"):
                assert i1[k].dtype == i2[k].dtype and i1[k].shape == i2[k].shape and torch.equal(i1[k], i2[k]), (t, k)
                assert torch.equal(i2["local"][k], i2[k][lo:hi])
            assert i3["collision"].dtype == torch.int32 and torch.equal(i3["steps_since_food"], i1["steps_since_food"])
            done = i1["_final_observation"]
            finished += int(done.sum())
            assert i1["final_observation"].shape == i2["final_observation"].shape
            assert torch.equal(i1["final_observation"][done], i2["final_observation"][done]), t
        assert finished > 0
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write(str(finished))
        for e in (plain, packed, narrow):
            e.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_step_packed_path_equals_the_packing_path(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    counts = [int(open(tmp_path / f"ok{r}").read()) for r in range(world)]
    assert counts[0] == counts[1] > 0          # every rank saw the same gathered batch finish episodes


# ---- the packed LDS tile
def test_packed_tile_is_the_modelled_layout_and_conflict_free():
    spec = importlib.util.spec_from_file_location("isa_lds_model", os.path.join(ROOT, "profiles", "isa_lds_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    # the kernel's own formulas (salp_vec.hip, PACKED, K = 3): QPMAX = 7, PITCH = 4 QPMAX floats, no swizzle; lane l writes
    # column q of row l (l & 31 in a half-height tile) at myrow4[q]; store j of a pass reads float4 j*64 + lane + r (PITCH/4 - NQ)
    QPMAX = NQ = 7
    PITCH = 4 * QPMAX
    assert m.QP == QPMAX
    for rows in (64, 32):
        for lane in range(64):
            for q in range(QPMAX):
                assert 4 * ((lane % rows) * PITCH + 4 * q) == m.PACKED(lane % rows, q)
        for j in range((rows * QPMAX + 63) // 64):
            for lane in range(64):
                f = j * 64 + lane
                if f < rows * NQ:
                    r = f // NQ
                    assert 16 * (f + r * (PITCH // 4 - NQ)) == m.PACKED(r, f - r * NQ)
        assert m.model_packed(rows=rows) == (8 * QPMAX, 4 * QPMAX)          # one LDS cycle per lane group: no conflict
    assert m.model_stash() == (8, 4)
    # the stash (tile bytes 384 .. 1407) clears what the rare paths use (0 .. 383) and fits the smallest tile (32 rows)
    assert 384 + 64 * 16 <= 32 * 4 * PITCH
    # DESIGN.md section 3.1 states these figures
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    w, rd = m.model_packed()
    assert re.search(rf"packed\s+tile[^.]*\b{w}\s+LDS\s+cycles[^.]*row\s+writes[^.]*\b{rd}\b[^.]*flush\s+reads", design), \
        "DESIGN.md 3.1 must state the modelled cycles of the packed tile"
