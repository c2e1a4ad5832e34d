"""The packed transition record (salp_vec_step_packed / salp_vec_rollout_packed, kernel signature 3) on the GPU: against a
twin handle running the unpacked entry points (bit for bit) and against the CPU oracle (the project's tolerances), on the
rollout-parity recipe of tests/parity_cases.py — every case ends episodes by wall and by truncation in mixed wavefronts.
Run with `pytest -m gpu`.

Layout under test (include/salp_vec.h "Packed transition record"): [obs | reward | flags word | food_collected |
steps_since_food | terminal observation of finished envs], flags bytes = terminated, truncated, collision, 0."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
from gpu_support import OBS_TOL, REW_TOL, assert_state_parity, device_state, started
from support import bits, free_port, obs_diff
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpLib
from underwater_swimmer_rl_amd.records import record_width, unpack_record

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D          # guard words behind the block (an unlikely float: -1.7e-16)
DEV = _capi.SALP_DEVICE_PTRS


@functools.lru_cache(maxsize=None)
def reference(name, n, H=pc.HORIZON, cfg_key=None):
    """The oracle's rollout of a case from the injected start state: computed once, shared, never written to."""
    cfg = pc.case_cfg(name) if cfg_key is None else pkg.load_env_config(cfg_key[0], **dict(cfg_key[1]))
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED, threads=4)
    act = pc.make_actions(cfg, H, n, seed=pc.ACTION_SEED)
    ref = orc.rollout(act, want_final=True)
    state = orc.get_state()
    orc.close()
    for a in (f64, i32, act, *state, *(v for v in ref.values() if v is not None)):
        a.setflags(write=False)
    return cfg, f64, i32, act, ref, state


def run_packed_device(dev, cfg, act, with_final):
    """rollout_packed with DEVICE pointers into a NaN-filled block followed by one guard step of sentinel words.
    Returns the block [H, n, width] and the guard, as host arrays."""
    import torch
    H, n = act.shape[:2]
    W = dev.record_width(with_final)
    assert W == record_width(cfg.obs_dim, with_final) == cfg.obs_dim + 4 + (cfg.obs_dim if with_final else 0)
    buf = torch.full((H + 1, n, W), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[H].view(torch.int32).fill_(int(np.uint32(SENTINEL).view(np.int32)))
    a = torch.tensor(act, device="cuda:0")          # (a copy: the shared reference stays read-only)
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    dev.rollout_packed(a, H, buf, None, DEV | (_capi.REC_FINAL_OBS if with_final else 0), 0)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[:H], host[H]


def run_twin(dev, cfg, act):
    H, n = act.shape[:2]
    out = dict(obs=np.empty((H, n, cfg.obs_dim), np.float32), reward=np.empty((H, n), np.float32),
               terminated=np.empty((H, n), np.uint8), truncated=np.empty((H, n), np.uint8),
               final_obs=np.full((H, n, cfg.obs_dim), np.nan, np.float32))
    dev.rollout(act, H, out["obs"], out["reward"], out["terminated"], out["truncated"], out["final_obs"], None, 0)
    return out


def check_record(cfg, rec, guard, ref, twin, with_final, label, need_done=True):
    """Every field of a record block against the oracle (tolerances) and, when given, the twin's unpacked outputs (bits).
    need_done: the block must contain finished episodes (a rollout; a single step of the acting path need not)."""
    D = cfg.obs_dim
    u = unpack_record(rec, D)
    assert np.shares_memory(u["obs"], rec) and u["terminated"].dtype == np.bool_ and u["food_collected"].dtype == np.int32
    term, trunc = u["terminated"].view(np.uint8), u["truncated"].view(np.uint8)
    assert np.array_equal(term, ref["terminated"]) and np.array_equal(trunc, ref["truncated"]), f"{label}: flags differ"
    assert np.array_equal(u["collision"], ref["info"][..., pc.INFO_COLLISION]), f"{label}: collision byte differs"
    assert np.array_equal(u["food_collected"], ref["info"][..., pc.INFO_FOOD_COLLECTED]), f"{label}: food_collected differs"
    assert np.array_equal(u["steps_since_food"], ref["info"][..., pc.INFO_STEPS_SINCE_FOOD]), f"{label}: steps_since_food differs"
    d = obs_diff(cfg, u["obs"], ref["obs"])
    assert d.max() <= OBS_TOL, f"{label}: obs diff {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    rd = np.abs(u["reward"].astype(np.float64) - ref["reward64"]) / np.maximum(1.0, np.abs(ref["reward64"]))
    assert rd.max() <= REW_TOL, f"{label}: reward diff {rd.max()}"
    assert not rec.view(np.uint8)[..., 4 * (D + _capi.REC_FLAGS) + 3].any(), f"{label}: byte 3 of a flags word is not 0"
    assert (guard.view(np.uint32) == SENTINEL).all(), f"{label}: words behind the block were written"
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert done.any() or not need_done, f"{label}: no episode ends"
    fin = u["final_observation"]
    if with_final:
        assert np.isnan(fin[~done]).all(), f"{label}: terminal words of unfinished rows were written"
        assert not np.isnan(fin[done]).any(), f"{label}: a finished row has no terminal observation"
        if done.any():
            fd = obs_diff(cfg, fin[done], ref["final_obs"][done])
            assert fd.max() <= OBS_TOL, f"{label}: final_obs diff {fd.max()}"
    else:
        assert fin is None and rec.shape[-1] == D + 4
    if twin is not None:        # same kernels' arithmetic (-ffp-contract=off), another output route: identical bits
        assert np.array_equal(bits(u["obs"]), bits(twin["obs"])), f"{label}: obs bits differ from the unpacked rollout"
        assert np.array_equal(bits(u["reward"]), bits(twin["reward"])), f"{label}: reward bits differ"
        assert np.array_equal(term, twin["terminated"]) and np.array_equal(trunc, twin["truncated"])
        if with_final:
            assert np.array_equal(bits(fin[done]), bits(twin["final_obs"][done])), f"{label}: terminal rows differ"
    return float(d.max()), float(rd.max())


def rollout_case(name, n, with_final, expect_launch, floors):
    cfg, f64, i32, act, ref, state = reference(name, n)
    H = act.shape[0]
    if floors:
        pc.assert_event_floors(name, pc.count_events(ref))
    dev, twin = started(cfg, n, f64, i32), started(cfg, n, f64, i32)
    rec, guard = run_packed_device(dev, cfg, act, with_final)
    tw = run_twin(twin, cfg, act)
    dmax, rmax = check_record(cfg, rec, guard, ref, tw, with_final, name)
    assert_state_parity(cfg, dev, state, name)
    assert_state_parity(cfg, twin, state, f"{name} (twin)")
    assert dev.stats() == twin.stats() and dev.stats()["env_steps"] == n * H
    assert dev.global_step == twin.global_step == H
    ll = dev.last_launch()
    assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == pc.EXPECT_KERNEL[name], ll
    assert {k: ll[k] for k in expect_launch} == expect_launch, ll
    assert ll["actions_in_kernel"] == 0
    print(f"{name} n={n} final={with_final}: max obs diff {dmax:.3g}, reward {rmax:.3g}, {pc.count_events(ref)}")
    dev.close()
    twin.close()


NARROW = ("single_food", "class_default_F5", "sac_gail_F12", "F16_sixteen_slots")


@pytest.mark.parametrize("name,with_final", [(c, True) for c in pc.CASES] + [(c, False) for c in NARROW])
def test_packed_rollout_matches_twin_and_oracle(name, with_final):
    n = pc.N_ENVS
    rollout_case(name, n, with_final, floors=True, expect_launch=dict(
        envs_unpredicated=n, envs_predicated=0, full_signature=3, signature_unpredicated=3, signature_predicated=-1))


@pytest.mark.parametrize("n", [pc.N_ENVS + 37, 37])
@pytest.mark.parametrize("name", ["single_food", "sac_gail_F12"])
def test_packed_ragged_batch_is_one_predicated_launch(name, n):
    """n H <= 2^22: one predicated launch over the whole range, in the packed layout (no fall-back to another signature).
    The event floors of the recipe are stated for 2048 envs and are held at 2048 + 37; at 37 envs alone (9 wall lanes)
    check_record still demands finished episodes, with terminal rows."""
    assert n * pc.HORIZON <= 1 << 22
    rollout_case(name, n, True, floors=n >= pc.N_ENVS, expect_launch=dict(
        envs_unpredicated=0, envs_predicated=n, full_signature=3, signature_unpredicated=-1, signature_predicated=3))


def test_packed_split_launch():
    """The smallest shape that splits (tests/test_gpu_parity.py::test_split_launch_with_final_obs_matches_oracle): 4096 envs
    unpredicated + 37 predicated, both halves in signature 3, both ending episodes."""
    key = ("sac_gail", (("max_steps_without_food", 300),))
    n, H = 4096 + 37, 1020
    cfg, f64, i32, act, ref, state = reference("split", n, H, key)
    ev_tail = pc.count_events({k: ref[k][:, 4096:] for k in ("terminated", "truncated", "info")})     # the predicated half
    assert ev_tail["wall"] > 0 and ev_tail["truncated"] > 0 and ev_tail["captures"] > 0, ev_tail
    dev = started(cfg, n, f64, i32)
    rec, guard = run_packed_device(dev, cfg, act, True)
    check_record(cfg, rec, guard, ref, None, True, "split launch")
    assert_state_parity(cfg, dev, state, "split launch")
    ll = dev.last_launch()
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (4096, 37), ll
    assert (ll["full_signature"], ll["signature_unpredicated"], ll["signature_predicated"]) == (3, 3, 3), ll
    dev.close()


@pytest.mark.parametrize("name", list(pc.STEP_CASES))
def test_step_packed_acting_path_matches_oracle(name):
    """salp_vec_step_packed with terminal observations and HOST pointers, step by step, every field against the oracle."""
    cfg, orc, f64, i32, act = pc.step_case(name)
    H, n = act.shape[:2]
    ref = orc.rollout(act, want_final=True)
    pc.assert_step_floors(name, pc.count_events(ref))
    state = orc.get_state()
    orc.close()
    dev = SalpLib(cfg, n, device_id=0, seed=pc.STEP_ENV_SEED)
    dev.set_state(f64, i32, 0)
    W = dev.record_width(True)
    buf = np.empty((2, n, W), np.float32)
    want = (dict(envs_unpredicated=0, envs_predicated=n, full_signature=3, signature_unpredicated=-1, signature_predicated=3)
            if n % 64 else
            dict(envs_unpredicated=n, envs_predicated=0, full_signature=3, signature_unpredicated=3, signature_predicated=-1))
    for t in range(H):
        buf[0].fill(np.nan)
        buf[1].view(np.uint32).fill(SENTINEL)
        dev.step_packed(act[t], buf[0], _capi.REC_FINAL_OBS)
        step_ref = {k: (None if v is None else v[t]) for k, v in ref.items()}
        check_record(cfg, buf[0], buf[1], step_ref, None, True, f"{name} step {t}", need_done=False)
        ll = dev.last_launch()
        assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == (12, 3, 1)
        assert {k: ll[k] for k in want} == want, ll
    assert dev.global_step == H
    assert_state_parity(cfg, dev, state, f"step_packed {name}")
    dev.close()


@pytest.mark.parametrize("foods,tank,min_wg,max_vgprs", [
    (1, False, 4, 128), (3, False, 4, 128), (5, False, 4, 128), (8, False, 4, 128), (12, False, 3, 168), (16, False, 3, 168),
    (5, True, 4, 128), (8, True, 4, 128), (1, True, 4, 128), (12, True, 3, 168), (16, True, 2, 256)])
def test_packed_kernel_occupancy_matches_the_design(foods, tank, min_wg, max_vgprs):
    """The table of tests/test_gpu_parity.py::test_kernel_occupancy_matches_the_design for the packed
    kernels, both record widths: the packed tile must not cost any instantiation a workgroup per CU (the 8-slot kernel
    would lose its fourth with a full-height packed tile), nor push it into scratch."""
    cfg = pc.make_cfg(dict(preset="sac_gail", num_food_items=foods, **(dict(width=801) if tank else {})))
    n, H = 2048, 4
    act = pc.make_actions(cfg, H, n, seed=1)
    dev = SalpLib(cfg, n, device_id=0, seed=3)
    for with_final in (False, True):
        rec = np.empty((H, n, dev.record_width(with_final)), np.float32)
        dev.rollout_packed(act, H, rec, None, _capi.REC_FINAL_OBS if with_final else 0)
        ll, res = dev.last_launch(), dev.last_kernel_resources()
        print(foods, tank, with_final, res)
        assert ll["literal_constants"] == (0 if tank else 1) and ll["full_signature"] == 3
        assert res["workgroups_per_cu"] >= min_wg, (ll, res)
        assert res["vgprs"] <= max_vgprs and res["scratch_bytes"] <= (32 if tank else 0), (ll, res)
    dev.close()


@pytest.mark.parametrize("preset", ["single_food", "sac_gail"])
def test_packed_rollout_with_device_generated_actions(preset):
    cfg = pkg.load_env_config(preset)
    n, H, seed = 640, 64, 9
    dev, twin = SalpLib(cfg, n, device_id=0, seed=seed), SalpLib(cfg, n, device_id=0, seed=seed)
    rec = np.empty((H, n, dev.record_width(False)), np.float32)
    a_p = np.empty((H, n, cfg.act_dim), np.float32)
    dev.rollout_packed(None, H, rec, a_p, 0)
    obs, rew = np.empty((H, n, cfg.obs_dim), np.float32), np.empty((H, n), np.float32)
    term, trunc = np.empty((H, n), np.uint8), np.empty((H, n), np.uint8)
    a_t = np.empty((H, n, cfg.act_dim), np.float32)
    twin.rollout(None, H, obs, rew, term, trunc, None, a_t, 0)
    u = unpack_record(rec, cfg.obs_dim)
    assert np.array_equal(a_p, a_t)
    assert np.array_equal(bits(u["obs"]), bits(obs)) and np.array_equal(bits(u["reward"]), bits(rew))
    assert np.array_equal(u["terminated"].view(np.uint8), term) and np.array_equal(u["truncated"].view(np.uint8), trunc)
    assert dev.global_step == twin.global_step == H
    assert dev.last_launch()["full_signature"] == 3 and dev.last_launch()["actions_in_kernel"] == 0
    # and the stream goes on where it stopped
    dev.rollout_packed(None, H, rec, a_p, 0)
    twin.rollout(None, H, obs, rew, term, trunc, None, a_t, 0)
    assert np.array_equal(a_p, a_t) and np.array_equal(bits(unpack_record(rec, cfg.obs_dim)["obs"]), bits(obs))
    assert dev.global_step == 2 * H
    dev.close()
    twin.close()


def test_packed_calls_refuse_bad_arguments():
    import ctypes
    import torch
    cfg = pkg.load_env_config("sac_gail")
    n, H = 256, 4
    dev = SalpLib(cfg, n, device_id=0, seed=1)
    W = dev.record_width(True)
    rec = torch.zeros((H * n * W + 4,), dtype=torch.float32, device="cuda:0")
    act = torch.zeros((H, n, cfg.act_dim), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    before = device_state(dev, cfg)
    vp, L, h = ctypes.c_void_p, dev.lib, dev._h
    p_rec, p_act = rec.data_ptr(), act.data_ptr()
    assert p_rec % 16 == 0
    F = DEV | _capi.REC_FINAL_OBS
    refusals = {
        "NULL rec (rollout)": L.salp_vec_rollout_packed(h, vp(p_act), H, None, None, F, None),
        "NULL rec (step)": L.salp_vec_step_packed(h, vp(p_act), None, F, None),
        "horizon 0": L.salp_vec_rollout_packed(h, vp(p_act), 0, vp(p_rec), None, F, None),
        "unknown flag bit": L.salp_vec_rollout_packed(h, vp(p_act), H, vp(p_rec), None, F | 4, None),
        "unknown flag bit (step)": L.salp_vec_step_packed(h, vp(p_act), vp(p_rec), DEV | 0x80000000, None),
        "misaligned device rec": L.salp_vec_rollout_packed(h, vp(p_act), H, vp(p_rec + 4), None, F, None),
        "misaligned device rec (step)": L.salp_vec_step_packed(h, vp(p_act), vp(p_rec + 8), DEV, None),
    }
    assert all(rc == -1 for rc in refusals.values()), refusals          # SALP_ERR_INVALID
    assert L.salp_last_error()
    torch.cuda.synchronize()
    after = device_state(dev, cfg)
    assert np.array_equal(before[0], after[0], equal_nan=True) and np.array_equal(before[1], after[1])
    assert dev.global_step == 0 and dev.stats()["env_steps"] == 0 and not rec.any()
    dev.rollout_packed(act, H, rec, None, F)                            # the same arguments, well-formed, are accepted
    torch.cuda.synchronize()
    assert dev.global_step == H and rec.any()
    dev.close()


ENV_CFG = dict(config="sac_gail", max_steps_without_food=40)
ENV_N, ENV_STEPS = 1024 + 37, 150


def assert_unpacked_equals_step_tuple(torch, u, tup, rec):
    obs, rew, term, trunc, info = tup
    lo, hi = rec.data_ptr(), rec.data_ptr() + rec.numel() * 4
    for k, v in u.items():
        assert lo <= v.data_ptr() < hi, f"{k} is not a view of the record"
    assert u["obs"].dtype == u["reward"].dtype == torch.float32 and u["terminated"].dtype == u["truncated"].dtype == torch.bool
    assert u["collision"].dtype == torch.uint8 and u["food_collected"].dtype == u["steps_since_food"].dtype == torch.int32
    assert torch.equal(u["obs"], obs) and torch.equal(u["reward"], rew)
    assert torch.equal(u["terminated"], term) and torch.equal(u["truncated"], trunc)
    assert torch.equal(u["food_collected"], info["food_collected"]) and torch.equal(u["steps_since_food"], info["steps_since_food"])
    assert torch.equal(u["collision"].to(torch.int32), info["collision"])
    done = info["_final_observation"]
    assert torch.equal(u["final_observation"][done], info["final_observation"][done])
    return int(done.sum())


def test_env_step_packed_and_rollout_packed():
    import torch
    env = pkg.SalpVectorEnv(num_envs=ENV_N, seed=5, **ENV_CFG)
    twin = pkg.SalpVectorEnv(num_envs=ENV_N, seed=5, **ENV_CFG)
    D = env.obs_dim
    g = torch.Generator(device=env.device).manual_seed(2)
    finished = 0
    for t in range(ENV_STEPS):
        a = torch.rand((ENV_N, env.act_dim), generator=g, device=env.device) * 2 - 1
        rec = env.step_packed(a)
        assert rec.shape == (ENV_N, 2 * D + 4) and rec.dtype == torch.float32
        finished += assert_unpacked_equals_step_tuple(torch, unpack_record(rec, D), twin.step(a), rec)
        assert env._lib.last_launch()["full_signature"] == 3
    assert finished > 0, "the twin finished no episode"
    narrow = env.step_packed(a, want_final_observation=False)
    o, r, te, tr, _ = twin.step(a)
    u = unpack_record(narrow, D)
    assert narrow.shape == (ENV_N, D + 4) and u["final_observation"] is None and torch.equal(u["obs"], o) and torch.equal(u["reward"], r)
    # rollout_packed == the twin's rollout, with and without an `out` block
    H = 48
    acts = torch.rand((H, ENV_N, env.act_dim), generator=g, device=env.device) * 2 - 1
    out = env.rollout_packed(acts, want_final_observation=True)
    tw = twin.rollout(acts, want_final_observation=True)
    u = unpack_record(out["record"], D)
    assert out["record"].shape == (H, ENV_N, 2 * D + 4) and out["actions"] is not None
    assert torch.equal(u["obs"], tw["obs"]) and torch.equal(u["reward"], tw["reward"])
    assert torch.equal(u["terminated"], tw["terminated"].bool()) and torch.equal(u["truncated"], tw["truncated"].bool())
    done = u["terminated"] | u["truncated"]
    assert bool(done.any()) and torch.equal(u["final_observation"][done], tw["final_obs"][done])
    mine = torch.zeros((H, ENV_N, D + 4), device=env.device)
    out = env.rollout_packed(None, horizon=H, out=mine)
    tw = twin.rollout(None, horizon=H)
    assert out["record"] is mine and torch.equal(out["actions"], tw["actions"])
    assert torch.equal(unpack_record(mine, D)["obs"], tw["obs"])
    with pytest.raises(ValueError):
        env.rollout_packed(acts, out=mine[:, :, :-1])
    env.close()
    twin.close()


def test_step_packed_is_graph_capturable():
    """Three step_packed calls captured with torch.cuda.graph, replayed twice == six eager steps on a twin."""
    import torch
    env = pkg.SalpVectorEnv(num_envs=ENV_N, seed=6, **ENV_CFG)
    twin = pkg.SalpVectorEnv(num_envs=ENV_N, seed=6, **ENV_CFG)
    D = env.obs_dim
    g = torch.Generator(device=env.device).manual_seed(3)
    acts = torch.rand((3, ENV_N, env.act_dim), generator=g, device=env.device) * 2 - 1
    kept = torch.zeros((3, ENV_N, 2 * D + 4), device=env.device)
    f64, i32 = env.get_state()
    side = torch.cuda.Stream(device=env.device)          # warm-up on a side stream, then back to the start state
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step_packed(acts[0])
    torch.cuda.current_stream(env.device).wait_stream(side)
    torch.cuda.synchronize()
    env.set_state(f64, i32)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(3):
            kept[k].copy_(env.step_packed(acts[k]))
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in range(3):
            obs, rew, term, trunc, info = twin.step(acts[k])
            u = unpack_record(kept[k], D)
            assert torch.equal(u["obs"], obs) and torch.equal(u["reward"], rew), (r, k)
            assert torch.equal(u["terminated"], term) and torch.equal(u["truncated"], trunc), (r, k)
            assert torch.equal(u["steps_since_food"], info["steps_since_food"]), (r, k)
    f_e, i_e = twin.get_state()
    f_g, i_g = env.get_state()
    assert np.array_equal(f_e, f_g, equal_nan=True) and np.array_equal(i_e, i_g)
    env.close()
    twin.close()


@pytest.mark.parametrize("gather_final", [True, False])
def test_sharded_step_gathers_the_kernels_records(gather_final):
    """ShardedSalpVectorEnv.step over RCCL (world size 1, shard 1 of 2): the engine's packed records are the collective's
    block; the 5-tuple equals a plain env's at the same global env indices — values, dtypes, terminal rows, mask."""
    import torch
    import torch.distributed as dist
    from underwater_swimmer_rl_amd.sharded import ShardedSalpVectorEnv
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n = ENV_N
        cfg = pkg.load_env_config(ENV_CFG["config"], max_steps_without_food=ENV_CFG["max_steps_without_food"])
        senv = ShardedSalpVectorEnv(cfg, 2 * n, device="cuda:0", seed=8, rehearse_shard=(1, 2),
                                    gather_final_observation=gather_final)
        twin = pkg.SalpVectorEnv(cfg, n, device="cuda:0", seed=8, env_index_base=n)
        assert senv.env_index_base == n and senv.local_envs == n
        g = torch.Generator(device=senv.device).manual_seed(4)
        finished = 0
        for t in range(ENV_STEPS):
            a = torch.rand((n, senv.act_dim), generator=g, device=senv.device) * 2 - 1
            obs, rew, term, trunc, info = senv.step(a)
            o2, r2, te2, tr2, i2 = twin.step(a)
            assert obs.shape == (n, cfg.obs_dim) and torch.equal(obs, o2) and torch.equal(rew, r2)
            assert term.dtype == trunc.dtype == torch.bool and torch.equal(term, te2) and torch.equal(trunc, tr2)
            for k in ("food_collected", "steps_since_food", "collision"):
                assert info[k].dtype == torch.int32 and info[k].shape == (n,) and torch.equal(info[k], i2[k]), (t, k)
                assert torch.equal(info["local"][k], i2[k])
            done = i2["_final_observation"]
            finished += int(done.sum())
            if gather_final:
                assert info["_final_observation"].dtype == torch.bool and torch.equal(info["_final_observation"], done)
                assert info["final_observation"].shape == (n, cfg.obs_dim)
                assert torch.equal(info["final_observation"][done], i2["final_observation"][done])
                assert torch.equal(info["local"]["final_observation"][done], i2["final_observation"][done])
            else:
                assert "final_observation" not in info and "_final_observation" not in info
            ll = senv.engine._lib.last_launch()
            assert ll["full_signature"] == 3 and ll["signature_predicated"] == 3, ll
        assert finished > 0
        twin.close()
        senv.close()
    finally:
        dist.destroy_process_group()
