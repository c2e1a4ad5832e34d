"""salp_vec_evaluate_policy on the GPU: closed-loop runs with the policy inside the kernel and NO per-step output, one
summary record per env (include/salp_vec.h "Policy evaluation"), over the case table of tests/policy_cases.py.  Run with
`pytest -m gpu`.

Per case: the record against `policy.summarize_rollout` of what salp_vec_rollout_policy writes from the same start state
(integers identical, the two float64 sums bit for bit), the food count against the oracle stepped on the actions taken and
against the statistics, the final state / global step / statistics against the rollout's; 100 + 284 steps with
SALP_EVAL_ACCUMULATE against 384 in one call; populations; no_autoreset; device pointers with guard words; refusals;
hipGraph capture with a weight update between replays; the SalpVectorEnv surface."""
import functools

import numpy as np
import pytest

import evaluate_cases as ec
import parity_cases as pc
import policy_cases as cases
from gpu_support import device_state, run_policy, started
from support import fields_diff, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpError, SalpLib
from underwater_swimmer_rl_amd.policy import MLPPolicy, evaluation_views, summarize_rollout

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
DEV, ACC = _capi.SALP_DEVICE_PTRS, _capi.EVAL_ACCUMULATE
W = _capi.EVAL_WORDS
H, CUT = cases.H, ec.CUT


def fresh_record(n, fill=0x5A):
    return np.full((n, W), np.int32(fill * 0x01010101), np.int32)        # junk: a call without ACCUMULATE overwrites it


def record_diff(got, want):
    return fields_diff(got, want, evaluation_views, ("return_sum", "first_return", "first_length", "first_end", "episodes", "food"))


@functools.lru_cache(maxsize=None)
def device_run(name):
    """A case on the GPU, computed once, shared, read-only: salp_vec_rollout_policy on one handle, salp_vec_evaluate_policy on
    a twin handle put into the same injected start state with set_state (a fresh handle, not the first one set back: the
    running episode return behind `episode_return_sum` is not part of a snapshot)."""
    c, cfg, policy, f64, i32 = cases.start_snapshot(name)
    n = c["n"]
    roll = started(cfg, n, f64, i32)
    ph_r = roll.policy_create(policy)
    out = run_policy(roll, ph_r, cfg, H)
    roll_end = dict(state=device_state(roll, cfg), stats=roll.stats(), step=roll.global_step, launch=roll.last_launch(),
                    res=roll.last_kernel_resources())
    ph_r.close()
    roll.close()
    ev = started(cfg, n, f64, i32)
    ph_e = ev.policy_create(policy)
    rec = fresh_record(n)
    step0, stats0 = ev.global_step, ev.stats()
    ev.evaluate_policy(ph_e, H, rec, 0)
    ev_end = dict(state=device_state(ev, cfg), stats=ev.stats(), step=ev.global_step, launch=ev.last_launch(),
                  res=ev.last_kernel_resources())
    ph_e.close()
    ev.close()
    assert step0 == 0 and stats0["env_steps"] == 0
    for a in (rec, *out.values(), *roll_end["state"], *ev_end["state"]):
        a.setflags(write=False)
    return dict(c=c, cfg=cfg, policy=policy, f64=f64, i32=i32, out=out, rec=rec, roll=roll_end, ev=ev_end)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_equals_the_rollout_it_replaces(name):
    r = device_run(name)
    c, cfg, out, rec, n = r["c"], r["cfg"], r["out"], r["rec"], r["c"]["n"]
    assert not np.isnan(out["reward"]).any() and out["terminated"].max() <= 1 and out["truncated"].max() <= 1
    # the food count of the oracle stepped on the actions the rollout took, from the same start state
    orc = pc.ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(r["f64"], r["i32"])
    ref = orc.rollout(np.array(out["actions"]), want_final=True)
    orc.close()
    assert np.array_equal(out["terminated"], ref["terminated"]) and np.array_equal(out["truncated"], ref["truncated"]), "flags differ from the oracle"
    cap = ec.captures_from_info(ref["info"], ref["terminated"], ref["truncated"], start_count=r["i32"][_capi.I_FOOD_COLLECTED])
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"], cap)
    v, w = evaluation_views(np.array(rec)), evaluation_views(want)
    print(f"{name}: return_sum in [{v['return_sum'].min():.3f}, {v['return_sum'].max():.3f}], episodes {int(v['episodes'].sum())}, "
          f"food {int(v['food'].sum())}, first_end counts {np.bincount(v['first_end'], minlength=3).tolist()}")
    for k in ("first_length", "first_end", "episodes", "food"):
        assert np.array_equal(v[k], w[k]), f"{k}: {record_diff(rec, want)}"
    # the float64 sums: the bits of a sequential host loop over the float32 rewards the rollout stored
    acc = np.zeros(n, np.float64)
    for t in range(H):
        acc += out["reward"][t].astype(np.float64)
    assert np.array_equal(v["return_sum"].view(np.int64), acc.view(np.int64)), record_diff(rec, want)
    assert np.array_equal(v["return_sum"].view(np.int64), w["return_sum"].view(np.int64))
    assert np.array_equal(v["first_return"].view(np.int64), w["first_return"].view(np.int64)), record_diff(rec, want)
    assert record_diff(rec, want) == ""
    # statistics, state and global step are those of the rollout
    assert int(v["food"].sum()) == r["ev"]["stats"]["food_collected"] == int(cap.sum())
    assert int(v["episodes"].sum()) == r["ev"]["stats"]["episodes"]
    assert same_state(r["ev"]["state"], r["roll"]["state"]), "final state differs from the rollout's"
    assert r["ev"]["step"] == r["roll"]["step"] == H
    assert r["ev"]["stats"] == r["roll"]["stats"] and r["ev"]["stats"]["env_steps"] == H * n
    ec.assert_not_vacuous(name, np.array(rec))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_intended_kernel_ran(name):
    r = device_run(name)
    c, ll, twin = r["c"], r["ev"]["launch"], r["roll"]["launch"]
    print(f"{name}: {ll} {r['ev']['res']} (rollout_policy: {r['roll']['res']})")
    assert (ll["food_slots"], ll["literal_constants"]) == c["kernel"] and ll["observed_capacity"] == 3
    assert ll["full_signature"] == 4 and ll["actions_in_kernel"] == 2 and ll["forced"] == int(r["cfg"].forced_breathing)
    # the split into an unpredicated and a predicated launch is that of salp_vec_rollout_policy
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (twin["envs_unpredicated"], twin["envs_predicated"])
    if c["predicated"]:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (0, c["n"])
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (-1, 4)
    else:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (c["n"], 0)
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (4, -1)
    assert twin["full_signature"] == 1
    # no more scratch than the rollout_policy kernel of the same shape
    assert r["ev"]["res"]["scratch_bytes"] <= r["roll"]["res"]["scratch_bytes"], (r["ev"]["res"], r["roll"]["res"])


def test_split_launch_both_kernels_write_one_record_block():
    """n % 64 != 0 and n * horizon > 2^22: the call is an unpredicated launch over 4096 envs and a predicated one over the
    last 37, both of signature 4, writing disjoint ranges of ONE record block (the case table's n = 293 folds into a single
    predicated launch, as it does for salp_vec_rollout_policy).  Against `summarize_rollout` of salp_vec_rollout_policy, and
    100 steps + the rest with SALP_EVAL_ACCUMULATE, the second part still a split launch."""
    import torch
    n, HS = 4096 + 37, 1200
    assert n * (HS - CUT) > 1 << 22
    cfg, policy = cases.case_cfg("one_food_mlp32"), cases.case_policy("one_food_mlp32")
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    roll = started(cfg, n, f64, i32)
    ph = roll.policy_create(policy)
    t = dict(obs=torch.empty((HS, n, cfg.obs_dim), device="cuda:0"), reward=torch.empty((HS, n), device="cuda:0"),
             terminated=torch.empty((HS, n), dtype=torch.uint8, device="cuda:0"), truncated=torch.empty((HS, n), dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    roll.rollout_policy(ph, HS, t["obs"], t["reward"], t["terminated"], t["truncated"], None, DEV, 0)
    torch.cuda.synchronize()
    twin = roll.last_launch()
    assert (twin["envs_unpredicated"], twin["envs_predicated"]) == (4096, 37)
    reward, term, trunc = (t[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
    del t
    state, stats = device_state(roll, cfg), roll.stats()
    ph.close()
    roll.close()
    want = summarize_rollout(reward, term, trunc)

    def check(dev, rec, ll):
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (4096, 37)
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (4, 4) and ll["full_signature"] == 4 and ll["actions_in_kernel"] == 2
        v = evaluation_views(rec)
        evaluation_views(want)["food"][:] = v["food"]              # (the food count is checked against the oracle per case, above)
        assert record_diff(rec, want) == ""
        assert int(v["food"].sum()) == dev.stats()["food_collected"] and int(v["episodes"].sum()) == dev.stats()["episodes"]
        assert (v["episodes"][4096:] >= 2).all() and (v["first_end"][:4096] == 1).any()      # both halves end episodes
        assert same_state(device_state(dev, cfg), state) and dev.global_step == HS
    # one call
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    rec = fresh_record(n)
    dev.evaluate_policy(ph, HS, rec, 0)
    check(dev, rec, dev.last_launch())
    assert dev.stats() == stats
    ph.close()
    dev.close()
    # 100 steps (one predicated launch over all envs), then the rest accumulated: a split launch continuing records that
    # the other launch form began
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    rec = fresh_record(n, 0x3C)
    dev.evaluate_policy(ph, CUT, rec, 0)
    first = dev.last_launch()
    assert (first["envs_unpredicated"], first["envs_predicated"]) == (0, n) and (first["signature_unpredicated"], first["signature_predicated"]) == (-1, 4)
    dev.evaluate_policy(ph, HS - CUT, rec, ACC)
    check(dev, rec, dev.last_launch())
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_split_equals_whole_and_zeros_equal_overwriting(name):
    r = device_run(name)
    c, cfg, n = r["c"], r["cfg"], r["c"]["n"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    rec = fresh_record(n, 0x3C)
    dev.evaluate_policy(ph, CUT, rec, 0)                       # overwrites the junk
    part = rec.copy()
    dev.evaluate_policy(ph, H - CUT, rec, ACC)
    assert record_diff(rec, r["rec"]) == ""
    assert same_state(device_state(dev, cfg), r["ev"]["state"]) and dev.global_step == H
    v = evaluation_views(part)
    assert (v["first_length"] <= CUT).all() and (v["first_length"][v["first_end"] == 0] == CUT).all()
    frozen = v["first_end"] != 0                                # finished before the cut: FIRST_* stay as they were
    full = evaluation_views(np.array(r["rec"]))
    assert frozen.any() and (~frozen).any()
    for k in ("first_return", "first_length", "first_end"):
        assert np.array_equal(v[k][frozen], full[k][frozen]), k
    ph.close()
    dev.close()
    # accumulating into zeros == overwriting
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    zero = np.zeros((n, W), np.int32)
    dev.evaluate_policy(ph, H, zero, ACC)
    assert record_diff(zero, r["rec"]) == ""
    assert same_state(device_state(dev, cfg), r["ev"]["state"])
    ph.close()
    dev.close()


@pytest.mark.parametrize("case,n", [("other_tank_F1", 192), ("F3_other_tank", 100), ("other_tank_F5_free", 192), ("other_tank_F5_free", 100),
                                    ("other_physics_F12", 192), ("F16_sixteen_slots_other_tank", 192), ("F16_sixteen_slots_other_tank", 100),
                                    ("class_default_F5", 100)])
def test_other_constant_sets_and_launch_forms(case, n):
    """The summary kernels that the case table does not reach — run-time constants with 1, 8, 12 and 16 slots (they take their
    constants from another place than their rollout twins, csrc/salp_rollout_traits.h MEMC) and the predicated forms (n = 100: one
    ragged launch) — against `summarize_rollout` of salp_vec_rollout_policy from the same start state."""
    HP = 160
    cfg = pc.case_cfg(case)
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    policy = cases.random_policy(cfg.obs_dim, cfg.act_dim, (16,), "tanh", 102, 1.5, 4.0, free_breathing=not cfg.forced_breathing)
    roll = started(cfg, n, f64, i32)
    ph = roll.policy_create(policy)
    out = run_policy(roll, ph, cfg, HP)
    state, stats, twin = device_state(roll, cfg), roll.stats(), roll.last_launch()
    ph.close()
    roll.close()
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    rec = fresh_record(n)
    dev.evaluate_policy(ph, CUT, rec, 0)
    dev.evaluate_policy(ph, HP - CUT, rec, ACC)
    ll = dev.last_launch()
    assert (ll["food_slots"], ll["observed_capacity"], ll["literal_constants"]) == pc.EXPECT_KERNEL[case]
    assert ll["full_signature"] == 4 and ll["actions_in_kernel"] == 2
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (twin["envs_unpredicated"], twin["envs_predicated"]) == ((n, 0) if n % 64 == 0 else (0, n))
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"])
    v = evaluation_views(rec)
    evaluation_views(want)["food"][:] = v["food"]
    assert record_diff(rec, want) == ""
    print(f"{case} n={n}: first_end counts {np.bincount(v['first_end'], minlength=3).tolist()}, episodes {int(v['episodes'].sum())}, food {int(v['food'].sum())}")
    assert (v["first_end"] == 2).any() and (v["first_length"] > CUT).any() and int(v["food"].sum()) == dev.stats()["food_collected"]
    assert same_state(device_state(dev, cfg), state)
    # statistics: the counters exactly; reward_sum is rounded to 2^-20 once per wavefront and launch (two launches against one)
    st = dev.stats()
    assert {k: x for k, x in st.items() if k != "reward_sum"} == {k: x for k, x in stats.items() if k != "reward_sum"}
    assert abs(st["reward_sum"] - stats["reward_sum"]) <= 3 * (n // 64 + 1) * 2.0 ** -21
    ph.close()
    dev.close()


@pytest.mark.parametrize("P,group", [(4, 64), (2, 128)])
def test_population_records_are_those_of_the_rollout(P, group):
    cfg = pc.case_cfg("single_food")
    n, HP = P * group, 96
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    pop = MLPPolicy.stack(cases.separated_population(P))
    roll = started(cfg, n, f64, i32)
    ph = roll.policy_create(pop)
    out = run_policy(roll, ph, cfg, HP)
    state = device_state(roll, cfg)
    # the groups do take different actions: the records below are not those of one policy for all
    first = out["actions"][0, :, 0].reshape(P, group)
    assert all(np.abs(first[k].mean() - first[j].mean()) > 0.1 for k in range(P) for j in range(k))
    ph.close()
    roll.close()
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(pop)
    rec = fresh_record(n)
    dev.evaluate_policy(ph, HP, rec, 0)
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"])
    evaluation_views(want)["food"][:] = evaluation_views(rec)["food"]          # (no oracle here: food is checked per case above)
    assert record_diff(rec, want) == ""
    assert evaluation_views(rec)["food"].sum() == dev.stats()["food_collected"]
    assert same_state(device_state(dev, cfg), state)
    ph.close()
    dev.close()


@pytest.mark.parametrize("case", ["single_food", "sac_gail_F12"])
def test_no_autoreset_counts_every_flagged_step(case):
    n, HP = 256, 192
    spec = dict(pc.CASES[case])
    spec.setdefault("max_steps_without_food", pc.DEFAULT_BUDGET)
    orc, f64, i32 = pc.start_oracle(pc.make_cfg(spec), n, pc.ENV_SEED)
    orc.close()
    cfg = pc.make_cfg(dict(spec, no_autoreset=True))
    name = {"single_food": "one_food_mlp32", "sac_gail_F12": "sac_gail_mlp64"}[case]
    policy = cases.case_policy(name)
    roll = started(cfg, n, f64, i32)
    ph = roll.policy_create(policy)
    out = run_policy(roll, ph, cfg, HP)
    state = device_state(roll, cfg)
    ph.close()
    roll.close()
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    rec = fresh_record(n)
    dev.evaluate_policy(ph, HP, rec, 0)
    v = evaluation_views(rec)
    done = (out["terminated"] | out["truncated"]).astype(bool)
    # a finished env that is not reset stays flagged (wall contact, or the budget still exceeded): many flagged steps per env
    assert np.array_equal(v["episodes"], done.sum(0)) and v["episodes"].max() >= 10
    ever = done.any(0)
    first = np.where(ever, done.argmax(0) + 1, HP)
    assert ever.any() and np.array_equal(v["first_length"], first)
    t_first = first - 1
    idx = np.arange(n)
    assert np.array_equal(v["first_end"], np.where(ever, np.where(out["terminated"][t_first, idx] != 0, 1, 2), 0))
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"])
    evaluation_views(want)["food"][:] = v["food"]
    assert record_diff(rec, want) == ""
    assert (v["first_return"] != v["return_sum"])[ever & (first < HP)].any()       # frozen at the first flagged step, the total goes on
    assert v["food"].sum() == dev.stats()["food_collected"] and dev.stats()["episodes"] == 0      # no episode ends without autoreset
    assert same_state(device_state(dev, cfg), state)
    ph.close()
    dev.close()


def _unchanged(dev, cfg, before, step0, stats0):
    return same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0


def test_device_pointers_guard_words_and_refusals():
    import torch
    name = "one_food_mlp32_ragged"
    r = device_run(name)
    c, cfg, n = r["c"], r["cfg"], r["c"]["n"]
    sent = int(np.uint32(SENTINEL).view(np.int32))
    G = 64                                                      # guard words in front of and behind the block (256 B: alignment kept)
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    block = torch.full((G + n * W + G,), sent, dtype=torch.int32, device="cuda:0")
    rec = block[G:G + n * W]
    assert rec.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    dev.evaluate_policy(ph, H, rec, DEV, 0)
    torch.cuda.synchronize()
    host = block.cpu().numpy()
    assert (host[:G].view(np.uint32) == SENTINEL).all() and (host[G + n * W:].view(np.uint32) == SENTINEL).all(), "guard words written"
    assert record_diff(host[G:G + n * W].reshape(n, W), r["rec"]) == ""
    assert same_state(device_state(dev, cfg), r["ev"]["state"])
    # refusals: nothing launched, the handle (state, global step, statistics) and the block unchanged
    other = SalpLib(cfg, n, device_id=0, seed=1)
    other_dims = SalpLib(pc.case_cfg("free_breathing"), n, device_id=0, seed=1)
    ph_other, ph_dims = other.policy_create(r["policy"]), other_dims.policy_create(cases.case_policy("free_breathing_mlp32"))
    before, step0, stats0 = device_state(dev, cfg), dev.global_step, dev.stats()
    host_rec = np.zeros((n, W), np.int32)
    block.fill_(sent)
    torch.cuda.synchronize()
    refusals = [
        ("NULL rec (host)", dict(handle=ph, horizon=2, rec=None, flags=0)),
        ("NULL rec (device)", dict(handle=ph, horizon=2, rec=None, flags=DEV)),
        ("horizon 0", dict(handle=ph, horizon=0, rec=host_rec, flags=0)),
        ("negative horizon", dict(handle=ph, horizon=-3, rec=host_rec, flags=ACC)),
        ("the packed record's flag", dict(handle=ph, horizon=2, rec=host_rec, flags=_capi.REC_FINAL_OBS)),
        ("an unknown flag", dict(handle=ph, horizon=2, rec=host_rec, flags=8)),
        ("an unknown flag next to the known ones", dict(handle=ph, horizon=2, rec=rec, flags=DEV | ACC | 0x100)),
        ("misaligned device rec (4 B)", dict(handle=ph, horizon=2, rec=rec.data_ptr() + 4, flags=DEV)),
        ("misaligned device rec (8 B)", dict(handle=ph, horizon=2, rec=rec.data_ptr() + 8, flags=DEV | ACC)),
        ("policy of another handle", dict(handle=ph_other, horizon=2, rec=host_rec, flags=0)),
        ("policy of other dimensions", dict(handle=ph_dims, horizon=2, rec=host_rec, flags=0)),
    ]
    for label, kw in refusals:
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.evaluate_policy(**kw)
        assert _unchanged(dev, cfg, before, step0, stats0), label
    torch.cuda.synchronize()
    assert (block.cpu().numpy().view(np.uint32) == SENTINEL).all() and not host_rec.any()
    # a misaligned HOST record is fine (it is staged), and the handle still works
    raw = np.zeros(n * W + 1, np.int32)
    dev.evaluate_policy(ph, 2, raw[1:].reshape(n, W), 0)
    assert dev.global_step == step0 + 2 and (evaluation_views(raw[1:].reshape(n, W).copy())["first_length"] >= 1).all()
    for h in (ph, ph_other, ph_dims):
        h.close()
    for d in (dev, other, other_dims):
        d.close()


def test_graph_capture_accumulates_over_replays_and_takes_new_weights():
    import torch
    name = "one_food_mlp32_ragged"
    r = device_run(name)
    c, cfg, policy, n = r["c"], r["cfg"], r["policy"], r["c"]["n"]
    K = 128
    assert 3 * K == H
    policy_b = cases.random_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["out"], 999, c["gain"], c["out_gain"])
    graphed = started(cfg, n, r["f64"], r["i32"])
    ph_g = graphed.policy_create(policy)
    rec = torch.zeros((n, W), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.evaluate_policy(ph_g, K, rec, DEV | ACC, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert same_state(device_state(graphed, cfg), (r["f64"], r["i32"])), "capture must not execute"
    assert not rec.any() and graphed.global_step == K
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert record_diff(rec.cpu().numpy(), r["rec"]) == "", "three replays of 128 steps != one eager call of 384"
    assert same_state(device_state(graphed, cfg), r["ev"]["state"])
    # new weights between replays (stream-ordered, nothing re-captured): the next replay runs them
    ph_g.update(torch.tensor(policy_b.pack(), device="cuda:0"), DEV, int(torch.cuda.current_stream().cuda_stream))
    g.replay()
    torch.cuda.synchronize()
    # two eager handles go the same way with host pointers: 384 steps, then 128 more under the new / the old weights
    eager, old = started(cfg, n, r["f64"], r["i32"]), started(cfg, n, r["f64"], r["i32"])
    ph_e, ph_o = eager.policy_create(policy), old.policy_create(policy)
    want_new, want_old = np.zeros((n, W), np.int32), np.zeros((n, W), np.int32)
    eager.evaluate_policy(ph_e, H, want_new, ACC)
    old.evaluate_policy(ph_o, H, want_old, ACC)
    assert record_diff(want_new, r["rec"]) == "" and record_diff(want_old, r["rec"]) == ""
    ph_e.update(policy_b.pack())
    eager.evaluate_policy(ph_e, K, want_new, ACC)
    old.evaluate_policy(ph_o, K, want_old, ACC)
    got = rec.cpu().numpy()
    assert record_diff(got, want_new) == "", "the replay behind salp_policy_update did not run the new weights"
    assert record_diff(got, want_old) != "" and not same_state(device_state(graphed, cfg), device_state(old, cfg))
    assert same_state(device_state(graphed, cfg), device_state(eager, cfg))
    assert graphed.stats()["env_steps"] == 4 * K * n
    for h in (ph_g, ph_e, ph_o):
        h.close()
    for d in (graphed, eager, old):
        d.close()


def test_vector_env_surface():
    import torch
    from underwater_swimmer_rl_amd import SalpVectorEnv, pursuit_policy
    from underwater_swimmer_rl_amd import evaluation_views as exported
    assert exported is evaluation_views
    env = SalpVectorEnv("single_food", num_envs=256, seed=3)
    env.reset()
    f64, i32 = env.get_state()
    f64, i32 = f64.copy(), i32.copy()
    p = pursuit_policy(3.0)
    out = env.rollout_policy(p, 48)
    reward, term, trunc = (out[k].cpu().numpy() for k in ("reward", "terminated", "truncated"))
    env.set_state(f64, i32)
    ev = env.evaluate_policy(p, 48)
    assert set(ev) == {"record", "return_sum", "first_return", "first_length", "first_end", "episodes", "food"}
    assert ev["record"].dtype == torch.int32 and tuple(ev["record"].shape) == (256, 8) and ev["record"].is_cuda
    for k in ("return_sum", "first_return"):
        assert ev[k].dtype == torch.float64 and tuple(ev[k].shape) == (256,)
    for k in ("first_length", "first_end", "episodes", "food"):
        assert ev[k].dtype == torch.int32 and tuple(ev[k].shape) == (256,)
    want = evaluation_views(summarize_rollout(reward, term, trunc))
    assert np.array_equal(ev["return_sum"].cpu().numpy().view(np.int64), want["return_sum"].view(np.int64))
    assert np.array_equal(ev["first_length"].cpu().numpy(), want["first_length"])
    assert env.global_step == 96 and env._lib.last_launch()["full_signature"] == 4
    # out= reuses the block (the tensor itself or the dict returned earlier); accumulate continues it
    kept = ev["record"].clone()
    again = env.evaluate_policy(p, 16, out=ev["record"], accumulate=True)
    assert again["record"].data_ptr() == ev["record"].data_ptr()
    assert (again["first_length"] >= torch.as_tensor(want["first_length"], device=again["record"].device)).all()
    assert (again["return_sum"] != evaluation_views(kept)["return_sum"]).any() and (again["episodes"] >= evaluation_views(kept)["episodes"]).all()
    third = env.evaluate_policy(p, 16, out=again)
    assert third["record"].data_ptr() == ev["record"].data_ptr() and (third["first_length"] <= 16).all()
    with pytest.raises(ValueError):
        env.evaluate_policy(p, 16, accumulate=True)
    with pytest.raises(ValueError):
        env.evaluate_policy(p, 0)
    with pytest.raises(ValueError):
        env.evaluate_policy(p, 4, out=torch.zeros((256, 8), dtype=torch.float32, device=ev["record"].device))
    with pytest.raises(ValueError):
        env.evaluate_policy(p, 4, out=torch.zeros((128, 8), dtype=torch.int32, device=ev["record"].device))
    with pytest.raises(ValueError):         # a block that is not on the env's device is refused, not handed to the kernel
        env.evaluate_policy(p, 4, out=torch.zeros((256, 8), dtype=torch.int32))
    with pytest.raises(ValueError):
        env.evaluate_policy(p, 4, out=np.zeros((256, 8), np.int32))
    host = SalpVectorEnv("single_food", num_envs=128, seed=3, output="numpy")
    host.reset()
    hv = host.evaluate_policy(p, 8)
    assert isinstance(hv["record"], np.ndarray) and hv["return_sum"].dtype == np.float64 and (hv["first_length"] >= 1).all()
    with pytest.raises(ValueError):         # and a host env takes numpy blocks only
        host.evaluate_policy(p, 4, out=torch.zeros((128, 8), dtype=torch.int32, device=ev["record"].device))
    assert host.global_step == 8
    host.close()
    assert env.global_step == 96 + 32
    env.close()
