"""Sampled closed-loop rollouts (salp_vec_rollout_policy_sampled / salp_vec_evaluate_policy_sampled) on the GPU, over the case
table of tests/sampled_cases.py (configurations and injected start state of tests/parity_cases.py).  Run with `pytest -m gpu`.

Per case: every action and log-probability against `GaussianPolicy.reference` of the row it saw and the noise of its step,
within `GaussianPolicy.error_bound`; a wrong noise step far outside it; the simulator against a twin handle running
salp_vec_rollout on the actions taken (bit for bit, draw counters included); H calls of horizon 1 against one call.  Then the
noise step and reseed, the mean path of the deterministic entry points, the clamps, the summary records, hipGraph capture,
populations, guard words and NULL outputs, refusals, the kernel that ran, and sac.collect_in_kernel."""
import ctypes
import functools

import numpy as np
import pytest

import evaluate_cases as ec
import parity_cases as pc
import policy_cases as dc
import sampled_cases as cases
from gpu_support import device_state, host_outputs, run_policy, run_sampled, started
from support import bits, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpError, SalpLib
from underwater_swimmer_rl_amd.policy import EVAL_WORDS, GaussianPolicy, evaluation_views, summarize_rollout

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
DEV, ACC = _capi.SALP_DEVICE_PTRS, _capi.EVAL_ACCUMULATE
H = cases.H


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One sampled closed-loop rollout of a case on the GPU from noise step 0: computed once, shared, read-only."""
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    dev = started(cfg, c["n"], f64, i32)
    obs0 = np.empty((c["n"], cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(policy)
    assert ph.gaussian and dev.policy_words(policy) == policy.words == ph.words
    assert ph.noise_step == 0 and dev.global_step == 0
    out = run_sampled(dev, ph, cfg, H)
    launch, res = dev.last_launch(), dev.last_kernel_resources()
    assert dev.global_step == H and ph.noise_step == H
    state, stats = device_state(dev, cfg), dev.stats()
    ph.close()
    dev.close()
    seen = np.concatenate([obs0[None], out["obs"][:-1]])        # act[0] <- observe(); act[t + 1] <- obs[t]
    for a in (seen, *out.values(), *state):
        a.setflags(write=False)
    return dict(c=c, cfg=cfg, policy=policy, f64=f64, i32=i32, seen=seen, out=out, launch=launch, res=res, state=state, stats=stats)


def assert_is_the_definition(policy, seen, out, n0, key=cases.KEY, label=""):
    """Every action and log-probability of `out` within the bounds of the definition on the rows seen and noise steps n0 + t."""
    z = cases.case_noise(policy, seen.shape[1], n0, seen.shape[0], key)
    (wa, wl), (ea, el) = policy.reference(seen, z), policy.error_bound(seen, z)
    da, dl = np.abs(out["actions"].astype(np.float64) - wa), np.abs(out["logp"].astype(np.float64) - wl)
    print(f"{label}: largest |action - reference| / bound = {(da / ea).max():.4f} (bound max {ea.max():.3g}); "
          f"|logp - reference| / bound = {(dl / el).max():.4f} (bound max {el.max():.3g})")
    assert (da <= ea).all(), f"{label}: {int((da > ea).sum())} actions outside the bound, worst ratio {(da / ea).max()} at {np.unravel_index((da / ea).argmax(), da.shape)}"
    assert (dl <= el).all(), f"{label}: {int((dl > el).sum())} logp outside the bound, worst ratio {(dl / el).max()} at {np.unravel_index((dl / el).argmax(), dl.shape)}"
    return ea, el


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_intended_kernel_ran(name):
    r = device_run(name)
    c, ll = r["c"], r["launch"]
    print(f"{name}: {ll} {r['res']}")
    assert (ll["food_slots"], ll["literal_constants"]) == c["kernel"] and ll["observed_capacity"] == 3
    assert ll["actions_in_kernel"] == 3 and ll["full_signature"] == 1 and ll["forced"] == int(r["cfg"].forced_breathing)
    if c["predicated"]:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (0, c["n"])
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (-1, 1)
    else:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (c["n"], 0)
    if c["kernel"][0] in (1, 12):       # no spill to memory in the one-food and 12-slot sampled kernels, as in their twins
        assert r["res"]["scratch_bytes"] == 0, r["res"]
    # the deterministic twin: the same case through salp_vec_rollout_policy differs in [5] alone
    dev = started(r["cfg"], c["n"], r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    run_policy(dev, ph, r["cfg"], 2)
    twin = dev.last_launch()
    assert twin["actions_in_kernel"] == 2 and {k: v for k, v in twin.items() if k != "actions_in_kernel"} == \
        {k: v for k, v in ll.items() if k != "actions_in_kernel"}
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_sampled_action_and_logp_is_the_definition(name):
    r = device_run(name)
    out = r["out"]
    assert not np.isnan(out["actions"]).any() and not np.isnan(out["logp"]).any() and not np.isnan(out["obs"]).any()
    ea, el = assert_is_the_definition(r["policy"], r["seen"], out, 0, label=name)
    assert ea.max() < cases.BOUND_CEILING and el.max() < r["cfg"].act_dim * cases.LOGP_BOUND_CEILING_PER_COMPONENT


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_noise_step_was_applied(name):
    """Under the noise of the wrong step (off by one) the actions taken are far outside the bound."""
    r = device_run(name)
    share = cases.off_by_one_share(r["policy"], r["seen"], r["out"]["actions"])
    # every entry counts, except in the one case whose nozzle log-std sits at the lower clamp (sd = e^-20: no noise to see)
    left_out = list(cases.floor_clamped_components(r["policy"]))
    assert left_out == ([1] if name == "free_breathing_mlp32_clamped" else [])
    print(f"{name}: {share:.3f} of the actions are more than {cases.OFF_BY_ONE_BOUNDS:.0f} bounds from the definition under n + 1")
    assert share > cases.OFF_BY_ONE_SHARE


@pytest.mark.parametrize("name", list(cases.CASES))
def test_simulator_untouched(name):
    """A twin handle running salp_vec_rollout on the actions taken: the same bits everywhere, and the same draw counters —
    sampling consumed no env draw."""
    r = device_run(name)
    c, cfg, out, n = r["c"], r["cfg"], r["out"], r["c"]["n"]
    twin = started(cfg, n, r["f64"], r["i32"])
    t = host_outputs(cfg, H, n)
    twin.rollout(np.array(out["actions"]), H, t["obs"], t["reward"], t["terminated"], t["truncated"], None, None, 0)
    assert twin.last_launch()["actions_in_kernel"] == 0
    for k in ("obs", "reward"):
        assert np.array_equal(bits(out[k]), bits(t[k])), f"{k} bits differ from salp_vec_rollout on the same actions"
    assert np.array_equal(out["terminated"], t["terminated"]) and np.array_equal(out["truncated"], t["truncated"])
    tw_state = device_state(twin, cfg)
    assert np.array_equal(r["state"][1][_capi.I_RNG_COUNTER], tw_state[1][_capi.I_RNG_COUNTER]), "sampling consumed env draws"
    assert same_state(r["state"], tw_state), "final state differs from the twin's"
    assert twin.global_step == H and twin.stats() == r["stats"] and r["stats"]["env_steps"] == H * n
    twin.close()
    # the events the deterministic cases demand, on the oracle stepped on these actions
    orc = pc.ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(r["f64"], r["i32"])
    ref = orc.rollout(np.array(out["actions"]), want_final=True)
    orc.close()
    assert np.array_equal(out["terminated"], ref["terminated"]) and np.array_equal(out["truncated"], ref["truncated"]), "flags differ from the oracle"
    ev = pc.count_events(ref)
    print(f"{name}: {ev}")
    cases.assert_closed_loop_events(name, ev)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_split_equals_whole(name):
    """H calls of horizon 1 == one call of H, bit for bit, in actions, logp, obs and reward; the noise step reads H after both."""
    r = device_run(name)
    c, cfg, out = r["c"], r["cfg"], r["out"]
    dev = started(cfg, c["n"], r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    got = host_outputs(cfg, H, c["n"], logp=True)
    for t in range(H):
        dev.rollout_policy_sampled(ph, 1, got["obs"][t:t + 1], got["reward"][t:t + 1], got["terminated"][t:t + 1],
                                   got["truncated"][t:t + 1], got["actions"][t:t + 1], got["logp"][t:t + 1], 0)
    assert ph.noise_step == H and dev.global_step == H
    for k in ("actions", "logp", "obs", "reward"):
        same = bits(got[k]) == bits(out[k])
        assert same.all(), f"{k}: first difference at {np.unravel_index(np.argmin(same), same.shape)} of {int((~same).sum())}"
    assert np.array_equal(got["terminated"], out["terminated"]) and np.array_equal(got["truncated"], out["truncated"])
    assert same_state(device_state(dev, cfg), r["state"])
    ph.close()
    dev.close()


def test_set_noise_step_continues_a_run_and_reseed_rekeys_the_stream():
    name, cut = "one_food_mlp32", 100
    r = device_run(name)
    c, cfg, out, n = r["c"], r["cfg"], r["out"], r["c"]["n"]
    # the first `cut` steps replayed by salp_vec_rollout (a state that a step left), then the tail under noise steps cut ..
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    t = host_outputs(cfg, cut, n)
    dev.rollout(np.array(out["actions"][:cut]), cut, t["obs"], t["reward"], t["terminated"], t["truncated"], None, None, 0)
    assert ph.noise_step == 0
    ph.set_noise_step(cut)
    assert ph.noise_step == cut
    tail = run_sampled(dev, ph, cfg, H - cut)
    assert ph.noise_step == H
    for k in ("actions", "logp", "obs", "reward"):
        assert np.array_equal(bits(tail[k]), bits(out[k][cut:])), f"{k}: the tail differs from the run started at 0"
    assert same_state(device_state(dev, cfg), r["state"])
    # a 64-bit step: the kernels take its low word, the object keeps all of it
    ph.set_noise_step((7 << 32) + 5)
    assert ph.noise_step == (7 << 32) + 5
    # reseed: another key, the step left alone
    other_seed, K = 12, 32
    obs0 = np.empty((n, cfg.obs_dim), np.float32)
    dev.reseed(other_seed, obs0, 0)
    assert ph.noise_step == (7 << 32) + 5
    ph.set_noise_step(0)
    o = run_sampled(dev, ph, cfg, K)
    seen = np.concatenate([obs0[None], o["obs"][:-1]])
    assert_is_the_definition(r["policy"], seen, o, 0, key=other_seed, label="after reseed, the new key")
    z_old = cases.case_noise(r["policy"], n, 0, K, pc.ENV_SEED)
    wa, _ = r["policy"].reference(seen, z_old)
    ea, _ = r["policy"].error_bound(seen, z_old)
    assert (np.abs(o["actions"] - wa) > 100.0 * ea).mean() > 0.5, "the old key's noise still fits"
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", ["one_food_mlp32", "sac_gail_mlp64"])
def test_the_deterministic_entry_points_run_the_mean(name):
    """A Gaussian policy through salp_vec_rollout_policy / salp_vec_evaluate_policy == its mean_policy(), bit for bit."""
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    n, HM = c["n"], 128
    runs = []
    for p in (policy, policy.mean_policy()):
        dev = started(cfg, n, f64, i32)
        ph = dev.policy_create(p)
        assert ph.gaussian == isinstance(p, GaussianPolicy)
        o = run_policy(dev, ph, cfg, HM)
        ll = dev.last_launch()
        rec = np.zeros((n, EVAL_WORDS), np.int32)
        dev.evaluate_policy(ph, HM, rec, 0)
        assert ll["actions_in_kernel"] == 2 and dev.last_launch()["actions_in_kernel"] == 2
        if ph.gaussian:
            assert ph.noise_step == 0            # the mean path draws nothing
        runs.append((o, rec, device_state(dev, cfg), dev.stats()))
        ph.close()
        dev.close()
    (a, ra, sa, ta), (b, rb, sb, tb) = runs
    for k in ("actions", "obs", "reward"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["terminated"], b["terminated"]) and np.array_equal(a["truncated"], b["truncated"])
    assert np.array_equal(ra, rb) and same_state(sa, sb) and ta == tb
    assert (a["terminated"] | a["truncated"]).any()


def test_log_std_clamps():
    """W_ls = 0: b_ls = -50 gives the bits of b_ls = -20, b_ls = +7 those of b_ls = +2."""
    name, HC = "one_food_mlp32", 48
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    n = c["n"]

    def run(b):
        W = np.zeros_like(policy.log_std[0])
        p = GaussianPolicy(policy.layers, (W, np.full_like(policy.log_std[1], b)), policy.scale, policy.shift)
        dev = started(cfg, n, f64, i32)
        ph = dev.policy_create(p)
        o = run_sampled(dev, ph, cfg, HC)
        ph.close()
        dev.close()
        return o
    for beyond, at in ((-50.0, -20.0), (7.0, 2.0)):
        x, y = run(beyond), run(at)
        for k in ("actions", "logp", "obs", "reward"):
            assert np.array_equal(bits(x[k]), bits(y[k])), (beyond, k)
    inside = run(1.0)
    assert not np.array_equal(bits(inside["actions"]), bits(y["actions"]))      # (the clamp is what made them equal)


def _captures(cfg, n, f64, i32, out):
    orc = pc.ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(f64, i32)
    ref = orc.rollout(np.array(out["actions"]), want_final=True)
    orc.close()
    assert np.array_equal(out["terminated"], ref["terminated"]) and np.array_equal(out["truncated"], ref["truncated"])
    return ec.captures_from_info(ref["info"], ref["terminated"], ref["truncated"], start_count=i32[_capi.I_FOOD_COLLECTED])


@pytest.mark.parametrize("name", ["one_food_mlp32_ragged", "sac_gail_mlp64", "free_breathing_mlp32_clamped"])
def test_evaluate_policy_sampled_is_the_summary_of_the_sampled_rollout(name):
    r = device_run(name)
    c, cfg, out, n = r["c"], r["cfg"], r["out"], r["c"]["n"]
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"], _captures(cfg, n, r["f64"], r["i32"], out))
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    rec = np.full((n, EVAL_WORDS), -1, np.int32)
    dev.evaluate_policy_sampled(ph, H, rec, 0)
    ll = dev.last_launch()
    assert ll["actions_in_kernel"] == 3 and ll["full_signature"] == 4 and ph.noise_step == H and dev.global_step == H
    assert np.array_equal(rec, want), f"{int((rec != want).any(axis=1).sum())} records differ"
    assert same_state(device_state(dev, cfg), r["state"]) and dev.stats() == r["stats"]
    v = evaluation_views(rec)
    print(f"{name}: first_end counts {np.bincount(v['first_end'], minlength=3).tolist()}, episodes {int(v['episodes'].sum())}, food {int(v['food'].sum())}")
    assert (v["first_end"] == 1).any() and (v["first_end"] == 2).any() and (v["episodes"] >= 2).any()
    ph.close()
    dev.close()
    # two halves with SALP_EVAL_ACCUMULATE == the whole
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    acc = np.zeros((n, EVAL_WORDS), np.int32)
    dev.evaluate_policy_sampled(ph, ec.CUT, acc, ACC)
    assert ph.noise_step == ec.CUT
    dev.evaluate_policy_sampled(ph, H - ec.CUT, acc, ACC)
    assert np.array_equal(acc, want) and ph.noise_step == H
    ph.close()
    dev.close()


def test_graph_capture_draws_fresh_noise_and_takes_new_weights():
    import torch
    name = "one_food_mlp32"
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    n, K = c["n"], 16
    policy_b = cases.gaussian_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], 999, c["gain"], c["out_gain"], c["b_ls"])
    assert policy_b.words == policy.words
    eager, graphed = started(cfg, n, f64, i32), started(cfg, n, f64, i32)
    ph_e, ph_g = eager.policy_create(policy), graphed.policy_create(policy)
    w_b = torch.tensor(policy_b.pack(), device="cuda:0")

    def blocks():
        return dict(obs=torch.zeros(K, n, cfg.obs_dim, device="cuda:0"), reward=torch.zeros(K, n, device="cuda:0"),
                    terminated=torch.zeros(K, n, dtype=torch.uint8, device="cuda:0"),
                    truncated=torch.zeros(K, n, dtype=torch.uint8, device="cuda:0"),
                    actions=torch.zeros(K, n, cfg.act_dim, device="cuda:0"), logp=torch.zeros(K, n, device="cuda:0"))
    bg, be = blocks(), blocks()

    def call(dev, ph, b, stream):
        dev.rollout_policy_sampled(ph, K, b["obs"], b["reward"], b["terminated"], b["truncated"], b["actions"], b["logp"], DEV, stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(graphed, ph_g, bg, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert same_state(device_state(graphed, cfg), (f64, i32)) and ph_g.noise_step == 0, "capture must not execute"
    taken = []
    for rep in range(3):
        if rep == 2:        # new weights between two replays: stream-ordered, nothing allocated, no re-capture
            ph_g.update(w_b, DEV, int(torch.cuda.current_stream().cuda_stream))
            ph_e.update(policy_b.pack())
        seen0 = np.empty((n, cfg.obs_dim), np.float32)
        eager.observe(seen0, 0)
        g.replay()
        call(eager, ph_e, be, 0)
        torch.cuda.synchronize()
        for k in bg:
            assert torch.equal(bg[k], be[k]), (rep, k)
        assert ph_g.noise_step == ph_e.noise_step == (rep + 1) * K       # advanced on the device, by the replay itself
        pol = policy if rep < 2 else policy_b
        seen = np.concatenate([seen0[None], be["obs"][:-1].cpu().numpy()])
        o = dict(actions=be["actions"].cpu().numpy(), logp=be["logp"].cpu().numpy())
        assert_is_the_definition(pol, seen, o, rep * K, label=f"replay {rep}")
        if rep == 2:        # and they are NOT the old policy's
            z = cases.case_noise(policy, n, rep * K, K)
            assert (np.abs(o["actions"] - policy.reference(seen, z)[0]) > 100 * policy.error_bound(seen, z)[0]).mean() > 0.5
        taken.append(o["actions"])
    assert not np.array_equal(taken[0], taken[1])
    assert same_state(device_state(graphed, cfg), device_state(eager, cfg)) and graphed.stats() == eager.stats()
    for h in (ph_e, ph_g):
        h.close()
    eager.close()
    graphed.close()


def test_population_each_group_samples_its_own_policy():
    cfg = pc.case_cfg("single_food")
    P, group, HP = 4, 64, 96
    n = P * group
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    ps = []
    for k in range(P):      # mean biases and log-std biases far apart
        p = cases.gaussian_policy(24, 1, (16,), 200 + k, 0.5, 0.1, (-3.0 + k,))
        (W0, b0), (W1, b1) = p.layers
        ps.append(GaussianPolicy([(W0, b0), (W1, np.full_like(b1, -0.9 + 1.8 * k / (P - 1)))], p.log_std, p.scale, p.shift))
    pop = GaussianPolicy.stack(ps)
    dev = started(cfg, n, f64, i32)
    obs0 = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(pop)
    out = run_sampled(dev, ph, cfg, HP)
    seen = np.concatenate([obs0[None], out["obs"][:-1]])
    z = cases.case_noise(pop, n, 0, HP)
    for k, p in enumerate(ps):      # its own policy on its own envs' noise (the env index is global, not per group)
        sl = slice(k * group, (k + 1) * group)
        (wa, wl), (ea, el) = p.reference(seen[:, sl], z[:, sl]), p.error_bound(seen[:, sl], z[:, sl])
        assert (np.abs(out["actions"][:, sl] - wa) <= ea).all() and (np.abs(out["logp"][:, sl] - wl) <= el).all(), k
        for j, q in enumerate(ps):
            if j != k:          # another policy's logp is far away (log_std differs by at least 1; the squash term may cancel it here and there)
                assert (np.abs(out["logp"][:, sl] - q.reference(seen[:, sl], z[:, sl])[1]) > 100.0 * el).mean() > 0.9, (k, j)
    assert_is_the_definition(pop, seen, out, 0, label=f"P = {P} x {group}")
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", ["one_food_mlp32_ragged", "free_breathing_mlp32_clamped"])
def test_device_pointers_guard_words_and_null_outputs(name):
    import torch
    r = device_run(name)
    c, cfg, out, n, HG = r["c"], r["cfg"], r["out"], r["c"]["n"], 48
    sent = int(np.uint32(SENTINEL).view(np.int32))

    def block(shape, dtype):
        rows = int(np.prod(shape))
        b = torch.empty(rows + 64, dtype=dtype, device="cuda:0")
        if dtype == torch.uint8:
            b.fill_(0xA5)
        else:
            b.view(torch.int32).fill_(sent)
        return b, rows
    for with_actions, with_logp in ((True, True), (False, True), (True, False), (False, False)):
        dev = started(cfg, n, r["f64"], r["i32"])
        ph = dev.policy_create(r["policy"])
        bl = dict(obs=block((HG, n, cfg.obs_dim), torch.float32), reward=block((HG, n), torch.float32),
                  terminated=block((HG, n), torch.uint8), truncated=block((HG, n), torch.uint8),
                  actions=block((HG, n, cfg.act_dim), torch.float32), logp=block((HG, n), torch.float32))
        torch.cuda.synchronize()
        dev.rollout_policy_sampled(ph, HG, bl["obs"][0], bl["reward"][0], bl["terminated"][0], bl["truncated"][0],
                                   bl["actions"][0] if with_actions else None, bl["logp"][0] if with_logp else None, DEV, 0)
        torch.cuda.synchronize()
        assert ph.noise_step == HG
        for k, (b, rows) in bl.items():
            host = b.cpu().numpy()
            guard = host[rows:]
            assert (guard == 0xA5).all() if host.dtype == np.uint8 else (guard.view(np.uint32) == SENTINEL).all(), f"{k}: guard words written"
            if (k == "actions" and not with_actions) or (k == "logp" and not with_logp):
                assert (host.view(np.uint32) == SENTINEL).all(), f"{k} == NULL, yet the block was written"
                continue
            want = out[k][:HG].reshape(-1)
            assert np.array_equal(host[:rows].view(np.uint32) if host.dtype != np.uint8 else host[:rows],
                                  bits(want) if want.dtype != np.uint8 else want), f"{k} differs from the host-pointer run"
        ph.close()
        dev.close()


def test_refusals_leave_the_handle_and_the_noise_step_unchanged():
    cfg, free = pc.case_cfg("single_food"), pc.case_cfg("free_breathing")
    n = 256
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    dev, other, other_dims = started(cfg, n, f64, i32), SalpLib(cfg, n, device_id=0, seed=1), SalpLib(free, n, device_id=0, seed=1)
    p = cases.case_policy("one_food_mlp32")
    ph, ph_other = dev.policy_create(p), other.policy_create(p)
    ph_plain = dev.policy_create(p.mean_policy())
    ph_dims = other_dims.policy_create(cases.case_policy("free_breathing_mlp32_clamped"))
    ph.set_noise_step(41)
    before, step0, stats0 = device_state(dev, cfg), dev.global_step, dev.stats()
    o = host_outputs(cfg, 2, n, logp=True)
    base = dict(handle=ph, horizon=2, obs=o["obs"], reward=o["reward"], term=o["terminated"], trunc=o["truncated"],
                act_out=o["actions"], logp_out=o["logp"], flags=0)
    refused = [("a plain policy", dict(handle=ph_plain)), ("policy of another handle", dict(handle=ph_other)),
               ("policy of other dimensions", dict(handle=ph_dims)), ("horizon 0", dict(horizon=0)), ("negative horizon", dict(horizon=-3))]
    refused += [(f"NULL {k}", {k: None}) for k in ("obs", "reward", "term", "trunc")]
    rec = np.zeros((n, EVAL_WORDS), np.int32)
    for label, kw in refused:
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.rollout_policy_sampled(**{**base, **kw})
        assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0, label
        assert ph.noise_step == 41, label
    # salp_vec_evaluate_policy_sampled: the deterministic twin's list (tests/test_gpu_policy_evaluate.py) and the plain policy;
    # a device block between guard words stays untouched, misaligned device records included
    import torch
    sent = int(np.uint32(SENTINEL).view(np.int32))
    G = 64
    block = torch.full((G + n * EVAL_WORDS + G,), sent, dtype=torch.int32, device="cuda:0")
    drec = block[G:G + n * EVAL_WORDS]
    assert drec.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ev_refused = [
        ("a plain policy", dict(handle=ph_plain, horizon=2, rec=rec, flags=0)),
        ("a plain policy (device)", dict(handle=ph_plain, horizon=2, rec=drec, flags=DEV)),
        ("NULL rec (host)", dict(handle=ph, horizon=2, rec=None, flags=0)),
        ("NULL rec (device)", dict(handle=ph, horizon=2, rec=None, flags=DEV)),
        ("horizon 0", dict(handle=ph, horizon=0, rec=rec, flags=0)),
        ("negative horizon", dict(handle=ph, horizon=-3, rec=rec, flags=ACC)),
        ("the packed record's flag", dict(handle=ph, horizon=2, rec=rec, flags=_capi.REC_FINAL_OBS)),
        ("an unknown flag", dict(handle=ph, horizon=2, rec=rec, flags=8)),
        ("an unknown flag next to the known ones", dict(handle=ph, horizon=2, rec=drec, flags=DEV | ACC | 0x100)),
        ("misaligned device rec (4 B)", dict(handle=ph, horizon=2, rec=drec.data_ptr() + 4, flags=DEV)),
        ("misaligned device rec (8 B)", dict(handle=ph, horizon=2, rec=drec.data_ptr() + 8, flags=DEV | ACC)),
        ("policy of another handle", dict(handle=ph_other, horizon=2, rec=rec, flags=0)),
        ("policy of other dimensions", dict(handle=ph_dims, horizon=2, rec=rec, flags=0)),
    ]
    for label, kw in ev_refused:
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.evaluate_policy_sampled(**kw)
        assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0, label
        assert ph.noise_step == 41 and not rec.any(), label
    torch.cuda.synchronize()
    assert (block.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to the device block"
    with pytest.raises(SalpError, match=r"\(-1\)"):      # a plain policy has no noise step
        ph_plain.noise_step
    with pytest.raises(SalpError, match=r"\(-1\)"):
        ph_plain.set_noise_step(3)
    # descriptors: a Gaussian policy squashes with tanh; the shape limits are those of salp_policy_create
    lib = dev.lib

    def desc(n_hidden=2, hidden=(32, 32), out=0, P=1):
        from underwater_swimmer_rl_amd.policy import CPolicyDesc
        d = CPolicyDesc()
        d.struct_size = ctypes.sizeof(CPolicyDesc)
        d.n_hidden, d.out_activation, d.n_policies = n_hidden, out, P
        d.hidden[0], d.hidden[1] = hidden
        return d
    assert lib.salp_policy_words_gaussian(dev._h, ctypes.byref(desc())) == p.words == p.mean_policy().words + 32 + 1
    w = np.zeros(4 * 4096, np.float32)
    for d in [desc(out=1), desc(out=2), desc(n_hidden=3), desc(hidden=(32, 24)), desc(hidden=(80, 32)), desc(P=0), desc(P=3)]:
        h = ctypes.c_void_p()
        assert lib.salp_policy_words_gaussian(dev._h, ctypes.byref(d)) == -1
        assert lib.salp_policy_create_gaussian(dev._h, ctypes.byref(d), w.ctypes.data_as(ctypes.c_void_p), 0, None, ctypes.byref(h)) == -1
        assert not h.value
    k2 = SalpLib(pc.case_cfg("K2_generic"), 64, device_id=0, seed=1)
    with pytest.raises(SalpError):
        k2.policy_create(cases.gaussian_policy(k2.obs_dim, 1, (16,), 0, 1, 1, (-1.0,)))
    assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0 and ph.noise_step == 41
    # the handle still works
    out = run_sampled(dev, ph, cfg, 2)
    assert not np.isnan(out["logp"]).any() and dev.global_step == step0 + 2 and ph.noise_step == 43
    for h in (ph, ph_other, ph_plain, ph_dims):
        h.close()
    for d in (dev, other, other_dims, k2):
        d.close()


def test_vector_env_surface_and_collect_in_kernel():
    import torch
    from underwater_swimmer_rl_amd import GaussianPolicy as Exported, SalpVectorEnv
    from underwater_swimmer_rl_amd import sac
    assert Exported is GaussianPolicy
    n, HC = 256, 32
    cfg_sac = sac.SACConfig(hidden_sizes=(32, 32))
    torch.manual_seed(0)
    agent = sac.SAC(24, 1, cfg_sac, device="cuda:0")
    with torch.no_grad():           # a lively mean head, a quiet log-std head
        agent.actor.mu.weight.mul_(4.0)
        agent.actor.log_std.bias.fill_(-1.0)
    pol = GaussianPolicy.from_actor(agent.actor)

    def fresh():
        env = SalpVectorEnv("single_food", num_envs=n, seed=5, max_steps_without_food=20)
        env.reset()
        return env
    # the rollout that collect_in_kernel must have made: a twin env, the same seed and noise step
    twin = fresh()
    first = twin.observe().clone()
    handle_t = twin.make_policy(pol)
    out = twin.rollout_policy(handle_t, HC, sample=True)
    assert set(out) == {"obs", "reward", "terminated", "truncated", "final_obs", "actions", "logp"} and out["logp"].shape == (HC, n)
    seen = torch.cat([first[None], out["obs"][:-1]])
    z = cases.case_noise(pol, n, 0, HC, key=5)
    o = dict(actions=out["actions"].cpu().numpy(), logp=out["logp"].cpu().numpy())
    assert_is_the_definition(pol, seen.cpu().numpy(), o, 0, key=5, label="vector env")
    assert handle_t.noise_step == HC
    # sample=False: the mean, the noise step untouched; evaluate_policy(sample=True) draws
    mean = twin.rollout_policy(handle_t, 4, sample=False)
    assert "logp" not in mean and handle_t.noise_step == HC
    ev = twin.evaluate_policy(handle_t, 8, sample=True)
    assert handle_t.noise_step == HC + 8 and int(ev["first_length"].max()) <= 8
    # collect_in_kernel
    env = fresh()
    buf = sac.DeviceReplayBuffer(HC * n, 24, 1, torch.device("cuda:0"))
    handle = sac.collect_in_kernel(env, agent, buf, HC)
    keep = (out["truncated"] == 0).reshape(-1)
    n_trunc = int((out["truncated"] != 0).sum())
    assert n_trunc >= 1 and int(out["terminated"].sum()) >= 0 and buf.size == HC * n - n_trunc
    flat = lambda t: t.reshape((HC * n,) + tuple(t.shape[2:]))[keep]
    k = buf.size
    assert torch.equal(buf.obs[:k], flat(seen)) and torch.equal(buf.next_obs[:k], flat(out["obs"]))
    assert torch.equal(buf.act[:k], flat(out["actions"])) and torch.equal(buf.rew[:k], flat(out["reward"]))
    assert torch.equal(buf.term[:k], flat(out["terminated"]).float())
    # the handle comes back for reuse: the next call uploads the actor's weights and continues the noise
    assert handle.noise_step == HC
    again = sac.collect_in_kernel(env, agent, buf, 4, handle=handle)
    assert again is handle and handle.noise_step == HC + 4 and env.global_step == HC + 4
    with pytest.raises(ValueError, match="64"):
        sac.collect_in_kernel(env, sac.SAC(24, 1, sac.SACConfig(hidden_sizes=(256, 256)), device="cuda:0"), buf, 4)
    env.close()
    twin.close()
