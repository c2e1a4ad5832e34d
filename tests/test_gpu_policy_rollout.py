"""Closed-loop rollouts with the policy evaluated inside the kernel (salp_vec_rollout_policy) on the GPU, over the case
table of tests/policy_cases.py (configurations and injected start state of tests/parity_cases.py).  Run with `pytest -m gpu`.

Per case: the simulator against the CPU oracle fed with the actions the kernel took (the project's tolerances) and against a
twin handle running salp_vec_rollout on those actions (bit for bit); every action against `MLPPolicy.reference` of the row
it saw, within `MLPPolicy.error_bound`; H calls of horizon 1 against one call of horizon H (bit for bit).  Then populations,
hipGraph capture with a weight update between replays, refusals, a NULL act_out and guard words behind every output."""
import ctypes
import functools

import numpy as np
import pytest

import parity_cases as pc
import policy_cases as cases
from gpu_support import OBS_TOL, REW_TOL, STATE_TOL, device_state, host_outputs, run_policy, started
from support import bits, obs_diff, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpError, SalpLib
from underwater_swimmer_rl_amd.policy import MLPPolicy

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
DEV = _capi.SALP_DEVICE_PTRS
H = cases.H


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One closed-loop rollout of a case on the GPU: computed once, shared by the tests below, read-only."""
    c, cfg, policy, f64, i32 = cases.start_snapshot(name)
    dev = started(cfg, c["n"], f64, i32)
    obs0 = np.empty((c["n"], cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(policy)
    assert dev.policy_words(policy) == policy.words == ph.words
    step0 = dev.global_step
    out = run_policy(dev, ph, cfg, H)
    launch, res = dev.last_launch(), dev.last_kernel_resources()
    assert dev.global_step == step0 + H
    state, stats = device_state(dev, cfg), dev.stats()
    ph.close()
    dev.close()
    for a in (obs0, *out.values(), *state):
        a.setflags(write=False)
    return dict(c=c, cfg=cfg, policy=policy, f64=f64, i32=i32, obs0=obs0, out=out, launch=launch, res=res, state=state, stats=stats)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_intended_kernel_ran(name):
    r = device_run(name)
    c, ll = r["c"], r["launch"]
    print(f"{name}: {ll} {r['res']}")
    assert (ll["food_slots"], ll["literal_constants"]) == c["kernel"] and ll["observed_capacity"] == 3
    assert ll["actions_in_kernel"] == 2 and ll["full_signature"] == 1 and ll["forced"] == int(r["cfg"].forced_breathing)
    if c["predicated"]:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (0, c["n"])
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (-1, 1)
    else:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (c["n"], 0)
    if c["kernel"][0] in (1, 12):       # no spill to memory in the one-food and 12-slot policy kernels
        assert r["res"]["scratch_bytes"] == 0, r["res"]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_simulator_parity_on_the_actions_taken(name):
    r = device_run(name)
    c, cfg, out, n = r["c"], r["cfg"], r["out"], r["c"]["n"]
    assert not np.isnan(out["actions"]).any() and not np.isnan(out["obs"]).any()
    # the oracle, open loop on the kernel's actions, from the same start state
    orc = pc.ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(r["f64"], r["i32"])
    ref = orc.rollout(np.array(out["actions"]), want_final=True)
    ref_state = orc.get_state()
    orc.close()
    assert np.array_equal(out["terminated"], ref["terminated"]) and np.array_equal(out["truncated"], ref["truncated"]), "flags differ"
    d = obs_diff(cfg, out["obs"], ref["obs"])
    assert d.max() <= OBS_TOL, f"obs diff {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    rd = np.abs(out["reward"].astype(np.float64) - ref["reward64"]) / np.maximum(1.0, np.abs(ref["reward64"]))
    assert rd.max() <= REW_TOL, f"reward diff {rd.max()}"
    f_d, i_d = r["state"]
    assert np.array_equal(i_d, ref_state[1]), "integer state differs"
    assert np.array_equal(np.isnan(f_d), np.isnan(ref_state[0]))
    assert np.where(np.isnan(ref_state[0]), 0.0, np.abs(f_d - ref_state[0])).max() <= STATE_TOL
    ev = pc.count_events(ref)
    print(f"{name}: obs diff {d.max():.3g}, reward diff {rd.max():.3g}, {ev}")
    cases.assert_closed_loop_events(name, ev, r["policy"], out["actions"])
    # statistics are those of a rollout
    assert r["stats"]["env_steps"] == H * n and r["stats"]["episodes"] == int((ref["terminated"] | ref["truncated"]).sum())
    # a twin handle running salp_vec_rollout on the same actions: the same arithmetic, identical bits
    twin = started(cfg, n, r["f64"], r["i32"])
    t = host_outputs(cfg, H, n)
    twin.rollout(np.array(out["actions"]), H, t["obs"], t["reward"], t["terminated"], t["truncated"], None, None, 0)
    assert twin.last_launch()["actions_in_kernel"] == 0
    for k in ("obs", "reward"):
        assert np.array_equal(bits(out[k]), bits(t[k])), f"{k} bits differ from salp_vec_rollout on the same actions"
    assert np.array_equal(out["terminated"], t["terminated"]) and np.array_equal(out["truncated"], t["truncated"])
    assert same_state(r["state"], device_state(twin, cfg)), "final state differs from the twin's"
    assert twin.global_step == H and twin.stats() == r["stats"]
    twin.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_action_is_the_policy_on_the_row_before_it(name):
    r = device_run(name)
    policy, out = r["policy"], r["out"]
    seen = np.concatenate([r["obs0"][None], out["obs"][:-1]])        # act[0] <- observe(); act[t + 1] <- obs[t]
    want, bound = policy.reference(seen), policy.error_bound(seen)
    err = np.abs(out["actions"].astype(np.float64) - want)
    ratio = err / bound
    print(f"{name}: largest |action - reference| / error_bound = {ratio.max():.4f} (error {err.max():.3g}, bound max {bound.max():.3g})")
    assert bound.max() < cases.BOUND_CEILING
    assert (err <= bound).all(), f"{int((err > bound).sum())} actions outside the bound, worst ratio {ratio.max()} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


@pytest.mark.parametrize("name", list(cases.CASES))
def test_split_equals_whole(name):
    """H calls of horizon 1 (each one's action comes from the prologue's observation of the stored state) == one call."""
    r = device_run(name)
    c, cfg, out = r["c"], r["cfg"], r["out"]
    dev = started(cfg, c["n"], r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    got = host_outputs(cfg, H, c["n"])
    for t in range(H):
        dev.rollout_policy(ph, 1, got["obs"][t:t + 1], got["reward"][t:t + 1], got["terminated"][t:t + 1],
                           got["truncated"][t:t + 1], got["actions"][t:t + 1], 0)
    for k in ("actions", "obs", "reward"):
        same = bits(got[k]) == bits(out[k])
        assert same.all(), f"{k}: first difference at {np.unravel_index(np.argmin(same), same.shape)} of {int((~same).sum())}"
    assert np.array_equal(got["terminated"], out["terminated"]) and np.array_equal(got["truncated"], out["truncated"])
    assert same_state(device_state(dev, cfg), r["state"]) and dev.global_step == H
    # statistics: the counters exactly; reward_sum is rounded to 2^-20 once per wavefront and LAUNCH, here H launches against one
    st, want = dev.stats(), r["stats"]
    assert {k: v for k, v in st.items() if k != "reward_sum"} == {k: v for k, v in want.items() if k != "reward_sum"}
    assert abs(st["reward_sum"] - want["reward_sum"]) <= (H + 1) * (c["n"] // 64 + 1) * 2.0 ** -21
    ph.close()
    dev.close()


PROBE_COLUMNS = (6, 10, 12, 13, 17, 23)     # body radius; the nearest food's offset, distance and bearing; the second food's bearing; mean distance


@pytest.mark.parametrize("case,no_autoreset", [("single_food", False), ("sac_gail_F12", False), ("single_food", True), ("sac_gail_F12", True)])
def test_prologue_observation_is_the_row_before_it(case, no_autoreset):
    """A linear probe policy a = clip(obs[c]) (one product by 1.0 behind a zero bias: exact) shows the observation a call's
    prologue forms from the stored state: in calls of horizon 1 it must be the row the call before wrote, column by column —
    whatever the case's MLP happens to be sensitive to.  Column 13 is the one that depends on more than the state's values:
    the step hands the reward's own bearing of the nearest food to the row unless the food set or the episode changed in
    that step (csrc/salp_rollout_kernel.h, the policy prologue); both kinds of wavefront-step must occur."""
    n, HP = 256, 64
    spec = dict(pc.CASES[case])
    spec.setdefault("max_steps_without_food", pc.DEFAULT_BUDGET)
    orc, f64, i32 = pc.start_oracle(pc.make_cfg(spec), n, pc.ENV_SEED)
    orc.close()
    cfg = pc.make_cfg(dict(spec, no_autoreset=no_autoreset))
    assert cfg.act_dim == 1
    for c in PROBE_COLUMNS:
        W = np.zeros((1, cfg.obs_dim), np.float32)
        W[0, c] = 1.0
        dev = started(cfg, n, f64, i32)
        ph = dev.policy_create(MLPPolicy.linear(W, out="clip"))
        got = host_outputs(cfg, HP, n)
        for t in range(HP):
            dev.rollout_policy(ph, 1, got["obs"][t:t + 1], got["reward"][t:t + 1], got["terminated"][t:t + 1],
                               got["truncated"][t:t + 1], got["actions"][t:t + 1], 0)
        ph.close()
        dev.close()
        want = np.clip(got["obs"][:-1, :, c], -1.0, 1.0)
        same = got["actions"][1:, :, 0] == want
        assert same.all(), f"column {c}: {int((~same).sum())} prologue values differ from the row before, first at {np.unravel_index(np.argmin(same), same.shape)}"
        # wavefront-steps in which some lane finished, and wavefront-steps in which none did
        done = (got["terminated"] | got["truncated"]).astype(bool)[:-1]
        per_wave = done.reshape(HP - 1, n // 64, 64).any(axis=2)
        assert per_wave.any() and not per_wave.all(), f"column {c}: {int(per_wave.sum())} of {per_wave.size} wavefront-steps with an episode end"


@pytest.mark.parametrize("P,group", [(4, 64), (2, 128)])
def test_population_each_group_runs_its_own_policy(P, group):
    cfg = pc.case_cfg("single_food")
    n, HP = P * group, 96
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    ps = cases.separated_population(P)
    pop = MLPPolicy.stack(ps)
    dev = started(cfg, n, f64, i32)
    obs0 = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(pop)
    out = run_policy(dev, ph, cfg, HP)
    seen = np.concatenate([obs0[None], out["obs"][:-1]])
    worst = 0.0
    for k, p in enumerate(ps):
        sl = slice(k * group, (k + 1) * group)
        x = seen[:, sl]
        want, bound = p.reference(x), p.error_bound(x)
        err = np.abs(out["actions"][:, sl].astype(np.float64) - want)
        assert (err <= bound).all(), f"group {k}: worst ratio {(err / bound).max()}"
        worst = max(worst, float((err / bound).max()))
        for j, q in enumerate(ps):     # any other policy is more than 100 bounds away on these observations
            if j != k:
                gap = np.abs(q.reference(x) - want)
                assert (gap > 100.0 * np.maximum(bound, q.error_bound(x))).all(), f"policies {k} and {j} are not separated"
    assert np.array_equal(pop.reference(seen), np.concatenate([p.reference(seen[:, k * group:(k + 1) * group]) for k, p in enumerate(ps)], axis=1))
    print(f"P = {P} x {group} envs: largest ratio {worst:.4f}")
    ph.close()
    dev.close()


def _refusal_cases(dev, other, ph, ph_other, cfg, n):
    o = host_outputs(cfg, 2, n)
    args = lambda **kw: {**dict(handle=ph, horizon=2, obs=o["obs"], reward=o["reward"], term=o["terminated"],
                                trunc=o["truncated"], act_out=o["actions"], flags=0), **kw}
    yield "policy of another handle", args(handle=ph_other)
    yield "horizon 0", args(horizon=0)
    yield "negative horizon", args(horizon=-3)
    for k in ("obs", "reward", "term", "trunc"):
        yield f"NULL {k}", args(**{k: None})


def test_refusals_leave_the_handle_unchanged():
    cfg = pc.case_cfg("single_food")
    free = pc.case_cfg("free_breathing")
    n = 256
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    dev, other = started(cfg, n, f64, i32), SalpLib(cfg, n, device_id=0, seed=1)
    other_dims = SalpLib(free, n, device_id=0, seed=1)
    p = cases.case_policy("one_food_mlp32")
    ph, ph_other = dev.policy_create(p), other.policy_create(p)
    ph_dims = other_dims.policy_create(cases.case_policy("free_breathing_mlp32"))
    before, step0, stats0 = device_state(dev, cfg), dev.global_step, dev.stats()
    tried = 0
    for label, kw in list(_refusal_cases(dev, other, ph, ph_other, cfg, n)) + [("policy of other dimensions", None)]:
        if kw is None:
            kw = dict(list(_refusal_cases(dev, other, ph, ph_dims, cfg, n))[0][1])
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.rollout_policy(**kw)
        assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0, label
        tried += 1
    assert tried == 8
    # descriptors outside the ranges, and P that n_envs does not allow: refused at create (and by salp_policy_words)
    lib = dev.lib

    def desc(n_hidden=2, hidden=(32, 32), out=0, P=1, size=None):
        from underwater_swimmer_rl_amd.policy import CPolicyDesc
        d = CPolicyDesc()
        d.struct_size = ctypes.sizeof(CPolicyDesc) if size is None else size
        d.n_hidden, d.out_activation, d.n_policies = n_hidden, out, P
        d.hidden[0], d.hidden[1] = hidden
        return d
    assert lib.salp_policy_words(dev._h, ctypes.byref(desc())) == p.words
    w = np.zeros(4 * 4096, np.float32)
    bad = [desc(n_hidden=3), desc(n_hidden=-1), desc(hidden=(32, 24)), desc(hidden=(80, 32)), desc(hidden=(0, 32)),
           desc(n_hidden=1, hidden=(32, 32)), desc(out=2), desc(P=0), desc(P=3), desc(P=8), desc(size=20)]
    for d in bad:
        h = ctypes.c_void_p()
        assert lib.salp_policy_words(dev._h, ctypes.byref(d)) == -1
        assert lib.salp_policy_create(dev._h, ctypes.byref(d), w.ctypes.data_as(ctypes.c_void_p), 0, None, ctypes.byref(h)) == -1
        assert not h.value
    assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0
    # max_observed_food != 3: no policy kernels
    k2 = SalpLib(pc.case_cfg("K2_generic"), 64, device_id=0, seed=1)
    with pytest.raises(SalpError):
        k2.policy_create(cases.random_policy(k2.obs_dim, 1, (16,), "tanh", 0, 1, 1))
    # the handle still works
    out = run_policy(dev, ph, cfg, 2)
    assert not np.isnan(out["obs"]).any() and dev.global_step == step0 + 2
    for h in (ph, ph_other, ph_dims):
        h.close()
    for d in (dev, other, other_dims, k2):
        d.close()


@pytest.mark.parametrize("name", ["one_food_mlp32_ragged", "free_breathing_mlp32"])
def test_device_pointers_guard_words_and_null_act_out(name):
    """Device pointers into blocks followed by sentinel words: nothing behind any output is written; without act_out the
    other outputs and the state are those of the run with it."""
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
    for with_actions in (True, False):
        dev = started(cfg, n, r["f64"], r["i32"])
        ph = dev.policy_create(r["policy"])
        bl = dict(obs=block((HG, n, cfg.obs_dim), torch.float32), reward=block((HG, n), torch.float32),
                  terminated=block((HG, n), torch.uint8), truncated=block((HG, n), torch.uint8),
                  actions=block((HG, n, cfg.act_dim), torch.float32))
        torch.cuda.synchronize()
        dev.rollout_policy(ph, HG, bl["obs"][0], bl["reward"][0], bl["terminated"][0], bl["truncated"][0],
                           bl["actions"][0] if with_actions else None, DEV, 0)
        torch.cuda.synchronize()
        for k, (b, rows) in bl.items():
            host = b.cpu().numpy()
            guard = host[rows:]
            assert (guard == 0xA5).all() if host.dtype == np.uint8 else (guard.view(np.uint32) == SENTINEL).all(), f"{k}: guard words written"
            if k == "actions" and not with_actions:
                assert (host.view(np.uint32) == SENTINEL).all(), "act_out == NULL, yet the block was written"
                continue
            want = out[k][:HG].reshape(-1)
            assert np.array_equal(host[:rows].view(np.uint32) if host.dtype != np.uint8 else host[:rows],
                                  bits(want) if want.dtype != np.uint8 else want), f"{k} differs from the host-pointer run"
        ph.close()
        dev.close()


def test_graph_capture_replays_and_takes_new_weights_without_recapture():
    import torch
    name = "one_food_mlp32"
    c, cfg, policy, f64, i32 = cases.start_snapshot(name)
    n, K = c["n"], 16
    policy_b = cases.random_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["out"], 999, c["gain"], c["out_gain"])
    assert policy_b.words == policy.words
    eager, graphed = started(cfg, n, f64, i32), started(cfg, n, f64, i32)
    ph_e, ph_g = eager.policy_create(policy), graphed.policy_create(policy)
    w_b = torch.tensor(policy_b.pack(), device="cuda:0")

    def blocks():
        return dict(obs=torch.zeros(K, n, cfg.obs_dim, device="cuda:0"), reward=torch.zeros(K, n, device="cuda:0"),
                    terminated=torch.zeros(K, n, dtype=torch.uint8, device="cuda:0"),
                    truncated=torch.zeros(K, n, dtype=torch.uint8, device="cuda:0"),
                    actions=torch.zeros(K, n, cfg.act_dim, device="cuda:0"))
    bg, be = blocks(), blocks()

    def call(dev, ph, b, stream):
        dev.rollout_policy(ph, K, b["obs"], b["reward"], b["terminated"], b["truncated"], b["actions"], DEV, stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    step_before = graphed.global_step
    with torch.cuda.graph(g):
        call(graphed, ph_g, bg, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert same_state(device_state(graphed, cfg), (f64, i32)), "capture must not execute"
    assert graphed.global_step == step_before + K          # the host counter advances per CALL, as for a captured rollout
    obs_last = None
    for rep in range(4):
        if rep == 2:        # new weights between two replays: stream-ordered, nothing allocated, no re-capture
            ph_g.update(w_b, DEV, int(torch.cuda.current_stream().cuda_stream))
            ph_e.update(policy_b.pack())                  # host pointers on the eager side
        seen0 = np.empty((n, cfg.obs_dim), np.float32)
        eager.observe(seen0, 0)
        g.replay()
        call(eager, ph_e, be, 0)
        torch.cuda.synchronize()
        for k in bg:
            assert torch.equal(bg[k], be[k]), (rep, k)
        pol = policy if rep < 2 else policy_b
        seen = np.concatenate([seen0[None], be["obs"][:-1].cpu().numpy()])
        acts = be["actions"].cpu().numpy().astype(np.float64)
        assert (np.abs(acts - pol.reference(seen)) <= pol.error_bound(seen)).all(), rep
        if rep == 2:        # and they are NOT the old policy's
            assert (np.abs(acts - policy.reference(seen)) > 100 * policy.error_bound(seen)).mean() > 0.5
        obs_last = be["obs"][-1]
    assert same_state(device_state(graphed, cfg), device_state(eager, cfg))
    assert graphed.stats() == eager.stats() and eager.stats()["env_steps"] == 4 * K * n
    assert eager.global_step == 4 * K
    # as for salp_vec_rollout: a twin stepping the eager handle's actions ends in the same place
    for h in (ph_e, ph_g):
        h.close()
    eager.close()
    graphed.close()


def test_vector_env_surface():
    import torch
    from underwater_swimmer_rl_amd import MLPPolicy as Exported, SalpVectorEnv, pursuit_policy
    assert Exported is MLPPolicy
    env = SalpVectorEnv("single_food", num_envs=256, seed=3)
    obs0, _ = env.reset()
    obs0 = obs0.clone()
    p = pursuit_policy(3.0)
    out = env.rollout_policy(p, 32)
    assert set(out) == {"obs", "reward", "terminated", "truncated", "final_obs", "actions"} and out["actions"].shape == (32, 256, 1)
    seen = torch.cat([obs0[None], out["obs"][:-1]])
    assert torch.equal(out["actions"], (-3.0 * seen[..., 13:14]).clamp(-1.0, 1.0))      # one product, exact in fp32
    assert env.rollout_policy(p, 4, want_actions=False)["actions"] is None
    assert env.global_step == 36
    with pytest.raises(ValueError):
        env.make_policy(MLPPolicy.stack([p] * 3))
    with pytest.raises(ValueError):
        env.make_policy(cases.random_policy(24, 2, (16,), "tanh", 0, 1, 1))
    env.close()
