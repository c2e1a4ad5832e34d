"""Closed-loop rollouts that return packed transition records (salp_vec_rollout_policy_packed and _sampled,
include/salp_vec_policy_packed.h) on the GPU, over the case table of tests/policy_packed_cases.py (configurations and injected
start state of tests/parity_cases.py).  Run with `pytest -m gpu`.

The calls define nothing new, so every check is against a parent.  Per case, from the same snapshot on fresh handles: the
record's obs / reward / flags, the actions, the final state, the statistics and the global step against
salp_vec_rollout_policy (bit for bit); the WHOLE block, NaN tails of unfinished rows included, against
salp_vec_rollout_packed on the actions taken (word for word: the same kernels' arithmetic, -ffp-contract=off, another
output route); the block and the state against the C oracle stepped on those actions (the project's tolerances).  Then the
kernel that ran, the sampled form (with logp_out and the noise step), a run cut in two, the split launch, a population,
refusals, hipGraph capture, the kernels' resources, and the Python surface with sac.collect_in_kernel(keep_truncated=True)."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
import policy_cases as dc
import policy_packed_cases as cases
from gpu_support import (assert_final_obs, assert_parity, assert_state_parity, device_state, run_policy, run_sampled, started)
from support import bits, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpError, SalpLib
from underwater_swimmer_rl_amd.policy import MLPPolicy
from underwater_swimmer_rl_amd.records import record_width, transitions, unpack_record

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D          # guard words behind the block (an unlikely float: -1.7e-16)
DEV, FIN = _capi.SALP_DEVICE_PTRS, _capi.REC_FINAL_OBS
H = cases.H
NOISE0 = (1 << 32) - 100       # above 2^32 - H: the low word of the noise step wraps inside every sampled run
CUT = 100                      # a run cut in two: 100 + 284 steps


def nan_block(horizon, n, width):
    """A device block [horizon + 1, n, width]: NaN rows for the call, then one guard row of sentinel words."""
    import torch
    buf = torch.full((horizon + 1, n, width), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[horizon].view(torch.int32).fill_(int(np.uint32(SENTINEL).view(np.int32)))
    assert buf.data_ptr() % 16 == 0
    return buf


def run_pp(dev, ph, horizon, final=True, sampled=False, want_actions=True, want_logp=True):
    """rollout_policy_packed(_sampled) with DEVICE pointers into a NaN-filled block behind which one guard row sits.
    Returns host arrays: record [horizon, n, width], guard, actions, logp (None where not asked for)."""
    import torch
    n = dev.n_envs
    buf = nan_block(horizon, n, dev.record_width(final))
    act = torch.full((horizon, n, dev.act_dim), float("nan"), device="cuda:0") if want_actions else None
    logp = torch.full((horizon, n), float("nan"), device="cuda:0") if sampled and want_logp else None
    torch.cuda.synchronize()
    flags = DEV | (FIN if final else 0)
    if sampled:
        dev.rollout_policy_packed_sampled(ph, horizon, buf, act, logp, flags, 0)
    else:
        dev.rollout_policy_packed(ph, horizon, buf, act, flags, 0)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return dict(record=host[:horizon], guard=host[horizon], actions=None if act is None else act.cpu().numpy(),
                logp=None if logp is None else logp.cpu().numpy())


def run_open(dev, actions, final=True):
    """salp_vec_rollout_packed on recorded actions, device pointers, into a NaN-filled block: the open-loop twin."""
    import torch
    horizon, n = actions.shape[:2]
    buf = nan_block(horizon, n, dev.record_width(final))
    a = torch.tensor(np.array(actions), device="cuda:0")
    torch.cuda.synchronize()
    dev.rollout_packed(a, horizon, buf, None, DEV | (FIN if final else 0), 0)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return dict(record=host[:horizon], guard=host[horizon])


def after(dev, cfg, ph=None):
    return dict(state=device_state(dev, cfg), stats=dev.stats(), step=dev.global_step, launch=dev.last_launch(),
                noise=ph.noise_step if ph is not None and ph.gaussian else None)


def freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


def device_run(name, sampled=False):
    return _device_run(name, bool(sampled))


@functools.lru_cache(maxsize=None)
def _device_run(name, sampled):
    """One case, three fresh handles in the case's snapshot: the packed closed loop (terminal tails on), its closed-loop twin
    salp_vec_rollout_policy(_sampled), and its open-loop twin salp_vec_rollout_packed on the actions taken.  Computed once,
    shared by the tests below, read-only."""
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    if sampled:
        policy = cases.gaussian_twin(name)
    n = c["n"]

    def handle():
        dev = started(cfg, n, f64, i32)
        ph = dev.policy_create(policy)
        if sampled:
            ph.set_noise_step(NOISE0)
        return dev, ph
    dev, ph = handle()
    pp = run_pp(dev, ph, H, True, sampled)
    pp.update(after(dev, cfg, ph), res=dev.last_kernel_resources())
    ph.close()
    dev.close()
    dev, ph = handle()
    closed = (run_sampled if sampled else run_policy)(dev, ph, cfg, H)
    closed.update(after(dev, cfg, ph))
    ph.close()
    dev.close()
    dev = started(cfg, n, f64, i32)
    opened = run_open(dev, pp["actions"])
    opened.update(after(dev, cfg))
    dev.close()
    return dict(c=c, cfg=cfg, policy=policy, f64=f64, i32=i32, pp=freeze(pp), closed=freeze(closed), open=freeze(opened))


def finished(rec, obs_dim):
    u = unpack_record(rec, obs_dim)
    return u["terminated"] | u["truncated"]


def check_against_closed_loop_twin(r, sampled, label):
    """Record obs / reward / flags, act_out (and logp_out), final state, statistics, global step (and noise step): the bits of
    salp_vec_rollout_policy(_sampled).  Guard words intact, byte 3 of every flags word zero."""
    cfg, pp, t = r["cfg"], r["pp"], r["closed"]
    D = cfg.obs_dim
    rec = pp["record"]
    assert rec.shape == (H, r["c"]["n"], record_width(D, True))
    u = unpack_record(rec, D)
    assert not np.isnan(t["obs"]).any() and not np.isnan(t["actions"]).any()
    for k in ("obs", "reward"):
        same = bits(u[k]) == bits(t[k])
        assert same.all(), f"{label}: {k}: {int((~same).sum())} words differ from the closed-loop twin, first at {np.unravel_index(np.argmin(same), same.shape)}"
    assert np.array_equal(u["terminated"].view(np.uint8), t["terminated"]) and np.array_equal(u["truncated"].view(np.uint8), t["truncated"]), label
    assert np.array_equal(bits(pp["actions"]), bits(t["actions"])), f"{label}: act_out differs"
    if sampled:
        assert not np.isnan(t["logp"]).any() and np.array_equal(bits(pp["logp"]), bits(t["logp"])), f"{label}: logp_out differs"
        assert pp["noise"] == t["noise"] == NOISE0 + H, (pp["noise"], t["noise"])
    assert same_state(pp["state"], t["state"]), f"{label}: final state differs from the closed-loop twin's"
    assert pp["stats"] == t["stats"] and pp["stats"]["env_steps"] == H * r["c"]["n"], (pp["stats"], t["stats"])
    assert pp["step"] == t["step"] == H
    assert (pp["guard"].view(np.uint32) == SENTINEL).all(), f"{label}: words behind the block were written"
    assert not rec.view(np.uint8)[..., 4 * (D + _capi.REC_FLAGS) + 3].any(), f"{label}: byte 3 of a flags word is not 0"


def check_against_open_loop_twin(r, label):
    """The WHOLE block, word for word: info counters, collision byte, terminal tails of finished rows, untouched NaN tails."""
    cfg, pp, o = r["cfg"], r["pp"], r["open"]
    assert o["launch"]["actions_in_kernel"] == 0 and o["launch"]["full_signature"] == 3
    same = pp["record"].view(np.uint32) == o["record"].view(np.uint32)
    assert same.all(), f"{label}: {int((~same).sum())} words differ from salp_vec_rollout_packed on the actions taken, first at {np.unravel_index(np.argmin(same), same.shape)}"
    done = finished(pp["record"], cfg.obs_dim)
    fin = unpack_record(pp["record"], cfg.obs_dim)["final_observation"]
    assert done.any() and np.isnan(fin[~done]).all() and not np.isnan(fin[done]).any(), f"{label}: the tails written are not those of the finished rows"
    assert (o["guard"].view(np.uint32) == SENTINEL).all()
    assert same_state(pp["state"], o["state"]) and pp["stats"] == o["stats"] and o["step"] == H, label


@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_the_closed_loop_twin(name):
    check_against_closed_loop_twin(device_run(name), False, name)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_the_open_loop_packed_twin(name):
    check_against_open_loop_twin(device_run(name), name)


class Snapshot:
    """What gpu_support.assert_state_parity reads of a handle, served from a stored state."""

    def __init__(self, state):
        self.state, self.n_envs = state, state[0].shape[1]

    def get_state(self, f64, i32, flags):
        f64[...] = self.state[0]
        i32[...] = self.state[1]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_the_oracle_on_the_actions_taken(name):
    r = device_run(name)
    c, cfg, pp, n = r["c"], r["cfg"], r["pp"], r["c"]["n"]
    orc = ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(r["f64"], r["i32"])
    ref = orc.rollout(np.array(pp["actions"]), want_final=True)
    ref_state = orc.get_state()
    orc.close()
    u = unpack_record(pp["record"], cfg.obs_dim)
    got = dict(obs=u["obs"], reward=u["reward"], terminated=u["terminated"].view(np.uint8), truncated=u["truncated"].view(np.uint8))
    dmax, rmax = assert_parity(cfg, got, ref, name)
    fmax = assert_final_obs(cfg, u["final_observation"], ref, name)        # demands done.any(): the tail branch is never dead
    assert np.array_equal(u["collision"], ref["info"][..., pc.INFO_COLLISION]), f"{name}: collision byte differs"
    assert np.array_equal(u["food_collected"], ref["info"][..., pc.INFO_FOOD_COLLECTED]), f"{name}: food_collected differs"
    assert np.array_equal(u["steps_since_food"], ref["info"][..., pc.INFO_STEPS_SINCE_FOOD]), f"{name}: steps_since_food differs"
    assert_state_parity(cfg, Snapshot(pp["state"]), ref_state, name)
    ev = pc.count_events(ref)
    print(f"{name}: obs diff {dmax:.3g}, reward diff {rmax:.3g}, final_obs diff {fmax:.3g}, {ev}")
    cases.assert_events(name, ev)
    assert pp["stats"]["episodes"] == int((ref["terminated"] | ref["truncated"]).sum())


def assert_launch(ll, c, cfg, source):
    assert (ll["food_slots"], ll["literal_constants"]) == c["kernel"] and ll["observed_capacity"] == 3, ll
    assert ll["full_signature"] == 3 and ll["actions_in_kernel"] == source and ll["forced"] == int(cfg.forced_breathing), ll
    if c["predicated"]:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (0, c["n"]), ll
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (-1, 3), ll
    else:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (c["n"], 0), ll
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (3, -1), ll


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_intended_kernel_ran(name):
    r = device_run(name)
    print(f"{name}: {r['pp']['launch']} {r['pp']['res']}")
    assert_launch(r["pp"]["launch"], r["c"], r["cfg"], 2)
    twin = r["closed"]["launch"]
    assert twin["full_signature"] == 1 and twin["actions_in_kernel"] == 2
    assert (twin["envs_unpredicated"], twin["envs_predicated"]) == (r["pp"]["launch"]["envs_unpredicated"], r["pp"]["launch"]["envs_predicated"])


@pytest.mark.parametrize("name", cases.NARROW)
def test_without_the_terminal_tail_the_block_is_the_narrow_one(name):
    r = device_run(name)
    c, cfg, D = r["c"], r["cfg"], r["cfg"].obs_dim
    dev = started(cfg, c["n"], r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    out = run_pp(dev, ph, H, final=False)
    assert out["record"].shape == (H, c["n"], D + 4) and dev.record_width(False) == D + 4
    assert_launch(dev.last_launch(), c, cfg, 2)
    assert np.array_equal(out["record"].view(np.uint32), r["pp"]["record"][..., :D + 4].view(np.uint32)), "the narrow record is not the wide one's head"
    assert np.array_equal(bits(out["actions"]), bits(r["pp"]["actions"]))
    assert (out["guard"].view(np.uint32) == SENTINEL).all()
    assert same_state(device_state(dev, cfg), r["pp"]["state"]) and dev.stats() == r["pp"]["stats"]
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", cases.SAMPLED)
def test_sampled_against_both_twins(name):
    r = device_run(name, True)
    assert_launch(r["pp"]["launch"], r["c"], r["cfg"], 3)
    assert r["closed"]["launch"]["actions_in_kernel"] == 3 and r["closed"]["launch"]["full_signature"] == 1
    check_against_closed_loop_twin(r, True, f"{name} (sampled)")
    check_against_open_loop_twin(r, f"{name} (sampled)")


@pytest.mark.parametrize("name", cases.SAMPLED)
def test_sampled_null_outputs_change_nothing_else(name):
    r = device_run(name, True)
    c, cfg = r["c"], r["cfg"]
    for want_actions, want_logp in ((False, True), (True, False), (False, False)):
        dev = started(cfg, c["n"], r["f64"], r["i32"])
        ph = dev.policy_create(r["policy"])
        ph.set_noise_step(NOISE0)
        out = run_pp(dev, ph, H, True, True, want_actions, want_logp)
        assert np.array_equal(out["record"].view(np.uint32), r["pp"]["record"].view(np.uint32)), (want_actions, want_logp)
        assert (out["guard"].view(np.uint32) == SENTINEL).all()
        if want_actions:
            assert np.array_equal(bits(out["actions"]), bits(r["pp"]["actions"]))
        if want_logp:
            assert np.array_equal(bits(out["logp"]), bits(r["pp"]["logp"]))
        assert same_state(device_state(dev, cfg), r["pp"]["state"]) and dev.stats() == r["pp"]["stats"]
        assert ph.noise_step == NOISE0 + H and dev.global_step == H
        ph.close()
        dev.close()
    # the deterministic form without act_out
    d = device_run(name)
    dev = started(cfg, c["n"], d["f64"], d["i32"])
    ph = dev.policy_create(d["policy"])
    out = run_pp(dev, ph, H, want_actions=False)
    assert np.array_equal(out["record"].view(np.uint32), d["pp"]["record"].view(np.uint32)) and same_state(device_state(dev, cfg), d["pp"]["state"])
    ph.close()
    dev.close()


@pytest.mark.parametrize("sampled", [False, True])
def test_split_equals_whole(sampled):
    """100 + 284 steps in two calls into the two halves of one block == one call of 384, bit for bit: the second call's first
    action comes from the prologue's observation of the stored state."""
    import torch
    name = "class_default_F5"
    r = device_run(name, sampled)
    c, cfg, n = r["c"], r["cfg"], r["c"]["n"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    if sampled:
        ph.set_noise_step(NOISE0)
    buf = nan_block(H, n, dev.record_width(True))
    act = torch.full((H, n, cfg.act_dim), float("nan"), device="cuda:0")
    logp = torch.full((H, n), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    for lo, hi in ((0, CUT), (CUT, H)):
        assert buf[lo:hi].data_ptr() % 16 == 0
        if sampled:
            dev.rollout_policy_packed_sampled(ph, hi - lo, buf[lo:hi], act[lo:hi], logp[lo:hi], DEV | FIN, 0)
        else:
            dev.rollout_policy_packed(ph, hi - lo, buf[lo:hi], act[lo:hi], DEV | FIN, 0)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    same = host[:H].view(np.uint32) == r["pp"]["record"].view(np.uint32)
    assert same.all(), f"{int((~same).sum())} words differ, first at {np.unravel_index(np.argmin(same), same.shape)}"
    assert (host[H].view(np.uint32) == SENTINEL).all()
    assert np.array_equal(bits(act.cpu().numpy()), bits(r["pp"]["actions"]))
    if sampled:
        assert np.array_equal(bits(logp.cpu().numpy()), bits(r["pp"]["logp"])) and ph.noise_step == NOISE0 + H
    assert same_state(device_state(dev, cfg), r["pp"]["state"]) and dev.global_step == H
    # statistics: the counters exactly; reward_sum is rounded to 2^-20 once per wavefront and LAUNCH, here two launches against one
    st, want = dev.stats(), r["pp"]["stats"]
    assert {k: v for k, v in st.items() if k != "reward_sum"} == {k: v for k, v in want.items() if k != "reward_sum"}
    assert abs(st["reward_sum"] - want["reward_sum"]) <= 3 * (n // 64 + 1) * 2.0 ** -21
    ph.close()
    dev.close()


def test_split_launch_both_halves_in_the_packed_signature():
    """The smallest shape that splits (tests/test_gpu_packed_record.py::test_packed_split_launch): 4096 envs unpredicated + 37
    predicated.  Against the two twins only, compared on the device (a block is 0.9 GB)."""
    import torch
    cfg = pc.make_cfg(dict(preset="sac_gail", max_steps_without_food=300))
    n, HS = 4096 + 37, 1020
    assert n * HS > 1 << 22
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED, threads=4)
    orc.close()
    policy = cases.case_policy("sac_gail_mlp64")
    D, W = cfg.obs_dim, record_width(cfg.obs_dim, True)
    words = lambda t: t.contiguous().view(torch.int32)
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    buf = nan_block(HS, n, W)
    act = torch.full((HS, n, cfg.act_dim), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    dev.rollout_policy_packed(ph, HS, buf, act, DEV | FIN, 0)
    torch.cuda.synchronize()
    ll = dev.last_launch()
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (4096, 37), ll
    assert (ll["full_signature"], ll["signature_unpredicated"], ll["signature_predicated"], ll["actions_in_kernel"]) == (3, 3, 3, 2), ll
    state, stats = device_state(dev, cfg), dev.stats()
    assert dev.global_step == HS and stats["env_steps"] == HS * n
    ph.close()
    dev.close()
    sent = int(np.uint32(SENTINEL).view(np.int32))
    assert bool((buf[HS].view(torch.int32) == sent).all()), "words behind the block were written"
    u = unpack_record(buf[:HS], D)
    done = u["terminated"] | u["truncated"]
    assert bool(done[:, :4096].any()) and bool(done[:, 4096:].any()), "a half of the launch finishes no episode"
    assert bool(torch.isnan(u["final_observation"][..., 0]).eq(~done).all()), "the tails written are not those of the finished rows"
    assert not bool(torch.isnan(act).any())
    # the closed-loop twin
    twin = started(cfg, n, f64, i32)
    pt = twin.policy_create(policy)
    t = dict(obs=torch.full((HS, n, D), float("nan"), device="cuda:0"), reward=torch.full((HS, n), float("nan"), device="cuda:0"),
             terminated=torch.full((HS, n), 7, dtype=torch.uint8, device="cuda:0"), truncated=torch.full((HS, n), 7, dtype=torch.uint8, device="cuda:0"),
             actions=torch.full((HS, n, cfg.act_dim), float("nan"), device="cuda:0"))
    torch.cuda.synchronize()
    twin.rollout_policy(pt, HS, t["obs"], t["reward"], t["terminated"], t["truncated"], t["actions"], DEV, 0)
    torch.cuda.synchronize()
    assert twin.last_launch()["full_signature"] == 1
    assert torch.equal(words(u["obs"]), words(t["obs"])) and torch.equal(words(u["reward"]), words(t["reward"]))
    assert torch.equal(u["terminated"].view(torch.uint8), t["terminated"]) and torch.equal(u["truncated"].view(torch.uint8), t["truncated"])
    assert torch.equal(words(act), words(t["actions"]))
    assert same_state(device_state(twin, cfg), state) and twin.stats() == stats
    pt.close()
    twin.close()
    del t
    # the open-loop packed twin: the whole block
    op = started(cfg, n, f64, i32)
    other = nan_block(HS, n, W)
    torch.cuda.synchronize()
    op.rollout_packed(act, HS, other, None, DEV | FIN, 0)
    torch.cuda.synchronize()
    lo = op.last_launch()
    assert (lo["envs_unpredicated"], lo["envs_predicated"], lo["actions_in_kernel"]) == (4096, 37, 0)
    assert torch.equal(buf.view(torch.int32), other.view(torch.int32)), "the block differs from salp_vec_rollout_packed on the actions taken"
    assert same_state(device_state(op, cfg), state) and op.stats() == stats
    op.close()


def test_population_each_group_runs_its_own_policy():
    cfg = pc.case_cfg("single_food")
    P, group, HP = 4, 64, 96
    n = P * group
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    ps = dc.separated_population(P)
    dev = started(cfg, n, f64, i32)
    obs0 = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(MLPPolicy.stack(ps))
    out = run_pp(dev, ph, HP)
    state = device_state(dev, cfg)
    ph.close()
    dev.close()
    seen = np.concatenate([obs0[None], unpack_record(out["record"], cfg.obs_dim)["obs"][:-1]])
    for k, p in enumerate(ps):
        sl = slice(k * group, (k + 1) * group)
        x = seen[:, sl]
        want, bound = p.reference(x), p.error_bound(x)
        err = np.abs(out["actions"][:, sl].astype(np.float64) - want)
        assert (err <= bound).all(), f"group {k}: worst ratio {(err / bound).max()}"
        for j, q in enumerate(ps):     # any other policy is more than 100 bounds away on these observations
            if j != k:
                assert (np.abs(q.reference(x) - want) > 100.0 * np.maximum(bound, q.error_bound(x))).all(), f"policies {k} and {j} are not separated"
    twin = started(cfg, n, f64, i32)
    o = run_open(twin, out["actions"])
    assert np.array_equal(out["record"].view(np.uint32), o["record"].view(np.uint32)), "the block differs from the open-loop twin's"
    assert finished(out["record"], cfg.obs_dim).any() and same_state(device_state(twin, cfg), state)
    twin.close()


def test_refusals_leave_the_handle_and_the_noise_step_unchanged():
    import torch
    from sampled_cases import gaussian_policy
    cfg, free = pc.case_cfg("single_food"), pc.case_cfg("free_breathing")
    n = 256
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    dev, other, other_dims = started(cfg, n, f64, i32), SalpLib(cfg, n, device_id=0, seed=1), SalpLib(free, n, device_id=0, seed=1)
    k5 = SalpLib(pc.case_cfg("F9_K5_generic_reg"), n, device_id=0, seed=1)
    g = gaussian_policy(cfg.obs_dim, 1, (32, 32), 123, 1.5, 2.0, (-1.0,))
    ph, ph_plain, ph_other = dev.policy_create(g), dev.policy_create(g.mean_policy()), other.policy_create(g)
    ph_dims = other_dims.policy_create(cases.case_policy("free_breathing_mlp32"))
    ph.set_noise_step(41)
    W = dev.record_width(True)
    first = run_pp(dev, ph, 2, True, True)      # a launch to remember: last_launch is not the empty one
    assert ph.noise_step == 43 and dev.global_step == 2
    sent = int(np.uint32(SENTINEL).view(np.int32))
    G = 64
    block = torch.full((G + 2 * n * W + G,), sent, dtype=torch.int32, device="cuda:0")
    drec = block[G:G + 2 * n * W].view(torch.float32)
    assert drec.data_ptr() % 16 == 0
    hrec = np.full((2, n, W), np.nan, np.float32)
    hact = np.full((2, n, 1), np.nan, np.float32)
    torch.cuda.synchronize()
    before, step0, stats0, launch0 = device_state(dev, cfg), dev.global_step, dev.stats(), dev.last_launch()
    base = dict(handle=ph, horizon=2, rec=hrec, act_out=hact, flags=FIN)
    refused = [
        ("NULL rec (host)", dict(rec=None)), ("NULL rec (device)", dict(rec=None, flags=DEV)),
        ("horizon 0", dict(horizon=0)), ("negative horizon", dict(horizon=-3, flags=0)),
        ("the summary's flag", dict(flags=_capi.EVAL_ACCUMULATE)), ("an unknown flag", dict(flags=8)),
        ("an unknown flag next to the known ones", dict(rec=drec, act_out=None, flags=DEV | FIN | 0x100)),
        ("misaligned device rec (4 B)", dict(rec=drec.data_ptr() + 4, act_out=None, flags=DEV)),
        ("misaligned device rec (8 B)", dict(rec=drec.data_ptr() + 8, act_out=None, flags=DEV | FIN)),
        ("policy of another handle", dict(handle=ph_other)), ("policy of other dimensions", dict(handle=ph_dims)),
    ]

    def unchanged(label):
        assert same_state(device_state(dev, cfg), before) and dev.global_step == step0 and dev.stats() == stats0, label
        assert dev.last_launch() == launch0 and ph.noise_step == 43, label
        assert np.isnan(hrec).all() and np.isnan(hact).all(), label
    tried = 0
    for label, kw in refused:
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.rollout_policy_packed(**{**base, **kw})
        unchanged(label)
        with pytest.raises(SalpError, match=r"\(-1\)"):
            dev.rollout_policy_packed_sampled(**{**base, "logp_out": None, **kw})
        unchanged(label + " (sampled)")
        tried += 2
    with pytest.raises(SalpError, match=r"\(-1\)"):      # the sampled form needs a Gaussian policy ...
        dev.rollout_policy_packed_sampled(ph_plain, 2, hrec, hact, None, FIN)
    unchanged("a plain policy, sampled")
    assert tried == 22
    torch.cuda.synchronize()
    assert (block.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to the device block"
    # a P that n_envs does not allow: refused where the policy is made, so no call ever sees one
    for P in (3, 8):
        with pytest.raises((SalpError, ValueError)):
            dev.policy_create(MLPPolicy.stack([g.mean_policy()] * P))
    # max_observed_food != 3 (a K = 5 handle): no policy can be made for it, and a policy of another handle is refused
    with pytest.raises((SalpError, ValueError)):
        k5.policy_create(dc.random_policy(k5.obs_dim, 1, (16,), "tanh", 0, 1, 1))
    rec5 = np.full((2, n, k5.record_width(True)), np.nan, np.float32)
    s5, l5 = device_state(k5, pc.case_cfg("F9_K5_generic_reg")), k5.last_launch()
    for call in (lambda: k5.rollout_policy_packed(ph_plain, 2, rec5, None, FIN),
                 lambda: k5.rollout_policy_packed_sampled(ph, 2, rec5, None, None, FIN)):
        with pytest.raises(SalpError, match=r"\(-1\)"):
            call()
        assert k5.global_step == 0 and k5.last_launch() == l5 and np.isnan(rec5).all()
        assert same_state(device_state(k5, pc.case_cfg("F9_K5_generic_reg")), s5)
    unchanged("after the K = 5 handle")
    # ... and the deterministic form runs a Gaussian policy's mean; the handle still works
    a = run_pp(dev, ph, 2)
    assert ph.noise_step == 43 and dev.global_step == step0 + 2 and not np.isnan(unpack_record(a["record"], cfg.obs_dim)["obs"]).any()
    assert not np.isnan(first["logp"]).any()
    for h in (ph, ph_plain, ph_other, ph_dims):
        h.close()
    for d in (dev, other, other_dims, k5):
        d.close()


@pytest.mark.parametrize("sampled", [False, True])
def test_graph_capture_replays_and_takes_new_weights_without_recapture(sampled):
    """The device-pointer call captured into a hipGraph, replayed twice with salp_policy_update between the replays == the same
    two eager calls.  The process keeps its default queue count."""
    import torch
    from sampled_cases import gaussian_policy
    name = "one_food_mlp32"
    c, cfg, policy, f64, i32 = dc.start_snapshot(name, cases)
    n, K = c["n"], 8
    if sampled:
        policy, policy_b = (gaussian_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], s, c["gain"], 2.0, (-1.0,)) for s in (c["seed"], 999))
    else:
        policy_b = dc.random_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["out"], 999, c["gain"], c["out_gain"])
    assert policy_b.words == policy.words
    eager, graphed = started(cfg, n, f64, i32), started(cfg, n, f64, i32)
    ph_e, ph_g = eager.policy_create(policy), graphed.policy_create(policy)
    w_b = torch.tensor(policy_b.pack(), device="cuda:0")
    W = eager.record_width(True)

    def blocks():
        return dict(rec=nan_block(K, n, W), act=torch.full((K, n, cfg.act_dim), float("nan"), device="cuda:0"),
                    logp=torch.full((K, n), float("nan"), device="cuda:0"))
    bg, be = blocks(), blocks()

    def call(dev, ph, b, stream):
        if sampled:
            dev.rollout_policy_packed_sampled(ph, K, b["rec"], b["act"], b["logp"], DEV | FIN, stream)
        else:
            dev.rollout_policy_packed(ph, K, b["rec"], b["act"], DEV | FIN, stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(graphed, ph_g, bg, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert same_state(device_state(graphed, cfg), (f64, i32)), "capture must not execute"
    assert bool(torch.isnan(bg["rec"][:K]).all())
    taken = []
    for rep in range(2):
        if rep == 1:        # new weights between the two replays: stream-ordered, nothing allocated, no re-capture
            ph_g.update(w_b, DEV, int(torch.cuda.current_stream().cuda_stream))
            ph_e.update(policy_b.pack())                  # host pointers on the eager side
        g.replay()
        call(eager, ph_e, be, 0)
        torch.cuda.synchronize()
        for k in bg:
            assert torch.equal(bg[k].view(torch.int32), be[k].view(torch.int32)), (rep, k)
        if sampled:
            assert ph_g.noise_step == ph_e.noise_step == (rep + 1) * K
        assert not bool(torch.isnan(be["rec"][:K, :, :cfg.obs_dim + 4]).any())
        taken.append(be["act"].cpu().numpy())
    assert not np.array_equal(taken[0], taken[1])
    assert same_state(device_state(graphed, cfg), device_state(eager, cfg)) and graphed.stats() == eager.stats()
    assert eager.stats()["env_steps"] == 2 * K * n and eager.global_step == 2 * K
    for h in (ph_e, ph_g):
        h.close()
    eager.close()
    graphed.close()


# Handle classes (tests/test_gpu_packed_record.py::test_packed_kernel_occupancy_matches_the_design) whose packed policy kernel
# may hold more scratch than its salp_vec_rollout_policy twin: (foods, other tank) -> bytes allowed, read from the code-object
# metadata of the cross-compiled library (profiles/r16/policy_packed_kernel_resources.txt).  None needs one: every forced-breathing
# unpredicated deterministic kernel holds 0 B, as its twin does.
SCRATCH_ALLOWANCE = {}


@pytest.mark.parametrize("foods,tank", [(1, False), (3, False), (5, False), (8, False), (12, False), (16, False),
                                        (5, True), (8, True), (1, True), (12, True), (16, True)])
def test_resources_are_those_of_the_rollout_policy_kernel(foods, tank):
    cfg = pc.make_cfg(dict(preset="sac_gail", num_food_items=foods, **(dict(width=801) if tank else {})))
    n, HR = 2048, 4
    dev = SalpLib(cfg, n, device_id=0, seed=3)
    ph = dev.policy_create(dc.random_policy(cfg.obs_dim, cfg.act_dim, (64, 64), "tanh", 1, 1.0, 1.0))
    obs, rew = np.empty((HR, n, cfg.obs_dim), np.float32), np.empty((HR, n), np.float32)
    term, trunc = np.empty((HR, n), np.uint8), np.empty((HR, n), np.uint8)
    dev.rollout_policy(ph, HR, obs, rew, term, trunc, None, 0)
    twin_ll, twin = dev.last_launch(), dev.last_kernel_resources()
    assert twin_ll["full_signature"] == 1 and twin_ll["actions_in_kernel"] == 2
    for with_final in (False, True):
        rec = np.empty((HR, n, dev.record_width(with_final)), np.float32)
        dev.rollout_policy_packed(ph, HR, rec, None, FIN if with_final else 0)
        ll, res = dev.last_launch(), dev.last_kernel_resources()
        print(foods, tank, with_final, res, "rollout_policy:", twin)
        assert ll["full_signature"] == 3 and ll["actions_in_kernel"] == 2 and ll["literal_constants"] == (0 if tank else 1)
        assert ll["food_slots"] == twin_ll["food_slots"] and ll["envs_unpredicated"] == n
        assert res["scratch_bytes"] <= twin["scratch_bytes"] + SCRATCH_ALLOWANCE.get((foods, tank), 0), (res, twin)
        assert res["workgroups_per_cu"] >= twin["workgroups_per_cu"], (res, twin)
    ph.close()
    dev.close()


def test_vector_env_surface():
    import torch
    from underwater_swimmer_rl_amd import GaussianPolicy, SalpVectorEnv, pursuit_policy
    from sampled_cases import gaussian_policy
    n, HV = 256, 32
    env = SalpVectorEnv("single_food", num_envs=n, seed=3, max_steps_without_food=20)
    obs0, _ = env.reset()
    obs0 = obs0.clone()
    p = pursuit_policy(3.0)
    out = env.rollout_policy_packed(p, HV)
    assert set(out) == {"record", "actions"} and tuple(out["record"].shape) == (HV, n, 52) and tuple(out["actions"].shape) == (HV, n, 1)
    u = unpack_record(out["record"], env.obs_dim)
    for k in ("obs", "reward", "terminated", "truncated", "collision", "food_collected", "steps_since_food", "final_observation"):
        assert u[k].untyped_storage().data_ptr() == out["record"].untyped_storage().data_ptr(), k
    assert u["terminated"].dtype == torch.bool and u["food_collected"].dtype == torch.int32
    seen = torch.cat([obs0[None], u["obs"][:-1]])
    assert torch.equal(out["actions"], (-3.0 * seen[..., 13:14]).clamp(-1.0, 1.0))      # one product, exact in fp32
    assert bool(u["truncated"].any()) and env.global_step == HV
    narrow = env.rollout_policy_packed(p, 4, want_final_observation=False, want_actions=False)
    assert tuple(narrow["record"].shape) == (4, n, 28) and narrow["actions"] is None
    assert unpack_record(narrow["record"], env.obs_dim)["final_observation"] is None
    mine = torch.zeros(4, n, 52, device="cuda:0")
    assert env.rollout_policy_packed(p, 4, out=mine)["record"] is mine and bool((mine[..., :24] != 0).any())
    with pytest.raises(ValueError, match="expected"):
        env.rollout_policy_packed(p, 4, want_final_observation=False, out=mine)
    with pytest.raises(ValueError, match="expected"):
        env.rollout_policy_packed(p, 5, out=mine)
    with pytest.raises(ValueError):
        env.rollout_policy_packed(p, 0)
    gp = gaussian_policy(24, 1, (32, 32), 123, 1.5, 2.0, (-1.0,))
    assert isinstance(gp, GaussianPolicy)
    handle = env.make_policy(gp)
    s = env.rollout_policy_packed(handle, 8, sample=True)
    assert set(s) == {"record", "actions", "logp"} and tuple(s["logp"].shape) == (8, n) and handle.noise_step == 8
    assert not bool(torch.isnan(s["logp"]).any())
    mean = env.rollout_policy_packed(handle, 4)
    assert "logp" not in mean and handle.noise_step == 8
    assert env.global_step == HV + 4 + 4 + 8 + 4
    env.close()


def test_collect_in_kernel_keeps_the_truncated_transitions():
    import torch
    from underwater_swimmer_rl_amd import GaussianPolicy, SalpVectorEnv
    from underwater_swimmer_rl_amd import sac
    n, HC = 256, 64
    torch.manual_seed(0)
    agent = sac.SAC(24, 1, sac.SACConfig(hidden_sizes=(32, 32)), device="cuda:0")
    with torch.no_grad():           # a lively mean head, a quiet log-std head
        agent.actor.mu.weight.mul_(4.0)
        agent.actor.log_std.bias.fill_(-1.0)
    pol = GaussianPolicy.from_actor(agent.actor)

    def fresh():
        env = SalpVectorEnv("sac_gail", num_envs=n, seed=5, max_steps_without_food=40)      # a budget of 40 < HC: truncations are certain
        env.reset()
        return env
    # the launch that collect_in_kernel must have made: a twin env, the same seed and noise step
    twin = fresh()
    first = twin.observe().clone()
    out = twin.rollout_policy_packed(twin.make_policy(pol), HC, sample=True)
    want = [t.clone() for t in transitions(first, out["record"], out["actions"], twin.obs_dim)]
    u = unpack_record(out["record"], twin.obs_dim)
    n_trunc = int(u["truncated"].sum())
    assert n_trunc >= 1, n_trunc
    env = fresh()
    buf = sac.DeviceReplayBuffer(HC * n, 24, 1, torch.device("cuda:0"))
    handle = sac.collect_in_kernel(env, agent, buf, HC, keep_truncated=True)
    assert buf.size == HC * n and handle.noise_step == HC and env.global_step == HC
    assert env._lib.last_launch()["full_signature"] == 3 and env._lib.last_launch()["actions_in_kernel"] == 3
    w_obs, w_act, w_rew, w_next, w_term = want
    assert torch.equal(buf.obs, w_obs) and torch.equal(buf.act, w_act) and torch.equal(buf.rew, w_rew)
    assert torch.equal(buf.next_obs, w_next) and torch.equal(buf.term, w_term.float())
    assert not bool(torch.isnan(buf.next_obs).any())
    # truncated transitions are stored, with the terminal row and not the next episode's first one (obs[t] of the record)
    trunc = u["truncated"].reshape(-1)
    rec_obs = u["obs"].reshape(HC * n, -1)
    moved = (buf.next_obs[trunc] != rec_obs[trunc]).any(dim=1)
    assert bool(moved.any()) and bool((buf.term[trunc & ~u["terminated"].reshape(-1)] == 0).all())
    assert torch.equal(buf.next_obs[trunc], u["final_observation"].reshape(HC * n, -1)[trunc])
    # the default is what it was: the truncated rows are left out
    env2 = fresh()
    buf2 = sac.DeviceReplayBuffer(HC * n, 24, 1, torch.device("cuda:0"))
    sac.collect_in_kernel(env2, agent, buf2, HC)
    assert env2._lib.last_launch()["full_signature"] == 1
    assert buf2.size == HC * n - n_trunc
    keep = ~trunc
    assert torch.equal(buf2.obs[:buf2.size], w_obs[keep]) and torch.equal(buf2.act[:buf2.size], w_act[keep])
    # the handle comes back for reuse
    again = sac.collect_in_kernel(env, agent, buf, 4, handle=handle, keep_truncated=True)
    assert again is handle and handle.noise_step == HC + 4 and env.global_step == HC + 4
    for e in (env, env2, twin):
        e.close()
