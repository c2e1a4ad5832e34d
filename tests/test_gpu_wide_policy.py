"""The wide in-kernel policy (include/salp_vec_policy_wide.h, csrc/salp_policy_wide.h) on the GPU.  Run with `pytest -m gpu`.

n = 128 (two full wavefronts; 100 where the predicated launch is meant), H = 6 compared steps behind one call of horizon 1
(only a state that a step left fixes the bits of the row the first action sees, tests/test_gpu_policy_matrix.py).  The
yardstick is the host twin's fmaf restatement from the public layout (tests/wide_policy_host.cpp), held bit for bit to the
oracle's where both exist (tests/test_wide_policy_host.py).  Every run asserts salp_vec_last_launch_policy_wide == 1.

  * the shape matrix: `clip` actions EQUAL the restatement's on the row the kernel itself wrote; `tanh` actions within
    tanhf's 5 ulp and the two final roundings of the restatement's own u (`policy_matrix.tanh_stage_bound`); all within
    `MLPPolicy.error_bound`; a twin salp_vec_rollout on the actions reproduces obs, reward and flags bit for bit;
  * both schemes, same bits, on the shapes both accept — rollout_policy and rollout_policy_packed, Gaussian with logp;
  * sampled: the restatement's heads plus `GaussianPolicy.sampling_stage` (the rule of tests/gaussian_matrix.py);
  * the other signatures on (256, 256): evaluate_policy, evaluate_navigation, the packed record, policy_update, the SAC
    collector; and the refusals, with nothing launched."""
import functools

import numpy as np
import pytest

import gaussian_matrix as gm
import policy_cases as dc
import policy_matrix as pm
import wide_policy_cases as wc
import wide_policy_host_lib as wl
from gpu_support import device_state, host_outputs, run_policy, run_sampled, started
from support import bits, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpError, SalpLib
from underwater_swimmer_rl_amd import policy as pol
from underwater_swimmer_rl_amd.policy import GaussianPolicy, MLPPolicy, evaluation_views, summarize_rollout
from underwater_swimmer_rl_amd.records import unpack_record

pytestmark = pytest.mark.gpu

pc = dc.pc                      # tests/parity_cases.py, as tests/policy_cases.py uses it: configurations and start states
H = 6
KEY = pc.ENV_SEED
RT_CASE = "other_tank_F1"       # one food, constants read at run time
OUT_GAIN = 0.5                  # the output layer's gain: keeps a good share of the clip actions off the clamp


def _matrix():
    rows = []
    for case in ("single_food", "free_breathing"):
        for i, hidden in enumerate(wc.GPU_SHAPES):
            rows.append((case, 128, hidden, ("tanh", "clip")[(i + (case != "single_food")) % 2], 1))
    rows += [(RT_CASE, 128, (256, 256), "clip", 1), (RT_CASE, 128, (96, 160), "tanh", 1), ("single_food", 100, (256, 256), "clip", 1),
             ("single_food", 128, (96, 160), "clip", 2)]
    return rows


MATRIX = _matrix()
IDS = [f"{c}-{'x'.join(map(str, h))}-{o}-n{n}" + (f"-P{P}" if P > 1 else "") for c, n, h, o, P in MATRIX]


def entry_policy(case, hidden, out, P, generation=0):
    A = pc.case_cfg(case).act_dim
    ps = [wc.dense(hidden, A, out, seed=7000 + 1000 * k + 100000 * generation, out_gain=OUT_GAIN) for k in range(P)]
    return ps[0] if P == 1 else MLPPolicy.stack(ps)


@functools.lru_cache(maxsize=None)
def start(case, n):
    cfg = pc.case_cfg(case)
    orc, f64, i32 = pc.start_oracle(cfg, n, KEY)
    orc.close()
    f64.setflags(write=False)
    i32.setflags(write=False)
    return cfg, f64, i32


def wide_ran(dev):
    assert dev.last_launch_policy_wide() == 1
    ll = dev.last_launch()
    assert ll["food_slots"] == 1 and ll["observed_capacity"] == 3 and ll["actions_in_kernel"] in (2, 3)
    return ll


@functools.lru_cache(maxsize=None)
def device_run(case, n, hidden, out, P):
    cfg, f64, i32 = start(case, n)
    policy = entry_policy(case, hidden, out, P)
    dev = started(cfg, n, f64, i32)
    assert dev.last_launch_policy_wide() == 0
    ph = dev.policy_create(policy)
    assert dev.policy_words(policy) == policy.words == ph.words
    first = run_policy(dev, ph, cfg, 1)
    wide_ran(dev)
    o = run_policy(dev, ph, cfg, H)
    ll, res = wide_ran(dev), dev.last_kernel_resources()
    state, stats = device_state(dev, cfg), dev.stats()
    ph.close()
    dev.close()
    for a in (*first.values(), *o.values(), *state):
        a.setflags(write=False)
    return dict(cfg=cfg, f64=f64, i32=i32, policy=policy, first=first, out=o, launch=ll, res=res, state=state, stats=stats)


def same_outputs(a, b, keys=("actions", "obs", "reward")):
    for k in keys:
        if not np.array_equal(bits(a[k]), bits(b[k])):
            same = bits(a[k]) == bits(b[k])
            return f"{k}: {int((~same).sum())} words differ, first at {np.unravel_index(np.argmin(same), same.shape)}"
    for k in ("terminated", "truncated"):
        if not np.array_equal(a[k], b[k]):
            return k
    return ""


def assert_actions_are_the_policy(label, policy, seen, actions):
    """tests/test_gpu_policy_matrix.py's rule with the twin's restatement (widths up to 256) in the oracle's place."""
    assert not np.isnan(actions).any()
    u, a = wl.policy_forward(policy, seen)
    want, bound = policy.reference(seen), policy.error_bound(seen)
    err = np.abs(actions.astype(np.float64) - want)
    print(f"{label}: |action - float64 reference| / error_bound <= {(err / bound).max():.3g} (error {err.max():.3g})")
    if policy.out == "clip":
        same = actions == a
        inside = (np.abs(u) < 1.0).mean()
        print(f"{label}: clip chain: {int((~same).sum())} of {same.size} values differ from the restatement; {inside:.2f} of the sums inside the clamp")
        assert same.all(), f"{int((~same).sum())} actions are not the restatement's, first at {np.unravel_index(np.argmin(same), same.shape)}"
        assert inside >= 0.25, "the check is blind: the clamp hides the sums"
    else:
        exact, tb = pm.tanh_stage_bound(policy, u)
        terr = np.abs(actions.astype(np.float64) - exact)
        print(f"{label}: tanh stage: |action - (tanh(u) scale + shift)| / bound <= {(terr / tb).max():.3g}")
        assert (terr <= tb).all(), f"{int((terr > tb).sum())} actions outside the tanh-stage bound, worst ratio {(terr / tb).max()}"
        assert (np.abs(u) < 2.0).mean() >= 0.25, "the check is blind: tanh is saturated"
    assert (err <= bound).all(), f"{int((err > bound).sum())} actions outside the forward bound, worst ratio {(err / bound).max()}"


# ------------------------------------------------------------------------------------------------ the shape matrix
@pytest.mark.parametrize("case, n, hidden, out, P", MATRIX, ids=IDS)
def test_every_action_is_the_restatement_on_the_row_before_it(case, n, hidden, out, P):
    r = device_run(case, n, hidden, out, P)
    ll = r["launch"]
    print(ll, r["res"])
    assert ll["literal_constants"] == (0 if case == RT_CASE else 1) and ll["full_signature"] == 1 and ll["actions_in_kernel"] == 2
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == ((n, 0) if n % 64 == 0 else (0, n))
    assert r["res"]["scratch_bytes"] == 0
    seen = np.concatenate([r["first"]["obs"], r["out"]["obs"][:-1]])
    assert_actions_are_the_policy(IDS[MATRIX.index((case, n, hidden, out, P))], r["policy"], seen, r["out"]["actions"])
    if P > 1:       # the two policies are told apart: the second half's actions are not the first policy's
        _, a0 = wl.policy_forward(MLPPolicy.stack([entry_policy(case, hidden, out, 1)] * P), seen)
        assert (a0[:, n // P:] != r["out"]["actions"][:, n // P:]).mean() > 0.5


@pytest.mark.parametrize("case, n, hidden, out, P", MATRIX, ids=IDS)
def test_twin_rollout_on_the_actions_taken(case, n, hidden, out, P):
    r = device_run(case, n, hidden, out, P)
    cfg = r["cfg"]
    twin = started(cfg, n, r["f64"], r["i32"])
    for part, steps in ((r["first"], 1), (r["out"], H)):
        t = host_outputs(cfg, steps, n)
        twin.rollout(np.array(part["actions"]), steps, t["obs"], t["reward"], t["terminated"], t["truncated"], None, None, 0)
        t["actions"] = part["actions"]
        assert same_outputs(part, t) == ""
    assert twin.last_launch_policy_wide() == 0 and twin.last_launch()["actions_in_kernel"] == 0
    assert same_state(r["state"], device_state(twin, cfg)) and twin.stats() == r["stats"]
    twin.close()


# ------------------------------------------------------------------------------------------------ both schemes, same bits
BOTH = [("single_food", (32, 32)), ("free_breathing", (64, 64)), ("free_breathing", (32, 64)), ("single_food", (64,))]


@pytest.mark.parametrize("case, hidden", BOTH)
def test_both_schemes_give_the_same_bits(case, hidden):
    cfg, f64, i32 = start(case, 128)
    wide = wc.dense_gauss(hidden, cfg.act_dim, out_gain=OUT_GAIN)
    narrow = wc.narrow_twin(wide)
    got = {}
    for name, p in (("wide", wide), ("narrow", narrow)):
        dev = started(cfg, 128, f64, i32)
        ph = dev.policy_create(p)
        mean = run_policy(dev, ph, cfg, H)
        assert dev.last_launch_policy_wide() == (name == "wide")
        sampled = run_sampled(dev, ph, cfg, H)
        assert dev.last_launch_policy_wide() == (name == "wide") and dev.last_launch()["actions_in_kernel"] == 3 and ph.noise_step == H
        w = dev.record_width(True)
        rec, act, logp = np.full((H, 128, w), np.nan, np.float32), np.empty((H, 128, cfg.act_dim), np.float32), np.empty((H, 128), np.float32)
        dev.rollout_policy_packed_sampled(ph, H, rec, act, logp, _capi.REC_FINAL_OBS)
        assert dev.last_launch_policy_wide() == (name == "wide") and dev.last_launch()["full_signature"] == 3 and ph.noise_step == 2 * H
        rec2, act2 = np.full((H, 128, w), np.nan, np.float32), np.empty((H, 128, cfg.act_dim), np.float32)
        dev.rollout_policy_packed(ph, H, rec2, act2, _capi.REC_FINAL_OBS)
        got[name] = dict(mean=mean, sampled=sampled, rec=rec, act=act, logp=logp, rec2=rec2, act2=act2, state=device_state(dev, cfg))
        ph.close()
        dev.close()
    a, b = got["wide"], got["narrow"]
    assert same_outputs(a["mean"], b["mean"]) == ""
    assert same_outputs(a["sampled"], b["sampled"], ("actions", "obs", "reward", "logp")) == ""
    for k in ("rec", "act", "logp", "rec2", "act2"):
        assert np.array_equal(bits(a[k]), bits(b[k]), ), k
    assert same_state(a["state"], b["state"])
    assert len(np.unique(a["logp"])) > H * 64 and not np.isnan(a["logp"]).any()


# ------------------------------------------------------------------------------------------------ sampled
def assert_is_the_stage(label, policy, seen, out, z):
    """`gaussian_matrix.assert_is_the_stage` with the twin's restatement of the two heads."""
    assert not np.isnan(out["actions"]).any() and not np.isnan(out["logp"]).any()
    m, r = wl.policy_forward_gaussian(policy, seen)
    s = gm.stage(policy, m, r, z)
    a, lp = out["actions"].astype(np.float64), out["logp"].astype(np.float64)
    sa, sl = np.abs(a - s["a"]) / s["ea"], np.abs(lp - s["lp"]) / s["el"]
    (wa, wlp), (ea, el) = policy.reference(seen, z), policy.error_bound(seen, z)
    fa, fl = np.abs(a - wa) / ea, np.abs(lp - wlp) / el
    print(f"{label}: error / stage bound: action {sa.max():.4f}, logp {sl.max():.4f}; error / error_bound: action {fa.max():.4f}, logp {fl.max():.4f}")
    assert (sa <= 1.0).all() and (sl <= 1.0).all(), f"{label}: outside the stage bound, worst ratios {sa.max()}, {sl.max()}"
    assert (fa <= 1.0).all() and (fl <= 1.0).all(), f"{label}: outside error_bound, worst ratios {fa.max()}, {fl.max()}"
    assert (np.abs(m) < 2.0).mean() >= gm.NOT_BLIND


@pytest.mark.parametrize("case, hidden", [("single_food", (256, 256)), ("free_breathing", (256, 256)), ("single_food", (96,)), ("free_breathing", (96,))])
def test_sampled_actions_and_logp_are_the_stage_of_the_restated_heads(case, hidden):
    cfg, f64, i32 = start(case, 128)
    policy = wc.dense_gauss(hidden, cfg.act_dim, out_gain=OUT_GAIN)
    dev = started(cfg, 128, f64, i32)
    ph = dev.policy_create(policy)
    assert ph.gaussian and ph.noise_step == 0
    first = run_sampled(dev, ph, cfg, 1)
    out = run_sampled(dev, ph, cfg, H)
    ll = wide_ran(dev)
    assert ll["actions_in_kernel"] == 3 and ph.noise_step == 1 + H and dev.last_kernel_resources()["scratch_bytes"] == 0
    seen = np.concatenate([first["obs"], out["obs"][:-1]])
    assert_is_the_stage(f"{case}-{hidden}", policy, seen, out, gm.noise(policy, 128, 1, H, KEY))
    # sample=False runs the mean: the plain wide policy, bit for bit, and the noise step stays
    state = device_state(dev, cfg)
    mean = run_policy(dev, ph, cfg, H)
    assert ph.noise_step == 1 + H and dev.last_launch_policy_wide() == 1
    ph.close()
    dev.close()
    plain = started(cfg, 128, *state)
    pp = plain.policy_create(policy.mean_policy())
    assert same_outputs(run_policy(plain, pp, cfg, H), mean) == ""
    pp.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ the other signatures, (256, 256)
BIG = ("single_food", 128, (256, 256), "clip", 1)


def test_evaluate_gives_the_summary_of_the_rollout_and_accumulates():
    r = device_run(*BIG)
    cfg, n, o = r["cfg"], 128, r["out"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    rec = np.full((n, _capi.EVAL_WORDS), 0x5A5A5A5A, np.int32)
    dev.evaluate_policy(ph, 1, rec, 0)
    dev.evaluate_policy(ph, H // 2, rec, 0)
    assert wide_ran(dev)["full_signature"] == 4 and dev.last_kernel_resources()["scratch_bytes"] == 0
    half = summarize_rollout(o["reward"][:H // 2], o["terminated"][:H // 2], o["truncated"][:H // 2])
    evaluation_views(half)["food"][:] = evaluation_views(rec)["food"]
    assert np.array_equal(rec, half)
    dev.evaluate_policy(ph, H - H // 2, rec, _capi.EVAL_ACCUMULATE)
    want = summarize_rollout(o["reward"], o["terminated"], o["truncated"])
    evaluation_views(want)["food"][:] = evaluation_views(rec)["food"]
    assert np.array_equal(rec, want)
    assert same_state(device_state(dev, cfg), r["state"]) and dev.stats() == r["stats"] and dev.global_step == 1 + H
    ph.close()
    dev.close()


def test_packed_records_with_terminal_observations_equal_the_unpacked_outputs():
    r = device_run(*BIG)
    cfg, n, o = r["cfg"], 128, r["out"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    run_policy(dev, ph, cfg, 1)
    rec, act = np.full((H, n, dev.record_width(True)), np.nan, np.float32), np.empty((H, n, cfg.act_dim), np.float32)
    dev.rollout_policy_packed(ph, H, rec, act, _capi.REC_FINAL_OBS)
    ll = wide_ran(dev)
    assert ll["full_signature"] == 3 and ll["actions_in_kernel"] == 2 and dev.last_kernel_resources()["scratch_bytes"] == 0
    f = unpack_record(rec, cfg.obs_dim)
    assert np.array_equal(bits(act), bits(o["actions"])) and np.array_equal(bits(np.ascontiguousarray(f["obs"])), bits(o["obs"]))
    assert np.array_equal(bits(np.ascontiguousarray(f["reward"])), bits(o["reward"]))
    assert np.array_equal(f["terminated"], o["terminated"].astype(bool)) and np.array_equal(f["truncated"], o["truncated"].astype(bool))
    done = (o["terminated"] | o["truncated"]).astype(bool)
    assert done.any() and np.array_equal(np.isnan(f["final_observation"][..., 0]), ~done)
    # the terminal rows are what salp_vec_rollout returns on the same actions
    twin = started(cfg, n, r["f64"], r["i32"])
    t1, t = host_outputs(cfg, 1, n), host_outputs(cfg, H, n)
    twin.rollout(np.array(r["first"]["actions"]), 1, t1["obs"], t1["reward"], t1["terminated"], t1["truncated"], None, None, 0)
    fin = np.full((H, n, cfg.obs_dim), np.nan, np.float32)
    twin.rollout(np.array(o["actions"]), H, t["obs"], t["reward"], t["terminated"], t["truncated"], fin, None, 0)
    assert np.array_equal(bits(np.ascontiguousarray(f["final_observation"])[done]), bits(fin[done]))
    assert same_state(device_state(dev, cfg), r["state"])
    twin.close()
    ph.close()
    dev.close()


def test_update_equals_a_fresh_policy():
    r = device_run(*BIG)
    cfg, n = r["cfg"], 128
    policy_b = entry_policy(BIG[0], BIG[2], BIG[3], 1, generation=1)
    outs = []
    for updated in (True, False):
        dev = started(cfg, n, *r["state"])
        ph = dev.policy_create(r["policy"] if updated else policy_b)
        if updated:
            ph.update(policy_b.pack())
        outs.append(run_policy(dev, ph, cfg, H))
        wide_ran(dev)
        ph.close()
        dev.close()
    assert same_outputs(*outs) == ""
    seen = np.concatenate([r["out"]["obs"][-1:], outs[0]["obs"][:-1]])
    assert_actions_are_the_policy("updated", policy_b, seen, outs[0]["actions"])
    _, a_old = wl.policy_forward(r["policy"], seen)
    assert (a_old != outs[0]["actions"]).mean() > 0.5


def test_navigation_records_equal_a_stepped_twin():
    import test_gpu_navigation_kernel as nk
    n, HN = 128, 200
    cfg, f64, i32, line, radius = nk.snapshot("centre", n, 800)
    policy = wc.dense((256, 256), 1, "tanh", seed=7100, out_gain=OUT_GAIN)
    dev = started(cfg, n, f64, i32, seed=nk.SEED)
    ph = dev.policy_create(policy)
    F, I = [f64.copy()], [i32.copy()]
    for t in range(HN):
        run_policy(dev, ph, cfg, 1)
        s = device_state(dev, cfg)
        F.append(s[0]); I.append(s[1])
    stats = dev.stats()
    ph.close()
    dev.close()
    F, I = np.stack(F), np.stack(I)
    pos = np.ascontiguousarray(np.stack([F[:, _capi.F_X], F[:, _capi.F_Y]], axis=2))
    col, cap = nk.collisions_of(cfg, F[1:]), np.diff(I[:, _capi.I_FOOD_COLLECTED], axis=0) > 0
    assert int(col.sum()) == stats["collisions"] and int(cap.sum()) == stats["food_collected"]
    # the trial lines of THIS test (the state keeps the snapshot's food): 60 % of the envs get as goal a point they pass
    # later in the run, the others one they never come near, so that envs stop at many different steps and some never do
    rng = np.random.default_rng(5)
    goal = pos[rng.integers(HN // 4, HN, n), np.arange(n)].copy()
    goal[rng.random(n) < 0.4] += 1000.0
    line = np.ascontiguousarray(np.concatenate([line[:, :2], goal], axis=1))
    radius = 0.25
    want = pol.navigation_record(pos, None, line, radius, collided=col, captured=cap)
    reached = (pol.navigation_views(want)["status"] & pol.NAV_REACHED) != 0
    assert 0.2 <= reached.mean() <= 0.8 and len(np.unique(pol.navigation_views(want)["steps"])) >= 8
    dev = started(cfg, n, f64, i32, seed=nk.SEED)
    ph = dev.policy_create(policy)
    rec, track = nk.junk(n), np.full((HN, n, 2), np.nan)
    dev.evaluate_navigation(ph, HN, line, radius, rec, track, 0)
    assert wide_ran(dev)["full_signature"] == 5 and dev.last_kernel_resources()["scratch_bytes"] == 0
    assert nk.record_diff(rec, want) == "" and np.array_equal(rec, want)
    stop = pol.navigation_views(want)["steps"].astype(np.int64)
    tt = np.minimum(np.arange(1, HN + 1)[:, None], stop[None, :])
    assert np.array_equal(track.view(np.int64), pos[tt, np.arange(n)[None, :]].view(np.int64))
    ph.close()
    dev.close()


def test_collect_in_kernel_with_the_default_size_actor():
    import torch
    from underwater_swimmer_rl_amd import SalpVectorEnv, sac
    n, HC = 128, H
    torch.manual_seed(0)
    agent = sac.SAC(24, 1, sac.SACConfig(), device="cuda:0")
    assert tuple(agent.cfg.hidden_sizes) == (256, 256)
    with torch.no_grad():
        agent.actor.log_std.bias.fill_(-1.0)
    policy = GaussianPolicy.from_actor(agent.actor, wide=True)

    def fresh():
        env = SalpVectorEnv("single_food", num_envs=n, seed=5, max_steps_without_food=3)
        env.reset()
        return env
    twin = fresh()
    first = twin.observe().clone()
    out = twin.rollout_policy(twin.make_policy(policy), HC, sample=True)
    assert twin._lib.last_launch_policy_wide() == 1
    seen = torch.cat([first[None], out["obs"][:-1]])
    env = fresh()
    buf = sac.DeviceReplayBuffer(HC * n, 24, 1, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="64"):
        sac.collect_in_kernel(env, agent, buf, HC)
    assert buf.size == 0 and env.global_step == 0
    handle = sac.collect_in_kernel(env, agent, buf, HC, wide=True)
    assert env._lib.last_launch_policy_wide() == 1 and handle.noise_step == HC
    keep = (out["truncated"] == 0).reshape(-1)
    assert int((~keep).sum()) >= 1 and buf.size == int(keep.sum())
    flat = lambda t: t.reshape((HC * n,) + tuple(t.shape[2:]))[keep]
    k = buf.size
    assert torch.equal(buf.obs[:k], flat(seen)) and torch.equal(buf.next_obs[:k], flat(out["obs"]))
    assert torch.equal(buf.act[:k], flat(out["actions"])) and torch.equal(buf.rew[:k], flat(out["reward"]))
    with pytest.raises(ValueError, match="wide"):
        sac.collect_in_kernel(env, sac.SAC(24, 1, sac.SACConfig(hidden_sizes=(48, 48)), device="cuda:0"), buf, HC, wide=True)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ refusals
def untouched(dev, cfg, before):
    return same_state(device_state(dev, cfg), before[0]) and dev.global_step == before[1] and dev.stats() == before[2] and dev.last_launch_policy_wide() == 0


@pytest.mark.parametrize("case, message", [("sac_gail_F12", "wide policies need a handle with num_food_items <= 1"),
                                           ("K2_generic", "policies need a handle with max_observed_food == 3")])
def test_create_is_refused_on_other_handle_classes(case, message):
    cfg = pc.case_cfg(case)
    dev = SalpLib(cfg, 128, device_id=0, seed=KEY)
    before = (device_state(dev, cfg), dev.global_step, dev.stats())
    p = wc.dense((64, 64), cfg.act_dim)
    for q in (p, wc.dense_gauss((64, 64), cfg.act_dim)):
        with pytest.raises(SalpError, match=message):
            dev.policy_create(q)
        with pytest.raises(SalpError, match=message):
            dev.policy_words(q)
    assert untouched(dev, cfg, before) and dev._policies == []
    dev.close()


def test_a_wide_policy_of_another_handle_is_refused():
    cfg, f64, i32 = start("single_food", 128)
    a, b = started(cfg, 128, f64, i32), started(cfg, 128, f64, i32)
    ph = a.policy_create(wc.dense_gauss((256, 256), 1))
    before = (device_state(b, cfg), b.global_step, b.stats())
    o = host_outputs(cfg, H, 128, logp=True)
    rec = np.zeros((128, _capi.EVAL_WORDS), np.int32)
    calls = [lambda: b.rollout_policy(ph, H, o["obs"], o["reward"], o["terminated"], o["truncated"], o["actions"], 0),
             lambda: b.rollout_policy_sampled(ph, H, o["obs"], o["reward"], o["terminated"], o["truncated"], o["actions"], o["logp"], 0),
             lambda: b.evaluate_policy(ph, H, rec, 0), lambda: b.evaluate_policy_sampled(ph, H, rec, 0)]
    for call in calls:
        with pytest.raises(SalpError, match="the policy belongs to another handle"):
            call()
    assert untouched(b, cfg, before) and ph.noise_step == 0 and np.isnan(o["obs"]).all()
    ph.close()
    a.close()
    b.close()
