"""The in-kernel Gaussian policy over the shape x kernel matrix of tests/gaussian_matrix.py on the GPU (its CPU guard:
tests/test_gaussian_matrix.py).  Run with `pytest -m gpu`.

Per entry, from the injected start state and behind one call of horizon 1 (only a state that a step left fixes the bits of
the row the first action sees, tests/test_gpu_policy_matrix.py): every action and log-probability that
salp_vec_rollout_policy_sampled returned within the STAGE bound of `GaussianPolicy.sampling_stage(m, r, z)` — m, r the C
restatement of the two heads (`oracle_lib.policy_forward_gaussian`) on the rows the kernel itself wrote, z the definition's
noise of (global env index, noise step) — and within `error_bound` of the float64 reference as before; the same handle
through the deterministic entry point against the restated mean head; a twin handle running salp_vec_rollout on the actions
taken (bit for bit, draw counters included); salp_vec_evaluate_policy_sampled against `summarize_rollout`; policy_update
against a fresh policy.  Once: mutant weights uploaded to the unchanged kernel leave the bound; handles at
env_index_base = 2^32 + 320 draw the noise of the global index, and a handle of 256 envs equals two of 128; the noise step
wraps at 2^32."""
import functools

import numpy as np
import pytest

import gaussian_matrix as gm
import oracle_lib as ol
import policy_matrix as pm
from gpu_support import assert_parity, assert_state_parity, device_state, host_outputs, run_policy, run_sampled, started
from support import bits, same_state
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd.policy import evaluation_views, summarize_rollout

pytestmark = pytest.mark.gpu

H, HU = gm.H, gm.UPDATE_STEPS
NAMES = list(gm.ENTRIES)
FLOAT_KEYS, FLAG_KEYS = ("actions", "logp", "obs", "reward"), ("terminated", "truncated")


def same_outputs(a, b, keys=FLOAT_KEYS):
    """'' when two sets of per-step outputs hold the same bits, else the first key that differs."""
    for k in keys:
        if not np.array_equal(bits(a[k]), bits(b[k])):
            same = bits(a[k]) == bits(b[k])
            return f"{k}: {int((~same).sum())} words differ, first at {np.unravel_index(np.argmin(same), same.shape)}"
    for k in FLAG_KEYS:
        if not np.array_equal(a[k], b[k]):
            return k
    return ""


def first_step_then_run(dev, ph, cfg, horizon=H):
    """One call of horizon 1 from the injected state (noise step 0), then the steps every comparison is about."""
    first = run_sampled(dev, ph, cfg, 1)
    return first, run_sampled(dev, ph, cfg, horizon)


@functools.lru_cache(maxsize=None)
def device_run(name, base=0):
    """One entry on the GPU, computed once, shared, read-only: one sampled step and then H of them under the entry's policy
    (noise steps 0 and 1 .. H), then — after policy_update to the second weight set — HU more."""
    e, cfg, f64, i32 = gm.start_snapshot(name, base)
    policy, policy_b, n = gm.entry_policy(name), gm.entry_policy(name, 1), e["n"]
    assert policy_b.words == policy.words and policy_b.hidden == policy.hidden
    dev = started(cfg, n, f64, i32, base=base)
    obs0 = np.empty((n, cfg.obs_dim), np.float32)
    dev.observe(obs0, 0)
    ph = dev.policy_create(policy)
    assert ph.gaussian and dev.policy_words(policy) == policy.words == ph.words and ph.noise_step == 0
    first, out = first_step_then_run(dev, ph, cfg)
    launch, res = dev.last_launch(), dev.last_kernel_resources()
    state, stats = device_state(dev, cfg), dev.stats()
    assert dev.global_step == 1 + H and ph.noise_step == 1 + H
    ph.update(policy_b.pack())
    assert ph.noise_step == 1 + H
    out_b = run_sampled(dev, ph, cfg, HU)
    state_b = device_state(dev, cfg)
    ph.close()
    dev.close()
    seen = np.concatenate([first["obs"], out["obs"][:-1]])          # act[0] <- the row that call wrote; act[t + 1] <- obs[t]
    for a in (obs0, seen, *first.values(), *out.values(), *out_b.values(), *state, *state_b):
        a.setflags(write=False)
    return dict(e=e, cfg=cfg, policy=policy, policy_b=policy_b, f64=f64, i32=i32, obs0=obs0, first=first, out=out, seen=seen,
                launch=launch, res=res, state=state, stats=stats, out_b=out_b, state_b=state_b, base=base)


@pytest.mark.parametrize("name", NAMES)
def test_the_intended_kernel_ran(name):
    r = device_run(name)
    e, ll = r["e"], r["launch"]
    print(f"{name}: {ll} {r['res']}")
    assert (ll["food_slots"], ll["literal_constants"]) == e["kernel"] and ll["observed_capacity"] == 3
    assert ll["actions_in_kernel"] == 3 and ll["full_signature"] == 1 and ll["forced"] == int(r["cfg"].forced_breathing)
    if e["predicated"]:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (0, e["n"])
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (-1, 1)
    else:
        assert (ll["envs_unpredicated"], ll["envs_predicated"]) == (e["n"], 0)
        assert (ll["signature_unpredicated"], ll["signature_predicated"]) == (1, -1)


@pytest.mark.parametrize("name", NAMES)
def test_every_action_and_logp_is_the_sampling_stage_of_the_restated_heads(name):
    r = device_run(name)
    policy, first, out, n = r["policy"], r["first"], r["out"], r["e"]["n"]
    # the call of horizon 1 from the injected state: salp_vec_observe's row up to the last bits of one column; noise step 0
    z0 = gm.noise(policy, n, 0, 1, gm.KEY)
    (wa, wl), (ea, el) = policy.reference(r["obs0"][None], z0), policy.error_bound(r["obs0"][None], z0)
    assert (np.abs(first["actions"] - wa) <= ea).all() and (np.abs(first["logp"] - wl) <= el).all()
    assert np.isfinite(first["obs"]).all() and np.abs(first["obs"][0] - r["obs0"]).max() > 0        # it is a step: the row moved on
    ratios = gm.assert_is_the_stage(name, policy, r["seen"], out, gm.noise(policy, n, 1, H, gm.KEY))
    print(f"RATIO {name} slots={r['e']['kernel'][0]} literal={r['e']['kernel'][1]} " + " ".join(f"{v:.4f}" for v in ratios))
    # the run is not a quiet one: episodes end in it, next to running ones
    ends, mixed = gm.mixed_wave_steps(out)
    assert ends >= 1 and mixed >= 1


@pytest.mark.parametrize("name", NAMES)
def test_the_deterministic_entry_point_runs_the_restated_mean_head(name):
    r = device_run(name)
    e, cfg, policy = r["e"], r["cfg"], r["policy"]
    mean = policy.mean_policy()
    dev = started(cfg, e["n"], r["f64"], r["i32"])
    ph = dev.policy_create(policy)
    first = run_policy(dev, ph, cfg, 1)
    out = run_policy(dev, ph, cfg, H)
    ll = dev.last_launch()
    assert ll["actions_in_kernel"] == 2 and (ll["food_slots"], ll["literal_constants"]) == e["kernel"] and ph.gaussian and ph.noise_step == 0
    ph.close()
    dev.close()
    seen = np.concatenate([first["obs"], out["obs"][:-1]])
    u, _ = pm.restated(mean, seen)
    m, _ = gm.restated(policy, seen)
    assert np.array_equal(bits(u), bits(m))
    exact, tb = pm.tanh_stage_bound(mean, u)
    terr = np.abs(out["actions"].astype(np.float64) - exact)
    err, bound = np.abs(out["actions"].astype(np.float64) - mean.reference(seen)), mean.error_bound(seen)
    print(f"{name}: mean path: |action - (tanh(m) scale + shift)| / bound <= {(terr / tb).max():.3g}; / error_bound <= {(err / bound).max():.3g}")
    assert (terr <= tb).all(), f"{int((terr > tb).sum())} actions outside the tanh-stage bound, worst ratio {(terr / tb).max()}"
    assert (err <= bound).all()


@pytest.mark.parametrize("name", NAMES)
def test_twin_rollout_on_the_actions_taken(name):
    """salp_vec_rollout on the actions taken: the same bits everywhere and the same draw counters — sampling consumed no env
    draw.  The handle classes that tests/gaussian_matrix.py defines itself (`EXTRA_CASES`, the two free-breathing multi-food
    classes among them) are held to the oracle as well, since no parity case runs their configurations."""
    r = device_run(name)
    e, cfg, out, n = r["e"], r["cfg"], r["out"], r["e"]["n"]
    twin = started(cfg, n, r["f64"], r["i32"])
    t1 = host_outputs(cfg, 1, n)
    twin.rollout(np.array(r["first"]["actions"]), 1, t1["obs"], t1["reward"], t1["terminated"], t1["truncated"], None, None, 0)
    assert same_outputs(r["first"], t1, ("obs", "reward")) == ""
    t = host_outputs(cfg, H, n)
    twin.rollout(np.array(out["actions"]), H, t["obs"], t["reward"], t["terminated"], t["truncated"], None, None, 0)
    ll = twin.last_launch()
    assert ll["actions_in_kernel"] == 0 and (ll["food_slots"], ll["literal_constants"]) == e["kernel"]
    assert same_outputs(out, t, ("obs", "reward")) == ""
    tw_state = device_state(twin, cfg)
    assert np.array_equal(r["state"][1][_capi.I_RNG_COUNTER], tw_state[1][_capi.I_RNG_COUNTER]), "sampling consumed env draws"
    assert same_state(r["state"], tw_state), "final state differs from the twin's"
    assert twin.global_step == 1 + H and twin.stats() == r["stats"] and r["stats"]["env_steps"] == (1 + H) * n
    if e["case"] in gm.EXTRA_CASES:     # the project's parity contract: flags equal, obs 1e-5, state 1e-9
        orc = ol.OracleVec(cfg, n, seed=gm.KEY)
        orc.set_state(r["f64"], r["i32"])
        ref = orc.rollout(np.concatenate([r["first"]["actions"], out["actions"]]), want_final=True)
        got = {k: np.concatenate([r["first"][k], out[k]]) for k in ("obs", "reward", "terminated", "truncated")}
        d, rd = assert_parity(cfg, got, ref, name)
        assert_state_parity(cfg, twin, orc, name)
        ev = gm.pc.count_events(ref)
        print(f"{name}: against the oracle: obs {d:.3g}, reward {rd:.3g}; {ev}")
        assert ev["mixed_wave_steps"] >= 1 and ev["wall"] + ev["truncated"] >= 1
        orc.close()
    twin.close()


@pytest.mark.parametrize("name", NAMES)
def test_evaluate_sampled_gives_the_summary_of_the_sampled_rollout(name):
    r = device_run(name)
    e, cfg, out, n = r["e"], r["cfg"], r["out"], r["e"]["n"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    rec = np.full((n, _capi.EVAL_WORDS), 0x5A5A5A5A, np.int32)          # junk: overwritten, twice
    dev.evaluate_policy_sampled(ph, 1, rec, 0)
    dev.evaluate_policy_sampled(ph, H, rec, 0)
    ll = dev.last_launch()
    assert (ll["food_slots"], ll["literal_constants"]) == e["kernel"] and ll["full_signature"] == 4 and ll["actions_in_kernel"] == 3
    assert (ll["envs_unpredicated"], ll["envs_predicated"]) == ((0, n) if e["predicated"] else (n, 0))
    assert ph.noise_step == 1 + H
    want = summarize_rollout(out["reward"], out["terminated"], out["truncated"])
    v = evaluation_views(rec)
    evaluation_views(want)["food"][:] = v["food"]         # the per-step outputs do not show captures: the statistics do
    assert np.array_equal(rec, want), [k for k in ("return_sum", "first_return", "first_length", "first_end", "episodes")
                                       if not np.array_equal(v[k], evaluation_views(want)[k])]
    ends_first = int((r["first"]["terminated"] | r["first"]["truncated"]).sum())
    assert dev.stats()["food_collected"] == r["stats"]["food_collected"] >= int(v["food"].sum())
    assert int(v["episodes"].sum()) == r["stats"]["episodes"] - ends_first >= 1
    assert same_state(device_state(dev, cfg), r["state"]) and dev.global_step == 1 + H and dev.stats() == r["stats"]
    ph.close()
    dev.close()


@pytest.mark.parametrize("name", NAMES)
def test_update_equals_a_fresh_policy(name):
    """After policy_update the handle samples from the second weight set: the bits of a policy created with that set on a
    handle brought to the same place and noise step, and the definition of the second set — not the first's."""
    r = device_run(name)
    e, cfg, n = r["e"], r["cfg"], r["e"]["n"]
    dev = started(cfg, n, r["f64"], r["i32"])
    ph = dev.policy_create(r["policy"])
    first, again = first_step_then_run(dev, ph, cfg)
    ph.close()
    assert same_outputs(first, r["first"]) == "" and same_outputs(again, r["out"]) == ""                 # deterministic
    assert same_state(device_state(dev, cfg), r["state"])
    fresh = dev.policy_create(r["policy_b"])
    fresh.set_noise_step(1 + H)
    got = run_sampled(dev, fresh, cfg, HU)
    assert same_outputs(got, r["out_b"]) == "" and fresh.noise_step == 1 + H + HU
    assert same_state(device_state(dev, cfg), r["state_b"]) and dev.global_step == 1 + H + HU
    fresh.close()
    dev.close()
    seen = np.concatenate([r["out"]["obs"][-1:], r["out_b"]["obs"][:-1]])
    z = gm.noise(r["policy_b"], n, 1 + H, HU, gm.KEY)
    gm.assert_is_the_stage(name + " (updated)", r["policy_b"], seen, r["out_b"], z)
    m, rr = gm.restated(r["policy"], seen)               # and they are not the first set's
    assert gm.outside(r["out_b"]["actions"], r["out_b"]["logp"], gm.stage(r["policy"], m, rr, z)).mean() > 0.5


# ------------------------------------------------------------------------------------------------ once
@pytest.mark.parametrize("name,label", gm.UPLOADED_MUTANTS)
def test_the_comparison_can_fail_mutant_weights_on_the_unchanged_kernel(name, label):
    """A mutant's WEIGHTS uploaded to the unchanged kernel: held to the unmutated policy the run leaves the stage bound on
    at least MUTANT_ROWS rows — and it is the stage of the heads the uploaded weights restate."""
    e, cfg, f64, i32 = gm.start_snapshot(name)
    policy, n = gm.entry_policy(name), e["n"]
    w, _ = gm.weight_mutants(policy)[label]
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy, weights=w)
    first, out = first_step_then_run(dev, ph, cfg)
    ph.close()
    dev.close()
    seen = np.concatenate([first["obs"], out["obs"][:-1]])
    z = gm.noise(policy, n, 1, H, gm.KEY)
    m, r = gm.restated(policy, seen)
    rows = int(gm.outside(out["actions"], out["logp"], gm.stage(policy, m, r, z)).sum())
    print(f"{name} with {label} uploaded: {rows} of {H * n} rows outside the stage bound of the unmutated policy")
    assert rows >= gm.MUTANT_ROWS
    mm, rm, sub = ol.policy_forward_gaussian(policy, seen, weights=w)
    assert sub == 0 and not gm.outside(out["actions"], out["logp"], gm.stage(policy, mm, rm, z)).any()


@pytest.mark.parametrize("name", gm.BASE_ENTRIES)
def test_env_base_the_noise_is_keyed_by_the_global_index(name):
    r = device_run(name, gm.BASE)
    e, cfg, policy, out, n = r["e"], r["cfg"], r["policy"], r["out"], r["e"]["n"]
    gm.assert_is_the_stage(f"{name} at base 2^32 + 320", policy, r["seen"], out, gm.noise(policy, n, 1, H, gm.KEY, gm.BASE))
    share = gm.local_index_share(policy, r["seen"], out["actions"], 1, gm.KEY)
    print(f"{name}: {share:.3f} of the actions are more than {gm.sc.OFF_BY_ONE_BOUNDS:.0f} bounds from the definition under the local env index")
    assert share > gm.sc.OFF_BY_ONE_SHARE
    # handle and oracle are keyed by the global index too: another start state than at base 0, the oracle's flags on these actions
    assert not np.array_equal(r["f64"], device_run(name)["f64"])
    orc = ol.OracleVec(cfg, n, seed=gm.KEY, env_index_base=gm.BASE)
    orc.set_state(r["f64"], r["i32"])
    ref = orc.rollout(np.concatenate([r["first"]["actions"], out["actions"]]), want_final=True)
    orc.close()
    got = {k: np.concatenate([r["first"][k], out[k]]) for k in ("obs", "reward", "terminated", "truncated")}
    assert_parity(cfg, got, ref, name)


@pytest.mark.parametrize("name", gm.BASE_ENTRIES)
def test_env_base_one_handle_equals_two_shards(name):
    """One handle of 256 envs at base B == two handles of 128 at bases B and B + 128 with their own policy objects, at the
    same noise step: bit for bit in actions, logp, obs, reward and flags."""
    HS, half = 32, 128
    e, cfg, f64, i32 = gm.start_snapshot(name, gm.BASE, n=2 * half)
    policy = gm.entry_policy(name)

    def run(base, cols):
        dev = started(cfg, cols.stop - cols.start, np.ascontiguousarray(f64[:, cols]), np.ascontiguousarray(i32[:, cols]), base=base)
        ph = dev.policy_create(policy)
        ph.set_noise_step(3)
        o = run_sampled(dev, ph, cfg, HS)
        assert ph.noise_step == 3 + HS
        ph.close()
        dev.close()
        return o
    whole = run(gm.BASE, slice(0, 2 * half))
    for k in range(2):
        cols = slice(k * half, (k + 1) * half)
        shard = run(gm.BASE + k * half, cols)
        assert same_outputs({key: v[:, cols] for key, v in whole.items()}, shard) == "", k
    assert not np.array_equal(whole["actions"][:, :half], whole["actions"][:, half:])
    assert (whole["terminated"] | whole["truncated"]).any()


def test_noise_step_wraps_at_2_to_the_32():
    name, HW, n0 = gm.WRAP_ENTRY, 8, 2 ** 32 - 5
    e, cfg, f64, i32 = gm.start_snapshot(name)
    policy, n = gm.entry_policy(name), e["n"]
    dev = started(cfg, n, f64, i32)
    ph = dev.policy_create(policy)
    first = run_sampled(dev, ph, cfg, 1)
    ph.set_noise_step(n0)
    assert ph.noise_step == n0
    out = run_sampled(dev, ph, cfg, HW)
    assert ph.noise_step == 2 ** 32 + 3
    ph.close()
    dev.close()
    seen = np.concatenate([first["obs"], out["obs"][:-1]])
    z = np.concatenate([gm.noise(policy, n, n0, 5, gm.KEY), gm.noise(policy, n, 0, 3, gm.KEY)])       # (n mod 2^32), written out
    assert np.array_equal(z, gm.noise(policy, n, n0, HW, gm.KEY))
    gm.assert_is_the_stage(f"{name} across the wrap", policy, seen, out, z)
    m, r = gm.restated(policy, seen)            # not the steps 2^32 - 5 .. 2^32 + 2 without the wrap taken one step late or early
    for wrong in (np.concatenate([z[1:], z[:1]]), np.concatenate([z[-1:], z[:-1]])):
        assert gm.outside(out["actions"], out["logp"], gm.stage(policy, m, r, wrong)).mean() > 0.9
