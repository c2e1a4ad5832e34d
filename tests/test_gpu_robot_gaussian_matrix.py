"""The robot's in-kernel 6 -> 3 policies over the robot entries of tests/gaussian_matrix.py on the GPU (CPU guard:
tests/test_gaussian_matrix.py).  Run with `pytest -m gpu`.

Every entry runs max_cycles = 3 behind one staggering step and a masked reset (every third robot), so that each wavefront
mixes finished and unfinished lanes, for H = 7 env steps.  Gaussian entries: every action and log-probability of
salp_robot_vec_rollout_policy_sampled within the stage bound of `GaussianPolicy.sampling_stage(m, r, z)` — m, r the C
restatement of the two heads on the rows the kernel wrote, z the noise of (global env index, noise step): components 0 and 1
from the stream-3 block, component 2 from the stream-4 block — and within `error_bound`; the mean path against the restated
mean head; a twin replaying the actions; the summary records; policy update.  `clip` entries: the deterministic call EQUAL
to the C restatement as float32 values — the robot policy's arithmetic bit for bit.  Once: mutant weights on the unchanged
kernel, env_index_base = 2^32 + 320 with the shard property, and the noise step's wrap at 2^32."""
import functools

import numpy as np
import pytest

import gaussian_matrix as gm
import oracle_lib as ol
import policy_matrix as pm
from support import bits
from underwater_swimmer_rl_amd.policy import robot_evaluation_views, summarize_robot_rollout
from underwater_swimmer_rl_amd.robot_env import R_RNG, SalpRobotVectorEnv

pytestmark = pytest.mark.gpu

H, HU, SEED = gm.ROBOT_H, 4, gm.ROBOT_SEED
OUT_KEYS = ("obs", "reward", "terminated", "truncated", "inner_steps", "_final_observation", "actions", "logp")


def host(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.array(x, copy=True)


def kept(out):
    """A rollout's dict as host copies (the blocks are the env's own buffers)."""
    return {k: (None if v is None else host(v)) for k, v in out.items()}


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b, keys=OUT_KEYS):
    """The keys whose blocks differ in bits; final observations are compared on the rows that ended."""
    bad = [k for k in keys if not np.array_equal(raw(a[k]), raw(b[k]))]
    done = a["_final_observation"]
    if not np.array_equal(raw(a["final_observation"][done]), raw(b["final_observation"][done])):
        bad.append("final_observation")
    return bad


def staggered_env(n, base=0, first=0):
    """A fresh env with max_cycles = 3 behind the staggering step and the masked reset; returns it and the entry row.
    `first`: the position of env 0 in the batch whose staggering this env takes part in (shards)."""
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=SEED, env_index_base=base, output="numpy", max_cycles=gm.ROBOT_MAX_CYCLES)
    env.step(gm.robot_first_action(n, first))
    env.reset(mask=gm.robot_reset_mask(n, first))
    return env, host(env.observe())


def rows_seen(entry, obs):
    return np.concatenate([entry[None], obs[:-1]])


@functools.lru_cache(maxsize=None)
def device_run(name, base=0):
    """One Gaussian entry on the GPU, computed once, shared, read-only: H sampled steps from noise step 0, then — after the
    update to the second weight set — HU more."""
    e = gm.ROBOT_ENTRIES[name]
    policy, policy_b, n = gm.entry_policy(name), gm.entry_policy(name, 1), e["n"]
    env, entry = staggered_env(n, base)
    handle = env.make_policy(policy)
    assert handle.gaussian and handle.words == policy.words and handle.noise_step == 0
    out = kept(env.rollout_policy(handle, H, sample=True))
    state = env.get_state()
    assert handle.noise_step == H
    handle.update(policy_b.pack())
    out_b = kept(env.rollout_policy(handle, HU, sample=True))
    state_b = env.get_state()
    assert handle.noise_step == H + HU
    env.close()
    seen = rows_seen(entry, out["obs"])
    for a in (entry, seen, state, state_b, *out.values(), *out_b.values()):
        a.setflags(write=False)
    return dict(e=e, policy=policy, policy_b=policy_b, entry=entry, seen=seen, out=out, state=state, out_b=out_b, state_b=state_b)


def assert_mixed_endings(out):
    done = out["_final_observation"]
    n = done.shape[1] // 64 * 64
    per_wave = done[:, :n].reshape(done.shape[0], -1, 64).sum(axis=2)
    assert ((per_wave > 0) & (per_wave < 64)).any() and out["truncated"].sum() > done.shape[1]
    assert np.ptp(out["inner_steps"][:, :64]) > 50, "cycle lengths must differ inside a wavefront"


@pytest.mark.parametrize("name", gm.ROBOT_GAUSSIAN)
def test_every_action_and_logp_is_the_sampling_stage_of_the_restated_heads(name):
    r = device_run(name)
    policy, out, n = r["policy"], r["out"], r["e"]["n"]
    assert out["actions"].shape == (H, n, 3) and out["logp"].shape == (H, n) and out["logp"].dtype == np.float32
    ratios = gm.assert_is_the_stage(name, policy, r["seen"], out, gm.noise(policy, n, 0, H, SEED))
    print(f"RATIO {name} slots=robot literal=- " + " ".join(f"{v:.4f}" for v in ratios))
    assert_mixed_endings(out)


@pytest.mark.parametrize("name", gm.ROBOT_GAUSSIAN)
def test_the_deterministic_call_runs_the_restated_mean_head(name):
    r = device_run(name)
    policy, n = r["policy"], r["e"]["n"]
    mean = policy.mean_policy()
    env, entry = staggered_env(n)
    handle = env.make_policy(policy)
    handle.set_noise_step(5)
    out = kept(env.rollout_policy(handle, H))
    assert "logp" not in out and handle.noise_step == 5 and np.array_equal(entry, r["entry"])
    env.close()
    seen = rows_seen(entry, out["obs"])
    u, _ = pm.restated(mean, seen)
    m, _ = gm.restated(policy, seen)
    assert np.array_equal(bits(u), bits(m))
    exact, tb = pm.tanh_stage_bound(mean, u)
    terr = np.abs(out["actions"].astype(np.float64) - exact)
    err, bound = np.abs(out["actions"].astype(np.float64) - mean.reference(seen)), mean.error_bound(seen)
    print(f"{name}: mean path: |action - (tanh(m) scale + shift)| / bound <= {(terr / tb).max():.3g}; / error_bound <= {(err / bound).max():.3g}")
    assert (terr <= tb).all(), f"{int((terr > tb).sum())} actions outside the tanh-stage bound, worst ratio {(terr / tb).max()}"
    assert (err <= bound).all()


@pytest.mark.parametrize("name", gm.ROBOT_CLIP)
def test_clip_policy_equals_the_restatement_bit_for_bit(name):
    """The deterministic `clip` chain is IEEE arithmetic only: every action of salp_robot_vec_rollout_policy EQUALS the C
    restatement's, as float32 values, on the row before it."""
    e, policy = gm.ROBOT_ENTRIES[name], gm.entry_policy(name)
    env, entry = staggered_env(e["n"])
    out = kept(env.rollout_policy(policy, H))
    env.close()
    seen = rows_seen(entry, out["obs"])
    u, a = pm.restated(policy, seen)
    same = out["actions"] == a
    open_ = (np.abs(u) < 1.0).mean()
    print(f"{name}: {int((~same).sum())} of {same.size} values differ from the restatement, {int((bits(out['actions']) != bits(a)).sum())} in bits; "
          f"{open_:.3f} of the entries inside the clamp")
    assert same.all(), (f"{int((~same).sum())} actions are not the restatement's, first at {np.unravel_index(np.argmin(same), same.shape)}: "
                        f"{out['actions'][np.unravel_index(np.argmin(same), same.shape)]!r} != {a[np.unravel_index(np.argmin(same), same.shape)]!r}")
    assert open_ >= gm.NOT_BLIND
    assert_mixed_endings(out)


@pytest.mark.parametrize("name", gm.ROBOT_GAUSSIAN)
def test_twin_rollout_on_the_actions_taken(name):
    r = device_run(name)
    twin, entry = staggered_env(r["e"]["n"])
    replay = kept(twin.rollout(r["out"]["actions"]))
    state = twin.get_state()
    twin.close()
    assert np.array_equal(entry, r["entry"])
    assert same_bits(r["out"], replay, tuple(k for k in OUT_KEYS if k not in ("actions", "logp"))) == []
    assert np.array_equal(r["state"][R_RNG], state[R_RNG]), "the env's own draw counter was consumed"
    assert np.array_equal(raw(r["state"]), raw(state)), "final state differs from the twin's"


@pytest.mark.parametrize("name", gm.ROBOT_GAUSSIAN)
def test_evaluate_sampled_gives_the_summary_of_the_sampled_rollout(name):
    r = device_run(name)
    out, n = r["out"], r["e"]["n"]
    env, _ = staggered_env(n)
    handle = env.make_policy(r["policy"])
    rec = np.full((n, 12), 0x5A5A5A5A, np.int32)
    v = env.evaluate_policy(handle, H, out=rec, sample=True)
    assert handle.noise_step == H
    want = summarize_robot_rollout(out["reward"], out["terminated"], out["truncated"], out["inner_steps"])
    assert np.array_equal(rec, want), [k for k, a in robot_evaluation_views(want).items() if k != "record" and not np.array_equal(a, v[k])]
    assert np.array_equal(raw(env.get_state()), raw(r["state"])) and int(v["episodes"].sum()) > n
    env.close()


@pytest.mark.parametrize("name", gm.ROBOT_GAUSSIAN)
def test_update_equals_a_fresh_policy(name):
    r = device_run(name)
    n = r["e"]["n"]
    env, _ = staggered_env(n)
    handle = env.make_policy(r["policy"])
    again = kept(env.rollout_policy(handle, H, sample=True))
    assert same_bits(again, r["out"]) == [] and np.array_equal(raw(env.get_state()), raw(r["state"]))      # deterministic
    fresh = env.make_policy(r["policy_b"])
    fresh.set_noise_step(H)
    got = kept(env.rollout_policy(fresh, HU, sample=True))
    assert same_bits(got, r["out_b"]) == [] and fresh.noise_step == H + HU
    assert np.array_equal(raw(env.get_state()), raw(r["state_b"]))
    env.close()
    seen = rows_seen(r["out"]["obs"][-1], r["out_b"]["obs"])
    z = gm.noise(r["policy_b"], n, H, HU, SEED)
    gm.assert_is_the_stage(name + " (updated)", r["policy_b"], seen, r["out_b"], z)
    m, rr = gm.restated(r["policy"], seen)               # and they are not the first set's
    assert gm.outside(r["out_b"]["actions"], r["out_b"]["logp"], gm.stage(r["policy"], m, rr, z)).mean() > 0.5


# ------------------------------------------------------------------------------------------------ once
def test_the_comparison_can_fail_mutant_weights_on_the_unchanged_kernel():
    name, label = "robot-16x64-n128", "ls_rows_at_stride_h0"
    e, policy = gm.ROBOT_ENTRIES[name], gm.entry_policy(name)
    n = e["n"]
    w, _ = gm.weight_mutants(policy)[label]
    env, entry = staggered_env(n)
    handle = env.make_policy(policy, weights=w)
    out = kept(env.rollout_policy(handle, H, sample=True))
    env.close()
    seen, z = rows_seen(entry, out["obs"]), gm.noise(policy, n, 0, H, SEED)
    m, r = gm.restated(policy, seen)
    rows = int(gm.outside(out["actions"], out["logp"], gm.stage(policy, m, r, z)).sum())
    print(f"{name} with {label} uploaded: {rows} of {H * n} rows outside the stage bound of the unmutated policy")
    assert rows >= gm.MUTANT_ROWS
    mm, rm, sub = ol.policy_forward_gaussian(policy, seen, weights=w)
    assert sub == 0 and not gm.outside(out["actions"], out["logp"], gm.stage(policy, mm, rm, z)).any()


def test_env_base_the_noise_is_keyed_by_the_global_index_and_shards_agree():
    name = gm.ROBOT_WRAP_ENTRY
    r = device_run(name, gm.BASE)
    policy, out, n = r["policy"], r["out"], r["e"]["n"]
    gm.assert_is_the_stage(f"{name} at base 2^32 + 320", policy, r["seen"], out, gm.noise(policy, n, 0, H, SEED, gm.BASE))
    share = gm.local_index_share(policy, r["seen"], out["actions"], 0, SEED)
    print(f"{name}: {share:.3f} of the actions are more than {gm.sc.OFF_BY_ONE_BOUNDS:.0f} bounds from the definition under the local env index")
    assert share > gm.sc.OFF_BY_ONE_SHARE
    assert not np.array_equal(r["entry"], device_run(name)["entry"])          # the targets are keyed by the global index too
    # one env of 256 robots at base B == two envs of 128 at B and B + 128 with their own policy objects, at one noise step
    def run(base, count):
        env, _ = staggered_env(count, base, base - gm.BASE)
        handle = env.make_policy(policy)
        handle.set_noise_step(3)
        o = kept(env.rollout_policy(handle, H, sample=True))
        env.close()
        return o
    whole = run(gm.BASE, 256)
    for k in range(2):
        cols = slice(128 * k, 128 * (k + 1))
        shard = run(gm.BASE + 128 * k, 128)
        part = {key: whole[key][:, cols] for key in OUT_KEYS + ("final_observation",)}
        assert same_bits(part, shard) == [], k
    assert not np.array_equal(whole["actions"][:, :128], whole["actions"][:, 128:])


def test_noise_step_wraps_at_2_to_the_32():
    name, HW, n0 = gm.ROBOT_WRAP_ENTRY, 8, 2 ** 32 - 5
    e, policy = gm.ROBOT_ENTRIES[name], gm.entry_policy(name)
    n = e["n"]
    env, entry = staggered_env(n)
    handle = env.make_policy(policy)
    handle.set_noise_step(n0)
    assert handle.noise_step == n0
    out = kept(env.rollout_policy(handle, HW, sample=True))
    assert handle.noise_step == 2 ** 32 + 3
    env.close()
    seen = rows_seen(entry, out["obs"])
    z = np.concatenate([gm.noise(policy, n, n0, 5, SEED), gm.noise(policy, n, 0, 3, SEED)])       # (n mod 2^32), written out
    assert np.array_equal(z, gm.noise(policy, n, n0, HW, SEED))
    gm.assert_is_the_stage(f"{name} across the wrap", policy, seen, out, z)
    m, r = gm.restated(policy, seen)
    for wrong in (np.concatenate([z[1:], z[:1]]), np.concatenate([z[-1:], z[:-1]])):
        assert gm.outside(out["actions"], out["logp"], gm.stage(policy, m, r, wrong)).mean() > 0.9
