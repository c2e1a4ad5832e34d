"""Host pointers equal device pointers, bit for bit, in every entry point whose host-pointer form goes through the staging
path of salp_vec.hip: reset, observe, get_state, set_state, step / rollout, step_packed / rollout_packed, rollout_policy
(and _sampled), evaluate_policy (and _sampled).

Two handles of one seed get the same calls, one with numpy arrays, one with device tensors and SALP_DEVICE_PTRS; every
output and, at the end, the state, the statistics and the counters must be equal.  The one-food and the 12-food preset,
100 envs (one predicated launch) and 192 (one unpredicated launch), H = 3.  Among the calls are the ones whose outputs are
also inputs — final_obs, the packed record's terminal-observation tail, SALP_EVAL_ACCUMULATE on a record that holds
something: what the call does not write must come back as it went in — and the rollout without actions, where the two
forms take different routes (generated ahead of the launch into act_out / generated in the kernel) to the same action
stream (include/salp_vec.h "Randomness")."""
import numpy as np
import pytest

import parity_cases as pc
import sampled_cases as sc
from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._capi import SalpLib

pytestmark = pytest.mark.gpu

H = 3
DEV, TAIL, ACC = _capi.SALP_DEVICE_PTRS, _capi.REC_FINAL_OBS, _capi.EVAL_ACCUMULATE
SENTINEL = {np.dtype(np.float32): np.uint32(0xA5C3F00D).view(np.float32), np.dtype(np.uint8): 0xA5,
            np.dtype(np.int32): -1515982835, np.dtype(np.float64): -7.25}


class Pair:
    """The same call on both handles: `out(...)` / `given(...)` make a host array and a device tensor of equal contents,
    `call` runs the method on each with its own set, `check` compares every array made since the last check."""

    def __init__(self, cfg, n):
        import torch
        self.torch = torch
        self.host, self.dev = SalpLib(cfg, n, device_id=0, seed=11), SalpLib(cfg, n, device_id=0, seed=11)
        self.made = []

    def given(self, a, name="input"):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.copy()).to("cuda:0")
        self.made.append((name, a, t))
        return (a, t)

    def out(self, name, shape, dtype):
        return self.given(np.full(shape, SENTINEL[np.dtype(dtype)], dtype), name)

    def call(self, method, *args, flags=0):
        for side, (obj, fl) in enumerate(((self.host, flags), (self.dev, flags | DEV))):
            getattr(obj, method)(*[a[side] if isinstance(a, tuple) else a for a in args], fl)
        self.torch.cuda.synchronize()

    def check(self, what):
        for name, a, t in self.made:
            got = t.cpu().numpy()
            assert np.array_equal(a.view(np.uint8), got.view(np.uint8)), f"{what}: {name} differs between host and device pointers"
        self.made = []

    def close(self):
        self.host.close()
        self.dev.close()


@pytest.mark.parametrize("n", [100, 192])
@pytest.mark.parametrize("preset", ["single_food", "sac_gail"])
def test_host_pointers_equal_device_pointers(preset, n):
    cfg = pc.make_cfg(dict(preset=preset, max_steps_without_food=8))      # episodes end within a few steps
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)
    orc.close()
    p = Pair(cfg, n)
    OD, AD = cfg.obs_dim, cfg.act_dim
    rng = np.random.default_rng(5)
    outputs = lambda h: [p.out("obs", (h, n, OD), np.float32), p.out("reward", (h, n), np.float32),
                         p.out("terminated", (h, n), np.uint8), p.out("truncated", (h, n), np.uint8)]
    state = lambda: [p.out("f64", (_capi.F_FOOD0 + 2 * cfg.num_food_items, n), np.float64), p.out("i32", (_capi.I_COUNT, n), np.int32)]

    p.call("reset", p.given((rng.uniform(size=n) < 0.5).astype(np.uint8), "mask"), p.out("obs", (n, OD), np.float32))
    p.check("reset(mask, obs)")
    p.call("reset", None, p.out("obs", (n, OD), np.float32))
    p.check("reset(NULL, obs)")
    p.call("set_state", p.given(f64), p.given(i32))
    p.call("get_state", *state())
    p.check("set_state / get_state")
    p.call("get_state", None, p.out("i32", (_capi.I_COUNT, n), np.int32))
    p.check("get_state(NULL, i32)")
    p.call("observe", p.out("obs", (n, OD), np.float32))
    p.check("observe")

    finished = 0
    for t in range(H):       # salp_vec_step with every output; final_obs goes in as well as out
        o = outputs(1)
        p.call("step", p.given(pc.make_actions(cfg, 1, n, 20 + t)), *o, p.out("final_obs", (1, n, OD), np.float32),
               p.out("info", (n, _capi.INFO_COLS), np.int32))
        finished += int((o[2][0] | o[3][0]).sum())
        p.check(f"step {t}")
    assert finished > 0, "no episode ended: final_obs was never written"
    act = p.given(pc.make_actions(cfg, H, n, 30), "act")
    p.call("rollout", act, H, *outputs(H), p.out("final_obs", (H, n, OD), np.float32), None)
    p.check("rollout(final_obs)")
    p.call("rollout", act, H, *outputs(H), None, None)
    p.check("rollout")
    o = outputs(H)
    p.call("rollout", act, H, o[0], None, o[2], o[3], None, None)
    p.check("rollout(reward = NULL)")
    p.call("rollout", None, H, *outputs(H), None, p.out("act_out", (H, n, AD), np.float32))
    p.check("rollout(act = NULL, act_out)")
    p.call("rollout", None, H, *outputs(H), None, None)
    p.check("rollout(act = NULL)")

    W, WT = p.host.record_width(False), p.host.record_width(True)
    p.call("step_packed", p.given(pc.make_actions(cfg, 1, n, 40)), p.out("rec", (n, W), np.float32))
    p.check("step_packed")
    p.call("rollout_packed", act, H, p.out("rec", (H, n, W), np.float32), None)
    p.check("rollout_packed")
    p.call("rollout_packed", act, H, p.out("rec", (H, n, WT), np.float32), None, flags=TAIL)
    p.check("rollout_packed(tail)")
    p.call("rollout_packed", None, H, p.out("rec", (H, n, WT), np.float32), p.out("act_out", (H, n, AD), np.float32), flags=TAIL)
    p.check("rollout_packed(act = NULL, act_out, tail)")

    policy = sc.gaussian_policy(OD, AD, (32, 32), 123, 1.5, 2.0, (-1.0,) * AD, free_breathing=not cfg.forced_breathing)
    ph = (p.host.policy_create(policy), p.dev.policy_create(policy))
    p.call("rollout_policy", ph, H, *outputs(H), p.out("act_out", (H, n, AD), np.float32))
    p.check("rollout_policy")
    p.call("rollout_policy", ph, H, *outputs(H), None)
    p.check("rollout_policy(act_out = NULL)")
    p.call("rollout_policy_sampled", ph, H, *outputs(H), p.out("act_out", (H, n, AD), np.float32), p.out("logp", (H, n), np.float32))
    p.check("rollout_policy_sampled")
    p.call("rollout_policy_sampled", ph, H, *outputs(H), None, None)
    p.check("rollout_policy_sampled(act_out = logp_out = NULL)")
    rec = p.out("rec", (n, _capi.EVAL_WORDS), np.int32)
    p.call("evaluate_policy", ph, H, rec)
    p.check("evaluate_policy")
    before = rec[0].copy()
    # (the record sat at the start of the host handle's staging block: observe() overwrites it there, so that a continued
    # record can only come from the copy in, never from what the call before left behind)
    p.call("observe", p.out("obs", (n, OD), np.float32))
    p.made.append(("rec", *rec))                           # compared again after it has been continued
    p.call("evaluate_policy", ph, H, rec, flags=ACC)
    p.check("evaluate_policy(accumulate)")
    assert not np.array_equal(before, rec[0]), "the records were not continued"
    assert (rec[0][:, _capi.EVAL_EPISODES] >= before[:, _capi.EVAL_EPISODES]).all(), "the episode counts did not go on from the record"
    p.call("observe", p.out("obs", (n, OD), np.float32))
    p.made.append(("rec", *rec))
    p.call("evaluate_policy_sampled", ph, H, rec, flags=ACC)
    p.check("evaluate_policy_sampled(accumulate)")
    p.call("evaluate_policy_sampled", ph, H, p.out("rec", (n, _capi.EVAL_WORDS), np.int32))
    p.check("evaluate_policy_sampled")

    assert ph[0].noise_step == ph[1].noise_step == 4 * H
    assert p.host.global_step == p.dev.global_step == H + 1 + 16 * H             # H steps, step_packed, 16 calls of H steps
    assert p.host.stats() == p.dev.stats()
    p.call("get_state", *state())
    p.check("the final state")
    p.close()
