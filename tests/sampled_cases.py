"""The sampled closed-loop case table (salp_vec_rollout_policy_sampled) shared by tests/test_gpu_policy_sampled.py and its
CPU guard tests/test_policy_sampled.py: which parity case (tests/parity_cases.py: configuration and injected start state),
how many envs, which Gaussian policy.  Needs numpy, the package's configuration, `policy.GaussianPolicy` and the oracle
binding — no GPU library.

Body and mean head are `policy_cases.random_policy` draws; the log-std head has small weights (gain 0.05) and a bias per
case, spread so that log_std lies in about [-3, 0]; the free-breathing case has its biases beyond both clamps (inhale
control +3 -> 2, nozzle -25 -> -20).  Seeds and gains were picked on the oracle until every case ends episodes by wall and
by truncation in mixed wavefronts under its own sampled actions and keeps both error bounds below their ceilings
(tests/test_policy_sampled.py asserts all of it).
"""
import functools

import numpy as np

import parity_cases as pc
import policy_cases as dc
from underwater_swimmer_rl_amd.policy import GaussianPolicy

H = pc.HORIZON
WAVE = pc.WAVE
KEY = pc.ENV_SEED           # the handles are created with this seed: the key of the noise stream

# name -> parity case, envs, hidden widths, weight seed, hidden gain, mean-head gain, log-std biases (one per action
#         component), the kernel that must run: (food slots, literal constants), whether the whole batch runs predicated
CASES = {
    "one_food_mlp32": dict(case="single_food", n=256, hidden=(32, 32), seed=123, gain=1.5, out_gain=2.0, b_ls=(-1.0,),
                           kernel=(1, 1), predicated=False),
    "one_food_mlp32_ragged": dict(case="single_food", n=293, hidden=(32, 32), seed=123, gain=1.5, out_gain=2.0, b_ls=(-2.0,),
                                  kernel=(1, 1), predicated=True),
    "sac_gail_mlp64": dict(case="sac_gail_F12", n=256, hidden=(64, 64), seed=125, gain=1.5, out_gain=2.0, b_ls=(-3.0,),
                           kernel=(12, 1), predicated=False),
    "free_breathing_mlp32_clamped": dict(case="free_breathing", n=256, hidden=(32, 32), seed=142, gain=1.5, out_gain=2.0,
                                         b_ls=(3.0, -25.0), kernel=(1, 1), predicated=False),
    "four_slots_other_tank_linear": dict(case="F3_other_tank", n=256, hidden=(), seed=102, gain=1.5, out_gain=2.0, b_ls=(-0.25,),
                                         kernel=(4, 0), predicated=False),
}
LS_GAIN = 0.05
BOUND_CEILING = dc.BOUND_CEILING      # the action bound's ceiling: the project's
# The log-probability bound's ceiling, per action component:
#   2 e_u with e_u <= BOUND_CEILING / min(scale) = 2e-4 (the action bound carries e_u through a 1-Lipschitz tanh and the
#     scale, 0.5 at the least: sac.Actor's [0, 1] component)                                                    4.0e-4
#   e_ls <= BOUND_CEILING (the same running bound as the mean head's, on a head with smaller weights)          1.0e-4
#   |z| e_z: |z| <= sqrt(48 ln 2) = 5.77, e_z <= |z| (0.5 ULP_LOGF + ULP_SQRTF + ULP_COSPIF + 0.5) 2^-23 < 4.5 |z| 2^-23   0.2e-4
#   the roundings: nine operations and library calls on magnitudes below 128 (z^2 / 2 <= 16.7, |ls| <= 20,
#     2 |log 2 - u - softplus| <= 2 |u| + 1.4 with |u| <= 40), 2^-24 each, the expf / log1pf ones ULP_* 2^-23 of values <= 1   0.8e-4
LOGP_BOUND_CEILING_PER_COMPONENT = 6e-4
OFF_BY_ONE_BOUNDS = 100.0            # a wrong noise step moves an action by more than this many bounds ...
OFF_BY_ONE_SHARE = 0.5               # ... in more than this share of the entries


def case_cfg(name):
    return pc.case_cfg(CASES[name]["case"])


def gaussian_policy(obs_dim, act_dim, hidden, seed, gain, out_gain, b_ls, free_breathing=False, ls_gain=LS_GAIN):
    mean = dc.random_policy(obs_dim, act_dim, hidden, "tanh", seed, gain, out_gain, free_breathing=free_breathing)
    rng = np.random.default_rng(seed + 5000)
    d = mean.layers[-1][0].shape[2]
    W = np.zeros((act_dim, d), np.float32)
    for r in range(act_dim):
        cols = rng.choice(d, size=min(4, d), replace=False)
        W[r, cols] = (rng.standard_normal(cols.size) * ls_gain / 2.0).astype(np.float32)
    b = np.asarray(b_ls, np.float32)
    assert b.shape == (act_dim,)
    return GaussianPolicy(mean.layers, (W[None], b[None]), mean.scale, mean.shift)


def case_policy(name):
    c, cfg = CASES[name], case_cfg(name)
    return gaussian_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["seed"], c["gain"], c["out_gain"], c["b_ls"],
                           free_breathing=not cfg.forced_breathing)


def floor_clamped_components(policy):
    """Components whose log-std bias is so far below the lower clamp (-24 or less, against |W_ls h| < 4 on every visited row:
    tests/test_policy_sampled.py) that the head is the constant -20: their standard deviation is e^-20 = 2e-9 and their
    action does not depend on the noise within any bound."""
    return np.nonzero(policy.log_std[1][0] <= -24.0)[0]


def case_noise(policy, n, n0=0, horizon=H, key=KEY, env_base=0):
    """z float64 [horizon, n, act_dim]: step t of a call that starts at noise step n0 draws block(env, n0 + t)."""
    env = np.arange(env_base, env_base + n, dtype=np.uint64)[None, :]
    steps = (n0 + np.arange(horizon, dtype=np.uint64))[:, None]
    return policy.noise(key, env, steps)


@functools.lru_cache(maxsize=None)
def oracle_closed_loop(name):
    """The oracle stepped closed-loop under `reference(obs, z)` (rounded to float32) from the injected start state and
    noise step 0: computed once, shared, read-only.  Returns cfg, policy, start snapshot, z, and the run: obs_in [H, n, OD]
    (what each action saw), actions, logp (float64) and the oracle's outputs with `info`."""
    c, cfg, policy = CASES[name], case_cfg(name), case_policy(name)
    n = c["n"]
    z = case_noise(policy, n)
    orc, f64, i32 = pc.start_oracle(cfg, n, pc.ENV_SEED)

    def act(t, o):
        a, lp = policy.reference(o, z[t])
        return a.astype(np.float32), lp
    obs_in, actions, outs, logp = dc.drive_oracle(orc, H, act)
    logp = np.array(logp, np.float64)
    orc.close()
    for a in (f64, i32, z, obs_in, actions, logp, *outs.values()):
        a.setflags(write=False)
    return cfg, policy, f64, i32, z, obs_in, actions, logp, outs


def assert_closed_loop_events(name, ev):
    """What a closed-loop case must show: a wall termination, a truncation, and a wavefront-step in which finished and
    unfinished lanes mix (what the deterministic cases demand, tests/policy_cases.py)."""
    assert ev["wall"] >= 1 and ev["truncated"] >= 1 and ev["mixed_wave_steps"] >= 1, f"{name}: {ev}"


def off_by_one_share(policy, seen, actions, n0=0, key=KEY):
    """Share of the action entries (components at the lower clamp aside) that lie more than OFF_BY_ONE_BOUNDS bounds from the
    definition evaluated with the noise of the NEXT step (n off by one)."""
    Hh, n = actions.shape[:2]
    z_wrong = case_noise(policy, n, n0 + 1, Hh, key)
    want, _ = policy.reference(seen, z_wrong)
    bound, _ = policy.error_bound(seen, z_wrong)
    keep = np.setdiff1d(np.arange(policy.act_dim), floor_clamped_components(policy))
    far = np.abs(np.asarray(actions, np.float64) - want) > OFF_BY_ONE_BOUNDS * bound
    return float(far[..., keep].mean())
