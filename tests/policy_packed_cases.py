"""The case table of the packed closed loop (salp_vec_rollout_policy_packed), shared by tests/test_gpu_policy_packed.py and
its CPU guard tests/test_policy_packed_cases.py: the six cases of tests/policy_cases.py and five more for the handle classes
that table does not reach — 8 slots (literal and run-time constants, the latter free-breathing), run-time constants at 12
and at 16 slots, and the 8-slot kernel as one predicated launch.  Needs numpy, the package's configuration,
`policy.MLPPolicy` and the oracle binding — no GPU library.

Every added policy is `policy_cases.random_policy(..., seed=123, gain=1.5, out_gain=6.0)`.  What a case must show, on the
oracle stepped closed-loop under its own policy from the injected start state of tests/parity_cases.py: an episode ended by
a wall, one ended by truncation, and a wavefront-step that mixes finished and unfinished lanes (the guard asserts it)."""
import functools

import numpy as np

import parity_cases as pc
import policy_cases as dc

H = pc.HORIZON
WAVE = pc.WAVE

_ADDED = dict(seed=123, gain=1.5, out_gain=6.0)
# the keys of policy_cases.CASES; kernel: (food slots, literal constants)
CASES = {
    **dc.CASES,
    "class_default_F5": dict(case="class_default_F5", n=256, hidden=(32, 32), out="tanh", kernel=(8, 1), predicated=False, **_ADDED),
    "other_tank_F5_free": dict(case="other_tank_F5_free", n=256, hidden=(48, 32), out="tanh", kernel=(8, 0), predicated=False, **_ADDED),
    "other_physics_F12": dict(case="other_physics_F12", n=256, hidden=(16,), out="tanh", kernel=(12, 0), predicated=False, **_ADDED),
    "F16_sixteen_slots_other_tank": dict(case="F16_sixteen_slots_other_tank", n=256, hidden=(32,), out="clip", kernel=(16, 0),
                                         predicated=False, **_ADDED),
    "class_default_F5_ragged": dict(case="class_default_F5", n=293, hidden=(32, 32), out="tanh", kernel=(8, 1), predicated=True, **_ADDED),
}
ADDED = tuple(k for k in CASES if k not in dc.CASES)
# the cases that also run sampled (tests/test_gpu_policy_packed.py): two of tests/sampled_cases.py, two of the added ones
SAMPLED = ("one_food_mlp32", "sac_gail_mlp64", "class_default_F5", "other_tank_F5_free")
NARROW = ("one_food_mlp32", "sac_gail_mlp64")       # the cases that also run without the terminal tail: one food and 12 slots


def case_cfg(name):
    return pc.case_cfg(CASES[name]["case"])


def case_policy(name):
    c, cfg = CASES[name], case_cfg(name)
    return dc.random_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["out"], c["seed"], c["gain"], c["out_gain"],
                            free_breathing=not cfg.forced_breathing)


def gaussian_twin(name):
    """The Gaussian policy of a sampled case: the case's own of tests/sampled_cases.py where that table has it, else built
    the same way (`sampled_cases.gaussian_policy`) on this table's widths, seed and hidden gain, with that table's mean-head
    gain of 2.0 and a log-std bias of -1 per component."""
    import sampled_cases as sc
    if name in sc.CASES:
        assert sc.CASES[name]["case"] == CASES[name]["case"] and sc.CASES[name]["n"] == CASES[name]["n"]
        return sc.case_policy(name)
    c, cfg = CASES[name], case_cfg(name)
    return sc.gaussian_policy(cfg.obs_dim, cfg.act_dim, c["hidden"], c["seed"], c["gain"], 2.0, (-1.0,) * cfg.act_dim,
                              free_breathing=not cfg.forced_breathing)


@functools.lru_cache(maxsize=None)
def oracle_closed_loop(name):
    """The oracle stepped closed-loop under `reference()` (rounded to float32) from the injected start state: computed once,
    shared, read-only.  Returns cfg, policy, the actions and the oracle's outputs with `info`."""
    c, cfg, policy = CASES[name], case_cfg(name), case_policy(name)
    orc, f64, i32 = pc.start_oracle(cfg, c["n"], pc.ENV_SEED)
    _, actions, outs, _ = dc.drive_oracle(orc, H, lambda t, o: (policy.reference(o).astype(np.float32), None))
    orc.close()
    for a in (actions, *outs.values()):
        a.setflags(write=False)
    return cfg, policy, actions, outs


def assert_events(name, ev):
    assert ev["wall"] >= 1 and ev["truncated"] >= 1 and ev["mixed_wave_steps"] >= 1, f"{name}: {ev}"
