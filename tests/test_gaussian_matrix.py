"""The CPU guard of the Gaussian policy matrix (tests/gaussian_matrix.py, run on the GPU by tests/test_gpu_gaussian_matrix.py
and tests/test_gpu_robot_gaussian_matrix.py): the table covers what it must; the C restatement of the two heads
(`oracle_lib.policy_forward_gaussian`) is the deterministic restatement of each head; `GaussianPolicy.sampling_stage` covers
an fp32 evaluation from the same heads; and on the oracles alone, stepped closed-loop under the float32-rounded definition,
every entry ends episodes in mixed wavefronts, forms no subnormal, keeps both `error_bound`s below the project's ceilings
and the stage bound below `error_bound`, stays out of tanh saturation, keeps its log_std where the table says — and every
mutant of the log-std head's layout and of the noise definition moves action or logp outside the STAGE bound on at least
`MUTANT_ROWS` of the rows tried.  A mutant is exempt only where it touches nothing but a component that its entry clamps
by design (`clamped` of the entry)."""
import numpy as np
import pytest

import gaussian_matrix as gm
import oracle_lib as ol
import policy_matrix as pm
from support import bits
from underwater_swimmer_rl_amd.policy import GaussianPolicy, MLPPolicy

SNAKE, ROBOT = list(gm.ENTRIES), gm.ROBOT_GAUSSIAN
BASE_RUNS = list(gm.BASE_ENTRIES) + [gm.ROBOT_WRAP_ENTRY]       # entries that also run at env_index_base = BASE


def test_the_table_covers_what_it_must():
    E = gm.ENTRIES
    plain = {k: e for k, e in E.items() if e["P"] == 1 and not e["clamped"]}
    for case, A in (("single_food", 1), ("free_breathing", 2)):       # all 21 shapes with one and with two components
        assert {e["hidden"] for e in plain.values() if e["case"] == case and e["n"] == 128} == set(pm.SHAPES), case
        assert gm.case_cfg(case).act_dim == A
    for case in pm.FAMILY_CASES + tuple(gm.EXTRA_CASES):
        have = {(e["n"], e["hidden"]) for e in plain.values() if e["case"] == case}
        assert {(128, (64, 64)), (128, (16, 64)), (100, (48, 32))} <= have, case
    # every kernel family, literal and run-time constants; the predicated launch in each; free-breathing multi-food classes
    assert {e["kernel"] for e in E.values()} == {(s, l) for s in (1, 4, 8, 12, 16) for l in (0, 1)}
    assert {e["kernel"] for e in E.values() if e["predicated"]} == {e["kernel"] for e in E.values()}
    free = {e["kernel"] for e in E.values() if not gm.case_cfg(e["case"]).forced_breathing}
    assert {(1, 1), (8, 0), (12, 1), (16, 0)} <= free
    assert gm.EXTRA_KERNEL["free_F12"] == (12, 3, 1) and gm.EXTRA_KERNEL["free_F16_other_tank"] == (16, 3, 0)
    for case, spec in gm.EXTRA_CASES.items():
        cfg = gm.case_cfg(case)
        assert cfg.act_dim == 2 - cfg.forced_breathing and cfg.max_observed_food == 3 and case not in gm.pc.CASES
    # every one of the twenty K = 3 handle classes, unpredicated and as one predicated launch
    classes = {(s, l, f) for s in (1, 4, 8, 12, 16) for l in (0, 1) for f in (False, True)}
    for predicated in (False, True):
        assert {e["kernel"] + (bool(gm.case_cfg(e["case"]).forced_breathing),) for e in E.values() if e["predicated"] == predicated} == classes
    pops = {(e["case"], e["P"], e["n"], e["hidden"]) for e in E.values() if e["P"] > 1}
    assert pops == {("sac_gail_F12", 3, 192, (48, 32)), ("free_breathing", 2, 128, (16, 64)), ("single_food", 4, 256, ())}
    # the clamp entries: two-component snake shapes and a robot shape; exactly one component beyond a clamp; both clamps used
    clamps = [(k, e) for k, e in gm.ALL.items() if e["clamped"]]
    assert len(clamps) == 3 and sum(gm.is_robot(k) for k, _ in clamps) == 1
    signs = set()
    for k, e in clamps:
        assert len(e["clamped"]) == 1 and len(e["b_ls"]) >= 2
        beyond = [j for j, b in enumerate(e["b_ls"]) if not -20.0 < b < 2.0]
        assert beyond == list(e["clamped"]), k
        signs.add(e["b_ls"][beyond[0]] > 0)
    assert signs == {True, False}
    assert all(not e["clamped"] or gm.case_cfg(e["case"]).act_dim == 2 for e in E.values())
    # the robot: six shapes at 128 envs (48x32 at 100), one population of two, three clip entries
    R = gm.ROBOT_ENTRIES
    assert {(e["hidden"], e["n"]) for e in R.values() if e["kind"] == "gaussian" and e["P"] == 1 and not e["clamped"]} == \
        {((), 128), ((16,), 128), ((64,), 128), ((16, 64), 128), ((48, 32), 100), ((64, 64), 128)}
    assert [e["P"] for e in R.values() if e["P"] > 1] == [2] and len(gm.ROBOT_CLIP) == 3
    assert (gm.ROBOT_H, gm.ROBOT_MAX_CYCLES) == (7, 3) and gm.BASE == 2 ** 32 + 320
    # the once-only runs name entries of the right kind
    assert [gm.entry_cfg(k).act_dim for k in gm.BASE_ENTRIES] == [1, 2, 1] and gm.ENTRIES[gm.BASE_ENTRIES[2]]["kernel"][0] == 12
    kinds = [m for _, m in gm.UPLOADED_MUTANTS]
    assert any("chunk" in m for m in kinds) and any("takes_row" in m for m in kinds) and any("stride" in m for m in kinds)
    for name, label in gm.UPLOADED_MUTANTS:
        assert label in gm.weight_mutants(gm.entry_policy(name)) and not gm.ENTRIES[name]["clamped"]
    assert all(e["n"] <= 256 for e in gm.ALL.values())


@pytest.mark.parametrize("generation", [0, 1])
@pytest.mark.parametrize("name", SNAKE + ROBOT)
def test_weights_are_dense_distinct_and_the_log_std_head_is_too(name, generation):
    pop = gm.entry_policy(name, generation)
    assert isinstance(pop, GaussianPolicy) and pop.hidden == gm.ALL[name]["hidden"]
    w = pop.pack()
    A = pop.act_dim
    body = w[:, :-2 * A]                                    # everything but scale and shift (the robot's Box has a shift of 0)
    assert w.shape == (gm.ALL[name]["P"], pop.words) and (body != 0).all() and np.isfinite(w).all()
    for row in body:                                        # within one policy no two words are equal
        assert np.unique(row).size == row.size
    for k in range(1, w.shape[0]):                          # the policies of a population differ in every word, log-std included
        assert (body[k] != body[k - 1]).all()
    if generation == 1:
        assert (body != gm.entry_policy(name, 0).pack()[:, :-2 * A]).all()
    L = gm.gaussian_layout(pop)                             # the layout the mutants index is the one `pack` writes
    assert np.array_equal(w[:, L["W_ls"]:L["b_ls"]], pop.log_std[0].reshape(w.shape[0], -1))
    assert np.array_equal(w[:, L["b_ls"]:L["b_ls"] + A], pop.log_std[1]) and L["b_ls"] + 3 * A == pop.words
    assert np.array_equal(w[:, L["W_mu"]:L["b_mu"]], pop.layers[-1][0].reshape(w.shape[0], -1))


@pytest.mark.parametrize("name", ["single_food-linear-n128", "free_breathing-16x48-n128", "sac_gail_F12-48x32-n192-P3", "robot-linear-n128",
                                  "robot-48x32-n100", "robot-16x64-n128-P2"])
def test_the_gaussian_restatement_is_the_deterministic_one_of_each_head(name):
    """m and r of salp_oracle_policy_forward_gaussian are the bits of salp_oracle_policy_forward's u — for the mean policy,
    and for the policy whose last layer is the log-std head — and of the numpy restatement `policy_matrix.py_forward`; with
    three action components too, which salp_oracle_policy_forward refused before."""
    r = gm.closed_loop(name)
    policy, seen = r["policy"], r["obs_in"][::3]
    m, rr, sub = ol.policy_forward_gaussian(policy, seen)
    assert sub == 0 and m.dtype == rr.dtype == np.float32 and m.shape == rr.shape == seen.shape[:-1] + (policy.act_dim,)
    mean = policy.mean_policy()
    as_ls = MLPPolicy(policy.layers[:-1] + [policy.log_std], policy.scale, policy.shift, "tanh")
    for head, values in ((mean, m), (as_ls, rr)):
        u, _, s = ol.policy_forward(head, seen)
        assert s == 0 and np.array_equal(bits(u), bits(values))
        pu, _ = pm.py_forward(head, head.pack(), seen)
        assert np.array_equal(bits(pu), bits(values))
    assert not np.array_equal(m, rr)
    # a clip policy of the same body: the whole chain in bits, three components included
    clip = MLPPolicy(policy.layers, policy.scale, policy.shift, "clip")
    u, a, _ = ol.policy_forward(clip, seen)
    pu, pa = pm.py_forward(clip, clip.pack(), seen)
    assert np.array_equal(bits(u), bits(m)) and np.array_equal(bits(pa), bits(a))
    with pytest.raises(ValueError):
        ol.policy_forward_gaussian(mean, seen)


def _fp32_from_heads(p, m, r, z32):
    """The library's sampling arithmetic behind the heads, restated in numpy float32 on the host (libm in place of the
    device library), for one policy."""
    f = np.float32
    ls = np.clip(r, f(-20), f(2))
    sd = np.exp(ls)
    u = (sd.astype(np.float64) * z32 + m).astype(f)               # one rounding: the fma
    a = np.tanh(u) * p.scale[0] + p.shift[0]
    m2 = f(-2) * u
    sp = np.maximum(m2, f(0)) + np.log1p(np.exp(-np.abs(m2)))
    c = (f(0.693147180559945309) - u) - sp
    g = f(-0.5) * (z32 * z32)
    g = g - ls
    g = g - f(0.918938533204672742)
    g = g - f(2) * c
    lp = g[..., 0]
    for k in range(1, g.shape[-1]):
        lp = lp + g[..., k]
    assert a.dtype == lp.dtype == f
    return a, lp


@pytest.mark.parametrize("name", ["single_food-32x32-n128", "free_breathing-32x48-n128-clamp0hi", "free_breathing-48x16-n128-clamp1lo",
                                  "robot-64x64-n128", "robot-64-n128-clamp1lo"])
def test_the_stage_bound_covers_an_fp32_evaluation_from_the_same_heads_and_is_tight(name):
    r = gm.closed_loop(name)
    policy, z, m, rr = r["policy"], r["z"], r["m"], r["r"]
    s = gm.stage(policy, m, rr, z)
    a, lp = _fp32_from_heads(policy, m, rr, z.astype(np.float32))
    assert not gm.outside(a, lp, s).any(), (np.abs(a - s["a"]) / s["ea"]).max()
    assert (s["ea"] > 0).all() and (s["el"] > 0).all()
    # a mean head off by 2^-16 of its value (128 units in the last place) is outside it on most rows
    moved_m = gm.stage(policy, (m * np.float32(1.0 + 2.0 ** -16)).astype(np.float32), rr, z)
    ea, el = policy.error_bound(r["obs_in"], z)
    lively = [k for k in range(policy.act_dim) if k not in r["e"]["clamped"]]
    assert (np.abs(moved_m["a"] - s["a"]) > s["ea"])[..., lively].mean() > 0.5
    # with nothing carried in it is far below the forward bound
    assert (s["ea"] <= ea).all() and (s["el"] <= el).all() and np.median(s["ea"] / ea) < 0.5


def _report(name, base=0):
    fig, fails = gm.guard(name, base)
    print(f"{name}{' at base 2^32 + 320' if base else ''}: {fig}")
    assert not fails, fails


@pytest.mark.parametrize("name", SNAKE)
def test_snake_entry_on_the_oracle(name):
    r = gm.closed_loop(name)
    e, cfg, policy = r["e"], r["cfg"], r["policy"]
    assert policy.act_dim == cfg.act_dim and policy.obs_dim == cfg.obs_dim == 24 and policy.n_policies == e["P"]
    assert np.array_equal(r["obs_in"][1:], r["outs"]["obs"][:-1])                # the chain is closed
    ev = gm.pc.count_events(r["outs"])                                           # the events criterion of the deterministic matrix
    assert ev["wall"] + ev["truncated"] + ev["completed"] >= 1 and ev["mixed_wave_steps"] >= 1, ev
    _report(name)


@pytest.mark.parametrize("name", ROBOT)
def test_robot_entry_on_the_robot_oracle(name):
    r = gm.closed_loop(name)
    assert r["policy"].act_dim == 3 and r["policy"].obs_dim == 6
    assert np.array_equal(r["obs_in"][1:], r["outs"]["obs"][:-1])
    assert np.ptp(r["outs"]["inner_steps"][:, :64]) > 50, "cycle lengths must differ inside a wavefront"
    _report(name)


@pytest.mark.parametrize("name", BASE_RUNS)
def test_entry_at_the_env_base_and_the_local_index_mutant(name):
    """The same entry with its envs at global indices 2^32 + 320 ..: another start state, other noise — and the noise of
    the LOCAL index is far outside the bound, as the GPU test asserts of the device's actions."""
    _report(name, gm.BASE)
    r0, r = gm.closed_loop(name), gm.closed_loop(name, gm.BASE)
    assert not np.array_equal(r0["z"], r["z"]) and not np.array_equal(r0["obs_in"][0], r["obs_in"][0])
    assert gm.local_index_share(r["policy"], r["obs_in"], r["actions"], 0, gm.key_of(name)) > gm.sc.OFF_BY_ONE_SHARE


@pytest.mark.parametrize("name", gm.ROBOT_CLIP)
def test_robot_clip_entry_on_the_robot_oracle(name):
    r = gm.robot_clip_closed_loop(name)
    policy, u = r["policy"], r["u"].reshape(-1, 3).astype(np.float64)
    assert policy.out == "clip" and type(policy) is MLPPolicy and r["subnormals"] == 0
    ends, mixed = gm.mixed_wave_steps(r["outs"])
    open_ = (np.abs(u) < 1.0).mean(axis=0)
    print(f"{name}: {ends} endings, {mixed} mixed wavefront-steps, unsaturated {np.round(open_, 3).tolist()}, u in [{u.min():.3g}, {u.max():.3g}]")
    assert ends >= 1 and mixed >= 1 and (open_ >= gm.NOT_BLIND).all()
    assert ((u > 1.0).any(axis=0) & (u < -1.0).any(axis=0)).all()             # and both clamps are reached, per component
    w = policy.pack()
    assert (w[:, :-6] != 0).all() and np.unique(w[0, :-6]).size == w.shape[1] - 6
