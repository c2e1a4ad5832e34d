"""The CPU guard of the policy matrix (tests/policy_matrix.py, run on the GPU by tests/test_gpu_policy_matrix.py): the table
covers what it must; on the oracle alone, stepped closed-loop under the C restatement of the policy
(`oracle_lib.policy_forward`), every entry ends episodes in mixed wavefronts, keeps its outputs out of saturation, forms no
subnormal, and agrees with the independent float64 statement `MLPPolicy.reference`; and every mutant of the restatement —
a wrong stride, a dropped chunk, a swapped pair of weights, another summation order — changes the actions the GPU test
compares."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
import policy_matrix as pm
from support import bits

NOT_BLIND = 0.25            # of the visited rows, per action component, must be out of saturation
NAMES = list(pm.ENTRIES)


def test_the_table_covers_what_it_must():
    E = pm.ENTRIES.values()
    sweep = {"single_food": {}, "free_breathing": {}}
    for e in E:
        if e["case"] in sweep and e["P"] == 1 and e["n"] == 128:
            sweep[e["case"]][e["hidden"]] = e["out"]
    for case, seen in sweep.items():                       # all 21 shapes on both one-food cases, both activations in each
        assert set(seen) == set(pm.SHAPES) and set(seen.values()) == {"tanh", "clip"}, case
    assert all(sweep["single_food"][s] != sweep["free_breathing"][s] for s in pm.SHAPES)
    assert pc.case_cfg("single_food").act_dim == 1 and pc.case_cfg("free_breathing").act_dim == 2
    families = ("sac_gail_F12", "other_physics_F12", "no_respawn_F3", "F3_other_tank", "class_default_F5", "other_tank_F5_free",
                "F16_sixteen_slots", "F16_sixteen_slots_other_tank", "other_tank_F1")
    for case in families:
        have = {(e["n"], e["hidden"]) for e in E if e["case"] == case and e["P"] == 1}
        assert {(128, (64, 64)), (128, (48, 32)), (128, (16, 64)), (100, (48, 32))} <= have, case
    # those cases are every policy kernel family: 1, 4, 8, 12 and 16 slots, each with literal and with run-time constants
    assert {pm.ENTRIES[n]["kernel"] for n in NAMES} == {(s, l) for s in (1, 4, 8, 12, 16) for l in (0, 1)}
    pops = {(e["case"], e["P"], e["hidden"], e["n"], e["out"]) for e in E if e["P"] > 1}
    assert {p[:4] for p in pops} == {("sac_gail_F12", 3, (48, 32), 192), ("free_breathing", 2, (16, 64), 128), ("single_food", 4, (), 256)}
    assert ("single_food", 4, (), 256, "clip") in pops
    assert all(e["n"] <= 256 for e in E) and pm.H + pm.UPDATE_STEPS <= 72
    assert {pm.ENTRIES[n]["kernel"][0] for n in pm.DEVICE_WEIGHT_ENTRIES} == {1, 8, 16}


@pytest.mark.parametrize("generation", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_weights_are_dense_distinct_and_rescaled(name, generation):
    pop = pm.entry_policy(name, generation)
    w = pop.pack()
    assert w.shape == (pm.ENTRIES[name]["P"], pop.words) and (w != 0).all() and np.isfinite(w).all()
    for row in w:                                           # within one policy no two words are equal
        assert np.unique(row).size == row.size
    for k in range(1, w.shape[0]):                          # and the policies of a population differ in every word but scale / shift
        assert (w[k, :-2 * pop.act_dim] != w[k - 1, :-2 * pop.act_dim]).all()
    assert (pop.scale != 1).all() and (pop.shift != 0).all() and (pop.scale != pop.shift).all()
    if pop.act_dim == 2:
        assert (pop.scale[:, 0] != pop.scale[:, 1]).all() and (pop.shift[:, 0] != pop.shift[:, 1]).all()
    if generation == 1:
        assert (w[:, :-2 * pop.act_dim] != pm.entry_policy(name, 0).pack()[:, :-2 * pop.act_dim]).all()


@pytest.mark.parametrize("name", NAMES)
def test_entry_on_the_oracle(name):
    r = pm.oracle_closed_loop(name)
    e, cfg, policy, obs_in, u, a, outs = r["e"], r["cfg"], r["policy"], r["obs_in"], r["u"], r["a"], r["outs"]
    assert pc.EXPECT_KERNEL[e["case"]][::2] == e["kernel"] and policy.hidden == e["hidden"] and policy.out == e["out"]
    assert policy.act_dim == cfg.act_dim and policy.obs_dim == cfg.obs_dim == 24 and policy.n_policies == e["P"]
    # the restatement is the independent float64 statement, within its forward bound, on every visited row
    err = np.abs(a.astype(np.float64) - policy.reference(obs_in))
    bound = policy.error_bound(obs_in)
    assert (err <= bound).all(), f"worst ratio {(err / bound).max()}"
    # the chain is closed
    assert np.array_equal(obs_in[1:], outs["obs"][:-1])
    # episodes end, next to running ones
    ev = pc.count_events(outs)
    assert ev["wall"] + ev["truncated"] + ev["completed"] >= 1 and ev["mixed_wave_steps"] >= 1, ev
    # not blind: enough rows out of saturation, both signs, per component
    uu = u.reshape(-1, cfg.act_dim).astype(np.float64)
    open_ = np.abs(uu) < 1.0 if policy.out == "clip" else np.abs(np.tanh(uu)) < 0.999
    frac = open_.mean(axis=0)
    print(f"{name}: {ev}; unsaturated {np.round(frac, 3).tolist()}, u in [{uu.min():.3g}, {uu.max():.3g}], "
          f"restatement / reference: error {err.max():.3g}, bound {bound.max():.3g}")
    assert (frac >= NOT_BLIND).all(), frac
    assert ((uu > 0).any(axis=0) & (uu < 0).any(axis=0)).all()
    # no subnormal anywhere in the restatement (the kernel may flush them; the header does not say)
    assert r["subnormals"] == 0
    if policy.out == "tanh":     # the tanh stage's own bound is part of the forward bound, and far below it for dense weights
        want, tb = pm.tanh_stage_bound(policy, u)
        assert (tb <= bound).all() and (np.abs(a.astype(np.float64) - want) <= tb).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_shows(name):
    r = pm.oracle_closed_loop(name)
    policy = r["policy"]
    seen = r["obs_in"][::pm.MUTANT_STEP_STRIDE]
    u0, a0 = r["u"][::pm.MUTANT_STEP_STRIDE], r["a"][::pm.MUTANT_STEP_STRIDE]
    w0 = policy.pack()
    # the numpy forward IS the restatement: u always, the action where no tanhf is involved
    pu, pa = pm.py_forward(policy, w0, seen)
    assert np.array_equal(bits(pu), bits(u0))
    if policy.out == "clip":
        assert np.array_equal(bits(pa), bits(a0))
    shown = {}
    for label, w in pm.weight_mutants(policy).items():
        assert w.shape == w0.shape and not np.array_equal(w, w0)
        _, am, _ = ol.policy_forward(policy, seen, weights=w)
        shown[label] = int((am != a0).any(axis=-1).sum())
    if len(policy.hidden) == 2:
        shown["no_relu_on_hidden1"] = int((pm.py_forward(policy, w0, seen, relu=(True, False))[1] != pa).any(axis=-1).sum())
    if policy.out == "clip":     # in BITS: the comparison on the GPU is known to see the order of summation
        ad = pm.py_forward(policy, w0, seen, descending=True)[1]
        shown["descending_order"] = int((bits(ad) != bits(a0)).any(axis=-1).sum())
    print(f"{name}: rows changed of {seen.shape[0] * seen.shape[1]}: {shown}")
    two, hid, A = len(policy.hidden) == 2, policy.hidden, policy.act_dim
    expect = {"inputs_16_23_dropped", "scale_shift_exchanged", "two_weights_swapped_within_a_row", "two_weights_swapped_across_chunks"}
    expect |= {f"hidden{l}_last_chunk_dropped" for l in range(len(hid))}
    if two and hid[0] != hid[1]:
        expect |= {"layer1_input_stride_h1"} | ({"last_layer_row_stride_h0"} if A == 2 else set())
    if A == 2:
        expect |= {f"component1_takes_component0_{k}" for k in ("b_last", "scale", "shift")}
    if two:
        expect.add("no_relu_on_hidden1")
    if policy.out == "clip":
        expect.add("descending_order")
    if policy.n_policies > 1:
        expect.add("policy_k_takes_policy_k_minus_1")
    assert set(shown) == expect
    assert all(v >= pm.MUTANT_ROWS for v in shown.values()), {k: v for k, v in shown.items() if v < pm.MUTANT_ROWS}
