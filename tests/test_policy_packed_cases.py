"""CPU guard of tests/policy_packed_cases.py: on the oracle alone, stepped closed-loop under each added case's own policy
from the injected start state, every case ends an episode by wall and one by truncation and has a wavefront-step that mixes
finished and unfinished lanes — so the terminal-tail branch of the packed policy kernels is never compared with nothing.
The six cases the table takes over are held to the same condition by tests/test_policy_rollout.py.  No GPU needed."""
import pytest

import parity_cases as pc
import policy_cases as dc
import policy_packed_cases as cases


def test_the_table_extends_the_closed_loop_table():
    assert list(cases.CASES)[:len(dc.CASES)] == list(dc.CASES) and all(cases.CASES[k] is dc.CASES[k] for k in dc.CASES)
    assert len(cases.ADDED) == 5
    for name in cases.ADDED:
        c = cases.CASES[name]
        assert (c["seed"], c["gain"], c["out_gain"]) == (123, 1.5, 6.0)
        assert c["predicated"] == (c["n"] % cases.WAVE != 0) and c["n"] * cases.H <= 1 << 22     # a ragged small batch: one predicated launch
    assert set(cases.SAMPLED) <= set(cases.CASES) and set(cases.NARROW) <= set(cases.CASES)
    # the handle classes of the whole table: every slot count, both kinds of constants at 8, 12 and 16 slots, a predicated 8-slot case
    kernels = {(c["kernel"], c["predicated"]) for c in cases.CASES.values()}
    assert {k for k, _ in kernels} >= {(1, 1), (4, 0), (8, 1), (8, 0), (12, 1), (12, 0), (16, 1), (16, 0)}
    assert ((8, 1), True) in kernels and ((1, 1), True) in kernels
    assert not cases.case_cfg("other_tank_F5_free").forced_breathing


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_expected_kernel_is_the_parity_table_s(name):
    c = cases.CASES[name]
    slots, k, literal = pc.EXPECT_KERNEL[c["case"]]
    assert k == 3 and c["kernel"] == (slots, literal)
    cfg = cases.case_cfg(name)
    p = cases.case_policy(name)
    assert (p.obs_dim, p.act_dim) == (cfg.obs_dim, cfg.act_dim) and cfg.max_observed_food == 3


@pytest.mark.parametrize("name", cases.ADDED)
def test_every_added_case_ends_episodes_both_ways_in_mixed_wavefronts(name):
    cfg, policy, actions, outs = cases.oracle_closed_loop(name)
    ev = pc.count_events(outs)
    print(f"{name}: {ev}")
    cases.assert_events(name, ev)


@pytest.mark.parametrize("name", cases.SAMPLED)
def test_the_gaussian_twins_fit_their_cases(name):
    cfg, g = cases.case_cfg(name), cases.gaussian_twin(name)
    assert g.gaussian and (g.obs_dim, g.act_dim) == (cfg.obs_dim, cfg.act_dim)
    assert tuple(g.hidden) == tuple(cases.CASES[name]["hidden"])
