"""CPU guard of the GPU parity tests' recipe (tests/parity_cases.py): the oracle alone, over the shared case table with
the shared start state, must produce the events the GPU tests exist to compare — wall terminations, truncations, food
captures, wavefronts in which some lanes finish and others go on, envs that finish twice.  Editing a seed, a preset or the
recipe on a machine without a GPU cannot quietly take them away."""
import numpy as np
import pytest

import parity_cases as pc


@pytest.mark.parametrize("name", list(pc.CASES))
def test_recipe_ends_episodes_on_the_oracle(name):
    cfg = pc.case_cfg(name)
    orc, f64, i32 = pc.start_oracle(cfg, pc.N_ENVS, pc.ENV_SEED)
    ref = orc.rollout(pc.make_actions(cfg, pc.HORIZON, pc.N_ENVS, seed=pc.ACTION_SEED), want_final=True)
    ev = pc.count_events(ref)
    print(f"{name}: {ev}")
    assert name in pc.FLOORS and name in pc.EXPECT_KERNEL
    assert all(pc.floors_for(name)[k] >= v for k, v in pc.MIN_FLOORS.items() if not (k == "captures" and cfg.num_food_items == 0))
    pc.assert_event_floors(name, ev)
    assert ev["wall_steps"] >= 20, f"{name}: wall terminations on {ev['wall_steps']} distinct steps only"
    done = (ref["terminated"] | ref["truncated"]).astype(bool)
    assert np.array_equal(np.isnan(ref["final_obs"][..., 0]), ~done)
    if name == "no_respawn_F3":
        assert pc.steps_left_short_of_foods(cfg, ref) >= pc.NO_RESPAWN_SHORT_STEPS_FLOOR, pc.steps_left_short_of_foods(cfg, ref)
        lanes = pc.completion_lanes(pc.N_ENVS)
        third = ref["terminated"][2].astype(bool) & (ref["info"][2, :, pc.INFO_COLLISION] == 0)
        assert third[lanes].all(), "completion lanes terminate by completion on their third step"
    orc.close()


def test_plain_reset_would_leave_the_terminal_branch_untested():
    """What the recipe is for: without it (reset state, the presets' own budgets) most cases finish no episode at all."""
    dead = 0
    for name in pc.CASES:
        cfg = pc.case_cfg(name, budget=None)
        orc = pc.ol.OracleVec(cfg, pc.N_ENVS, seed=pc.ENV_SEED)
        ref = orc.rollout(pc.make_actions(cfg, pc.HORIZON, pc.N_ENVS, seed=pc.ACTION_SEED))
        ev = pc.count_events(ref)
        assert ev["wall"] == 0, name
        dead += (ev["wall"] + ev["truncated"] + ev["completed"]) == 0
        orc.close()
    assert dead >= 17


@pytest.mark.parametrize("name", list(pc.STEP_CASES))
def test_step_recipe_has_every_event_on_the_oracle(name):
    cfg, orc, f64, i32, act = pc.step_case(name)
    ev = pc.count_events(orc.rollout(act))
    print(f"step case {name}: {ev}")
    assert name in pc.STEP_FLOORS
    pc.assert_step_floors(name, ev)
    orc.close()
