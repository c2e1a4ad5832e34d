"""CPU guard of the vectors generated off the reference's default constants (tests/golden/ref_rt_*.npz, gen_golden.py
`rt_cases`).  Oracle only, no GPU.

A vector pins a run-time constant only if the constant shows in it: an oracle (or a kernel) that ignored `food_radius` would
still match a vector whose swimmers never come near a food.  So for every vector and every one of the thirteen run-time
values it stores off its default, the oracle is run once more with THAT value put back to its default — everything else as
stored, the injected state included — and the env-steps whose observation, reward or flags then differ from the vector
are counted.  Every value but `rest_duration` must change at least 100 env-steps (of 4000) in at least one vector.

`rest_duration` must change none: the reference restarts `breathing_timer` at every change of phase (salp_robot.py:196,
221, 227, 258), so the timer never exceeds max(inhale_duration, exhale_duration + 1), which is below the modulus
inhale + exhale + rest of the forced-breathing schedule (:161-162): `timer % modulus` is the timer itself whatever
`rest_duration` is.  The value is dead in the reference, and the configuration field is tested for exactly that.

The same file asserts, from the stored arrays, the events the vectors were made to hold (golden_util.RT_*)."""
import os

import numpy as np
import pytest

import golden_util as gu
import oracle_lib as ol

NAMES = gu.rt_fixture_names()
MIN_CHANGED, ENVS, MAX_STEPS = 100, 16, 250


@pytest.fixture(scope="module")
def vectors():
    return {name: gu.load_fixture(name) for name in NAMES}


def oracle_steps_differing(z, meta, cfg):
    """[H, n] mask: the oracle under `cfg`, from the vector's injected state, differs from the vector in obs, reward or flags."""
    n = z["actions"].shape[1]
    orc = ol.OracleVec(cfg, n, seed=meta["seed"], env_index_base=meta["env_index_base"])
    orc.set_state(z["inject_f64"], z["inject_i32"])
    out = orc.rollout(z["actions"], want_final=True)
    orc.close()
    with np.errstate(invalid="ignore"):
        obs_same = ((out["obs"] == z["obs"]) | (np.isnan(out["obs"]) & np.isnan(z["obs"]))).all(axis=2)
    return ~obs_same | (out["reward64"] != z["reward"]) | (out["terminated"] != z["terminated"]) | (out["truncated"] != z["truncated"])


def test_the_set_is_the_six_kernel_classes(vectors):
    assert sorted(NAMES) == sorted(gu.RT_KERNEL)
    assert sorted(gu.RT_KERNEL.values()) == [(1, 3, 0), (4, 3, 0), (8, 3, 0), (12, 3, 0), (12, 8, 0), (16, 3, 0)]
    largest = os.path.getsize(os.path.join(gu.GOLDEN_DIR, "ref_wall_events.npz"))
    for name, (z, meta, cfg) in vectors.items():
        H, n, _ = z["actions"].shape
        assert n == ENVS and H <= MAX_STEPS, name
        assert os.path.getsize(os.path.join(gu.GOLDEN_DIR, f"ref_{name}.npz")) <= largest, name
        slots, cap, _ = gu.RT_KERNEL[name]
        assert cfg.num_food_items <= slots and (cap == 3) == (cfg.max_observed_food == 3), name
        assert cfg.angular_drag == 0.95 and any(getattr(cfg, k) != gu.DEFAULTS[k] for k in gu.RUNTIME_VALUES), name
        # the stored constants are exactly the non-default ones, and they reached the configuration
        assert {k: meta[k] for k in gu.CONSTANTS if k in meta} == gu.non_default_constants(cfg), name


def test_oracle_agrees_with_the_stored_configuration(vectors):
    """The counter counts nothing when nothing is changed (test_oracle_golden.py holds the full bit-for-bit comparison)."""
    for name, (z, meta, cfg) in vectors.items():
        assert not oracle_steps_differing(z, meta, cfg).any(), name


def test_every_runtime_value_shows_in_the_vectors(vectors):
    changed = {k: {} for k in gu.RUNTIME_VALUES}
    for name, (z, meta, cfg) in vectors.items():
        for k in gu.RUNTIME_VALUES:
            if getattr(cfg, k) != gu.DEFAULTS[k]:
                back = gu.cfg_from_meta(meta, **{k: gu.DEFAULTS[k]})
                assert getattr(back, k) == gu.DEFAULTS[k]
                changed[k][name] = int(oracle_steps_differing(z, meta, back).sum())
    for k, per in changed.items():
        print(f"{k:22s} back to {gu.DEFAULTS[k]!r:>20}: env-steps changed " + ", ".join(f"{n[3:]} {c}" for n, c in per.items()))
    for k, per in changed.items():
        assert per, f"{k} is at its default in every vector"
        if k == "rest_duration":
            assert set(per.values()) == {0}, f"rest_duration shows in the reference's vectors after all: {per}"
        else:
            assert max(per.values()) >= MIN_CHANGED, f"{k} changes at most {max(per.values())} env-steps: {per}"


def test_events_the_vectors_were_made_for(vectors):
    events, clamps = {}, {}
    for name, (z, meta, cfg) in vectors.items():
        events[name] = gu.rt_events(cfg, z)
        clamps[name] = int(z["wall_clamp_without_collision"].sum())
        print(f"{name:18s} {events[name]} clamps without collision {clamps[name]}")
        gu.check_rt_case(name, events[name])
        assert z["wall_clamp_without_collision"].shape == z["terminated"].shape
        assert not (z["wall_clamp_without_collision"].astype(bool) & (z["info"][..., gu.INFO_COLLISION] != 0)).any()
    gu.check_rt_set(events, clamps)


def test_start_states_head_for_the_four_walls(vectors):
    """Env i heads for wall i % 4, body edge at its widest (1.3 base_radius) 3 to 60 px away, at 0.3 to 3 px/step."""
    for name, (z, meta, cfg) in vectors.items():
        f = z["inject_f64"]
        lo = cfg.tank_margin + 1.3 * cfg.base_radius
        for i in range(f.shape[1]):
            gap, speed = ((f[ol.F_X, i] - lo, -f[ol.F_VX, i]), (cfg.width - lo - f[ol.F_X, i], f[ol.F_VX, i]),
                          (f[ol.F_Y, i] - lo, -f[ol.F_VY, i]), (cfg.height - lo - f[ol.F_Y, i], f[ol.F_VY, i]))[i % 4]
            assert 3.0 - 1e-9 <= gap <= 60.0 + 1e-9 and 0.3 <= speed <= 3.0, (name, i, gap, speed)


def test_oracle_clamps_without_collision_where_the_reference_did(vectors):
    """The reference's `wall_clamp_without_collision` steps (position exactly on the clamp line after the step, no collision
    reported: `(margin + r) - r <= margin` decided by rounding), found again in the oracle's fp64 state step by step."""
    for name, (z, meta, cfg) in vectors.items():
        act = z["actions"]
        H, n, _ = act.shape
        orc = ol.OracleVec(cfg, n, seed=meta["seed"], env_index_base=meta["env_index_base"])
        orc.set_state(z["inject_f64"], z["inject_i32"])
        got = np.zeros((H, n), bool)
        done = (z["terminated"] | z["truncated"]).astype(bool)
        for t in range(H):
            out = orc.step(act[t], want_final=True)
            f, _ = orc.get_state()
            m = cfg.tank_margin + np.maximum(f[ol.F_ELLIPSE_A], f[ol.F_ELLIPSE_B])
            x, y = f[ol.F_X], f[ol.F_Y]
            on_line = (x == m) | (x == cfg.width - m) | (y == m) | (y == cfg.height - m)
            got[t] = on_line & (out["info"][:, gu.INFO_COLLISION] == 0) & ~done[t]       # a finished env shows its reset state
        orc.close()
        assert np.array_equal(got, z["wall_clamp_without_collision"].astype(bool) & ~done), name
