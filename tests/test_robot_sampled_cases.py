"""The recipe guard of the robot's sampled GPU cases (tests/robot_sampled_cases.py): on the oracle alone, driven closed loop
under `reference(obs, z)`, every case must keep both error bounds below their ceilings, tell a wrong noise step from the
right one, and spread its cycle lengths inside a wavefront — so that the GPU comparison means something.  No GPU needed."""
import numpy as np
import pytest

import robot_sampled_cases as cases


def test_the_case_table():
    assert [tuple(c["hidden"]) for c in cases.CASES.values()] == [(), (16,), (32, 16), (64, 64)]
    assert cases.LOGP_BOUND_CEILING_PER_COMPONENT == 2.9e-3 and cases.BOUND_CEILING == 1e-4
    assert float(cases.SCALE.min()) == np.float32(0.075)
    for name in cases.CASES:
        p = cases.case_policy(name)
        assert p.gaussian and (p.obs_dim, p.act_dim, p.n_policies) == (6, 3, 1) and p.hidden == tuple(cases.CASES[name]["hidden"])
        assert np.array_equal(p.scale[0], cases.SCALE) and np.array_equal(p.shift[0], cases.SHIFT)
        b = p.log_std[1][0]
        clamped = cases.floor_clamped_components(p)
        if name == cases.CLAMPED:
            assert b[0] > 2.0 and b[1] < -24.0 and -3.0 <= b[2] <= 0.0 and list(clamped) == [1]
        else:
            assert (-3.0 <= b).all() and (b <= 0.0).all() and clamped.size == 0


@pytest.mark.parametrize("name", list(cases.CASES))
def test_sampled_closed_loop_recipe_on_the_oracle(name):
    policy, z, seen, actions, logp, inner = cases.oracle_closed_loop(name)
    ea, el = policy.error_bound(seen, z)
    share = cases.off_by_one_share(policy, seen, actions)
    print(f"{name}: bounds: action {ea.max():.3g}, logp {el.max():.3g}; logp in [{logp.min():.3f}, {logp.max():.3f}]; "
          f"off-by-one share {share:.3f}; inner steps {inner.min()}..{inner.max()}, spread in wavefront 0: {np.ptp(inner[:, :64])}")
    assert np.isfinite(actions).all() and np.isfinite(logp).all()
    assert ea.max() < cases.BOUND_CEILING, ea.max()
    assert el.max() < 3 * cases.LOGP_BOUND_CEILING_PER_COMPONENT, el.max()
    assert share > cases.OFF_BY_ONE_SHARE, share
    lo, hi = cases.SHIFT - cases.SCALE, cases.SHIFT + cases.SCALE
    assert np.all(actions >= lo) and np.all(actions <= hi)
    # cycle lengths differ inside a wavefront, in every wavefront and on every step
    for w in range(0, cases.N, cases.WAVE):
        assert np.ptp(inner[:, w:w + cases.WAVE], axis=1).min() > 50, w
    # the log-std head where the table says: about [-3, 0] — or beyond both clamps, by more than the head's weights can undo
    x = seen.astype(np.float64)
    for W, b in policy.layers[:-1]:
        x = np.maximum(x @ W[0].astype(np.float64).T + b[0], 0.0)
    wh = x @ policy.log_std[0][0].astype(np.float64).T
    assert np.abs(wh).max() < 4.0
    ls = wh + policy.log_std[1][0]
    if name == cases.CLAMPED:
        assert ls[..., 0].min() > 2.0 and ls[..., 1].max() < -20.0
        # the floor-clamped component takes its mean action, whatever the noise
        assert np.abs(actions[..., 1] - policy.mean_policy().reference(seen)[..., 1]).max() < 1e-7
        ls = ls[..., 2]
    assert -3.6 < ls.min() and ls.max() < 0.6
