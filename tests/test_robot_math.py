"""The robot kernels' fp64 primitives (csrc/salp_fp64_math.h) against mpmath at 256 bits, through the host twin
(tests/robot_math_host.cpp: the same header compiled for the CPU; tests/test_gpu_robot_math.py holds the device to it
bit for bit).  Every bound here is one the header or DESIGN.md §8f-4 states.  Worst cases are printed (pytest -s)."""
import math

import numpy as np
import pytest

import robot_math_cases as cases
import robot_math_lib as ml

ULP1 = cases.ULP1


def _report(what, worst, bound):
    print(f"{what}: worst {worst:.3g}, bound {bound:.3g} ({worst / bound:.2f} of it)")


@pytest.mark.parametrize("limit", cases.SMALL_RANGES)
def test_sincos_small_is_within_one_ulp_of_one_up_to_1e9(limit):
    x = cases.small_range_points(limit)
    s, c = ml.host(ml.SINCOS_SMALL, x)
    err = cases.sincos_error(x, s, c)
    _report(f"sincos_small |x| <= {limit:g}", err.max(), ULP1)
    assert err.max() <= ULP1, x[err.argmax()]


def test_sincos_small_next_to_zeros_and_quadrant_switches():
    x = cases.small_edge_points()
    s, c = ml.host(ml.SINCOS_SMALL, x)
    err = cases.sincos_error(x, s, c)
    _report(f"sincos_small at {len(x)} edge points", err.max(), ULP1)
    assert err.max() <= ULP1, x[err.argmax()]
    z = ml.host(ml.SINCOS_SMALL, np.array([0.0, -0.0]))
    assert np.all(z[0] == 0.0) and np.all(z[1] == 1.0)


def test_sincos_euler_fold_is_within_two_ulps_of_one_up_to_1e15():
    x = cases.euler_points()
    s, c = ml.host(ml.SINCOS_EULER, x)
    err = cases.sincos_error(x, s, c)
    _report("sincos_euler 1e8 < |x| <= 1e15", err.max(), 2 * ULP1)
    assert err.max() <= 2 * ULP1, x[err.argmax()]


def test_sincos_euler_on_both_sides_of_the_fold_switch():
    t = ml.euler_fold_above()
    assert t == 1e8
    x = cases.euler_switch_points(t)
    s, c = ml.host(ml.SINCOS_EULER, x)
    err = cases.sincos_error(x, s, c)
    _report("sincos_euler around the switch", err.max(), 2 * ULP1)
    assert err.max() <= 2 * ULP1, x[err.argmax()]
    # a group with no lane above the switch does not fold: exactly sincos_small, and within its bound
    plain = ml.host(ml.SINCOS_SMALL, x)
    assert np.array_equal(plain[:, :64], np.stack([s, c])[:, :64]) and err[:64].max() <= ULP1
    # one lane above it folds the whole group: the small angles of that group take the fold too
    assert not np.array_equal(plain[:, 64:128], np.stack([s, c])[:, 64:128])


def test_rotate_sincos_single_call():
    """From a correctly rounded (s, c): 4 * 2^-53 of rounding plus the first dropped Taylor term, |d|^11 / 11!."""
    limit = ml.rotate_max_step()
    th, s0, c0, d = cases.rotate_points(limit)
    s, c = ml.host(ml.ROTATE, [s0, c0, d])
    err = cases.rotate_error(th, d, s, c)
    bound = 4 * 2.0 ** -53 + np.abs(d) ** 11 / math.factorial(11)
    worst = int(np.argmax(err / bound))
    _report(f"rotate_sincos |d| <= {limit}", err[worst], bound[worst])
    print(f"  dropped term at the threshold: {limit ** 11 / math.factorial(11):.3g}; worst error {err.max():.3g}")
    assert np.all(err <= bound), (th[worst], d[worst], err[worst])


@pytest.fixture(scope="module")
def chain():
    limit = ml.rotate_max_step()
    inp = cases.chain_inputs(limit)
    (s, c, angle), exact = ml.host(ml.CHAIN, inp, steps=cases.STEPS, want_exact_steps=True)
    assert not exact.any()                       # no increment exceeds the threshold: carried all the way
    ea, eb = cases.chain_errors(inp, s, c, angle)
    return inp, ea, eb


def test_chain_drift_against_the_exact_angle(chain):
    """1460 steps of the carried pair against sin / cos of x0 + sum d summed exactly: DESIGN.md's 1e-12."""
    inp, ea, _ = chain
    i = int(ea.argmax())
    _report(f"chain vs exact angle, {inp.shape[1]} chains x {cases.STEPS} steps", ea[i], 1e-12)
    print(f"  worst chain: start {inp[0, i]!r}, first increments {inp[1:4, i]}")
    assert ea.max() <= 1e-12, (inp[0, i], inp[1:4, i])


def test_chain_against_its_own_accumulated_angle(chain):
    """Against sin / cos of the double the kernel accumulates (r.eul, what the reference simulator takes sin / cos of):
    1e-12 plus the rounding of `eul += d`, steps * ulp(max |angle|) / 2."""
    inp, _, eb = chain
    bound = 1e-12 + cases.accumulation_bound(inp)
    i = int(np.argmax(eb / bound))
    _report("chain vs accumulated angle", eb[i], bound[i])
    j = int(eb.argmax())
    print(f"  largest: {eb[j]:.3g} at start {inp[0, j]!r} (bound {bound[j]:.3g})")
    assert np.all(eb <= bound), (inp[0, i], eb[i], bound[i])


def test_one_large_increment_takes_the_exact_path_for_its_whole_group():
    limit = ml.rotate_max_step()
    steps = 40
    plain, big = cases.mixed_group_inputs(limit, steps)
    (s0, c0, a0), ex0 = ml.host(ml.CHAIN, plain, steps=steps, want_exact_steps=True)
    (s1, c1, a1), ex1 = ml.host(ml.CHAIN, big, steps=steps, want_exact_steps=True)
    assert not ex0.any()
    want = np.zeros_like(ex1)
    want[steps - 1, 1] = 1
    assert np.array_equal(ex1, want)
    g = slice(64, 128)
    # the whole group is exact at that step: sincos of its own accumulated angle, to sincos_small's bound
    err = cases.sincos_error(a1[g], s1[g], c1[g])
    _report("exact path of a mixed group", err.max(), ULP1)
    assert err.max() <= ULP1
    assert np.array_equal(np.stack([s1[g], c1[g]]), ml.host(ml.SINCOS_SMALL, a1[g]))
    assert not np.array_equal(s1[g], s0[g])      # ... and the carried values of the plain run were not that
    # the other groups are untouched, bit for bit
    for o in (slice(0, 64), slice(128, 192)):
        assert np.array_equal(s1[o], s0[o]) and np.array_equal(c1[o], c0[o]) and np.array_equal(a1[o], a0[o])
