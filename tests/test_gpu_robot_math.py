"""The robot kernels' fp64 primitives on the device (salp_robot_math_probe: csrc/salp_fp64_math.h as the kernels compile
it, element i on thread i), 65536 elements per call.

Pure functions and the carried chain: bit for bit the host twin (tests/robot_math_host.cpp, held to mpmath by
tests/test_robot_math.py), mixed wavefronts included, so the twin's vote over 64 indices is the device's __any.  This
pins the compile flags of the robot unit: a contraction or a reassociation of this code shows here.
rcp_nr / sqrt_nr have no host form (their seeds are hardware instructions): held to their stated 1 ulp against 1/x and
sqrt(x) in long double, cross-checked with mpmath.  Worst cases are printed (pytest -s)."""
import math

import mpmath
import numpy as np
import pytest

import robot_math_cases as cases
import robot_math_lib as ml

pytestmark = pytest.mark.gpu
N = 65536


def _fit(x, n=N):
    """The first n of x, repeated if it is shorter."""
    return np.resize(np.asarray(x, np.float64), n)


def _same_bits(got, want, what, inputs=None):
    g, w = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    bad = np.argwhere(g != w)
    if len(bad):
        j = tuple(bad[0])
        detail = "" if inputs is None else f", input {np.asarray(inputs)[..., j[-1]]!r}"
        pytest.fail(f"{what}: {len(bad)} of {g.size} values differ; first at {j} (wavefront {j[-1] // 64}, lane {j[-1] % 64}): "
                    f"device {got[j]!r} ({int(g[j]):#018x}), host {want[j]!r} ({int(w[j]):#018x}){detail}")


def test_sincos_small_equals_the_host_twin():
    x = np.concatenate([cases.small_range_points(r)[:7000] for r in cases.SMALL_RANGES] + [cases.small_edge_points()[::2]])
    x = _fit(x)
    _same_bits(ml.device(ml.SINCOS_SMALL, x), ml.host(ml.SINCOS_SMALL, x), "sincos_small", x)


def test_sincos_euler_equals_the_host_twin_in_folding_and_mixed_wavefronts():
    rng = np.random.default_rng(21)
    t = ml.euler_fold_above()
    rest = rng.uniform(-1e4, 1e4, N - 192 - 20032)
    g = np.arange(0, len(rest) // 64, 5)                       # every fifth of these wavefronts: one lane above the switch
    rest[64 * g + rng.integers(0, 64, len(g))] = 10.0 ** rng.uniform(8.01, 15, len(g))
    x = np.concatenate([cases.euler_switch_points(t), _fit(cases.euler_points(), 20032), rest])
    assert len(x) == N
    got, want = ml.device(ml.SINCOS_EULER, x), ml.host(ml.SINCOS_EULER, x)
    _same_bits(got, want, "sincos_euler", x)
    # the vote did something: wavefronts with a lane above the switch differ from the unfolded function, the others do not
    plain = ml.host(ml.SINCOS_SMALL, np.where(np.abs(x) > 1e9, 0.0, x))      # (past its own range it is not called)
    folded = (np.abs(x) > t).reshape(-1, 64).any(axis=1)
    differs = (plain != want).any(axis=0).reshape(-1, 64).any(axis=1)
    assert np.array_equal(differs[~folded], np.zeros((~folded).sum(), bool)) and differs[folded].mean() > 0.9


def test_rotate_sincos_equals_the_host_twin():
    rng = np.random.default_rng(22)
    limit = ml.rotate_max_step()
    th = rng.uniform(-math.pi, math.pi, N)
    d = rng.uniform(-limit, limit, N)
    d[::4] = np.where(d[::4] < 0, -limit, limit)
    d[1::64] = rng.uniform(-2e-3, 2e-3, N // 64)               # the kernel's normal regime
    d[2::64] = 0.0
    inp = [np.sin(th), np.cos(th), d]
    _same_bits(ml.device(ml.ROTATE, inp), ml.host(ml.ROTATE, inp), "rotate_sincos", inp)


def test_chain_equals_the_host_twin_with_mixed_wavefronts():
    """48 steps x 65536 chains: increments of every size, one lane above the threshold on ~3 % of the wavefront-steps
    (the whole wavefront then takes the exact path), and wavefronts whose angles are past the fold switch, so that the
    exact path folds."""
    rng = np.random.default_rng(23)
    limit, steps = ml.rotate_max_step(), 48
    x0 = rng.uniform(-200.0, 200.0, N)
    x0[: 64 * 40] = rng.uniform(0.9e8, 1.2e8, 64 * 40) * rng.choice([-1.0, 1.0], 64 * 40)
    d = rng.uniform(-limit, limit, (steps, N))
    d[:, N // 2:] = rng.uniform(-2e-3, 2e-3, (steps, N // 2))
    d[:, ::7] = np.where(d[:, ::7] < 0, -limit, limit)          # at the threshold: not above it
    hit = rng.random((steps, N // 64)) < 0.03
    k, g = np.nonzero(hit)
    d[k, 64 * g + rng.integers(0, 64, len(k))] = rng.uniform(1.0001, 4.0, len(k)) * limit * rng.choice([-1.0, 1.0], len(k))
    inp = np.concatenate([x0[None], d])
    want, exact = ml.host(ml.CHAIN, inp, steps=steps, want_exact_steps=True)
    assert np.array_equal(exact.astype(bool), hit)
    _same_bits(ml.device(ml.CHAIN, inp, steps=steps), want, "chain", inp[:4])
    # and the single-lane case of the CPU suite, as it stands there
    plain, big = cases.mixed_group_inputs(limit)
    for a in (plain, big):
        _same_bits(ml.device(ml.CHAIN, a, steps=a.shape[0] - 1), ml.host(ml.CHAIN, a, steps=a.shape[0] - 1), "mixed group")


def test_full_length_chain_equals_the_host_twin():
    """The 1460-step chains of the CPU suite (64 chains) tiled over 64 wavefronts."""
    inp = np.tile(cases.chain_inputs(ml.rotate_max_step()), (1, 64))
    _same_bits(ml.device(ml.CHAIN, inp, steps=cases.STEPS), ml.host(ml.CHAIN, inp, steps=cases.STEPS), "full chain")


# ---- rcp_nr / sqrt_nr: 1 ulp of the exact value ---------------------------------------------------------------------

def _ulp_of(ref):
    """Spacing of binary64 at the (long double) value |ref|, normal range."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(np.longdouble(1.0), e - 53)


def _ulps(got, ref):
    return np.asarray(np.abs(got.astype(np.longdouble) - ref) / _ulp_of(ref), np.float64)


def _mp_ulps(got, exact_of, x):
    out = []
    with mpmath.workprec(cases.PREC):
        for g, xi in zip(got, x):
            ref = exact_of(mpmath.mpf(float(xi)))
            ulp = mpmath.ldexp(1, int(mpmath.floor(mpmath.log(abs(ref), 2))) - 52)
            out.append(float(abs(mpmath.mpf(float(g)) - ref) / ulp))
    return np.array(out)


def _kernel_rcp_arguments(count):
    """What the cycle body feeds rcp_nr: dt, mass, width, the inertia diagonal, the aspect span and cos(pitch) down to 1e-6,
    for the default config (column 0) and the random parameter box of the trajectory tests."""
    from underwater_swimmer_rl_amd.robot_compare import ROBOT_PARAM_NAMES, robot_params
    rng = np.random.default_rng(24)
    P = cases.random_robot_params(rng, count)
    P[:, 0] = robot_params(1, "cpu").numpy()[:, 0]
    p = {name: P[j] for j, name in enumerate(ROBOT_PARAM_NAMES)}
    u = rng.uniform(0, 1, count)
    contraction = rng.uniform(0, 0.06, count)
    length, width = p["init_length"] - contraction * u, p["init_width"] + contraction * u
    volume = 4.0 / 3 * math.pi * (length / 2) * (width / 2) ** 2
    mass = p["dry_mass"] + p["density"] * volume + p["nozzle_mass"]
    arm = -(p["nozzle_length1"] + p["nozzle_length2"]) - length / 2
    hw2, hl2 = (width / 2) ** 2, (length / 2) ** 2
    i0, i1 = 0.2 * mass * (hw2 + hw2), 0.2 * mass * (hl2 + hw2) + p["nozzle_mass"] * arm * arm
    contracted = p["init_length"] - p["max_contraction"]
    span = p["init_length"] / p["init_width"] - contracted / (p["init_length"] - contracted + p["init_width"])
    cos_pitch = 10.0 ** rng.uniform(-6, 0, count) * rng.choice([-1.0, 1.0], count)
    return np.concatenate([[0.01, 0.005, 0.02, 1e-3], mass, width, i0, i1, span, cos_pitch])


def test_rcp_nr_is_within_one_ulp():
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(25)
    edges = np.concatenate([s * m * 2.0 ** np.arange(-300, 301, 25) for s in (1.0, -1.0)
                            for m in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52)])
    fed = _kernel_rcp_arguments(2000)
    logu = 10.0 ** rng.uniform(-100, 100, N - len(edges) - len(fed)) * rng.choice([-1.0, 1.0], N - len(edges) - len(fed))
    x = np.concatenate([edges, fed, logu])
    y = ml.device(ml.RCP_NR, x)[0]
    err = _ulps(y, np.longdouble(1.0) / x.astype(np.longdouble))
    sub = np.concatenate([np.arange(len(edges) + 64), rng.integers(0, N, 400), [int(err.argmax())]])
    assert np.max(np.abs(_mp_ulps(y[sub], lambda v: 1 / v, x[sub]) - err[sub])) < 1e-3
    j = int(err.argmax())
    k = len(edges) + int(err[len(edges):len(edges) + len(fed)].argmax())
    print(f"rcp_nr: worst {err[j]:.4f} ulp at x = {x[j]!r}; on the kernel's own arguments {err[k]:.4f} ulp at {x[k]!r}; "
          f"{np.mean(err > 0.5) * 100:.2f} % not correctly rounded; bound 1 ulp")
    assert err[j] <= 1.0, (x[j], y[j], err[j])
    pw = np.abs(edges) == 2.0 ** np.round(np.log2(np.abs(edges)))
    assert np.array_equal(y[:len(edges)][pw], 1.0 / edges[pw])           # powers of two: exact


def test_sqrt_nr_is_within_one_ulp_and_tiny_lanes_switch_their_wavefront():
    rng = np.random.default_rng(26)
    plain = 10.0 ** rng.uniform(-190, 190, N)
    zeros, nans = np.array([0, 63, 64 * 9 + 31, N - 1]), np.array([64 * 7 + 5, 64 * 300 + 40])
    plain[zeros] = 0.0
    plain[nans] = np.nan
    tiny_waves = np.array([3, 100, 513, 1023])
    x = plain.copy()
    x[64 * tiny_waves + 17] = [1e-320, 1e-250, 1e-320, 1e-250]
    y0, y = ml.device(ml.SQRT_NR, plain)[0], ml.device(ml.SQRT_NR, x)[0]
    tiny = np.zeros(N // 64, bool)
    tiny[tiny_waves] = True
    lanes_tiny = np.repeat(tiny, 64)
    # wavefronts without a tiny lane are unaffected
    _same_bits(y[~lanes_tiny], y0[~lanes_tiny], "sqrt_nr outside the tiny wavefronts")
    # a tiny lane sends its whole wavefront to the library routine: correctly rounded, the subnormal argument too
    with np.errstate(invalid="ignore"):
        _same_bits(y[lanes_tiny], np.sqrt(x[lanes_tiny]), "sqrt_nr in a tiny wavefront", x[lanes_tiny])
    assert np.all(y[zeros] == 0.0) and np.all(np.isnan(y[nans])) and np.isnan(y).sum() == len(nans)
    ok = np.ones(N, bool)
    ok[zeros] = ok[nans] = False
    ok &= ~lanes_tiny
    err = np.zeros(N)
    err[ok] = _ulps(y[ok], np.sqrt(x[ok].astype(np.longdouble)))
    sub = np.concatenate([np.flatnonzero(ok)[:400], [int(err.argmax())]])
    assert np.max(np.abs(_mp_ulps(y[sub], mpmath.sqrt, x[sub]) - err[sub])) < 1e-3
    j = int(err.argmax())
    print(f"sqrt_nr: worst {err[j]:.4f} ulp at x = {x[j]!r}; {np.mean(err[ok] > 0.5) * 100:.2f} % not correctly rounded; bound 1 ulp")
    assert err[j] <= 1.0, (x[j], y[j], err[j])


def test_probe_rejects_what_it_cannot_run():
    from underwater_swimmer_rl_amd import _capi
    L = _capi.load_library()
    x, out = np.ones(64), np.full((3, 64), -7.0)
    ml.device(ml.SQRT_NR, x)                                   # declares the prototype
    for fn, n, steps, xp, op in ((99, 64, 0, x, out), (-1, 64, 0, x, out), (ml.RCP_NR, 0, 0, x, out), (ml.RCP_NR, -5, 0, x, out),
                                 (ml.RCP_NR, (1 << 24) + 1, 0, x, out), (ml.CHAIN, 64, -1, x, out), (ml.CHAIN, 64, 65537, x, out),
                                 (ml.RCP_NR, 64, 0, None, out), (ml.RCP_NR, 64, 0, x, None)):
        rc = L.salp_robot_math_probe(0, fn, None if xp is None else xp.ctypes.data, None if op is None else op.ctypes.data, n, steps)
        assert rc == -1 and L.salp_robot_last_error(), (fn, n, steps)
    assert L.salp_robot_math_probe(1 << 20, ml.RCP_NR, x.ctypes.data, out.ctypes.data, 64, 0) == -2
    assert np.all(out == -7.0)                                  # nothing was written
