"""The snake step's math primitives on the device (salp_snake_math_probe: csrc/salp_snake_math.h, csrc/salp_philox.h and
jet_thrust_terms of csrc/salp_step.h compiled with the rollout units' flags, element i on thread i), 65536 elements per
call, every element compared.

The references are those of tests/test_snake_math.py: the host twin of sincos_small bit for bit, sin / atan2 / cos in fp64,
long double and mpmath, the thrust formulas of the reference in exact arithmetic, the Python Philox.  Where the device
differs from the Python emulation by its reciprocal alone (v_rcp_f32, 1 ulp), the bound is the emulation's worst error on
the same inputs plus one ulp of t (tests/snake_math_cases.py gpu_bound); tests/test_snake_math.py shows that a 1e-3 slip in
any coefficient breaks what is asserted here.  Worst cases are printed (pytest -s) and recorded in DESIGN.md §4."""
import math

import mpmath
import numpy as np
import pytest

import robot_math_lib as rml
import snake_math_cases as cases
import snake_math_lib as ml

pytestmark = pytest.mark.gpu
N = cases.N
F32 = np.float32


def _same_bits(got, want, what, inputs=None):
    g, w = np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64)
    bad = np.argwhere(g != w)
    if len(bad):
        j = tuple(bad[0])
        detail = "" if inputs is None else f", input {np.asarray(inputs)[..., j[-1]]!r}"
        pytest.fail(f"{what}: {len(bad)} of {g.size} values differ; first at {j}: device {np.asarray(got)[j]!r} ({int(g[j]):#018x}), "
                    f"reference {np.asarray(want)[j]!r} ({int(w[j]):#018x}){detail}")


def _is_f32(a):
    return np.array_equal(a.astype(F32).astype(np.float64), a)


def _report(what, worst, bound, unit=""):
    print(f"{what}: worst {worst:.3g}{unit}, bound {bound:.3g}{unit} ({worst / bound:.2f} of it)")


def test_sincos_small_t_equals_the_host_twin_of_sincos_small():
    """The table's values and evaluation order are sincos_small's: bit for bit the host twin, which tests/test_robot_math.py
    holds to 2^-52."""
    x = cases.sincos_points()
    assert len(x) == N and np.abs(x[-20000:]).max() > 103.9
    _same_bits(ml.device(ml.SINCOS_T, x), rml.host(rml.SINCOS_SMALL, x), "sincos_small_t", x)


def test_sin_nozzle_t_is_within_one_ulp():
    """Bound 1 ulp of sin x: the last fma rounds x + x z p once (half an ulp); the correction x z p is at most 0.19 |x| at
    pi / 3 with a few ulps of relative error (z, x z, ten Horner steps of which only the last weigh), under 0.48 ulp.  The
    emulation measures 0.95 ulp."""
    x = cases.nozzle_points()
    got = ml.device(ml.SIN_NOZZLE_T, x)[0]
    ulps = cases.ld_sin_ulps(x, got)
    j = int(ulps.argmax())
    sub = np.concatenate([np.arange(0, 200), np.arange(200, N, 331), [j]])
    assert np.max(np.abs(cases.mp_sin_ulps(x[sub], got[sub]) - ulps[sub])) < 1e-3          # long double against mpmath
    _report("sin_nozzle_t", ulps[j], 1.0, " ulp")
    print(f"  at x = {x[j]!r}; {np.mean(ulps > 0.5) * 100:.2f} % not correctly rounded; "
          f"{np.mean(got != cases.sin_nozzle_t(x)) * 100:.3f} % differ from the emulation")
    assert ulps[j] <= 1.0, (x[j], got[j])
    zero = x == 0
    assert zero.sum() >= 2 and np.all(got[zero] == 0) and np.array_equal(np.signbit(got[zero]), np.signbit(x[zero]))
    tiny = np.abs(x) == 1e-300
    assert tiny.sum() == 2 and np.array_equal(got[tiny], x[tiny])


@pytest.mark.parametrize("precise", [False, True])
def test_atan2_fast(precise):
    y, x, below = cases.atan2_points()
    ok = ~below
    got = ml.device(ml.ATAN2_PRECISE if precise else ml.ATAN2, [y, x])[0]
    assert _is_f32(got)
    emu = cases.atan2_fast(y, x, precise).astype(np.float64)
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err, err_emu = np.abs(got - ref), np.abs(emu - ref)
    bound = cases.gpu_bound(err_emu[ok].max())
    j = int(np.argmax(np.where(ok, err, 0)))
    _report(f"atan2_fast<{precise}>, radii 1e-3 .. 2e3 px", err[j], bound, " rad")
    print(f"  at y = {y[j]!r}, x = {x[j]!r}; emulation {err_emu[ok].max():.3g} rad; {err[j] / math.pi:.3g} of pi, contract {cases.CONTRACT}")
    assert err[j] <= bound, (y[j], x[j], got[j])
    assert err[j] <= 0.25 * cases.CONTRACT * math.pi
    zero = (x == 0) & (y == 0)
    assert zero.sum() == 2 and np.all(got[zero] == 0) and np.array_equal(np.signbit(got[zero]), np.signbit(y[zero]))
    axis = (y == 0) & (x < 0)                                      # y = +-0 at x < 0: +-pi_f32
    assert axis.sum() >= 12 and np.array_equal(got[axis], np.copysign(np.float64(cases.PI_F), y[axis]))
    diag = (np.abs(y) == np.abs(x)) & ok & ~zero                   # |y| = |x| exactly: t = 1 whatever the reciprocal's last bit
    assert diag.sum() >= 160 and err[diag].max() <= bound
    # under the 1e-30 floor the function is not atan2 (t = min * 1e30): held to the emulation, one ulp of t apart
    d = np.abs(got[below] - emu[below])
    print(f"  under the floor ({below.sum()} elements): {d.max():.3g} rad from the emulation, {err[below].max():.3g} rad from atan2")
    assert below.sum() >= 6 and d.max() <= cases.RCP_ALLOWANCE + np.spacing(cases.PI_F)     # and the last rounding of the result
    assert np.array_equal(np.signbit(got[below]), np.signbit(y[below]))


def test_cos_wrapped():
    """The two-level bound of atan2_fast, and bit for bit the emulation: cos_wrapped has no reciprocal in it, every
    operation is an IEEE fp32 one, and the unit is compiled without contraction."""
    x = cases.cos_points()
    got = ml.device(ml.COS_WRAPPED, x)[0]
    assert _is_f32(got)
    emu = cases.cos_wrapped(x).astype(np.float64)
    ref = np.cos(x.astype(np.float64))
    err = np.abs(got - ref)
    bound = cases.gpu_bound(np.abs(emu - ref).max())
    j = int(err.argmax())
    _report("cos_wrapped on [-pi_f32, pi_f32]", err[j], bound)
    print(f"  at x = {x[j]!r}; emulation {np.abs(emu - ref).max():.3g}; contract {cases.CONTRACT}")
    assert err[j] <= bound and err[j] <= 0.25 * cases.CONTRACT
    _same_bits(got, emu, "cos_wrapped against its emulation", x)


@pytest.mark.parametrize("precise", [False, True])
def test_relative_heading(precise):
    dy, dx, th, inner = cases.heading_points()
    got = ml.device(ml.REL_HEADING_PRECISE if precise else ml.REL_HEADING, [dy, dx, th])[0]
    assert _is_f32(got)
    emu = cases.relative_heading(dy, dx, th, precise)
    err, err_emu = cases.circle_error(got, dy, dx, th), cases.circle_error(emu, dy, dx, th)
    bound = cases.gpu_bound(err_emu[inner].max())
    j, k = int(np.argmax(np.where(inner, err, 0))), int(err.argmax())
    _report(f"relative_heading<{precise}>, |th| <= pi", err[j], bound, " rad")
    _report(f"relative_heading<{precise}>, |th| <= 100", err[k] / math.pi, cases.CONTRACT, " of pi")
    print(f"  emulation {err_emu[inner].max():.3g} / {err_emu.max():.3g} rad; largest magnitude - pi_f32: {np.abs(got).max() - float(cases.PI_F):.3g}")
    assert np.abs(got).max() <= float(np.nextafter(cases.PI_F, F32(4)))
    assert err[k] / math.pi < cases.CONTRACT, (dy[k], dx[k], th[k], got[k])
    assert err[j] <= bound, (dy[j], dx[j], th[j], got[j])
    edge = np.abs(np.abs(got) - float(cases.PI_F)) <= np.spacing(cases.PI_F)
    assert edge.sum() >= 8                                          # the cases do land on +-pi and next to it
    if precise:
        # the proximity term of the reward: weight 5 (single_food.yaml) times the cosine of this heading
        c = ml.device(ml.COS_WRAPPED, got)[0]
        exact = np.cos(np.arctan2(dy.astype(np.float64), dx.astype(np.float64)) - th.astype(np.float64))
        e = 5.0 * np.abs(c - exact)
        i = int(np.argmax(np.where(inner, e, 0)))
        _report("5 cos_wrapped(relative_heading<true>), |th| <= pi", e[i], cases.CONTRACT)
        assert e[i] <= cases.CONTRACT, (dy[i], dx[i], th[i])


def test_philox_known_answers_counter_edges_and_random_words():
    import ref_harness as rh
    a = cases.philox_points()
    got = ml.device(ml.PHILOX, a.astype(np.float64))
    assert np.array_equal(got, np.floor(got)) and got.min() >= 0 and got.max() < 2.0 ** 32
    got = got.astype(np.uint64)
    for j, (_, _, want) in enumerate(cases.PHILOX_KAT):
        assert tuple(int(v) for v in got[:, j]) == want, j
    for j in range(N):                                              # the Python Philox, one by one
        assert tuple(int(v) for v in got[:, j]) == tuple(rh.philox4x32_10(a[:4, j], a[4:, j])), (j, a[:, j])
    assert np.array_equal(got, cases.philox(a[:4], a[4:]))


def test_u53_is_exact():
    rng = np.random.default_rng(60)
    hi, lo = rng.integers(0, 1 << 32, (2, N), dtype=np.uint64)
    hi[:6], lo[:6] = [0xFFFFFFFF, 0, 0xFFFFFFFF, 0, 31, 1 << 5], [0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 63, 1 << 6]
    got = ml.device(ml.U53, [hi.astype(np.float64), lo.astype(np.float64)])[0]
    # ((hi >> 5) 2^26 + (lo >> 6)) 2^-53 in exact (integer) arithmetic: the numerator is below 2^53, so a double holds it
    num = (hi >> np.uint64(5)) * np.uint64(1 << 26) + (lo >> np.uint64(6))
    assert int(num.max()) < 1 << 53
    _same_bits(got, np.ldexp(num.astype(np.float64), -53), "u53")
    assert got[0] == 1 - 2.0 ** -53 and got[0] < 1 and got[1] == 0 and got[4] == 0 and got[5] == (2.0 ** 26 + 1) * 2.0 ** -53


def _thrust_config(thrust_force):
    from underwater_swimmer_rl_amd.config import SalpSnakeConfig
    return None if thrust_force is None else SalpSnakeConfig(max_thrust_force=thrust_force)


@pytest.mark.parametrize("form, thrust_force, seed, points", [("std", None, 7, 1), ("std", None, 0x9E3779B97F4A7C15, 2),
                                                              ("rt", None, 123456789, 3), ("rt", 63.5, (1 << 63) + 5, 4)])
def test_thrust_terms(form, thrust_force, seed, points):
    """jet_thrust_terms against legacy:261-314 as oracle/salp_oracle.c:225-253 restates it, in exact arithmetic (long
    double for every element, mpmath on a subsample and the worst) at the reference's own rounded angles
    fl(phi + pi / 2) and fl(phi + fl((u - 0.5) 0.05)), u from Philox at the same (genv, rng, seed).

    Each term is bounded by scale (2^-52 + ulp(|angle|) / 2 + k 2^-53): scale is T = thrust 0.4 water times the term's
    constants (and |nozzle| for the side term; for the turning term the sum of its three parts' magnitudes).
      2^-52            sincos_small_t's absolute error on the sine or cosine of phi (not in the turning term);
      ulp(|angle|)/2   side and jitter terms: the reference rounds phi + pi / 2 and phi + d to a double, the kernel rotates
                       the exact sincos of phi instead (by dl = fl(pi / 2) - pi / 2, and by d through a short series whose
                       dropped terms are below 1e-22), so the two angles differ by that rounding: 2.2e-16 rad for |phi| < 2,
                       4.4e-16 up to 4, 7.1e-15 at |theta| = 100;
      k 2^-53          the roundings of the term, each relative to at most the scale: T has 2;
                       main jet (c T) K: 2 + 2 = 4;  side: fma(dl, c, s) 1, S = (T |noz|) K 2 + 2, (sc S) K 2: 7;
                       jitter: sD and cD 1 each, c cD - s sD 3, the second sincos error weighed by |sD| <= 0.025 under 1,
                       nf = T K 2 + 1, (nc nf) K 2: 11;
                       turning: its moment part has sin_nozzle_t's ulp 2, T 2, T sin 1, r K 1, perp arm 1, K 1 = 8, the two
                       additions 2: 10."""
    P = cases.thrust_points(points)
    cfg = _thrust_config(thrust_force)
    tf = 100.0 if thrust_force is None else thrust_force
    got = ml.device(ml.THRUST_STD if form == "std" else ml.THRUST_RT, P, cfg=cfg, seed=seed)
    u = cases.jitter_uniform(P[5].astype(np.uint64), P[6].astype(np.uint64), P[4].astype(np.uint64), seed)
    bound = cases.thrust_bound(P[0], P[1], P[2], P[3], u, tf)
    ref = cases.thrust_reference(P[0], P[1], P[2], P[3], u, tf)
    err = np.asarray(np.abs(got.astype(np.longdouble) - ref), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    sub = np.unique(np.concatenate([np.arange(0, 70), np.arange(70, N, 997), ratio.argmax(axis=1)]))
    mp = cases.thrust_reference_mp(*(P[k][sub] for k in range(4)), u[sub], tf)
    with mpmath.workprec(cases.PREC):
        e_mp = np.array([[float(abs(mpmath.mpf(float(got[k][i])) - mp[j][k])) for j, i in enumerate(sub)] for k in range(7)])
    with np.errstate(invalid="ignore", divide="ignore"):
        r_mp = np.where(bound[:, sub] > 0, e_mp / bound[:, sub], np.where(e_mp == 0, 0.0, np.inf))
    assert np.max(np.abs(r_mp - ratio[:, sub])) < 1e-3              # long double against mpmath
    names = ("ax", "ay", "bx", "by", "cx", "cy", "om")
    wide = np.abs(P[0]) > math.pi
    print(f"jet_thrust_terms<{form}> thrust {tf}: worst ratio to the bound " + ", ".join(f"{n} {r:.2f}" for n, r in zip(names, ratio.max(axis=1))))
    print(f"  side / jitter error {err[2:6][:, ~wide].max():.3g} for |theta| <= pi, {err[2:6][:, wide].max():.3g} up to 100 rad; "
          f"{np.mean(got != cases.thrust_terms(P[0], P[1], P[2], P[3], u, tf)) * 100:.3f} % of the values differ from the emulation")
    k = int(ratio.max(axis=1).argmax())
    assert ratio.max() <= 1.0, (names[k], ratio.max(), P[:, int(ratio[k].argmax())])


def test_thrust_forms_agree_bit_for_bit_on_the_default_config():
    from underwater_swimmer_rl_amd.config import SalpSnakeConfig
    P = cases.thrust_points(5)
    std = ml.device(ml.THRUST_STD, P, seed=99)
    _same_bits(ml.device(ml.THRUST_RT, P, seed=99), std, "runtime-constant form, NULL config", P)
    _same_bits(ml.device(ml.THRUST_RT, P, cfg=SalpSnakeConfig(), seed=99), std, "runtime-constant form, default config", P)
    _same_bits(ml.device(ml.THRUST_STD, P, cfg=SalpSnakeConfig(), seed=99), std, "literal form, default config", P)
    assert not np.array_equal(ml.device(ml.THRUST_STD, P, seed=100)[4], std[4])     # the key does reach the jitter


def test_probe_rejects_what_it_cannot_run():
    import ctypes
    from underwater_swimmer_rl_amd.config import SalpSnakeConfig
    L = ml.library()
    x, out = np.ones((7, 64)), np.full((7, 64), -7.0)
    other = SalpSnakeConfig(max_thrust_force=80.0).to_c()           # runs through the runtime-constant kernels
    skewed = SalpSnakeConfig().to_c()
    skewed.struct_size += 8
    bad_range = SalpSnakeConfig().to_c()
    bad_range.base_radius = -1.0
    for fn, n, cfg, xp, op in ((99, 64, None, x, out), (-1, 64, None, x, out), (11, 64, None, x, out), (ml.U53, 0, None, x, out),
                               (ml.U53, -5, None, x, out), (ml.U53, (1 << 24) + 1, None, x, out), (ml.U53, 64, None, None, out),
                               (ml.U53, 64, None, x, None), (ml.THRUST_STD, 64, other, x, out), (ml.THRUST_RT, 64, skewed, x, out),
                               (ml.ATAN2, 64, bad_range, x, out)):
        rc = L.salp_snake_math_probe(0, fn, None if cfg is None else ctypes.byref(cfg), 0, None if xp is None else xp.ctypes.data,
                                     None if op is None else op.ctypes.data, n)
        assert rc == -1 and L.salp_last_error(), (fn, n)
    assert L.salp_snake_math_probe(1 << 20, ml.U53, None, 0, x.ctypes.data, out.ctypes.data, 64) == -2
    assert np.all(out == -7.0)                                      # nothing was written
    assert L.salp_snake_math_probe(0, ml.THRUST_RT, ctypes.byref(other), 0, x.ctypes.data, out.ctypes.data, 64) == 0
