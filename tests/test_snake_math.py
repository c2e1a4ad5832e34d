"""The snake step's math primitives without a GPU: the thrust table row by row against its definitions, the Python
emulations of tests/snake_math_cases.py (the kernel's operation order, exact fma) against mpmath, the power of the bounds
tests/test_gpu_snake_math.py asserts, and Philox against the Random123 known answers.  The worst cases printed here
(pytest -s) are the figures the device is judged against; DESIGN.md §4 records them."""
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import snake_math_cases as cases

F32 = np.float32


def _report(what, worst, bound, unit=""):
    print(f"{what}: worst {worst:.3g}{unit}, bound {bound:.3g}{unit} ({worst / bound:.2f} of it)")


# ---- kThrustTbl: every row is its definition ----------------------------------------------------------------------------

def _rounded(fraction):
    return fraction.numerator / fraction.denominator            # int / int is correctly rounded


def test_table_has_count_rows_plus_padding():
    names, values, size = cases.thrust_table()
    assert names[-1] == "TT_COUNT" and len(set(names)) == len(names) == 47
    assert size == "TT_COUNT + 2" and len(values) == len(names) - 1 + 2
    T = cases.table()
    assert T["TT_PAD0"] == 0.0 and values[-2:] == [0.0, 0.0]
    assert all(math.copysign(1.0, v) == 1.0 for v in (T["TT_PAD0"], *values[-2:]))


def test_reduction_and_kernel_rows_are_the_literals_of_sincos_small():
    src = cases._strip_comments(cases._source("salp_fp64_math.h"))
    body = src[src.index("void sincos_small("):src.index("void sincos_euler(")]
    literals = re.findall(r"-?\d\.\d{20}e[-+]\d\d", body)
    rows = ["TT_2OPI", "TT_PIO2_1", "TT_PIO2_1T", "TT_S5", "TT_S4", "TT_S3", "TT_S2", "TT_S1", "TT_S0",
            "TT_C6", "TT_C5", "TT_C4", "TT_C3", "TT_C2", "TT_C1"]
    assert len(literals) == len(rows)
    T = cases.table()
    # in sincos_small's order: the reduction, the sine kernel from its highest power down, the cosine kernel likewise
    assert [T[r] for r in rows] == [float(v) for v in literals]
    tbl = cases._strip_comments(cases._source("salp_snake_math.h"))
    for v in literals:                                           # and digit for digit
        assert v in tbl, v


def test_nozzle_rows_are_the_correctly_rounded_taylor_coefficients():
    T = cases.table()
    for k in range(1, 11):
        assert T[f"TT_N{k}"] == _rounded(Fraction((-1) ** k, math.factorial(2 * k + 1))), k


def test_jitter_rows_are_the_correctly_rounded_reciprocal_factorials():
    T = cases.table()
    for k in range(4):                                           # sin D = D + D^3 (S0 + z (S1 + z (S2 + z S3)))
        assert T[f"TT_J_S{k}"] == _rounded(Fraction((-1) ** (k + 1), math.factorial(2 * k + 3))), k
    for k in range(1, 4):                                        # cos D = 1 + z (-1/2 + z (C1 + z (C2 + z C3)))
        assert T[f"TT_J_C{k}"] == _rounded(Fraction((-1) ** (k + 1), math.factorial(2 * k + 2))), k


def test_scalings_are_the_constants_of_the_oracle():
    with open(os.path.join(cases.ROOT, "oracle", "salp_oracle.c")) as f:
        src = f.read()
    body = src[src.index("static void apply_jet_thrust("):src.index("/* snake:232-276 _respawn_food */")]
    num = r"([0-9.]+);"
    where = {"TT_K04": r"max_thrust_force \* e->water \* ", "TT_K012": r"tx \* ", "TT_K0002": r"primary = -e->nozzle \* T \* ",
             "TT_K07": r"pymax\(e->a, e->b\) \* ", "TT_K00005": r"perp \* moment_arm \* ", "TT_K00003": r"T \* e->water \* ",
             "TT_K03": r"fabs\(e->nozzle\) \* ", "TT_K008": r"sx \* ", "TT_K005": r"\(u - 0\.5\) \* ",
             "TT_K004": r"noise_force = T \* ", "TT_K0002J": r"cos\(noise_angle\) \* noise_force \* "}
    T = cases.table()
    for row, pattern in where.items():
        found = re.findall(pattern + num, body)
        assert len(found) == 1, (row, found)
        assert T[row] == float(found[0]), (row, found)
    for a, b in (("ty", "TT_K012"), ("sy", "TT_K008"), (r"sin\(noise_angle\) \* noise_force", "TT_K0002J")):
        assert T[b] == float(re.search(a + r" \* " + num, body).group(1))
    assert "thrust_angle + M_PI / 2" in body and T["TT_PIO2"] == math.pi / 2 == cases.PIO2


def test_dl_row_is_the_rounding_error_of_pi_over_two():
    with mpmath.workprec(cases.PREC):
        dl = mpmath.mpf(math.pi / 2) - mpmath.pi / 2
        assert cases.table()["TT_DL"] == float(dl)
        # a 17-digit literal would name the double exactly; the row has 16 and must still round to it
        assert abs(mpmath.mpf(cases.table()["TT_DL"]) - dl) < mpmath.mpf(2) ** -105


def test_emulation_uses_the_headers_fp32_numbers():
    precise, plain, cw = cases.source_fp32_coefficients()
    assert precise == cases.ATAN_COEF[True] and plain == cases.ATAN_COEF[False]
    assert cw == cases.COS_COEF
    src = cases._source("salp_snake_math.h")
    for text in ("1.57079632679489662f", "3.14159265358979324f", "0.15915494309189535f", "-6.28318530717959f", "1.0e-30f",
                 "fmaf(z, p, 1.0f)"):
        assert text in src, text
    step = cases._source("salp_step.h")
    for text in ("fma(z, cp, -0.5)", "fma(z, cp, 1.0)", "fma(dl, c, s)", "fma(-dl, s, c)"):
        assert text in step, text


# ---- the exact fma of the emulation ------------------------------------------------------------------------------------

def test_fmaf_rounds_once():
    rng = np.random.default_rng(50)
    a, b = rng.uniform(-2, 2, 20000).astype(F32), rng.uniform(-2, 2, 20000).astype(F32)
    c = (rng.uniform(-2, 2, 20000) * 10.0 ** rng.integers(-9, 1, 20000)).astype(F32)
    # a case a double-rounded a * b + c gets wrong: the sum is 2^-30 above a float32 tie
    a[0], b[0], c[0] = F32(1 + 2.0 ** -23), F32(1 + 2.0 ** -23) * F32(0.5) + F32(0.5), F32(2.0 ** -70)
    a[1], b[1], c[1] = F32(1.0), F32(1 + 2.0 ** -23), F32(2.0 ** -24 + 2.0 ** -60)
    got = cases.fmaf(a, b, c)
    want = np.array([F32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got, want)
    assert got[1] == F32(1 + 2.0 ** -22)                         # above the tie: up; a * b + c in fp64 rounds it to even, down


def test_fma_is_exact():
    rng = np.random.default_rng(51)
    a, b, c = rng.uniform(-2, 2, (3, 3000))
    c *= 10.0 ** rng.integers(-20, 1, 3000)
    want = np.array([_rounded(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(cases.fma(a, b, c), want)
    assert np.any(want != a * b + c)


# ---- emulation against exact references: the figures the device is judged against -----------------------------------------

def _mp_check(values, exact_of, inputs, tol=4e-16):
    """numpy's fp64 reference against mpmath on a subsample: the reference's own error."""
    with mpmath.workprec(cases.PREC):
        worst = max(abs(float(mpmath.mpf(float(v)) - exact_of(*[mpmath.mpf(float(a)) for a in args])))
                    for v, args in zip(values, zip(*inputs)))
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("precise", [False, True])
def test_atan2_emulation_error(precise):
    y, x, below = cases.atan2_points()
    ok = ~below
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    sub = np.concatenate([np.arange(0, 600), np.arange(600, cases.N, 97)])
    sub = sub[ok[sub] & (y[sub] != 0)]                           # (mpmath has no signed zero)
    _mp_check(ref[sub], mpmath.atan2, (y[sub], x[sub]), tol=5e-16)
    got = cases.atan2_fast(y, x, precise).astype(np.float64)
    err = np.abs(got - ref)
    j = int(np.argmax(np.where(ok, err, 0)))
    _report(f"atan2_fast<{precise}> emulation, radii 1e-3 .. 2e3 px", err[j], cases.CONTRACT * math.pi, " rad")
    print(f"  at y = {y[j]!r}, x = {x[j]!r}; device bound {cases.gpu_bound(err[j]):.3g} rad")
    assert err[j] <= 0.25 * cases.CONTRACT * math.pi
    zero = (x == 0) & (y == 0)
    assert zero.sum() == 2 and np.array_equal(np.signbit(got[zero]), np.signbit(y[zero])) and np.all(got[zero] == 0)
    # under the floor it is not atan2 (t = min * 1e30): finite, in [0, pi / 2] or [pi / 2, pi] by the sign of x, sign of y kept
    assert below.sum() >= 6 and np.all(np.isfinite(got[below])) and np.all(np.abs(got[below]) <= float(cases.PI_F))
    assert np.array_equal(np.signbit(got[below]), np.signbit(y[below]))
    print(f"  under the 1e-30 floor ({below.sum()} elements) the error reaches {err[below].max():.3g} rad: not atan2 there")


def test_cos_wrapped_emulation_error():
    x = cases.cos_points()
    ref = np.cos(x.astype(np.float64))
    _mp_check(ref[::131], mpmath.cos, (x[::131],))
    err = np.abs(cases.cos_wrapped(x).astype(np.float64) - ref)
    j = int(err.argmax())
    _report("cos_wrapped emulation on [-pi_f32, pi_f32] and a neighbour beyond", err[j], cases.CONTRACT)
    print(f"  at x = {x[j]!r}; device bound {cases.gpu_bound(err[j]):.3g}")
    assert err[j] <= 0.25 * cases.CONTRACT


@pytest.mark.parametrize("precise", [False, True])
def test_relative_heading_emulation_error(precise):
    dy, dx, th, inner = cases.heading_points()
    got = cases.relative_heading(dy, dx, th, precise)
    err = cases.circle_error(got, dy, dx, th)
    j, k = int(np.argmax(np.where(inner, err, 0))), int(err.argmax())
    _report(f"relative_heading<{precise}> emulation, |th| <= pi", err[j], cases.CONTRACT * math.pi, " rad")
    _report(f"relative_heading<{precise}> emulation, |th| <= 100", err[k], cases.CONTRACT * math.pi, " rad")
    print(f"  at th = {th[k]!r}; largest magnitude - pi_f32: {np.abs(got).max() - cases.PI_F!r}")
    assert err[k] < cases.CONTRACT * math.pi
    assert np.abs(got).max() <= np.nextafter(cases.PI_F, F32(4))
    if precise:
        exact = np.cos(np.arctan2(dy.astype(np.float64), dx.astype(np.float64)) - th.astype(np.float64))
        e = 5.0 * np.abs(cases.cos_wrapped(got).astype(np.float64) - exact)
        _report("5 cos_wrapped(relative_heading<true>), |th| <= pi", e[inner].max(), cases.CONTRACT)
        assert e[inner].max() <= cases.CONTRACT


def test_sin_nozzle_emulation_is_within_one_ulp():
    """The final fma rounds x + x z p once (half an ulp); the correction x z p is at most 0.19 |x| at pi / 3 and carries a
    few ulps of relative error (the rounding of z, of x z and of each Horner step), so under 0.19 * 2.5 = 0.48 ulp: 1 ulp."""
    x = cases.nozzle_points()
    got = cases.sin_nozzle_t(x)
    ulps = cases.ld_sin_ulps(x, got)
    j = int(ulps.argmax())
    sub = np.concatenate([np.arange(0, 200), np.arange(200, cases.N, 67), [j]])
    assert np.max(np.abs(cases.mp_sin_ulps(x[sub], got[sub]) - ulps[sub])) < 1e-3      # long double against mpmath
    _report("sin_nozzle_t emulation, |x| <= pi / 3", ulps[j], 1.0, " ulp")
    print(f"  at x = {x[j]!r}; {np.mean(ulps > 0.5) * 100:.2f} % not correctly rounded")
    assert ulps[j] <= 1.0
    assert np.array_equal(np.signbit(got[x == 0]), np.signbit(x[x == 0])) and got[list(x).index(1e-300)] == 1e-300


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


@pytest.mark.parametrize("thrust_force, seed", [(100.0, 7), (63.5, 0x9E3779B97F4A7C15)])
def test_thrust_terms_emulation_is_within_the_bound(thrust_force, seed):
    """Against legacy:261-314 (oracle/salp_oracle.c:225-253) in exact arithmetic at the reference's own rounded angles; the
    bound and its derivation are those of tests/test_gpu_snake_math.py."""
    P = cases.thrust_points(1)
    u = cases.jitter_uniform(P[5].astype(np.uint64), P[6].astype(np.uint64), P[4].astype(np.uint64), seed)
    got = cases.thrust_terms(P[0], P[1], P[2], P[3], u, thrust_force)
    bound = cases.thrust_bound(P[0], P[1], P[2], P[3], u, thrust_force)
    ref = cases.thrust_reference(P[0], P[1], P[2], P[3], u, thrust_force)
    ratio = _ratio(np.asarray(np.abs(got.astype(np.longdouble) - ref), np.float64), bound)
    sub = np.unique(np.concatenate([np.arange(0, 130), np.arange(130, cases.N, 211), ratio.argmax(axis=1)]))
    mp = cases.thrust_reference_mp(*(P[k][sub] for k in range(4)), u[sub], thrust_force)
    with mpmath.workprec(cases.PREC):
        r_mp = np.array([[float(abs(mpmath.mpf(float(got[k][i])) - mp[j][k])) for j, i in enumerate(sub)] for k in range(7)])
    r_mp = _ratio(r_mp, bound[:, sub])
    assert np.max(np.abs(r_mp - ratio[:, sub])) < 1e-3              # long double against mpmath
    names = ("ax", "ay", "bx", "by", "cx", "cy", "om")
    print(f"jet_thrust_terms emulation, thrust {thrust_force}: worst ratio to the bound " +
          ", ".join(f"{n} {r:.2f}" for n, r in zip(names, ratio.max(axis=1))))
    wide = np.abs(P[0]) > math.pi
    err = np.asarray(np.abs(got.astype(np.longdouble) - ref), np.float64)
    print(f"  side / jitter error: {err[2:6][:, ~wide].max():.3g} for |theta| <= pi, {err[2:6][:, wide].max():.3g} up to 100 rad")
    assert ratio.max() <= 1.0, (names[int(ratio.max(axis=1).argmax())], ratio.max())


# ---- the bounds of the GPU test see a slip of 1e-3 in any one coefficient --------------------------------------------------

def _moved(coef, k, rel):
    c = list(coef)
    c[k] = float(F32(c[k])) * (1 + rel)
    return c


def test_a_moved_fp32_coefficient_fails_what_the_gpu_test_asserts():
    """Each coefficient of the three fp32 polynomials moved by 1e-3 relative, either way.  atan2_fast and relative_heading:
    the emulation's worst error then exceeds emulation worst + reciprocal allowance, the bound the device is held to.
    cos_wrapped: the same for its five low coefficients; a move of the x^12 and x^10 coefficients changes the value by
    4.7e-10 and 2.5e-8 at most, under half an ulp of the result, which no error bound on an fp32 value can see — the GPU
    test therefore also holds cos_wrapped to the emulation bit for bit (it has no reciprocal in it), and that comparison
    sees them."""
    y, x, below = cases.atan2_points()
    ok = ~below
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))[ok]
    dy, dx, th, inner = cases.heading_points()
    for precise in (False, True):
        base = np.abs(cases.atan2_fast(y, x, precise).astype(np.float64)[ok] - ref).max()
        base_h = cases.circle_error(cases.relative_heading(dy, dx, th, precise), dy, dx, th)[inner].max()
        for k in range(len(cases.ATAN_COEF[precise])):
            for rel in (1e-3, -1e-3):
                c = _moved(cases.ATAN_COEF[precise], k, rel)
                worst = np.abs(cases.atan2_fast(y, x, precise, c).astype(np.float64)[ok] - ref).max()
                assert worst > cases.gpu_bound(base), (precise, k, rel, worst, base)
                worst = cases.circle_error(cases.relative_heading(dy, dx, th, precise, c), dy, dx, th)[inner].max()
                assert worst > cases.gpu_bound(base_h), (precise, k, rel, worst, base_h)
    xc = cases.cos_points()
    refc = np.cos(xc.astype(np.float64))
    plain = cases.cos_wrapped(xc)
    base = np.abs(plain.astype(np.float64) - refc).max()
    by_bound = []
    for k in range(len(cases.COS_COEF)):
        for rel in (1e-3, -1e-3):
            moved = cases.cos_wrapped(xc, _moved(cases.COS_COEF, k, rel))
            over = np.abs(moved.astype(np.float64) - refc).max() > cases.gpu_bound(base)
            by_bound.append(over)
            assert over or not np.array_equal(moved, plain), (k, rel)
    print("cos_wrapped coefficients (x^12 first, both directions) whose move exceeds the bound:", by_bound)
    assert all(by_bound[4:]) and not any(by_bound[:4])


# ---- Philox ------------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    import ref_harness as rh
    for counter, key, want in cases.PHILOX_KAT:
        assert tuple(rh.philox4x32_10(counter, key)) == want
        assert tuple(int(v) for v in cases.philox(np.array(counter)[:, None], np.array(key)[:, None])[:, 0]) == want


def test_oracle_philox_known_answers():
    import oracle_lib as ol
    for counter, key, want in cases.PHILOX_KAT:
        assert ol.philox(counter, key) == want


def test_vectorised_philox_and_u53_equal_the_python_ones():
    import ref_harness as rh
    a = cases.philox_points()[:, :4096]
    w = cases.philox(a[:4], a[4:])
    for j in range(a.shape[1]):
        assert tuple(int(v) for v in w[:, j]) == tuple(rh.philox4x32_10(a[:4, j], a[4:, j])), j
    u = cases.u53(a[0], a[1])
    for j in range(0, a.shape[1], 7):
        hi, lo = int(a[0, j]), int(a[1, j])
        assert Fraction(float(u[j])) == Fraction((hi >> 5) * (1 << 26) + (lo >> 6), 1 << 53) and u[j] == rh.u53(hi, lo)
    assert cases.u53([0xFFFFFFFF], [0xFFFFFFFF])[0] == 1 - 2.0 ** -53 and cases.u53([0], [0])[0] == 0.0
