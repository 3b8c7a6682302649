"""The capped-softmax numerators exp(cap tanh(x / cap)) of the attention kernels, restated in fp32 NumPy with the
constants parsed from the sources, against fp64.  CPU only.

  * capped_exp16 (videoprism-mlx_amd/csrc/vp_common.h; attention_long_bf16 and the spatial kernel): the LIN / QUAD /
    cubic tiers exp2(x P(x^2)) with the coefficients make_cap_poly folds (log2e t_i / cap^(2i)), over each tier's whole
    range |x| <= factor cap, and capped_exp_exact out to |x| = 4 cap;
  * capped_exp_f32x16 (attention.hip; attention_f32_mfma): the degree-5 fit, the 0.55 cap threshold, the clamp at 64,
    the hi / lo split of log2e, out to |x| = 4 cap;
  * caps 50, 20, 5 and 1: a mistake in folding cap^(-2i) into the coefficients cancels at no two caps.

Every error below is the relative error of the numerator, |p / exp(cap tanh(x / cap)) - 1|, which to first order is
the absolute error of the natural-log exponent.  The bars are derived from the operations, none is fitted to what
the code gives (u = 2^-24, the relative error of one fp32 rounding; edge = factor cap):

  polynomial tiers.  cap tanh(x / cap) = x T((x/cap)^2) and the fit of T has the relative error the header states
    (LIN 1.7e-6, QUAD 3.5e-7, cubic 4.5e-7), so the exponent is off by at most fit * |x| <= fit * edge.  The base-2
    exponent g = x P(x^2), |g| <= edge log2e, carries about four fp32 roundings of relative size u (x * x, the last
    fma, x * P and the folded coefficient; the inner fmas are scaled down by (x/cap)^2 <= 0.23): 4 u edge log2e in
    base 2, times ln 2 for the numerator:
        bar = fit * edge + 4 * 2^-24 * edge        cap 50: 9.69e-6 / 7.06e-6 / 1.65e-5   (measured 8.6e-6 / 4.4e-6 / 1.13e-5)
    v_exp_f32's own result error (1 ulp, 1.2e-7) is not in it; it is 1 % of the bar at cap 50 but comparable to the
    bar at cap 1 (edge 0.1: 1.9e-7), so the tests compare the fp32 exponent g through an fp64 exp2 there: what the
    tiers own is g, the instruction's rounding is the same for every tier.  The fp32 numerator is held to bar + 2^-24
    (NumPy's exp2 rounds to nearest); the GPU test adds 2^-23 for the instruction.

  capped_exp_exact(x) = exp2(c2 - 2 c2 r), r = rcp(exp2(x c1) + 1), c1 = 2 log2e / cap, c2 = cap log2e.  With
    a = x c1 (two roundings: c1 and the product, |da| <= 2 u |a|), t = exp2(a) is off by ln2 |da| + 2u relative
    (v_exp_f32: 1 ulp), r by e_r = (t / (t + 1)) (2 u ln2 |a| + 2u) + u + 2u (the add, v_rcp_f32: 1 ulp), the exponent
    c2 (1 - 2 r) by 2 c2 r e_r plus one rounding of each of 2 c2 r and the difference (or one of the fma) and the
    rounding of c2 itself; times ln 2 (ln2 c2 = cap), plus the last exp2:
        bar(x) = cap (2 r e_r + u (2 r + |1 - 2 r|) + u (1 + 2 r)) + 2u
    At cap 50: 3.6e-5 as x -> -inf (r -> 1), 2.1e-5 at 0, 6.1e-6 as x -> +inf.

  capped_exp_f32x16.  |x| < 0.55 cap: t = x * (1/cap) (two roundings), u = t^2 (rel. 5u), P's error is
    |c1| u 5u <= 0.5u plus its own last rounding and the inner ones (< 0.5u): 2u, and g = x P one more: |dg| <= 3u |g|
    plus the fit's 9.4e-10 |g| (header).  Else g = cap (1 - 2 r), r = 1 / (exp2(a2) + 1), a2 = |x| k2 clamped to 64
    (k2 = 2 log2e / cap: rel. 2u, the product 1 more): exp2 off by 3u ln2 a2 + 2u, r by e_r = that + u (the add) + u
    (the Newton step's last fma), 1 - 2 r by 2 r e_r + u (1 - 2 r), the product with cap by u:
        |dg| <= cap 2 r e_r + 2u |g|
    The compensated exponential adds only v_exp_f32's 2u and the last fma's u (the product g log2e is recovered by
    the hi / lo fma to ~u^2):
        bar(x) = |dg| + 3u
    At cap 50: 4.9e-6 below 0.55 cap, at most 1.7e-5 above it.  (The header's emulation measured 5.4e-6 on |x| <= 200;
    the dense grid here finds 7.7e-6 at x = -38.7, 2.1e-6 below the threshold: both inside the bar.)

Negative control: each tier's polynomial over the next tier's range is past its own bar by more than 100x (LIN over
the QUAD range 4.3e-3, QUAD over the cubic range 9.3e-3), so a wrong threshold is a wrong result, not a slower one.
"""

import os
import re

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videoprism-mlx_amd", "csrc")
CAPS = (50.0, 20.0, 5.0, 1.0)
TIERS = ("LIN", "QUAD", "CUBIC")
FACTORS = {"LIN": 0.10, "QUAD": 0.24, "CUBIC": 0.48}        # a tier's range: group maximum <= factor * cap
FIT_ERR = {"LIN": 1.7e-6, "QUAD": 3.5e-7, "CUBIC": 4.5e-7}  # the header's stated fit errors
F32_FIT_ERR = 9.4e-10
U = 2.0 ** -24
LOG2E = 1.4426950408889634
f32 = np.float32


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; the sum is rounded to 53 bits, then to 24."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def parse_cap_poly():
    """t[] (cubic), u[] (QUAD), w[] (LIN) and the threshold factors of make_cap_poly, from the header's text."""
    src = open(os.path.join(CSRC, "vp_common.h")).read()
    body = src[src.index("inline CapPoly make_cap_poly(float cap)"):]
    body = body[:body.index("\n}\n")]
    coef = {}
    for name, n in (("t", 4), ("u", 3), ("w", 2)):
        m = re.search(r"const double %s\[%d\] = \{([^}]*)\};" % (name, n), body)
        coef[name] = [float(v) for v in m.group(1).split(",")]
        assert len(coef[name]) == n
    fac = [f32(v) for v in re.findall(r"(\d\.\d+)f \* cap", body)]
    assert len(fac) == 3  # x0 (cubic), x1 (QUAD), x2 (LIN), in the struct's order
    assert re.search(r"const double l2e = 1\.4426950408889634, c2 = \(double\)cap \* cap;", body)
    return coef, {"CUBIC": fac[0], "QUAD": fac[1], "LIN": fac[2]}


def make_cap_poly(cap):
    """make_cap_poly: the coefficients folded in double, rounded to fp32; the thresholds as fp32 products."""
    coef, fac = parse_cap_poly()
    c2 = float(f32(cap)) * float(f32(cap))
    fold = lambda c: [f32(LOG2E * v / c2 ** i) for i, v in enumerate(c)]
    return {"CUBIC": fold(coef["t"]), "QUAD": fold(coef["u"]), "LIN": fold(coef["w"]),
            "x": {k: f32(v * f32(cap)) for k, v in fac.items()}}


def tier_exponent(x, cp, tier):
    """The base-2 exponent x * P(x^2) of a polynomial tier in fp32, capped_exp16's operation order."""
    x = np.asarray(x, f32)
    k = cp[tier]
    u = (x * x).astype(f32)
    P = _fma(k[-1], u, k[-2])
    for i in range(len(k) - 3, -1, -1):
        P = _fma(P, u, k[i])
    return (x * P).astype(f32)


def capped_exp_tier(x, cp, tier):
    return np.exp2(tier_exponent(x, cp, tier)).astype(f32)


def capped_exp_exact(x, cap):
    """capped_exp_exact with attention_long_kernel.h's c1 = 2 log2e / cap, c2 = cap log2e (kLog2e a float)."""
    x = np.asarray(x, f32)
    l2e, cap = f32(LOG2E), f32(cap)
    c1, c2 = f32(f32(2.0) * l2e / cap), f32(cap * l2e)
    with np.errstate(over="ignore"):  # exp2 -> inf, rcp -> 0 past |x| ~ 44 cap, as on the device
        t = np.exp2((x * c1).astype(f32)).astype(f32)
        r = (f32(1.0) / (t + f32(1.0)).astype(f32)).astype(f32)
    return np.exp2(_fma(-(f32(2.0) * c2), r, c2)).astype(f32)


def parse_f32x16():
    src = open(os.path.join(CSRC, "attention.hip")).read()
    body = src[src.index("void capped_exp_f32x16("):]
    body = body[:body.index("\n}\n")]
    c = [f32(re.search(r"\bc%d = (-?[\d.e-]+)f" % i, body).group(1)) for i in range(6)]
    k = {n: f32(re.search(r"\b%s = (-?[\d.e-]+)f" % n, body).group(1)) for n in ("kL", "kLlo", "kLn2")}
    thr = f32(re.search(r"xthr = ([\d.]+)f \* cap", body).group(1))
    clamp = f32(re.search(r"fminf\(fabsf\(x\[i\]\) \* k2, ([\d.]+)f\)", body).group(1))
    assert "mx >= xthr" in body and "fabsf(x[i]) < xthr ? g : gl" in body
    return c, k, thr, clamp


def capped_exp_f32x16(x, cap):
    """capped_exp_f32x16 per value: the tile ballot only skips the exp form where no |x| reaches the threshold, the
    select fabsf(x) < xthr decides each value."""
    c, k, thr, clamp = parse_f32x16()
    x = np.asarray(x, f32)
    cap = f32(cap)
    inv_cap = f32(f32(1.0) / cap)
    xthr, k2 = f32(thr * cap), f32(f32(2.0) * k["kL"] * inv_cap)
    with np.errstate(over="ignore", invalid="ignore"):  # the polynomial of a huge |x| overflows and is not selected
        t = (x * inv_cap).astype(f32)
        u = (t * t).astype(f32)
        P = _fma(c[5], u, c[4])
        for i in (3, 2, 1, 0):
            P = _fma(P, u, c[i])
        g = (x * P).astype(f32)
        a2 = np.minimum((np.abs(x) * k2).astype(f32), clamp)
    d = (np.exp2(a2).astype(f32) + f32(1.0)).astype(f32)
    r0 = (f32(1.0) / d).astype(f32)
    r = _fma(r0, _fma(-d, r0, f32(1.0)), r0)
    gl = np.copysign((cap * _fma(f32(-2.0), r, f32(1.0))).astype(f32), x)
    g = np.where(np.abs(x) < xthr, g, gl).astype(f32)
    p = (g * k["kL"]).astype(f32)
    lo = _fma(g, k["kLlo"], _fma(g, k["kL"], -p))
    E = np.exp2(p).astype(f32)
    return _fma(E, (lo * k["kLn2"]).astype(f32), E)


def numerator(x, cap):
    x = np.asarray(x, np.float64)
    return np.exp(cap * np.tanh(x / cap))


def tier_bar(tier, cap):
    """fit * edge + 4 * 2^-24 * edge (module docstring), edge = factor * cap."""
    edge = FACTORS[tier] * cap
    return FIT_ERR[tier] * edge + 4 * U * edge


def exact_bar(x, cap):
    x = np.asarray(x, np.float64)
    a = 2.0 * LOG2E * x / cap
    r = 1.0 / (np.exp2(a) + 1.0)
    e_r = (1.0 - r) * (2 * U * np.log(2.0) * np.abs(a) + 2 * U) + 3 * U
    return cap * (2 * r * e_r + U * (2 * r + np.abs(1 - 2 * r)) + U * (1 + 2 * r)) + 2 * U


def f32x16_bar(x, cap):
    x = np.asarray(x, np.float64)
    thr = float(parse_f32x16()[2])
    g = np.abs(cap * np.tanh(x / cap))
    a2 = np.minimum(2.0 * LOG2E * np.abs(x) / cap, 64.0)
    r = 1.0 / (np.exp2(a2) + 1.0)
    e_r = 3 * U * np.log(2.0) * a2 + 2 * U + 2 * U
    poly = (3 * U + F32_FIT_ERR) * g
    big = cap * 2 * r * e_r + 2 * U * g
    # a value within an fp32 rounding of the threshold may take either form
    near = np.abs(np.abs(x) - thr * cap) <= 4 * U * thr * cap
    return np.where(near, np.maximum(poly, big), np.where(np.abs(x) < thr * cap, poly, big)) + 3 * U


def _grid(lo, hi, n=200001):
    """fp32 values of both signs with lo <= |x| <= hi (fp32 bounds), the ends included."""
    lo, hi = f32(lo), f32(hi)
    x = np.linspace(float(lo), float(hi), n).astype(f32)
    x = np.clip(x, lo, hi)
    return np.concatenate([x, -x])


def _rel(p, x, cap):
    n = numerator(x, cap)
    return np.abs(np.asarray(p, np.float64) / n - 1.0)


def test_threshold_factors():
    coef, fac = parse_cap_poly()
    assert fac == {k: f32(v) for k, v in FACTORS.items()}
    assert parse_f32x16()[2] == f32(0.55) and parse_f32x16()[3] == f32(64.0)
    # T(0) = 1 and T'(0) = -1/3 to within the fits' errors: the arrays are in ascending order of the power
    for name in "tuw":
        assert abs(coef[name][0] - 1.0) < 2e-6 and abs(coef[name][1] + 1.0 / 3.0) < 2e-3


def test_tier_bars_at_cap_50():
    """The derivation's figures, so a change of the parsed factors or of the formula shows here."""
    bars = [tier_bar(t, 50.0) for t in TIERS]
    np.testing.assert_allclose(bars, [9.69e-6, 7.06e-6, 1.65e-5], rtol=5e-3)
    assert 3.5e-5 < exact_bar(-200.0, 50.0) < 3.7e-5 and 2.0e-5 < exact_bar(0.0, 50.0) < 2.2e-5
    assert exact_bar(200.0, 50.0) < 6.2e-6
    assert f32x16_bar(27.0, 50.0) < 5.0e-6 and f32x16_bar(np.linspace(-200, 200, 4001), 50.0).max() < 1.7e-5


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("tier", TIERS)
def test_polynomial_tier_within_bar(tier, cap):
    cp = make_cap_poly(cap)
    x = _grid(0.0, cp["x"][tier])
    assert np.abs(x).max() == cp["x"][tier]  # the threshold itself belongs to the tier (the ballot is mx > x)
    g = tier_exponent(x, cp, tier)
    err_g = _rel(np.exp2(g.astype(np.float64)), x, cap)      # the tier's own error: the fp32 exponent
    err_p = _rel(capped_exp_tier(x, cp, tier), x, cap)        # with exp2's fp32 result rounding
    bar = tier_bar(tier, cap)
    print(f"{tier} cap {cap}: exponent {err_g.max():.3e}, numerator {err_p.max():.3e}, bar {bar:.3e}")
    assert err_g.max() <= bar, (err_g.max(), bar)
    assert err_p.max() <= bar + U, (err_p.max(), bar)


@pytest.mark.parametrize("cap", CAPS)
def test_exact_form_within_bar(cap):
    x = np.concatenate([_grid(0.0, 4.0 * cap), _grid(0.0, 0.5 * cap)])
    err = _rel(capped_exp_exact(x, cap), x, cap)
    bar = exact_bar(x, cap)
    print(f"exact cap {cap}: max {err.max():.3e}, largest err / bar {(err / bar).max():.3f}")
    assert np.all(err <= bar), (err / bar).max()


def test_exact_form_saturates():
    """Past the grid: exp2 overflows to inf, rcp gives 0 and the numerator is e^cap; -> e^-cap on the other side."""
    p = capped_exp_exact(np.array([1e4, -1e4, 3e38, -3e38], f32), 50.0).astype(np.float64)
    np.testing.assert_allclose(p, np.exp([50.0, -50.0, 50.0, -50.0]), rtol=4e-5)


@pytest.mark.parametrize("cap", CAPS)
def test_f32x16_within_bar(cap):
    thr = float(parse_f32x16()[2]) * cap
    x = np.concatenate([_grid(0.0, 4.0 * cap), _grid(0.0, thr), _grid(0.99 * thr, 1.01 * thr),
                        np.array([1e4, -1e4, 3e38, -3e38], f32)])
    err = _rel(capped_exp_f32x16(x, cap), x, cap)
    bar = f32x16_bar(x, cap)
    print(f"f32x16 cap {cap}: max {err.max():.3e}, largest err / bar {(err / bar).max():.3f}")
    assert np.all(err <= bar), (err / bar).max()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("tier,nxt", [("LIN", "QUAD"), ("QUAD", "CUBIC"), ("CUBIC", None)])
def test_tier_polynomial_fails_beyond_its_threshold(tier, nxt, cap):
    """Why the thresholds matter: over the next tier's range (for the cubic, the exact form's, up to twice its
    threshold) a tier's polynomial is past its own bar by more than 100x."""
    cp = make_cap_poly(cap)
    hi = cp["x"][nxt] if nxt else f32(2.0) * cp["x"][tier]
    x = _grid(cp["x"][tier], hi)
    err = _rel(capped_exp_tier(x, cp, tier), x, cap).max()
    print(f"{tier} polynomial over ({float(cp['x'][tier]):.3g}, {float(hi):.3g}], cap {cap}: {err:.3e}")
    assert err > 100 * tier_bar(tier, cap), (err, tier_bar(tier, cap))
    if cap == 50.0 and nxt:
        np.testing.assert_allclose(err, {"LIN": 4.3e-3, "QUAD": 9.3e-3}[tier], rtol=0.05)
