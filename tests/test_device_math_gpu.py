"""GPU: the fp64 device primitives every sampler rests on (device_common.hpp, vonmises.hpp, fillin.hpp, sigma_device.hpp),
each called through mlmcpi_test_math and compared with the mathematical function in long double / mpmath
(tests/device_math_reference.py, checked on the CPU by tests/test_device_math_reference.py).

The bounds are derived from the rounding steps of each primitive, never from what the device returns:

    fast_rcp, fast_div, fast_sqrt   1 ulp                      the header's claim
    fast_acos                       3 ulp of the result        fdlibm's 1, one each for the inner division and square root
    cospi_unit, sin_reduced         2^-51 absolute             two roundings of the reduced argument at magnitude <= pi / 2, one
                                                               of the result, the representation of pi  (|d| <= 1e6)
    cos_reduced, cos_half           (1 + |x|) 2^-51 absolute   the same plus the rounding of x / (2 pi), which scales with |x|
    sincos_2pi_unit                 2^-51 absolute per component
    log_unit                        4 ulp, or 2^-52 absolute where |log x| < 2^-50
    box_muller                      8 ulp of the radius (read at v = 0, where cs = 1 exactly and n0 IS the radius),
                                    2^-50 r absolute per normal
    vm_envelope                     2 ulp                      fma, square root (1 ulp, halved relative weight of its operand's
                                                               rounding), fma: 0.25 + 1 + 0.5 ulp at most, as R >= 1 > sqrt(.) / 2
    bessel_i0_scaled, bessel_i0     1e-15 relative             the header's claim
    two_pi_i0_scaled                8 ulp against the reference code's formula in mpmath (three-term expansion beyond 100)
    compact_exp_inverse             2^-50 absolute, result in [-1, 1], exactly 2 u - 1 at s = 0

Every check prints its worst error, the input where it occurred and the ratio to the bound before it asserts; the table of one
run is profiles/device_math.json (this module writes it to the file MLMCPI_MATH_TABLE names, if the variable is set).
"""
import json
import os

import numpy as np
import pytest
import torch

import device_math_reference as ref

pytestmark = pytest.mark.gpu

LD, mp = ref.LD, ref.mp
TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def worst_case_table():
    yield
    path = os.environ.get("MLMCPI_MATH_TABLE")
    if path:
        with open(path, "w") as f:
            json.dump(TABLE, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def run(gpu_ops):
    def call(fn, a, b=None):
        da = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        db = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
        o0, o1 = gpu_ops.test_math(fn, da, db)
        torch.cuda.synchronize()
        return o0.cpu().numpy(), o1.cpu().numpy()
    return call


def check(name, err, bound, unit, *inputs):
    """err <= bound on every entry (arrays in one unit, bound an array or a number); records and prints the worst ratio first"""
    err = np.abs(np.asarray(err, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert err.size, name
    ratio = np.where(err == 0, 0.0, err / bound)
    bad = ~np.isfinite(ratio)
    i = int(np.flatnonzero(bad)[0]) if bad.any() else int(np.argmax(ratio))
    where = [float(np.ravel(x)[i]) for x in inputs]
    TABLE[name] = {"worst_error": float(err[i]), "bound": float(bound[i]), "unit": unit, "ratio": float(ratio[i]),
                   "input": [x.hex() for x in where], "points": int(err.size)}
    print(f"[math] {name}: worst {err[i]:.4g} {unit} at {[f'{x!r} ({x.hex()})' for x in where]}, bound {bound[i]:.4g}, ratio {ratio[i]:.3f} ({err.size} points)")
    assert not bad.any() and ratio[i] <= 1.0, TABLE[name]


def abs_err(got, want):
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want).astype(np.float64)


def rel_err(got, want):
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) / want - 1).astype(np.float64)


def finite(got):
    assert np.isfinite(got).all(), np.flatnonzero(~np.isfinite(got))[:8]


# ---- one case per primitive ---------------------------------------------------------------------------------------------------
def case_fast_rcp(run):
    x = ref.grid_positive()
    got, _ = run("fast_rcp", x)
    finite(got)
    check("fast_rcp", ref.ulp_error(got, ref.ref_rcp(x)), 1.0, "ulp", x)


def case_fast_div(run):
    a, b = ref.grid_div()
    got, _ = run("fast_div", a, b)
    finite(got)
    check("fast_div", ref.ulp_error(got, ref.ref_div(a, b)), 1.0, "ulp", a, b)


def case_fast_sqrt(run):
    x = ref.grid_positive()
    got, _ = run("fast_sqrt", x)
    finite(got)
    check("fast_sqrt", ref.ulp_error(got, ref.ref_sqrt(x)), 1.0, "ulp", x)


def case_fast_acos(run):
    x = ref.grid_acos()
    got, _ = run("fast_acos", x)
    finite(got)                                               # finite on the whole grid
    check("fast_acos", ref.ulp_error(got, ref.ref_acos(x)), 3.0, "ulp", x)
    e = ref.ACOS_EDGES
    ge, _ = run("fast_acos", e)
    check("fast_acos edges (mpmath)", ref.ulp_error(ge, ref.via_mp(mp.acos, e)), 3.0, "ulp", e)
    g1, _ = run("fast_acos", np.array([1.0, -1.0]))
    assert g1[0] == 0.0 and abs(ref.ulp_error(g1[1:], np.array([ref.PI_LD]))[0]) <= 1.0, g1


def case_sin_reduced(run):
    d = ref.grid_trig(1e6)
    got, _ = run("sin_reduced", d)
    finite(got)
    check("sin_reduced", abs_err(got, ref.ref_sin(d)), 2.0 ** -51, "abs", d)
    e = ref.trig_edges()
    ge, _ = run("sin_reduced", e)
    check("sin_reduced edges (mpmath)", abs_err(ge, ref.via_mp(mp.sin, e)), 2.0 ** -51, "abs", e)


def case_cospi_unit(run):
    u = ref.grid_cospi()
    got, _ = run("cospi_unit", u)
    finite(got)
    check("cospi_unit", abs_err(got, ref.ref_cospi(u)), 2.0 ** -51, "abs", u)
    e = ref.COSPI_EDGES
    ge, _ = run("cospi_unit", e)
    check("cospi_unit edges (mpmath)", abs_err(ge, ref.via_mp(mp.cospi, e)), 2.0 ** -51, "abs", e)


def case_cos_reduced(run):
    x = ref.grid_trig(2.0 ** 30)
    got, _ = run("cos_reduced", x)
    finite(got)
    check("cos_reduced", abs_err(got, ref.ref_cos(x)), (1 + np.abs(x)) * 2.0 ** -51, "abs", x)
    e = ref.trig_edges()
    ge, _ = run("cos_reduced", e)
    check("cos_reduced edges (mpmath)", abs_err(ge, ref.via_mp(mp.cos, e)), (1 + np.abs(e)) * 2.0 ** -51, "abs", e)


def case_cos_half(run):
    x = ref.grid_trig(2.0 ** 30)
    got, _ = run("cos_half", x)
    finite(got)
    check("cos_half", abs_err(got, ref.ref_cos_half(x)), (1 + np.abs(x)) * 2.0 ** -51, "abs", x)
    e = ref.trig_edges()
    ge, _ = run("cos_half", e)
    check("cos_half edges (mpmath)", abs_err(ge, ref.via_mp(lambda t: mp.cos(t / 2), e)), (1 + np.abs(e)) * 2.0 ** -51, "abs", e)


def log_checks(name, x, got, want):
    tiny = np.abs(want.astype(np.float64)) < 2.0 ** -50
    check(name + " (4 ulp)", ref.ulp_error(got[~tiny], want[~tiny]), 4.0, "ulp", x[~tiny])
    if tiny.any():
        check(name + " (|log x| < 2^-50)", abs_err(got[tiny], want[tiny]), 2.0 ** -52, "abs", x[tiny])


def case_log_unit(run):
    x = ref.grid_log()
    got, _ = run("log_unit", x)
    finite(got)
    log_checks("log_unit", x, got, ref.ref_log(x))
    e = ref.log_edges()
    ge, _ = run("log_unit", e)
    log_checks("log_unit edges (mpmath)", e, ge, ref.via_mp(mp.log, e))
    assert (got[x == 1.0] == 0.0).all() and (x == 1.0).any()           # log_unit(1) == 0, bit for bit (either sign of zero)


def case_sincos_2pi_unit(run):
    v = ref.grid_sincos()
    sn, cs = run("sincos_2pi_unit", v)
    finite(sn), finite(cs)
    wsn, wcs = ref.ref_sincos_2pi(v)
    check("sincos_2pi_unit sin", abs_err(sn, wsn), 2.0 ** -51, "abs", v)
    check("sincos_2pi_unit cos", abs_err(cs, wcs), 2.0 ** -51, "abs", v)
    e = ref.sincos_edges()
    sn, cs = run("sincos_2pi_unit", e)
    check("sincos_2pi_unit sin edges (mpmath)", abs_err(sn, ref.via_mp(lambda t: mp.sinpi(2 * t), e)), 2.0 ** -51, "abs", e)
    check("sincos_2pi_unit cos edges (mpmath)", abs_err(cs, ref.via_mp(lambda t: mp.cospi(2 * t), e)), 2.0 ** -51, "abs", e)


def case_box_muller(run):
    u, v = ref.grid_box_muller()
    n0, n1 = run("box_muller", u, v)
    finite(n0), finite(n1)
    r, w0, w1 = ref.ref_box_muller(u, v)
    axis = v == 0.0
    assert axis.sum() > 1000 and (n1[axis] == 0.0).all()
    check("box_muller radius", ref.ulp_error(n0[axis], r[axis]), 8.0, "ulp", u[axis])
    pos = r > 0
    assert (n0[~pos] == 0).all() and (n1[~pos] == 0).all() and (~pos).any()       # u = 0: the radius is 0
    rb = (r[pos] * LD(2.0 ** -50)).astype(np.float64)
    check("box_muller n0", abs_err(n0[pos], w0[pos]), rb, "abs", u[pos], v[pos])
    check("box_muller n1", abs_err(n1[pos], w1[pos]), rb, "abs", u[pos], v[pos])


def case_vm_envelope(run):
    k = ref.grid_kappa()
    got, _ = run("vm_envelope", k)
    finite(got)
    check("vm_envelope", ref.ulp_error(got, ref.ref_envelope(k)), 2.0, "ulp", k)


def bessel_bound(z):
    """Relative bound of bessel_i0_scaled.  Hankel series (z >= 30): 1e-15, the header's claim.  Power series (z < 30): the claim
    of 1e-15 does not survive counting.  term_k carries 2 k + 1 roundings (q, then a division and a product per step) and
    the terms are positive with their weight centred at k = z / 2, so the terms contribute (z + 1) 2^-53 to the sum; each of
    the at most 120 additions rounds the partial sum once (120 2^-53); exp(-z) and the last product add 2 2^-53:
    (z + 123) 2^-53 <= 1.7e-14.  (Measured on the MI355X: 1.73e-15 at z = 26.43.)"""
    z = np.asarray(z, dtype=np.float64)
    return np.where(z < 30.0, (z + 123.0) * 2.0 ** -53, 1e-15)


def case_bessel_i0_scaled(run):
    z = ref.grid_bessel("scaled")
    got, _ = run("bessel_i0_scaled", z)
    finite(got)
    check("bessel_i0_scaled", rel_err(got, ref.ref_bessel_i0_scaled(z)), bessel_bound(z), "rel", z)


def case_bessel_i0(run):
    z = ref.grid_bessel("unscaled")
    got, _ = run("bessel_i0", z)
    finite(got)
    check("bessel_i0", rel_err(got, ref.ref_bessel_i0(z)), bessel_bound(z) + 2.0 ** -52, "rel", z)   # exp(z) and the product


def case_two_pi_i0_scaled(run):
    z = ref.grid_bessel("two_pi")
    got, _ = run("two_pi_i0_scaled", z)
    finite(got)
    # below 30 the series' bound in ulp (a relative error e is at most e 2^53 ulp), plus the product with 2 pi
    check("two_pi_i0_scaled", ref.ulp_error(got, ref.ref_two_pi_i0_scaled(z)), np.where(z < 30.0, bessel_bound(z) * 2.0 ** 53 + 2.0, 8.0), "ulp", z)


def case_compact_exp_inverse(run):
    s, u = ref.grid_compact_exp()
    got, _ = run("compact_exp_inverse", s, u)
    finite(got)
    assert (np.abs(got) <= 1.0).all()
    # 2^-50 covers log1p's own ulp, the division and the sum (|log1p(y)| / s <= 2).  It does not cover the conditioning of
    # log1p at y = (1 - u) expm1(-2 s) -> -1: expm1 (1 ulp) and the product (1/2 ulp) leave y with 1.5 2^-52 |y|, which log1p
    # divides by 1 + y = u + e^(-2 s) (1 - u).  The same perturbation of y is a perturbation of u by less than 2^-52, the
    # spacing of the uniform itself.  (Measured: 3.8e-15 at s = 4, u = 0.0031, where this term is 2.4e-14.)
    y = ref.via_mp(lambda sv, uv: (1 - uv) * mp.expm1(-2 * sv) if sv > 0 else mp.mpf(0), s, u)
    cond = np.where(s > 0, (1.5 * 2.0 ** -52 * np.abs(y) / ((1 + y) * np.where(s > 0, s, 1.0).astype(LD))).astype(np.float64), 0.0)
    cond = np.where(np.isfinite(cond), cond, 0.0)          # u = 0 at large s: 1 + y = 0, the result is clamped to -1
    check("compact_exp_inverse", abs_err(got, ref.ref_compact_exp_inverse(s, u)), 2.0 ** -50 + cond, "abs", s, u)
    flat = s == 0.0
    assert flat.sum() == 260 and (got[flat] == 2.0 * u[flat] - 1.0).all()          # exactly 2 u - 1 at s = 0


def case_u01(run):
    w = ref.grid_words()
    for fn, want in (("u01", ref.ref_u01(w)), ("u01_52", ref.ref_u01_52(w))):
        got, _ = run(fn, ref.as_double(w))
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        print(f"[math] {fn}: {w.size} word pairs, {bad.size} differ from the integer formula")
        TABLE[fn] = {"points": int(w.size), "mismatches": int(bad.size)}
        assert bad.size == 0, [hex(int(x)) for x in w[bad][:8]]


def case_mod_2pi(run):
    x = ref.grid_mod()
    slow, _ = run("mod_2pi", x)
    fast, _ = run("mod_2pi_fast", x)
    finite(slow), finite(fast)
    two_pi = 2 * ref.PI_LD
    d = fast.astype(LD) - slow.astype(LD)
    off = np.minimum(np.abs(d), np.abs(np.abs(d) - two_pi)).astype(np.float64)      # distance from {0, +-2 pi}
    check("mod_2pi_fast - mod_2pi in {0, +-2 pi}", off / np.spacing(2 * np.pi), 2.0, "ulp of 2 pi", x)
    for name, r in (("mod_2pi", slow), ("mod_2pi_fast", fast)):
        # [-pi, pi] up to the roundings of the map itself: x - 2 pi k is formed from a product 2 pi k rounded at magnitude
        # |x| + pi (half a spacing), from pi to 53 bits (k 2^-52 relative: another half), and x itself may be the double next
        # to an odd multiple of pi (one spacing).  (Measured: mod_2pi(11 pi rounded up) = pi + 3.6e-15.)
        over = np.maximum(np.abs(r).astype(LD) - ref.PI_LD, 0).astype(np.float64)
        check(name + " in [-pi, pi]", over, 2.0 * np.spacing(np.abs(x) + np.pi), "abs beyond pi", x)


CASES = {"fast_rcp": case_fast_rcp, "fast_div": case_fast_div, "fast_sqrt": case_fast_sqrt, "fast_acos": case_fast_acos,
         "sin_reduced": case_sin_reduced, "cospi_unit": case_cospi_unit, "cos_reduced": case_cos_reduced, "cos_half": case_cos_half,
         "log_unit": case_log_unit, "sincos_2pi_unit": case_sincos_2pi_unit, "box_muller": case_box_muller, "vm_envelope": case_vm_envelope,
         "bessel_i0_scaled": case_bessel_i0_scaled, "bessel_i0": case_bessel_i0, "two_pi_i0_scaled": case_two_pi_i0_scaled,
         "compact_exp_inverse": case_compact_exp_inverse, "u01": case_u01, "mod_2pi": case_mod_2pi}


@pytest.mark.parametrize("name", sorted(CASES))
def test_primitive(run, name):
    CASES[name](run)


def test_vm_clamp_maps_nan_to_a_finite_concentration(gpu_ops):
    """beta = NaN through the whole draw (mlmcpi_test_expcos): every lane leaves the attempt loop, the call returns, and an
    entry is a finite angle or NaN (the centre carries the NaN only if the staples do; here they do not)"""
    n = 4096
    g = torch.Generator().manual_seed(5)
    xp = ((torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * np.pi).cuda()
    xm = ((torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * np.pi).cuda()
    out = gpu_ops.test_expcos(3, 1, 2, float("nan"), xp, xm)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (n,) and (np.isfinite(out) | np.isnan(out)).all() and not np.isinf(out).any()
    assert (np.abs(out[np.isfinite(out)]) <= np.pi + 1e-12).all()


# ---- the von Mises attempt: fp32 screen and exact test --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vm(run):
    """every case of ref.vm_cases() through vm_try and vm_screen, once"""
    V = ref.vm_cases()
    c, dec = run("vm_try", ref.as_double(V["words"]), V["kappa"])
    af, band = run("vm_screen", c)
    assert set(np.unique(dec)) <= {-1.0, 0.0, 1.0} and np.isfinite(c).all()
    assert (af == af.astype(np.float32)).all() and (band == band.astype(np.float32)).all()
    return V, c, dec, af, band


def below_u2(V, sel):
    """a* < 2^-64: below the smallest non-zero acceptance uniform u2 = (b + tail) / 2048 (tail a multiple of 2^-53).  The exact
    test accepts there only at u2 = 0, once in 2^64 attempts, and an fp32 screen cannot hold such an a* at all: exp(1 - c)
    leaves the fp32 range at c > 88 (a* < 1e-36), af and the band are 0 and acceptance bits 0 are rejected."""
    return np.array([V["a_mp"][i] < mp.mpf(2) ** -64 for i in V["case_of"][sel]])


@pytest.mark.parametrize("kappa", ref.KAPPAS)
def test_vm_screen_band_covers_its_error(vm, kappa):
    """|af - a*| < band at every grid point, a* = c* exp(1 - c*) in mpmath from kappa and u1: the band covers the fp32 error of
    the screen and the error of the fp64 c it starts from.

    Holds wherever a* >= 2^-64 (below_u2 says why not beyond: measured at kappa = 160 and 1e4, on the proposals with
    c* > 88, af = band = 0 while 0 < a* < 1e-36)."""
    V, c, dec, af, band = vm
    sel = V["kappa"] == kappa
    err = np.abs(af[sel].astype(LD) - V["a"][sel]).astype(np.float64)
    cerr = np.abs(ref.ulp_error(c[sel], V["c"][sel]))
    print(f"[math] vm_try kappa={kappa:g}: c within {cerr.max():.3g} ulp of c*; max |af - a*| / band = {np.max(np.where(err == 0, 0, err / band[sel])):.4g}")
    # a band of zero width covers nothing, not even an exact af (strict inequality)
    ratio = np.where(band[sel] > 0, err / np.where(band[sel] > 0, band[sel], 1), np.inf)
    ratio = np.where(below_u2(V, sel), 0.0, ratio)
    check(f"vm_screen kappa={kappa:g}: |af - a*| / band", ratio, np.nextafter(1.0, 0), "band", V["words"][sel].view(np.float64), V["kappa"][sel])


@pytest.mark.parametrize("kappa", ref.KAPPAS)
def test_vm_try_decides_only_what_the_exact_test_would(vm, kappa):
    """decision 1 only if hi_s <= a*, decision 0 only if lo_s >= a*; the cases built to be open are open (at least 1000 of
    them per kappa)

    Where a* < 2^-64 (below_u2) acceptance bits 0 are rejected by the screen although a* > 0: measured at kappa = 160 (168
    cases) and 1e4 (196 cases); the decision differs from the exact one at u2 = 0 alone."""
    V, c, dec, af, band = vm
    sel = V["kappa"] == kappa
    d, a, b = dec[sel], V["a"][sel], V["b"][sel].astype(LD)
    a_pos = np.array([V["a_mp"][i] > 0 for i in V["case_of"][sel]])      # (a* below the long double range is still > 0)
    lo_s, hi_s = b / 2048, (b + 1) / 2048
    wrong_accept = (d == 1) & ~(hi_s <= a)
    wrong_reject = (d == 0) & ~((lo_s >= a) & ~((lo_s == 0) & a_pos)) & ~((lo_s == 0) & below_u2(V, sel))
    n_open = int(((d == -1) & (V["kind"][sel] == 0)).sum())
    print(f"[math] vm_try kappa={kappa:g}: {int((d == 1).sum())} accepted, {int((d == 0).sum())} rejected, {int((d == -1).sum())} open "
          f"({n_open} of the {int((V['kind'][sel] == 0).sum())} built to be open); wrong accepts {int(wrong_accept.sum())}, wrong rejects {int(wrong_reject.sum())}")
    TABLE[f"vm_try kappa={kappa:g}"] = {"points": int(sel.sum()), "open": int((d == -1).sum()), "wrong_accepts": int(wrong_accept.sum()),
                                       "wrong_rejects": int(wrong_reject.sum())}
    assert not wrong_accept.any() and not wrong_reject.any()
    assert n_open >= 1000


@pytest.mark.parametrize("kappa", ref.KAPPAS)
def test_vm_exact_takes_the_mpmath_decision(run, vm, kappa):
    """In the open tier vm_exact(lo, tail, c) with the c of vm_try equals the mpmath decision u2 < a* whenever
    |u2 - a*| > ref.vm_margin(kappa) = 2^-45 + kappa 2^-51; the tails put u2 at a* -+ twice that and a* -+ 2^-30
    (ref.vm_exact_tails, margins checked on the CPU).  A margin of 2^-45 at every kappa does not hold: c = R - kappa f carries
    kappa times the rounding of f (measured: c within 3e4 ulp of c* at kappa = 1e4, 376 ulp at 160, 2.6 ulp at 1), and at
    kappa = 1e4 3140 of 16008 decisions at a* -+ 2^-44 differed.  The decision is still the exact one for the f the sampler
    returns, since c is one fma away from that f: the second assertion holds vm_exact to 2^-45 against a = c exp(1 - c) of the
    c it is given."""
    V, c, dec, af, band = vm
    idx = np.flatnonzero((V["kappa"] == kappa) & (dec == -1))
    assert idx.size >= 1000
    cc, bt, want, marg = [], [], [], []
    for i in idx:
        a_mp, b = V["a_mp"][V["case_of"][i]], int(V["b"][i])
        if b / 2048 <= a_mp < (b + 1) / 2048:
            tails = ref.vm_exact_tails(a_mp, b, kappa)
        else:     # a* lies within the band of this interval's end, outside it: both ends and the middle, where they clear the margin
            tails = [(t, (b + mp.mpf(t)) / 2048, 1 if (b + mp.mpf(t)) / 2048 < a_mp else 0) for t in (0.0, 0.5, 1 - 2.0 ** -41)]
            tails = [x for x in tails if abs(x[1] - a_mp) > ref.vm_margin(kappa)]
        assert tails, (kappa, i)                      # no case is skipped
        for t, u2, w in tails:
            assert abs(u2 - a_mp) > ref.vm_margin(kappa)
            cc.append(c[i]); bt.append(b + t); want.append(w); marg.append(float(abs(u2 - a_mp)))
    got, _ = run("vm_exact", np.array(cc), np.array(bt))
    want, marg = np.array(want, dtype=np.float64), np.array(marg)
    bad = got != want
    # against the acceptance probability of the c the test was given
    a_dev = {}
    own_bad = own_n = 0
    for cv, x, g in zip(cc, bt, got):
        if cv not in a_dev:
            a_dev[cv] = ref.mpf(cv) * mp.exp(1 - ref.mpf(cv))
        u2 = ref.mpf(x) / 2048
        if abs(u2 - a_dev[cv]) > ref.VM_MARGIN:
            own_n += 1
            own_bad += int(g != (1.0 if u2 < a_dev[cv] else 0.0))
    print(f"[math] vm_exact kappa={kappa:g}: against a(c) of its own c, margin 2^-45: {own_bad} of {own_n} differ")
    print(f"[math] vm_exact kappa={kappa:g}: {idx.size} open cases, {want.size} tails, {int(bad.sum())} decisions differ from mpmath"
          + (f" (largest margin among them {marg[bad].max():.3g})" if bad.any() else ""))
    TABLE[f"vm_exact kappa={kappa:g}"] = {"open_cases": int(idx.size), "tails": int(want.size), "mismatches": int(bad.sum()),
                                         "largest_margin_of_a_mismatch": float(marg[bad].max()) if bad.any() else 0.0}
    assert not bad.any()
    assert own_bad == 0 and own_n >= 1000
