"""CPU: the reference of tests/test_device_math_gpu.py checks itself -- long double against mpmath on a sample of every bulk
grid, ulp_error on hand-made cases, every grid against its list of edge values and the primitive's domain, mpmath's Bessel
function against scipy, and the cases of the von Mises screen against their own conditions (which acceptance bits are open,
which tails clear the margin of the exact test)."""
import os
import re

import numpy as np
import pytest

import device_math_reference as ref

mp, LD = ref.mp, ref.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample(x, n=2000):
    x = np.asarray(x)
    return x[np.linspace(0, x.size - 1, min(n, x.size)).astype(np.int64)]


def rel_vs_mp(ld_values, mp_values):
    worst = 0.0
    for got, want in zip(ld_values, mp_values):
        if want == 0:
            assert got == 0
            continue
        worst = max(worst, float(abs((ref.mpf(LD(got)) - want) / want)))
    return worst


LD_CASES = {
    "rcp": (lambda: (ref.grid_positive(),), ref.ref_rcp, lambda x: 1 / x),
    "div": (ref.grid_div, ref.ref_div, lambda a, b: a / b),
    "sqrt": (lambda: (ref.grid_positive(),), ref.ref_sqrt, lambda x: mp.sqrt(x)),
    "acos": (lambda: (ref.grid_acos(),), ref.ref_acos, lambda x: mp.acos(x)),
    "sin": (lambda: (ref.grid_trig(1e6),), ref.ref_sin, lambda x: mp.sin(x)),
    "cos": (lambda: (ref.grid_trig(2.0 ** 30),), ref.ref_cos, lambda x: mp.cos(x)),
    "cos_half": (lambda: (ref.grid_trig(2.0 ** 30),), ref.ref_cos_half, lambda x: mp.cos(x / 2)),
    "cospi": (lambda: (ref.grid_cospi(),), ref.ref_cospi, lambda u: mp.cospi(u)),
    "log": (lambda: (ref.grid_log(),), ref.ref_log, lambda x: mp.log(x)),
    "sin_2pi": (lambda: (ref.grid_sincos(),), lambda v: ref.ref_sincos_2pi(v)[0], lambda v: mp.sinpi(2 * v)),
    "cos_2pi": (lambda: (ref.grid_sincos(),), lambda v: ref.ref_sincos_2pi(v)[1], lambda v: mp.cospi(2 * v)),
    "radius": (ref.grid_box_muller, lambda u, v: ref.ref_box_muller(u, v)[0], lambda u, v: mp.sqrt(-2 * mp.log(1 - u))),
    "envelope": (lambda: (ref.grid_kappa(),), ref.ref_envelope, lambda k: (1 + mp.sqrt(1 + 4 * k * k)) / 2),
}


@pytest.mark.parametrize("name", sorted(LD_CASES))
def test_long_double_agrees_with_mpmath(name):
    """2^-60 relative on a 2000-point sample of the grid (the whole of its edge sets lies in the sample's tail end or is
    checked by the GPU test against the same function); a zero of the function must be an exact zero of the reference"""
    if not ref.ld_ok:
        pytest.skip("long double has fewer than 63 mantissa bits here: the references are mpmath's own")
    grid, fn_ld, fn_mp = LD_CASES[name]
    args = [sample(a) for a in grid()]
    got = fn_ld(*args)
    want = [fn_mp(*[ref.mpf(x) for x in xs]) for xs in zip(*args)]
    worst = rel_vs_mp(got, want)
    print(f"{name}: long double vs mpmath, worst relative difference 2^{np.log2(max(worst, 1e-30)):.1f}")
    assert worst < 2.0 ** -60


def test_long_double_agrees_with_mpmath_on_the_edge_sets():
    if not ref.ld_ok:
        pytest.skip("long double has fewer than 63 mantissa bits here")
    for edges, fn_ld, fn_mp in ((ref.ACOS_EDGES, ref.ref_acos, mp.acos), (ref.COSPI_EDGES, ref.ref_cospi, lambda u: mp.cospi(u)),
                                (ref.log_edges(), ref.ref_log, mp.log), (ref.trig_edges(), ref.ref_sin, mp.sin),
                                (ref.trig_edges(), ref.ref_cos, mp.cos), (ref.sincos_edges(), lambda v: ref.ref_sincos_2pi(v)[0], lambda v: mp.sinpi(2 * v)),
                                (ref.sincos_edges(), lambda v: ref.ref_sincos_2pi(v)[1], lambda v: mp.cospi(2 * v))):
        assert rel_vs_mp(fn_ld(edges), [fn_mp(ref.mpf(x)) for x in edges]) < 2.0 ** -60


def test_ulp_error_on_hand_made_cases():
    one = np.array([1.0])
    assert ref.ulp_error(one, one.astype(LD))[0] == 0.0
    assert ref.ulp_error(np.nextafter(one, 2), one.astype(LD))[0] == 1.0
    assert ref.ulp_error(np.nextafter(one, 0), one.astype(LD))[0] == -0.5     # the spacing is that of |want| = 1, upwards
    assert ref.ulp_error(np.array([3.0]), np.array([2.0], dtype=LD))[0] == 2.0 ** 51
    assert ref.ulp_error(np.array([-8.0]), np.array([-8.0], dtype=LD) - LD(2.0 ** -51))[0] == 0.25        # spacing(8) = 2^-49
    # a want between two doubles: the unit is the spacing at its rounded value, the error keeps the long double part
    want = LD(1.0) + LD(2.0 ** -54)
    assert ref.ulp_error(one, np.array([want]))[0] == -0.25
    assert ref.ulp_error(np.array([0.0]), np.array([0.0], dtype=LD))[0] == 0.0
    assert ref.ulp_error(np.array([5e-324]), np.array([0.0], dtype=LD))[0] == 1.0
    third = ref.to_ld(mp.mpf(1) / 3)
    assert abs(ref.ulp_error(np.array([1.0 / 3.0]), np.array([third]))[0] - float((mp.mpf(1.0 / 3.0) - mp.mpf(1) / 3) / mp.mpf(2.0 ** -54))) < 1e-3


def has(grid, values):
    g = np.asarray(grid, dtype=np.float64).view(np.uint64)
    return all(np.any(g == np.array([v], dtype=np.float64).view(np.uint64)[0]) for v in np.ravel(values))


def test_grids_hold_their_edge_values_and_stay_in_the_domain():
    pos = ref.grid_positive()
    assert pos.size >= ref.N_BULK and (pos > 1e-101).all() and (pos < 1e101).all() and np.isfinite(pos).all()
    assert has(pos, [1 + 4 * k * k for k in ref.KAPPAS]) and has(pos, ref.neighbours(np.array([1.0, 2.0 ** -300, 2.0 ** 295])))
    z = ref.chebyshev(257)
    assert z[0] == 1.0 and z[-1] == -1.0 and z.size == 257
    a, b = ref.grid_div()
    assert a.size == b.size and (b > 1e-101).all() and np.isfinite(a).all() and (np.abs(a[a != 0]) > 1e-101).all() and (np.abs(a) < 1e101).all()
    for k in ref.KAPPAS:
        R = ref.envelope(k)
        i = np.flatnonzero((a == k + R) & (b == R + k))
        assert i.size and has(a, k + R * z) and has(b, R + k * z)
    x = ref.grid_acos()
    assert (np.abs(x) <= 1.0).all() and has(x, [1.0, -1.0, 0.0, -0.0, 0.5, -0.5]) and has(x, ref.neighbours(np.array([0.5, -0.5])))
    assert has(x, [np.nextafter(1.0, 0), np.nextafter(-1.0, 0)]) and has(x, [1 - 2.0 ** -k for k in range(1, 54)]) and has(x, [-1 + 2.0 ** -k for k in range(1, 54)])
    assert np.signbit(x[(x == 0)]).any() and not np.signbit(x[x == 0]).all()
    u = ref.grid_cospi()
    assert ((u >= 0) & (u <= 1)).all() and (u * 2.0 ** 52 == np.rint(u * 2.0 ** 52)).sum() >= ref.N_BULK
    assert has(u, [0.0, 0.5, 1.0, 2.0 ** -52]) and has(u, ref.neighbours(np.array([0.5])))
    for limit in (1e6, 2.0 ** 30):
        d = ref.grid_trig(limit)
        assert (np.abs(d) <= limit).all() and (np.abs(d) <= 4 * np.pi).sum() >= ref.N_BULK // 2 and (np.abs(d) > 1e5).any()
        assert has(d, [float(n * mp.pi) for n in (1, 2, 3, 1000, 318309)]) and has(d, [float((n + mp.mpf(0.5)) * mp.pi) for n in (1, 2, 3, 1000, 318309)])
    assert np.abs(ref.grid_trig(2.0 ** 30)).max() == 2.0 ** 30 and (np.abs(ref.grid_trig(2.0 ** 30)) > 1e8).any()
    x = ref.grid_log()
    assert ((x > 0) & (x <= 1)).all() and x.min() == 2.0 ** -53 and has(x, [2.0 ** -53, 1.0, 0.5]) and has(x, 2.0 ** -np.arange(1.0, 54.0))
    r = ref.both_roundings(mp.sqrt(mp.mpf(0.5)))
    assert mp.mpf(r[0]) < mp.sqrt(mp.mpf(0.5)) < mp.mpf(r[1]) and r[1] == np.nextafter(r[0], 1) and has(x, ref.neighbours(r))
    assert ((x < 1) & (x > 1 - 2.0 ** -20)).any()     # 1 - m 2^-53 with small m: where log -> 0
    v = ref.grid_sincos()
    assert ((v >= 0) & (v < 1)).all() and has(v, np.arange(8) / 8.0) and has(v, [1 - 2.0 ** -53, np.nextafter(0.5, 0), np.nextafter(0.5, 1)])
    bu, bv = ref.grid_box_muller()
    assert ((bu >= 0) & (bu < 1) & (bv >= 0) & (bv < 1)).all() and (bu * 2.0 ** 53 == np.rint(bu * 2.0 ** 53)).all()
    assert (bv == 0).sum() >= 1 << 14 and has(bu, [0.0, 1 - 2.0 ** -53])
    m = ref.grid_mod()
    assert (np.abs(m) <= 1e6).all() and has(m, [1e6, -1e6]) and (np.abs(m) <= 40).sum() >= 1 << 16
    for k in range(-6, 7):
        lo, hi = ref.both_roundings((2 * k + 1) * mp.pi)
        assert mp.mpf(lo) < (2 * k + 1) * mp.pi < mp.mpf(hi) and has(m, [np.nextafter(lo, -np.inf), lo, hi, np.nextafter(hi, np.inf)])
    w = ref.grid_words()
    assert w.size == 49 + 4096 and w.dtype == np.uint64
    for lo in ref.U01_WORDS:
        for hi in ref.U01_WORDS:
            assert ((hi << 32) | lo) in w[:49]
    for kind, top in (("scaled", 1e6), ("two_pi", 1e6), ("unscaled", ref.I0_OVERFLOW)):
        zb = ref.grid_bessel(kind)
        assert (zb >= 0).all() and zb.max() <= top and has(zb, [0.0, 1e-300, 1e-8]) and has(zb, ref.neighbours(np.array([30.0])))
        assert ((zb > 0) & (zb < 30)).sum() >= 600 and (zb > 30).sum() >= 600
    assert has(ref.grid_bessel("two_pi"), ref.neighbours(np.array([100.0])))
    assert mp.isfinite(mp.besseli(0, mp.mpf(ref.I0_OVERFLOW))) and mp.besseli(0, mp.mpf(ref.I0_OVERFLOW)) < mp.mpf(np.finfo(np.float64).max)
    s, u = ref.grid_compact_exp()
    assert s.size == len(ref.CEI_S) * 260 and set(s) == set(ref.CEI_S) and ((u >= 0) & (u < 1)).all()
    for sv in ref.CEI_S:
        assert has(u[s == sv], [0.0, 2.0 ** -53, 1 - 2.0 ** -53])
    kap = ref.grid_kappa()
    assert has(kap, ref.KAPPAS) and (kap >= 1e-12).all() and (kap <= 1e4).all()


def test_mpmath_bessel_agrees_with_scipy():
    from scipy import special
    z = np.concatenate([ref.grid_bessel("scaled"), ref.grid_bessel("two_pi")])
    want = special.i0e(z)
    got = np.array([float(ref.mp_i0_scaled(ref.mpf(x))) for x in z])
    assert np.max(np.abs(got / want - 1)) < 1e-14
    zu = ref.grid_bessel("unscaled")
    assert np.max(np.abs(np.array([float(mp.besseli(0, ref.mpf(x))) for x in zu]) / special.i0(zu) - 1)) < 1e-14
    # the reference code's own expansion beyond 100 is close to, and is not, the Bessel function
    for x in (100.5, 1e3, 1e6):
        three = ref.mp_two_pi_i0_scaled(mp.mpf(x))
        true = 2 * mp.pi * ref.mp_i0_scaled(mp.mpf(x))
        assert 0 < abs(three / true - 1) < 0.08 / x ** 3


def test_compact_exp_inverse_reference_inverts_the_cdf():
    for s in (1e-8, 0.5, 4.0, 40.0):
        for u in (2.0 ** -53, 0.25, 0.5, 1 - 2.0 ** -53):
            x = ref.mp_compact_exp_inverse(mp.mpf(s), mp.mpf(u))
            cdf = mp.expm1(s * (x + 1)) / mp.expm1(2 * s)       # int_{-1}^{x} e^{s t} dt / int_{-1}^{1}
            assert abs(cdf - u) < mp.mpf(10) ** -40 and -1 <= x <= 1
    assert ref.mp_compact_exp_inverse(mp.mpf(0), mp.mpf(0.25)) == -0.5 and ref.mp_compact_exp_inverse(mp.mpf(4), mp.mpf(0)) == -1


def test_von_mises_cases():
    """4097 proposals with both ends, every kappa, four acceptance words each; b0's interval holds a*; the closed form of c*
    equals R - kappa f; every open case has a tail on the grid of 2^-41 that clears the margin, on either side of a* for
    nearly all of them"""
    m52 = ref.vm_u1()
    assert len(m52) == 4097 and m52[0] == 0 and m52[-1] == (1 << 52) - 1 and all(b > a for a, b in zip(m52, m52[1:]))
    V = ref.vm_cases()
    n = len(ref.KAPPAS) * 4097
    assert V["words"].size == 4 * n and len(V["a_mp"]) == n and sorted(set(V["kappa"])) == sorted(ref.KAPPAS)
    assert (((V["words"] >> np.uint64(1)) & np.uint64(0x7FF)).astype(np.int64) == V["b"]).all() and ((V["b"] >= 0) & (V["b"] < 2048)).all()
    assert ((V["words"] & np.uint64(1)) == 1).any() and ((V["words"] & np.uint64(1)) == 0).any()
    open_ = V["kind"] == 0
    a, b = V["a"][open_], V["b"][open_].astype(LD)
    assert ((b / 2048 <= a) & ((a < (b + 1) / 2048) | (b == 2047))).all() and (a > 0).sum() >= n - 2 * 4097 and (a <= 1).all()
    far = V["kind"] >= 2
    assert (np.abs(V["b"][far].astype(LD) / 2048 - V["a"][far]) > 0.2).all()
    for kappa, m in ((0.5, m52[100]), (16.0, m52[3000]), (1e4, m52[4000])):
        k = mp.mpf(kappa)
        R = (1 + mp.sqrt(1 + 4 * k * k)) / 2
        z = mp.cos(mp.pi * mp.mpf(m) / 2 ** 52)
        c, _ = ref.mp_vm_c_a(kappa, m)
        assert abs(c - (R - k * (k + R * z) / (R + k * z))) < mp.mpf(10) ** -40 * R
    both = 0
    idx = np.flatnonzero(open_)[:: 37]
    for i in idx:
        tails = ref.vm_exact_tails(V["a_mp"][V["case_of"][i]], int(V["b"][i]), float(V["kappa"][i]))
        assert tails, i
        for t, u2, want in tails:
            assert 0 <= t < 1 and t * 2.0 ** 41 == np.rint(t * 2.0 ** 41) and abs(u2 - V["a_mp"][V["case_of"][i]]) > ref.vm_margin(float(V["kappa"][i])) >= ref.VM_MARGIN
            assert float(int(V["b"][i]) + t) - int(V["b"][i]) == t       # b + tail is exact in a double
        both += len({w for _, _, w in tails}) == 2
    assert both >= 0.75 * idx.size          # (a* < 2^-44 at the large concentrations has no tail below it)


def test_math_fn_numbers_are_the_header_s():
    from mlmcpathintegral_amd import abi
    text = open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read()
    found = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"MLMCPI_MATH_([A-Z0-9_]+) = (\d+)", text)}
    count = found.pop("count")
    assert found == abi.MATH_FN and count == len(abi.MATH_FN) and sorted(found.values()) == list(range(count))


def test_test_math_refuses_bad_arguments_before_any_launch():
    """unknown fn, n == 0 and null pointers are MLMCPI_ERR_INVALID on the host side: no GPU is needed to be told so"""
    import ctypes as C
    from mlmcpathintegral_amd import abi
    buf = (C.c_double * 4)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    for args in ((len(abi.MATH_FN), p, p, 4, p, p), (0, p, p, 0, p, p), (0, null, p, 4, p, p), (0, p, p, 4, null, p), (0, p, p, 4, p, null),
                 (abi.MATH_FN["fast_div"], p, null, 4, p, p), (abi.MATH_FN["vm_exact"], p, null, 4, p, p)):
        with pytest.raises(abi.MlmcpiError, match="status -1"):
            abi.call("mlmcpi_test_math", *args, null)
