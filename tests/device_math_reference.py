"""CPU reference of the fp64 device primitives (device_common.hpp, vonmises.hpp, fillin.hpp, sigma_device.hpp): the input
grids of tests/test_device_math_gpu.py and the values the primitives should return there, from the formulas alone.

Bulk grids are evaluated in numpy long double (63-bit mantissa; `ld_ok` says whether that holds on this machine, and every
reference falls back to mpmath where it does not); the edge sets, the Bessel functions, the expm1 / log1p chain of
compact_exp_inverse and c exp(1 - c) of the von Mises screen come from mpmath at 50 digits.  Nothing here restates a device
polynomial or a device reduction constant: the references are the mathematical functions (the one exception, by intent, is
two_pi_i0_scaled above z = 100, whose three-term expansion IS the function the reference code defines).

Every grid is generated from a fixed seed; tests/test_device_math_reference.py checks the grids (edge values present, domain
respected) and the references (long double against mpmath, mpmath's Bessel against scipy) on the CPU.
"""
import functools

import mpmath
import numpy as np

LD = np.longdouble
ld_ok = np.finfo(LD).nmant >= 63
mp = mpmath.mp.clone() if hasattr(mpmath.mp, "clone") else mpmath.mp
mp.dps = 50
SEED = 20261019
KAPPAS = (1e-12, 1e-8, 1e-3, 0.1, 0.5, 1.0, 4.0, 8.0, 16.0, 40.0, 160.0, 1e4)
N_BULK = 1 << 17
PI_LD = LD(0)  # set below


def mpf(x):
    """exact mpf of a double (or of a long double, through its two double halves)"""
    if isinstance(x, LD):
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))
    return mp.mpf(float(x))


def to_ld(v):
    """an mpf rounded to long double (two doubles: 106 bits, more than the 64 kept)"""
    v = mp.mpf(v)
    if not mp.isfinite(v):
        return LD(float(v))
    hi = float(v)
    return LD(hi) + LD(float(v - mp.mpf(hi)))


def ld_array(values):
    return np.array([to_ld(v) for v in values], dtype=LD)


PI_LD = to_ld(mp.pi)


def via_mp(fn, *arrays):
    """fn evaluated in mpmath at every entry (exact inputs), as a long double array"""
    return ld_array([fn(*[mpf(x) for x in xs]) for xs in zip(*[np.ravel(a) for a in arrays])])


def ulp_error(got, want):
    """(got - want) in units of np.spacing(|want| rounded to double), elementwise; `want` long double (or anything numpy
    converts to it)"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD)
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    return ((got.astype(LD) - want) / ulp.astype(LD)).astype(np.float64)


def neighbours(x):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def both_roundings(v):
    """the doubles just below and just above the mpf v (v itself twice if it is a double)"""
    v = mp.mpf(v)
    d = float(v)
    if mp.mpf(d) == v:
        return np.array([d, d])
    return np.array([np.nextafter(d, -np.inf), d]) if mp.mpf(d) > v else np.array([d, np.nextafter(d, np.inf)])


def _rng(tag):
    return np.random.default_rng([SEED, sum(ord(c) * (k + 1) for k, c in enumerate(tag))])


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def envelope(kappa):
    """R = (1 + sqrt(1 + 4 kappa^2)) / 2 as a double (what the sampler forms; here only to build operands)"""
    k = LD(kappa)
    return float((1 + np.sqrt(1 + 4 * k * k)) / 2)


def chebyshev(n):
    return np.cos(np.pi * np.arange(n) / (n - 1))


# ---- grids ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def grid_positive():
    """fast_rcp, fast_sqrt (and the denominators of fast_div): log-uniform, the sampler's own operands, powers of two"""
    rng = _rng("positive")
    bulk = _loguniform(rng, 1e-100, 1e100, N_BULK)
    sampler = [np.array([1 + 4 * k * k for k in KAPPAS])]
    z = chebyshev(257)
    for k in KAPPAS:
        R = envelope(k)
        sampler += [k + R * z, R + k * z]
    sampler = np.concatenate(sampler)
    sampler = sampler[sampler > 0]   # (kappa + R z changes sign: the numerators of fast_div keep it, see grid_div)
    pow2 = neighbours(2.0 ** np.arange(-300, 301, 7, dtype=np.float64))
    return np.concatenate([bulk, sampler, pow2, neighbours(np.array([1.0, 2.0, 4.0, 0.5, 0.25]))])


@functools.lru_cache(None)
def grid_div():
    """fast_div(a, b): log-uniform pairs with either sign of a, the sampler's pairs (kappa + R z, R + kappa z), powers of two"""
    rng = _rng("div")
    a = _loguniform(rng, 1e-100, 1e100, N_BULK) * rng.choice([-1.0, 1.0], N_BULK)
    b = _loguniform(rng, 1e-100, 1e100, N_BULK)
    z = chebyshev(257)
    sa, sb = [], []
    for k in KAPPAS:
        R = envelope(k)
        sa.append(k + R * z)
        sb.append(R + k * z)
    p = neighbours(2.0 ** np.arange(-300, 301, 7, dtype=np.float64))
    a = np.concatenate([a] + sa + [p, np.ones_like(p), p])
    b = np.concatenate([b] + sb + [np.full_like(p, 3.0), p, p[::-1].copy()])
    return a, b


ACOS_EDGES = np.concatenate([neighbours(np.array([0.5, -0.5])), np.array([1.0, np.nextafter(1.0, 0), -1.0, np.nextafter(-1.0, 0)]),
                             np.array([0.0, -0.0, 5e-324, -5e-324]), 1.0 - 2.0 ** -np.arange(1.0, 54.0), -1.0 + 2.0 ** -np.arange(1.0, 54.0)])


@functools.lru_cache(None)
def grid_acos():
    return np.concatenate([_rng("acos").uniform(-1.0, 1.0, N_BULK), ACOS_EDGES])


COSPI_EDGES = np.concatenate([np.array([0.0, 0.5, 1.0, 2.0 ** -52]), neighbours(np.array([0.5]))])


@functools.lru_cache(None)
def grid_cospi():
    m = _rng("cospi").integers(0, 1 << 52, N_BULK, dtype=np.int64)
    return np.concatenate([m.astype(np.float64) * 2.0 ** -52, COSPI_EDGES])


def trig_edges():
    out = []
    for n in (1, 2, 3, 1000, 318309):
        out += [float(n * mp.pi), float((n + mp.mpf(0.5)) * mp.pi)]
    e = np.array(out)
    return np.concatenate([e, -e])


@functools.lru_cache(None)
def grid_trig(limit):
    """sin_reduced (limit 1e6), cos_reduced and cos_half (limit 2^30): uniform in +-4 pi, log-uniform up to the limit with
    either sign, the doubles nearest n pi and (n + 1/2) pi"""
    rng = _rng("trig%g" % limit)
    n = N_BULK // 2
    return np.concatenate([rng.uniform(-4 * np.pi, 4 * np.pi, n), _loguniform(rng, 1e-6, limit, n) * rng.choice([-1.0, 1.0], n),
                           trig_edges(), np.array([0.0, limit, -limit])])


def log_edges():
    s = mp.sqrt(mp.mpf(0.5))
    r = both_roundings(s)
    return np.concatenate([np.array([2.0 ** -53, 1.0, 0.5, np.nextafter(1.0, 0)]), 2.0 ** -np.arange(1.0, 54.0), neighbours(r)])


@functools.lru_cache(None)
def grid_log():
    rng = _rng("log")
    n = N_BULK // 2
    m = rng.integers(0, 1 << 53, n, dtype=np.int64)
    near_one = 1.0 - m.astype(np.float64) * 2.0 ** -53        # exact: multiples of 2^-53 in (0, 1]
    near_one = near_one[near_one > 0]
    return np.concatenate([near_one, _loguniform(rng, 2.0 ** -53, 1.0, n), log_edges()])


def sincos_edges():
    # (above 0 the neighbour is 2^-53, the smallest non-zero value u01 produces, not the smallest denormal)
    return np.concatenate([np.array([0.0, 2.0 ** -53]), neighbours(np.arange(1, 8) / 8.0), np.array([1.0 - 2.0 ** -53])])


@functools.lru_cache(None)
def grid_sincos():
    m = _rng("sincos").integers(0, 1 << 53, N_BULK, dtype=np.int64)
    return np.concatenate([m.astype(np.float64) * 2.0 ** -53, sincos_edges()])


@functools.lru_cache(None)
def grid_box_muller():
    """(u, v) in [0, 1)^2, both multiples of 2^-53 (what u01 produces): random pairs, the ends of u against the octants of v,
    and v = 0 throughout a sample of u (there cs = 1 exactly, so n0 IS the radius)"""
    rng = _rng("box")
    n = 1 << 14
    u = rng.integers(0, 1 << 53, n, dtype=np.int64).astype(np.float64) * 2.0 ** -53
    v = rng.integers(0, 1 << 53, n, dtype=np.int64).astype(np.float64) * 2.0 ** -53
    ue = np.array([0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -30, 2.0 ** -30])
    ve = sincos_edges()
    uu, vv = np.meshgrid(ue, ve, indexing="ij")
    return np.concatenate([u, uu.ravel(), u, ue]), np.concatenate([v, vv.ravel(), np.zeros(n), np.zeros(ue.size)])


def mod_edges():
    out = []
    for k in range(-6, 7):
        r = both_roundings((2 * k + 1) * mp.pi)
        out.append(np.array([np.nextafter(r[0], -np.inf), r[0], r[1], np.nextafter(r[1], np.inf)]))
    return np.concatenate(out + [np.array([1e6, -1e6, 0.0])])


@functools.lru_cache(None)
def grid_mod():
    return np.concatenate([_rng("mod").uniform(-40.0, 40.0, 1 << 16), mod_edges()])


U01_WORDS = (0, 0xFFFFFFFF, 1, 0x800, 0xFFF, 0x1000, 0x80000000)


@functools.lru_cache(None)
def grid_words():
    """(lo, hi) as uint64 hi << 32 | lo: every pairing of U01_WORDS, then 4096 random pairs"""
    pairs = [(lo, hi) for lo in U01_WORDS for hi in U01_WORDS]
    r = _rng("words").integers(0, 1 << 32, (4096, 2), dtype=np.uint64)
    v = np.array([(hi << 32) | lo for lo, hi in pairs], dtype=np.uint64)
    return np.concatenate([v, (r[:, 1] << np.uint64(32)) | r[:, 0]])


def as_double(words):
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.float64)


@functools.lru_cache(None)
def grid_kappa():
    """vm_envelope: the kappa list and log-uniform concentrations between its ends"""
    return np.concatenate([np.array(KAPPAS), _loguniform(_rng("kappa"), 1e-12, 1e4, 4096)])


I0_OVERFLOW = 713.0   # exp(z) I0e(z) is finite up to z = 713.98...; stop one unit short


@functools.lru_cache(None)
def grid_bessel(kind):
    """kind: 'scaled', 'two_pi' (the same plus 100 with neighbours) or 'unscaled' (stops where I0 overflows)"""
    rng = _rng("bessel")
    top = I0_OVERFLOW if kind == "unscaled" else 1e6
    pts = [np.array([0.0, 1e-300, 1e-8]), np.sort(rng.uniform(0.0, 30.0, 600)), neighbours(np.array([30.0])),
           np.sort(_loguniform(rng, 30.0, top, 600))]
    if kind == "two_pi":
        pts.append(neighbours(np.array([100.0])))
    return np.concatenate(pts)


CEI_S = (0.0, 1e-300, 1e-16, 1e-8, 1e-3, 0.5, 4.0, 40.0, 400.0, 1e4)


@functools.lru_cache(None)
def grid_compact_exp():
    u = np.concatenate([np.array([0.0, 2.0 ** -53]), _rng("cei").integers(0, 1 << 53, 257, dtype=np.int64).astype(np.float64) * 2.0 ** -53,
                        np.array([1.0 - 2.0 ** -53])])
    ss, uu = np.meshgrid(np.array(CEI_S), u, indexing="ij")
    return ss.ravel().copy(), uu.ravel().copy()


# ---- references ---------------------------------------------------------------------------------------------------------------
def _ld(fn_ld, fn_mp, *arrays):
    if ld_ok:
        return fn_ld(*[np.asarray(a, dtype=np.float64).astype(LD) for a in arrays])
    return via_mp(fn_mp, *arrays)


def ref_rcp(x):
    return _ld(lambda x: 1 / x, lambda x: 1 / x, x)


def ref_div(a, b):
    return _ld(lambda a, b: a / b, lambda a, b: a / b, a, b)


def ref_sqrt(x):
    return _ld(np.sqrt, mp.sqrt, x)


def ref_acos(x):
    return _ld(np.arccos, mp.acos, x)


def ref_sin(x):
    return _ld(np.sin, mp.sin, x)


def ref_cos(x):
    return _ld(np.cos, mp.cos, x)


def ref_cos_half(x):
    return _ld(lambda x: np.cos(x / 2), lambda x: mp.cos(x / 2), x)


def ref_cospi(u):
    """cos(pi u) = sin(pi (1/2 - u)): 1/2 - u is exact for u in [0, 1], so the zero at u = 1/2 keeps its relative accuracy"""
    return _ld(lambda u: np.sin(PI_LD * (LD(0.5) - u)), lambda u: mp.cospi(u), u)


def ref_log(x):
    return _ld(np.log, mp.log, x)


def _sincos_2pi_ld(v):
    # exact reduction to a quarter turn (4 v - q is exact in double), then the rotation: keeps relative accuracy at the zeros
    a = 4 * v
    q = np.rint(a)
    x = (PI_LD / 2) * (a - q)
    s0, c0 = np.sin(x), np.cos(x)
    k = q.astype(np.int64) & 3
    cr = np.where(k & 1, -s0, c0)
    sr = np.where(k & 1, c0, s0)
    return np.where(k & 2, -sr, sr), np.where(k & 2, -cr, cr)


def ref_sincos_2pi(v):
    """(sin, cos)(2 pi v)"""
    if ld_ok:
        return _sincos_2pi_ld(np.asarray(v, dtype=np.float64).astype(LD))
    return via_mp(lambda v: mp.sinpi(2 * v), v), via_mp(lambda v: mp.cospi(2 * v), v)


def mp_sincos_2pi(v):
    v = mpf(v)
    return mp.sinpi(2 * v), mp.cospi(2 * v)


def ref_box_muller(u, v):
    """(radius, n0, n1): r = sqrt(-2 log(1 - u)) (1 - u is exact for u a multiple of 2^-53), n0 = r cos(2 pi v), n1 = r sin(2 pi v)"""
    r = _ld(lambda u: np.sqrt(-2 * np.log(1 - u)), lambda u: mp.sqrt(-2 * mp.log(1 - u)), u)
    sn, cs = ref_sincos_2pi(v)
    return r, r * cs, r * sn


def ref_envelope(kappa):
    return _ld(lambda k: (1 + np.sqrt(1 + 4 * k * k)) / 2, lambda k: (1 + mp.sqrt(1 + 4 * k * k)) / 2, kappa)


def mp_i0_scaled(z):
    return mp.besseli(0, z) * mp.exp(-z)


def ref_bessel_i0_scaled(z):
    return via_mp(mp_i0_scaled, z)


def ref_bessel_i0(z):
    return via_mp(lambda z: mp.besseli(0, z), z)


def mp_two_pi_i0_scaled(z):
    """ExpSin2Distribution::fast_2pi_I0_scaled as the reference code defines it: the three-term expansion beyond z = 100"""
    if z > 100:
        return mp.sqrt(2 * mp.pi / z) * (1 + mp.mpf(0.125) / z + mp.mpf(0.0703125) / (z * z))
    return 2 * mp.pi * mp_i0_scaled(z)


def ref_two_pi_i0_scaled(z):
    return via_mp(mp_two_pi_i0_scaled, z)


def mp_compact_exp_inverse(s, u):
    """the inverse CDF of p(x) ~ exp(s x) on [-1, 1] at u"""
    if s == 0:
        return 2 * u - 1
    if u == 0:
        return mp.mpf(-1)
    return 1 + mp.log1p((1 - u) * mp.expm1(-2 * s)) / s


def ref_compact_exp_inverse(s, u):
    return via_mp(mp_compact_exp_inverse, s, u)


def ref_u01(words):
    return (np.asarray(words, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def ref_u01_52(words):
    return (np.asarray(words, dtype=np.uint64) >> np.uint64(12)).astype(np.float64) * 2.0 ** -52


# ---- the von Mises attempt ----------------------------------------------------------------------------------------------------
VM_POINTS = 4097


def vm_u1():
    """4097 proposals (v >> 12) spread evenly over [0, 2^52): both ends included"""
    return [(j * ((1 << 52) - 1)) // (VM_POINTS - 1) for j in range(VM_POINTS)]


def mp_vm_c_a(kappa, m52):
    """c* and a* = c* exp(1 - c*) of the attempt with proposal u1 = m52 2^-52 at concentration kappa.  c = R - kappa f with
    f = (kappa + R z) / (R + kappa z) is R / (R + kappa z) (R^2 - R = kappa^2): evaluated in that form, free of cancellation."""
    k = mp.mpf(kappa)
    R = (1 + mp.sqrt(1 + 4 * k * k)) / 2
    z = mp.cospi(mp.mpf(m52) / mp.mpf(1 << 52))
    c = R / (R + k * z)
    return c, c * mp.exp(1 - c)


@functools.lru_cache(None)
def vm_cases():
    """Every case of the von Mises screen: for each kappa and each proposal the acceptance bits b0 = floor(2048 a*) (the
    interval [b0, b0 + 1) / 2048 holds a*: the screen cannot decide), the neighbour of b0 on the side a* is nearer to, and two
    far ones (b0 + 512 and b0 + 1024 modulo 2048).  Returns a dict of arrays over the cases: kappa, words (uint64), b, kind
    (0: b0, 1: neighbour, 2, 3: far), c (long double c*), a (long double a*), and a_mp (the mpf a* per (kappa, proposal))."""
    m52 = vm_u1()
    kap, words, bs, kind, cs, as_, a_mp = [], [], [], [], [], [], []
    sign = 0
    for kappa in KAPPAS:
        for m in m52:
            c, a = mp_vm_c_a(kappa, m)
            a_mp.append(a)
            x = 2048 * a
            b0 = min(int(mp.floor(x)), 2047)
            near = b0 + 1 if (x - b0 >= 0.5 and b0 < 2047) else (b0 - 1 if b0 > 0 else b0 + 1)
            for j, b in enumerate((b0, near, (b0 + 512) % 2048, (b0 + 1024) % 2048)):
                sign ^= 1   # bit 0 (the sign of the angle) takes no part in the decision: alternate it
                kap.append(kappa)
                words.append((m << 12) | (b << 1) | sign)
                bs.append(b)
                kind.append(j)
                cs.append(c)
                as_.append(a)
    return {"kappa": np.array(kap), "words": np.array(words, dtype=np.uint64), "b": np.array(bs, dtype=np.int64), "kind": np.array(kind),
            "c": ld_array(cs), "a": ld_array(as_), "a_mp": a_mp, "case_of": np.repeat(np.arange(len(a_mp)), 4)}


VM_MARGIN = 2.0 ** -45


def vm_margin(kappa):
    """How far u2 must be from a* = a(kappa, u1) for the exact test on the DEVICE's c to have to agree with it: 2^-45, plus
    what the fp64 c may differ from c* by.  c = R - kappa f inherits kappa times the error of f: 1.5 ulp of the division
    (|f| <= 1) and the 2^-51 of cospi_unit through df/dz = c^2 / R, so |c - c*| <= kappa (1.5 2^-52 + 2^-51 c^2 / R), and
    a = c exp(1 - c) moves by |1 - c| exp(1 - c) times that: with kappa <= R, max |1 - c| exp(1 - c) = 0.37 beyond c = 1 and
    max |1 - c| c^2 exp(1 - c) = 1.6, at most (0.56 kappa + 3.2) 2^-52 < 2^-47 + kappa 2^-52.  (The decision is exact for the
    c the test is given, which is the c of the f the sampler returns; see the GPU test.)  Doubled for safety of the count."""
    return VM_MARGIN + kappa * 2.0 ** -51


def vm_exact_tails(a_mp, b, kappa):
    """For an open case (acceptance bits b, a* in [b, b + 1) / 2048) the tails of the exact test: u2 = (b + tail) / 2048 at
    a* -+ 2 vm_margin(kappa) and a* -+ 2^-30, tail rounded to a multiple of 2^-41 and kept inside [0, 1).  Returns [(tail, u2
    as mpf, decision u2 < a*)] for the offsets whose u2 clears vm_margin(kappa) on its side of a* (at least one always does)."""
    out = []
    m = vm_margin(kappa)
    for off in (-2 * m, 2 * m, -2.0 ** -30, 2.0 ** -30):
        t = (a_mp + mp.mpf(off)) * 2048 - b
        t = mp.floor(t * 2 ** 41 + mp.mpf(0.5)) / 2 ** 41
        if not (0 <= t < 1):
            continue
        u2 = (b + t) / 2048
        if abs(u2 - a_mp) > m:
            out.append((float(t), u2, 1 if u2 < a_mp else 0))
    return out
