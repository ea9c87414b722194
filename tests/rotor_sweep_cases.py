"""Shapes, concentrations, inputs and oracle runs of tests/test_rotor_sweeps_gpu.py, with the launch arithmetic of
path_sweep_impl (rotor_sweeps.hip) they are chosen by.  Everything here is decided without a device;
tests/test_rotor_sweep_cases.py asserts that every named case reaches the geometry and the sampler its comment claims, and
the conditions on the inputs (step-envelope classes, concentrations at both ends of the range).
"""
import functools

import numpy as np

SEED = 0x1234567812345678
B, CHAIN0, SWEEP0 = 3, 11, 70

# ---- the constants of rotor_sweeps.hip / step_envelope.hpp -----------------------------------------------------------------
LDS_IMAGE = 2048          # doubles of a segment with its halos
CAP_CLOSED, CAP_BLOCK = 16, 8   # overrelaxation sweeps per launch: closed form / sweep by sweep (MLMCPI_OR_KERNEL=block)
POOL_CAP = 256            # entries of the heat-bath retry pool
VS_KAPPA_MAX = 16.0       # 2 m0 / a up to here: step envelope; beyond: wrapped Cauchy
VS_CLASSES = 8
GRID_Y_MAX = 65535


# ---- concentrations ---------------------------------------------------------------------------------------------------------
# name -> (m0, 1 / a); T_final = M / (1 / a) is exact for a power of two, and so is a = T_final / M, on the device
# (path_common.hpp make_params) as in the oracle: both then form 2.0 * m0 / a from the same doubles
SCALES = {
    "flat": (0.25, 1),            # 0.5     step envelope, nearly flat conditionals
    "mid": (0.25, 8),             # 4       step envelope (the scale of tests/test_gpu_parity.py)
    "top": (0.25, 32),            # 16      step envelope, the last value of its range
    "over": (0.2500001, 32),      # 16.0000064  wrapped Cauchy, the first values of its range
    "peaked": (0.25, 128),        # 64      wrapped Cauchy
    "sharp": (0.25, None),        # 400     wrapped Cauchy: _rotor(M, 400.0) of tests/test_cluster_gpu.py
}
SAMPLER = {"flat": "step", "mid": "step", "top": "step", "over": "cauchy", "peaked": "cauchy", "sharp": "cauchy"}


def params(scale, M):
    """M, T_final, m0 of the rotor at the named concentration"""
    m0, inv_a = SCALES[scale]
    if inv_a is None:
        return dict(M=M, T_final=M * 2.0 * m0 / 400.0, m0=m0)
    return dict(M=M, T_final=M / float(inv_a), m0=m0)


def sig_scale(p):
    """2 m0 / a as the device and the oracle compute it"""
    a = p["T_final"] / p["M"]
    return 2.0 * p["m0"] / a


# ---- the launch arithmetic of path_sweep_impl, mirrored ------------------------------------------------------------------------
def launches(M, n_or, n_hb, with_qoi=False, block_mode=False, split_heat=False, scale=4.0):
    """the launches of one draw: dicts of n (sweeps), n_closed, kinds (bit s: sweep s is a heat bath), halo, owned, nseg2,
    olen and L per segment, cells per colour phase and segment, sampler ("step" / "cauchy" / None without heat bath), qoi"""
    assert M % 2 == 0
    closed, total, out, s = not block_mode, n_or + n_hb, [], 0
    while s < total:
        n, kinds, n_closed = 1, 0, 0
        if s < n_or:
            cap = CAP_CLOSED if closed else CAP_BLOCK
            n = min(n_or - s, cap)
            if closed:
                n_closed = n
            if not split_heat and s + n == n_or and n_hb >= 1 and (n < cap or closed):
                kinds = 1 << n
                n += 1
        else:
            kinds = 1
        qoi = with_qoi and s + n == total
        halo = 2 * n + (2 if qoi else 0)
        owned = min(LDS_IMAGE - 2 * halo, M)
        nseg = -(-M // owned)
        owned = -(-M // nseg)
        rounded = owned & 1
        owned += rounded
        nseg2 = -(-M // owned)
        olen = [min(owned, M - seg * owned) for seg in range(nseg2)]
        L = [o + 2 * halo for o in olen]
        out.append(dict(n=n, n_closed=n_closed, kinds=kinds, halo=halo, owned=owned, rounded=bool(rounded), nseg2=nseg2, olen=olen, L=L,
                        cells=[((l - 2) // 2, (l - 1) // 2) for l in L], qoi=qoi,
                        sampler=None if not kinds else ("step" if scale <= VS_KAPPA_MAX else "cauchy")))
        s += n
    return out


def lands_in_callers_buffer(plan):
    """mlmcpi_path_sweep_draw alternates between the scratch buffer and the caller's: an even number of launches ends in
    the caller's (no copy behind the last launch)"""
    return len(plan) % 2 == 0


# ---- shapes -------------------------------------------------------------------------------------------------------------------
# (M, n_or, n_hb, with QoI) -> what of path_sweep_impl it reaches; tests/test_rotor_sweep_cases.py asserts each comment
SMALL = [(M, n_or, n_hb, qoi) for M in (2, 4, 6) for n_or, n_hb in ((16, 1), (3, 2), (0, 1)) for qoi in (False, True)]
# the halo (34 or 36, 8, 2 or 4 sites) wraps the ring up to 18 times; at M = 6 halo % M is 4, 0 and 2; at M = 2 both
# neighbours of a site are one site
EDGES = [
    (1980, 16, 1, False),   # one segment, L = 2048 exactly: H2 = 1024 = 4 x 256 pairs in the closed form
    (1976, 16, 1, True),    # the same with the QoI launch's extra halo pair
    (1982, 16, 1, False),   # the first M with two segments: owned 991 -> 992, segments of 992 and 990
    (1978, 16, 1, True),    # the same with QoI: owned 989 -> 990, segments of 990 and 988
    (2044, 0, 1, False),    # heat-bath-only launch on the full image: 1023 cells per colour phase against a pool of 256
    (2046, 0, 1, False),    # its first two-segment M: owned 1023 -> 1024, segments of 1024 and 1022
    (5930, 16, 1, True),    # four segments, owned 1483 -> 1484, short last segment of 1478
    (4096, 33, 2, False),   # four launches: 16, 16, 1 + heat, heat; the result lands in the caller's buffer without a copy
]
SHAPES = SMALL + EDGES
MULTI_SEGMENT = [s for s in EDGES if s[0] in (1982, 1978, 2046, 5930, 4096)]
TWO_SEGMENT = [s for s in EDGES if s[0] in (1982, 1978, 2046)]
PARITY = [(shape, scale) for shape in SHAPES for scale in ("flat", "top", "over", "sharp")] + \
         [(shape, scale) for shape in TWO_SEGMENT for scale in ("mid", "peaked")]
QOI = [(shape, scale) for shape in SHAPES if shape[3] for scale in ("flat", "top", "over", "sharp")]
CLOSED_FORM_M = (2, 4, 6, 1980, 1982)    # n_hb == 0 draws of 16 and 3 sweeps against closed_form.rotor_overrelax_closed_form
BLOCK = [(M, n_or, n_hb, scale) for M in (1982, 6) for n_or, n_hb in ((7, 1), (8, 1), (9, 2)) for scale in ("mid", "over")]
FUSED_SPLIT = [(M, scale) for M in (1980, 1982, 6) for scale in ("top", "over", "sharp")]
# the draws of test_rotor_heat_bath_behind_the_last_overrelaxation_launch, and (16, 1): the launch of 17 sweeps that makes
# M = 1980 the full image and M = 1982 two segments
FUSED_SPLIT_DRAWS = ((10, 1), (8, 1), (3, 2), (1, 1), (17, 1), (16, 1))
POOL = [(2046, scale) for scale in ("top", "over")]
SITE_B = 70                               # rotor_site_update_kernel: 64 threads per block; the second block has 6 live threads
SITE = [(M, scale) for M in (2, 34) for scale in ("mid", "over")]


def case_id(shape, scale=None):
    M, n_or, n_hb, qoi = shape
    return f"M{M}-{n_or}+{n_hb}" + ("-qoi" if qoi else "") + (f"-{scale}" if scale else "")


# ---- inputs and oracle runs ---------------------------------------------------------------------------------------------------
def start(M, n_or, n_hb, scale):
    """[B, M] uniform in [-pi, pi), seeded by the case; every chain its own data"""
    rng = np.random.default_rng([M, n_or, n_hb, list(SCALES).index(scale)])
    return rng.uniform(-np.pi, np.pi, (B, M))


def oracle_action(scale, M):
    import oracle
    return oracle.Action(oracle.ROTOR, **params(scale, M))


@functools.lru_cache(maxsize=None)    # the largest entry: 4 x 3 x 5930 doubles
def oracle_run(M, n_or, n_hb, scale):
    """The draw by the oracle's device-order sweeps, one at a time with keys (SEED, CHAIN0 + b, SWEEP0 + s): (start, state
    in front of the first heat-bath sweep, state behind it, final state); read-only"""
    A = oracle_action(scale, M)
    x = start(M, n_or, n_hb, scale)
    x0, pre, post = x.copy(), None, None
    for s in range(n_or + n_hb):
        if s == n_or:
            pre = x.copy()
        for b in range(B):
            A.dev_sweep(x[b], s >= n_or, SEED, CHAIN0 + b, SWEEP0 + s)
        if s == n_or:
            post = x.copy()
    for a in (x0, pre, post, x):
        if a is not None:
            a.setflags(write=False)
    return x0, pre, post, x


def first_heat_cells(pre, post):
    """(x_plus, x_minus) [B, M] of every cell of a heat-bath sweep from the state in front of it and behind it: the even
    sites (first colour) see the old odd sites, the odd sites the new even ones"""
    nb = pre.copy()
    nb[:, ::2] = post[:, ::2]      # the even sites' new values are what the odd sites read ...
    xp, xm = np.roll(nb, -1, axis=1), np.roll(nb, 1, axis=1)
    ev_p, ev_m = np.roll(pre, -1, axis=1), np.roll(pre, 1, axis=1)
    xp[:, ::2], xm[:, ::2] = ev_p[:, ::2], ev_m[:, ::2]   # ... and the even sites read the old odd ones
    return xp, xm


def step_class(xp, xm):
    """the step envelope's class of a cell, as dev_vonmises_table of the oracle: t = |(x- - x+) / (4 pi)| reduced to
    [0, 1/2], class floor(32 |t - 1/4|), at most 7"""
    v = (xm - xp) * (0.25 / np.pi)
    t = np.abs(v - np.rint(v))
    return np.minimum(VS_CLASSES - 1, (32.0 * np.abs(t - 0.25)).astype(int))


def kappa(scale_value, xp, xm):
    return scale_value * np.abs(np.cos(0.5 * (xm - xp)))


# ---- site-at-a-time updates --------------------------------------------------------------------------------------------------
def site_list(M):
    """a permutation of the sites followed by repeats, with sites 0 and M - 1 next to each other (both orders)"""
    rng = np.random.default_rng(M)
    tail = [0, M - 1, M - 1, 0, M // 2, M // 2, 0]
    return np.concatenate([rng.permutation(M), tail]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def site_run(M, scale, heat):
    """SITE_B chains: the list with step 21, then site M - 1 alone with step 22 (start, want)"""
    A = oracle_action(scale, M)
    rng = np.random.default_rng([M, int(heat), list(SCALES).index(scale)])
    x0 = rng.uniform(-np.pi, np.pi, (SITE_B, M))
    want = x0.copy()
    for b in range(SITE_B):
        for l in site_list(M):
            A.dev_site_update(want[b], l, heat, SEED, CHAIN0 + b, 21)
        A.dev_site_update(want[b], M - 1, heat, SEED, CHAIN0 + b, 22)
    x0.setflags(write=False)
    want.setflags(write=False)
    return x0, want
