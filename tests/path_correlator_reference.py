"""The definition of mlmcpi_path_correlator in numpy.longdouble, the error bound of its fp64 evaluation, the closed forms of
<C(tau)> on the periodic lattice (harmonic oscillator, rotor), and the geometry rule of mlmcpi_path_correlator_plan restated.

  kinds 0, 1   C(tau) = (1/M) sum_j x_j x_{(j + tau) mod M}
  kind 2       C(tau) = (1/M) sum_j cos(x_j - x_{(j + tau) mod M})
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
ROTOR = 2


def components(kind, x):
    """the 1 or 2 planes whose circular autocorrelation C is: (x,) or (cos x, sin x), long double"""
    x = np.asarray(x, dtype=LD)
    return (np.cos(x), np.sin(x)) if kind == ROTOR else (x,)


def _sums(kind, x, n_lag):
    """(sum_j p_j(tau), sum_j |p_j(tau)|) over the components, [..., n_lag] long double; p_j = c_j c_{j+tau}.  Paths that are zero
    almost everywhere (the spike inputs of the oscillators) are summed over their non-zero sites only: the same numbers"""
    comps = components(kind, x)
    M = comps[0].shape[-1]
    val = np.zeros(comps[0].shape[:-1] + (n_lag,), dtype=LD)
    mag = np.zeros_like(val)
    for c in comps:
        nz = np.flatnonzero(np.any(c.reshape(-1, M) != 0, axis=0))
        if 8 * nz.size < M:
            for j in nz:
                k = (j + np.arange(n_lag)) % M
                p = c[..., j:j + 1] * c[..., k]
                val += p
                mag += np.abs(p)
        else:
            for tau in range(n_lag):
                p = c * np.roll(c, -tau, axis=-1)
                val[..., tau] += np.sum(p, axis=-1)
                mag[..., tau] += np.sum(np.abs(p), axis=-1)
    return val, mag, M


def correlator(kind, x, n_lag):
    """[..., n_lag] long double"""
    val, _, M = _sums(kind, x, n_lag)
    return val / LD(M)


def correlator_and_bound(kind, x, n_lag):
    """the correlator and, per entry, the bound on its fp64 evaluation: 2 (M + 4) eps (1/M) sum_j |x_j x_{j+tau}| -- M rounded
    products summed in any order --, for the rotor with (2 (M + 4) + 16) eps and |c c'| + |s s'|: a few ulp for each sincos"""
    val, mag, M = _sums(kind, x, n_lag)
    k = 2 * (M + 4) + (16 if kind == ROTOR else 0)
    return val / LD(M), (k * EPS * mag / LD(M)).astype(np.float64)


def weights(M):
    """correlator_weight of include/mlmcpi/correlator.hh over tau = 0 .. M/2 (odd M: 1, then 2 everywhere)"""
    tau = np.arange(M // 2 + 1)
    return np.where((tau == 0) | (2 * tau == M), 1.0, 2.0)


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def ho_omega(M, T_final, mu2):
    a = T_final / M
    return float(np.arccosh(1.0 + 0.5 * a * a * mu2))


def ho_exact(M, T_final, m0, mu2, tau):
    """(a / m0) cosh(w (M/2 - tau)) / (2 sinh w sinh(w M/2)), cosh w = 1 + a^2 mu2 / 2"""
    a, w = T_final / M, ho_omega(M, T_final, mu2)
    return (a / m0) * np.cosh(w * (0.5 * M - np.asarray(tau))) / (2.0 * np.sinh(w) * np.sinh(0.5 * w * M))


def ho_eigen_sum(M, T_final, m0, mu2, tau):
    """(1/M) sum_k cos(2 pi k tau / M) / lambda_k, lambda_k = (m0/a)(2 - 2 cos(2 pi k / M)) + a m0 mu2"""
    a, k = LD(T_final) / LD(M), np.arange(M, dtype=LD)
    two_pi = 2 * np.arccos(LD(-1))
    lam = LD(m0) / a * (2 - 2 * np.cos(two_pi * k / M)) + a * LD(m0) * LD(mu2)
    return np.array([float(np.sum(np.cos(two_pi * k * t / M) / lam) / M) for t in np.atleast_1d(tau)])


def bessel_i(n, kappa, points=256):
    """I_n(kappa) = (1/pi) int_0^pi exp(kappa cos t) cos(n t) dt: the periodic trapezoid rule, exact to rounding here"""
    t = (np.arange(2 * points, dtype=LD) + LD(0.5)) * (np.arccos(LD(-1)) / points)
    return np.sum(np.exp(LD(kappa) * np.cos(t)) * np.cos(n * t)) / (2 * points)


def rotor_exact(M, kappa, tau, nmax=40):
    """sum_n I_n^(M - tau) I_(n+1)^tau / sum_n I_n^M over all integers n (the character expansion)"""
    I = {n: bessel_i(abs(n), kappa) for n in range(-nmax - 1, nmax + 2)}
    Z = sum(I[n] ** M for n in range(-nmax, nmax + 1))
    return np.array([float(sum(I[n] ** (M - t) * I[n + 1] ** t for n in range(-nmax, nmax + 1)) / Z) for t in np.atleast_1d(tau)])


def rotor_brute_force(M, kappa, tau, points=64):
    """<cos(x_0 - x_tau)> under exp(kappa sum_j cos(x_j - x_{j+1})) by the periodic trapezoid rule on every angle"""
    t = np.arange(points, dtype=LD) * (2 * np.arccos(LD(-1)) / points)
    K = np.exp(LD(kappa) * np.cos(t[:, None] - t[None, :]))  # transfer matrix
    D = np.cos(t[:, None] - t[None, :])
    Kp = {0: np.eye(points, dtype=LD)}
    for k in range(1, M + 1):
        Kp[k] = Kp[k - 1] @ K
    Z = np.trace(Kp[M])
    # sum over x_0, x_tau of K^tau(x_0, x_tau) cos(x_0 - x_tau) K^(M - tau)(x_tau, x_0)
    return np.array([float(np.sum(Kp[t_] * D * Kp[M - t_].T) / Z) for t_ in np.atleast_1d(tau)])


# ---- the geometry rule of mlmcpi_path_correlator_plan -----------------------------------------------------------------------
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -3
J = T = 8
WORKGROUP, LDS_LIMIT, TILE_BYTES = 256, 65536, 80
MAX_BLOCKS = 2 ** 31 // WORKGROUP * 65535


def max_tiles(kind):
    return LDS_LIMIT // (TILE_BYTES * (2 if kind == ROTOR else 1))


def lag_cap(kind):
    """the largest n_lag whose lag tiles leave room for one site tile in the LDS image"""
    return T * (max_tiles(kind) - 1)


def plan(kind, M, n_lag, B):
    """(status, dict) as mlmcpi_path_correlator_plan reports them"""
    if kind not in (0, 1, 2) or M == 0 or B == 0 or n_lag == 0 or n_lag > M // 2 + 1:
        return ERR_INVALID, None
    ncomp, mt = (2 if kind == ROTOR else 1), max_tiles(kind)
    tiles, lag_tiles = -(-M // J), -(-n_lag // T)
    if lag_tiles + 1 > mt:
        return ERR_UNSUPPORTED, None
    if tiles + lag_tiles <= mt:
        nseg, own_tiles = 1, tiles
    else:
        n = -(-tiles // (mt - lag_tiles))
        own_tiles = -(-tiles // n)
        nseg = -(-tiles // own_tiles)
    image_tiles = own_tiles + lag_tiles
    packed = nseg == 1 and own_tiles * lag_tiles <= 256 and image_tiles <= mt // 4
    wpc = 1 if packed else 4
    cpw = 4 // wpc
    G = 1
    while G < 64 and G < own_tiles:
        G *= 2
    grid = -(-B // cpw) * nseg
    if grid > MAX_BLOCKS:
        return ERR_INVALID, None
    return OK, dict(workgroup=WORKGROUP, chains_per_workgroup=cpw, waves_per_chain=wpc, group=G, owned=M if nseg == 1 else J * own_tiles,
                    nseg=nseg, J=J, T=T, lag_tiles=lag_tiles, image_tiles=image_tiles, components=ncomp,
                    lds_bytes=cpw * ncomp * image_tiles * TILE_BYTES, lds_limit=LDS_LIMIT, grid=grid,
                    work_bytes=((B * nseg * n_lag * 8 + 255) // 256 * 256) if nseg > 1 else 256)
