"""numpy reference, in long double, of the time-slice correlators of the O(3) sigma model on a level of its CoarsenRotate
hierarchy (mlmcpi_sigma_level_correlator, include/mlmcpi_hip.h), written from the definitions:

    S^t_i = sum_j sigma(i, j),  S^x_j = sum_i sigma(i, j)   over the vertices of the level (rotated: those with i + j even)
    C_t(tau) = (1/N) sum_i S^t_i . S^t_{(i + tau) mod Mt}, tau = 0 .. Mt/2;  C_x likewise;  output C_t then C_x.

Slice sums go by explicit coordinates: `coords` is the index map of tests/sigma_level_model.py (Level.lin2cart) for a whole level
at once, pinned to it by tests/test_sigma_correlator_reference.py.  The host arithmetic of include/mlmcpi/correlator.hh
(weights, chi, F, xi_2) is mirrored here as well.
"""
import numpy as np

import sigma_model as sm

LD = np.longdouble
EPS = 2.0 ** -52


def nvert(Mt, Mx, rotated):
    return Mt * Mx // 2 if rotated else Mt * Mx


def n_out(Mt, Mx):
    return (Mt // 2 + 1) + (Mx // 2 + 1)


def coords(Mt, Mx, rotated):
    """(i, j) of every vertex index l of the level: Level.lin2cart of sigma_level_model, vectorised"""
    l = np.arange(nvert(Mt, Mx, rotated))
    if not rotated:
        return l % Mt, l // Mt
    q, ht = Mt * Mx // 4, Mt // 2
    p, r = l // q, l % q
    return 2 * (r % ht) + p, 2 * (r // ht) + p


def spins(phi, n):
    """[B, 2 n] float64 angles -> [B, n, 3] long double unit vectors"""
    a = np.asarray(phi, dtype=np.float64).astype(LD).reshape(phi.shape[0], n, 2)
    st = np.sin(a[..., 0])
    return np.stack([st * np.cos(a[..., 1]), st * np.sin(a[..., 1]), np.cos(a[..., 0])], axis=-1)


def slice_sums(Mt, Mx, rotated, phi):
    """S^t [B, Mt, 3] and S^x [B, Mx, 3]"""
    sig = spins(phi, nvert(Mt, Mx, rotated))
    i, j = coords(Mt, Mx, rotated)
    St = np.zeros((sig.shape[0], Mt, 3), dtype=LD)
    Sx = np.zeros((sig.shape[0], Mx, 3), dtype=LD)
    for b in range(sig.shape[0]):
        np.add.at(St[b], i, sig[b])
        np.add.at(Sx[b], j, sig[b])
    return St, Sx


def _lags(S, N):
    M = S.shape[1]
    return np.stack([(S * np.roll(S, -tau, axis=1)).sum(axis=(1, 2)) for tau in range(M // 2 + 1)], axis=1) / LD(N)


def correlator(Mt, Mx, rotated, phi):
    """[B, n_out] long double: C_t(0 .. Mt/2), then C_x(0 .. Mx/2)"""
    St, Sx = slice_sums(Mt, Mx, rotated, phi)
    N = nvert(Mt, Mx, rotated)
    return np.concatenate([_lags(St, N), _lags(Sx, N)], axis=1)


def brute_force(Mt, Mx, rotated, phi):
    """the same numbers as a double sum over vertex pairs with the same coordinate difference (small levels only)"""
    N = nvert(Mt, Mx, rotated)
    sig = spins(phi, N)
    i, j = coords(Mt, Mx, rotated)
    dots = np.einsum("bvc,bwc->bvw", sig, sig)
    out = []
    for x, M in ((i, Mt), (j, Mx)):
        diff = (x[None, :] - x[:, None]) % M    # [v, w]: coordinate of w minus that of v
        out += [dots[:, diff == tau].sum(axis=1) / LD(N) for tau in range(M // 2 + 1)]
    return np.stack(out, axis=1)


def split(C, Mt, Mx):
    """[..., n_out] -> C_t [..., Mt/2 + 1], C_x [..., Mx/2 + 1]"""
    return C[..., :Mt // 2 + 1], C[..., Mt // 2 + 1:]


# ---- include/mlmcpi/correlator.hh ---------------------------------------------------------------------------------------
def weights(M):
    w = np.full(M // 2 + 1, 2.0)
    w[0] = w[M // 2] = 1.0
    return w


def susceptibility(C, M):
    return (np.asarray(C) * weights(M)).sum(axis=-1)


def structure_factor(C, M):
    return (np.asarray(C) * weights(M) * np.cos(2.0 * np.pi * np.arange(M // 2 + 1) / M)).sum(axis=-1)


def xi_second_moment(C, M):
    return np.sqrt(susceptibility(C, M) / structure_factor(C, M) - 1.0) / (2.0 * np.sin(np.pi / M))


def single_cosh(M, m):
    """C(tau) = sum_n exp(-m |tau + n M|), tau = 0 .. M/2 (the periodic image sum in closed form)"""
    tau = np.arange(M // 2 + 1)
    return (np.exp(-m * tau) + np.exp(-m * (M - tau))) / (1.0 - np.exp(-m * M))


# ---- the 2 x 2 lattice ------------------------------------------------------------------------------------------------------
def ring_c1_c2(beta, lmax=60):
    """<sigma_n . sigma_{n+1}> and <sigma_n . sigma_{n+2}> on the ring of four spins the 2 x 2 lattice is (coupling 2 beta): the
    transfer-matrix sums of sigma_model.ring_exact.  C_t(0) = C_x(0) = 1 + c1, C_t(1) = C_x(1) = c1 + c2."""
    lam = np.array([sm._sph_in(l, 2.0 * beta) for l in range(lmax + 1)])
    l = np.arange(lmax)
    Z = np.sum((2 * np.arange(lmax + 1) + 1) * lam ** 4)
    c1 = np.sum((l + 1) * (lam[:-1] * lam[1:] ** 3 + lam[:-1] ** 3 * lam[1:])) / Z
    c2 = np.sum(2 * (l + 1) * lam[:-1] ** 2 * lam[1:] ** 2) / Z
    return c1, c2


# ---- what the device tests share --------------------------------------------------------------------------------------------
def tolerance(Mt, Mx, rotated):
    """absolute bound per entry [n_out]: 4 (n_s + M_d) eps n_s, n_s the vertices per slice, M_d the extent: the worst case of two
    nested fp64 sums of unit vectors whose components carry a few ulp from sincos"""
    h = 2 if rotated else 1
    tt = 4.0 * (Mx // h + Mt) * EPS * (Mx // h)
    tx = 4.0 * (Mt // h + Mx) * EPS * (Mt // h)
    return np.concatenate([np.full(Mt // 2 + 1, tt), np.full(Mx // 2 + 1, tx)])


def planted(Mt, Mx, rotated, B, seed):
    """angles [B, 2 n] of sigma ~ e_z + 0.8 cos(2 pi i / Mt) e_x + 0.6 cos(2 pi 2 j / Mx) e_y + 0.3 noise, normalised: C_t and C_x
    take distinct O(slice length) values at every lag and differ from each other"""
    i, j = coords(Mt, Mx, rotated)
    rng = np.random.default_rng(seed)
    v = 0.3 * rng.normal(size=(B, i.size, 3))
    v[..., 0] += 0.8 * np.cos(2.0 * np.pi * i / Mt)
    v[..., 1] += 0.6 * np.cos(2.0 * np.pi * 2 * j / Mx)
    v[..., 2] += 1.0
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return sm.angles_of(v).reshape(B, 2 * i.size)
