"""Long-double reference of the momentum-projected GFF slice correlators (mlmcpi_gff_correlator, include/mlmcpi_hip.h), written
from the definitions:

    S^t_i(q) = sum_j phi(i, j) e^{-2 pi i q j / Mx}      C_t(tau; q) = (1/N) sum_i Re[S^t_i(q) conj S^t_{(i + tau) mod Mt}(q)]
    S^x_j(q) = sum_i phi(i, j) e^{-2 pi i q i / Mt}      C_x(tau; q) = (1/N) sum_j Re[S^x_j(q) conj S^x_{(j + tau) mod Mx}(q)]

a direct DFT of every slice with twiddles computed in numpy.longdouble (the angle 2 pi ((q j) mod M) / M with a long-double pi), both
layouts.  Beside it: the restated launch plan (bands, chunks, workspace bytes), the rounding count of the route the kernels take, the
sites next to every band, tile and chunk boundary, and the exact law of the GFF action in long double."""
import numpy as np

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
EPS = 2.0 ** -53
MAX_MOMENTA = 8
TILE, BAND, THREADS, LAGS_PER_WORKGROUP, LDS_LIMIT = 64, 256, 256, 32, 65536


def n_vertices(Mt, Mx, rotated):
    return Mt * Mx // 2 if rotated else Mt * Mx


def n_out(Mt, Mx, P):
    return P * (Mt // 2 + 1) + P * (Mx // 2 + 1)


def coordinates(Mt, Mx, rotated):
    """(i, j) of every entry of a state, in its order: unrotated l = Mt j + i; rotated: planes E then O of Mt/2 x Mx/2, index
    p (Mt Mx / 4) + (Mt/2) b + a = vertex (2 a + p, 2 b + p)"""
    if not rotated:
        l = np.arange(Mt * Mx)
        return l % Mt, l // Mt
    ht, hx = Mt // 2, Mx // 2
    l = np.arange(2 * ht * hx)
    p, r = l // (ht * hx), l % (ht * hx)
    return 2 * (r % ht) + p, 2 * (r // ht) + p


def grid(phi, Mt, Mx, rotated):
    """F[b, i, j] = phi(i, j) of chain b in long double, zero where the level has no vertex"""
    phi = np.asarray(phi)
    i, j = coordinates(Mt, Mx, rotated)
    F = np.zeros((phi.shape[0], Mt, Mx), dtype=LD)
    F[:, i, j] = phi.astype(LD)
    return F


def twiddles(M, P):
    """(cos, sin)(2 pi q k / M) [M, P] in long double, the product q k reduced mod M in integers"""
    k = (np.arange(M, dtype=np.int64)[:, None] * np.arange(P, dtype=np.int64)[None, :]) % M
    a = 2 * PI * k.astype(LD) / LD(M)
    return np.cos(a), np.sin(a)


def slice_sums(F, P):
    """S^t [B, P, Mt] and S^x [B, P, Mx] as (re, im) pairs of long-double arrays"""
    B, Mt, Mx = F.shape
    cx, sx = twiddles(Mx, P)
    ct, st = twiddles(Mt, P)
    St = (np.einsum("bij,jq->bqi", F, cx), -np.einsum("bij,jq->bqi", F, sx))
    Sx = (np.einsum("bij,iq->bqj", F, ct), -np.einsum("bij,iq->bqj", F, st))
    return St, Sx


def _lags(re, im, n):
    M = re.shape[-1]
    out = np.empty(re.shape[:-1] + (M // 2 + 1,), dtype=LD)
    for tau in range(M // 2 + 1):
        out[..., tau] = (re * np.roll(re, -tau, axis=-1) + im * np.roll(im, -tau, axis=-1)).sum(axis=-1) / LD(n)
    return out


def correlator(phi, Mt, Mx, P, rotated=False):
    """[B, n_out] in long double: C_t first, momentum-major, lag fastest"""
    F = grid(phi, Mt, Mx, rotated)
    St, Sx = slice_sums(F, P)
    n = n_vertices(Mt, Mx, rotated)
    Ct, Cx = _lags(*St, n), _lags(*Sx, n)
    B = F.shape[0]
    return np.concatenate([Ct.reshape(B, -1), Cx.reshape(B, -1)], axis=1)


def split(out, Mt, Mx, P):
    """C_t [.., P, Mt/2 + 1] and C_x [.., P, Mx/2 + 1] of a vector of n_out entries"""
    nt, nx = Mt // 2 + 1, Mx // 2 + 1
    lead = out.shape[:-1]
    return out[..., :P * nt].reshape(lead + (P, nt)), out[..., P * nt:].reshape(lead + (P, nx))


# ---- the launch plan, restated (gff_correlator.hip; mlmcpi_gff_correlator_plan) ----

def _align256(n):
    return (n + 255) // 256 * 256


def plan(Mt, Mx, rotated, P, n_chains=1):
    W, H, planes = (Mt // 2, Mx // 2, 2) if rotated else (Mt, Mx, 1)
    chunks, bands = -(-W // TILE), -(-H // BAND)
    lag_blocks = -(-(Mt // 2 + 1) // LAGS_PER_WORKGROUP) + -(-(Mx // 2 + 1) // LAGS_PER_WORKGROUP)
    in_lds = max(Mt, Mx) * 16 <= LDS_LIMIT
    work = (_align256((Mt + Mx) * 16) + _align256(n_chains * planes * bands * P * W * 16)
            + _align256(n_chains * planes * chunks * P * H * 16) + _align256(n_chains * P * (Mt + Mx) * 16))
    return dict(work_bytes=work, grid=n_chains * planes * bands * chunks, gather_grid=n_chains * -(-(P * (Mt + Mx)) // THREADS),
                lag_grid=n_chains * P * lag_blocks, workgroup=THREADS, tile=TILE, band_rows=BAND, planes=planes, plane_w=W, plane_h=H,
                chunks=chunks, bands=bands, vector_loads=int(W % 2 == 0), table_entries=Mt + Mx, lags_per_workgroup=LAGS_PER_WORKGROUP,
                lags_in_lds=int(in_lds), lds_bytes=TILE * (TILE + 1) * 8 + 2 * MAX_MOMENTA * TILE * 16,
                lag_lds_bytes=max(Mt, Mx) * 16 if in_lds else 0, lds_limit=LDS_LIMIT)


def rounding_count(Mt, Mx, rotated, direction):
    """k of the bound k eps (1/N) sum_i A_i A_{i + tau}, A_i = sum over the slice of |phi|, for the route gff_correlator.hip takes.
    A component (re or im) of a slice sum: each term is phi times a table entry with an absolute error of 3 eps at the most (the
    division of the reduced argument, sincospi to 2 ulp), added by an FMA (the product is not rounded); the additions of a slice
    run over the rows of a band (columns of a chunk) and then over the bands (chunks): n = min(H, 256) + bands (min(W, 64) +
    chunks) roundings, each of a partial sum <= A_i: |dS| <= (n + 3) eps A_i.  A term Re[S_i conj S_k] = re re' + im im' has two
    such factors: (|re'| + |im'|) dS_i + (|re| + |im|) dS_k <= 2 sqrt(2) (n + 3) eps A_i A_k, and a rounded product plus an FMA: 2.
    The lag sum adds ceil(M_d / 64) terms per lane and six levels of the lane tree, each rounding of a partial sum <= sum A_i A_k;
    the factor 1/N is itself rounded and applied by a rounded product: 2."""
    p = plan(Mt, Mx, rotated, 1)
    if direction == 0:
        n, M = min(p["plane_h"], BAND) + p["bands"], Mt
    else:
        n, M = min(p["plane_w"], TILE) + p["chunks"], Mx
    return 2 * np.sqrt(2.0) * (n + 3) + 2 + -(-M // 64) + 6 + 2


def bound(phi, Mt, Mx, P, rotated=False):
    """the absolute bound per entry of correlator(), [B, n_out] float64: rounding_count eps (1/N) sum_i A_i A_{i + tau}; the same
    for every momentum"""
    A = np.abs(grid(phi, Mt, Mx, rotated))
    n = n_vertices(Mt, Mx, rotated)
    At, Ax = A.sum(axis=2), A.sum(axis=1)
    zt, zx = np.zeros_like(At), np.zeros_like(Ax)
    bt = _lags(At, zt, n) * rounding_count(Mt, Mx, rotated, 0) * EPS
    bx = _lags(Ax, zx, n) * rounding_count(Mt, Mx, rotated, 1) * EPS
    B = A.shape[0]
    return np.concatenate([np.repeat(bt[:, None, :], P, axis=1).reshape(B, -1), np.repeat(bx[:, None, :], P, axis=1).reshape(B, -1)],
                          axis=1).astype(np.float64)


def boundary_sites(Mt, Mx, rotated):
    """state indices of the vertices in the first and last row and column of every plane (its corners among them) and on both
    sides of every tile, band and chunk boundary of the plan"""
    p = plan(Mt, Mx, rotated, 1)
    W, H = p["plane_w"], p["plane_h"]
    rows = {0, H - 1} | {r + d for r in range(TILE, H, TILE) for d in (-1, 0)}   # band boundaries are tile boundaries as well
    cols = {0, W - 1} | {c + d for c in range(TILE, W, TILE) for d in (-1, 0)}
    return np.array(sorted(pl * W * H + r * W + c for pl in range(p["planes"]) for r in rows for c in cols), dtype=np.int64)


def spiked_field(seed, B, Mt, Mx, rotated):
    """normals plus single spikes of 20 .. 100 times their size, either sign, at boundary_sites of every chain"""
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((B, n_vertices(Mt, Mx, rotated)))
    sites = boundary_sites(Mt, Mx, rotated)
    phi[:, sites] += rng.uniform(20.0, 100.0, (B, sites.size)) * rng.choice([-1.0, 1.0], (B, sites.size))
    return phi


# ---- the exact law of the GFF action on the unrotated Mt x Mx lattice, mu^2 = (mass / Mt)^2 ----

def dispersion_exact(Mt, Mx, mass, q):
    mu2 = (LD(mass) / Mt) ** 2
    return np.arccosh(1 + (mu2 + 2 - 2 * np.cos(2 * PI * q / Mx)) / 2)


def correlator_exact(Mt, Mx, mass, q, tau):
    """the mode sum (1/Mt) sum_k cos(2 pi k tau / Mt) / (4 + mu^2 - 2 cos(2 pi k / Mt) - 2 cos(2 pi q / Mx))"""
    mu2 = (LD(mass) / Mt) ** 2
    k = np.arange(Mt)
    lam = 4 + mu2 - 2 * np.cos(2 * PI * k.astype(LD) / Mt) - 2 * np.cos(2 * PI * q / Mx)
    return (np.cos(2 * PI * ((k * tau) % Mt).astype(LD) / Mt) / lam).sum() / Mt


def correlator_closed(Mt, Mx, mass, q, tau):
    """cosh(E (Mt/2 - tau)) / (2 sinh E sinh(E Mt / 2))"""
    E = dispersion_exact(Mt, Mx, mass, q)
    return np.cosh(E * (LD(Mt) / 2 - tau)) / (2 * np.sinh(E) * np.sinh(E * Mt / 2))


def effective_mass(C, tau):
    return np.arccosh((C[tau - 1] + C[tau + 1]) / (2 * C[tau]))
