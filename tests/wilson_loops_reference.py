"""The definition of mlmcpi_schwinger_wilson_loops in numpy.longdouble, the error bound of its fp64 evaluation, the exact law of
<W(r, s)> on the periodic lattice, and the geometry rule of mlmcpi_schwinger_wilson_loops_plan restated.

State layout: theta[b, 2 (Mt j + i) + mu]; as an array theta4[b, j, i, mu].  For a base vertex (i, j), r links along direction 0
and s along direction 1, all indices periodic,

  Theta(i,j;r,s) = sum_{k<r} theta0(i+k, j) + sum_{l<s} theta1(i+r, j+l) - sum_{k<r} theta0(i+k, j+s) - sum_{l<s} theta1(i, j+l)
  W(r,s)         = (1 / (Mt Mx)) sum_{i,j} cos Theta(i,j;r,s)

wilson_loops() takes this first line literally: boundary-link sums, then cos.  The device kernel multiplies plaquette phases
instead; the two routes share nothing but the definition.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def links(theta, Mt, Mx):
    """theta [B, 2 Mt Mx] -> (theta0, theta1), each [B, Mx, Mt] long double (axis 1: j, axis 2: i)"""
    t = np.asarray(theta, dtype=LD).reshape(-1, Mx, Mt, 2)
    return t[..., 0], t[..., 1]


def loop_angles(theta, Mt, Mx, R, S):
    """Theta [B, R, S, Mx, Mt] long double from the boundary links"""
    t0, t1 = links(theta, Mt, Mx)
    out = np.empty((t0.shape[0], R, S, Mx, Mt), dtype=LD)
    A = np.zeros_like(t0)                       # A_r(i, j) = sum_{k<r} theta0(i + k, j)
    for r in range(1, R + 1):
        A = A + np.roll(t0, -(r - 1), axis=2)
        Bs = np.zeros_like(t1)                  # B_s(i, j) = sum_{l<s} theta1(i, j + l)
        for s in range(1, S + 1):
            Bs = Bs + np.roll(t1, -(s - 1), axis=1)
            out[:, r - 1, s - 1] = A + np.roll(Bs, -r, axis=2) - np.roll(A, -s, axis=1) - Bs
    return out


def wilson_loops(theta, Mt, Mx, R, S):
    """W [B, R, S] long double"""
    return np.cos(loop_angles(theta, Mt, Mx, R, S)).sum(axis=(3, 4)) / LD(Mt * Mx)


def plaquette_angles(theta, Mt, Mx):
    """the unreduced plaquette angle of every cell, [B, Mx, Mt] long double: theta0(i,j) + theta1(i+1,j) - theta0(i,j+1) - theta1(i,j)"""
    t0, t1 = links(theta, Mt, Mx)
    return t0 + np.roll(t1, -1, axis=2) - np.roll(t0, -1, axis=1) - t1


def loop_angles_from_cells(theta, Mt, Mx, R, S):
    """Theta [B, R, S, Mx, Mt] as the sum of the plaquette angles of the r x s cells"""
    p = plaquette_angles(theta, Mt, Mx)
    out = np.empty((p.shape[0], R, S, Mx, Mt), dtype=LD)
    strip = np.zeros_like(p)
    for r in range(1, R + 1):
        strip = strip + np.roll(p, -(r - 1), axis=2)
        acc = np.zeros_like(p)
        for s in range(1, S + 1):
            acc = acc + np.roll(strip, -(s - 1), axis=1)
            out[:, r - 1, s - 1] = acc
    return out


def gauge_transform(theta, Mt, Mx, g):
    """theta_mu(n) + g(n) - g(n + mu^), reduced back to [-pi, pi); g [B, Mx, Mt]"""
    t = np.asarray(theta, dtype=np.float64).reshape(-1, Mx, Mt, 2).copy()
    t[..., 0] += g - np.roll(g, -1, axis=2)
    t[..., 1] += g - np.roll(g, -1, axis=1)
    t -= 2 * np.pi * np.floor((t + np.pi) / (2 * np.pi))
    return t.reshape(t.shape[0], -1)


# ---- the error bound of the device evaluation --------------------------------------------------------------------------------
# Per entry, absolute, in units of eps = 2^-52:  (24 r s + c_sum) eps.
#   24 per cell of the loop: the plaquette angle of four terms in [-pi, pi) carries at most 3 roundings of magnitude <= 4 pi eps / 2,
#   together <= 19 eps of phase; the device sincos (Cody-Waite reduction, one rounding of |r| <= pi/4, Taylor kernels truncated
#   below 0.25 eps) a further 2 eps; and the r s - 1 complex multiplies that join the cells (s (r - 1) in the strips, s - 1 across
#   them), each two rounded products and two FMAs on numbers of modulus 1, i.e. <= sqrt(2) eps < 3 eps.  Errors of unit-modulus
#   factors add to first order, and |Re P - cos Theta| <= |P - e^(i Theta)|.
#   c_sum: every one of the V terms |Re P| <= 1 passes through at most `depth` rounded additions -- J in its thread, 6 levels of
#   the lane tree, 4 waves, `tiles` tiles -- then the product with 1 / V and the rounding of 1 / V itself: the sum / V is off by at
#   most depth eps / 2, depth = J + 6 + 4 + tiles + 2.
def c_sum(plan):
    return 0.5 * (plan["J"] + 6 + 4 + plan["tiles"] + 2)


def bound(plan, R, S):
    """[R, S] float64"""
    r, s = np.arange(1, R + 1)[:, None], np.arange(1, S + 1)[None, :]
    return (24.0 * r * s + c_sum(plan)) * EPS


# ---- the exact law ------------------------------------------------------------------------------------------------------------
def bessel_ratio(n, beta, terms=400):
    """I_n(beta) / I_0(beta) in long double from the power series I_n = sum_k (beta/2)^(2k+n) / (k! (k+n)!) (all terms positive)"""
    h = LD(beta) / 2

    def series(m):
        t = LD(1)
        for q in range(1, m + 1):
            t = t * h / q          # h^m / m!
        s = LD(0)
        for k in range(terms):
            s += t
            t = t * h * h / (LD(k + 1) * LD(k + 1 + m))
            if t < s * LD(1e-25):
                break
        return s

    return series(abs(n)) / series(0)


def wilson_loop_exact(beta, Mt, Mx, r, s, nmax=60):
    """sum_n I_n^(V-A) I_(n+1)^A / sum_n I_n^V over all integers n, V = Mt Mx, A = r s <= V (I_n / I_0 throughout: the common
    factor I_0^V cancels)"""
    V, A = Mt * Mx, r * s
    rho = {n: bessel_ratio(n, beta) for n in range(-nmax - 1, nmax + 2)}
    num = sum(rho[n] ** (V - A) * rho[n + 1] ** A for n in range(-nmax, nmax + 1))
    den = sum(rho[n] ** V for n in range(-nmax, nmax + 1))
    return float(num / den)


def wilson_loops_exact(beta, Mt, Mx, R, S):
    return np.array([[wilson_loop_exact(beta, Mt, Mx, r, s) for s in range(1, S + 1)] for r in range(1, R + 1)])


def string_tension_exact(beta):
    return float(-np.log(bessel_ratio(1, beta)))


def creutz_ratio(W, r, s):
    """-log[W(r,s) W(r-1,s-1) / (W(r-1,s) W(r,s-1))] of W [R, S] (entry [r-1, s-1]), W(0,.) = W(.,0) = 1"""
    w = lambda a, b: 1.0 if a == 0 or b == 0 else W[a - 1][b - 1]
    return float(-np.log(w(r, s) * w(r - 1, s - 1) / (w(r - 1, s) * w(r, s - 1))))


def quadrature_2x2(beta, points=40):
    """<cos a>, <cos(a + b)>, <cos(a + b + c + d)> (areas 1, 2, 4) under the constrained plaquette law of the 2 x 2 torus,
    exp(beta (cos a + cos b + cos c + cos d)) with d = -(a + b + c): the periodic trapezoid rule on the three free plaquettes"""
    t = np.arange(points, dtype=LD) * (2 * np.arccos(LD(-1)) / points)
    a, b, c = t[:, None, None], t[None, :, None], t[None, None, :]
    w = np.exp(LD(beta) * (np.cos(a) + np.cos(b) + np.cos(c) + np.cos(a + b + c) - 4))
    Z = w.sum()
    return float((w * np.cos(a)).sum() / Z), float((w * np.cos(a + b)).sum() / Z), 1.0


# ---- the geometry rule of mlmcpi_schwinger_wilson_loops_plan ----------------------------------------------------------------
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -3
TILE, J, CAP = 32, 4, 16
WORKGROUP, LDS_LIMIT = 256, 65536
MAX_BLOCKS = 2 ** 31 // WORKGROUP * 65535


def plan(Mt, Mx, R, S, B):
    """(status, dict) as mlmcpi_schwinger_wilson_loops_plan reports them"""
    if Mt < 2 or Mx < 2 or Mt * Mx > 2 ** 30 or B == 0 or R == 0 or S == 0:
        return ERR_INVALID, None
    if R > CAP or S > CAP:
        return ERR_UNSUPPORTED, None
    if R > Mt or S > Mx:
        return ERR_INVALID, None
    tw, th = -(-Mt // TILE), -(-Mx // TILE)
    grid = B * tw * th
    if grid > MAX_BLOCKS:
        return ERR_INVALID, None
    return OK, dict(work_bytes=(grid * R * S * 8 + 255) // 256 * 256, grid=grid, workgroup=WORKGROUP, tile_w=TILE, tile_h=TILE,
                    halo_w=R - 1, halo_h=S - 1, J=J, tiles_w=tw, tiles_h=th, tiles=tw * th,
                    lds_bytes=(min(TILE, Mt) + R) * (min(TILE, Mx) + S) * 16, lds_limit=LDS_LIMIT)


def tile_ranges(p, Mt, Mx):
    """the base vertices [i0, i1) x [j0, j1) of every tile of a plan, in tile order"""
    return [(tx * p["tile_w"], min(Mt, (tx + 1) * p["tile_w"]), ty * p["tile_h"], min(Mx, (ty + 1) * p["tile_h"]))
            for ty in range(p["tiles_h"]) for tx in range(p["tiles_w"])]
