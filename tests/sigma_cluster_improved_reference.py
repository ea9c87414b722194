"""long double reference of the improved estimators of the Wolff single-cluster update (sigma_cluster.hip,
mlmcpi_sigma_level_cluster_improved_draw), built on the cluster and the normal that sigma_cluster_model.dev_update
and sigma_level_cluster_model.dev_update return, and a Python statement of the device's integer arithmetic.

A level vertex sits at (i, j) (sigma_correlator_reference.coords), direction 0 = t has x_0 = i, M_0 = Mt, direction 1 = x has
x_1 = j, M_1 = Mx.  With C the cluster of the update, |C| its size and a_l = r . sigma_l of the field before the update

  P_d(i)     = sum_{l in C, x_d(l) = i} a_l,   A = sum_{l in C} a_l
  chi^W      = 3 A^2 / |C|
  F_d^W      = 3 (Ac_d^2 + As_d^2) / |C|,   Ac_d, As_d = sum_i P_d(i) (cos, sin)(2 pi i / M_d)
  C_d^W(tau) = (3 / |C|) sum_{i < M_d} P_d(i) P_d((i + tau) mod M_d),   tau = 0 .. M_d / 2

in the layout of the plain correlator, [n_out] with C_t first.  The seed vertex is uniform and independent of the bonds, so the
mean over the seeds of f(C_seed) / |C_seed| is (1 / n) sum_C f(C): the Swendsen-Wang improved estimators of the same bonds.
"""
import numpy as np

import sigma_correlator_reference as ref
import sigma_sw_correlator_reference as scr
import sigma_sw_structure_reference as ssr
from sigma_cluster_model import _dots
from sigma_model import sigma_of

LD = np.longdouble
FIX = 2.0 ** 32
DELTA = scr.DELTA     # per member: 2^-33 for the rounding of q(a), 2^-32 where a libm ulp in a moves it


def dots(L, phi, r):
    """a_l = r . sigma_l of one chain phi [2 n], float64, formed as the models form it"""
    return _dots(sigma_of(np.asarray(phi, dtype=np.float64).reshape(L.n, 2)), r)


def slices(L, a, members, d):
    """of direction d: (P [M] long double, the sum of |a| [M] float64, the number of members [M]) over the slices"""
    M = (L.Mt, L.Mx)[d]
    x = ref.coords(L.Mt, L.Mx, L.rotated)[d][members]
    am = np.asarray(a, dtype=np.float64)[members]
    P, S, cnt = np.zeros(M, dtype=LD), np.zeros(M), np.zeros(M, dtype=np.int64)
    np.add.at(P, x, am.astype(LD))
    np.add.at(S, x, np.abs(am))
    np.add.at(cnt, x, 1)
    return P, S, cnt


def slice_phases(M):
    """(cos, sin)(2 pi i / M), i < M, long double; exact on the axes"""
    c, s = ssr.phases(type("Ring", (), {"Mt": M, "Mx": 1, "rotated": False})(), 0)   # the M vertices of an M x 1 lattice sit at i
    return c, s


def estimators(L, a, members):
    """(chi^W, F^W [2], C^W [n_out]) of the cluster `members` (vertex indices), long double"""
    size = LD(len(members))
    A = np.asarray(a, dtype=np.float64)[members].astype(LD).sum()
    F, C = [], []
    for d, M in enumerate((L.Mt, L.Mx)):
        P, _, _ = slices(L, a, members, d)
        c, s = slice_phases(M)
        F.append(LD(3) * ((P * c).sum() ** 2 + (P * s).sum() ** 2) / size)
        C.append(LD(3) * np.array([(P * np.roll(P, -tau)).sum() for tau in range(M // 2 + 1)], dtype=LD) / size)
    return LD(3) * A * A / size, np.array(F, dtype=LD), np.concatenate(C)


def seed_average(L, a, labels):
    """the mean over ALL n seed vertices of the estimators of the seed's cluster under the labelling `labels`"""
    by_root = {int(c): estimators(L, a, np.nonzero(labels == c)[0]) for c in np.unique(labels)}
    chi = sum(by_root[int(c)][0] for c in labels) / LD(L.n)
    F = sum(by_root[int(c)][1] for c in labels) / LD(L.n)
    C = sum(by_root[int(c)][2] for c in labels) / LD(L.n)
    return chi, F, C


# ---- the device's arithmetic, restated ------------------------------------------------------------------------------------------
scale_bits = scr.scale_bits   # s = min(32, 62 - ceil(log2(n n_slice))): one cluster's sum |P| |P'| is at most n n_slice as well


def device_model(L, a, members, order=None):
    """what the kernel computes, in its integers: q(a) = rint(a 2^32) of the members onto the slice table (in the order `order`),
    A = sum_i P_0(i), Ac_d = sum_i rint(float(P_d(i)) w^c), the terms rint((float(P) float(P')) 2^(s - 64)) over the occupied
    slices, and the fixed expressions at the end.  (chi, F [2], C [n_out]) float64"""
    s, size = scale_bits(L), len(members)
    f = 3.0 / float(size)
    members = list(members) if order is None else [members[k] for k in order]
    q = np.rint(np.asarray(a, dtype=np.float64) * FIX).astype(np.int64)
    coords = ref.coords(L.Mt, L.Mx, L.rotated)
    tables = []
    for d, M in enumerate((L.Mt, L.Mx)):
        tab = [0] * M
        for l in members:
            tab[int(coords[d][l])] += int(q[l])
        tables.append(tab)
    x = float(sum(tables[0])) * 2.0 ** -32
    chi = (x * x) * f
    F, C = [], []
    for d, M in enumerate((L.Mt, L.Mx)):
        tab = tables[d]
        c, sn = (w.astype(np.float64) for w in slice_phases(M))
        Ac = sum(int(np.rint(float(P) * c[i])) for i, P in enumerate(tab) if P)
        As = sum(int(np.rint(float(P) * sn[i])) for i, P in enumerate(tab) if P)
        xc, xs = float(Ac) * 2.0 ** -32, float(As) * 2.0 ** -32
        Fd = 0.0
        Fd += (xc * xc) * f
        Fd += (xs * xs) * f
        F.append(Fd)
        occ = [i for i, P in enumerate(tab) if P]
        acc = [0] * (M // 2 + 1)
        for i in occ:
            for j in occ:
                tau = (j - i) % M
                if tau <= M // 2:
                    acc[tau] += int(np.rint((float(tab[i]) * float(tab[j])) * 2.0 ** (s - 64)))
        assert all(abs(v) < 2 ** 63 for v in acc)
        C.append(np.array([(float(v) * 2.0 ** -s) * f for v in acc]))
    return chi, np.array(F), np.concatenate(C)


def device_bound(L, a, members):
    """absolute bound on |device C^W - estimators(...)[2]| per lag, [n_out], from the roundings and nothing else, as
    sigma_sw_correlator_reference.device_bound builds it.  (1) The device's P~(i) is a sum of llrint(a 2^32): off by at most
    delta_i = n(i) DELTA, n(i) the members in the slice; with S_i the sum of |a| there, a product is off by S_i delta_j + S_j delta_i
    + delta_i delta_j.  (2) The conversions of the two integers, their product, the conversion of the accumulator, 3 / |C| and the
    last product: 8 x 2^-53 of (S_i + delta_i)(S_j + delta_j) covers them with room.  (3) Every term is rounded to the accumulator's
    unit: 2^-(s + 1) per pair of occupied slices."""
    s, size = scale_bits(L), len(members)
    out = []
    for d, M in enumerate((L.Mt, L.Mx)):
        _, S, cnt = slices(L, a, members, d)
        delta = cnt * DELTA
        b = np.zeros(M // 2 + 1)
        for tau in range(M // 2 + 1):
            Sj, dj, hit = np.roll(S, -tau), np.roll(delta, -tau), (cnt > 0) & (np.roll(cnt, -tau) > 0)
            b[tau] = ((S * dj + Sj * delta + delta * dj)[hit]).sum() + 8 * 2.0 ** -53 * (((S + delta) * (Sj + dj))[hit]).sum() \
                + hit.sum() * 2.0 ** -(s + 1)
        out.append(3.0 * b / size)
    return np.concatenate(out)


def susceptibility_bound(L, a, members):
    """absolute bound on |device chi^W - 3 A^2 / |C||: A~ is off by delta = |C| DELTA, its square by delta (2 S + delta) with S the
    sum of |a| >= |A|; the conversion of A~, the square, 3 / |C| and the last product are four roundings: 6 x 2^-53 (S + delta)^2"""
    size = len(members)
    S = float(np.abs(np.asarray(a, dtype=np.float64)[members]).sum())
    delta = size * DELTA
    return 3.0 * (delta * (2.0 * S + delta) + 6 * 2.0 ** -53 * (S + delta) ** 2) / size


def structure_bound(L, a, members, d):
    """absolute bound on |device F_d^W - estimators(...)[1][d]|.  Ac~ = sum_i llrint((double)P~(i) w(i)): P~(i) is off by delta_i
    (|w| <= 1), its conversion, the device's weight against the exact one (4 x 2^-53 absolute: two ulp of sincospi) and the product
    cost 8 x 2^-53 S_i, and llrint half a unit, 2^-33, per occupied slice: e in all.  |Ac| <= S, so the square is off by e (2 S + e),
    and there are two sums; the conversions, squares, 3 / |C|, products and the two adds: 8 x 2^-53 x 2 (S + e)^2."""
    size = len(members)
    _, S, cnt = slices(L, a, members, d)
    e = float((cnt * DELTA + 8 * 2.0 ** -53 * S + (cnt > 0) * 2.0 ** -33).sum())
    tot = float(S.sum())
    return 3.0 * (2.0 * e * (2.0 * tot + e) + 16 * 2.0 ** -53 * (tot + e) ** 2) / size
