"""long double reference of the cluster-improved structure factor of the Swendsen-Wang update (sigma_sw.hip,
mlmcpi_sigma_level_sw_structure_draw), built on the labels and a = r . sigma that sigma_sw_model.dev_update and
sigma_level_sw_model.dev_update return.

A level vertex sits at (i, j) (sigma_correlator_reference.coords: unrotated l = Mt j + i; rotated plane p, cell (a, b) at (2 a + p,
2 b + p)), direction 0 = t has x_0 = i, M_0 = Mt, direction 1 = x has x_1 = j, M_1 = Mx.  With w^c = cos(2 pi x_d / M_d), w^s = sin:

  plain     F_d     = |sum_l sigma_l e^{2 pi i x_d / M_d}|^2 / n
  improved  F_d^imp = (3 / n) sum_C [ (sum_{l in C} a_l w^c)^2 + (sum_{l in C} a_l w^s)^2 ]

F_d^imp is the mean over the coins (each cluster's sign) of 3 |sum_l +-a_l e^{ipx}|^2 / n: the cross terms of two clusters vanish,
and the mean over r of (r . v)^2 is |v|^2 / 3 (the argument of the improved chi_m, with the phases carried along).
"""
import itertools

import numpy as np

import sigma_correlator_reference as ref

LD = np.longdouble
PI = LD(np.pi) + LD(1.2246467991473532e-16)   # pi to long double: the double and what it leaves out


def phases(L, d):
    """(cos, sin)(2 pi x_d / M_d) of every vertex, long double; exact on the axes (an extent of 2 gives +-1 and 0)"""
    x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
    M = (L.Mt, L.Mx)[d]
    table_c = np.array([LD(1) if 4 * k == 0 else LD(-1) if 2 * k == M else LD(0) if 4 * k in (M, 3 * M) else np.cos(2 * PI * LD(k) / LD(M))
                        for k in range(M)], dtype=LD)
    table_s = np.array([LD(0) if 2 * k in (0, M) else LD(1) if 4 * k == M else LD(-1) if 4 * k == 3 * M else np.sin(2 * PI * LD(k) / LD(M))
                        for k in range(M)], dtype=LD)
    return table_c[x], table_s[x]


def plain(L, sig, d):
    """F_d of unit vectors sig [n, 3] from the positions"""
    c, s = phases(L, d)
    v = np.asarray(sig, dtype=LD)
    re, im = (v * c[:, None]).sum(axis=0), (v * s[:, None]).sum(axis=0)
    return ((re * re).sum() + (im * im).sum()) / LD(len(v))


def cluster_sums(L, a, labels, d):
    """{root: (sum a w^c, sum a w^s, n_C, sum |a|)} in long double"""
    c, s = phases(L, d)
    a = np.asarray(a, dtype=np.float64).astype(LD)
    out = {}
    for root in np.unique(labels):
        m = labels == root
        out[int(root)] = ((a[m] * c[m]).sum(), (a[m] * s[m]).sum(), int(m.sum()), np.abs(a[m]).sum())
    return out


def improved(L, a, labels, d):
    return LD(3) * sum(Ac * Ac + As * As for Ac, As, _, _ in cluster_sums(L, a, labels, d).values()) / LD(len(a))


def coin_mean(L, a, labels, d):
    """the mean over ALL coin assignments of 3 |sum_l s_C(l) a_l e^{ipx}|^2 / n, by enumeration (few clusters only)"""
    sums = list(cluster_sums(L, a, labels, d).values())
    assert len(sums) <= 12
    tot = LD(0)
    for signs in itertools.product((1, -1), repeat=len(sums)):
        re = sum(sg * Ac for sg, (Ac, _, _, _) in zip(signs, sums))
        im = sum(sg * As for sg, (_, As, _, _) in zip(signs, sums))
        tot += re * re + im * im
    return LD(3) * tot / LD(2 ** len(sums)) / LD(len(a))


DELTA = 1.5 * 2.0 ** -32   # per vertex: half a unit of the fixed point for its rounding, one unit for a libm ulp that moves it


def device_bound(L, a, labels, d):
    """absolute bound on |device F_d^imp - improved(...)|.  The device adds llrint((a w) 2^32) per vertex: against the exact a w
    that is off by at most half a unit 2^-32 (rounding) and, where an ulp of the device's libm against numpy's moves a w across a
    rounding boundary, one unit more: delta = 1.5 x 2^-32 per vertex.  A cluster sum S of n_C vertices is then off by at most n_C
    delta, its square by n_C delta (2 |S| + n_C delta) <= n_C delta (2 sum_C |a| + n_C delta), and a direction has two sums (cos,
    sin): (3 / n) sum_C [4 delta n_C sum_C |a| + 2 (n_C delta)^2], i.e. 3 x (3 / n) sum_C n_C sum_C |a| 2^-31 plus a second-order term.
    Phases cancel inside a cluster, so nothing relative to F holds.  The squares are then summed in double: at most 11 + 8 adds
    deep (8 per thread at the chain plan's bound, the tree of 10, the two halves), 32 ulp of the sum of the absolute terms."""
    n = len(a)
    first = sum(4.0 * DELTA * nC * float(sa) + 2.0 * (nC * DELTA) ** 2 for _, _, nC, sa in cluster_sums(L, a, labels, d).values())
    rounding = 32 * 2.0 ** -53 * sum(2.0 * float(sa) ** 2 for _, _, _, sa in cluster_sums(L, a, labels, d).values())
    return 3.0 * (first + rounding) / n
