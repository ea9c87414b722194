"""numpy model of the parallel random-order sweep (mlmcpathintegral_amd/csrc/random_sweep.hip): the order contract (Philox
purpose 18), the conflict stencils, the round schedule, and the local updates that need no sampler of their own
(overrelaxation of both stencils, GFF heat bath), applied one by one or a round at a time.

Order: index l of a chain takes word l & 3 of Philox (site l >> 2, chain, step, 18 << 24) as its 32-bit key; a sweep visits
the indices in ascending (key, l).  Round of an index = 1 + the largest round among its conflict neighbours that precede it."""
import numpy as np

import sigma_model as sm

P_SWEEP_ORDER, P_GFF_NORMAL = 18, 3
GFF, SCHWINGER, SIGMA = 3, 4, 5


def n_indices(kind, Mt, Mx):
    return (2 if kind == SCHWINGER else 1) * Mt * Mx


def keys(seed, chain, step, n):
    """the 32-bit keys of the n indices of (seed, chain, step)"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    r = sm.philox(q, chain, step, P_SWEEP_ORDER << 24, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(r, axis=1).reshape(-1)[:n].astype(np.uint32)


def order_of(key):
    """ascending (key, l)"""
    return np.lexsort((np.arange(key.size), key)).astype(np.uint32)


def neighbours(kind, Mt, Mx):
    """[n, 6 or 4] conflict neighbours: the links of a link's two staples, in the order the update reads them; a vertex's
    four neighbours +i, -i, +j, -j"""
    if kind == SCHWINGER:
        l = np.arange(2 * Mt * Mx)
        mu, v = l & 1, l >> 1
        j, i = v // Mt, v % Mt
        ip, im, jp, jm = (i + 1) % Mt, (i - 1) % Mt, (j + 1) % Mx, (j - 1) % Mx
        L = lambda a, c, m: 2 * (Mt * c + a) + m
        n0 = np.stack([L(i, jp, 0), L(i, j, 1), L(ip, j, 1), L(i, jm, 0), L(ip, jm, 1), L(i, jm, 1)], axis=1)
        n1 = np.stack([L(i, j, 0), L(ip, j, 1), L(i, jp, 0), L(im, jp, 0), L(im, j, 1), L(im, j, 0)], axis=1)
        return np.where((mu == 0)[:, None], n0, n1)
    l = np.arange(Mt * Mx)
    j, i = l // Mt, l % Mt
    ip, im, jp, jm = (i + 1) % Mt, (i - 1) % Mt, (j + 1) % Mx, (j - 1) % Mx
    return np.stack([Mt * j + ip, Mt * j + im, Mt * jp + i, Mt * jm + i], axis=1)


def rounds_of(key, nb):
    """round of every index, counted from 1, by the ready rule: iteration k takes the pending indices all of whose preceding
    conflict neighbours were done before it"""
    n = key.size
    l = np.arange(n)[:, None]
    kn, kl = key[nb], key[:, None]
    before = (kn < kl) | ((kn == kl) & (nb < l))
    rnd = np.zeros(n, dtype=np.uint32)
    k = 0
    while (rnd == 0).any():
        k += 1
        done = rnd != 0
        ready = ~done & (~before | done[nb]).all(axis=1)
        assert ready.any()
        rnd[ready] = k
    return rnd


def schedule(kind, Mt, Mx, seed, chain, step):
    """(order, rounds) of one chain's sweep"""
    key = keys(seed, chain, step, n_indices(kind, Mt, Mx))
    return order_of(key), rounds_of(key, neighbours(kind, Mt, Mx))


def mod_2pi(x):
    return x - 2 * np.pi * np.floor(0.5 * (x + np.pi) / np.pi)


def gff_normals(seed, chain, step, l):
    u, v = sm.uniforms(seed, chain, step, np.asarray(l, dtype=np.uint64) >> np.uint64(1), P_GFF_NORMAL)
    r, a = np.sqrt(-2.0 * np.log(np.maximum(u, 2.0 ** -53))), 2 * np.pi * v
    return np.where(np.asarray(l) & 1, r * np.sin(a), r * np.cos(a))


def update(kind, x, idx, nb, heat, normals=None, mu2=0.0):
    """the local update of the indices `idx` (an array: all at once, each from the values x holds now), in place.
    Schwinger / vertex-stencil overrelaxation and the GFF heat bath (normals[l] = the normal of index l)."""
    idx = np.atleast_1d(idx)
    if kind == SCHWINGER:
        assert not heat
        m = nb[idx]
        tp = x[m[:, 0]] + x[m[:, 1]] - x[m[:, 2]]
        tm = x[m[:, 3]] + x[m[:, 4]] - x[m[:, 5]]
        x[idx] = mod_2pi((tp + tm) - x[idx])
        return
    m = nb[idx]
    delta = ((x[m[:, 0]] + x[m[:, 1]]) + x[m[:, 2]]) + x[m[:, 3]]
    kappa = 4.0 + mu2
    x[idx] = delta / kappa + normals[idx] / np.sqrt(kappa) if heat else (2.0 / kappa) * delta - x[idx]


def sweep_sequential(kind, x, order, nb, heat, **kw):
    for l in order:
        update(kind, x, int(l), nb, heat, **kw)


def sweep_rounds(kind, x, rnd, nb, heat, **kw):
    for k in range(1, int(rnd.max()) + 1):
        update(kind, x, np.nonzero(rnd == k)[0], nb, heat, **kw)
