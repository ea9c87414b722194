"""numpy restatement of the Wolff single-cluster update of the O(3) sigma model on a level of its CoarsenRotate hierarchy
(mlmcpathintegral_amd/csrc/sigma_cluster.hip): the contract's second statement.

An unrotated Level calls through to tests/sigma_cluster_model.py, so that the two stay one definition.  A rotated Level is
table driven from sigma_level_model.Level (L.nbr, L.n): n = Mt Mx / 2 vertices, plane E (indices < n / 2) then plane O.  The
level is bipartite, so every link has exactly one E end: the 2 n links are (e, d), e an E vertex, d its direction in the order of
L.nbr (E(a, b) -> O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1)).  Seen from an O vertex, direction d' (O(a, b) -> E(a+1, b+1), E(a+1, b),
E(a, b+1), E(a, b)) crosses link (L.nbr[x, d'], 3 - d').  Where a plane extent is 1 several neighbours of a vertex coincide: they
are distinct links with a uniform each.

Random numbers, Philox (site, chain, step, purpose << 24 | sub) keyed by the seed, step = update counter:
  P_SIGMA_REFLECT = 19  site 0: sub 0 (u, v) -> normal r, r_z = 1 - 2 u, azimuth 2 pi v - pi; sub 1 u -> seed vertex
                        min(floor(u n), n - 1)
  P_SIGMA_BOND    = 20  site e, sub d >> 1: u decides link (e, d) for d even, v for d odd
With a_l = r . sigma_l before the update, link (x, y) is bonded iff its uniform < 1 - exp(min(0, -(2 beta (a_x a_y)))).

(a) walk_update   ClusterSampler::single_cluster_update (sampler/clustersampler.cc:52-89) over the four neighbours of L.nbr,
                  flip on joining, S_ell on the current state, a queue; the uniform of a link is injected.
(b) dev_update    the device's statement: 2 n independent bonds from the field BEFORE the update, the connected component
                  of the seed vertex is reflected.
"""
import math
from collections import deque

import numpy as np

import sigma_cluster_model as scm
from sigma_cluster_model import P_SIGMA_BOND, _dots, reflection
from sigma_model import angles_of, sigma_of, uniforms


def plane_task(L, x, d):
    """the kernel's plane arithmetic for task (x, d) of a rotated level: (neighbour, link site e, link direction)"""
    ht, hx = L.Mt // 2, L.Mx // 2
    q = ht * hx
    odd = x >= q
    c = x - q if odd else x
    b, a = divmod(c, ht)
    if odd:      # O(a, b) -> E(a + 1 - (d >> 1), b + 1 - (d & 1))
        ya = a if d & 2 else (a + 1) % ht
        yb = b if d & 1 else (b + 1) % hx
        y = yb * ht + ya
        return y, y, 3 - d
    ya = (a - 1) % ht if d & 2 else a
    yb = (b - 1) % hx if d & 1 else b
    return q + yb * ht + ya, x, d


def link_tables(L):
    """(site [n, 4], which [n, 4]) from L.nbr: direction d of vertex x crosses link (site[x, d], which[x, d])"""
    assert L.rotated
    nE = L.n // 2
    x = np.arange(L.n)[:, None]
    d = np.arange(4)[None, :]
    east = x < nE
    return np.where(east, x, L.nbr), np.where(east, d, 3 - d)


def link_uniforms(seed, chain, step, nE):
    """U [nE, 4]: the uniform of link (e, d)"""
    e = np.arange(nE, dtype=np.uint64)
    u0, v0 = uniforms(seed, chain, step, e, P_SIGMA_BOND, 0)
    u1, v1 = uniforms(seed, chain, step, e, P_SIGMA_BOND, 1)
    return np.stack([u0, v0, u1, v1], axis=-1)


def _bonds(L, a, U):
    """(bonded [.., nE, 4], p, prod) of the links (e, d) from a = r . sigma before the update"""
    nE = L.n // 2
    prod = a[..., :nE, None] * a[..., L.nbr[:nE]]
    p = 1.0 - np.exp(np.minimum(0.0, -(2.0 * L.beta * prod)))
    return (prod > 0.0) & (U < p), p, prod


def dev_update(L, phi, seed, chain, step):
    """one update of one chain phi [2 n] on the level L (L.beta); returns (new state, info): `sites` the flipped vertices
    (ascending), r, seed and `margin` = min |u - p| over the links with an end in the cluster whose test could go either way"""
    if not L.rotated:
        return scm.dev_update(phi, L.Mt, L.Mx, L.beta, seed, chain, step)
    n, nE = L.n, L.n // 2
    site, which = link_tables(L)
    ang = np.asarray(phi, dtype=np.float64).reshape(n, 2)
    sig = sigma_of(ang)
    r, s0 = reflection(seed, chain, step, n)
    a = _dots(sig, r)
    U = link_uniforms(seed, chain, step, nE)
    bonded, p, prod = _bonds(L, a, U)
    member = np.zeros(n, dtype=bool)
    member[s0] = True
    frontier = np.array([s0])
    while frontier.size:
        cand = []
        for d in range(4):
            y = L.nbr[frontier, d]
            cand.append(y[bonded[site[frontier, d], which[frontier, d]] & ~member[y]])
        frontier = np.unique(np.concatenate(cand))
        member[frontier] = True
    sites = np.nonzero(member)[0]
    touched = (member[:nE, None] | member[L.nbr[:nE]]) & (prod > 0.0)
    margin = float(np.min(np.abs(U - p)[touched])) if touched.any() else np.inf
    out = ang.copy()
    out[sites] = angles_of(sig[sites] - (2.0 * a[sites])[:, None] * r[None, :])
    return out.reshape(2 * n), {"sites": sites, "r": r, "seed": s0, "margin": margin}


def dev_update_batch(L, phi, seed, chain0, step):
    """dev_update of every chain of phi [B, 2 n] at once: the component by propagating membership along bonded links until
    nothing changes; returns (new states, cluster sizes)"""
    if not L.rotated:
        return scm.dev_update_batch(phi, L.Mt, L.Mx, L.beta, seed, chain0, step)
    B, n, nE = phi.shape[0], L.n, L.n // 2
    site, which = link_tables(L)
    ang = phi.reshape(B, n, 2)
    sig = sigma_of(ang)
    chain = chain0 + np.arange(B, dtype=np.uint64)
    u, v = uniforms(seed, chain, step, 0, scm.P_SIGMA_REFLECT, 0)
    us, _ = uniforms(seed, chain, step, 0, scm.P_SIGMA_REFLECT, 1)
    rz = 1.0 - 2.0 * u
    rho = np.sqrt(np.maximum(0.0, 1.0 - rz * rz))
    az = 2.0 * np.pi * v - np.pi
    r = np.stack([rho * np.cos(az), rho * np.sin(az), rz], axis=1)                       # [B, 3]
    s0 = np.minimum((us * n).astype(np.int64), n - 1)
    a = (r[:, None, 0] * sig[..., 0] + r[:, None, 1] * sig[..., 1]) + r[:, None, 2] * sig[..., 2]
    e = np.arange(nE, dtype=np.uint64)[None, :]
    u0, v0 = uniforms(seed, chain[:, None], step, e, P_SIGMA_BOND, 0)
    u1, v1 = uniforms(seed, chain[:, None], step, e, P_SIGMA_BOND, 1)
    bonded, _, _ = _bonds(L, a, np.stack([u0, v0, u1, v1], axis=-1))                     # [B, nE, 4]
    member = np.zeros((B, n), dtype=bool)
    member[np.arange(B), s0] = True
    while True:
        grown = member.copy()
        for d in range(4):
            grown |= member[:, L.nbr[:, d]] & bonded[:, site[:, d], which[:, d]]
        if np.array_equal(grown, member):
            break
        member = grown
    new = angles_of(sig - (2.0 * a)[..., None] * r[:, None, :])
    return np.where(member[..., None], new, ang).reshape(B, 2 * n), member.sum(axis=1)


def dev_draw(L, phi, seed, chain0, update0, n_updates):
    """mlmcpi_sigma_level_cluster_draw on [B, 2 n]: returns (new states, flipped vertices per chain, min margin)"""
    if not L.rotated:
        return scm.dev_draw(phi, L.Mt, L.Mx, L.beta, seed, chain0, update0, n_updates)
    out = np.array(phi, dtype=np.float64, copy=True)
    count = np.zeros(out.shape[0], dtype=np.int64)
    margin = np.inf
    for b in range(out.shape[0]):
        for k in range(n_updates):
            out[b], info = dev_update(L, out[b], seed, chain0 + b, update0 + k)
            count[b] += len(info["sites"])
            margin = min(margin, info["margin"])
    return out, count, margin


def walk_update(L, phi, r, s0, link_uniform):
    """clustersampler.cc:52-89 on one chain phi [2 n] over the four neighbours of L.nbr; link_uniform(ell, k, nb) is the uniform
    drawn when the walk tests the link from vertex ell to its k-th neighbour nb.  Returns (new state, flipped vertices in the
    order of the flips)."""
    if not L.rotated:
        return scm.walk_update(phi, L.Mt, L.Mx, L.beta, r, s0, link_uniform)
    x = np.array(phi, dtype=np.float64, copy=True)

    def r_sigma(l):
        th, ph = x[2 * l], x[2 * l + 1]
        return r[0] * math.sin(th) * math.cos(ph) + r[1] * math.sin(th) * math.sin(ph) + r[2] * math.cos(th)

    def flip(l):
        th, ph = x[2 * l], x[2 * l + 1]
        s = np.array([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
        s = s - 2.0 * float(s @ r) * r
        x[2 * l + 1] = math.atan2(s[1], s[0])
        x[2 * l] = math.atan2(math.sqrt(s[0] * s[0] + s[1] * s[1]), s[2])

    cluster, flipped, active = {s0}, [s0], deque([s0])
    flip(s0)
    while active:
        ell = active.popleft()
        for k in range(4):
            y = int(L.nbr[ell, k])
            if y in cluster:
                continue
            S_ell = -2.0 * L.beta * r_sigma(ell) * r_sigma(y)
            if link_uniform(ell, k, y) < 1.0 - math.exp(min(0.0, -S_ell)):
                flip(y)
                cluster.add(y)
                flipped.append(y)
                active.append(y)
    return x, flipped


def walk_with_device_uniforms(L, phi, seed, chain, step):
    """the four-neighbour walk fed with the link-keyed uniforms of the device rule"""
    if not L.rotated:
        return scm.walk_with_device_uniforms(phi, L.Mt, L.Mx, L.beta, seed, chain, step)
    site, which = link_tables(L)
    U = link_uniforms(seed, chain, step, L.n // 2)
    r, s0 = reflection(seed, chain, step, L.n)
    return walk_update(L, phi, r, s0, lambda ell, k, y: U[site[ell, k], which[ell, k]])
