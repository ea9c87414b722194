"""numpy restatement of the cluster samplers (mlmcpathintegral_amd/csrc/cluster.hip): the contract's second statement.

(a) ref_update1d   ClusterSampler::single_cluster_update1d with RotorAction::{S_ell, flip} as the reference walks it
                   (flip the seed, walk forward link by link from the already flipped site, then backward), quirks at the
                   wrap-around included; the uniform of a link is injected, so the walk can be fed the device's numbers.
(b) dev_update     the device's statement: M independent bonds from the path BEFORE the update, the run of bonded links
                   around the seed site is reflected; a run that reaches all M sites flips all M once.
(c) schwinger_links  QuenchedSchwingerClusterSampler::draw's rebuild of the link field in sequential order, np.longdouble.

Random numbers, Philox (site, chain, step, purpose << 24) keyed by the seed:
  P_CLUSTER_REFLECT = 15  site 0, step = global update counter: xbar = 2 pi u - pi, i0 = min(floor(v M), M - 1)
  P_CLUSTER_BOND    = 16  site l >> 1, same step: u decides link l = (l, l + 1 mod M) for even l, v for odd l
  P_GAUGE           = 17  site vertex >> 1, vertex = Mt j + i, step = draw counter: g = 2 pi (u | v by parity) - pi
The plaquette path psi of the Schwinger sampler starts from the rotor's P_INIT uniforms on a path of M = Mt Mx sites.
"""
import math

import numpy as np

from sigma_model import uniforms

P_INIT, P_CLUSTER_REFLECT, P_CLUSTER_BOND, P_GAUGE = 6, 15, 16, 17
LD = np.longdouble


def mod_2pi(x):
    """common/auxilliary.hh:42-44, operation for operation"""
    return x - 2.0 * np.pi * np.floor(0.5 * (x + np.pi) / np.pi)


def reflection(seed, chain, step, M):
    """(xbar, i0) of update `step` of a chain"""
    u, v = uniforms(seed, chain, step, 0, P_CLUSTER_REFLECT)
    return 2.0 * np.pi * float(u) - np.pi, min(int(float(v) * M), M - 1)


def bond_uniforms(seed, chain, step, links):
    links = np.asarray(links, dtype=np.uint64)
    u, v = uniforms(seed, chain, step, links >> np.uint64(1), P_CLUSTER_BOND)
    return np.where(links & np.uint64(1), v, u)


def bond_probabilities(x, xbar, kappa2):
    """p_l of link l = (l, l + 1 mod M) from the path before the update; kappa2 = 2 m0 / a"""
    c = np.cos(x - xbar)
    return 1.0 - np.exp(np.minimum(0.0, -(kappa2 * c) * np.roll(c, -1)))


def flip(x, xbar):
    return mod_2pi(np.pi + 2.0 * xbar - x)


def run_of(bonded, i0):
    """(f, b): bonded links in a row forward from site i0 (links i0, i0 + 1, ...; at most M - 1) and backward (links
    i0 - 1, i0 - 2, ...; at most M - 1 - f: the sites of the run are distinct)"""
    M = len(bonded)
    f = 0
    while f < M - 1 and bonded[(i0 + f) % M]:
        f += 1
    b = 0
    while b < M - 1 - f and bonded[(i0 - 1 - b) % M]:
        b += 1
    return f, b


def dev_update(x, kappa2, seed, chain, step):
    """one update of one chain; returns (new path, info): sites flipped (in path order from the lower end of the run),
    f, b, xbar, i0 and `margin` = min |u - p| over the links whose test decided the run"""
    M = len(x)
    xbar, i0 = reflection(seed, chain, step, M)
    u = bond_uniforms(seed, chain, step, np.arange(M))
    p = bond_probabilities(x, xbar, kappa2)
    f, b = run_of(u < p, i0)
    sites = (i0 - b + np.arange(f + b + 1)) % M
    decided = [(i0 + k) % M for k in range(min(f + 1, M - 1))]
    if f < M - 1:
        decided += [(i0 - 1 - k) % M for k in range(min(b + 1, M - 1 - f))]
    decided = np.array(decided, dtype=int)
    out = x.copy()
    out[sites] = flip(x[sites], xbar)
    return out, {"sites": sites, "f": f, "b": b, "xbar": xbar, "i0": i0, "margin": float(np.min(np.abs(u[decided] - p[decided])))}


def dev_update_batch(x, kappa2, seed, chain0, step):
    """dev_update of every chain of x [B, M] at once (for long CPU chains on small rings); returns (new paths, run sizes)"""
    B, M = x.shape
    chain = (chain0 + np.arange(B, dtype=np.uint64))
    u, v = uniforms(seed, chain, step, 0, P_CLUSTER_REFLECT)
    xbar = 2.0 * np.pi * u - np.pi
    i0 = np.minimum((v * M).astype(np.int64), M - 1)
    ub = bond_uniforms(seed, chain[:, None], step, np.arange(M)[None, :])
    c = np.cos(x - xbar[:, None])
    bonded = ub < 1.0 - np.exp(np.minimum(0.0, -(kappa2 * c) * np.roll(c, -1, axis=1)))
    rows = np.arange(B)
    f = np.zeros(B, dtype=np.int64)
    going = np.ones(B, dtype=bool)
    for k in range(M - 1):
        going &= bonded[rows, (i0 + k) % M]
        f += going
    b = np.zeros(B, dtype=np.int64)
    going = np.ones(B, dtype=bool)
    for k in range(M - 1):
        going &= (k < M - 1 - f) & bonded[rows, (i0 - 1 - k) % M]
        b += going
    off = (np.arange(M)[None, :] - (i0 - b)[:, None]) % M       # position of each site counted from the run's lower end
    inside = off <= (f + b)[:, None]
    return np.where(inside, flip(x, xbar[:, None]), x), f + b + 1


def dev_draw(x, kappa2, seed, chain0, update0, n_updates):
    """mlmcpi_path_cluster_draw on [B, M]: returns (new paths, flipped sites per chain, min margin, longest run)"""
    out = np.array(x, dtype=np.float64, copy=True)
    count = np.zeros(out.shape[0], dtype=np.int64)
    margin, longest = np.inf, 0
    for b in range(out.shape[0]):
        for k in range(n_updates):
            out[b], info = dev_update(out[b], kappa2, seed, chain0 + b, update0 + k)
            count[b] += len(info["sites"])
            margin = min(margin, info["margin"])
            longest = max(longest, len(info["sites"]))
    return out, count, margin, longest


def ref_update1d(x, kappa2, xbar, i0, link_uniform):
    """clustersampler.cc:92-132; link_uniform(l) is the uniform drawn when the link l = (l, l + 1 mod M) is tested.
    Returns (new path, list of flipped sites in the order of the flips -- a site may appear twice at a wrap)"""
    x = np.array(x, dtype=np.float64, copy=True)
    M = len(x)
    flipped = []

    def do_flip(l):
        x[l] = mod_2pi(np.pi + 2.0 * xbar - x[l])
        flipped.append(l)

    def process_link(i, direction):
        nb = (i + direction + M) % M
        S_ell = -kappa2 * math.cos(x[i] - xbar) * math.cos(x[nb] - xbar)
        p_connect = 1.0 - math.exp(min(0.0, -S_ell))
        bonded = link_uniform(i if direction > 0 else nb) < p_connect
        if bonded:
            do_flip(nb)
        return bonded, nb

    do_flip(i0)
    i_p = i0
    while True:
        i_last_p = i_p
        bonded, i_p = process_link(i_p, +1)
        if not (i_p != i0 and bonded):
            break
    i_m = i0
    while True:
        bonded, i_m = process_link(i_m, -1)
        if not (i_m != i_last_p and bonded):
            break
    return x, flipped


# ---- quenched Schwinger ----------------------------------------------------------------------------------------------
def initial_path(B, N, seed, chain0=0):
    chain = (chain0 + np.arange(B, dtype=np.uint64))[:, None]
    u, _ = uniforms(seed, chain, 0, np.arange(N, dtype=np.uint64)[None, :], P_INIT)
    return -np.pi + 2.0 * np.pi * u


def gauge_angles(seed, chain, draw, Mt, Mx):
    """g[i, j] of one chain"""
    jj, ii = np.meshgrid(np.arange(Mx, dtype=np.uint64), np.arange(Mt, dtype=np.uint64), indexing="xy")  # [Mt, Mx]
    vertex = np.uint64(Mt) * jj + ii
    u, v = uniforms(seed, chain, draw, vertex >> np.uint64(1), P_GAUGE)
    return 2.0 * np.pi * np.where(vertex & np.uint64(1), v, u) - np.pi


def schwinger_links(psi, Mt, Mx, g=None):
    """quenchedschwingerclustersampler.cc:48-82 in the reference's order of additions, long double; psi [Mt Mx], g [Mt, Mx]
    or None; returns theta [2 Mt Mx] (entry 2 (Mt j + i) + mu), mod_2pi applied once at the end, in [-pi, pi]"""
    from lattice_reference import mod_2pi as mod_2pi_ld
    psi = np.asarray(psi, dtype=LD)
    N = Mt * Mx
    d = psi[1:] - psi[:-1]                                   # d[c], c <= N - 2
    t0 = np.zeros((Mt, Mx), dtype=LD)
    t1 = np.zeros((Mt, Mx), dtype=LD)
    # theta_1(i + 1, j) = theta_1(i, j) + d[i Mx + j], i < Mt - 1: np.cumsum adds in sequence
    t1[1:, :] = np.cumsum(d[:(Mt - 1) * Mx].reshape(Mt - 1, Mx), axis=0)
    # theta_0(Mt - 1, j + 1) = theta_0(Mt - 1, j) - theta_1(Mt - 1, j) - d[(Mt - 1) Mx + j], j < Mx - 1
    last = np.zeros(Mx, dtype=LD)
    acc = LD(0)
    for j in range(Mx - 1):
        acc = acc - t1[Mt - 1, j] - psi[(Mt - 1) * Mx + j + 1] + psi[(Mt - 1) * Mx + j]
        last[j + 1] = acc
    t0[Mt - 1, :] = last
    if g is not None:
        g = np.asarray(g, dtype=LD)
        t0 = t0 + g - np.roll(g, -1, axis=0)
        t1 = t1 + g - np.roll(g, -1, axis=1)
    theta = np.stack([t0.T, t1.T], axis=-1).reshape(2 * N)   # [Mx, Mt, 2]: entry 2 (Mt j + i) + mu
    return mod_2pi_ld(theta)


def rotor_action(psi, beta):
    """S of the closed plaquette path: beta sum (1 - cos(psi[c + 1] - psi[c])) (rotor with m0 / a = beta)"""
    psi = np.asarray(psi, dtype=LD)
    return LD(beta) * np.sum(1 - np.cos(np.roll(psi, -1) - psi))


# ---- exact values ------------------------------------------------------------------------------------------------------
def ring_link_energy(kappa, M, nmax=40):
    """<cos(x_{j+1} - x_j)> of the rotor ring, (1 / M) d ln Z / d kappa with Z = sum_n I_n(kappa)^M (character expansion),
    and, with `M - 1` powers, the average plaquette of the quenched Schwinger model on N = M cells"""
    from scipy.special import ive
    n = np.arange(-nmax, nmax + 1)
    I0 = ive(0, kappa)                                       # everything relative to I_0: no underflow of the M-th powers
    In = ive(n, kappa) / I0
    dIn = 0.5 * (ive(n - 1, kappa) + ive(n + 1, kappa)) / I0
    return float(np.sum(In ** (M - 1) * dIn) / np.sum(In ** M))
