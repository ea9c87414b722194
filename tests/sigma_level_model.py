"""numpy restatement of the O(3) nonlinear sigma model on the levels of its CoarsenRotate hierarchy, of its conditioned fine
action and of the two-level Metropolis step (mlmcpathintegral_amd/csrc/sigma_levels.hip, sigma_twolevel.hip), built on
tests/sigma_model.py.  Everything is table driven: a Level holds the reference's index map, neighbour table (first four
columns of lattice2d.cc:137-155), fine-only list and fine2coarse map (lattice2d.cc:83-134), built here from the definitions and
pinned to the reference's own tables by tests/test_sigma_level_model.py.
"""
import numpy as np

import sigma_model as sm

P_SIGMA_FILLIN, P_ACCEPT2 = 24, 8


class Level:
    """(Mt, Mx, rotated): extents of the Cartesian frame, both even.  Rotated: the (i + j) even vertices, E plane then O plane."""

    def __init__(self, Mt, Mx, rotated, beta=1.0):
        assert Mt % 2 == 0 and Mx % 2 == 0 and Mt >= 2 and Mx >= 2
        self.Mt, self.Mx, self.rotated, self.beta = Mt, Mx, bool(rotated), beta
        self.n = Mt * Mx // 2 if rotated else Mt * Mx
        steps = [(1, 1), (1, -1), (-1, 1), (-1, -1)] if rotated else [(1, 0), (-1, 0), (0, 1), (0, -1)]
        self.coords = [self.lin2cart(l) for l in range(self.n)]
        self.nbr = np.array([[self.cart2lin(i + di, j + dj) for di, dj in steps] for i, j in self.coords], dtype=np.int64)
        if rotated:   # fine-only: odd-odd; coarse partner: unrotated (Mt / 2, Mx / 2), vertex (i, j) -> (i / 2, j / 2)
            self.fineonly = np.array([l for l, (i, j) in enumerate(self.coords) if i % 2 == 1], dtype=np.int64)
            pairs = [(l, (Mt // 2) * (j // 2) + i // 2) for l, (i, j) in enumerate(self.coords) if i % 2 == 0]
        else:         # fine-only: (i + j) odd; coarse partner: rotated (Mt, Mx), the same vertex
            self.fineonly = np.array([l for l, (i, j) in enumerate(self.coords) if (i + j) % 2 == 1], dtype=np.int64)
            pairs = [(l, rot_cart2lin(Mt, Mx, i, j)) for l, (i, j) in enumerate(self.coords) if (i + j) % 2 == 0]
        self.fine2coarse = np.array(pairs, dtype=np.int64)   # ascending in the fine index

    def cart2lin(self, i, j):
        if self.rotated:
            return rot_cart2lin(self.Mt, self.Mx, i, j)
        return self.Mt * (j % self.Mx) + i % self.Mt

    def lin2cart(self, l):
        if self.rotated:
            q, ht = self.Mt * self.Mx // 4, self.Mt // 2
            p, r = divmod(l, q)
            return 2 * (r % ht) + p, 2 * (r // ht) + p
        return l % self.Mt, l // self.Mt

    def coarse(self, beta=None):
        b = self.beta if beta is None else beta
        return Level(self.Mt // 2, self.Mx // 2, False, b) if self.rotated else Level(self.Mt, self.Mx, True, b)


def rot_cart2lin(Mt, Mx, i, j):
    """lattice2d.hh:230-268: vertex (2 a + p, 2 b + p) of the rotated lattice -> p Mt Mx / 4 + (Mt / 2) b + a"""
    assert (i + j) % 2 == 0
    p = i % 2
    return p * (Mt * Mx // 4) + (Mt // 2) * (((j - p) // 2) % (Mx // 2)) + ((i - p) // 2) % (Mt // 2)


def spins(L, phi):
    """[B, 2 n] -> [B, n, 3]"""
    return sm.sigma_of(phi.reshape(phi.shape[0], L.n, 2))


def delta(L, sig):
    """sum of the four neighbours in the reference's order, ((a + b) + c) + d"""
    return ((sig[:, L.nbr[:, 0]] + sig[:, L.nbr[:, 1]]) + sig[:, L.nbr[:, 2]]) + sig[:, L.nbr[:, 3]]


def initialise(L, B, seed, chain0=0):
    chain = (chain0 + np.arange(B, dtype=np.uint64))[:, None]
    u, _ = sm.uniforms(seed, chain, 0, np.arange(2 * L.n, dtype=np.uint64)[None, :], sm.P_INIT)
    out = np.empty((B, 2 * L.n))
    out[:, 0::2] = np.arccos(1.0 - 2.0 * u[:, 0::2])
    out[:, 1::2] = -np.pi + 2.0 * np.pi * u[:, 1::2]
    return out


def evaluate(L, phi):
    """S = -1/2 beta sum_n sigma_n . Delta_n (nonlinearsigmaaction.cc:7-21)"""
    sig = spins(L, phi)
    return -0.5 * L.beta * np.einsum("bnc,bnc->b", sig, delta(L, sig))


def magnetic_susceptibility(L, phi):
    m = spins(L, phi).sum(axis=1)
    return (m * m).sum(axis=-1) / L.n


def unit_vectors(L, phi):
    return spins(L, phi)


def _update(L, phi, sites, heat, seed, chain0, step, purpose=sm.P_SIGMA_HB):
    """heat-bath (or overrelaxation) update of the mutually non-adjacent vertices `sites`, all at once"""
    B = phi.shape[0]
    a = phi.reshape(B, L.n, 2).copy()
    sig = sm.sigma_of(a)
    D = delta(L, sig)[:, sites]
    if heat:
        chain = (chain0 + np.arange(B, dtype=np.uint64))[:, None]
        u, v = sm.uniforms(seed, chain, step, sites.astype(np.uint64)[None, :], purpose)
        new = sm.heatbath(sig[:, sites], D, L.beta, u, v)
    else:
        new = sm.overrelax(sig[:, sites], D)
    a[:, sites] = sm.angles_of(new)
    return a.reshape(B, 2 * L.n)


def sweep(L, phi, heat, seed=0, chain0=0, step=0):
    """one sweep: rotated: phase E then phase O; unrotated: (i + j) even then odd"""
    if L.rotated:
        halves = [np.arange(L.n // 2), np.arange(L.n // 2, L.n)]
    else:
        par = np.array([(i + j) % 2 for i, j in L.coords])
        halves = [np.nonzero(par == 0)[0], np.nonzero(par == 1)[0]]
    for s in halves:
        phi = _update(L, phi, s, heat, seed, chain0, step)
    return phi


def sweep_draw(L, phi, n_or, n_hb, seed=0, chain0=0, sweep0=0):
    for s in range(n_or + n_hb):
        phi = sweep(L, phi, s >= n_or, seed, chain0, sweep0 + s)
    return phi


def copy_from_fine(L, fine):
    """state on L -> state on L.coarse()"""
    B = fine.shape[0]
    out = np.zeros((B, len(L.fine2coarse), 2))
    out[:, L.fine2coarse[:, 1]] = fine.reshape(B, L.n, 2)[:, L.fine2coarse[:, 0]]
    return out.reshape(B, -1)


def copy_from_coarse(L, coarse, fine):
    B = fine.shape[0]
    out = fine.reshape(B, L.n, 2).copy()
    out[:, L.fine2coarse[:, 0]] = coarse.reshape(B, -1, 2)[:, L.fine2coarse[:, 1]]
    return out.reshape(B, 2 * L.n)


def cfa_fill(L, phi, seed, chain0, step):
    """fill_fine_points: every fine-only vertex from its four (coarse) neighbours, one Philox call of purpose 24 each"""
    return _update(L, phi, L.fineonly, True, seed, chain0, step, P_SIGMA_FILLIN)


def log_density(z, s):
    """log p(z; s), p = s exp(s z) / (2 sinh s): s (z - 1) + log s - log(1 - exp(-2 s)); log 1/2 at s = 0"""
    z, s = np.broadcast_arrays(np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64))
    pos = s > 0
    ss = np.where(pos, s, 1.0)
    return np.where(pos, (ss * (z - 1.0) + np.log(ss)) - np.log(-np.expm1(-2.0 * ss)), np.log(0.5))


def cfa_evaluate(L, phi):
    sig = spins(L, phi)
    D = delta(L, sig)[:, L.fineonly]
    nrm = np.sqrt(D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2])
    d = D / np.where(nrm > 0, nrm, 1.0)[..., None]
    s0 = sig[:, L.fineonly]
    z = s0[..., 0] * d[..., 0] + s0[..., 1] * d[..., 1] + s0[..., 2] * d[..., 2]
    return -log_density(z, L.beta * nrm).sum(axis=1)


def decimation_F(L, phi):
    """F(theta_C) = sum_X log(2 sinh s_X / s_X), s_X = beta |Delta_X|: the exact decimation of the fine-only vertices"""
    D = delta(L, spins(L, phi))[:, L.fineonly]
    s = L.beta * np.sqrt((D * D).sum(axis=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s > 0, s + np.log(-np.expm1(-2.0 * s)) - np.log(np.where(s > 0, s, 1.0)), np.log(2.0))
    return f.sum(axis=1)


def twolevel_draw(L, Lc, phi_coarse, theta, seed, chain0, step, always_accept=False):
    """TwoLevelMetropolisStep::draw: returns (new theta, accept, terms [B, 3], trial, margin = u - exp(-dS))"""
    B = theta.shape[0]
    trial = cfa_fill(L, copy_from_coarse(L, phi_coarse, theta), seed, chain0, step)
    dS_fine = evaluate(L, trial) - evaluate(L, theta)
    dS_coarse = evaluate(Lc, copy_from_fine(L, theta)) - evaluate(Lc, phi_coarse)
    dS_trial = cfa_evaluate(L, theta) - cfa_evaluate(L, trial)
    dS = dS_fine + dS_coarse + dS_trial
    chain = chain0 + np.arange(B, dtype=np.uint64)
    u, _ = sm.uniforms(seed, chain, step, np.zeros(B, dtype=np.uint64), P_ACCEPT2)
    thr = np.exp(-dS)
    accept = (dS < 0) | (u < thr)
    if always_accept:
        accept = np.ones(B, dtype=bool)
    margin = np.where(dS < 0, np.inf, np.abs(u - thr))
    new = np.where(accept[:, None], trial, theta)
    return new, accept, np.stack([dS_fine, dS_coarse, dS_trial], axis=1), trial, margin
