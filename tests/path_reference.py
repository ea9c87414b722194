"""Plain extended-precision restatement of the 1-D path formulas (harmonic / quartic oscillator, topological rotor).  For
the tests only; the shapes and inputs of tests/test_path_splits_gpu.py are in tests/path_cases.py.

numpy in np.longdouble (x87 80-bit, eps = 2^-63), vectorised over chains with np.roll and written from the formulas, not
from any kernel's order of operations; tests/test_path_reference.py pins it to the oracle and to the survey's known
answers on the CPU.  Every function takes one path ([M]) or a batch ([B, M]) and returns long doubles.

With a = T_final / M, d_j = x_j - x_{j-1} (periodic):
  harmonic   S = (a m0 / 2) sum [ d^2 / a^2 + mu2 x^2 ]                                 harmonicoscillatoraction.cc:8-18
             dS/dx_j = (m0 / a) ((2 + a^2 mu2) x_j - x_{j-1} - x_{j+1})                  harmonicoscillatoraction.cc:21-35
  quartic    S = (a / 2) sum [ m0 (d^2 / a^2 + mu2 x^2) + (lambda / 2) (x - x0)^4 ]      quarticoscillatoraction.cc:7-27
             dS/dx_j = harmonic + a lambda (x_j - x0)^3                                  quarticoscillatoraction.cc:30-53
  rotor      S = (m0 / a) sum [ 1 - cos d ]                                              rotoraction.cc:9-18
             dS/dx_j = (m0 / a) (sin(x_j - x_{j-1}) + sin(x_j - x_{j+1}))                rotoraction.cc:59-79
  <x^2> = sum x^2 / M                                                                    qoixsquared.cc:7-20
  chi = Q^2 / (4 pi^2 T_final),  Q = sum mod_2pi(d)                                      qoisusceptibility.cc:8-23
  copy_from_fine: coarse_j = fine_{2j};  copy_from_coarse: fine_{2j} = coarse_j, odd sites untouched   qmaction.cc:7-24
  hierarchical two-level step: a chain whose mask is 0 (rejected further down) does not move, comes back rejected with
  three zero terms; any other chain is TwoLevelMetropolisStep::draw                      hierarchicalsampler.cc:62-76
  Statistics' packed sums per chain: [n, sum q, sum q^2, sum q^3, sum q^4]
"""
import numpy as np

from lattice_reference import LD, PI, mod_2pi


# ---- formulas --------------------------------------------------------------------------------------------------------------
def action(kind, p, x):
    x = np.asarray(x, dtype=LD)
    a, m0 = LD(p["T_final"]) / LD(p["M"]), LD(p.get("m0", 1.0))
    d = x - np.roll(x, 1, axis=-1)
    if kind == "rotor":
        return m0 / a * np.sum(1 - np.cos(d), axis=-1)
    mu2 = LD(p.get("mu2", 1.0))
    if kind == "harmonic":
        return a * m0 / 2 * np.sum(d * d / (a * a) + mu2 * x * x, axis=-1)
    lam, x0 = LD(p.get("lam", 0.0)), LD(p.get("x0", 0.0))
    return a / 2 * np.sum(m0 * (d * d / (a * a) + mu2 * x * x) + lam / 2 * ((x - x0) * (x - x0)) ** 2, axis=-1)


def force(kind, p, x):
    x = np.asarray(x, dtype=LD)
    a, m0 = LD(p["T_final"]) / LD(p["M"]), LD(p.get("m0", 1.0))
    xl, xr = np.roll(x, 1, axis=-1), np.roll(x, -1, axis=-1)
    if kind == "rotor":
        s = np.sin(x - xl)                      # sin(x_j - x_{j+1}) = -sin(d_{j+1})
        return m0 / a * (s - np.roll(s, -1, axis=-1))
    f = m0 / a * ((2 + a * a * LD(p.get("mu2", 1.0))) * x - xl - xr)
    if kind == "quartic":
        sh = x - LD(p.get("x0", 0.0))
        f = f + a * LD(p.get("lam", 0.0)) * (sh * sh * sh)
    return f


def xsquared(x):
    x = np.asarray(x, dtype=LD)
    return np.sum(x * x, axis=-1) / LD(x.shape[-1])


def winding(x):
    """Q = sum_j mod_2pi(x_j - x_{j-1}): 2 pi times an integer, up to rounding"""
    x = np.asarray(x, dtype=LD)
    return np.sum(mod_2pi(x - np.roll(x, 1, axis=-1)), axis=-1)


def susceptibility(x, T_final):
    Q = winding(x)
    return Q * Q / (4 * PI * PI * LD(T_final))


def distance_to_branch_cut(x):
    """min_j | |mod_2pi(d_j)| - pi |: how far the path is from a difference whose wrap depends on rounding"""
    x = np.asarray(x, dtype=LD)
    return np.min(np.abs(np.abs(mod_2pi(x - np.roll(x, 1, axis=-1))) - PI), axis=-1)


def copy_from_fine(fine):
    return np.array(np.asarray(fine)[..., ::2])


def copy_from_coarse(coarse, fine):
    out = np.array(fine)
    out[..., ::2] = coarse
    return out


def masked_twolevel_draw(F, Cc, x_coarse, theta, mask, seed, chain0, step):
    """One hierarchical two-level step on B chains with the oracle's actions F (fine) and Cc (coarse): theta [B, M] is
    updated in place, returns (accept [B] int32, terms [B, 3]).  Chain b is stream chain0 + b whatever the mask holds."""
    B = theta.shape[0]
    accept, terms = np.zeros(B, dtype=np.int32), np.zeros((B, 3))
    for b in range(B):
        if mask is None or mask[b]:
            accept[b], terms[b] = F.dev_twolevel_draw(Cc, x_coarse[b], theta[b], seed, chain0 + b, step)
    return accept, terms


def power_sums(series):
    """series [n, B] -> [B, 5]: n, sum q, sum q^2, sum q^3, sum q^4"""
    q = np.asarray(series, dtype=LD)
    return np.stack([np.full(q.shape[1], LD(q.shape[0]))] + [np.sum(q ** k, axis=0) for k in (1, 2, 3, 4)], axis=1)
