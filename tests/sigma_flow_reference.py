"""numpy restatement of the gradient flow of the O(3) sigma model on a level of its CoarsenRotate hierarchy and of the flowed
charge, susceptibility and energy by step count (mlmcpathintegral_amd/csrc/sigma_flow.hip; include/mlmcpi_hip.h:
mlmcpi_sigma_level_flowed_charge), once in longdouble (the reference) and once in float64 (the yardstick of how far float64
arithmetic of this very definition strays from it).

    sigma^0 = sigma_of(angles)
    F(Y)_l  = Delta_l - (Y_l . Delta_l) Y_l,  Delta_l = ((Y_0 + Y_1) + Y_2) + Y_3 over the neighbour table of
              sigma_cooling_reference.neighbours,  a . b = (x x' + y y') + z z'
    one step of size eps, all sites at once from the previous stage's Y, starting from A = 0, Y = sigma:
              A <- a_i A + eps F(Y),  Y <- Y + b_i A,  i = 1, 2, 3,  a = (0, -17/32, -32/27),  b = (1/4, 8/9, 3/4)
              sigma <- Y / |Y|,  |Y| = sqrt((x^2 + y^2) + z^2), three divisions; stage values are not normalised
    step count s = the field after s steps, flow time t = s eps
    Q_s, chi_s = Q_s^2 / n, E_s: sigma_cooling_reference.charge_of and .energy on sigma^s

eps is the float64 the device is handed, in either precision.  The neighbours, the charge and the energy are those of the
cooling and topology models, not rewritten.  The result of a step count does not depend on which others are listed: the model
steps one by one and measures where asked.  `project_stages=True` normalises after EVERY stage: not the definition, the control
of the order test (it is second order, the definition third).

TOLERANCES of the device comparison (tests/test_sigma_flow_gpu.py) are those of sigma_cooling_reference.py, for the same
reasons: vectors within tau = 8 max(dev64, 2^-50) with dev64 the float64 model's own distance from the longdouble model on that
very input and step count (a step is the same kind and number of operations in the float64 model and on the device: additions,
multiplications, one square root and three divisions, all correctly rounded on both, so the device differs from the float64
model only through its 2-ulp sincos at step 0 and its atan2 on the way out, which the factor 8 covers as it does for cooling; the
three stages compound in dev64 itself); Q within (12 tau + 256 eps) weight and E within n (7 tau + 96 eps), as derived there."""
import functools
import json
import os

import numpy as np

import sigma_cooling_reference as cool
import sigma_topology_reference as topo

LD = np.longdouble
MIN_NORM = 0.5
MIN_MARGIN = topo.MIN_MARGIN
MAX_EPS = 0.25
RECORDS = os.environ.get("MLMCPI_SIGMA_FLOW_RECORDS")


def record(file, name, payload):
    """keep a run's figures in the directory MLMCPI_SIGMA_FLOW_RECORDS names, if set (profiles/sigma_flow*.json are such runs)"""
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        path = os.path.join(RECORDS, file)
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = payload
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


def coefficients(dtype):
    """[(a_i, b_i)] rounded once in dtype"""
    t = dtype
    return [(t(0), t(1) / t(4)), (t(-17) / t(32), t(8) / t(9)), (t(-32) / t(27), t(3) / t(4))]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def force(Y, nbr):
    D = cool.delta(Y, nbr)
    return D - dot(Y, D)[..., None] * Y


def norm(Y):
    return np.sqrt((Y[..., 0] * Y[..., 0] + Y[..., 1] * Y[..., 1]) + Y[..., 2] * Y[..., 2])


def step(sig, nbr, eps, project_stages=False):
    """one step; returns (the new field, min |Y| over its normalisations)"""
    t = sig.dtype.type
    e, Y, A, least = t(eps), sig, np.zeros_like(sig), np.inf
    for k, (a, b) in enumerate(coefficients(t)):
        A = a * A + e * force(Y, nbr)
        Y = Y + b * A
        if project_stages or k == 2:
            nrm = norm(Y)
            least = min(least, float(nrm.min()))
            Y = Y / nrm[..., None]
    return Y, least


class Flowed(cool.Cooled):
    """the model at the listed step counts: the fields of sigma_cooling_reference.Cooled (Q, chi, E, margin, weight, dev64, sig and
    the bounds built on them), `depths` holding the step counts, and min_norm = min |Y| over every normalisation"""

    def __init__(self, n, steps, eps):
        super().__init__(n, steps)
        self.eps, self.min_norm = eps, np.inf


def flow(Mt, Mx, rotated, phi, eps, steps, with_float64=True, project_stages=False, chunk=1 << 21):
    """the definition for every chain of phi [B, 2 n] at the ascending list `steps`"""
    steps = list(steps)
    assert steps == sorted(set(steps)) and steps[0] >= 0
    assert np.isfinite(eps) and 0 < eps <= MAX_EPS
    n = cool.n_vertices(Mt, Mx, rotated)
    assert phi.ndim == 2 and phi.shape[1] == 2 * n, (phi.shape, n)
    nbr = cool.neighbours(Mt, Mx, rotated)
    per = max(1, chunk // n)
    parts = []
    for b0 in range(0, phi.shape[0], per):
        out = Flowed(n, steps, eps)
        sig = cool.sigma_of(phi[b0:b0 + per], n, LD)
        s64 = cool.sigma_of(phi[b0:b0 + per], n, np.float64) if with_float64 else None
        done = 0
        for s in steps:
            while done < s:
                sig, least = step(sig, nbr, eps, project_stages)
                out.min_norm = min(out.min_norm, least)
                if with_float64:
                    s64, _ = step(s64, nbr, eps, project_stages)
                done += 1
            c = cool.charge_of(Mt, Mx, rotated, sig)
            out.Q.append(c.Q)
            out.margin.append(c.margin)
            out.weight.append(c.weight)
            out.E.append(cool.energy(sig, nbr))
            out.dev64.append(float(np.abs(s64.astype(LD) - sig).max()) if with_float64 else 0.0)
        out.sig = sig
        parts.append(out.finish())
    if len(parts) == 1:
        return parts[0]
    out = Flowed(n, steps, eps)
    for k in ("Q", "E", "margin", "weight", "chi", "sig"):
        setattr(out, k, np.concatenate([getattr(p, k) for p in parts], axis=0))
    out.dev64 = np.max([p.dev64 for p in parts], axis=0)
    out.min_norm = min(p.min_norm for p in parts)
    return out


def level_flow(L, phi, eps, steps, **kw):
    return flow(L.Mt, L.Mx, L.rotated, phi, eps, steps, **kw)


def flow_scale(times, tE, c):
    """the flow time at which t <E> / n, given as tE at the ascending `times`, first crosses c, by linear interpolation; NaN where
    no neighbouring pair brackets c (include/mlmcpi/correlator.hh flow_scale)"""
    for k in range(len(times) - 1):
        lo, hi = tE[k], tE[k + 1]
        if (lo <= c <= hi or hi <= c <= lo) and lo != hi:
            return times[k] + (times[k + 1] - times[k]) * (c - lo) / (hi - lo)
    return float("nan")


# ---- the instanton and dislocation tables --------------------------------------------------------------------------------------
TABLE_EPS = 0.05
INSTANTON_STEPS = list(range(0, 41, 4))            # t = 0, 0.2, .., 2
INSTANTON_CASES = [(16, 16, 3.0, 1), (16, 16, 3.0, 2)]   # (Mt, Mx, lambda, k)
DISLOCATION = (4, 4, 1.0, 1)
DISLOCATION_STEPS = list(range(0, 32))             # the first step count at which round(Q) = 0 lies inside, both layouts
# that step count by layout (rotated?), as the longdouble model measures it (tests/test_sigma_flow_reference.py; recorded in
# profiles/sigma_flow.json): the dislocation keeps Q = 1 to t = 0.45 on the plain level and to t = 0.2 on the rotated one
DISLOCATION_LOSS_STEP = {False: 10, True: 5}


@functools.lru_cache(maxsize=None)
def instanton_table(Mt, Mx, rotated, lam, k, steps):
    """(Q [len(steps)], E / 4 pi [len(steps)]) of the discretised instanton at eps = TABLE_EPS, float64 of the longdouble model"""
    c = flow(Mt, Mx, rotated, topo.instanton(Mt, Mx, rotated, lam, k), TABLE_EPS, list(steps), with_float64=False)
    four_pi = 4 * np.arctan2(LD(0), LD(-1))
    return c.Q[0].astype(np.float64), (c.E[0] / four_pi).astype(np.float64)


def charge_loss_step(Q):
    """the first listed position at which round(Q) = 0 and stays 0"""
    r = np.rint(Q)
    assert r[-1] == 0, Q
    k = len(r) - 1
    while k > 0 and r[k - 1] == 0:
        k -= 1
    return k


# ---- the inputs of the GPU comparisons (tests/test_sigma_flow_gpu.py) ---------------------------------------------------------------
# Uniform random spins, the seed chosen as sigma_topology_reference.gpu_case chooses it: the first of seed0, seed0 + 1, .. for
# which the reference itself finds min |Y| >= MIN_NORM at every normalisation and the charge margin >= MIN_MARGIN at every listed
# step count, in BOTH runs of the case (tests/test_sigma_flow_reference.py asserts both for every case).  No case is dropped to
# meet the conditions.
RUNS = [(0.05, [0, 1, 2, 3, 7, 10]), (0.25, [0, 4])]   # (eps, steps) of every parity case
EDGE_RUN = (0.05, [0, 2])
EDGE_SHAPE, EDGE_CHAINS = (2, 2), 65581
EDGE_PINNED = [0, 1, 255, 65534, 65535, 65580]     # the chains of the edge case compared against the model
SMALL_SHAPES, SMALL_CHAINS = [(2, 2), (2, 6), (6, 4), (18, 10)], [3, 300]
LARGE_SHAPES, LARGE_CHAINS = [(66, 34), (130, 70)], [3]
SEEDS = {}


def parity_cases():
    keys = [(Mt, Mx, rot, B) for Mt, Mx in SMALL_SHAPES for rot in (False, True) for B in SMALL_CHAINS]
    return keys + [(Mt, Mx, rot, B) for Mt, Mx in LARGE_SHAPES for rot in (False, True) for B in LARGE_CHAINS]


def gpu_cases():
    return parity_cases() + [EDGE_SHAPE + (rot, EDGE_CHAINS) for rot in (False, True)]


def case_runs(key):
    return [EDGE_RUN] if key[3] == EDGE_CHAINS else RUNS


@functools.lru_cache(maxsize=None)
def gpu_input(Mt, Mx, rotated, B):
    phi = topo.uniform_spins(Mt, Mx, rotated, B, SEEDS[(Mt, Mx, rotated, B)])
    phi.setflags(write=False)
    return phi


def _models(key, phi, with_float64=True):
    sub = phi[EDGE_PINNED] if key[3] == EDGE_CHAINS else phi
    return [flow(*key[:3], sub, eps, steps, with_float64=with_float64) for eps, steps in case_runs(key)]


@functools.lru_cache(maxsize=None)
def gpu_case(Mt, Mx, rotated, B):
    """(phi [B, 2 n] float64, [Flowed per run of case_runs]) of a comparison's input; computed once per session and shared, never
    written to.  The edge case carries the model of its EDGE_PINNED chains only."""
    phi = gpu_input(Mt, Mx, rotated, B)
    return phi, _models((Mt, Mx, rotated, B), phi)


def conditions(c):
    return c.min_norm >= MIN_NORM and float(c.margin.min()) >= MIN_MARGIN


# `python tests/sigma_flow_reference.py` prints this table
SEEDS.update({
    (2, 2, False, 3): 302020, (2, 2, False, 300): 30002020, (2, 2, True, 3): 302025, (2, 2, True, 300): 30002025,
    (2, 6, False, 3): 302060, (2, 6, False, 300): 30002060, (2, 6, True, 3): 302065, (2, 6, True, 300): 30002065,
    (6, 4, False, 3): 306040, (6, 4, False, 300): 30006040, (6, 4, True, 3): 306045, (6, 4, True, 300): 30006045,
    (18, 10, False, 3): 318100, (18, 10, False, 300): 30018101, (18, 10, True, 3): 318105, (18, 10, True, 300): 30018105,
    (66, 34, False, 3): 366340, (66, 34, True, 3): 366345, (130, 70, False, 3): 430700, (130, 70, True, 3): 430705,
    (2, 2, False, 65581): 6558102020, (2, 2, True, 65581): 6558102025,
})


if __name__ == "__main__":
    for key in gpu_cases():
        seed = topo._seed0(*key)
        while not all(conditions(c) for c in _models(key, topo.uniform_spins(*key, seed), with_float64=False)):
            seed += 1
        print(f"    {key}: {seed},", flush=True)
