"""The launch plan of path_hmc.hip restated, and the cases of tests/test_path_hmc_plan.py and
tests/test_path_hmc_geometry_gpu.py with the geometry each is meant to reach.  Everything here is decided without a device.

The rule, from the comment above plan_hmc (path_hmc.hip):

  register-resident   the whole periodic path in one workgroup when M = NT * R with NT a multiple of 64, R in
                      {16, 8, 4, 2, 1} (the rotor: R <= 8), NT <= 512 for R >= 8 and <= 1024 otherwise.  Of the R that fit,
                      the largest with B * NT / 64 >= 2048 waves (it still fills the chip); if none does, the one with the
                      most threads.  nseg = 1, owned_len = M, halo = 0.
  segmented           otherwise: buffers of L = NT * R = 4096 sites (R = 16, NT = 256; the rotor R = 8, NT = 512) whose first
                      and last halo = nt + 1 sites are recomputed copies of the neighbouring segments; L = 1024 (R = 4,
                      NT = 256) where M + 2 halo <= 1024.  A buffer must own at least 64 sites: 2 halo + 64 > L is refused.
                      nseg = ceil(M / (L - 2 halo)) segments of owned_len = ceil(M / nseg) sites, the last one shorter.
"""
import functools

import numpy as np

from path_cases import KINDS, SEED, params

OK, ERR_INVALID = 0, -1
FIELDS = ("R", "NT", "nseg", "owned_len", "halo", "chain_major")


def plan(kind, M, B, nt):
    """(status, {R, NT, nseg, owned_len, halo, chain_major} or None) for kind in KINDS"""
    if M < 2 or B < 1:                       # check_action, and the entry points' own argument check
        return ERR_INVALID, None
    fits = []
    for R in (16, 8, 4, 2, 1):
        if R > (8 if kind == "rotor" else 16) or M % R:
            continue
        NT = M // R
        if NT % 64 == 0 and 64 <= NT <= (512 if R >= 8 else 1024):
            fits.append((R, NT))
    if fits:
        filling = [f for f in fits if B * (f[1] // 64) >= 2048]
        R, NT = filling[0] if filling else max(fits, key=lambda f: f[1])
        return OK, dict(R=R, NT=NT, nseg=1, owned_len=M, halo=0, chain_major=1)
    halo = nt + 1
    R, NT = (8, 512) if kind == "rotor" else (16, 256)
    if M + 2 * halo <= 1024:
        R, NT = 4, 256
    L = R * NT
    if 2 * halo + 64 > L:
        return ERR_INVALID, None
    nseg = -(-M // (L - 2 * halo))
    return OK, dict(R=R, NT=NT, nseg=nseg, owned_len=-(-M // nseg), halo=halo, chain_major=0)


def owned_ranges(p, M):
    """[(lo, hi)) of global sites each segment of a plan owns (hmc_trajectory_kernel: o0 = seg * owned_len, olen = min(owned_len, M - o0))"""
    return [(s * p["owned_len"], min(M, (s + 1) * p["owned_len"])) for s in range(p["nseg"])]


GRID_M = list(range(1, 71)) + list(range(128, 8193, 64)) + [8193, 8200, 12000, 32768, 65536]
GRID_B = (1, 2, 255, 256, 512, 1024, 2048, 2100)
GRID_NT = (1, 5, 100, 479, 480, 2015, 2016)


def geometry(R, NT, nseg=1, owned_len=None, halo=0):
    return dict(R=R, NT=NT, nseg=nseg, owned_len=owned_len, halo=halo, chain_major=1 if halo == 0 else 0)


# ---- a. mlmcpi_path_hmc_draw, segmented ------------------------------------------------------------------------------------------
# B = 3 chains from chain0 = 40, two consecutive draws.  dt: nt * dt <= 2 on the two long trajectories; elsewhere the steps of
# tests/test_gpu_parity.py at this lattice spacing (a = 1/8), shortened where nt is longer.  `refused`: the first nt the plan refuses.
SEG_B, SEG_CHAIN0, SEG_DRAWS = 3, 40, 2
SEGMENTED = [
    dict(kind="quartic", M=16, nt=20, dt=0.05, plan=geometry(4, 256, 1, 16, 21),
         what="path shorter than the halo: the 1024-site buffer wraps the ring 64 times, g0 = (M - 21 % 16) % 16"),
    dict(kind="rotor", M=16, nt=100, dt=0.02, plan=geometry(4, 256, 1, 16, 101),
         what="the coarsest level of a hierarchy at the production nt: halo = 101 = 6 M + 5"),
    dict(kind="harmonic", M=10, nt=479, dt=0.004, plan=geometry(4, 256, 1, 10, 480), refused=480, long=True,
         what="the nt limit of the short plan: 2 halo + 64 == 1024, halo = 48 M"),
    dict(kind="quartic", M=1000, nt=11, dt=0.08, plan=geometry(4, 256, 1, 1000, 12),
         what="M + 2 halo == 1024: the short plan with its buffer exactly full"),
    dict(kind="rotor", M=1000, nt=12, dt=0.1, plan=geometry(8, 512, 1, 1000, 13),
         what="M + 2 halo == 1026: the rotor's R = 8, NT = 512 with one segment"),
    dict(kind="quartic", M=8200, nt=10, dt=0.08, plan=geometry(16, 256, 3, 2734, 11),
         what="the smallest multi-segment quartic path: 3 segments of 2734, the last of 2732"),
    dict(kind="rotor", M=4160, nt=10, dt=0.1, plan=geometry(8, 512, 2, 2080, 11),
         what="the smallest multi-segment rotor path: 2 segments of 2080"),
    dict(kind="quartic", M=1000, nt=2015, dt=0.00099, plan=geometry(16, 256, 16, 63, 2016), refused=2016, long=True,
         what="the nt limit of the long plan: 16 segments of 63 (the last of 55), halo = 2016 > 2 M"),
]

# ---- b. draw and run, geometries the batch size selects --------------------------------------------------------------------------
# nt = 6, n_draws = 2, n_rep = 2; dt as test_hmc_run_one_wave_chains_equal_repeated_draws (tests/test_gpu_parity.py) at the same
# lattice spacing.  Accepted draws 0 / 1 / 2 of the first 48 chains under the oracle (batch_outcomes below, asserted in
# tests/test_path_hmc_plan.py):
BATCH_NT, BATCH_DRAWS, BATCH_REP = 6, 2, 2
BATCH = [
    dict(kind="quartic", M=1024, B=256, dt=0.34, plan=geometry(2, 512, 1, 1024)),     # 0 / 2 / 46
    dict(kind="quartic", M=1024, B=512, dt=0.34, plan=geometry(4, 256, 1, 1024)),     # 0 / 1 / 47
    dict(kind="quartic", M=1024, B=1024, dt=0.34, plan=geometry(8, 128, 1, 1024)),    # 0 / 3 / 45
    dict(kind="quartic", M=2048, B=1024, dt=0.34, plan=geometry(16, 128, 1, 2048)),   # 0 / 2 / 46
    dict(kind="rotor", M=1024, B=1024, dt=0.45, plan=geometry(8, 128, 1, 1024)),      # 1 / 26 / 21
]

# ---- c. mlmcpi_path_hmc_run, more than one wave and R > 1 ----------------------------------------------------------------------
# B = 3 chains from chain0 = 3, nt = 6, n_draws = 3, n_rep = 2 (and 5 draws for the split run).  dt chosen with the oracle so
# that the three chains hold a rejected repetition and an accepted draw; accepted draws per chain of the 3-draw run | of the
# 5-draw run, and rejected repetitions in each (run_outcomes below, asserted in tests/test_path_hmc_plan.py):
RUN_B, RUN_CHAIN0, RUN_NT, RUN_DRAWS, RUN_REP = 3, 3, 6, 3, 2
RUN = [
    # (the leapfrog of the quartic action at a = 1/8 is unstable from dt = 0.346: nothing is accepted there)
    dict(kind="quartic", M=2048, qoi_kind=1, dt=0.34, plan=geometry(2, 1024, 1, 2048)),    # 3 2 3, 2 rejected | 4 4 5, 6
    dict(kind="quartic", M=4096, qoi_kind=1, dt=0.34, plan=geometry(4, 1024, 1, 4096)),    # 3 2 3, 2 | 4 3 4, 11
    dict(kind="quartic", M=8192, qoi_kind=1, dt=0.342, plan=geometry(16, 512, 1, 8192)),   # 2 3 3, 3 | 3 3 4, 12
    # (the rotor from angles in (-pi, pi), so that the charges of qoi_kind 2 are not all zero: nothing is accepted from dt = 0.6)
    dict(kind="rotor", M=2048, qoi_kind=2, dt=0.52, plan=geometry(2, 1024, 1, 2048)),      # 3 2 3, 4 | 4 3 3, 14
    dict(kind="rotor", M=4096, qoi_kind=2, dt=0.54, plan=geometry(4, 1024, 1, 4096)),      # 2 1 2, 10 | 2 1 2, 22
]
SEGMENTED_RUN = dict(kind="quartic", M=1000, nt=12, dt=0.08, n_draws=3, n_rep=1, qoi_kind=1, plan=geometry(16, 256, 1, 1000, 13))

MARGIN = 1e-6   # every Metropolis test the GPU tests assert on keeps |u - exp(-dH)| above this under the oracle


def oracle_action(kind, M):
    import oracle
    return oracle.Action(KINDS[kind], **params(kind, M))


def start(kind, M, B, seed):
    """[B, M]: uniform in (-1, 1), the rotor in (-pi, pi), as test_hmc_trajectories_match_oracle"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-np.pi, np.pi, (B, M)) if kind == "rotor" else rng.uniform(-1.0, 1.0, (B, M))


def batch_start(M, B):
    """[B, M] torch.float64 in (-1, 1) for both kinds, as test_hmc_run_one_wave_chains_equal_repeated_draws"""
    import torch
    return torch.rand((B, M), generator=torch.Generator().manual_seed(M + B), dtype=torch.float64) * 2 - 1


def accept_uniform(chain, step):
    import oracle
    out = np.zeros(4)
    oracle.lib().orc_dev_random(SEED, chain, step, 0, oracle.P_ACCEPT, 0, out)
    return out[0]


@functools.lru_cache(maxsize=None)
def oracle_momenta(M, chain, step):
    """the momenta of dev_hmc_trajectory: the cosine branch of one Box-Muller pair per site (purpose P_MOMENTUM)"""
    import oracle
    L, out, p = oracle.lib(), np.zeros(4), np.empty(M)
    for l in range(M):
        L.orc_dev_random(SEED, chain, step, l, oracle.P_MOMENTUM, 0, out)
        p[l] = out[2]
    return p


def oracle_draws(A, x, nt, dt, n_rep, chain, n_draws, traj0=0):
    """HMCSampler::draw n_draws times on one chain by the oracle (hmcsampler.cc:10-12: repetitions stop at the first
    acceptance; repetition r of draw d is Philox step traj0 + d * n_rep + r).  x is updated in place.  Returns per draw the
    accept flag, the energies of the last repetition that ran and the state after it; the number of rejected repetitions;
    and the smallest |u - exp(-dH)| over the Metropolis tests."""
    flags, energies, states, rejected, margin = [], [], [], 0, np.inf
    for d in range(n_draws):
        a = 0
        for r in range(n_rep):
            if a:
                break
            step = traj0 + d * n_rep + r
            a, en, dH = A.dev_hmc_trajectory(x, nt, dt, SEED, chain, step)
            margin = min(margin, abs(accept_uniform(chain, step) - np.exp(min(-dH, 700.0))))
            rejected += 0 if a else 1
        flags.append(a)
        energies.append(en)
        states.append(x.copy())
    return np.array(flags), np.array(energies), states, rejected, margin


@functools.lru_cache(maxsize=None)
def segmented_run(i):
    """the oracle's SEG_DRAWS draws of SEGMENTED[i] on its SEG_B chains: (x0, flags [B, draws], energies [B, draws, 4],
    states [draws][B, M], margin)"""
    c = SEGMENTED[i]
    A, x0 = oracle_action(c["kind"], c["M"]), start(c["kind"], c["M"], SEG_B, c["M"] + c["nt"])
    x = x0.copy()
    out = [oracle_draws(A, x[b], c["nt"], c["dt"], 1, SEG_CHAIN0 + b, SEG_DRAWS) for b in range(SEG_B)]
    states = [np.stack([out[b][2][d] for b in range(SEG_B)]) for d in range(SEG_DRAWS)]
    return x0, np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), states, min(o[4] for o in out)


@functools.lru_cache(maxsize=None)
def ulp_sensitivity(i):
    """The oracle's own sensitivity on SEGMENTED[i]: the largest difference of the state after a draw between the start x0
    and x0 moved by one ulp at every site (towards +inf), same momenta, worst over the case's chains and its SEG_DRAWS
    consecutive draws.  Returns it with the number of (chain, draw) pairs that entered: the state after a draw is the
    trajectory's end only where both starts accept (all of them do: asserted in tests/test_path_hmc_plan.py)."""
    c = SEGMENTED[i]
    A, x0 = oracle_action(c["kind"], c["M"]), start(c["kind"], c["M"], SEG_B, c["M"] + c["nt"])
    worst, counted = 0.0, 0
    for b in range(SEG_B):
        xa, xb = x0[b].copy(), np.nextafter(x0[b], np.inf)
        for d in range(SEG_DRAWS):
            a, _, _ = A.dev_hmc_trajectory(xa, c["nt"], c["dt"], SEED, SEG_CHAIN0 + b, d)
            a2, _, _ = A.dev_hmc_trajectory(xb, c["nt"], c["dt"], SEED, SEG_CHAIN0 + b, d)
            if a and a2:
                worst, counted = max(worst, float(np.max(np.abs(xa - xb)))), counted + 1
    return worst, counted


@functools.lru_cache(maxsize=None)
def batch_outcomes(i, chains):
    """accepted draws (of BATCH_DRAWS) of the given chains of BATCH[i] under the oracle, the states after the run, the
    first draw alone (flag, energies, state: n_rep = 1, what mlmcpi_path_hmc_draw is compared with), and the margin"""
    c = BATCH[i]
    A, x0 = oracle_action(c["kind"], c["M"]), batch_start(c["M"], c["B"]).numpy()
    counts, states, first, margin = [], [], [], np.inf
    for b in chains:
        x = x0[b].copy()
        f, e, s, _, m1 = oracle_draws(A, x, BATCH_NT, c["dt"], 1, b, 1)
        first.append((f[0], e[0], s[0]))
        x = x0[b].copy()
        f, _, _, _, m2 = oracle_draws(A, x, BATCH_NT, c["dt"], BATCH_REP, b, BATCH_DRAWS)
        counts.append(int(f.sum()))
        states.append(x)
        margin = min(margin, m1, m2)
    return counts, states, first, margin


def batch_chains(B):
    return (0, 1, B // 2, B - 1)


@functools.lru_cache(maxsize=None)
def run_outcomes(i, n_draws=RUN_DRAWS):
    """RUN[i] under the oracle: (x0, flags [B, n_draws], states after the run [B, M], QoI [B, n_draws], rejected repetitions,
    margin, and the distance of the states' neighbour differences from the branch cut of mod_2pi)"""
    import oracle
    c = RUN[i]
    M = c["M"]
    A, x0 = oracle_action(c["kind"], M), start(c["kind"], M, RUN_B, M)
    x, flags, q, rejected, margin, cut = x0.copy(), [], np.zeros((RUN_B, n_draws)), 0, np.inf, np.inf
    L = oracle.lib()
    for b in range(RUN_B):
        f, _, states, rej, m = oracle_draws(A, x[b], RUN_NT, c["dt"], RUN_REP, RUN_CHAIN0 + b, n_draws)
        flags.append(f)
        rejected, margin = rejected + rej, min(margin, m)
        for d, s in enumerate(states):
            q[b, d] = L.orc_qoi_xsquared(s, M) if c["qoi_kind"] == 1 else L.orc_qoi_susceptibility(s, M, params(c["kind"], M)["T_final"])
            w = np.mod(s - np.roll(s, 1) + np.pi, 2 * np.pi) - np.pi
            cut = min(cut, float(np.min(np.pi - np.abs(w))))
    return x0, np.stack(flags), x, q, rejected, margin, cut
