"""Shapes, inputs and oracle-driven runs of tests/test_path_splits_gpu.py, with the launch arithmetic of path1d.hip they are
chosen by.  Everything here is decided without a device; tests/test_path_reference.py asserts the conditions the GPU tests
rely on (splits reached, distance from the branch cut of mod_2pi, both outcomes of the two-level steps, both mask values on
every level of the hierarchy).  Long-double values come from tests/path_reference.py.
"""
import functools

import numpy as np

from path_reference import LD, PI, action, force, masked_twolevel_draw, mod_2pi, susceptibility, xsquared

KINDS = {"harmonic": 0, "quartic": 1, "rotor": 2}
SEED = 0x1234567812345678


def params(kind, M):
    """the parameters tests/test_gpu_parity.py uses for the 1-D actions, at lattice spacing a = 1/8"""
    if kind == "rotor":
        return dict(M=M, T_final=M / 8.0, m0=0.25)
    p = dict(M=M, T_final=M / 8.0, m0=1.0, mu2=1.0)
    if kind == "quartic":
        p.update(lam=1.0, x0=1.0)
    return p


# ---- the launch arithmetic of path1d.hip, mirrored -------------------------------------------------------------------------
def choose_split(sites, B):
    """workgroups per chain (path1d.hip choose_split): fill 256 CUs, at least ~1024 sites each"""
    return max(1, min(-(-2048 // B), -(-sites // 1024)))


def split_bounds(M, B):
    """[(lo, hi)] of the splits path_reduce_kernel gives a chain"""
    n = choose_split(M, B)
    per = -(-M // n)
    return [(s * per, min(M, s * per + per)) for s in range(n)]


# ---- inputs of the reductions, force, initialise -------------------------------------------------------------------------------
# (M, B) -> what of choose_split it reaches
SHAPES = [
    (1025, 3),      # 2 splits of 513 and 512
    (2050, 2),      # 3 splits of 684, 684, 682: short last split, three passes of 256 with a tail
    (4100, 1500),   # want = 2 < cap = 5: 2 splits of 2050, 9 passes each
    (1100, 300),    # 2 splits, two blocks of path_finish_kernel (the second with 44 live threads)
    (1100, 2100),   # want = 1: one workgroup per chain, in-kernel finish, M > 1024
]
BRANCH_MARGIN = 1e-6   # every |mod_2pi(d)| of a rotor input stays this far from pi


def spike_sites(M, B):
    """site 0, site M - 1, and the first and last site of every split"""
    s = {0, M - 1}
    for lo, hi in split_bounds(M, B):
        s.update((lo, hi - 1))
    return sorted(s)


@functools.lru_cache(maxsize=2)   # (4100, 1500) is 49 MB: the current case and the one before, no more
def path_input(kind, M, B):
    """[B, M] float64, every chain its own seeded data; the last chain carries the spikes.  Rotor: angles whose differences
    keep 10 * BRANCH_MARGIN away from the branch cut of mod_2pi (entries that do not are moved by 0.05 until they do)."""
    rng = np.random.default_rng(1000 * M + 10 * B + KINDS[kind])
    sites = spike_sites(M, B)
    if kind == "rotor":
        x = rng.uniform(-np.pi, np.pi, (B, M))
        x[B - 1, sites] = [2.9 - 0.31 * i if i % 2 else -2.9 + 0.31 * i for i in range(len(sites))]
        for _ in range(20):
            d = mod_2pi(x.astype(LD) - np.roll(x, 1, axis=1).astype(LD))
            bad = np.abs(np.abs(d) - PI) < 10 * BRANCH_MARGIN
            if not bad.any():
                break
            x[bad] += 0.05
        else:
            raise AssertionError("rotor input still at the branch cut")
    else:
        x = rng.uniform(-3.0, 3.0, (B, M))
        x[B - 1, sites] = [(6.0 + 0.25 * i) * (-1) ** i for i in range(len(sites))]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)   # long-double forces are 16 bytes a site: not kept beyond the test that uses them
def reference(what, kind, M, B):
    """the long-double value of `what` on path_input(kind, M, B); every value has one GPU test that reads it"""
    x, p = path_input(kind, M, B), params(kind, M)
    if what == "action":
        return action(kind, p, x)
    if what == "force":
        return force(kind, p, x)
    if what == "xsquared":
        return xsquared(x)
    assert what == "susceptibility"
    return susceptibility(x, p["T_final"])


# ---- the two-level step ----------------------------------------------------------------------------------------------------
# (kind, fine M, width of the rough proposals): Mc = M / 2 against the block size (1024 threads, 512 for the rotor).  On the
# paths of 8 and 4 sites the two levels differ by so little that a proposal of width 1 is always accepted; the widths
# there are the smallest of 1, 2, 3, 5, 10 at which the oracle refuses some (see twolevel_run)
TWOLEVEL_CASES = [
    ("harmonic", 4100, 1.0),   # Mc = 2050: three passes, the last with 2 live lanes
    ("quartic", 2052, 1.0),    # Mc = 1026: second pass of 2 lanes
    ("rotor", 1030, 1.0),      # Mc = 515 against 512 threads
    ("harmonic", 8, 1.0), ("quartic", 8, 10.0), ("rotor", 8, 3.0),   # Mc = 4: one wave, 60 idle lanes
    ("harmonic", 4, 1.0), ("quartic", 4, 10.0), ("rotor", 4, 3.0),   # Mc = 2: the coarse path's two neighbours are one site
]
TWOLEVEL_B, TWOLEVEL_CHAIN0 = 5, 9
TWOLEVEL_MASKS = [[1, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 1, 0, 1, 1], [1, 1, 0, 0, 1]]


def twolevel_actions(orc, kind, M):
    p = params(kind, M)
    return orc.Action(KINDS[kind], **p), orc.Action(KINDS[kind], **dict(p, M=M // 2))


@functools.lru_cache(maxsize=None)
def twolevel_run(kind, M, rough=1.0):
    """Six masked draws of the oracle on TWOLEVEL_B chains: (theta0, [(x_coarse, mask, accept, terms, theta after)]).
    Coarse proposals as in test_twolevel_step_matches_oracle: the coarse points of the current state, perturbed a little
    on even draws and by `rough` on odd ones, so that both outcomes occur."""
    import oracle
    F, Cc = twolevel_actions(oracle, kind, M)
    B = TWOLEVEL_B
    rng = np.random.default_rng(100 * M + KINDS[kind])
    theta0 = rng.uniform(-np.pi, np.pi, (B, M)) if kind == "rotor" else rng.normal(0.5, 0.6, (B, M))
    theta, draws = theta0.copy(), []
    for t, mask in enumerate(TWOLEVEL_MASKS):
        xc = theta[:, ::2] + rng.normal(0, 1e-3 if t % 2 == 0 else rough, (B, M // 2))
        accept, terms = masked_twolevel_draw(F, Cc, xc, theta, mask, SEED, TWOLEVEL_CHAIN0, t)
        draws.append((xc, np.array(mask, dtype=np.int32), accept, terms, theta.copy()))
    return theta0, draws


# ---- the hierarchical sampler ----------------------------------------------------------------------------------------------
HIER = dict(levels=(256, 128, 64), T_final=32.0, B=8, nt=6, dt=0.34, n_draws=4, seed=SEED + 77, chain0=3)


def hier_actions(orc):
    return [orc.Action(orc.QUARTIC, M=M, T_final=HIER["T_final"], m0=1.0, mu2=1.0, lam=1.0, x0=1.0) for M in HIER["levels"]]


def hier_start():
    """a smooth start on the finest level (coarse random walk, interpolated, plus a little noise)"""
    M, B = HIER["levels"][0], HIER["B"]
    rng = np.random.default_rng(7)
    walk = np.cumsum(rng.normal(0, 0.2, (B, M // 16)), axis=1)
    walk -= np.linspace(0, 1, M // 16)[None, :] * (walk[:, -1:] - walk[:, :1])
    return 1.0 + 0.3 * np.repeat(walk, 16, axis=1) + rng.normal(0, 0.02, (B, M))


@functools.lru_cache(maxsize=None)
def hier_run():
    """HierarchicalSampler::draw (hierarchicalsampler.cc:55-81) written with the oracle, as mlmc.HierChain numbers its
    streams: restriction down the levels, one HMC trajectory on the coarsest, then two-level steps upwards where a chain
    refused below does not move.  Returns [{level: (mask into the level, accept, state after)}] per draw."""
    import oracle
    acts, L, B = hier_actions(oracle), len(HIER["levels"]), HIER["B"]
    seed, chain0 = HIER["seed"], HIER["chain0"]
    host = [hier_start()[:, :: (1 << k)].copy() for k in range(L)]
    draws = []
    for d in range(HIER["n_draws"]):
        for k in range(1, L):
            host[k] = host[k - 1][:, ::2].copy()
        mask = np.zeros(B, dtype=np.int32)
        for b in range(B):
            mask[b], _, _ = acts[-1].dev_hmc_trajectory(host[L - 1][b], HIER["nt"], HIER["dt"], seed, chain0 + b, d)
        rec = {L - 1: (np.ones(B, dtype=np.int32), mask.copy(), host[L - 1].copy())}
        for k in range(L - 2, -1, -1):
            acc, _ = masked_twolevel_draw(acts[k], acts[k + 1], host[k + 1], host[k], mask, seed + 31 * (k + 1), chain0, d)
            rec[k] = (mask.copy(), acc.copy(), host[k].copy())
            mask = acc
        draws.append(rec)
    return draws


# ---- the rotor draw + QoI + moments in one call -------------------------------------------------------------------------------
# rotor_sweeps.hip goes through path_finish (with d_acc) whenever a QoI is asked for, whatever the number of segments, so
# the smallest M is the smallest the sweeps take with a charge that can be non-zero: M = 2 has Q = 0 identically, M = 4 (the
# next even M) allows Q = +-2 pi.  T_final = M (a = 1, 2 m0 / a = 0.5): a nearly flat conditional, so that charges occur.
SWEEP_QOI = dict(M=4, T_final=4.0, m0=0.25, B=300, n_or=3, n_hb=1, chain0=9, sweep0=50)
