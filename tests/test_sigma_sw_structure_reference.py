"""CPU: the cluster-improved structure factor of the Swendsen-Wang update as tests/sigma_sw_structure_reference.py states it:
the positions against the time-slice correlator's slice assignment, the identity F^imp = mean over the coins by enumeration,
the closed form on an extent of 2, and the law F^imp = plain F on a model chain."""
import math

import numpy as np
import pytest

import sigma_correlator_reference as cref
import sigma_level_model as slm
import sigma_level_sw_model as slsw
import sigma_sw_structure_reference as ssr
from conftest import zcheck

LD = np.longdouble
LEVELS = [(2, 2), (2, 6), (4, 6), (16, 16), (66, 34)]


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", LEVELS)
def test_plain_structure_factor_from_the_positions_equals_the_correlators(Mt, Mx, rot):
    """|sum sigma e^{ipx}|^2 / n from the positions = sum_tau w(tau) C(tau) cos(2 pi tau / M) of the correlator reference: the
    positions are the slice assignment of mlmcpi_sigma_level_correlator"""
    L = slm.Level(Mt, Mx, rot)
    phi = slm.initialise(L, 2, 17 + Mt)
    Ct, Cx = cref.split(cref.correlator(Mt, Mx, rot, phi), Mt, Mx)
    sig = cref.spins(phi, L.n)
    for b in range(2):
        for d, (C, M) in enumerate(((Ct, Mt), (Cx, Mx))):
            tau = np.arange(M // 2 + 1)
            want = (C[b] * cref.weights(M).astype(LD) * np.cos(2 * ssr.PI * tau.astype(LD) / LD(M))).sum()
            got = ssr.plain(L, sig[b], d)
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (b, d, got, want)


def _few_clusters(L, most=12):
    """the first (seed, update) of a model chain from a heat-bath start whose update has 2 .. `most` clusters, one larger than 1"""
    for seed in range(1, 200):
        phi = slm.sweep_draw(L, slm.initialise(L, 1, seed), 10, 1, seed)[0]
        for step in range(4):
            new, info = slsw.dev_update(L, phi, seed, 0, step)
            if 2 <= info["clusters"] <= most and np.bincount(info["labels"]).max() > 1:
                return seed, step, phi, info
            phi = new
    raise AssertionError("no update with few clusters")


@pytest.mark.parametrize("Mt,Mx,rot,beta", [(4, 4, False, 2.0), (4, 6, True, 2.0)])
def test_improved_equals_the_mean_over_all_coin_assignments(Mt, Mx, rot, beta):
    L = slm.Level(Mt, Mx, rot, beta)
    seed, step, phi, info = _few_clusters(L)
    print(f"{Mt}x{Mx} rotated={rot}: seed {seed} update {step}, {info['clusters']} clusters")
    assert 2 <= info["clusters"] <= 12
    for d in range(2):
        got, want = ssr.improved(L, info["a"], info["labels"], d), ssr.coin_mean(L, info["a"], info["labels"], d)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (d, got, want)


@pytest.mark.parametrize("Mt,Mx,rot", [(2, 6, False), (2, 2, True), (6, 2, True), (2, 2, False)])
def test_an_extent_of_two_weighs_even_and_odd_positions_with_plus_and_minus_one(Mt, Mx, rot):
    L = slm.Level(Mt, Mx, rot, 1.0)
    phi = slm.sweep_draw(L, slm.initialise(L, 1, 5), 10, 1, 5)[0]
    _, info = slsw.dev_update(L, phi, 5, 0, 0)
    a, lab = info["a"].astype(LD), info["labels"]
    for d, M in enumerate((Mt, Mx)):
        if M != 2:
            continue
        x = cref.coords(Mt, Mx, rot)[d]
        want = LD(3) * sum((a[(lab == c) & (x == 0)].sum() - a[(lab == c) & (x == 1)].sum()) ** 2 for c in np.unique(lab)) / LD(L.n)
        assert abs(ssr.improved(L, a, lab, d) - want) <= 1e-15 * max(1.0, abs(want))
        c, s = ssr.phases(L, d)
        assert set(np.unique(c)) <= {LD(1), LD(-1)} and not s.any()


def test_the_improved_structure_factor_has_the_mean_of_the_plain_one_on_a_model_chain():
    """4 x 4 unrotated, beta = 1, 32 chains x (100 + 400) updates of the model: mean F^imp against mean plain F of the field
    before each update, both directions, errors over the chains.  Run first on the CPU: z = -0.42 (t), +0.54 (x)."""
    L = slm.Level(4, 4, False, 1.0)
    B, burn, meas = 32, 100, 400
    phi = slm.initialise(L, B, 71)
    imp, pl = np.zeros((B, 2)), np.zeros((B, 2))
    for step in range(burn + meas):
        if step >= burn:
            sig = cref.spins(phi, L.n)
            for b in range(B):
                _, info = slsw.dev_update(L, phi[b], 72, b, step)
                for d in range(2):
                    imp[b, d] += float(ssr.improved(L, info["a"], info["labels"], d))
                    pl[b, d] += float(ssr.plain(L, sig[b], d))
        phi, _ = slsw.dev_update_batch(L, phi, 72, 0, step)
    imp, pl = imp / meas, pl / meas
    err = lambda v: float(v.std(ddof=1) / math.sqrt(B))  # noqa: E731
    for d, name in enumerate("tx"):
        print(f"F_{name}: improved {imp[:, d].mean():.5f} +- {err(imp[:, d]):.2g}, plain {pl[:, d].mean():.5f} +- {err(pl[:, d]):.2g}")
        zcheck(f"sigma SW model 4x4 beta=1: improved F_{name} vs plain F_{name}", float(imp[:, d].mean()), err(imp[:, d]),
               float(pl[:, d].mean()), err(pl[:, d]))
