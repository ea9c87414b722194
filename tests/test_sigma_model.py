"""CPU checks of the O(3) nonlinear sigma model's numpy restatement (tests/sigma_model.py), which the GPU tests compare the
kernels with: its random numbers, its action and force, the overrelaxation map, the heat-bath law (pinned to the reference
author's Python, tests/golden/sigma_compactexp.json) and the exact answers of the 2 x 2 lattice."""
import json
import math
import os

import numpy as np
import pytest

import sigma_model as sm
from conftest import zcheck

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _state(B, Mt, Mx, seed):
    return sm.initialise(B, Mt, Mx, seed)


def test_philox_matches_known_answers():
    kat = _load("philox_kat.json")
    for v in kat["vectors"]:
        r = sm.philox(*[int(x, 16) for x in v["ctr"]], *[int(x, 16) for x in v["key"]])
        assert [f"{int(x):08x}" for x in r] == v["out"]


@pytest.mark.parametrize("purpose,sub", [(6, 0), (14, 0), (14, 5)])
def test_uniforms_match_oracle(orc, purpose, sub):
    seed, chain, step, n = 0x1234_5678_9ABC, 3, 77, 300
    u, v = sm.uniforms(seed, chain, step, np.arange(n, dtype=np.uint64), purpose, sub)
    want = np.zeros(4)
    for k in range(n):
        orc.lib().orc_dev_random(seed, chain, step, k, purpose, sub, want)
        assert (u[k], v[k]) == (want[0], want[1])


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (4, 6), (8, 8)])
def test_evaluate_is_the_bond_sum(Mt, Mx):
    beta = 0.73
    phi = _state(3, Mt, Mx, 11)
    sig = sm.unit_vectors(phi, Mt, Mx).reshape(3, Mx, Mt, 3)
    bonds = np.zeros(3)
    for j in range(Mx):
        for i in range(Mt):
            bonds += np.einsum("bc,bc->b", sig[:, j, i], sig[:, j, (i + 1) % Mt] + sig[:, (j + 1) % Mx, i])
    np.testing.assert_allclose(sm.evaluate(phi, Mt, Mx, beta), -beta * bonds, rtol=1e-13, atol=1e-13)


def test_force_is_the_gradient_of_evaluate():
    Mt, Mx, beta, h = 4, 6, 1.3, 1e-6
    phi = _state(2, Mt, Mx, 5)
    f = sm.force(phi, Mt, Mx, beta)
    for e in range(0, 2 * Mt * Mx, 5):
        p, m = phi.copy(), phi.copy()
        p[:, e] += h
        m[:, e] -= h
        fd = (sm.evaluate(p, Mt, Mx, beta) - sm.evaluate(m, Mt, Mx, beta)) / (2 * h)
        np.testing.assert_allclose(f[:, e], fd, atol=2e-8)


@pytest.mark.parametrize("colour", [0, 1])
def test_overrelaxation_keeps_the_action_and_is_an_involution(colour):
    Mt, Mx, beta = 8, 6, 1.1
    phi = _state(4, Mt, Mx, 9)
    once = sm.phase(phi, Mt, Mx, beta, colour, False)
    S0, S1 = sm.evaluate(phi, Mt, Mx, beta), sm.evaluate(once, Mt, Mx, beta)
    np.testing.assert_allclose(S1, S0, rtol=1e-12)
    twice = sm.phase(once, Mt, Mx, beta, colour, False)
    np.testing.assert_allclose(sm.unit_vectors(twice, Mt, Mx), sm.unit_vectors(phi, Mt, Mx), atol=1e-13)
    assert np.abs(sm.unit_vectors(once, Mt, Mx) - sm.unit_vectors(phi, Mt, Mx)).max() > 1e-3  # it did move


def test_heatbath_keeps_spins_when_the_neighbour_sum_vanishes():
    sig = np.array([[0.6, 0.0, 0.8]])
    out = sm.heatbath(sig, np.zeros((1, 3)), 1.0, np.array([0.3]), np.array([0.7]))
    assert np.array_equal(out, sig)
    assert np.array_equal(sm.overrelax(sig, np.zeros((1, 3))), sig)


def test_fixture_is_the_compact_exponential_law():
    fx = _load("sigma_compactexp.json")
    x = np.array(fx["x"])
    for row in fx["table"]:
        s = row["s"]
        want = s / (2.0 * math.sinh(s)) * np.exp(s * x)
        np.testing.assert_allclose(np.array(row["density"]), want, rtol=1e-12, atol=0)
        # the CDF the KS tests use is the integral of that density
        cdf = sm.compact_exp_cdf(s, x)
        trap = np.concatenate([[0.0], np.cumsum(0.5 * (want[1:] + want[:-1]) * np.diff(x))])
        assert np.max(np.abs(cdf - trap)) < 2e-3 * max(1.0, s / 10)


def _ks(sample, cdf):
    xs = np.sort(sample)
    n = len(xs)
    F = cdf(xs)
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)) * math.sqrt(n)


@pytest.mark.parametrize("s", [0.0, 1e-8, 0.1, 1.0, 4.0, 16.0, 40.0])
def test_inversion_follows_the_law(s):
    n = 200_000
    u, _ = sm.uniforms(99, 1, 2, np.arange(n, dtype=np.uint64), sm.P_SIGMA_HB)
    x = sm.compact_exp_inverse(s, u)
    assert np.all(np.isfinite(x)) and np.all(np.abs(x) <= 1.0)
    d = _ks(x, lambda t: sm.compact_exp_cdf(s, t))
    assert d < 1.95, f"KS sqrt(n) D = {d:.3f} (5 % level 1.36, 0.1 % level 1.95)"
    # and the inversion agrees with the issue's form log1p(u expm1(2 s)) / s - 1 where that one is finite
    if 0 < s <= 16:
        np.testing.assert_allclose(x, np.log1p(u * np.expm1(2 * s)) / s - 1.0, atol=1e-9)


def test_ring_closed_form_values():
    table = {0.5: (-1.3513512166, 1.8675717559), 1.0: (-4.8471325592, 2.7061452532), 1.5: (-8.8839929225, 3.1433862817)}
    for beta, (S, chi) in table.items():
        gS, gchi = sm.ring_exact(beta)
        assert abs(gS - S) < 1e-9 and abs(gchi - chi) < 1e-9
        # c1 = 1/4 d ln Z / dK (K = 2 beta): <S> = -8 beta c1
        def lnZ(K):
            lam = np.array([sm._sph_in(l, K) for l in range(61)])
            return math.log(np.sum((2 * np.arange(61) + 1) * lam ** 4))
        K, h = 2 * beta, 1e-5
        c1 = 0.25 * (lnZ(K + h) - lnZ(K - h)) / (2 * h)
        assert abs(-8 * beta * c1 - S) < 1e-7


@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_restatement_chain_on_the_ring(beta):
    """the restatement's heat-bath chain (3 overrelaxation + 1 heat-bath sweeps per draw) on 2 x 2 against the exact
    transfer-matrix answers"""
    B, n_draw, Mt = 2000, 40, 2
    phi = sm.initialise(B, Mt, Mt, 21)
    S, chi = [], []
    for d in range(n_draw):
        phi = sm.sweep_draw(phi, Mt, Mt, beta, 3, 1, seed=21, sweep0=4 * d)
        if d >= 5:
            S.append(sm.evaluate(phi, Mt, Mt, beta))
            chi.append(sm.magnetic_susceptibility(phi, Mt, Mt))
    S, chi = np.array(S).mean(axis=0), np.array(chi).mean(axis=0)  # per chain time averages: independent
    eS, echi = sm.ring_exact(beta)
    zcheck(f"restatement 2x2 beta={beta} <S>", S.mean(), S.std(ddof=1) / math.sqrt(B), eS)
    zcheck(f"restatement 2x2 beta={beta} <chi_m>", chi.mean(), chi.std(ddof=1) / math.sqrt(B), echi)
