"""CPU: pins tests/path_correlator_reference.py (the long-double definition of mlmcpi_path_correlator) to the identities of the
header, and the closed forms of <C(tau)> -- harmonic oscillator and rotor on the periodic lattice -- to independent sums."""
import math

import numpy as np
import pytest

import path_correlator_reference as ref
import path_reference as pr

MS = [2, 7, 16, 130]


def _paths(kind, M, B=4, seed=5):
    rng = np.random.default_rng(seed + 100 * kind + M)
    return rng.uniform(-4 * np.pi, 4 * np.pi, (B, M)) if kind == ref.ROTOR else rng.standard_normal((B, M))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_lag_zero(kind, M):
    x = _paths(kind, M)
    C = ref.correlator(kind, x, M // 2 + 1)
    assert C.dtype == np.longdouble and C.shape == (4, M // 2 + 1)
    want = np.ones(4, dtype=np.longdouble) if kind == ref.ROTOR else pr.xsquared(x)
    assert float(np.max(np.abs(C[:, 0] - want))) <= 4e-19 * M * float(np.max(np.abs(want)))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_weighted_sum_is_the_squared_sum_of_the_path(kind, M):
    x = _paths(kind, M)
    C = ref.correlator(kind, x, M // 2 + 1)
    w = ref.weights(M)
    if M % 2:
        assert w[0] == 1.0 and np.all(w[1:] == 2.0)
    else:
        assert w[0] == w[-1] == 1.0 and np.all(w[1:-1] == 2.0)
    want = sum(np.sum(c, axis=-1) ** 2 for c in ref.components(kind, x)) / np.longdouble(M)
    scale = sum(np.sum(np.abs(c), axis=-1) ** 2 for c in ref.components(kind, x)) / M
    assert float(np.max(np.abs((C * w).sum(axis=-1) - want) / scale)) <= 1e-17 * M


@pytest.mark.parametrize("kind", [0, 2])
def test_definition_against_the_plain_double_loop(kind):
    M, x = 7, _paths(kind, 7)
    C = ref.correlator(kind, x, 4)
    for b in range(x.shape[0]):
        for tau in range(4):
            xs = x[b].astype(np.longdouble)
            terms = [np.cos(xs[j] - xs[(j + tau) % M]) if kind == ref.ROTOR else xs[j] * xs[(j + tau) % M] for j in range(M)]
            assert abs(float(C[b, tau] - sum(terms) / M)) <= 1e-17


@pytest.mark.parametrize("M,T_final,m0,mu2", [(16, 4.0, 1.0, 1.0), (128, 4.0, 1.0, 1.0), (7, 2.0, 0.7, 3.0), (16, 4.0, 1.0, 0.0625 * 16)])
def test_ho_closed_form_is_the_eigenvalue_sum(M, T_final, m0, mu2):
    tau = np.arange(M // 2 + 1)
    got, want = ref.ho_exact(M, T_final, m0, mu2, tau), ref.ho_eigen_sum(M, T_final, m0, mu2, tau)
    assert float(np.max(np.abs(got - want))) <= 1e-13, (got, want)


def test_rotor_closed_form_against_brute_force_quadrature():
    tau = np.arange(3)
    brute, closed = ref.rotor_brute_force(4, 1.3, tau, points=64), ref.rotor_exact(4, 1.3, tau)
    print("rotor M = 4, kappa = 1.3:", brute, closed)
    assert abs(brute[0] - 1.0) <= 1e-12
    assert abs(brute[1] - 0.62256273) <= 1e-8 and abs(brute[2] - 0.51500743) <= 1e-8
    assert float(np.max(np.abs(brute - closed))) <= 1e-12


def test_bessel_quadrature_is_the_power_series():
    for n, kappa in ((0, 1.0), (1, 1.0), (2, 1.3), (5, 1.0)):
        series = sum((kappa / 2) ** (2 * k + n) / (math.factorial(k) * math.factorial(k + n)) for k in range(30))
        assert abs(float(ref.bessel_i(n, kappa)) - series) <= 2e-16 * series, (n, kappa)
