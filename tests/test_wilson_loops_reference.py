"""CPU: tests/wilson_loops_reference.py pinned -- the boundary-link definition against the sum over cells, W(1, 1) against the
oracle's average plaquette, W(Mt, Mx) = 1, gauge invariance, the single-link spike in closed form, and the exact series against
direct quadrature of the constrained plaquette law on 2 x 2 and against its infinite-volume limit at 64 x 64."""
import numpy as np
import pytest

import oracle
import wilson_loops_reference as ref

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _theta(Mt, Mx, B, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, (B, 2 * Mt * Mx))


@pytest.mark.parametrize("Mt,Mx,R,S", [(2, 2, 2, 2), (5, 3, 5, 3), (9, 12, 4, 7)])
def test_boundary_sum_is_the_cell_sum(Mt, Mx, R, S):
    th = _theta(Mt, Mx, 2, Mt + Mx)
    a, b = ref.loop_angles(th, Mt, Mx, R, S), ref.loop_angles_from_cells(th, Mt, Mx, R, S)
    # both are sums of at most 4 R S links of magnitude <= pi
    assert np.max(np.abs(a - b)) <= 4 * R * S * np.pi * 4 * R * S * EPS_LD
    assert np.max(np.abs(a[:, 0, 0] - ref.plaquette_angles(th, Mt, Mx))) <= 16 * np.pi * EPS_LD


def test_the_smallest_loop_is_the_average_plaquette():
    Mt, Mx = 6, 10
    th = _theta(Mt, Mx, 3, 4)
    W = ref.wilson_loops(th, Mt, Mx, 1, 1)
    for b in range(3):
        assert abs(float(W[b, 0, 0]) - oracle.lib().orc_qoi_avg_plaquette(np.ascontiguousarray(th[b]), Mt, Mx)) <= 1e-14


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (5, 3), (8, 8)])
def test_the_loop_around_the_lattice_is_one(Mt, Mx):
    W = ref.wilson_loops(_theta(Mt, Mx, 2, 1), Mt, Mx, Mt, Mx)
    assert np.max(np.abs(W[:, -1, -1] - 1)) <= (4 * Mt * Mx * np.pi) ** 2 * EPS_LD


def test_gauge_invariance():
    Mt, Mx, R, S = 7, 5, 4, 5
    th = _theta(Mt, Mx, 2, 8)
    g = np.random.default_rng(9).uniform(-np.pi, np.pi, (2, Mx, Mt))
    a, b = ref.wilson_loops(th, Mt, Mx, R, S), ref.wilson_loops(ref.gauge_transform(th, Mt, Mx, g), Mt, Mx, R, S)
    # the transformed links are fp64 roundings of the exact ones: <= 2 (r + s) links per loop, each off by <= 3 pi eps
    assert np.max(np.abs(a - b)) <= 2 * (R + S) * 3 * np.pi * ref.EPS


def test_single_link_spike_in_closed_form():
    Mt, Mx, R, S, alpha = 7, 6, 6, 5, 0.9
    th = np.zeros((2, Mx, Mt, 2))
    th[0, 2, 3, 0] = th[1, 5, 6, 1] = alpha
    W = ref.wilson_loops(th.reshape(2, -1), Mt, Mx, R, S)
    r, s = np.arange(1, R + 1)[:, None], np.arange(1, S + 1)[None, :]
    # the closed forms are evaluated in fp64: a few roundings of numbers below 1
    assert np.max(np.abs(W[0] - (1 - 2 * r / (Mt * Mx) * (1 - np.cos(alpha)) + 0 * s))) <= 4 * ref.EPS
    assert np.max(np.abs(W[1] - (1 - 2 * s / (Mt * Mx) * (1 - np.cos(alpha)) + 0 * r))) <= 4 * ref.EPS
    # wrapped: r = Mt puts the two theta1 edges on one another, so a theta1 spike cancels; the theta0 edges still count
    Ww = ref.wilson_loops(th.reshape(2, -1), Mt, Mx, Mt, 2)
    assert abs(float(Ww[1, Mt - 1, 0]) - 1) <= 1e-18 and abs(float(Ww[0, Mt - 1, 0]) - (1 - 2 * Mt / (Mt * Mx) * (1 - np.cos(alpha)))) <= 4 * ref.EPS


@pytest.mark.parametrize("beta", [0.5, 2.0, 4.0])
def test_exact_series_against_quadrature_on_2x2(beta):
    """three free plaquettes, the fourth fixed by the torus constraint: areas 1, 2 and 4"""
    q1, q2, q4 = ref.quadrature_2x2(beta)
    assert abs(ref.wilson_loop_exact(beta, 2, 2, 1, 1) - q1) <= 1e-14
    assert abs(ref.wilson_loop_exact(beta, 2, 2, 2, 1) - q2) <= 1e-14 and abs(ref.wilson_loop_exact(beta, 2, 2, 1, 2) - q2) <= 1e-14
    assert abs(ref.wilson_loop_exact(beta, 2, 2, 2, 2) - q4) <= 1e-15


@pytest.mark.parametrize("beta", [0.5, 2.0, 10.0])
def test_exact_series_tends_to_the_area_law(beta):
    ratio = float(ref.bessel_ratio(1, beta))
    for r, s in ((1, 1), (2, 3), (4, 4)):
        assert abs(ref.wilson_loop_exact(beta, 64, 64, r, s) / ratio ** (r * s) - 1) <= 1e-13
    assert abs(ref.string_tension_exact(beta) + np.log(ratio)) <= 1e-15
    W = ref.wilson_loops_exact(beta, 64, 64, 3, 3)
    assert abs(ref.creutz_ratio(W, 3, 3) - ref.string_tension_exact(beta)) <= 1e-12
    # on a small lattice the torus constraint shows: 4 x 4 at beta = 10 is far from the area law
    assert abs(ref.wilson_loop_exact(10.0, 4, 4, 2, 2) / float(ref.bessel_ratio(1, 10.0)) ** 4 - 1) > 1e-3


def test_bessel_ratio_against_the_integral_representation():
    """I_n(beta) = (1/pi) int_0^pi exp(beta cos t) cos(n t) dt by the periodic trapezoid rule in long double (exact to rounding);
    scipy's ive as well where it is installed"""
    t = (np.arange(512, dtype=LD) + LD(0.5)) * (np.arccos(LD(-1)) / 256)
    try:
        from scipy import special
    except ImportError:
        special = None
    for beta in (0.5, 2.0, 10.0):
        I = lambda n: np.sum(np.exp(LD(beta) * (np.cos(t) - 1)) * np.cos(n * t)) / 512
        for n in (1, 2, 5):   # the ratios the rule resolves: I_5(0.5) / I_0 = 8e-6 against its rounding of 1e-19
            assert abs(float(ref.bessel_ratio(n, beta) / (I(n) / I(0))) - 1) <= 1e-13
        for n in (1, 2, 5, 20):
            if special is not None:
                assert abs(float(ref.bessel_ratio(n, beta)) / (special.ive(n, beta) / special.ive(0, beta)) - 1) <= 1e-13
