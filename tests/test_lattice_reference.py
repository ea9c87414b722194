"""CPU: the long-double restatement (tests/lattice_reference.py) against the oracle's Action.force / evaluate and QoIs
and against the plaquettes, action and QoIs held in tests/golden/schwinger_ref_python.json (the reference author's own
Python), so that it is trusted before tests/test_lattice_bands_gpu.py holds a kernel to it."""
import json
import os

import numpy as np
import pytest

import lattice_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble


def seq(n):
    return np.sin(np.arange(n) + 1.0)


def test_long_double_is_extended_and_its_libm_is_too():
    assert np.finfo(LD).eps <= 2.0 ** -63
    # fp64 pi is 1.22e-16 below pi: a long-double sine sees that, a double-precision one behind a cast would not
    assert abs(np.sin(LD(np.pi)) - LD("1.2246467991473531772e-16")) < 1e-34
    assert abs(np.sin(ref.PI / 6) - LD(0.5)) <= 2.0 ** -63
    assert abs(np.cos(ref.PI / 3) - LD(0.5)) <= 2.0 ** -63
    x = np.linspace(-12.0, 12.0, 1001).astype(LD)
    assert np.max(np.abs(np.sin(x) ** 2 + np.cos(x) ** 2 - 1)) <= 4 * 2.0 ** -63
    assert np.max(np.abs(np.sin(x) - np.sin(x.astype(np.float64)))) <= 2.0 ** -52  # and agrees with fp64 to fp64's error


def test_mod_2pi_and_branch_cut_distance():
    x = np.array([0.0, 1.0, -1.0, 3.0, -3.0, 4.0, -4.0, 7.0, 100.0])
    w = ref.mod_2pi(x)
    assert np.all(np.abs(w) <= ref.PI)
    k = (x - w) / ref.TWO_PI
    assert np.max(np.abs(k - np.rint(k))) < 1e-17
    assert abs(ref.mod_2pi(4.0) - (4 - ref.TWO_PI)) < 1e-18
    # a 2 x 2 field whose only non-zero plaquette angles are +-(pi - 1e-3)
    t = np.zeros(8)
    t[0] = np.pi - 1e-3
    assert abs(ref.distance_to_branch_cut(t, 2, 2) - 1e-3) < 1e-12


SCHW_SHAPES = [(4, 4, 1.0), (16, 6, 2.5), (7, 5, 0.7)]     # square, Mt != Mx, both odd
GFF_SHAPES = [(4, 10.0), (30, 2.0), (17, 0.3)]


@pytest.mark.parametrize("Mt,Mx,beta", SCHW_SHAPES)
def test_schwinger_reference_equals_oracle(orc, Mt, Mx, beta):
    L = orc.lib()
    A = orc.Action(orc.SCHWINGER, Mt=Mt, Mx=Mx, beta=beta)
    n = A.size
    assert n == 2 * Mt * Mx
    rng = np.random.default_rng(n)
    x = np.vstack([seq(n), rng.uniform(-np.pi, np.pi, n)])
    # storage order [(j * Mt + i), mu] is the oracle's link map
    for i, j, mu in [(0, 0, 0), (1, 0, 1), (Mt - 1, Mx - 1, 0), (2, 3, 1)]:
        assert L.orc_link_cart2lin(Mt, Mx, i, j, mu) == 2 * (j * Mt + i) + mu
    P = ref.schwinger_plaquettes(x, Mt, Mx)
    F = ref.schwinger_force(x, Mt, Mx, beta)
    S = ref.schwinger_action(x, Mt, Mx, beta)
    plaq = ref.schwinger_avg_plaquette(x, Mt, Mx)
    chi = ref.schwinger_susceptibility(x, Mt, Mx)
    assert F.dtype == LD and S.dtype == LD
    assert np.all(ref.distance_to_branch_cut(x, Mt, Mx) > 1e-9)
    for b in range(2):
        raw = np.zeros(Mt * Mx)
        L.orc_schwinger_plaquettes(A.h, x[b], raw)
        assert np.max(np.abs(P[b] - raw)) <= 1e-14
        assert np.max(np.abs(F[b] - A.force(x[b]))) <= 1e-14 * beta * 4
        assert abs(S[b] - A.evaluate(x[b])) <= 1e-13 * max(1.0, float(S[b]))
        assert abs(plaq[b] - L.orc_qoi_avg_plaquette(x[b], Mt, Mx)) <= 1e-14
        assert abs(chi[b] - L.orc_qoi_2d_susceptibility(x[b], Mt, Mx)) <= 1e-10 * max(1.0, float(chi[b]))
        assert abs(chi[b] - np.rint(np.sqrt(chi[b])) ** 2) < 1e-12   # Q is an integer
    # a batch of one and a bare state give the same numbers as rows of a batch
    assert np.array_equal(ref.schwinger_force(x[1], Mt, Mx, beta), F[1])
    assert ref.schwinger_action(x[1], Mt, Mx, beta) == S[1]
    # the force rebuilt from given plaquettes is the force
    assert np.array_equal(ref.schwinger_force(None, Mt, Mx, beta, plaquettes=P), F)


def test_schwinger_force_is_the_gradient_of_the_action():
    """central differences in long double, h = 1e-6: truncation <= 2 beta h^2 / 6 = 4e-13 (two plaquettes per link),
    rounding <= n 2^-63 S / h with n = 20 terms and S <= 52: 1.1e-11"""
    Mt, Mx, beta = 5, 4, 1.3
    rng = np.random.default_rng(5)
    x = rng.uniform(-np.pi, np.pi, 2 * Mt * Mx).astype(LD)
    F = ref.schwinger_force(x, Mt, Mx, beta)
    h = LD(1e-6)
    for l in range(x.size):
        e = np.zeros_like(x)
        e[l] = h
        g = (ref.schwinger_action(x + e, Mt, Mx, beta) - ref.schwinger_action(x - e, Mt, Mx, beta)) / (2 * h)
        assert abs(g - F[l]) < 2e-11, (l, g, F[l])


@pytest.mark.parametrize("M,mass", GFF_SHAPES)
def test_gff_reference_equals_oracle(orc, M, mass):
    L = orc.lib()
    A = orc.Action(orc.GFF, Mt=M, Mx=M, mass=mass)
    n = A.size
    mu2 = L.orc_action_gff_mu2(A.h)
    rng = np.random.default_rng(n)
    x = np.vstack([seq(n), rng.uniform(-3, 3, n)])
    F = ref.gff_force(x, M, M, mu2)
    S = ref.gff_action(x, M, M, mu2)
    q = ref.phi_squared(x)
    for b in range(2):
        assert np.max(np.abs(F[b] - A.force(x[b]))) <= 1e-14 * (8 + mu2) * 3
        assert abs(S[b] - A.evaluate(x[b])) <= 1e-13 * max(1.0, abs(float(S[b])))
        assert abs(q[b] - L.orc_qoi_2d_phi_squared(x[b], n)) <= 1e-14 * max(1.0, float(q[b]))
    assert abs(ref.kinetic_energy(x[1]) - LD(n) * q[1] / 2) <= 1e-16 * n


def test_gff_force_is_the_gradient_of_the_action():
    M, mu2 = 5, 0.37
    rng = np.random.default_rng(6)
    x = rng.uniform(-3, 3, M * M).astype(LD)
    F = ref.gff_force(x, M, M, mu2)
    # the action is quadratic, so central differences are exact for any h; with h = 1 their rounding error is that of
    # the two actions, n * 2^-63 * |S| <= 25 * 1.1e-19 * 1e3 = 3e-15
    h = LD(1)
    for l in range(x.size):
        e = np.zeros_like(x)
        e[l] = h
        g = (ref.gff_action(x + e, M, M, mu2) - ref.gff_action(x - e, M, M, mu2)) / (2 * h)
        assert abs(g - F[l]) < 1e-14, (l, g, F[l])


@pytest.mark.parametrize("beta", [1.0, 2.5])
def test_reference_equals_the_reference_authors_python(orc, beta):
    """plaquettes (stored wrapped), and action / average plaquette / charge rebuilt from them as
    tests/test_reference_python_pins.py does for the oracle"""
    with open(os.path.join(HERE, "golden", "schwinger_ref_python.json")) as f:
        pins = json.load(f)
    assert len(pins["schwinger"]) == 9
    for case in pins["schwinger"]:
        m = case["m"]
        x = np.zeros(2 * m * m)
        for i, j, mu, v in case["links"]:
            x[2 * (j * m + i) + mu] = v
        want = np.zeros(m * m)
        for i, j, p in case["plaquettes"]:
            want[m * j + i] = p
        P = ref.schwinger_plaquettes(x, m, m)
        d = ref.mod_2pi(P - want)     # on the circle: a plaquette within rounding of +-pi may be stored either way
        assert np.max(np.abs(d)) < 1e-13, (m, case["field"])
        assert abs(ref.schwinger_action(x, m, m, beta) - beta * np.sum(1.0 - np.cos(want))) <= 1e-12 * beta * m * m
        assert abs(ref.schwinger_avg_plaquette(x, m, m) - np.cos(want).mean()) <= 1e-13
        Q = np.sum(want) / (2 * np.pi)
        assert abs(Q - round(Q)) < 1e-9
        if ref.distance_to_branch_cut(x, m, m) > 1e-9:
            assert abs(ref.schwinger_charge(x, m, m) - round(Q)) < 1e-12
            assert abs(ref.schwinger_susceptibility(x, m, m) - round(Q) ** 2) <= 1e-10 * max(1.0, Q * Q)
        F = ref.schwinger_force(x, m, m, beta)
        assert np.max(np.abs(F - ref.schwinger_force(None, m, m, beta, plaquettes=want))) <= 1e-13 * beta
