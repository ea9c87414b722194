"""CPU: the cooling model of tests/sigma_cooling_reference.py -- its tables against sigma_level_model.Level, the input conditions
of every GPU comparison, and the invariants of the definition (the energy never rises, the uniform field is a fixed point, the
instanton and dislocation tables, depth lists)."""
import numpy as np
import pytest

import sigma_cooling_reference as ref
import sigma_level_model as slm
import sigma_topology_reference as topo

SMALL = [k for k in ref.gpu_cases() if k[3] not in (topo.BIG_CHAINS, topo.EDGE_CHAINS)]
_id = lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3])   # noqa: E731


@pytest.mark.parametrize("Mt,Mx", topo.PARITY_SHAPES + [(8, 8), (16, 16)])
@pytest.mark.parametrize("rot", [False, True])
def test_tables_are_those_of_the_level_model(Mt, Mx, rot):
    L = slm.Level(Mt, Mx, rot)
    assert np.array_equal(ref.neighbours(Mt, Mx, rot), L.nbr)
    i, j = ref.coords(Mt, Mx, rot)
    assert list(zip(i.tolist(), j.tolist())) == [tuple(c) for c in L.coords]
    # the halves of sigma_level_model.sweep
    want = ([np.arange(L.n // 2), np.arange(L.n // 2, L.n)] if rot else
            [np.array([l for l, (a, b) in enumerate(L.coords) if (a + b) % 2 == p]) for p in (0, 1)])
    for got, w in zip(ref.phases(Mt, Mx, rot), want):
        assert np.array_equal(got, w)


def test_every_gpu_case_has_a_seed():
    assert set(ref.SEEDS) == set(ref.gpu_cases())


@pytest.mark.parametrize("key", ref.gpu_cases(), ids=_id)
def test_input_conditions(key):
    """min |Delta| >= 1e-3 over all updates and charge margin >= 1e-6 at every listed depth, for every GPU comparison input"""
    _, c = ref.gpu_case(*key)
    print(f"{_id(key)}: min |Delta| = {c.min_delta:.3g}, margin = {c.margin.min():.3g}, dev64 = {c.dev64.max():.3g}")
    assert c.min_delta >= ref.MIN_DELTA
    assert c.margin.min() >= ref.MIN_MARGIN
    # float64 stays with longdouble closely enough that the bounds built on it can still tell one charge from the next
    assert c.q_bound().max() < 0.01 and c.e_bound().max() < 1e-6 * c.n


@pytest.mark.parametrize("key", SMALL, ids=_id)
def test_energy_never_rises(key):
    _, c = ref.gpu_case(*key)
    assert np.all(np.diff(c.E.astype(np.float64), axis=1) <= 1e-12 * c.n)
    assert np.all(c.E >= -1e-12 * c.n)


@pytest.mark.parametrize("rot", [False, True])
def test_uniform_field_is_a_fixed_point(rot):
    for Mt, Mx in topo.PARITY_SHAPES:
        n = ref.n_vertices(Mt, Mx, rot)
        phi = np.tile(np.array([0.7, -1.1]), (2, n))
        c = ref.cool(Mt, Mx, rot, phi, [0, 1, 5])
        assert np.all(np.abs(c.Q) < 1e-15) and np.all(np.abs(c.E) < 1e-15 * n)
        assert np.abs(c.sig - ref.sigma_of(phi, n, ref.LD)).max() < 1e-18


@pytest.mark.parametrize("k", [1, 2])
def test_instantons_on_the_plain_level_keep_their_charge(k):
    Q, E = ref.instanton_table(16, 16, False, 3.0, k)
    assert np.all(np.rint(Q) == k), Q
    assert np.all(np.diff(E) <= 1e-12) and E[-1] >= k * 0.5


@pytest.mark.parametrize("k", [1, 2])
def test_instantons_on_the_rotated_level_are_cooled_away(k):
    """a lattice artefact of the coarser frame: the charge survives a few sweeps, then falls to 0"""
    Q, E = ref.instanton_table(16, 16, True, 3.0, k)
    r = np.rint(Q)
    assert r[0] == k and r[1] == k and r[-1] == 0, Q
    assert np.all(np.diff(r) <= 0), Q


# E_0 / 4 pi of the (4, 4, lambda = 1) dislocation in the longdouble model: the issue's "1.2 - 1.3", pinned per layout
DISLOCATION_E0 = {False: 1.3009, True: 1.1993}


@pytest.mark.parametrize("rot", [False, True])
def test_the_dislocation_is_removed(rot):
    Q, E = ref.instanton_table(4, 4, rot, 1.0, 1)
    assert np.rint(Q[0]) == 1 and np.all(np.rint(Q[2:]) == 0), Q
    print(f"dislocation, {'rotated' if rot else 'plain'}: E_0 / 4 pi = {E[0]:.6f}")
    assert abs(E[0] - (DISLOCATION_E0[rot])) < 5e-4 and E[-1] < 1e-3, E


@pytest.mark.parametrize("rot", [False, True])
def test_depth_lists(rot):
    """Q_d, E_d and the field from [d] are those from any list containing d"""
    phi = topo.uniform_spins(6, 4, rot, 5, seed=99)
    full = ref.cool(6, 4, rot, phi, [0, 1, 2, 5])
    for k, d in enumerate(full.depths):
        one = ref.cool(6, 4, rot, phi, [d])
        assert np.array_equal(one.Q[:, 0], full.Q[:, k]) and np.array_equal(one.E[:, 0], full.E[:, k])
    assert np.array_equal(ref.cool(6, 4, rot, phi, [5]).sig, full.sig)
    assert np.array_equal(ref.cool(6, 4, rot, phi, [2, 5]).Q[:, 1], full.Q[:, 3])


def test_depth_zero_is_the_charge_reference():
    phi = topo.uniform_spins(6, 4, True, 5, seed=7)
    c0, c = topo.charge(6, 4, True, phi), ref.cool(6, 4, True, phi, [0])
    assert np.array_equal(c0.Q, c.Q[:, 0]) and np.array_equal(c0.margin, c.margin[:, 0])
    assert np.allclose(np.asarray(slm.evaluate(slm.Level(6, 4, True, 1.0), phi)), -(2 * c.n - c.E[:, 0]).astype(np.float64), rtol=0, atol=1e-12)
