"""CPU: the long-double reference of the GFF slice correlators (tests/gff_correlator_reference.py) against fields whose
correlators can be written down by hand, Parseval over all momenta, the exact law (mode sum against the closed cosh form, the
effective mass against the dispersion relation), and the host plan query and refusals of the library against the restated plan."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gff_correlator_reference as ref

LD = ref.LD


def _field(fn, Mt, Mx, rotated):
    i, j = ref.coordinates(Mt, Mx, rotated)
    return np.asarray(fn(i.astype(LD), j.astype(LD)), dtype=LD)[None, :]


@pytest.mark.parametrize("rotated", [False, True])
def test_coordinates_are_the_layouts_of_the_header(rotated):
    Mt, Mx = 6, 4
    i, j = ref.coordinates(Mt, Mx, rotated)
    assert len(i) == ref.n_vertices(Mt, Mx, rotated) and len(set(zip(i, j))) == len(i)
    if rotated:
        assert ((i + j) % 2 == 0).all()
        assert (i[0], j[0]) == (0, 0) and (i[1], j[1]) == (2, 0) and (i[3], j[3]) == (0, 2) and (i[6], j[6]) == (1, 1) and (i[7], j[7]) == (3, 1)
    else:
        assert (i[1], j[1]) == (1, 0) and (i[Mt], j[Mt]) == (0, 1)


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (4, 6), (8, 8)])
def test_constant_field(Mt, Mx):
    """only q = 0 survives: C_t(tau; 0) = Mx c^2, C_x(tau; 0) = Mt c^2 unrotated; a rotated level has half the vertices in every slice:
    (Mx/2)^2 Mt c^2 / (Mt Mx / 2) = Mx c^2 / 2, and its momentum Mx/2 (e^{-i pi j} = the parity of the slice) alternates with the lag"""
    c, P = LD(1.75), min(Mt, Mx) // 2 + 1
    for rotated in (False, True):
        Ct, Cx = ref.split(ref.correlator(_field(lambda i, j: c + 0 * i, Mt, Mx, rotated), Mt, Mx, P, rotated)[0], Mt, Mx, P)
        h = 2 if rotated else 1
        assert np.abs(Ct[0] - Mx * c * c / h).max() <= 1e-17 * Mx and np.abs(Cx[0] - Mt * c * c / h).max() <= 1e-17 * Mt
        for q in range(1, P):
            if rotated and 2 * q == Mx:
                assert np.abs(Ct[q] - (Mx * c * c / 2) * (-1.0) ** np.arange(Mt // 2 + 1)).max() <= 1e-17 * Mx
            else:
                assert np.abs(Ct[q]).max() <= 1e-17 * Mx
            if not (rotated and 2 * q == Mt):
                assert np.abs(Cx[q]).max() <= 1e-17 * Mt


@pytest.mark.parametrize("Mt,Mx,k,q0", [(8, 8, 1, 2), (6, 10, 2, 3), (16, 4, 3, 1)])
def test_plane_wave_lands_in_one_momentum(Mt, Mx, k, q0):
    """phi = cos(2 pi (k i / Mt + q0 j / Mx)), 0 < q0 < Mx/2: S^t_i(q0) = (Mx/2) e^{2 pi i k i / Mt}, so C_t(tau; q0) =
    (Mx/4) cos(2 pi k tau / Mt) and every other momentum q <= Mx/2 is empty; along x the wave sits in momentum k likewise"""
    P = min(Mt, Mx) // 2 + 1
    phi = _field(lambda i, j: np.cos(2 * ref.PI * (k * i / Mt + q0 * j / Mx)), Mt, Mx, False)
    Ct, Cx = ref.split(ref.correlator(phi, Mt, Mx, P)[0], Mt, Mx, P)
    for q in range(P):
        want = LD(Mx) / 4 * np.cos(2 * ref.PI * k * np.arange(Mt // 2 + 1) / Mt) if q == q0 else 0
        assert np.abs(Ct[q] - want).max() <= 1e-17 * Mx, q
        want = LD(Mt) / 4 * np.cos(2 * ref.PI * q0 * np.arange(Mx // 2 + 1) / Mx) if q == k else 0
        assert np.abs(Cx[q] - want).max() <= 1e-17 * Mt, q


@pytest.mark.parametrize("rotated", [False, True])
def test_single_spike(rotated):
    """one vertex of value v: |S|^2 = v^2 in its own slice at every momentum, so C(0; q) = v^2 / N and C(tau > 0; q) = 0"""
    Mt, Mx, P, v = 6, 8, 4, 3.0
    n = ref.n_vertices(Mt, Mx, rotated)
    phi = np.zeros((1, n))
    phi[0, n - 2] = v
    Ct, Cx = ref.split(ref.correlator(phi, Mt, Mx, P, rotated)[0], Mt, Mx, P)
    for Cd in (Ct, Cx):
        assert np.abs(Cd[:, 0] - LD(v * v) / n).max() <= 1e-18 and np.abs(Cd[:, 1:]).max() <= 1e-18


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (4, 6), (8, 8)])
def test_parseval_over_all_momenta(Mt, Mx):
    """sum_q w_q C_t(0; q) = Mx (1/N) sum phi^2 with the momenta 0 .. Mx/2, those that are not their own conjugate counted twice; the
    reference itself is run at P = Mx (it has no cap) and both ways of counting agree"""
    rng = np.random.default_rng(5)
    phi = rng.standard_normal((2, Mt * Mx))
    P = Mx
    F = ref.grid(phi, Mt, Mx, False)
    St, _ = ref.slice_sums(F, P)
    Ct0 = (St[0] ** 2 + St[1] ** 2).sum(axis=2) / (Mt * Mx)      # C_t(0; q), q < Mx
    want = Mx * (phi.astype(LD) ** 2).sum(axis=1) / (Mt * Mx)
    assert np.abs(Ct0.sum(axis=1) - want).max() <= 1e-17 * Mx
    w = np.array([1 if q == 0 or 2 * q == Mx else 2 for q in range(Mx // 2 + 1)])
    assert np.abs((w * Ct0[:, :Mx // 2 + 1]).sum(axis=1) - want).max() <= 1e-17 * Mx


@pytest.mark.parametrize("Mt,Mx", [(16, 16), (64, 32)])
@pytest.mark.parametrize("mass", [1.0, 8.0])
def test_mode_sum_is_the_closed_cosh_form(Mt, Mx, mass):
    """A mode sum of terms of the size of C(0) carries an absolute error of a few ulp of C(0), 1e-18 C(0) in long double.  At q = 0
    (E Mt / 2 <= 4 on these shapes) 1e-13 relative holds at every lag; at q > 0 the law falls by up to e^(-E Mt / 2) = 2e-8 across
    the lags (1.7e-13 relative was seen at (64, 32), mass 1, q = 3, tau = 31), so there the deviation is taken relative to C(0; q)."""
    for q in range(min(Mx // 2 + 1, 8)):
        C = np.array([ref.correlator_exact(Mt, Mx, mass, q, tau) for tau in range(Mt // 2 + 1)])
        closed = np.array([ref.correlator_closed(Mt, Mx, mass, q, tau) for tau in range(Mt // 2 + 1)])
        if q == 0:
            assert np.abs(C / closed - 1).max() <= 1e-13, (q, np.abs(C / closed - 1).max())
        assert np.abs(C - closed).max() <= 1e-17 * closed[0], (q, np.abs(C - closed).max() / closed[0])
        E = ref.dispersion_exact(Mt, Mx, mass, q)
        for tau in range(1, Mt // 2):
            assert abs(ref.effective_mass(closed, tau) - E) <= 1e-13, (q, tau)     # long double: three values to 1e-19, over sinh E >= 0.015


# ---- the library's host side ----

def test_abi_symbols_exist():
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    for name in ("mlmcpi_gff_correlator_size", "mlmcpi_gff_correlator_workspace_bytes", "mlmcpi_gff_correlator", "mlmcpi_gff_correlator_plan"):
        assert hasattr(lib, name) and name in abi.SIGNATURES
    assert ref.MAX_MOMENTA == 8


def test_plan_query_is_the_restated_plan():
    from mlmcpathintegral_amd import abi, ops
    checked = 0
    for Mt, Mx in itertools.product(range(2, 71, 2), repeat=2):
        for rotated in (0, 1):
            for P in range(1, min(8, Mt // 2 + 1, Mx // 2 + 1) + 1):
                B = 1 + (Mt + 3 * Mx + P) % 7
                got = ops.gff_correlator_plan(Mt, Mx, P, rotated, B)
                assert got == ref.plan(Mt, Mx, rotated, P, B), (Mt, Mx, rotated, P, B, got)
                checked += 1
    assert checked > 10000
    for Mt, Mx, rotated, P, B in [(1024, 1024, 0, 8, 32), (1024, 1024, 1, 1, 2), (130, 514, 1, 5, 70), (8192, 64, 0, 8, 3), (4096, 4098, 0, 2, 1)]:
        assert ops.gff_correlator_plan(Mt, Mx, P, rotated, B) == ref.plan(Mt, Mx, rotated, P, B)
        nbytes = C.c_size_t(0)
        abi.call("mlmcpi_gff_correlator_workspace_bytes", Mt, Mx, rotated, P, B, C.byref(nbytes))
        assert nbytes.value == ref.plan(Mt, Mx, rotated, P, B)["work_bytes"]
        assert ops.gff_correlator_size(Mt, Mx, P, rotated) == ref.n_out(Mt, Mx, P)
    assert ref.plan(8192, 64, 0, 8)["lags_in_lds"] == 0 and ref.plan(4096, 64, 0, 8)["lags_in_lds"] == 1
    assert ref.plan(1024, 1024, 0, 8)["lds_bytes"] <= 65536


def test_shapes_of_the_gpu_test_span_bands_and_chunks():
    """what tests/test_gff_correlator_gpu.py relies on: with bands of 256 rows and chunks of 64 columns the issue's (66, 34) and
    (130, 70) span several chunks but one band, so (130, 514) is there: the smallest even extents whose rotated planes (65 x 257)
    and plain plane both pass one band and one chunk; 1024^2 does in both layouts"""
    for Mt, Mx in [(130, 514), (1024, 1024)]:
        for rotated in (0, 1):
            p = ref.plan(Mt, Mx, rotated, 1)
            assert p["bands"] > 1 and p["chunks"] > 1, (Mt, Mx, rotated, p)
    assert ref.plan(128, 514, 1, 1)["chunks"] == 1 and ref.plan(130, 512, 1, 1)["bands"] == 1
    assert ref.plan(66, 34, 0, 1)["chunks"] == 2 and ref.plan(130, 70, 0, 1)["chunks"] == 3 and ref.plan(130, 70, 1, 1)["chunks"] == 2
    assert {ref.plan(66, 34, 1, 1)["vector_loads"], ref.plan(130, 70, 1, 1)["vector_loads"], ref.plan(16, 16, 1, 1)["vector_loads"]} == {0, 1}


REFUSALS = [  # (Mt, Mx, rotated, P, n_chains), status, part of the message
    ((3, 4, 0, 1, 1), -1, "even extents"), ((4, 0, 0, 1, 1), -1, "even extents"), ((4, 5, 1, 1, 1), -1, "even extents"),
    ((1 << 16, 1 << 15, 0, 1, 1), -1, "too large"), ((4, 4, 0, 0, 1), -1, "at least one momentum"), ((4, 16, 0, 4, 1), -1, "more than"),
    ((16, 4, 0, 4, 1), -1, "more than"), ((2, 2, 1, 3, 1), -1, "more than"), ((64, 64, 0, 9, 1), -3, "up to 8 momenta"),
    ((4, 4, 0, 1, 0), -1, "n_chains > 0"),
]


@pytest.mark.parametrize("args,status,message", REFUSALS)
def test_host_refusals(args, status, message):
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    info, nbytes = abi.GffCorrelatorPlan(), C.c_size_t(7)
    want = status                                          # MLMCPI_ERR_INVALID = -1, MLMCPI_ERR_UNSUPPORTED = -3
    assert lib.mlmcpi_gff_correlator_plan(*args, C.byref(info)) == want
    assert message in lib.mlmcpi_last_error().decode()
    assert lib.mlmcpi_gff_correlator_workspace_bytes(*args, C.byref(nbytes)) == want and nbytes.value == 7
    # the call itself refuses on the host, before any device is touched
    assert lib.mlmcpi_gff_correlator(*args[:4], None, args[4], None, None, None, 0, None) == want
    if args[4]:
        n = C.c_uint32(7)
        assert lib.mlmcpi_gff_correlator_size(*args[:4], C.byref(n)) == want and n.value == 7
