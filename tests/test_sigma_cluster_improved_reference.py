"""CPU: the improved estimators of the Wolff single-cluster update as tests/sigma_cluster_improved_reference.py states them: the
mean over all seed vertices against the Swendsen-Wang improved estimators of the same labels, the two identities on the clusters
of the Wolff models, the device's integers inside the bounds, the scale of the accumulators, and the new symbols."""
import math
import os
import re

import numpy as np
import pytest

import sigma_cluster_improved_reference as wir
import sigma_correlator_reference as cref
import sigma_level_cluster_model as slcm
import sigma_level_model as slm
import sigma_level_sw_model as slsw
import sigma_sw_correlator_reference as scr
import sigma_sw_structure_reference as ssr

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mlmcpi_sigma_level_cluster_improved_workspace_bytes", "mlmcpi_sigma_level_cluster_improved_draw"]
REGIMES = [("singletons", 0.05), ("mixed", 1.5), ("spanning", 8.0)]


def _cold(L):
    phi = np.empty(2 * L.n)
    phi[0::2], phi[1::2] = 0.5 * math.pi, 0.25
    return phi


def _start(L, seed, regime):
    if regime == "spanning":
        return _cold(L)
    if regime == "singletons":
        return slm.initialise(L, 1, seed)[0]
    return slm.sweep_draw(L, slm.initialise(L, 1, seed), 10, 1, seed)[0]


def _wolff_cluster(L, seed, regime):
    """(a, members) of a Wolff model update in one of the three regimes"""
    phi = _start(L, seed, regime)
    for s in range(seed, seed + 50):                      # spanning: the first seed whose normal is not nearly orthogonal to the spins
        _, info = slcm.dev_update(L, phi, s, 0, 0)
        if regime != "spanning" or len(info["sites"]) > L.n // 2:
            return wir.dots(L, phi, info["r"]), info["sites"]
    raise AssertionError("no spanning cluster")


# ---- 1. the mean over the seeds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.05, 1.5, 8.0])
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 4), (16, 16)])
def test_the_mean_over_all_seeds_is_the_swendsen_wang_improved_estimator(Mt, Mx, rot, beta):
    """a fixed field, normal and bond configuration (the Swendsen-Wang model's update): every vertex in turn is the seed, its
    cluster is its label's; the mean of chi^W, F^W and C^W over the n seeds against 3 sum_C A_C^2 / n, ssr.improved and scr.improved"""
    L = slm.Level(Mt, Mx, rot, beta)
    phi = _cold(L) if beta == 8.0 else slm.sweep_draw(L, slm.initialise(L, 1, 7 + Mt), 10, 1, 7 + Mt)[0]
    info = slsw.dev_update(L, phi, 7 + Mx, 0, 0)[1]
    a, lab = info["a"], info["labels"]
    chi, F, C = wir.seed_average(L, a, lab)
    a_ld = np.asarray(a, dtype=np.float64).astype(LD)
    want_chi = LD(3) * sum(a_ld[lab == c].sum() ** 2 for c in np.unique(lab)) / LD(L.n)
    tol = 1e-17 * L.n
    assert abs(chi - want_chi) <= tol * max(1.0, float(want_chi))
    for d in range(2):
        assert abs(F[d] - ssr.improved(L, a, lab, d)) <= tol * max(1.0, float(want_chi)), d
    assert np.all(np.abs(C - scr.improved(L, a, lab)) <= tol * max(1.0, float(want_chi)))


# ---- 2. the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,beta", REGIMES)
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (6, 2), (4, 4), (16, 16), (66, 34)])
def test_the_weighted_sums_are_chi_and_the_structure_factor(Mt, Mx, rot, regime, beta):
    """sum_tau w C_d^W = chi^W and sum_tau w C_d^W cos(2 pi tau / M_d) = F_d^W on the cluster of the Wolff model's update; the
    device's integers (device_model) within the bounds of the reference, whatever the order of the queue"""
    L = slm.Level(Mt, Mx, rot, beta)
    a, members = _wolff_cluster(L, 11 + Mx, regime)
    if regime == "singletons":
        assert len(members) == 1
        assert abs(float(wir.estimators(L, a, members)[0]) - 3.0 * a[members[0]] ** 2) <= 1e-15
    if regime == "spanning":
        assert len(members) > L.n // 2
    chi, F, C = wir.estimators(L, a, members)
    Ct, Cx = cref.split(C[None, :], Mt, Mx)
    for d, (Cd, M) in enumerate(((Ct[0], Mt), (Cx[0], Mx))):
        w = cref.weights(M).astype(LD)
        cos = wir.slice_phases(M)[0][:M // 2 + 1]
        assert abs((w * Cd).sum() - chi) <= 1e-15 * max(1.0, float(chi)), d
        assert abs((w * Cd * cos).sum() - F[d]) <= 1e-15 * max(1.0, float(chi)), d
    if L.n <= 600:
        got = wir.device_model(L, a, members)
        assert abs(got[0] - float(chi)) <= wir.susceptibility_bound(L, a, members)
        for d in range(2):
            assert abs(got[1][d] - float(F[d])) <= wir.structure_bound(L, a, members, d), d
        assert np.all(np.abs(got[2] - C.astype(np.float64)) <= wir.device_bound(L, a, members))
        order = np.random.default_rng(Mt).permutation(len(members))
        again = wir.device_model(L, a, members, order)
        assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2])


# ---- 3. the accumulators ----------------------------------------------------------------------------------------------------
def test_the_scale_keeps_the_accumulator_inside_63_bits():
    """the arithmetic of s up to n = 2^30: one cluster's sum_i |P(i)| |P(i + tau)| <= n n_slice (|a| <= 1, at most n_slice members a
    slice, n members in all), in units of 2^-s, plus half a unit per term, and the slice table itself: n 2^32 <= 2^62"""
    for Mt, Mx, rot in [(2, 2, True), (16, 16, False), (1024, 1024, True), (1024, 1024, False), (32768, 32768, False), (2, 2 ** 29, False),
                        (2 ** 15, 2 ** 16, True)]:
        L = slm.Level.__new__(slm.Level)
        L.Mt, L.Mx, L.rotated, L.n = Mt, Mx, rot, (Mt * Mx // 2 if rot else Mt * Mx)
        assert L.n <= 2 ** 30
        s = wir.scale_bits(L)
        n_slice = L.n // min(Mt, Mx)
        assert 0 <= s <= 32 and L.n * n_slice * 2 ** s + L.n <= 2 ** 63 - 1
        assert s == 32 or L.n * n_slice * 2 ** (s + 1) > 2 ** 62
        assert L.n * 2 ** 32 + L.n <= 2 ** 63 - 1


# ---- 4. surface -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in abi.SIGNATURES
    assert lib.mlmcpi_abi_version() == 1
    assert callable(ops.sigma_level_cluster_improved_workspace) and callable(ops.sigma_level_cluster_improved_draw)


def test_refusals_need_no_device():
    import ctypes as C
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    size, plain = C.c_size_t(0), C.c_size_t(0)
    ws, draw = lib.mlmcpi_sigma_level_cluster_improved_workspace_bytes, lib.mlmcpi_sigma_level_cluster_improved_draw
    assert ws(None, 1, C.byref(size)) == -1
    assert draw(None, None, 1, 1, 1, 0, 0, None, None, None, None, None, 0, None) == -1
    for rot in (0, 1):
        for Mt, Mx, beta in ((3, 8, 1.0), (8, 5, 1.0), (0, 8, 1.0), (8, 8, 0.0), (8, 8, -1.0)):
            bad = abi.sigma_level(Mt, Mx, rot, beta)
            assert ws(C.byref(bad), 1, C.byref(size)) == -1, (rot, Mt, Mx, beta)
        lv = abi.sigma_level(6, 10, rot, 1.0)
        assert ws(C.byref(lv), 0, C.byref(size)) == -1
        assert ws(C.byref(lv), 3, C.byref(size)) == 0
        assert lib.mlmcpi_sigma_level_cluster_workspace_bytes(C.byref(lv), 3, C.byref(plain)) == 0
        a256 = lambda v: -(-v // 256) * 256  # noqa: E731
        n_out = cref.n_out(6, 10)
        assert size.value == plain.value + a256(3 * 16 * 8) + a256(3 * (5 + n_out) * 8) + a256(3 * 16 * 4) + a256(3 * 16 * 16)
        assert draw(C.byref(lv), None, 3, 1, 1, 0, 0, None, None, None, None, None, size.value, None) == -1
