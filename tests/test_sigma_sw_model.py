"""CPU: the Swendsen-Wang multi-cluster update of the O(3) sigma model restated (tests/sigma_sw_model.py) -- the kernels'
partition of the links covers each link once, its components are those the Wolff model grows, the improved estimator's
identity, its law against the heat bath -- and the surface the feature adds to the C ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sigma_cluster_model as scm
import sigma_model as sm
import sigma_sw_model as swm
from conftest import zcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mlmcpi_sigma_sw_workspace_bytes", "mlmcpi_sigma_sw_draw"]


# ---- 1. the partition of the links -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(8, 8), (16, 16), (64, 32)])
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 6), (16, 16), (17, 9), (64, 32), (130, 70)])
def test_every_link_is_interior_to_one_tile_or_crossing_exactly_once(Mt, Mx, W, H):
    N = Mt * Mx
    nb, _, _ = scm.link_tables(Mt, Mx)
    interior, crossing = swm.tile_links(Mt, Mx, W, H)
    seen = np.zeros((N, 2), dtype=int)
    seen[interior >= 0] += 1
    for l, mu in crossing:
        seen[l, mu] += 1
    assert np.all(seen == 1), (np.argwhere(seen != 1)[:5], seen.sum(), 2 * N)
    assert np.count_nonzero(interior >= 0) + len(crossing) == 2 * N
    # an interior link has both ends in its tile, side by side (it does not wrap)
    l = np.arange(N)
    i, j = l % Mt, l // Mt
    tile = (j // H) * (-(-Mt // W)) + i // W
    for mu, d in enumerate((0, 2)):
        inside = interior[:, mu] >= 0
        y = nb[:, d]
        assert np.all(interior[inside, mu] == tile[inside]) and np.all(tile[y[inside]] == tile[inside])
        assert np.all(y[inside] == l[inside] + (1 if mu == 0 else Mt))


# ---- 2. the same component rule as the Wolff model -----------------------------------------------------------------------------
def _wolff_component(monkeypatch, phi, Mt, Mx, beta, r, U, s):
    """the component sigma_cluster_model grows from s on the bond set of (r, U)"""
    monkeypatch.setattr(scm, "reflection", lambda seed, chain, step, N: (r, s))
    monkeypatch.setattr(scm, "link_uniforms", lambda seed, chain, step, N: U)
    return scm.dev_update(phi, Mt, Mx, beta, 0, 0, 0)[1]["sites"]


@pytest.mark.parametrize("Mt,Mx,seeds,every", [(6, 4, [5], True), (16, 16, list(range(100, 132)), False)])
def test_clusters_are_the_components_the_wolff_model_grows(monkeypatch, Mt, Mx, seeds, every):
    N, beta, chain, step = Mt * Mx, 1.5, 2, 7
    sizes = []
    for seed in seeds:
        phi = sm.sweep_draw(sm.initialise(1, Mt, Mx, seed), Mt, Mx, beta, 0, 6, seed=seed)[0]
        _, info = swm.dev_update(phi, Mt, Mx, beta, seed, chain, step)
        U = swm.link_uniforms(seed, chain, step, N)
        lab = info["labels"]
        for s in (range(N) if every else [int(sm.uniforms(seed, 0, 0, 0, 6)[0] * N)]):
            want = _wolff_component(monkeypatch, phi, Mt, Mx, beta, info["r"], U, s)
            got = np.nonzero(lab == lab[s])[0]
            assert np.array_equal(got, want), (seed, s)
            assert lab[s] == want.min()
            sizes.append(len(want))
    assert max(sizes) > 1


def test_batched_model_equals_the_single_chain_model():
    Mt, Mx, beta, B = 4, 6, 1.5, 5
    phi = sm.initialise(B, Mt, Mx, 9)
    for step in range(8):
        new, info = swm.dev_update_batch(phi, Mt, Mx, beta, 21, 3, step)
        for b in range(B):
            one, i1 = swm.dev_update(phi[b], Mt, Mx, beta, 21, 3 + b, step)
            assert np.array_equal(one, new[b])
            assert info["flipped"][b] == len(i1["flipped"]) and info["clusters"][b] == i1["clusters"]
            assert abs(info["improved"][b] - i1["improved"]) <= 1e-13 * i1["improved"]
        phi = new


# ---- 3. the estimator identity ---------------------------------------------------------------------------------------------------
def test_mean_of_the_projected_magnetisation_over_the_coins_is_the_sum_of_squares():
    """4 x 4, 20 fields and normals: the mean of (M' . r)^2 over all 2^{n_C} flip patterns, M' the magnetisation of the field
    with those clusters reflected, equals sum_C A_C^2"""
    Mt = Mx = 4
    N, beta = 16, 1.0
    for n in range(20):
        seed = 40 + n
        phi = sm.sweep_draw(sm.initialise(1, Mt, Mx, seed), Mt, Mx, beta, 0, 3, seed=seed)[0]
        _, info = swm.dev_update(phi, Mt, Mx, beta, seed, 1, n)
        lab, a, r = info["labels"], info["a"], info["r"]
        roots = np.unique(lab)
        nC = len(roots)
        assert nC <= 16
        sig = sm.sigma_of(phi.reshape(N, 2))
        pattern = (np.arange(1 << nC)[:, None] >> np.arange(nC)[None, :]) & 1                # [P, n_C]
        flip = pattern[:, np.searchsorted(roots, lab)].astype(np.float64)                    # [P, N]
        Mp = (sig[None] - 2.0 * (flip * a[None])[..., None] * r[None, None, :]).sum(axis=1)  # [P, 3]
        mean = float(np.mean((Mp @ r) ** 2))
        A = np.array([a[lab == c].sum() for c in roots])
        assert abs(mean - float((A * A).sum())) < 1e-12, (n, nC, mean, float((A * A).sum()))
        # and the fixed-point value is that sum x 3 / N
        assert abs(info["improved"] - 3.0 * float((A * A).sum()) / N) < 1e-8


# ---- 4. the law ------------------------------------------------------------------------------------------------------------------
def _sw_chain(seed, B, burn, meas, Mt, Mx, beta):
    phi = sm.initialise(B, Mt, Mx, seed)
    chi, imp = [], []
    for step in range(burn + meas):
        phi, info = swm.dev_update_batch(phi, Mt, Mx, beta, seed + 1, 0, step)
        if step >= burn:
            chi.append(sm.magnetic_susceptibility(phi, Mt, Mx))
            imp.append(info["improved"])
    c, i = np.mean(chi, axis=0), np.mean(imp, axis=0)
    se = lambda x: float(x.std(ddof=1) / math.sqrt(B))  # noqa: E731
    return float(c.mean()), se(c), float(i.mean()), se(i)


def test_swendsen_wang_samples_the_heat_bath_law_and_the_improved_estimator_is_unbiased():
    """4 x 4, beta = 1, 64 chains x 3000 updates after 500: chi_m and the improved value agree with sigma_model's heat bath;
    the improved value agrees with the plain chi_m of OTHER chains (the two estimators of one chain are correlated).  The
    eight-neighbour walk's 12.03 would be more than a hundred sigma away."""
    Mt = Mx = 4
    beta, B = 1.0, 64
    chi, chi_err, imp, imp_err = _sw_chain(5, B, 500, 3000, Mt, Mx, beta)
    chi2, chi2_err, _, _ = _sw_chain(15, B, 500, 3000, Mt, Mx, beta)
    phi = sm.initialise(B, Mt, Mx, 7)
    h = []
    for s in range(3500):
        phi = sm.sweep_draw(phi, Mt, Mx, beta, 0, 1, seed=8, sweep0=s)
        if s >= 500:
            h.append(sm.magnetic_susceptibility(phi, Mt, Mx))
    h = np.mean(h, axis=0)
    heat, heat_err = float(h.mean()), float(h.std(ddof=1) / math.sqrt(B))
    zcheck("sigma SW model vs heat-bath model chi_m 4x4 beta=1", chi, chi_err, heat, heat_err)
    zcheck("sigma SW model improved chi_m vs heat-bath model chi_m 4x4 beta=1", imp, imp_err, heat, heat_err)
    zcheck("sigma SW model improved chi_m vs plain chi_m of other SW chains 4x4 beta=1", imp, imp_err, chi2, chi2_err)
    print(f"distance of the eight-neighbour value 12.03: {(12.03 - chi) / chi_err:.0f} sigma")


# ---- 5. surface ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in abi.SIGNATURES
    assert lib.mlmcpi_abi_version() == 1


def test_unsupported_kinds_invalid_arguments_and_no_device():
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    size = C.c_size_t(0)
    for kind in (abi.GFF, abi.SCHWINGER):
        act = abi.lattice_action(kind, 8, 8, beta=1.0, mass=1.0)
        assert lib.mlmcpi_sigma_sw_workspace_bytes(C.byref(act), 1, C.byref(size)) == -3
        assert lib.mlmcpi_sigma_sw_draw(C.byref(act), None, 1, 1, 1, 0, 0, None, None, None, None, None) == -3
        assert b"sigma" in lib.mlmcpi_last_error()
    act = abi.lattice_action(abi.NONLINEAR_SIGMA, 6, 10, beta=1.0)
    assert lib.mlmcpi_sigma_sw_workspace_bytes(C.byref(act), 3, C.byref(size)) == 0
    assert size.value >= 3 * 60 * 21      # label, q(a), cluster sum and bond bits of every vertex
    buf = (C.c_double * 120)()
    work = (C.c_char * size.value)()
    # update0 + n_updates beyond 32 bits: MLMCPI_ERR_INVALID, before anything is launched
    assert lib.mlmcpi_sigma_sw_draw(C.byref(act), buf, 1, 2, 1, 0, 0xFFFFFFFF, None, None, None, work, None) == -1
    assert b"overflow" in lib.mlmcpi_last_error()
    assert lib.mlmcpi_sigma_sw_draw(C.byref(act), buf, 1, 1, 1, 0, 0, None, None, None, None, None) == -1   # no workspace
    for Mt, Mx in ((1, 8), (8, 1), (1 << 16, 1 << 15)):                                                      # too small, too large
        bad = abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=1.0)
        assert lib.mlmcpi_sigma_sw_workspace_bytes(C.byref(bad), 1, C.byref(size)) == -1
        assert lib.mlmcpi_sigma_sw_draw(C.byref(bad), buf, 1, 1, 1, 0, 0, None, None, None, work, None) == -1
    if not torch.cuda.is_available():
        # no silent CPU path: with valid arguments and no device the launch fails with the runtime's no-device error
        rc = lib.mlmcpi_sigma_sw_draw(C.byref(act), buf, 1, 1, 1, 0, 0, None, None, None, work, None)
        assert rc in (-2, -4), rc
        assert all(v == 0.0 for v in buf) and not any(work.raw)
