"""CPU: the Swendsen-Wang multi-cluster update of the O(3) sigma model on a rotated level restated
(tests/sigma_level_sw_model.py) -- the link naming agrees with the level's neighbour table, the tiles' interior links and the
merge launch's crossing links partition the 2 n links, the labels are those of a sequential union-find, an unrotated Level is
the unrotated model, it samples the law of the rotated heat bath and its improved estimator is unbiased -- and the surface the
feature adds to the C ABI and to host/driver."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sigma_level_cluster_model as slcm
import sigma_level_model as slm
import sigma_level_sw_model as slsw
import sigma_model as sm
import sigma_sw_model as swm
from conftest import zcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mlmcpi_sigma_level_sw_workspace_bytes", "mlmcpi_sigma_level_sw_draw"]
LEVELS = [(2, 2), (2, 6), (4, 6), (16, 16), (66, 34)]


# ---- 1. link naming and the partition of the links over tiles ------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", LEVELS)
def test_plane_arithmetic_of_the_link_naming_agrees_with_the_neighbour_table(Mt, Mx):
    """link (e, d) ends at L.nbr[e, d]; from its O end y it is direction 3 - d (the tables of the level Wolff model); every O
    vertex is the end of exactly four links, also where several of them come from one E vertex (plane extents of 1)"""
    L = slm.Level(Mt, Mx, True)
    nE = L.n // 2
    site, which = slcm.link_tables(L)
    ends = np.zeros(L.n, dtype=int)
    for e in range(nE):
        for d in range(4):
            y = slsw.plane_link(L, e, d)
            assert y == L.nbr[e, d] and nE <= y < L.n, (e, d, y)
            assert (site[e, d], which[e, d]) == (e, d)
            assert L.nbr[y, 3 - d] == e and (site[y, 3 - d], which[y, 3 - d]) == (e, d)
            ends[y] += 1
    assert np.all(ends[nE:] == 4) and np.all(ends[:nE] == 0)
    if (Mt, Mx) == (2, 2):
        assert [slsw.plane_link(L, 0, d) for d in range(4)] == [1, 1, 1, 1]     # four links between the only two vertices


@pytest.mark.parametrize("W,H", [(8, 8), (64, 32)])
@pytest.mark.parametrize("Mt,Mx", LEVELS + [(130, 70)])
def test_every_link_is_interior_to_one_tile_or_crossing_exactly_once(Mt, Mx, W, H):
    L = slm.Level(Mt, Mx, True)
    nE, ht, hx = L.n // 2, Mt // 2, Mx // 2
    interior, crossing = slsw.tile_links(L, W, H)
    count = np.zeros((nE, 4), dtype=int)
    for e, d in crossing:
        assert 0 <= e < nE and 0 <= d < 4
        count[e, d] += 1
    assert np.all(count <= 1), "a link is crossed twice (the d = 3 link of a corner cell?)"
    assert np.all((interior >= 0) ^ (count == 1)), "a link is both interior and crossing, or neither"
    assert int((interior >= 0).sum()) + len(crossing) == 2 * L.n
    # interior: the O end is a cell of the same tile, reached without a wrap; crossing: it is not
    ntx = -(-ht // W)
    for e in range(nE):
        a, b = e % ht, e // ht
        for d in range(4):
            o = L.nbr[e, d] - nE
            oa, ob = o % ht, o // ht
            same = (oa // W, ob // H) == (a // W, b // H) and oa == a - (d >> 1) and ob == b - (d & 1)
            assert same == (interior[e, d] >= 0), (e, d)
            if same:
                assert interior[e, d] == (b // H) * ntx + a // W
    corner = [(e, d) for e, d in crossing if d == 3 and (e % ht) % W == 0 and (e // ht) % H == 0]
    assert len(corner) == len(set(corner)) == ntx * -(-hx // H)            # one d = 3 link per tile corner, once


# ---- 2. labels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", LEVELS[:4] + [(32, 32)])
def test_labels_are_those_of_a_sequential_union_find_and_roots_are_smallest_indices(Mt, Mx):
    seen_lone_O = False
    for k, beta in enumerate((0.5, 1.0, 1.5, 3.0)):
        L = slm.Level(Mt, Mx, True, beta)
        seed = 300 + 7 * k + Mt
        phi = slm.sweep_draw(L, slm.initialise(L, 1, seed), 0, 12, seed=seed)[0]
        for step in range(10):
            new, info = slsw.dev_update(L, phi, seed, 2, step)
            lab = info["labels"]
            assert np.array_equal(lab, slsw.sequential_labels(L, info["bonded"])), (Mt, Mx, beta, step)
            assert np.all(lab <= np.arange(L.n)) and np.all(lab[lab] == lab)
            assert info["clusters"] == len(np.unique(lab))
            seen_lone_O |= bool(np.any(lab[L.n // 2:] == np.arange(L.n // 2, L.n)))     # an O vertex that is its own root
            untouched = np.setdiff1d(np.arange(L.n), info["flipped"])
            assert np.array_equal(new.reshape(L.n, 2)[untouched], phi.reshape(L.n, 2)[untouched])
            mask = np.zeros(L.n, dtype=bool)
            mask[info["flipped"]] = True
            assert np.array_equal(mask, mask[lab]), "a cluster is reflected whole or not at all, as its root's coin says"
            phi = new
    assert seen_lone_O


def test_batched_model_equals_the_single_chain_model_on_a_rotated_level():
    L = slm.Level(4, 6, True, 1.5)
    B = 5
    phi = slm.initialise(L, B, 9)
    for step in range(8):
        new, binfo = slsw.dev_update_batch(L, phi, 21, 3, step)
        for b in range(B):
            one, info = slsw.dev_update(L, phi[b], 21, 3 + b, step)
            assert np.array_equal(one, new[b])
            assert binfo["flipped"][b] == len(info["flipped"]) and binfo["clusters"][b] == info["clusters"]
            assert abs(binfo["improved"][b] - info["improved"]) <= 1e-13 * info["improved"]
        phi = new
    out, flipped, clusters, improved, _ = slsw.dev_draw(L, slm.initialise(L, B, 9), 21, 3, 0, 8)
    assert np.array_equal(out, phi) and np.all(clusters >= 8) and np.all(improved > 0) and flipped.sum() > 0


# ---- 3. an unrotated Level is the unrotated model -----------------------------------------------------------------------------
def test_unrotated_level_reproduces_the_unrotated_model():
    Mt, Mx, beta = 6, 4, 1.5
    L = slm.Level(Mt, Mx, False, beta)
    phi = sm.sweep_draw(sm.initialise(3, Mt, Mx, 2), Mt, Mx, beta, 0, 6, seed=2)
    for step in range(6):
        new, info = slsw.dev_update(L, phi[0], 17, 4, step)
        want, winfo = swm.dev_update(phi[0], Mt, Mx, beta, 17, 4, step)
        assert np.array_equal(new, want) and np.array_equal(info["labels"], winfo["labels"])
        assert info["improved"] == winfo["improved"] and info["margin"] == winfo["margin"]
        nb, binfo = slsw.dev_update_batch(L, phi, 17, 4, step)
        wb, wbinfo = swm.dev_update_batch(phi, Mt, Mx, beta, 17, 4, step)
        assert np.array_equal(nb, wb) and all(np.array_equal(binfo[k], wbinfo[k]) for k in wbinfo)
        phi = nb
    a, b = slsw.dev_draw(L, phi, 17, 4, 9, 3), swm.dev_draw(phi, Mt, Mx, beta, 17, 4, 9, 3)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


# ---- 4. the law ---------------------------------------------------------------------------------------------------------------
def _sw_chain(L, seed, B, burn, meas):
    phi = slm.initialise(L, B, seed)
    chi, imp = [], []
    for step in range(burn + meas):
        phi, info = slsw.dev_update_batch(L, phi, seed + 1, 0, step)
        if step >= burn:
            chi.append(slm.magnetic_susceptibility(L, phi))
            imp.append(info["improved"])
    c, i = np.mean(chi, axis=0), np.mean(imp, axis=0)
    se = lambda x: float(x.std(ddof=1) / math.sqrt(B))  # noqa: E731
    return float(c.mean()), se(c), float(i.mean()), se(i)


def test_swendsen_wang_samples_the_law_of_the_rotated_heat_bath_and_the_improved_estimator_is_unbiased():
    """rotated (4, 4), n = 8, beta = 1, 64 chains x 3000 updates after 500: chi_m under the model's SW updates agrees with
    sigma_level_model's heat-bath sweeps; the improved value agrees with the plain chi_m of the same chain (the issue's
    comparison; the two are correlated, which makes the test stricter than its gate) and with that of other chains"""
    L = slm.Level(4, 4, True, 1.0)
    B = 64
    chi, chi_err, imp, imp_err = _sw_chain(L, 5, B, 500, 3000)
    chi2, chi2_err, _, _ = _sw_chain(L, 15, B, 500, 3000)
    phi = slm.initialise(L, B, 7)
    h = []
    for s in range(3500):
        phi = slm.sweep_draw(L, phi, 0, 1, seed=8, sweep0=s)
        if s >= 500:
            h.append(slm.magnetic_susceptibility(L, phi))
    h = np.mean(h, axis=0)
    heat, heat_err = float(h.mean()), float(h.std(ddof=1) / math.sqrt(B))
    zcheck("sigma level SW model vs rotated heat-bath model chi_m 4x4 beta=1", chi, chi_err, heat, heat_err)
    zcheck("sigma level SW model improved chi_m vs plain chi_m of the same chain, rotated 4x4 beta=1", imp, imp_err, chi, chi_err)
    zcheck("sigma level SW model improved chi_m vs plain chi_m of other SW chains, rotated 4x4 beta=1", imp, imp_err, chi2, chi2_err)
    zcheck("sigma level SW model improved chi_m vs rotated heat-bath model chi_m 4x4 beta=1", imp, imp_err, heat, heat_err)


# ---- 5. surface ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in abi.SIGNATURES
    assert lib.mlmcpi_abi_version() == 1
    assert callable(ops.sigma_level_sw_workspace) and callable(ops.sigma_level_sw_draw)


def test_invalid_levels_counters_and_no_device():
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    size = C.c_size_t(0)
    ws, draw = lib.mlmcpi_sigma_level_sw_workspace_bytes, lib.mlmcpi_sigma_level_sw_draw
    assert ws(None, 1, C.byref(size)) == -1
    assert draw(None, None, 1, 1, 1, 0, 0, None, None, None, None, None) == -1
    for rot in (0, 1):
        for Mt, Mx, beta in ((3, 8, 1.0), (8, 5, 1.0), (0, 8, 1.0), (8, 0, 1.0), (1 << 16, 1 << 15, 1.0), (8, 8, 0.0), (8, 8, -1.0)):
            bad = abi.sigma_level(Mt, Mx, rot, beta)
            assert ws(C.byref(bad), 1, C.byref(size)) == -1, (rot, Mt, Mx, beta)
            assert draw(C.byref(bad), None, 1, 1, 1, 0, 0, None, None, None, None, None) == -1, (rot, Mt, Mx, beta)
        lv = abi.sigma_level(6, 10, rot, 1.0)
        n = 30 if rot else 60
        assert ws(C.byref(lv), 0, C.byref(size)) == -1                                    # B = 0
        assert ws(C.byref(lv), 3, C.byref(size)) == 0
        if rot:     # the status word, then label 4 B, q(a) 8 B, root slot 8 B per vertex and a byte per E vertex, four sections
            assert 256 + 3 * n * 20 + 3 * (n // 2) <= size.value < 256 + 3 * n * 20 + 3 * (n // 2) + 4 * 256
        else:       # the workspace of mlmcpi_sigma_sw_draw
            act = abi.lattice_action(abi.NONLINEAR_SIGMA, 6, 10, beta=1.0)
            want = C.c_size_t(0)
            assert lib.mlmcpi_sigma_sw_workspace_bytes(C.byref(act), 3, C.byref(want)) == 0 and want.value == size.value
        buf = (C.c_double * (2 * n))()
        work = (C.c_char * size.value)()
        # update0 + n_updates beyond 32 bits: MLMCPI_ERR_INVALID, before anything is launched
        assert draw(C.byref(lv), buf, 1, 2, 1, 0, 0xFFFFFFFF, None, None, None, work, None) == -1
        assert b"overflow" in lib.mlmcpi_last_error()
        assert draw(C.byref(lv), buf, 1, 1, 1, 0, 0, None, None, None, None, None) == -1   # no workspace
        assert draw(C.byref(lv), buf, 0, 1, 1, 0, 0, None, None, None, work, None) == -1   # B = 0
        if not torch.cuda.is_available():
            # no silent CPU path: with valid arguments and no device the call fails with the runtime's no-device error
            rc = draw(C.byref(lv), buf, 1, 1, 1, 0, 0, None, None, None, work, None)
            assert rc in (-2, -4), rc
            assert all(v == 0.0 for v in buf) and not any(work.raw)


def test_chain_plan_forced_beyond_its_bound_is_unsupported_before_any_launch():
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    lv = abi.sigma_level(512, 300, 1, 1.5)                 # n = 76 800 > 7552
    buf = (C.c_double * 4)()                               # never touched: the plan is refused before anything is launched
    abi.set_option("MLMCPI_SIGMA_SW_PLAN", "chain")
    try:
        assert lib.mlmcpi_sigma_level_sw_draw(C.byref(lv), buf, 1, 1, 1, 0, 0, None, None, None, buf, None) == -3
        assert b"7552" in lib.mlmcpi_last_error()
    finally:
        abi.set_option("MLMCPI_SIGMA_SW_PLAN", "")


def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,why", [
    (["--action", "gff", "--coarsening", "rotate", "--sampler", "hierarchical", "--coarsesampler", "levelsw"], "nonlinearsigma only"),
    (["--action", "schwinger", "--method", "twolevel", "--coarsesampler", "levelsw"], "nonlinearsigma only"),
    (["--action", "rotor", "--method", "twolevel", "--coarsesampler", "levelsw"], "nonlinearsigma only"),
    (["--action", "nonlinearsigma", "--method", "singlelevel", "--sampler", "heatbath", "--coarsesampler", "levelsw"],
     "--method twolevel or --sampler hierarchical"),
    (["--action", "nonlinearsigma", "--method", "throughput", "--sampler", "heatbath", "--coarsesampler", "levelsw"],
     "--method twolevel or --sampler hierarchical"),
    (["--action", "nonlinearsigma", "--sampler", "levelsw"], "--sampler swendsenwang"),
    (["--action", "nonlinearsigma", "--coarsening", "both", "--sampler", "hierarchical", "--coarsesampler", "levelsw"],
     "--coarsening rotate"),
    (["--action", "nonlinearsigma", "--coarsening", "temporal", "--method", "twolevel", "--sampler", "heatbath", "--coarsesampler",
      "levelsw"], "--coarsening rotate")])
def test_driver_refuses_levelsw_by_name_where_it_does_not_apply_and_says_why(args, why):
    r = _driver(*args)
    assert r.returncode != 0
    out = r.stderr + r.stdout
    assert "levelsw" in out and why in out, out


def test_driver_accepts_levelsw_as_a_coarse_sampler_up_to_the_first_device_call():
    """with --coarsening rotate and a hierarchical or two-level run the option passes every check of the command line: the run
    gets as far as the action (it prints it) and, on a machine without a device, ends in the runtime's error, not in a refusal"""
    import torch
    for extra in (["--sampler", "hierarchical", "--n_level", "2"], ["--sampler", "heatbath", "--method", "twolevel"]):
        r = _driver("--action", "nonlinearsigma", "--Mt_lat", "8", "--coarsening", "rotate", "--coarsesampler", "levelsw", "--n_updates", "2",
                    "--n_samples", "20", "--n_burnin", "2", "--n_meas", "2", *extra)
        out = r.stderr + r.stdout
        assert "Action:" in r.stdout, out
        assert "not supported" not in out and "heatbath only" not in out and "unknown sampler" not in out, out
        if torch.cuda.is_available():
            assert r.returncode == 0, out


def test_driver_still_refuses_the_coarse_samplers_it_refused_and_names_levelsw_as_allowed():
    r = _driver("--action", "nonlinearsigma", "--sampler", "heatbath", "--coarsesampler", "swendsenwang")
    assert r.returncode != 0 and "--coarsesampler swendsenwang is not supported" in r.stderr + r.stdout
    r = _driver("--action", "nonlinearsigma", "--sampler", "heatbath", "--coarsesampler", "wolff")
    assert r.returncode != 0 and "--coarsesampler wolff is not supported" in r.stderr + r.stdout
    r = _driver("--action", "nonlinearsigma", "--coarsening", "rotate", "--sampler", "hierarchical", "--coarsesampler", "hmc")
    out = r.stderr + r.stdout
    assert r.returncode != 0 and "--coarsesampler heatbath only" in out and "levelsw" in out
