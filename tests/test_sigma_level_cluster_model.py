"""CPU: the Wolff single-cluster update of the O(3) sigma model on a rotated level restated
(tests/sigma_level_cluster_model.py) -- the link naming covers every (vertex, direction) pair once from each end, the
component statement equals the reference's walk over the four rotated neighbours, it samples the law of the rotated heat
bath, an unrotated Level is the unrotated model -- and the surface the feature adds to the C ABI and to host/driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sigma_cluster_model as scm
import sigma_level_cluster_model as slcm
import sigma_level_model as slm
import sigma_model as sm
from conftest import zcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mlmcpi_sigma_level_cluster_workspace_bytes", "mlmcpi_sigma_level_cluster_draw"]


# ---- 1. link ownership ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 6), (16, 16), (66, 34)])
def test_every_link_is_named_once_from_each_end(Mt, Mx):
    """the kernel's plane arithmetic (plane_task) gives the neighbours of Level.nbr, and over all (x, d) every link (e, d) is
    hit exactly twice: once from its E end as (x, d), once from its O end as (neighbour, 3 - d'); the model's tables agree"""
    L = slm.Level(Mt, Mx, True)
    nE = L.n // 2
    site, which = slcm.link_tables(L)
    from_E = np.zeros((nE, 4), dtype=int)
    from_O = np.zeros((nE, 4), dtype=int)
    ends = {}
    for x in range(L.n):
        for d in range(4):
            y, e, de = slcm.plane_task(L, x, d)
            assert y == L.nbr[x, d], (x, d, y, L.nbr[x, d])
            assert (e, de) == (site[x, d], which[x, d])
            assert 0 <= e < nE and 0 <= de < 4
            if x < nE:
                assert (e, de) == (x, d)
                from_E[e, de] += 1
                ends[(e, de)] = ends.get((e, de), ()) + (y,)
            else:
                assert (e, de) == (y, 3 - d)
                from_O[e, de] += 1
                ends[(e, de)] = ends.get((e, de), ()) + (x,)
    assert np.all(from_E == 1) and np.all(from_O == 1)
    assert len(ends) == 2 * L.n and all(len(v) == 2 and v[0] == v[1] for v in ends.values())   # both ends name one O vertex


# ---- 2. the identity: the component of the seed in the graph of bonds == the walk over the four rotated neighbours -----------
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 6), (16, 16), (32, 32)])
def test_component_equals_the_four_neighbour_walk_on_rotated_levels(Mt, Mx):
    total = largest = 0
    for n, beta in enumerate((0.5, 1.0, 1.5, 3.0)):
        L = slm.Level(Mt, Mx, True, beta)
        seed, chain = 400 + 7 * n + Mt, 2
        phi = slm.sweep_draw(L, slm.initialise(L, 1, seed), 0, 12, seed=seed)[0]   # some order to grow clusters in
        for step in range(60 if L.n <= 128 else 40):
            new, info = slcm.dev_update(L, phi, seed, chain, step)
            ref, flipped = slcm.walk_with_device_uniforms(L, phi, seed, chain, step)
            assert info["margin"] > 1e-12, "a bond decision within rounding of its uniform: change the seed"
            assert len(flipped) == len(set(flipped)), "a vertex was flipped twice"
            assert sorted(flipped) == info["sites"].tolist(), (Mt, Mx, beta, step)
            assert flipped[0] == info["seed"]
            d = np.abs(slm.unit_vectors(L, ref[None]) - slm.unit_vectors(L, new[None])).max()
            assert d < 1e-13, (Mt, Mx, beta, step, d)
            untouched = np.setdiff1d(np.arange(L.n), info["sites"])
            assert np.array_equal(new.reshape(L.n, 2)[untouched], phi.reshape(L.n, 2)[untouched])
            total += 1
            largest = max(largest, len(flipped))
            phi = new
    print(f"rotated {Mt} x {Mx}: {total} updates, largest cluster {largest} of {Mt * Mx // 2} vertices")
    assert total >= 160 and largest > 1


def test_batched_model_equals_the_single_chain_model_on_a_rotated_level():
    L = slm.Level(4, 6, True, 1.5)
    B = 5
    phi = slm.initialise(L, B, 9)
    for step in range(8):
        new, sizes = slcm.dev_update_batch(L, phi, 21, 3, step)
        for b in range(B):
            one, info = slcm.dev_update(L, phi[b], 21, 3 + b, step)
            assert np.array_equal(one, new[b]) and sizes[b] == len(info["sites"])
        phi = new
    out, count, _ = slcm.dev_draw(L, slm.initialise(L, B, 9), 21, 3, 0, 8)
    assert np.array_equal(out, phi) and count.sum() > 8 * B


# ---- 3. the law -------------------------------------------------------------------------------------------------------------
def test_wolff_updates_sample_the_law_of_the_rotated_heat_bath():
    """rotated (4, 4), n = 8, beta = 1: chi_m under the model's Wolff updates agrees with sigma_level_model's heat-bath sweeps at
    3 sigma of the two errors, each at or below 1 % of chi_m (lengths and seeds after tests/test_sigma_cluster_model.py)"""
    L = slm.Level(4, 4, True, 1.0)
    B = 128
    phi = slm.initialise(L, B, 5)
    chi = []
    for step in range(1500):
        phi, _ = slcm.dev_update_batch(L, phi, 6, 0, step)
        if step >= 100:
            chi.append(slm.magnetic_susceptibility(L, phi))
    w = np.mean(chi, axis=0)
    wolff, wolff_err = float(w.mean()), float(w.std(ddof=1) / np.sqrt(B))

    phi = slm.initialise(L, B, 7)
    chi = []
    for s in range(630):
        phi = slm.sweep_draw(L, phi, 0, 1, seed=8, sweep0=s)
        if s >= 30:
            chi.append(slm.magnetic_susceptibility(L, phi))
    h = np.mean(chi, axis=0)
    heat, heat_err = float(h.mean()), float(h.std(ddof=1) / np.sqrt(B))
    print(f"chi_m rotated 4x4 beta=1: Wolff {wolff:.4f} +- {wolff_err:.4f}, heat bath {heat:.4f} +- {heat_err:.4f}")
    assert wolff_err <= 0.01 * wolff and heat_err <= 0.01 * heat
    zcheck("sigma level Wolff model vs rotated heat-bath model chi_m 4x4 beta=1", wolff, wolff_err, heat, heat_err, gate=3.0)


# ---- 4. an unrotated Level is the unrotated model ---------------------------------------------------------------------------
def test_unrotated_level_calls_through_to_the_unrotated_model():
    Mt, Mx, beta = 6, 4, 1.5
    L = slm.Level(Mt, Mx, False, beta)
    phi = sm.sweep_draw(sm.initialise(3, Mt, Mx, 2), Mt, Mx, beta, 0, 6, seed=2)
    for step in range(6):
        new, info = slcm.dev_update(L, phi[0], 17, 4, step)
        want, winfo = scm.dev_update(phi[0], Mt, Mx, beta, 17, 4, step)
        assert np.array_equal(new, want) and np.array_equal(info["sites"], winfo["sites"])
        assert info["seed"] == winfo["seed"] and info["margin"] == winfo["margin"] and np.array_equal(info["r"], winfo["r"])
        nb, sizes = slcm.dev_update_batch(L, phi, 17, 4, step)
        wb, wsizes = scm.dev_update_batch(phi, Mt, Mx, beta, 17, 4, step)
        assert np.array_equal(nb, wb) and np.array_equal(sizes, wsizes)
        phi = nb
    a, b = slcm.dev_draw(L, phi, 17, 4, 9, 3), scm.dev_draw(phi, Mt, Mx, beta, 17, 4, 9, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    r, s0 = scm.reflection(17, 4, 0, Mt * Mx)
    rng_a, rng_b = np.random.default_rng(1), np.random.default_rng(1)
    xa, fa = slcm.walk_update(L, phi[0], r, s0, lambda ell, k, y: rng_a.random())
    xb, fb = scm.walk_update(phi[0], Mt, Mx, beta, r, s0, lambda ell, k, y: rng_b.random())
    assert np.array_equal(xa, xb) and fa == fb


# ---- 5. surface -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in abi.SIGNATURES
    assert lib.mlmcpi_abi_version() == 1
    assert callable(ops.sigma_level_cluster_workspace) and callable(ops.sigma_level_cluster_draw)


def test_invalid_levels_counters_and_no_device():
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    size = C.c_size_t(0)
    ws, draw = lib.mlmcpi_sigma_level_cluster_workspace_bytes, lib.mlmcpi_sigma_level_cluster_draw
    assert ws(None, 1, C.byref(size)) == -1
    assert draw(None, None, 1, 1, 1, 0, 0, None, None, None) == -1
    for rot in (0, 1):
        for Mt, Mx, beta in ((3, 8, 1.0), (8, 5, 1.0), (0, 8, 1.0), (8, 0, 1.0), (1 << 16, 1 << 15, 1.0), (8, 8, 0.0), (8, 8, -1.0)):
            bad = abi.sigma_level(Mt, Mx, rot, beta)
            assert ws(C.byref(bad), 1, C.byref(size)) == -1, (rot, Mt, Mx, beta)
            assert draw(C.byref(bad), None, 1, 1, 1, 0, 0, None, None, None) == -1, (rot, Mt, Mx, beta)
        lv = abi.sigma_level(6, 10, rot, 1.0)
        n = 30 if rot else 60
        assert ws(C.byref(lv), 0, C.byref(size)) == -1                                    # B = 0
        assert ws(C.byref(lv), 3, C.byref(size)) == 0
        assert size.value >= 3 * n * 12 + 3 * ((n + 31) // 32) * 4      # the queue's (vertex, a) pairs and the membership bits
        assert size.value < 3 * n * 12 + 3 * ((n + 31) // 32) * 4 + 3 * 256              # and the alignment of three sections
        buf = (C.c_double * (2 * n))()
        work = (C.c_char * size.value)()
        # update0 + n_updates beyond 32 bits: MLMCPI_ERR_INVALID, before anything is launched
        assert draw(C.byref(lv), buf, 1, 2, 1, 0, 0xFFFFFFFF, None, work, None) == -1
        assert b"overflow" in lib.mlmcpi_last_error()
        assert draw(C.byref(lv), buf, 1, 1, 1, 0, 0, None, None, None) == -1            # no workspace
        assert draw(C.byref(lv), buf, 0, 1, 1, 0, 0, None, work, None) == -1            # B = 0
        if not torch.cuda.is_available():
            # no silent CPU path: with valid arguments and no device the launch fails with the runtime's no-device error
            rc = draw(C.byref(lv), buf, 1, 1, 1, 0, 0, None, work, None)
            assert rc in (-2, -4), rc
            assert all(v == 0.0 for v in buf) and not any(work.raw)


def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,why", [
    (["--action", "gff", "--coarsening", "rotate", "--sampler", "hierarchical", "--coarsesampler", "levelwolff"], "nonlinearsigma only"),
    (["--action", "schwinger", "--method", "twolevel", "--coarsesampler", "levelwolff"], "nonlinearsigma only"),
    (["--action", "rotor", "--method", "twolevel", "--coarsesampler", "levelwolff"], "nonlinearsigma only"),
    (["--action", "nonlinearsigma", "--method", "singlelevel", "--sampler", "heatbath", "--coarsesampler", "levelwolff"],
     "--method twolevel or --sampler hierarchical"),
    (["--action", "nonlinearsigma", "--method", "throughput", "--sampler", "heatbath", "--coarsesampler", "levelwolff"],
     "--method twolevel or --sampler hierarchical"),
    (["--action", "nonlinearsigma", "--sampler", "levelwolff"], "--sampler wolff"),
    (["--action", "nonlinearsigma", "--coarsening", "both", "--sampler", "hierarchical", "--coarsesampler", "levelwolff"],
     "--coarsening rotate"),
    (["--action", "nonlinearsigma", "--coarsening", "temporal", "--method", "twolevel", "--sampler", "heatbath", "--coarsesampler",
      "levelwolff"], "--coarsening rotate")])
def test_driver_refuses_levelwolff_by_name_where_it_does_not_apply_and_says_why(args, why):
    r = _driver(*args)
    assert r.returncode != 0
    out = r.stderr + r.stdout
    assert "levelwolff" in out and why in out, out


def test_driver_still_refuses_the_coarse_samplers_it_refused():
    r = _driver("--action", "nonlinearsigma", "--sampler", "heatbath", "--coarsesampler", "wolff")
    assert r.returncode != 0 and "--coarsesampler wolff is not supported" in r.stderr + r.stdout
    r = _driver("--action", "nonlinearsigma", "--coarsening", "rotate", "--sampler", "hierarchical", "--coarsesampler", "hmc")
    assert r.returncode != 0 and "--coarsesampler heatbath only" in r.stderr + r.stdout
