"""CPU: the Wolff single-cluster update of the O(3) sigma model restated (tests/sigma_cluster_model.py) -- the component
statement equals the reference's walk restricted to the four links per vertex, it samples the law of the heat bath while
the reference's eight-neighbour walk does not -- and the surface the feature adds to the C ABI and to host/driver."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sigma_cluster_model as scm
import sigma_model as sm
from conftest import zcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mlmcpi_sigma_cluster_workspace_bytes", "mlmcpi_sigma_cluster_draw"]


# ---- 1. the identity: the component of the seed in the graph of bonds == the reference's walk over four neighbours ---------
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 6), (16, 16), (64, 64)])
def test_component_equals_the_four_neighbour_walk(Mt, Mx):
    """the walk (flip on joining, S_ell on the current state, a queue, each link tested once) fed with the link-keyed
    uniforms of the device rule flips exactly the component computed from the field before the update"""
    N = Mt * Mx
    total = largest = 0
    for n, beta in enumerate((0.5, 1.0, 1.5, 3.0)):
        seed, chain = 300 + 7 * n + Mt, 2
        phi = sm.sweep_draw(sm.initialise(1, Mt, Mx, seed), Mt, Mx, beta, 0, 12, seed=seed)[0]   # some order to grow clusters in
        for step in range(20 if N <= 256 else 12):
            new, info = scm.dev_update(phi, Mt, Mx, beta, seed, chain, step)
            ref, flipped = scm.walk_with_device_uniforms(phi, Mt, Mx, beta, seed, chain, step)
            assert info["margin"] > 1e-12, "a bond decision within rounding of its uniform: change the seed"
            assert len(flipped) == len(set(flipped)), "a vertex was flipped twice"
            assert sorted(flipped) == info["sites"].tolist(), (Mt, Mx, beta, step)
            assert flipped[0] == info["seed"]
            d = np.abs(sm.unit_vectors(ref[None], Mt, Mx) - sm.unit_vectors(new[None], Mt, Mx)).max()
            assert d < 1e-13, (Mt, Mx, beta, step, d)
            untouched = np.setdiff1d(np.arange(N), info["sites"])
            assert np.array_equal(new.reshape(N, 2)[untouched], phi.reshape(N, 2)[untouched])
            total += 1
            largest = max(largest, len(flipped))
            phi = new
    print(f"{Mt} x {Mx}: {total} updates, largest cluster {largest} of {N} vertices")
    assert largest > 1


def test_batched_model_equals_the_single_chain_model():
    Mt, Mx, beta, B = 4, 6, 1.5, 5
    phi = sm.initialise(B, Mt, Mx, 9)
    for step in range(8):
        new, sizes = scm.dev_update_batch(phi, Mt, Mx, beta, 21, 3, step)
        for b in range(B):
            one, info = scm.dev_update(phi[b], Mt, Mx, beta, 21, 3 + b, step)
            assert np.array_equal(one, new[b]) and sizes[b] == len(info["sites"])
        phi = new


# ---- 2. the law, and the reason for the sampler's own name ---------------------------------------------------------------
def _batch_means(x, n=50):
    m = np.asarray(x)[: len(x) // n * n].reshape(n, -1).mean(axis=1)
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(n))


def test_four_links_sample_the_heat_bath_law_and_eight_neighbours_do_not():
    """4 x 4, beta = 1: chi_m under the model's updates agrees with sigma_model's heat-bath sweeps; the same walk over the
    eight entries of Lattice2D::neighbour_vertices (diagonals carry no energy) lies more than 20 sigma away"""
    Mt = Mx = 4
    beta, B = 1.0, 128
    phi = sm.initialise(B, Mt, Mx, 5)
    chi = []
    for step in range(700):
        phi, _ = scm.dev_update_batch(phi, Mt, Mx, beta, 6, 0, step)
        if step >= 100:
            chi.append(sm.magnetic_susceptibility(phi, Mt, Mx))
    w = np.mean(chi, axis=0)
    wolff, wolff_err = float(w.mean()), float(w.std(ddof=1) / math.sqrt(B))

    phi = sm.initialise(B, Mt, Mx, 7)
    chi = []
    for s in range(330):
        phi = sm.sweep_draw(phi, Mt, Mx, beta, 0, 1, seed=8, sweep0=s)
        if s >= 30:
            chi.append(sm.magnetic_susceptibility(phi, Mt, Mx))
    h = np.mean(chi, axis=0)
    heat, heat_err = float(h.mean()), float(h.std(ddof=1) / math.sqrt(B))
    zcheck("sigma Wolff model vs heat-bath model chi_m 4x4 beta=1", wolff, wolff_err, heat, heat_err)

    rng = np.random.default_rng(11)
    x = sm.initialise(1, Mt, Mx, 12)[0]
    chi8 = []
    for step in range(12500):
        r = rng.normal(size=3)
        r /= np.linalg.norm(r)
        x, _ = scm.walk_update(x, Mt, Mx, beta, r, int(rng.integers(Mt * Mx)), lambda ell, k, y: rng.random(), n_neighbours=8)
        if step >= 500:
            chi8.append(sm.magnetic_susceptibility(x[None], Mt, Mx)[0])
    eight, eight_err = _batch_means(chi8)
    z = (eight - wolff) / math.hypot(eight_err, wolff_err)
    print(f"chi_m: four links {wolff:.4f} +- {wolff_err:.4f}, heat bath {heat:.4f} +- {heat_err:.4f}, "
          f"eight neighbours {eight:.4f} +- {eight_err:.4f}: {z:.1f} sigma from the four-link chain")
    assert abs(z) > 20.0, z


# ---- 3. surface ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in abi.SIGNATURES
    assert lib.mlmcpi_abi_version() == 1


def test_unsupported_kinds_invalid_counters_and_no_device():
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    size = C.c_size_t(0)
    for kind in (abi.GFF, abi.SCHWINGER):
        act = abi.lattice_action(kind, 8, 8, beta=1.0, mass=1.0)
        assert lib.mlmcpi_sigma_cluster_workspace_bytes(C.byref(act), 1, C.byref(size)) == -3
        assert lib.mlmcpi_sigma_cluster_draw(C.byref(act), None, 1, 1, 1, 0, 0, None, None, None) == -3
        assert b"sigma" in lib.mlmcpi_last_error()
    act = abi.lattice_action(abi.NONLINEAR_SIGMA, 6, 10, beta=1.0)
    assert lib.mlmcpi_sigma_cluster_workspace_bytes(C.byref(act), 3, C.byref(size)) == 0
    assert size.value >= 3 * 60 * 12 + 3 * 2 * 4      # the queue's (vertex, a) pairs and the membership bits
    buf = (C.c_double * 120)()
    work = (C.c_char * size.value)()
    # update0 + n_updates beyond 32 bits: MLMCPI_ERR_INVALID, before anything is launched
    assert lib.mlmcpi_sigma_cluster_draw(C.byref(act), buf, 1, 2, 1, 0, 0xFFFFFFFF, None, work, None) == -1
    assert b"overflow" in lib.mlmcpi_last_error()
    assert lib.mlmcpi_sigma_cluster_draw(C.byref(act), buf, 1, 1, 1, 0, 0, None, None, None) == -1   # no workspace
    small = abi.lattice_action(abi.NONLINEAR_SIGMA, 1, 8, beta=1.0)
    assert lib.mlmcpi_sigma_cluster_workspace_bytes(C.byref(small), 1, C.byref(size)) == -1
    if not torch.cuda.is_available():
        # no silent CPU path: with valid arguments and no device the launch fails with the runtime's no-device error
        rc = lib.mlmcpi_sigma_cluster_draw(C.byref(act), buf, 1, 1, 1, 0, 0, None, work, None)
        assert rc in (-2, -4), rc
        assert all(v == 0.0 for v in buf) and not any(work.raw)


def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,why", [
    (["--action", "gff"], "built for nonlinearsigma only"),
    (["--action", "schwinger"], "built for nonlinearsigma only"),
    (["--action", "rotor"], "built for nonlinearsigma only"),
    (["--action", "nonlinearsigma", "--method", "twolevel"], "singlelevel only"),
    (["--action", "nonlinearsigma", "--method", "multilevel"], "singlelevel only")])
def test_driver_refuses_wolff_where_it_does_not_apply_and_says_why(args, why):
    r = _driver(*args, "--sampler", "wolff")
    assert r.returncode != 0
    out = r.stderr + r.stdout
    assert "wolff" in out and why in out, out


def test_driver_refuses_wolff_as_a_coarse_sampler():
    r = _driver("--action", "nonlinearsigma", "--sampler", "heatbath", "--coarsesampler", "wolff")
    assert r.returncode != 0
    assert "--coarsesampler wolff is not supported" in r.stderr + r.stdout
