"""CPU: the order contract and the round schedule of the parallel random-order sweep (tests/random_sweep_model.py), and the
C surface of its three entry points (which is what fails without the feature)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import random_sweep_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567812345678
CHI2_15_Q999 = 37.697  # 0.999 quantile of chi^2 with 15 degrees of freedom


def test_keys_follow_the_contract_and_orders_are_permutations():
    import sigma_model as sm
    n = 50
    seen = []
    for seed, chain, step in [(SEED, 0, 0), (SEED, 1, 0), (SEED, 0, 1), (7, 3000000000, 4000000000), (SEED, 17, 5)]:
        key = rm.keys(seed, chain, step, n)
        for l in (0, 1, 6, 49):
            r = sm.philox(l >> 2, chain, step, 18 << 24, seed & 0xFFFFFFFF, seed >> 32)
            assert int(key[l]) == int(r[l & 3])
        order = rm.order_of(key)
        assert sorted(order.tolist()) == list(range(n))
        k = key[order].astype(np.int64)
        assert ((np.diff(k) > 0) | ((np.diff(k) == 0) & (np.diff(order.astype(np.int64)) > 0))).all()
        seen.append(tuple(order.tolist()))
    assert len(set(seen)) == len(seen), "orders must differ between chains and between sweeps"
    # ties go to the smaller index
    assert rm.order_of(np.array([5, 3, 5, 3, 1], dtype=np.uint32)).tolist() == [4, 1, 3, 0, 2]


def test_order_is_uniform():
    n, sweeps, l0 = 64, 20000, 37
    ranks = np.empty(sweeps, dtype=np.int64)
    less = np.zeros(3)
    pairs = [(0, 1), (5, 4), (2, 63)]
    for s in range(sweeps):
        key = rm.keys(SEED, 11, s, n)
        ranks[s] = np.count_nonzero((key < key[l0]) | ((key == key[l0]) & (np.arange(n) < l0)))
        less += [key[a] < key[b] for a, b in pairs]
    cells = np.bincount(ranks // 4, minlength=16)
    chi2 = float(((cells - sweeps / 16.0) ** 2 / (sweeps / 16.0)).sum())
    print(f"rank of index {l0} over {sweeps} sweeps: chi^2(15) = {chi2:.2f}")
    assert chi2 < CHI2_15_Q999
    for (a, b), c in zip(pairs, less):
        z = (c / sweeps - 0.5) / (0.5 / np.sqrt(sweeps))
        print(f"P(key {a} < key {b}) = {c / sweeps:.4f}, z = {z:+.2f}")
        assert abs(z) < 3.29  # two-sided 0.999


@pytest.mark.parametrize("kind,Mt,Mx", [(rm.SCHWINGER, 2, 2), (rm.SCHWINGER, 5, 4), (rm.SCHWINGER, 16, 16),
                                        (rm.GFF, 2, 2), (rm.GFF, 3, 4), (rm.GFF, 16, 16)])
def test_the_schedule_is_the_sequential_walk(kind, Mt, Mx):
    n = rm.n_indices(kind, Mt, Mx)
    nb = rm.neighbours(kind, Mt, Mx)
    # the conflict relation is symmetric and has no self loops
    pairs = {(l, int(m)) for l in range(n) for m in nb[l]}
    assert all((m, l) in pairs for l, m in pairs) and all(l != m for l, m in pairs)
    rng = np.random.default_rng(n)
    mu2 = 0.3
    for chain, step in [(0, 0), (5, 3), (77, 1234)]:
        order, rnd = rm.schedule(kind, Mt, Mx, SEED, chain, step)
        assert rnd.min() >= 1 and rnd.size == n                      # every index is in exactly one round
        for l, m in pairs:
            assert rnd[l] != rnd[m], "a round holds a conflicting pair"
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        for l, m in pairs:
            assert (pos[l] < pos[m]) == (rnd[l] < rnd[m]), "a conflicting pair runs out of order"
        x0 = rng.uniform(-np.pi, np.pi, n) if kind == rm.SCHWINGER else rng.normal(size=n)
        for heat in ([False] if kind == rm.SCHWINGER else [False, True]):
            kw = {} if kind == rm.SCHWINGER else dict(normals=rm.gff_normals(SEED, chain, step, np.arange(n)), mu2=mu2)
            a, b = x0.copy(), x0.copy()
            rm.sweep_sequential(kind, a, order, nb, heat, **kw)
            rm.sweep_rounds(kind, b, rnd, nb, heat, **kw)
            d = a - b
            if kind == rm.SCHWINGER:
                d -= 2 * np.pi * np.round(d / (2 * np.pi))
            assert np.max(np.abs(d)) <= 1e-13, f"heat={heat}: rounds differ from the sequential walk by {np.max(np.abs(d)):.2e}"


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (3, 4), (16, 16)])
def test_the_schedule_is_the_sequential_walk_sigma_heat_bath(Mt, Mx):
    """the sigma model's heat bath on the vertex stencil, through sigma_model's own update, one vertex or one round at a time"""
    import sigma_model as sm
    n, beta = Mt * Mx, 1.3
    nb = rm.neighbours(rm.SIGMA, Mt, Mx)
    order, rnd = rm.schedule(rm.SIGMA, Mt, Mx, SEED, 2, 9)
    rng = np.random.default_rng(n)
    a0 = np.stack([np.arccos(rng.uniform(-1, 1, n)), rng.uniform(-np.pi, np.pi, n)], axis=1)
    u, v = sm.uniforms(SEED, 2, 9, np.arange(n, dtype=np.uint64), sm.P_SIGMA_HB)

    def upd(a, idx, heat):
        idx = np.atleast_1d(idx)
        sig = sm.sigma_of(a)
        m = nb[idx]
        D = ((sig[m[:, 0]] + sig[m[:, 1]]) + sig[m[:, 2]]) + sig[m[:, 3]]
        new = sm.heatbath(sig[idx], D, beta, u[idx], v[idx]) if heat else sm.overrelax(sig[idx], D)
        a[idx] = sm.angles_of(new)

    for heat in (False, True):
        a, b = a0.copy(), a0.copy()
        for l in order:
            upd(a, int(l), heat)
        for k in range(1, int(rnd.max()) + 1):
            upd(b, np.nonzero(rnd == k)[0], heat)
        assert np.max(np.abs(sm.sigma_of(a) - sm.sigma_of(b))) <= 1e-13


def test_round_counts_are_a_dozen_odd():
    for kind, M, lo, hi in [(rm.SCHWINGER, 64, 10, 26), (rm.GFF, 64, 7, 20)]:
        r = [int(rm.schedule(kind, M, M, SEED, c, 0)[1].max()) for c in range(4)]
        print(kind, M, r)
        assert lo <= min(r) and max(r) <= hi


# ---- the C surface ----------------------------------------------------------------------------------------------------
NAMES = ["mlmcpi_lattice_random_sweep_workspace_bytes", "mlmcpi_lattice_random_sweep_draw", "mlmcpi_lattice_random_sweep_order"]


def test_entry_points_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi
    header = open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read()
    lib = abi.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert name in abi.SIGNATURES and hasattr(lib, name)
    assert header.count("overrelaxedheatbathsampler.cc:8-31") >= 4
    assert lib.mlmcpi_abi_version() == 1


def test_bad_arguments_return_status_codes_and_no_device_touches_nothing():
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    nbytes = C.c_size_t(0)
    good = abi.lattice_action(abi.SCHWINGER, 5, 4, beta=1.0)
    buf = np.full(40, 3.25)
    work = np.zeros(1024, dtype=np.uint8)
    order = np.full(40, 0xABCDEF01, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for kind in (abi.HARMONIC, abi.QUARTIC, abi.ROTOR, 17):
        act = abi.lattice_action(kind, 8, 8, beta=1.0)
        assert lib.mlmcpi_lattice_random_sweep_workspace_bytes(C.byref(act), 1, C.byref(nbytes)) == -3
        assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(act), vp(buf), 1, 1, 1, SEED, 0, 0, vp(work), None) == -3
        assert lib.mlmcpi_lattice_random_sweep_order(C.byref(act), 1, SEED, 0, 0, vp(order), None, None) == -3
    assert b"2-D actions" in lib.mlmcpi_last_error()
    assert lib.mlmcpi_lattice_random_sweep_workspace_bytes(None, 1, C.byref(nbytes)) == -1
    assert lib.mlmcpi_lattice_random_sweep_workspace_bytes(C.byref(good), 1, None) == -1
    assert lib.mlmcpi_lattice_random_sweep_workspace_bytes(C.byref(good), 0, C.byref(nbytes)) == -1
    assert lib.mlmcpi_lattice_random_sweep_draw(None, vp(buf), 1, 1, 1, SEED, 0, 0, vp(work), None) == -1
    assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(good), None, 1, 1, 1, SEED, 0, 0, vp(work), None) == -1
    assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(good), vp(buf), 1, 1, 1, SEED, 0, 0, None, None) == -1
    assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(good), vp(buf), 0, 1, 1, SEED, 0, 0, vp(work), None) == -1
    assert lib.mlmcpi_lattice_random_sweep_order(None, 1, SEED, 0, 0, vp(order), None, None) == -1
    assert lib.mlmcpi_lattice_random_sweep_order(C.byref(good), 1, SEED, 0, 0, None, None, None) == -1
    for Mt, Mx in ((1, 8), (8, 1), (0, 0)):
        small = abi.lattice_action(abi.GFF, Mt, Mx, mass=1.0)
        assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(small), vp(buf), 1, 1, 1, SEED, 0, 0, vp(work), None) == -1
    assert lib.mlmcpi_lattice_random_sweep_workspace_bytes(C.byref(good), 3, C.byref(nbytes)) == 0
    assert nbytes.value >= 3 * 6 * 40 and nbytes.value % 256 == 0
    count = C.c_int(0)
    if lib.mlmcpi_device_count(C.byref(count)) == 0 and count.value > 0:
        return  # a GPU is present: the calls below would run (tests/test_random_sweep_gpu.py covers them)
    assert lib.mlmcpi_lattice_random_sweep_draw(C.byref(good), vp(buf), 1, 1, 1, SEED, 0, 0, vp(work), None) in (-2, -4)
    assert lib.mlmcpi_lattice_random_sweep_order(C.byref(good), 1, SEED, 0, 0, vp(order), None, None) in (-2, -4)
    assert (buf == 3.25).all() and (order == 0xABCDEF01).all() and not work.any()
