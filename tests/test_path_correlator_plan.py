"""mlmcpi_path_correlator_plan (host only: the geometry pc_plan of path_correlator.hip chooses from (kind, M, n_lag)) against
the rule as tests/path_correlator_reference.py restates it, and the invariants every plan must keep.  Nothing here needs a
device."""
import ctypes as C
import os
import re

import pytest

import path_correlator_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_M = (1, 2, 7, 64, 128, 130, 1026, 4096, 8200, 20000, 2 ** 20)
GRID_B = (1, 3, 300, 70000)


def lags(kind, M):
    cap = ref.lag_cap(kind)
    return sorted({1, 2, ref.T - 1, ref.T, ref.T + 1, M // 2 + 1, cap, cap + 1})


def raw_plan(kind, M, n_lag, B):
    """(status, plan or None) straight through the ABI"""
    from mlmcpathintegral_amd import abi
    act = abi.path_action(kind, M, 4.0)
    info = abi.PathCorrelatorPlan(*([0xFFFFFFFF] * 15))
    rc = abi.load().mlmcpi_path_correlator_plan(C.byref(act), n_lag, B, C.byref(info))
    return rc, ({n: getattr(info, n) for n, _ in abi.PathCorrelatorPlan._fields_} if rc == 0 else None)


@pytest.fixture(scope="module")
def grid():
    return {(k, M, n, B): raw_plan(k, M, n, B) for k in (0, 1, 2) for M in GRID_M for n in lags(k, M) for B in GRID_B}


def test_query_equals_the_restated_rule(grid):
    for key, got in grid.items():
        assert got == ref.plan(*key), (key, got, ref.plan(*key))
    status = [rc for rc, _ in grid.values()]
    assert status.count(ref.OK) > 300 and status.count(ref.ERR_INVALID) > 100 and status.count(ref.ERR_UNSUPPORTED) >= 3 * 4


def test_status_codes(grid):
    for (kind, M, n_lag, B), (rc, _) in grid.items():
        if n_lag > M // 2 + 1:
            assert rc == ref.ERR_INVALID, (kind, M, n_lag, B)
        elif n_lag > ref.lag_cap(kind):
            assert rc == ref.ERR_UNSUPPORTED, (kind, M, n_lag, B)
        else:
            assert rc == ref.OK, (kind, M, n_lag, B)
    assert ref.lag_cap(0) == ref.lag_cap(1) == 6544 and ref.lag_cap(2) == 3264
    from mlmcpathintegral_amd import abi
    lib, info, size = abi.load(), abi.PathCorrelatorPlan(), C.c_size_t(0)
    act = abi.path_action(abi.HARMONIC, 64, 4.0)
    assert lib.mlmcpi_path_correlator_plan(C.byref(act), 33, 3, C.byref(info)) == ref.OK
    for bad in ((None, 33, 3, C.byref(info)), (C.byref(act), 0, 3, C.byref(info)), (C.byref(act), 33, 0, C.byref(info)),
                (C.byref(act), 34, 3, C.byref(info)), (C.byref(act), 33, 3, None)):
        assert lib.mlmcpi_path_correlator_plan(*bad) == ref.ERR_INVALID, bad
    for kind, M in ((-1, 64), (3, 64), (0, 0)):
        a = abi.path_action(abi.HARMONIC, 64, 4.0)
        a.kind, a.M = kind, M
        assert lib.mlmcpi_path_correlator_plan(C.byref(a), 1, 3, C.byref(info)) == ref.ERR_INVALID
        assert lib.mlmcpi_path_correlator_workspace_bytes(C.byref(a), 1, 3, C.byref(size)) == ref.ERR_INVALID
    # the cap, where the lattice allows it and one lag beyond: the same status from the workspace query
    for kind in (0, 2):
        cap = ref.lag_cap(kind)
        a = abi.path_action(kind, 2 * cap, 4.0)
        assert lib.mlmcpi_path_correlator_workspace_bytes(C.byref(a), cap, 1, C.byref(size)) == ref.OK
        assert lib.mlmcpi_path_correlator_workspace_bytes(C.byref(a), cap + 1, 1, C.byref(size)) == ref.ERR_UNSUPPORTED
        assert b"at most %d lags" % cap in lib.mlmcpi_last_error()
    # chains are no grid dimension of their own: 2^31 / 256 workgroups and more are taken
    a = abi.path_action(abi.HARMONIC, 4096, 4.0)
    assert lib.mlmcpi_path_correlator_plan(C.byref(a), 8, 2 ** 31 // 256 + 1, C.byref(info)) == ref.OK and info.grid == 2 ** 31 // 256 + 1
    assert lib.mlmcpi_path_correlator_plan(C.byref(a), 8, 2 ** 32 - 1, C.byref(info)) == ref.OK and info.grid == 2 ** 32 - 1


def test_plans_keep_their_invariants(grid):
    seen = set()
    for (kind, M, n_lag, B), (rc, p) in grid.items():
        if rc:
            continue
        key = (kind, M, n_lag, B, p)
        # owned ranges tile [0, M) exactly once
        ranges = [(s * p["owned"], min(M, (s + 1) * p["owned"])) for s in range(p["nseg"])]
        assert ranges[0][0] == 0 and ranges[-1][1] == M and all(lo < hi for lo, hi in ranges), key
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), key
        assert p["nseg"] == 1 or p["owned"] % p["J"] == 0, key
        # lag tiles cover [0, n_lag) exactly once
        tiles = [(q * p["T"], min(n_lag, (q + 1) * p["T"])) for q in range(p["lag_tiles"])]
        assert tiles[0][0] == 0 and tiles[-1][1] == n_lag and all(lo < hi for lo, hi in tiles), key
        # the image holds a segment's tiles and the window of the last pair (site tile, lag tile), and fits the LDS
        own_tiles = -(-min(p["owned"], M) // p["J"])
        assert p["image_tiles"] >= (own_tiles - 1) + (p["lag_tiles"] - 1) + 2, key
        assert p["lds_bytes"] == p["chains_per_workgroup"] * p["components"] * p["image_tiles"] * 80, key
        assert p["lds_bytes"] <= p["lds_limit"] == 65536, key
        assert p["workgroup"] == 256 == 64 * p["chains_per_workgroup"] * p["waves_per_chain"], key
        assert p["group"] in (1, 2, 4, 8, 16, 32, 64) and (p["group"] == 64 or p["group"] >= own_tiles), key
        assert p["grid"] == -(-B // p["chains_per_workgroup"]) * p["nseg"] <= ref.MAX_BLOCKS, key
        seen.add((p["nseg"] > 1, p["chains_per_workgroup"]))
    assert seen == {(False, 4), (False, 1), (True, 1)}


def test_geometry_is_independent_of_the_batch(grid):
    for (kind, M, n_lag, B), (rc, p) in grid.items():
        rc1, p1 = grid[(kind, M, n_lag, 1)]
        assert rc == rc1
        if rc == 0:
            drop = ("grid", "work_bytes")
            assert {k: v for k, v in p.items() if k not in drop} == {k: v for k, v in p1.items() if k not in drop}


def test_new_symbols_are_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    for name in ("mlmcpi_path_correlator", "mlmcpi_path_correlator_workspace_bytes", "mlmcpi_path_correlator_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in abi.SIGNATURES
    body = re.search(r"typedef struct mlmcpi_path_correlator_plan_info \{(.*?)\} mlmcpi_path_correlator_plan_info;", header, flags=re.S).group(1)
    declared = [(t, n.strip()) for t, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body) for n in names.split(",")]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for t, n in declared] == list(abi.PathCorrelatorPlan._fields_)
    act = abi.path_action(abi.ROTOR, 20000, 4.0, 0.25)
    assert ops.path_correlator_plan(act, 64, 2) == ref.plan(2, 20000, 64, 2)[1]
    assert ops.path_correlator_plan(act, 64, 2)["nseg"] >= 3
    with pytest.raises(abi.MlmcpiError, match="beyond M / 2 \\+ 1"):
        ops.path_correlator_plan(act, 10002, 2)
