"""CPU: mlmcpi_schwinger_wilson_loops_plan and _workspace_bytes (host only) against the rule restated in
tests/wilson_loops_reference.py, every status code, and the invariant that the tiles cover every base vertex exactly once."""
import ctypes as C
import itertools

import numpy as np
import pytest

import wilson_loops_reference as ref

T = ref.TILE
EXTENTS = [2, 3, 17, T - 1, T, T + 1, 130, 1024]
SIDES = [1, 2, 15, 16]


def _plan(Mt, Mx, R, S, B):
    from mlmcpathintegral_amd import abi
    lib, info = abi.load(), abi.WilsonLoopsPlan()
    rc = lib.mlmcpi_schwinger_wilson_loops_plan(Mt, Mx, R, S, B, C.byref(info))
    return rc, ({n: getattr(info, n) for n, _ in abi.WilsonLoopsPlan._fields_} if rc == 0 else None)


def _bytes(Mt, Mx, R, S, B):
    from mlmcpathintegral_amd import abi
    n = C.c_size_t(0)
    return abi.load().mlmcpi_schwinger_wilson_loops_workspace_bytes(Mt, Mx, R, S, B, C.byref(n)), n.value


@pytest.mark.parametrize("Mt", EXTENTS)
def test_plan_and_workspace_follow_the_rule(Mt):
    for Mx, R, S, B in itertools.product(EXTENTS, SIDES, SIDES, (1, 3)):
        want = ref.plan(Mt, Mx, R, S, B)
        assert _plan(Mt, Mx, R, S, B) == want, (Mt, Mx, R, S, B)
        rc, n = _bytes(Mt, Mx, R, S, B)
        assert rc == want[0] and (rc != 0 or n == want[1]["work_bytes"]), (Mt, Mx, R, S, B)
        if want[0] == 0:
            p = want[1]
            assert p["lds_bytes"] <= p["lds_limit"] // 2 + 4096 and p["work_bytes"] % 256 == 0 and p["work_bytes"] >= B * p["tiles"] * R * S * 8


def test_the_header_names_the_cap():
    from mlmcpathintegral_amd import ops
    assert ops.wilson_loops_plan(64, 64, ref.CAP, ref.CAP, 1)["halo_w"] == ref.CAP - 1
    assert _plan(64, 64, ref.CAP + 1, 1, 1)[0] == ref.ERR_UNSUPPORTED and _plan(64, 64, 1, ref.CAP + 1, 1)[0] == ref.ERR_UNSUPPORTED


@pytest.mark.parametrize("args,status", [
    ((1, 8, 1, 1, 1), ref.ERR_INVALID), ((8, 1, 1, 1, 1), ref.ERR_INVALID), ((0, 0, 1, 1, 1), ref.ERR_INVALID),
    ((2 ** 16, 2 ** 15, 1, 1, 1), ref.ERR_INVALID), ((2 ** 15, 2 ** 15, 1, 1, 1), ref.OK),
    ((8, 8, 1, 1, 0), ref.ERR_INVALID), ((8, 8, 0, 1, 1), ref.ERR_INVALID), ((8, 8, 1, 0, 1), ref.ERR_INVALID),
    ((8, 8, 9, 1, 1), ref.ERR_INVALID), ((8, 8, 1, 9, 1), ref.ERR_INVALID), ((8, 8, 8, 8, 1), ref.OK),
    ((64, 64, 17, 1, 1), ref.ERR_UNSUPPORTED), ((64, 64, 1, 17, 1), ref.ERR_UNSUPPORTED), ((8, 8, 17, 17, 1), ref.ERR_UNSUPPORTED),
    ((2 ** 15, 2 ** 15, 1, 1, 2 ** 20), ref.ERR_INVALID),           # 2^40 workgroups: beyond the grid
    ((64, 64, 4, 4, 2 ** 32 - 1), ref.OK),                           # chains ride the linear workgroup index: no 65535 limit
])
def test_every_status_code(args, status):
    from mlmcpathintegral_amd import abi
    assert ref.plan(*args)[0] == status
    assert _plan(*args)[0] == status and _bytes(*args)[0] == status
    if status != 0:
        assert abi.load().mlmcpi_last_error()


def test_null_outputs_are_invalid():
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    assert lib.mlmcpi_schwinger_wilson_loops_plan(8, 8, 2, 2, 1, None) == ref.ERR_INVALID
    assert lib.mlmcpi_schwinger_wilson_loops_workspace_bytes(8, 8, 2, 2, 1, None) == ref.ERR_INVALID


@pytest.mark.parametrize("Mt,Mx", [(2, 2), (3, 17), (T - 1, T + 1), (T, T), (130, 70), (1024, T + 1)])
def test_the_tiles_cover_every_base_vertex_once(Mt, Mx):
    rc, p = _plan(Mt, Mx, 2, 2, 1)
    assert rc == 0
    count = np.zeros((Mx, Mt), dtype=np.int32)
    ranges = ref.tile_ranges(p, Mt, Mx)
    assert len(ranges) == p["tiles"] == p["grid"]
    for i0, i1, j0, j1 in ranges:
        assert 0 < i1 - i0 <= p["tile_w"] and 0 < j1 - j0 <= p["tile_h"]
        count[j0:j1, i0:i1] += 1
    assert np.all(count == 1)
    # every thread's run of J base rows lies in the tile: workgroup / tile_w row groups of J rows make up tile_h
    assert p["workgroup"] // p["tile_w"] * p["J"] == p["tile_h"]
