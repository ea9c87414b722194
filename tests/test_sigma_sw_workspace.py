"""CPU: the workspace sizes of the three Swendsen-Wang draws (mlmcpi_sigma_sw_workspace_bytes, mlmcpi_sigma_level_sw_workspace_bytes,
_structure_ and _correlator_workspace_bytes) against the layout DESIGN.md 4.6b and include/mlmcpi_hip.h document, restated
here.  The queries are host code: no device is needed.  Callers hold workspaces sized by these numbers, so they are pinned."""
import ctypes as C

import pytest

SHAPES = [(2, 2), (4, 6), (12, 10), (64, 64), (128, 96)]
BATCHES = [1, 3, 300]
STATUS = 256                     # the status word's section


def _a256(nbytes):
    return -(-nbytes // 256) * 256


def _plain(n, owners_bits, B, slots=0):
    """status word, label [B n] uint32, q(a) [B n] int64, cluster sums [B n] int64, `slots` further [B n] int64 sections, bond bits"""
    return STATUS + _a256(4 * B * n) + (2 + slots) * _a256(8 * B * n) + _a256(B * owners_bits)


def _documented(Mt, Mx, rot, B):
    """(plain, structure, correlator) bytes.  Unrotated: n = Mt Mx vertices, one byte of bond bits per vertex.  Rotated: n = Mt Mx / 2,
    one byte per E vertex (n / 2).  Structure: four more root slots.  Correlator: behind the plain draw's, per chain and direction a
    table of 2^lg >= 2 n slots of 16 B, the occupied-slice counts [n] uint32, and per chain n_out = Mt/2 + Mx/2 + 2 int64 lags."""
    n = Mt * Mx // 2 if rot else Mt * Mx
    owners = n // 2 if rot else n
    lg = 1
    while (1 << lg) < 2 * n:
        lg += 1
    n_out = Mt // 2 + Mx // 2 + 2
    plain = _plain(n, owners, B)
    return plain, _plain(n, owners, B, slots=4), plain + _a256(2 * B * (1 << lg) * 16) + _a256(2 * B * n * 4) + _a256(B * n_out * 8)


def _query(lib, name, obj, B):
    size = C.c_size_t(0)
    assert getattr(lib, name)(C.byref(obj), B, C.byref(size)) == 0, name
    return size.value


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("Mt,Mx", SHAPES)
@pytest.mark.parametrize("rot", [0, 1])
def test_the_three_queries_return_the_documented_layout(rot, Mt, Mx, B):
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    lv = abi.sigma_level(Mt, Mx, rot, 1.25)
    plain, structure, correlator = _documented(Mt, Mx, rot, B)
    assert _query(lib, "mlmcpi_sigma_level_sw_workspace_bytes", lv, B) == plain
    assert _query(lib, "mlmcpi_sigma_level_sw_structure_workspace_bytes", lv, B) == structure
    assert _query(lib, "mlmcpi_sigma_level_sw_correlator_workspace_bytes", lv, B) == correlator
    if not rot:                  # an unrotated level IS the lattice: the lattice's own query gives the same size
        act = abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=1.25)
        assert _query(lib, "mlmcpi_sigma_sw_workspace_bytes", act, B) == plain
