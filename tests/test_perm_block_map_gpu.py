"""The closed-form Schwinger sweeps with a wave's tasks as a BLOCK of consecutive row pairs (schwinger_perm.hpp, PermTasks:
a mu = 0 thread sums the stream two neighbouring row pairs share once and hands it down its block) against the
sweep-by-sweep kernels of the same draw (MLMCPI_OR_KERNEL=block: one colour phase at a time), on the smallest shapes at
which the map can go wrong:

  128 x 128, 3 chains   the fused launch at its minimum size (every tile has every neighbour across the wrap), in BOTH
                        workgroup widths: 512 threads (MLMCPI_OR_HEAT=narrow: 8 waves, blocks of 5 and 4 row pairs plus the
                        left-over columns) and 1024 (wide, with one chain too: 16 waves, blocks of 3 and 2)
  64 x 64               the closed-form kernel alone; the plane is its own halo several times over
  64 x 32, 96 x 32      its TH = 32 instance (blocks of 2)
  130 x 70              masked edge tiles on 64 x 32 tiles
  192 x 136             the fused launch with the last tile row masked

at the depths K = 1 (every stream is one plaquette), 2, 5 (one batch of five reads per stream), 6 (a batch and a tail)
and 10, with and without the heat-bath sweep and the QoI.  States are compared element by element; the first link that
differs is reported as (chain, row, column, mu), so that a wrong hand-over shows as the row pair it belongs to.

Tolerance: that of tests/test_perm_plane_packed_gpu.py and tests/test_closed_form.py for the same two arithmetics,
4e-15 (2 K + 2) 8 -- the closed form adds 2 K plaquettes of four angles each per link where the sweeps add them one update
at a time; behind a heat-bath sweep the same bound on the states, and 4 times it on the average plaquette."""
import numpy as np
import pytest
import torch

from mlmcpathintegral_amd import abi

pytestmark = pytest.mark.gpu
SEED = 0x1234567812345678
DEPTHS = (1, 2, 5, 6, 10)
PERM64, PERM32 = "schwinger_perm_kernel<64>", "schwinger_perm_kernel<32>"
HEAT512, HEAT1024 = "schwinger_perm_heat_kernel<512, true>", "schwinger_perm_heat_kernel<1024, true>"
TILE_HEAT = "schwinger_sweep_kernel<true, 256, 0, 0, true>"

# (Mt, Mx, chains, MLMCPI_OR_HEAT, first launch without heat bath, launches with it): instantiation, grid x, threads, LDS bytes
# -- what mlmcpi_lattice_sweep_plan answered for these shapes BEFORE the slot map changed (the map is internal to the kernels)
CASES = [
    (128, 128, 3, "narrow", (PERM64, 4, 512, 65536), [(HEAT512, 4, 512, 77408)]),
    (128, 128, 3, "wide", (PERM64, 4, 512, 65536), [(HEAT1024, 4, 1024, 77408)]),
    (128, 128, 1, "wide", (PERM64, 4, 512, 65536), [(HEAT1024, 4, 1024, 77408)]),
    (64, 64, 2, "", (PERM64, 1, 512, 65536), [(PERM64, 1, 512, 65536), (TILE_HEAT, 2, 256, 40864)]),
    (64, 32, 2, "", (PERM32, 1, 512, 34944), [(PERM32, 1, 512, 34944), (TILE_HEAT, 1, 256, 40864)]),
    (96, 32, 2, "", (PERM32, 2, 512, 34944), [(PERM32, 2, 512, 34944), (TILE_HEAT, 2, 256, 40864)]),
    (130, 70, 2, "", (PERM32, 9, 512, 34944), [(PERM32, 9, 512, 34944), (TILE_HEAT, 9, 256, 40864)]),
    (192, 136, 2, "narrow", (PERM64, 9, 512, 65536), [(HEAT512, 9, 512, 77408)]),
    (192, 136, 2, "wide", (PERM64, 9, 512, 65536), [(HEAT1024, 9, 1024, 77408)]),
]
IDS = [f"{c[0]}x{c[1]}-B{c[2]}-{c[3] or 'default'}" for c in CASES]


class options:
    def __init__(self, **kw):
        self.kw = {k: v for k, v in kw.items() if v}

    def __enter__(self):
        for k, v in self.kw.items():
            abi.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            abi.set_option(k, "")


def _draws(ops, act, x0, K, n_hb):
    a, b = x0.clone(), torch.empty_like(x0)
    state, _ = ops.lattice_sweep_draw_pingpong(act, a, b, K, n_hb, SEED, 0, 5)
    state = state.clone()
    q = None
    if n_hb:
        xq, _, q = ops.lattice_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), K, n_hb, SEED, 0, 5, 1)
        assert torch.equal(xq, state), "the draw with the QoI is the draw without it"
    return state, q


def _first_difference(got, want, Mt, Mx, tol):
    """(max angular difference, the first link beyond tol as text)"""
    d = (got - want).cpu().numpy().reshape(-1, Mx, Mt, 2)
    d = np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi)))
    bad = np.argwhere(d > tol)
    where = ""
    if len(bad):
        b, r, c, mu = (int(v) for v in bad[0])
        where = f"first at chain {b}, row {r}, column {c}, mu {mu}: {d[b, r, c, mu]:.3e}; {len(bad)} links differ"
    return float(d.max()), where


def _plan_rows(ops, act, B, K, n_hb):
    return [(l["instantiation"], l["grid_x"], l["threads"], l["lds_bytes"]) for l in ops.lattice_sweep_plan(act, B, K, n_hb)]


@pytest.mark.parametrize("Mt,Mx,B,heat_opt,alone,with_heat", CASES, ids=IDS)
def test_block_map_matches_the_sweep_by_sweep_kernels(gpu_ops, Mt, Mx, B, heat_opt, alone, with_heat):
    ops = gpu_ops
    act = abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=1.0)
    x0 = ops.lattice_initialise(act, B, 17, 0)
    for K in DEPTHS:
        tol = 4e-15 * (2 * K + 2) * 8
        for n_hb in (0, 1):
            with options(MLMCPI_OR_HEAT=heat_opt):
                # plan invariance: kernel, grid, threads and LDS bytes are what they were
                assert _plan_rows(ops, act, B, K, n_hb) == ([alone] if n_hb == 0 else with_heat), (K, n_hb)
                got, q = _draws(ops, act, x0, K, n_hb)
            with options(MLMCPI_OR_KERNEL="block"):
                want, qw = _draws(ops, act, x0, K, n_hb)
            err, where = _first_difference(got, want, Mt, Mx, tol)
            print(f"{Mt} x {Mx} B = {B} {heat_opt or 'default'} K = {K} heat bath {n_hb}: max angular difference {err:.3e} (bound {tol:.3e})")
            assert err <= tol, f"{Mt} x {Mx}, K = {K}, {n_hb} heat-bath sweeps: {err:.3e} > {tol:.3e}; {where}"
            if n_hb:
                dq = float((q - qw).abs().max())
                print(f"    average plaquette differs by {dq:.3e}")
                assert dq <= 4 * tol, f"{Mt} x {Mx}, K = {K}: QoI {dq:.3e}"


def test_closed_form_stage_is_the_same_in_every_kernel(gpu_ops):
    """schwinger_perm.hpp's definition: a result depends on the field and K only, not on the kernel, the workgroup size or the
    lane.  At 128 x 128, K = 10: the closed-form kernel alone (8 waves, no left-over columns), then the heat-bath sweep as a
    launch of its own (MLMCPI_OR_HEAT=split), against the fused launch in both widths -- whose closed-form stages have
    other blocks per wave (8 and 16 waves over 17 row pairs and the columns beyond 64) -- bit for bit, element by element."""
    ops = gpu_ops
    act = abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0)
    x0 = ops.lattice_initialise(act, 3, 23, 0)
    res = {}
    for mode in ("split", "narrow", "wide"):
        with options(MLMCPI_OR_HEAT=mode):
            res[mode], _ = _draws(ops, act, x0, 10, 1)
    for mode in ("narrow", "wide"):
        err, where = _first_difference(res[mode], res["split"], 128, 128, 0.0)
        assert torch.equal(res[mode], res["split"]), f"{mode} against split: {where}"
