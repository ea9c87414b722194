"""The closed-form Schwinger sweeps on the plane packed to its read set (schwinger_perm.hpp: one build per workgroup at
every depth) against the sweep-by-sweep kernels (MLMCPI_OR_KERNEL=block: the updates of quenchedschwingeraction.cc:57-65
one colour phase at a time), on the lattices where the packing can go wrong: 64 x 64 (the plane wraps round the lattice
twice), 128 x 128 (smallest fused launch: four tiles, each the other's neighbour across the wrap), 130 x 70 (ragged,
64 x 32 tiles) and 192 x 128; depths 1, 6, 7 (where the plane used to be split in two) and 10 (the pitch is full).

Tolerance: that of tests/test_closed_form.py for the same two arithmetics, 4e-15 (2 K + 2) 8 -- the closed form adds 2 K
plaquettes of four angles each per link where the sweeps add them one update at a time.  Behind a heat-bath sweep the
same bound is asked of the states (both plans then run the same sampler on the same Philox words; a draw moves with its
staple at slope <= 1), and the average plaquette, a mean of cosines of sums of four angles, may differ by 4 times it."""
import numpy as np
import pytest
import torch

from mlmcpathintegral_amd import abi

pytestmark = pytest.mark.gpu
SEED = 0x1234567812345678
DEPTHS = (1, 6, 7, 10)


def _draws(ops, act, x0, K, n_hb):
    a, b = x0.clone(), torch.empty_like(x0)
    state, _ = ops.lattice_sweep_draw_pingpong(act, a, b, K, n_hb, SEED, 0, 5)
    q = None
    if n_hb:
        xq, _, q = ops.lattice_sweep_draw_qoi(act, x0.clone(), torch.empty_like(x0), torch.empty_like(x0), K, n_hb, SEED, 0, 5, 1)
        assert torch.equal(xq, state), "the draw with the QoI is the draw without it"
    return state.clone(), q


@pytest.mark.parametrize("Mt,Mx", [(64, 64), (128, 128), (130, 70), (192, 128)])
def test_packed_plane_matches_the_sweep_by_sweep_kernels(gpu_ops, Mt, Mx):
    ops = gpu_ops
    act = abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=1.0)
    x0 = ops.lattice_initialise(act, 2, 17, 0)
    for K in DEPTHS:
        tol = 4e-15 * (2 * K + 2) * 8
        for n_hb in (0, 1):
            plan = ops.lattice_sweep_plan(act, 2, K, n_hb)
            assert plan[0]["instantiation"].startswith("schwinger_perm") and plan[0]["n_overrelax"] == K and plan[0]["planes"] == 1
            got, q = _draws(ops, act, x0, K, n_hb)
            abi.set_option("MLMCPI_OR_KERNEL", "block")
            try:
                want, qw = _draws(ops, act, x0, K, n_hb)
            finally:
                abi.set_option("MLMCPI_OR_KERNEL", "")
            d = (got - want).cpu().numpy()
            err = float(np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi))).max())
            print(f"{Mt} x {Mx} K = {K} heat bath {n_hb}: max angular difference {err:.3e} (bound {tol:.3e})")
            assert err <= tol, f"{Mt} x {Mx}, K = {K}, {n_hb} heat-bath sweeps: {err:.3e} > {tol:.3e}"
            if n_hb:
                dq = float((q - qw).abs().max())
                print(f"    average plaquette differs by {dq:.3e}")
                assert dq <= 4 * tol, f"{Mt} x {Mx}, K = {K}: QoI {dq:.3e}"
