"""GPU: the parallel random-order sweep (mlmcpi_lattice_random_sweep_*): the order and the rounds against the numpy model,
parity with the site-at-a-time entry point walking the very same order (and with the oracle's updates on small lattices),
bit-for-bit invariances (sweeps per call, batch split, LDS or global home, rounds per pass), Monte Carlo statistics against
exact values, and host/driver."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import random_sweep_model as rm
import sigma_model as sm
from conftest import zcheck
from test_gpu_parity import HB_TOL, assert_angles_close, assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "driver")
SEED = 0x1234567812345678
I1_OVER_I0 = 0.446390  # I_1(1) / I_0(1): <P> of the quenched Schwinger model at beta = 1


def _act(kind, Mt, Mx, coupling):
    from mlmcpathintegral_amd import abi
    if kind == "schwinger":
        return abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=coupling)
    if kind == "gff":
        return abi.lattice_action(abi.GFF, Mt, Mx, mass=coupling)
    return abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=coupling)


def _start(ops, act, B, seed=SEED, chain0=0):
    from mlmcpathintegral_amd import abi
    if act.kind == abi.GFF:  # any start will do; the library's own is an exact draw through an FFT
        g = torch.Generator(device="cuda").manual_seed(seed % (1 << 31) + chain0)
        return torch.randn((B, act.Mt * act.Mx), dtype=torch.float64, device="cuda", generator=g)
    return ops.lattice_initialise(act, B, seed, chain0)


# ---- 5. the order and the rounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Mt,Mx", [("schwinger", 2, 2), ("schwinger", 5, 4), ("schwinger", 16, 16), ("schwinger", 64, 64),
                                        ("schwinger", 130, 70), ("gff", 16, 16), ("gff", 128, 128), ("sigma", 8, 8)])
def test_order_and_rounds_equal_the_model(gpu_ops, kind, Mt, Mx):
    act = _act(kind, Mt, Mx, 1.0)
    B, chain0, sweep = 3, 41, 1000003
    order, rnd = gpu_ops.lattice_random_sweep_order(act, B, SEED, chain0, sweep)
    order, rnd = order.cpu().numpy().view(np.uint32), rnd.cpu().numpy().view(np.uint32)
    for b in range(B):
        o, r = rm.schedule(act.kind, Mt, Mx, SEED, chain0 + b, sweep)
        assert np.array_equal(order[b], o), f"chain {b}: order"
        assert np.array_equal(rnd[b], r), f"chain {b}: rounds"
    print(f"{kind} {Mt} x {Mx}: rounds per sweep {rnd.max(axis=1).tolist()}, mean round of an index {rnd.mean():.2f}")
    only, none = gpu_ops.lattice_random_sweep_order(act, B, SEED, chain0, sweep, rounds=False)
    assert none is None and np.array_equal(only.cpu().numpy().view(np.uint32), order)


# ---- 6. parity with the site-at-a-time entry point ----------------------------------------------------------------------
def _walk(ops, act, x0, heat, chain0, step):
    """mlmcpi_lattice_site_updates walking every chain's own order: a B = 1 call per chain"""
    B = x0.shape[0]
    order, _ = ops.lattice_random_sweep_order(act, B, SEED, chain0, step, rounds=False)
    want = x0.clone()
    for b in range(B):
        ops.lattice_site_updates(act, want[b:b + 1], order[b].contiguous(), heat, SEED, chain0 + b, step)
    return want, order


def _compare(kind, got, want, heat, what):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    if kind == "gff":
        assert_close(got, want, tol=1e-11, what=what)
    elif kind == "sigma":
        B = got.shape[0]
        d = np.max(np.abs(sm.sigma_of(got.reshape(B, -1, 2)) - sm.sigma_of(want.reshape(B, -1, 2))))
        print(f"{what}: max |diff of unit vectors| = {d:.3e}")
        assert d <= 1e-11, what
    else:
        assert_angles_close(got, want, tol=HB_TOL[1] if heat else 1e-12, what=what)


PARITY = [("schwinger", 16, 16, 1.0, 3), ("schwinger", 64, 64, 1.0, 2), ("schwinger", 6, 8, 1.0, 3), ("schwinger", 6, 8, 3.0, 3),
          ("schwinger", 6, 8, 10.0, 3), ("schwinger", 16, 16, 10.0, 2), ("gff", 16, 16, 3.0, 3), ("sigma", 8, 8, 1.2, 3),
          ("sigma", 16, 16, 0.7, 2),
          # beyond the LDS: the state stays in global memory (the GFF action is defined on square lattices only, here as in
          # the reference: mlmcpi_lattice_site_updates, the yardstick, refuses 257 x 130; the odd extent is kept)
          ("schwinger", 130, 70, 1.0, 2), ("schwinger", 256, 300, 1.0, 2), ("gff", 257, 257, 3.0, 2)]


@pytest.mark.parametrize("kind,Mt,Mx,coupling,B", PARITY)
def test_one_sweep_equals_the_site_at_a_time_walk_in_that_order(gpu_ops, kind, Mt, Mx, coupling, B):
    act = _act(kind, Mt, Mx, coupling)
    chain0, step = 9, 77
    x0 = _start(gpu_ops, act, B, chain0=chain0)
    for heat in (False, True):
        want, _ = _walk(gpu_ops, act, x0, heat, chain0, step)
        got = x0.clone()
        gpu_ops.lattice_random_sweep_draw(act, got, 0 if heat else 1, 1 if heat else 0, SEED, chain0, step)
        assert not torch.equal(got, x0)
        _compare(kind, got, want, heat, f"{kind} {Mt} x {Mx} coupling {coupling:g} heat={heat}")


@pytest.mark.parametrize("kind,Mt,Mx,kw", [("schwinger", 8, 6, dict(beta=1.0)), ("schwinger", 6, 6, dict(beta=3.0)),
                                           ("schwinger", 8, 8, dict(beta=10.0)), ("schwinger", 5, 3, dict(beta=1.0)),
                                           ("gff", 8, 8, dict(mass=3.0)), ("gff", 5, 5, dict(mass=3.0))])
def test_one_sweep_equals_the_oracle_walk(gpu_ops, orc, kind, Mt, Mx, kw):
    """the oracle's dev_site_update applied in the model's order, as test_site_at_a_time_updates_match_oracle does"""
    from test_gpu_parity import dev, make_lattice
    act, A = make_lattice(orc, kind, Mt, Mx, **kw)
    B, chain0, step, n = 3, 5, 21, A.size
    x0 = np.random.default_rng(n).uniform(-np.pi, np.pi, (B, n))
    for heat in (False, True):
        xd = dev(x0)
        gpu_ops.lattice_random_sweep_draw(act, xd, 0 if heat else 1, 1 if heat else 0, SEED, chain0, step)
        want = x0.copy()
        for b in range(B):
            for l in rm.schedule(act.kind, Mt, Mx, SEED, chain0 + b, step)[0]:
                A.dev_site_update(want[b], int(l), heat, SEED, chain0 + b, step)
        if kind == "gff":
            assert_close(xd.cpu().numpy(), want, tol=1e-11, what=f"heat={heat}")
        else:
            assert_angles_close(xd.cpu().numpy(), want, tol=HB_TOL[2] if heat else 1e-12, what=f"heat={heat}")


# ---- 7. invariances, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Mt,Mx,coupling", [("schwinger", 16, 16, 1.0), ("schwinger", 20, 18, 10.0), ("gff", 12, 12, 3.0),
                                                 ("sigma", 8, 8, 1.2)])
def test_draw_does_not_depend_on_calls_batch_home_or_pass_length(gpu_ops, kind, Mt, Mx, coupling):
    from mlmcpathintegral_amd import abi
    act = _act(kind, Mt, Mx, coupling)
    B, chain0, sweep0 = 300, 3, 50
    x0 = _start(gpu_ops, act, B, chain0=chain0)
    one = x0.clone()
    gpu_ops.lattice_random_sweep_draw(act, one, 10, 1, SEED, chain0, sweep0)
    many = x0.clone()
    for s in range(11):
        gpu_ops.lattice_random_sweep_draw(act, many, 1 if s < 10 else 0, 0 if s < 10 else 1, SEED, chain0, sweep0 + s)
    assert torch.equal(one, many), "10 + 1 sweeps in one call differ from eleven calls"
    split = x0.clone()
    gpu_ops.lattice_random_sweep_draw(act, split[:100], 10, 1, SEED, chain0, sweep0)
    gpu_ops.lattice_random_sweep_draw(act, split[100:], 10, 1, SEED, chain0 + 100, sweep0)
    assert torch.equal(one, split), "B = 300 differs from 100 + 200"
    for name, value in (("MLMCPI_RANDOM_SWEEP_HOME", "global"), ("MLMCPI_RANDOM_SWEEP_CHUNK", "3")):
        abi.set_option(name, value)
        try:
            other = x0.clone()
            gpu_ops.lattice_random_sweep_draw(act, other, 10, 1, SEED, chain0, sweep0)
            o2, r2 = gpu_ops.lattice_random_sweep_order(act, 2, SEED, chain0, sweep0)
        finally:
            abi.set_option(name, "")
        assert torch.equal(one, other), f"{name}={value} changes the draw"
        o1, r1 = gpu_ops.lattice_random_sweep_order(act, 2, SEED, chain0, sweep0)
        assert torch.equal(o1, o2) and torch.equal(r1, r2), f"{name}={value} changes the schedule"


# ---- 8. statistics ------------------------------------------------------------------------------------------------------
def _chain_mean(q):
    """q [draws, B]: mean and error from the spread of the per-chain means (chains are independent)"""
    m = q.mean(axis=0)
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(len(m)))


def _run(ops, act, B, burnin, draws, n_or, qois):
    x = _start(ops, act, B, seed=SEED + 1)
    work = ops.lattice_random_sweep_workspace(act, B)
    out = [[] for _ in qois]
    for d in range(burnin + draws):
        ops.lattice_random_sweep_draw(act, x, n_or, 1, SEED + 1, 0, d * (n_or + 1), work=work)
        if d >= burnin:
            for k, q in enumerate(qois):
                out[k].append(q(x).cpu().numpy())
    return [_chain_mean(np.array(o)) for o in out]


def test_schwinger_plaquette_in_random_order(gpu_ops):
    act = _act("schwinger", 16, 16, 1.0)
    (m, e), = _run(gpu_ops, act, 2048, 20, 20, 10, [lambda x: gpu_ops.qoi_avg_plaquette(x, 16, 16)])
    assert e <= 1e-3 * I1_OVER_I0
    zcheck("random-order sweep: Schwinger 16^2 beta=1 <P> vs I1/I0", m, e, I1_OVER_I0)


def test_gff_phi_squared_in_random_order(gpu_ops):
    import oracle
    act = _act("gff", 16, 16, 10.0)
    exact = oracle.lib().orc_gff_phi_squared_analytical(10.0, 16, 16)
    (m, e), = _run(gpu_ops, act, 4096, 5, 20, 2, [lambda x: gpu_ops.qoi_phi_squared(x)])
    assert e <= 1e-3 * exact
    zcheck("random-order sweep: GFF 16^2 <phi^2> vs closed form", m, e, exact)


@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_sigma_ring_in_random_order(gpu_ops, beta):
    act = _act("sigma", 2, 2, beta)
    S_exact, chi_exact = sm.ring_exact(beta)
    (ms, es), (mc, ec) = _run(gpu_ops, act, 32768, 20, 60, 2, [lambda x: gpu_ops.lattice_evaluate(act, x),
                                                             lambda x: gpu_ops.qoi_magnetic_susceptibility(x, 2, 2)])
    assert es <= 1e-3 * abs(S_exact) and ec <= 1e-3 * chi_exact, (es / abs(S_exact), ec / chi_exact)
    zcheck(f"random-order sweep: sigma 2x2 beta={beta:g} <S>", ms, es, S_exact)
    zcheck(f"random-order sweep: sigma 2x2 beta={beta:g} <chi_m>", mc, ec, chi_exact)


# ---- 9. host/driver -----------------------------------------------------------------------------------------------------
def _driver(*args, timeout=600):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def test_driver_schwinger_in_device_random_order():
    r = _driver("--action", "schwinger", "--Mt_lat", "16", "--beta", "1", "--sampler", "heatbath", "--random_order", "2",
                "--n_samples", "4000")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "device order" in r.stderr
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    zcheck("host/driver --random_order 2: Schwinger 16^2 beta=1 <P> vs I1/I0", float(m.group(1)), float(m.group(2)), I1_OVER_I0)


def test_driver_refuses_the_device_random_order_for_1d_actions():
    r = _driver("--action", "rotor", "--M_lat", "64", "--T_final", "6.4", "--m0", "0.25", "--sampler", "heatbath",
                "--random_order", "2", "--n_samples", "10")
    assert r.returncode != 0
    assert "the parallel random order is built for the 2-D actions" in r.stdout + r.stderr
