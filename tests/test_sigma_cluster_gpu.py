"""GPU: the Wolff single-cluster update of the O(3) sigma model (mlmcpi_sigma_cluster_draw, sigma_cluster.hip) against its
numpy restatement (tests/sigma_cluster_model.py) update by update, its invariances bit for bit (call split, batch split, every
knob of the launch plan), its law against the device heat bath and the CPU model, and host/driver --sampler wolff."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sigma_cluster_model as scm
import sigma_model as sm
from conftest import zcheck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [("wave", "lds"), ("wave", "global"), ("block", "lds"), ("block", "global")]


def _act(ops, Mt, Mx, beta):
    from mlmcpathintegral_amd import abi
    return abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=beta)


def _thermalised(ops, act, B, seed, draws=2, aligned=False):
    """device states with some order in them: a random (or all-aligned) start, then `draws` heat-bath draws of 10 + 1 sweeps"""
    x = ops.lattice_initialise(act, B, seed)
    if aligned:
        x[:, 0::2] = 0.5 * math.pi
        x[:, 1::2] = 0.25
    w = torch.empty_like(x)
    for d in range(draws):
        ops.lattice_sweep_draw(act, x, w, 10, 1, seed, 0, 11 * d)
    return x


class _plan:
    """a launch plan forced through mlmcpi_set_option, the defaults restored on exit"""

    def __init__(self, team, bitmap):
        self.team, self.bitmap = team, bitmap

    def __enter__(self):
        from mlmcpathintegral_amd import abi
        abi.set_option("MLMCPI_SIGMA_CLUSTER_TEAM", self.team)
        abi.set_option("MLMCPI_SIGMA_CLUSTER_BITMAP", self.bitmap)

    def __exit__(self, *exc):
        from mlmcpathintegral_amd import abi
        abi.set_option("MLMCPI_SIGMA_CLUSTER_TEAM", "")
        abi.set_option("MLMCPI_SIGMA_CLUSTER_BITMAP", "")


# ---- 5. parity, update by update -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [1.0, 1.5])
@pytest.mark.parametrize("Mt,Mx,B,n", [(2, 2, 5, 12), (4, 6, 5, 12), (16, 16, 4, 10), (130, 70, 3, 5), (256, 300, 2, 4)])
def test_every_update_equals_the_model(gpu_ops, Mt, Mx, B, n, beta):
    """each device update against the model applied to the device's own previous state: same flipped set, unit vectors to
    1e-11, same count.  A bond whose uniform lies within 1e-10 of its probability could flip between two libms: the margin
    is asserted (seeds chosen so that every case clears it), never skipped."""
    ops, N = gpu_ops, Mt * Mx
    act = _act(ops, Mt, Mx, beta)
    seed, chain0, update0 = 1000 + Mt + int(10 * beta), 3, 40
    x = _thermalised(ops, act, B, seed)
    work = ops.sigma_cluster_workspace(act, B)
    largest = 0
    for k in range(n):
        before = x.cpu().numpy()
        sites = ops.sigma_cluster_draw(act, x, 1, seed, chain0, update0 + k, work=work).cpu().numpy()
        after = x.cpu().numpy()
        for b in range(B):
            want, info = scm.dev_update(before[b], Mt, Mx, beta, seed, chain0 + b, update0 + k)
            print(f"{Mt}x{Mx} beta={beta} update {k} chain {b}: cluster {len(info['sites'])}, margin {info['margin']:.3g}")
            assert info["margin"] > 1e-10, "a bond decision within 1e-10 of its uniform: change the seed"
            changed = np.nonzero(np.any(after[b].reshape(N, 2) != before[b].reshape(N, 2), axis=1))[0]
            assert np.array_equal(changed, info["sites"]), (k, b, len(changed), len(info["sites"]))
            assert sites[b] == len(info["sites"])
            d = np.abs(sm.unit_vectors(after[b][None], Mt, Mx) - sm.unit_vectors(want[None], Mt, Mx)).max()
            assert d < 1e-11, (k, b, d)
            largest = max(largest, len(info["sites"]))
    assert largest > 1


# ---- 6. invariances, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B,beta", [(2, 2, 8, 1.5), (16, 16, 8, 1.0), (130, 70, 8, 1.5), (256, 300, 8, 1.5), (1024, 1024, 4, 1.5)])
def test_call_split_batch_split_and_launch_plans_give_the_same_bits(gpu_ops, Mt, Mx, B, beta):
    ops = gpu_ops
    act = _act(ops, Mt, Mx, beta)
    seed, chain0, update0 = 77 + Mt, 5, 1000
    x0 = _thermalised(ops, act, B, seed, aligned=Mt == 1024)   # 1024^2 at beta = 1.5 from order: clusters span the lattice
    ref = x0.clone()
    count = ops.sigma_cluster_draw(act, ref, 10, seed, chain0, update0)
    mean = count.double().mean().item() / 10
    print(f"{Mt} x {Mx} beta = {beta}: {mean:.1f} flipped vertices per update ({mean / (Mt * Mx):.3f} of the lattice)")
    assert mean > 1 and not torch.equal(ref, x0)
    if Mt == 1024:
        assert mean > 0.05 * Mt * Mx, "the large case is there for clusters that span a sizeable share of the lattice"

    a = x0.clone()
    c1 = ops.sigma_cluster_draw(act, a, 5, seed, chain0, update0)
    c2 = ops.sigma_cluster_draw(act, a, 5, seed, chain0, update0 + 5)
    assert torch.equal(a, ref) and torch.equal(c1 + c2, count)

    h = B // 2
    lo, hi = x0[:h].clone(), x0[h:].clone()
    cl = ops.sigma_cluster_draw(act, lo, 10, seed, chain0, update0)
    ch = ops.sigma_cluster_draw(act, hi, 10, seed, chain0 + h, update0)
    assert torch.equal(torch.cat([lo, hi]), ref) and torch.equal(torch.cat([cl, ch]), count)

    for team, bitmap in PLANS:
        with _plan(team, bitmap):
            y = x0.clone()
            c = ops.sigma_cluster_draw(act, y, 10, seed, chain0, update0)
        assert torch.equal(y, ref) and torch.equal(c, count), (team, bitmap)


def test_unknown_plan_values_are_refused(gpu_ops):
    from mlmcpathintegral_amd import abi
    with pytest.raises(abi.MlmcpiError):
        abi.set_option("MLMCPI_SIGMA_CLUSTER_TEAM", "lane")
    with pytest.raises(abi.MlmcpiError):
        abi.set_option("MLMCPI_SIGMA_CLUSTER_BITMAP", "registers")


# ---- 7. statistics -----------------------------------------------------------------------------------------------------------
def _chain_means(samples, B):
    m = torch.stack(samples).mean(dim=0).cpu().numpy()
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(B))


@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_chi_m_agrees_with_the_heat_bath_and_with_the_cpu_model(gpu_ops, beta):
    ops = gpu_ops
    Mt = Mx = 16
    act = _act(ops, Mt, Mx, beta)
    B, burn, meas = 512, 100, 300

    def wolff(x, seed):
        work = ops.sigma_cluster_workspace(act, B)
        chi = []
        for d in range(burn + meas):
            ops.sigma_cluster_draw(act, x, 10, seed, 0, 10 * d, count=False, work=work)
            if d >= burn:
                chi.append(ops.qoi_magnetic_susceptibility(x, Mt, Mx))
        return _chain_means(chi, B)

    w, w_err = wolff(ops.lattice_initialise(act, B, 31), 32)
    aligned = torch.empty((B, 2 * Mt * Mx), dtype=torch.float64, device="cuda")
    aligned[:, 0::2] = 0.5 * math.pi
    aligned[:, 1::2] = 0.25
    wa, wa_err = wolff(aligned, 33)
    zcheck(f"sigma Wolff chi_m 16x16 beta={beta}: aligned start vs random start", wa, wa_err, w, w_err)

    x = ops.lattice_initialise(act, B, 34)
    scratch = torch.empty_like(x)
    chi = []
    for d in range(burn + meas):
        ops.lattice_sweep_draw(act, x, scratch, 10, 1, 35, 0, 11 * d)
        if d >= burn:
            chi.append(ops.qoi_magnetic_susceptibility(x, Mt, Mx))
    h, h_err = _chain_means(chi, B)
    zcheck(f"sigma Wolff chi_m 16x16 beta={beta}: device Wolff vs device heat bath", w, w_err, h, h_err)

    Bc = 48
    phi = sm.initialise(Bc, Mt, Mx, 36)
    chi = []
    for step in range(1500):
        phi, _ = scm.dev_update_batch(phi, Mt, Mx, beta, 37, 0, step)
        if step >= 500:
            chi.append(sm.magnetic_susceptibility(phi, Mt, Mx))
    c = np.mean(chi, axis=0)
    zcheck(f"sigma Wolff chi_m 16x16 beta={beta}: device Wolff vs CPU model chain", w, w_err, float(c.mean()),
           float(c.std(ddof=1) / math.sqrt(Bc)))


# ---- 8. driver ---------------------------------------------------------------------------------------------------------------
def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


def _avg_err(out):
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


def test_driver_wolff_agrees_with_the_heat_bath_sampler():
    common = ["--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1", "--n_samples", "4000", "--n_burnin", "100"]
    r = _driver(*common, "--sampler", "wolff", "--n_updates", "10")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    w, w_err = _avg_err(r.stdout)
    m = re.search(r"mean cluster size\s+= ([0-9.]+) sites", r.stdout)
    assert m, r.stdout[-2000:]
    print("wolff chi_m =", w, "+-", w_err, " mean cluster size =", m.group(1))
    assert float(m.group(1)) > 1.0
    h = _driver(*common, "--sampler", "heatbath")
    assert h.returncode == 0, h.stdout[-2000:] + h.stderr[-2000:]
    hb, hb_err = _avg_err(h.stdout)
    zcheck("host/driver chi_m 16x16 beta=1: --sampler wolff vs --sampler heatbath", w, w_err, hb, hb_err)
