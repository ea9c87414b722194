"""GPU: the Wolff single-cluster update of the O(3) sigma model on the levels of its CoarsenRotate hierarchy
(mlmcpi_sigma_level_cluster_draw, sigma_cluster.hip) against its numpy restatement (tests/sigma_level_cluster_model.py)
update by update, its invariances bit for bit (call split, batch split, every knob of the launch plan), the delegation of an
unrotated level, its law against the device's rotated heat bath and the CPU model, the hierarchical chain it is there for, and
host/driver --coarsesampler levelwolff."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sigma_level_cluster_model as slcm
import sigma_level_model as slm
from conftest import zcheck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [("wave", "lds"), ("wave", "global"), ("block", "lds"), ("block", "global")]
# Wolff updates per coarse draw of the hierarchical chain at 8 x 8, beta = 1: the smallest k of {10, 20, 40, 80} at which the
# numpy model chain lies within 3 of its own sigma of the model's heat-bath value (tools/exp_sigma_level_hier_model.py,
# profiles/sigma_level_hier_model.json, DESIGN.md 7.6: k = 10 reads +3.7 sigma, k = 20 +1.0 sigma, at an error of 0.55 % of chi_m)
K_HIER = 20


def _level(Mt, Mx, rot, beta):
    from mlmcpathintegral_amd import abi
    return abi.sigma_level(Mt, Mx, rot, beta)


def _thermalised(ops, lv, B, seed, draws=2, aligned=False):
    """device states with some order in them: a random (or all-aligned) start, then `draws` heat-bath draws of 10 + 1 sweeps"""
    x = ops.sigma_level_initialise(lv, B, seed)
    if aligned:
        x[:, 0::2] = 0.5 * math.pi
        x[:, 1::2] = 0.25
    w = torch.empty_like(x)
    for d in range(draws):
        ops.sigma_level_sweep_draw(lv, x, w, 10, 1, seed, 0, 11 * d)
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


# ---- parity, update by update ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [1.0, 1.5])
@pytest.mark.parametrize("Mt,Mx,B,n", [(2, 2, 5, 12), (2, 6, 5, 12), (4, 6, 5, 12), (16, 16, 4, 10), (66, 34, 3, 6), (130, 70, 3, 5)])
def test_every_update_equals_the_model(gpu_ops, Mt, Mx, B, n, beta):
    """each device update on a rotated level against the model applied to the device's own previous state: same flipped set,
    unit vectors to 1e-11, same count.  A bond whose uniform lies within 1e-10 of its probability could flip between two libms:
    the margin is asserted, never skipped.  The seeds (1000 + Mt + 10 beta) were run through the model on the CPU, from the
    model's own two 10 + 1 draws: every case clears the margin (smallest: 7.2e-5) and grows a cluster larger than 1."""
    ops = gpu_ops
    L = slm.Level(Mt, Mx, True, beta)
    lv = _level(Mt, Mx, 1, beta)
    seed, chain0, update0 = 1000 + Mt + int(10 * beta), 3, 40
    x = _thermalised(ops, lv, B, seed)
    work = ops.sigma_level_cluster_workspace(lv, B)
    largest = 0
    for k in range(n):
        before = x.cpu().numpy()
        sites = ops.sigma_level_cluster_draw(lv, x, 1, seed, chain0, update0 + k, work=work).cpu().numpy()
        after = x.cpu().numpy()
        for b in range(B):
            want, info = slcm.dev_update(L, before[b], seed, chain0 + b, update0 + k)
            print(f"rotated {Mt}x{Mx} beta={beta} update {k} chain {b}: cluster {len(info['sites'])}, margin {info['margin']:.3g}")
            assert info["margin"] > 1e-10, "a bond decision within 1e-10 of its uniform: change the seed"
            changed = np.nonzero(np.any(after[b].reshape(L.n, 2) != before[b].reshape(L.n, 2), axis=1))[0]
            assert np.array_equal(changed, info["sites"]), (k, b, len(changed), len(info["sites"]))
            assert sites[b] == len(info["sites"])
            d = np.abs(slm.unit_vectors(L, after[b][None]) - slm.unit_vectors(L, want[None])).max()
            assert d < 1e-11, (k, b, d)
            largest = max(largest, len(info["sites"]))
    assert largest > 1


# ---- invariances, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B,beta", [(2, 2, 8, 1.5), (16, 16, 8, 1.0), (130, 70, 8, 1.5), (512, 300, 8, 1.5), (1024, 1024, 4, 1.5)])
def test_call_split_batch_split_and_launch_plans_give_the_same_bits(gpu_ops, Mt, Mx, B, beta):
    """rotated levels; (512, 300) has n = 76 800, past the wave team's LDS bitmap and the 1024-thread threshold, (1024, 1024) has
    n = 524 288 and starts aligned so that the clusters take many frontier levels across the waves of a workgroup.  The share of
    the level the large case flips in its 40 updates is heavy-tailed: measured once over 13 seeds of this start it ran from 2.6 %
    to 7.3 % (mean 4.7 %), so that case takes a seed of its own (2000: 7.3 %) to be the input it is there to be."""
    ops = gpu_ops
    lv = _level(Mt, Mx, 1, beta)
    n = Mt * Mx // 2
    seed, chain0, update0 = 2000 if Mt == 1024 else 77 + Mt, 5, 1000
    x0 = _thermalised(ops, lv, B, seed, aligned=Mt == 1024)
    ref = x0.clone()
    count = ops.sigma_level_cluster_draw(lv, ref, 10, seed, chain0, update0)
    mean = count.double().mean().item() / 10
    print(f"rotated {Mt} x {Mx} beta = {beta}: {mean:.1f} flipped vertices per update ({mean / n:.3f} of the level)")
    assert mean > 1 and not torch.equal(ref, x0)
    if Mt == 1024:
        assert mean > 0.05 * n, "the large case is there for clusters that span a sizeable share of the level"

    a = x0.clone()
    c1 = ops.sigma_level_cluster_draw(lv, a, 5, seed, chain0, update0)
    c2 = ops.sigma_level_cluster_draw(lv, a, 5, seed, chain0, update0 + 5)
    assert torch.equal(a, ref) and torch.equal(c1 + c2, count)

    h = B // 2
    lo, hi = x0[:h].clone(), x0[h:].clone()
    cl = ops.sigma_level_cluster_draw(lv, lo, 10, seed, chain0, update0)
    ch = ops.sigma_level_cluster_draw(lv, hi, 10, seed, chain0 + h, update0)
    assert torch.equal(torch.cat([lo, hi]), ref) and torch.equal(torch.cat([cl, ch]), count)

    for team, bitmap in PLANS:
        with _plan(team, bitmap):
            y = x0.clone()
            c = ops.sigma_level_cluster_draw(lv, y, 10, seed, chain0, update0)
        assert torch.equal(y, ref) and torch.equal(c, count), (team, bitmap)


# ---- an unrotated level is mlmcpi_sigma_cluster_draw ----------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", [(16, 16), (130, 70)])
def test_unrotated_level_gives_the_bits_of_the_lattice_entry_point(gpu_ops, Mt, Mx):
    from mlmcpathintegral_amd import abi
    ops, B, beta = gpu_ops, 6, 1.5
    lv = _level(Mt, Mx, 0, beta)
    act = abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=beta)
    x0 = _thermalised(ops, lv, B, 50 + Mt)
    a, b = x0.clone(), x0.clone()
    assert ops.sigma_level_cluster_workspace(lv, B).numel() == ops.sigma_cluster_workspace(act, B).numel()
    ca = ops.sigma_level_cluster_draw(lv, a, 10, 9, 2, 30)
    cb = ops.sigma_cluster_draw(act, b, 10, 9, 2, 30)
    assert torch.equal(a, b) and torch.equal(ca, cb) and not torch.equal(a, x0)


# ---- statistics -----------------------------------------------------------------------------------------------------------
def _chain_means(samples, B):
    m = torch.stack(samples).mean(dim=0).cpu().numpy()
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(B))


@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_chi_m_agrees_with_the_rotated_heat_bath_and_with_the_cpu_model(gpu_ops, beta):
    ops = gpu_ops
    Mt = Mx = 16
    lv = _level(Mt, Mx, 1, beta)
    L = slm.Level(Mt, Mx, True, beta)
    B, burn, meas = 512, 100, 300

    def wolff(x, seed):
        work = ops.sigma_level_cluster_workspace(lv, B)
        chi = []
        for d in range(burn + meas):
            ops.sigma_level_cluster_draw(lv, x, 10, seed, 0, 10 * d, count=False, work=work)
            if d >= burn:
                chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
        return _chain_means(chi, B)

    w, w_err = wolff(ops.sigma_level_initialise(lv, B, 31), 32)
    aligned = torch.empty((B, 2 * L.n), dtype=torch.float64, device="cuda")
    aligned[:, 0::2] = 0.5 * math.pi
    aligned[:, 1::2] = 0.25
    wa, wa_err = wolff(aligned, 33)
    zcheck(f"sigma level Wolff chi_m rotated 16x16 beta={beta}: aligned start vs random start", wa, wa_err, w, w_err)

    x = ops.sigma_level_initialise(lv, B, 34)
    scratch = torch.empty_like(x)
    chi = []
    for d in range(burn + meas):
        ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 35, 0, 11 * d)
        if d >= burn:
            chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
    h, h_err = _chain_means(chi, B)
    zcheck(f"sigma level Wolff chi_m rotated 16x16 beta={beta}: device Wolff vs device heat bath", w, w_err, h, h_err)

    Bc = 48
    phi = slm.initialise(L, Bc, 36)
    chi = []
    for step in range(1500):
        phi, _ = slcm.dev_update_batch(L, phi, 37, 0, step)
        if step >= 500:
            chi.append(slm.magnetic_susceptibility(L, phi))
    c = np.mean(chi, axis=0)
    zcheck(f"sigma level Wolff chi_m rotated 16x16 beta={beta}: device Wolff vs CPU model chain", w, w_err, float(c.mean()),
           float(c.std(ddof=1) / math.sqrt(Bc)))


def test_hierarchical_chain_with_a_cluster_coarse_sampler_samples_the_fine_law(gpu_ops):
    """The reason for the feature.  8 x 8, beta = beta_coarse = 1, 4096 chains: the coarse proposals are the successive states of
    one rotated-level Wolff chain, ONE draw of K_HIER updates between proposals, then the two-level step, against the
    single-level 10 + 1 heat-bath draw of the same run (chi_m 8.735 +- 0.016); zcheck of the two device chains.
    Both levels start from 200 overrelaxation and 20 heat-bath sweeps of their own, so a valid step keeps the fine law from the
    first draw on.  With one 10 + 1 heat-bath draw between proposals this comparison reads z = +4.08 (chi_m 2.6 % high)."""
    ops = gpu_ops
    B, beta, n_meas = 4096, 1.0, 60
    lv = _level(8, 8, 0, beta)
    lc = _level(8, 8, 1, beta)
    single = ops.sigma_level_initialise(lv, B, 3, 0)
    fine = ops.sigma_level_initialise(lv, B, 4, 0)
    coarse = ops.sigma_level_initialise(lc, B, 5, 0)
    sf, sc = torch.empty_like(fine), torch.empty_like(coarse)
    ops.sigma_level_sweep_draw(lv, single, sf, 10 * 20, 20, 3, 0, 0)
    ops.sigma_level_sweep_draw(lv, fine, sf, 10 * 20, 20, 4, 0, 0)
    ops.sigma_level_sweep_draw(lc, coarse, sc, 10 * 20, 20, 5, 0, 0)
    work = ops.sigma_level_cluster_workspace(lc, B)
    step = ops.SigmaTwoLevelStep(lv, lc, B, seed=6)
    step.set_state(fine)
    tot_two = torch.zeros(B, dtype=torch.float64, device="cuda")
    tot_one = torch.zeros_like(tot_two)
    n_acc = torch.zeros(B, dtype=torch.float64, device="cuda")
    flipped = torch.zeros(B, dtype=torch.float64, device="cuda")
    for k in range(n_meas):
        flipped += ops.sigma_level_cluster_draw(lc, coarse, K_HIER, 5, 0, K_HIER * k, work=work)
        n_acc += step.draw(coarse)
        tot_two += ops.sigma_level_magnetic_susceptibility(lv, step.theta)
        ops.sigma_level_sweep_draw(lv, single, sf, 10, 1, 3, 0, 1000 + 11 * k)
        tot_one += ops.sigma_level_magnetic_susceptibility(lv, single)
    two, one = (tot_two / n_meas).cpu().numpy(), (tot_one / n_meas).cpu().numpy()
    rate = float(n_acc.sum()) / (B * n_meas)
    print(f"sigma hierarchical chain 8x8 beta=1, {K_HIER} Wolff updates per coarse draw: acceptance rate {rate:.4f}, "
          f"mean cluster {float(flipped.sum()) / (B * n_meas * K_HIER):.2f} of 32 vertices")
    assert 0.0 < rate < 1.0
    err = lambda v: v.std(ddof=1) / math.sqrt(B)
    zcheck(f"sigma hierarchical chain, {K_HIER} rotated Wolff updates per proposal, vs 10+1 heat bath, chi_m 8x8 beta=1", two.mean(),
           err(two), one.mean(), err(one))


# ---- driver ---------------------------------------------------------------------------------------------------------------
COMMON = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1"]
COARSE = ["--coarsening", "rotate", "--coarsesampler", "levelwolff", "--n_updates", str(K_HIER)]


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


def test_driver_hierarchical_with_levelwolff_agrees_with_the_heat_bath_sampler():
    h = _driver(*COMMON, *COARSE, "--sampler", "hierarchical", "--n_level", "2", "--n_samples", "6000", "--n_burnin", "200", "--n_meas", "20")
    assert h.returncode == 0, h.stdout[-2000:] + h.stderr[-2000:]
    s = _driver(*COMMON, "--sampler", "heatbath", "--n_samples", "4000", "--n_burnin", "100")
    assert s.returncode == 0, s.stdout[-2000:] + s.stderr[-2000:]
    (ha, he), (sa, se) = _avg_err(h.stdout), _avg_err(s.stdout)
    zcheck(f"host/driver chi_m 8x8 beta=1: hierarchical over levelwolff ({K_HIER} updates) vs --sampler heatbath", ha, he, sa, se)


def test_driver_levelwolff_on_three_levels_and_in_the_twolevel_method():
    # three levels: 8 x 8, rotated 8 x 8, 4 x 4 -- the Wolff sampler runs on the unrotated 4 x 4 level
    k = _driver(*COMMON, *COARSE, "--sampler", "hierarchical", "--n_level", "3", "--n_samples", "200", "--n_burnin", "20", "--n_meas", "10")
    assert k.returncode == 0, k.stdout[-2000:] + k.stderr[-2000:]
    assert "level 2" in k.stdout
    r = _driver(*COMMON, *COARSE, "--sampler", "heatbath", "--method", "twolevel", "--n_samples", "300", "--n_burnin", "50", "--n_meas", "20")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for what in ("QoI[fine]", "QoI[coarse]", "acceptance probability"):
        assert what in r.stdout, (what, r.stdout[-2000:])
    rate = float(re.findall(r"acceptance probability\s+p = ([0-9.]+)", r.stdout)[-1])
    print("two-level acceptance rate over levelwolff", rate)
    assert 0.0 < rate < 1.0
