"""The cluster samplers on the GPU (mlmcpathintegral_amd/csrc/cluster.hip) through the C ABI: parity with the numpy
restatement (tests/cluster_model.py), invariance under how the updates and the batch are split, the link rebuild against
long double, Monte Carlo statistics against exact values, and host/driver."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cluster_model as cm
import lattice_reference as lr
from conftest import zcheck

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "driver")
SEED = 0xC1057E5
M0 = 0.25


def _rotor(M, kappa2):
    """rotor with 2 m0 / a = kappa2 on M sites (m0 = 0.25)"""
    from mlmcpathintegral_amd import abi
    return abi.path_action(abi.ROTOR, M, M * 2.0 * M0 / kappa2, M0)


def _schwinger(Mt, Mx, beta):
    from mlmcpathintegral_amd import abi
    return abi.lattice_action(abi.SCHWINGER, Mt, Mx, beta=beta)


def _thermal(ops, act, B, sweeps=60, seed=SEED + 1):
    """paths with long runs: cumulated Gaussian steps of the equilibrium variance a / m0, then the library's own heat-bath
    sweeps (code older than this feature)"""
    kappa = act.m0 / (act.T_final / act.M)
    rng = np.random.default_rng(seed)
    start = cm.mod_2pi(np.cumsum(rng.normal(size=(B, act.M)) / math.sqrt(kappa), axis=1))   # steps of the equilibrium variance
    x = torch.from_numpy(start).cuda()
    ops.path_sweep_draw(act, x, torch.empty_like(x), 0, sweeps, seed, 0, 0)
    return x


def _ulp(v):
    return float(np.spacing(v))


def _chit_exact(kappa, M, T_final):
    from mlmcpathintegral_amd import abi
    v = C.c_double()
    abi.call("mlmcpi_schwinger_chit_analytical", kappa, M, C.byref(v))
    return v.value / T_final


# ---- 5. parity with the restatement -----------------------------------------------------------------------------------
# (M, B, 2 m0 / a, updates, chain0, update0, long): `long` cases must show a run of more than 128 sites (several windows)
PARITY = [(64, 300, 0.5, 10, 0, 0, False), (1000, 37, 8.0, 10, 5, 3, False), (4096, 5, 64.0, 10, 0, 100, False),
          (65536, 3, 400.0, 10, 2, 7, True), (4096, 16, 400.0, 10, 0, 0, True), (1000, 1, 0.5, 10, 9, 0, False),
          (8, 64, 6.0, 10, 0, 0, False)]


@pytest.mark.parametrize("M,B,kappa2,n_updates,chain0,update0,long_runs", PARITY)
def test_cluster_draw_matches_restatement(gpu_ops, M, B, kappa2, n_updates, chain0, update0, long_runs):
    act = _rotor(M, kappa2)
    if M >= 64:
        x = _thermal(gpu_ops, act, B)
    else:  # the small ring: equilibrated by the restatement itself
        start = cm.initial_path(B, M, SEED + 1)
        x = torch.from_numpy(cm.dev_draw(start, kappa2, SEED + 9, 0, 0, 30)[0]).cuda()
    x0 = x.cpu().numpy().copy()
    want, count, margin, longest = cm.dev_draw(x0, kappa2, SEED, chain0, update0, n_updates)
    print(f"M = {M}, B = {B}, 2 m0 / a = {kappa2}: longest run {longest}, mean {count.sum() / (B * n_updates):.1f}, margin {margin:.3g}")
    # a bond is u < p with p from libm on both sides: no decision of this case may be a tie
    assert margin > 1e-9, margin
    if long_runs:
        assert longest > 128, longest
    if M == 8:
        assert longest == 8, "the small ring is there for the runs that reach every site"
    sites = gpu_ops.path_cluster_draw(act, x, n_updates, SEED, chain0, update0).cpu().numpy()
    got = x.cpu().numpy()
    # tolerance: mod_2pi(pi + 2 xbar - x) is four roundings (sum, difference, the product inside mod_2pi, the final
    # difference) at magnitude <= 4 pi, half an ulp each, plus one ulp of xbar (fma on the device, two roundings in numpy)
    # doubled; a site flipped in every update carries it n_updates times
    tol = n_updates * (4 * 0.5 * _ulp(4 * np.pi) + 2 * _ulp(np.pi))
    d = got - want
    d -= 2 * np.pi * np.round(d / (2 * np.pi))
    assert np.array_equal(sites, count), (sites, count)
    moved_dev = np.abs((got - x0) - 2 * np.pi * np.round((got - x0) / (2 * np.pi))) > 1e-12
    moved_ref = np.abs((want - x0) - 2 * np.pi * np.round((want - x0) / (2 * np.pi))) > 1e-12
    assert np.array_equal(moved_dev, moved_ref), "flipped sets differ"
    assert np.max(np.abs(d)) <= tol, (np.max(np.abs(d)), tol)
    assert got.min() >= -np.pi and got.max() <= np.pi   # = [-pi, pi) in doubles, see test_links_match_long_double


def test_unsupported_kinds(gpu_ops):
    from mlmcpathintegral_amd import abi
    x = torch.zeros((2, 64), dtype=torch.float64, device="cuda")
    for kind in (abi.HARMONIC, abi.QUARTIC):
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            gpu_ops.path_cluster_draw(abi.path_action(kind, 64, 4.0), x, 1, 1, 0, 0)
    for kind in (abi.GFF, abi.NONLINEAR_SIGMA):
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            gpu_ops.schwinger_cluster_links(abi.lattice_action(kind, 8, 8, beta=1.0, mass=1.0), x, 0, 1, 0, 0)


# ---- 6. invariance ----------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_split(gpu_ops):
    M, B, kappa2 = 1000, 300, 24.0
    act = _rotor(M, kappa2)
    x0 = _thermal(gpu_ops, act, B)
    a = x0.clone()
    na = gpu_ops.path_cluster_draw(act, a, 10, SEED, 0, 40)
    b = x0.clone()
    nb = gpu_ops.path_cluster_draw(act, b, 5, SEED, 0, 40) + gpu_ops.path_cluster_draw(act, b, 5, SEED, 0, 45)
    assert torch.equal(a, b) and torch.equal(na, nb), "10 updates != 5 + 5"
    c = x0.clone()
    c1, c2 = c[:100].contiguous(), c[100:].contiguous()
    n1 = gpu_ops.path_cluster_draw(act, c1, 10, SEED, 0, 40)
    n2 = gpu_ops.path_cluster_draw(act, c2, 10, SEED, 100, 40)
    assert torch.equal(a, torch.cat([c1, c2])) and torch.equal(na, torch.cat([n1, n2])), "300 != 100 + 200 chains"
    # a chain among other neighbours: chain 17 alone, and placed last in a batch of 3 whose other chains differ
    d = x0[17:18].clone()
    gpu_ops.path_cluster_draw(act, d, 10, SEED, 17, 40)
    assert torch.equal(d[0], a[17])
    e = torch.stack([x0[200], x0[3], x0[19]])
    gpu_ops.path_cluster_draw(act, e, 10, SEED, 17, 40)
    assert torch.equal(e[2], a[19])


# ---- 8. the link rebuild ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B", [(16, 8, 3), (4, 4, 2), (6, 10, 2), (130, 70, 2), (64, 256, 2), (1024, 1024, 1)])
@pytest.mark.parametrize("gauge", [0, 1])
def test_links_match_long_double(gpu_ops, Mt, Mx, B, gauge):
    beta, draw, chain0 = 2.0, 11, 4
    N = Mt * Mx
    psi = cm.initial_path(B, N, SEED + 2, chain0)
    # a smooth closed path is what the sampler holds; a random one exercises the same sums with larger terms
    act = _schwinger(Mt, Mx, beta)
    theta = gpu_ops.schwinger_cluster_links(act, torch.from_numpy(psi).cuda(), gauge, SEED, chain0, draw).cpu().numpy()
    # [-pi, pi) in doubles: np.pi is the double below pi (pi - 1.2e-16) and the next double lies above pi, so a value is in
    # [-pi, pi) exactly when -np.pi <= value <= np.pi; mod_2pi may round to np.pi itself, never beyond
    assert theta.min() >= -np.pi and theta.max() <= np.pi
    # bound used: theta_1(i, j) is a sum of i differences of angles in [-pi, pi), partial sums bounded by 2 pi i, so i
    # additions cost at most i * ulp(2 pi Mt) / 2; the device adds them as a wave scan plus a carry (other order, same
    # bound); theta_0 of the last row sums Mt such terms twice (columns j and 0) and is reduced across lanes; the gauge
    # angles and mod_2pi add a handful of roundings at magnitude <= 2 pi Mt.
    tol = (2 * Mt + 16) * 0.5 * _ulp(2 * np.pi * Mt)
    worst_l = worst_p = 0.0
    for b in range(B):
        g = cm.gauge_angles(SEED, chain0 + b, draw, Mt, Mx) if gauge else None
        want = cm.schwinger_links(psi[b], Mt, Mx, g)
        d = lr.mod_2pi(theta[b].astype(lr.LD) - want)
        worst_l = max(worst_l, float(np.max(np.abs(d))))
        P = lr.schwinger_plaquettes(theta[b], Mt, Mx).reshape(Mx, Mt).T.reshape(N)     # cell c = i Mx + j
        dpsi = np.roll(psi[b].astype(lr.LD), -1) - psi[b].astype(lr.LD)
        worst_p = max(worst_p, float(np.max(np.abs(lr.mod_2pi(P - dpsi)))))
    print(f"{Mt} x {Mx} gauge {gauge}: links {worst_l:.3g}, plaquettes {worst_p:.3g}, tolerance {tol:.3g}")
    assert worst_l <= tol, (worst_l, tol)
    assert worst_p <= 4 * tol, (worst_p, tol)       # a plaquette is four links
    if gauge and N >= 1024:
        n = theta.size
        zcheck(f"cluster links {Mt}x{Mx} <cos theta>", float(np.cos(theta).mean()), math.sqrt(0.5 / n), 0.0)
        zcheck(f"cluster links {Mt}x{Mx} <sin theta>", float(np.sin(theta).mean()), math.sqrt(0.5 / n), 0.0)


def test_schwinger_draw_is_updates_then_links(gpu_ops):
    """mlmcpi_schwinger_cluster_draw = n_updates rotor updates of psi (2 m0 / a = 2 beta, counters draw n_updates + k),
    then the rebuild with the gauge of that draw"""
    Mt, Mx, B, beta = 32, 16, 5, 3.0
    act = _schwinger(Mt, Mx, beta)
    s = gpu_ops.SchwingerClusterSampler(act, B, n_updates=10, seed=SEED, chain0=2)
    np.testing.assert_allclose(s.psi.cpu().numpy(), cm.initial_path(B, Mt * Mx, SEED, 2), rtol=0, atol=1e-14)
    theta = torch.full((B, 2 * Mt * Mx), 7.0, dtype=torch.float64, device="cuda")
    for _ in range(3):
        before = s.psi.clone()
        s.draw(theta)
    rot = _rotor(Mt * Mx, 2.0 * beta)
    gpu_ops.path_cluster_draw(rot, before, 10, SEED, 2, 20)
    assert torch.equal(before, s.psi)
    assert torch.equal(theta, gpu_ops.schwinger_cluster_links(act, s.psi, 1, SEED, 2, 2))
    S = gpu_ops.lattice_evaluate(act, theta).cpu().numpy()
    want = np.array([float(cm.rotor_action(p, beta)) for p in s.psi.cpu().numpy()])
    np.testing.assert_allclose(S, want, rtol=1e-12, atol=1e-10)


# ---- 7. statistics ----------------------------------------------------------------------------------------------------
def _chain_mean(q):
    """q [draws, B]: mean and error from the spread of the per-chain means (chains are independent)"""
    m = q.mean(axis=0)
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(len(m)))


def test_rotor_chit_from_cluster_chains(gpu_ops):
    M, T = 256, 25.6
    from mlmcpathintegral_amd import abi
    act = abi.path_action(abi.ROTOR, M, T, M0)
    B = 1024
    x = gpu_ops.path_initialise(act, B, SEED + 3)
    upd = 0
    for _ in range(3 * M):  # from a random start; ten updates move about a hundred of the M sites
        gpu_ops.path_cluster_draw(act, x, 10, SEED, 0, upd, count=False)
        upd += 10
    q = []
    for _ in range(400):
        gpu_ops.path_cluster_draw(act, x, 10, SEED, 0, upd, count=False)
        upd += 10
        q.append(gpu_ops.qoi_susceptibility(x, T).cpu().numpy())
    mean, err = _chain_mean(np.array(q))
    zcheck("rotor cluster chi_t M=256 T=25.6 m0=0.25", mean, err, _chit_exact(M0 / (T / M), M, T))


def _tau_int(q):
    """integrated autocorrelation time of q [draws, B] in draws, chains pooled: tau = 1 + 2 sum_{k=1}^{W} rho(k) with the
    autocovariance averaged over chains and start times about the ensemble mean, W the first lag with W >= 5 tau(W)
    (Sokal's window), at most draws / 3.  Where the cap ends the sum the figure is a LOWER bound of tau."""
    n = q.shape[0]
    d = q - q.mean()
    c0 = float((d * d).mean())
    tau, capped = 1.0, True
    for k in range(1, n // 3 + 1):
        tau += 2.0 * float((d[:-k] * d[k:]).mean()) / c0
        if k >= 5.0 * tau:
            capped = False
            break
    return tau, capped


def test_rotor_chit_on_a_fine_lattice_where_the_heat_bath_freezes(gpu_ops):
    """(M, T, m0) = (256, 8, 0.25): a / m0 = 0.125, 2 m0 / a = 16.  A local update changes the winding only by taking one link
    difference through pi, against a Boltzmann factor of about exp(-2 m0 / a) = 1e-7: the heat-bath chain (10 overrelaxation
    + 1 heat-bath sweep per draw, the sampler's default) keeps its charge for thousands of draws, the cluster chain (10
    updates per draw) does not.  Both tau_int of Q^2 are measured and printed; the heat-bath figure is a lower bound when
    its window is cut (frozen chains).  Gated: the ratio, and the cluster chain's chi_t against the exact value."""
    from mlmcpathintegral_amd import abi
    M, T, B, n_draws = 256, 8.0, 512, 3000
    act = abi.path_action(abi.ROTOR, M, T, M0)
    x = gpu_ops.path_initialise(act, B, SEED + 6)
    upd = 0
    for _ in range(3 * M):
        gpu_ops.path_cluster_draw(act, x, 10, SEED, 0, upd, count=False)
        upd += 10
    y = x.clone()   # the heat-bath chains start from the cluster chains' equilibrium ensemble (every charge sector filled)
    qc = []
    for _ in range(n_draws):
        gpu_ops.path_cluster_draw(act, x, 10, SEED, 0, upd, count=False)
        upd += 10
        qc.append(gpu_ops.qoi_susceptibility(x, T).cpu().numpy())
    qc = np.array(qc)
    scratch, sweep, qh = torch.empty_like(y), 0, []
    for _ in range(n_draws):
        gpu_ops.path_sweep_draw(act, y, scratch, 10, 1, SEED + 7, 0, sweep)
        sweep += 11
        qh.append(gpu_ops.qoi_susceptibility(y, T).cpu().numpy())
    qh = np.array(qh)
    tau_c, cap_c = _tau_int(qc)
    tau_h, cap_h = _tau_int(qh)
    moved = float(np.mean(np.abs(qh[-1] - qh[0]) > 1e-9))
    print(f"tau_int of chi_t in draws: cluster {tau_c:.2f}{' (window cut)' if cap_c else ''}, heat bath {tau_h:.1f}"
          f"{' (window cut: lower bound)' if cap_h else ''}, ratio {tau_h / tau_c:.0f}; heat-bath chains whose Q^2 differs "
          f"between the first and the last of {n_draws} draws: {moved:.3f}")
    mean, err = _chain_mean(qc)
    hm, he = _chain_mean(qh)
    print(f"chi_t: cluster {mean:.5f} +- {err:.5f}, heat bath (frozen, same start) {hm:.5f} +- {he:.5f}")
    assert not cap_c, "the cluster chain's autocorrelation must be resolved"
    assert tau_h > 50 * tau_c, (tau_h, tau_c)
    zcheck("rotor cluster chi_t M=256 T=8 m0=0.25 (heat bath frozen)", mean, err, _chit_exact(M0 / (T / M), M, T))


@pytest.mark.parametrize("Mt,beta", [(16, 1.0), (16, 4.0), (32, 1.0), (32, 4.0)])
def test_schwinger_cluster_statistics(gpu_ops, Mt, beta):
    B, N = 512, Mt * Mt
    act = _schwinger(Mt, Mt, beta)
    s = gpu_ops.SchwingerClusterSampler(act, B, n_updates=10, seed=SEED + 4)
    theta = torch.empty((B, 2 * N), dtype=torch.float64, device="cuda")
    for _ in range(3 * N):  # from a random path; ten updates move a few dozen of the N plaquettes
        s.draw(theta)
    P, Q2 = [], []
    for _ in range(300):
        s.draw(theta)
        P.append(gpu_ops.qoi_avg_plaquette(theta, Mt, Mt).cpu().numpy())
        Q2.append(gpu_ops.qoi_2d_susceptibility(theta, Mt, Mt).cpu().numpy())
    mean, err = _chain_mean(np.array(P))
    zcheck(f"schwinger cluster <P> {Mt}^2 beta={beta:g}", mean, err, cm.ring_link_energy(beta, N))
    from mlmcpathintegral_amd import abi
    v = C.c_double()
    abi.call("mlmcpi_schwinger_chit_analytical", beta, N, C.byref(v))
    mean, err = _chain_mean(np.array(Q2))
    zcheck(f"schwinger cluster V chi_t {Mt}^2 beta={beta:g}", mean, err, v.value)
    # second reference: the heat-bath chain of the same shape
    y = gpu_ops.lattice_initialise(act, B, SEED + 5)
    scratch = torch.empty_like(y)
    sweep, H = 0, []
    for k in range(400):
        gpu_ops.lattice_sweep_draw(act, y, scratch, 2, 1, SEED + 5, 0, sweep)
        sweep += 3
        if k >= 100:
            H.append(gpu_ops.qoi_avg_plaquette(y, Mt, Mt).cpu().numpy())
    hm, he = _chain_mean(np.array(H))
    pm, pe = _chain_mean(np.array(P))
    zcheck(f"schwinger cluster <P> vs heat bath {Mt}^2 beta={beta:g}", pm, pe, hm, he)


# ---- 9. host/driver ---------------------------------------------------------------------------------------------------
def _driver(*args, timeout=600):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def test_driver_rotor_cluster_singlelevel():
    r = _driver("--action", "rotor", "--M_lat", "256", "--T_final", "25.6", "--m0", "0.25", "--sampler", "cluster",
                "--n_samples", "20000", "--n_burnin", "100")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-1500:])
    m = re.search(r"\|analytic - numerical\| / error = ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert float(m.group(1)) < 3
    assert "mean cluster size" in r.stdout


def test_driver_rotor_twolevel_and_throughput_with_cluster():
    r = _driver("--method", "twolevel", "--action", "rotor", "--M_lat", "64", "--T_final", "6.4", "--m0", "0.25",
                "--coarsesampler", "cluster", "--n_samples", "2000", "--n_burnin", "100")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Two level MC" in r.stdout
    print(r.stdout[-800:])
    for action, size in (("rotor", ["--M_lat", "4096", "--T_final", "409.6", "--m0", "0.25"]), ("schwinger", ["--Mt_lat", "64", "--beta", "2"])):
        t = _driver("--method", "throughput", "--action", action, *size, "--sampler", "cluster", "--batch", "32", "--n_samples", "50")
        assert t.returncode == 0, t.stdout[-2000:] + t.stderr[-2000:]
        line = json.loads([l for l in t.stdout.splitlines() if l.startswith("{")][-1])
        print(line)
        assert line["batch"] == 32 and line["units_per_draw"] > 0 and line["updates_per_s"] > 0
