"""The O(3) nonlinear sigma model on the GPU (mlmcpathintegral_amd/csrc/sigma2d.hip): parity with the numpy restatement
(tests/sigma_model.py), bit-for-bit invariances of the launch plan, the single-site heat-bath law, initialisation, Monte Carlo
statistics against exact answers and an independent CPU chain, and refusals of what the model does not support."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sigma_model as sm
from conftest import zcheck

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0003


def _act(ops, Mt, Mx, beta):
    from mlmcpathintegral_amd import abi
    return abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=beta)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(phi, Mt, Mx):
    return sm.unit_vectors(np.asarray(phi), Mt, Mx)


def _ks(sample, cdf):
    xs = np.sort(sample)
    n = len(xs)
    F = cdf(xs)
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)) * math.sqrt(n)


# ---- parity with the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (4, 6), (16, 16), (130, 70), (256, 300), (1024, 1024)])
def test_evaluate_force_qoi_match_restatement(gpu_ops, Mt, Mx):
    B, beta = 2, 0.9
    phi = sm.initialise(B, Mt, Mx, 3)
    act = _act(gpu_ops, Mt, Mx, beta)
    x = _dev(phi)
    assert gpu_ops.lattice_size(act) == 2 * Mt * Mx
    S = gpu_ops.lattice_evaluate(act, x).cpu().numpy()
    np.testing.assert_allclose(S, sm.evaluate(phi, Mt, Mx, beta), rtol=1e-12, atol=1e-12 * Mt * Mx)
    f = gpu_ops.lattice_force(act, x).cpu().numpy()
    np.testing.assert_allclose(f, sm.force(phi, Mt, Mx, beta), rtol=0, atol=1e-12)
    q = gpu_ops.qoi_magnetic_susceptibility(x, Mt, Mx).cpu().numpy()
    np.testing.assert_allclose(q, sm.magnetic_susceptibility(phi, Mt, Mx), rtol=1e-12, atol=1e-12)


def test_initialise_matches_restatement_and_is_uniform_on_the_sphere(gpu_ops):
    B, Mt, Mx = 4, 64, 64
    act = _act(gpu_ops, Mt, Mx, 1.0)
    x = gpu_ops.lattice_initialise(act, B, SEED, chain0=7).cpu().numpy()
    want = sm.initialise(B, Mt, Mx, SEED, chain0=7)
    np.testing.assert_allclose(x, want, rtol=0, atol=1e-14)
    s = _unit(x, Mt, Mx).reshape(-1, 3)
    n = s.shape[0]
    zcheck("sigma init <z>", s[:, 2].mean(), math.sqrt(1 / 3 / n), 0.0)
    zcheck("sigma init <z^2>", (s[:, 2] ** 2).mean(), math.sqrt((1 / 5 - 1 / 9) / n), 1 / 3)
    assert _ks(x[:, 1::2].ravel(), lambda t: (t + np.pi) / (2 * np.pi)) < 1.95


SWEEP_CASES = [(2, 2, 32), (4, 6, 32), (16, 16, 5), (16, 16, 1), (130, 70, 5), (256, 300, 1)]


@pytest.mark.parametrize("n_or,n_hb", [(0, 1), (1, 0), (3, 1), (10, 1), (2, 2)])
@pytest.mark.parametrize("Mt,Mx,B", SWEEP_CASES)
def test_sweeps_match_restatement_at_every_fuse_depth(gpu_ops, Mt, Mx, B, n_or, n_hb):
    """Every sweep of the draw, run alone on the device, against the restatement applied to the device's own previous state
    (unit vectors at 1e-11); the whole draw at every fuse depth bit for bit against that chain of single sweeps; and for
    draws of up to four sweeps the whole draw against the restatement's whole draw.  Longer draws are not compared whole:
    overrelaxation sweeps amplify rounding (a 1e-16 perturbation of the input grows to ~3e-9 over 10 sweeps of the
    restatement itself on 16 x 16), so two correct implementations with different libm drift apart beyond 1e-11."""
    beta = 1.1
    phi = sm.initialise(B, Mt, Mx, 17, chain0=3)
    act = _act(gpu_ops, Mt, Mx, beta)
    x = _dev(phi)
    for s in range(n_or + n_hb):
        heat = s >= n_or
        prev = x.cpu().numpy()
        gpu_ops.lattice_sweep_draw(act, x, torch.empty_like(x), int(not heat), int(heat), SEED, 3, 40 + s, fuse=1)
        want = _unit(sm.sweep_draw(prev, Mt, Mx, beta, int(not heat), int(heat), seed=SEED, chain0=3, sweep0=40 + s), Mt, Mx)
        err = np.abs(_unit(x.cpu().numpy(), Mt, Mx) - want).max()
        assert err < 1e-11, f"sweep {s}: unit vectors differ by {err:.3g}"
    chained = x
    if n_or + n_hb <= 4:
        want = _unit(sm.sweep_draw(phi, Mt, Mx, beta, n_or, n_hb, seed=SEED, chain0=3, sweep0=40), Mt, Mx)
        err = np.abs(_unit(chained.cpu().numpy(), Mt, Mx) - want).max()
        assert err < 1e-11, f"whole draw: unit vectors differ by {err:.3g}"
    for fuse in (0, 1, 2, 3, 4, 6):
        x = _dev(phi)
        gpu_ops.lattice_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, 3, 40, fuse=fuse)
        assert torch.equal(x, chained), f"fuse {fuse} is not bit-identical to the draw sweep by sweep"


# ---- bit-for-bit invariances of the launch plan -----------------------------------------------------------------------
def _draw(ops, act, phi, n_or, n_hb, chain0=0, fuse=0):
    x = phi.clone()
    ops.lattice_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, chain0, 11, fuse=fuse)
    return x


@pytest.mark.parametrize("Mt,Mx", [(70, 48), (64, 64)])
def test_launch_plan_invariances(gpu_ops, Mt, Mx):
    from mlmcpathintegral_amd import abi
    B, beta, n_or, n_hb = 6, 1.3, 5, 2
    act = _act(gpu_ops, Mt, Mx, beta)
    phi = gpu_ops.lattice_initialise(act, B, SEED)
    ref = _draw(gpu_ops, act, phi, n_or, n_hb)
    for fuse in range(1, 8):
        assert torch.equal(_draw(gpu_ops, act, phi, n_or, n_hb, fuse=fuse), ref), f"fuse {fuse}"
    try:
        for tile in ("16x16x256", "64x64x512", "32x64x1024", "8x4x256"):
            abi.set_option("MLMCPI_SWEEP_TILE", tile)
            assert torch.equal(_draw(gpu_ops, act, phi, n_or, n_hb), ref), f"MLMCPI_SWEEP_TILE={tile}"
    finally:
        abi.set_option("MLMCPI_SWEEP_TILE", "")
    # batch split by chain0
    lo = _draw(gpu_ops, act, phi[:2].contiguous(), n_or, n_hb, chain0=0)
    hi = _draw(gpu_ops, act, phi[2:].contiguous(), n_or, n_hb, chain0=2)
    assert torch.equal(torch.cat([lo, hi]), ref)
    # ping-pong and _from forms
    a, b = phi.clone(), torch.empty_like(phi)
    res, _ = gpu_ops.lattice_sweep_draw_pingpong(act, a, b, n_or, n_hb, SEED, 0, 11)
    assert torch.equal(res, ref)
    src = phi.clone()
    w0, w1 = torch.empty_like(phi), torch.empty_like(phi)
    where = C.c_int32(-5)
    abi.call("mlmcpi_lattice_sweep_draw_from", C.byref(act), gpu_ops._p(src), gpu_ops._p(w0), gpu_ops._p(w1), B, n_or, n_hb,
             SEED, 0, 11, 0, C.byref(where), gpu_ops._stream())
    assert torch.equal((w0, w1)[where.value], ref) and torch.equal(src, phi)
    # fused QoI and record = separate QoI + stats_accumulate (to rounding)
    res, _, q = gpu_ops.lattice_sweep_draw_qoi(act, phi.clone(), torch.empty_like(phi), torch.empty_like(phi), n_or, n_hb, SEED, 0,
                                               11, 4)
    assert torch.equal(res, ref)
    qs = gpu_ops.qoi_magnetic_susceptibility(ref, Mt, Mx)
    torch.testing.assert_close(q, qs, rtol=1e-13, atol=1e-13)
    acc = torch.zeros((B, 5), dtype=torch.float64, device="cuda")
    acc2 = torch.zeros_like(acc)
    for _ in range(2):
        res, _, q = gpu_ops.lattice_sweep_draw_qoi(act, phi.clone(), torch.empty_like(phi), torch.empty_like(phi), n_or, n_hb, SEED,
                                                   0, 11, 4, acc=acc)
        gpu_ops.stats_accumulate(acc2, gpu_ops.qoi_magnetic_susceptibility(res, Mt, Mx))
    assert torch.equal(res, ref)
    torch.testing.assert_close(acc, acc2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("heat", [0, 1])
def test_site_updates_over_the_two_colours_are_one_sweep(gpu_ops, heat):
    Mt, Mx, B, beta = 12, 10, 5, 0.8
    act = _act(gpu_ops, Mt, Mx, beta)
    phi = gpu_ops.lattice_initialise(act, B, SEED)
    ref = phi.clone()
    gpu_ops.lattice_sweep_draw(act, ref, torch.empty_like(ref), 1 - heat, heat, SEED, 0, 9)
    even = [j * Mt + i for j in range(Mx) for i in range(Mt) if (i + j) % 2 == 0]
    odd = [j * Mt + i for j in range(Mx) for i in range(Mt) if (i + j) % 2 == 1]
    rng = np.random.default_rng(0)
    x = phi.clone()
    for cls in (even, odd):  # any order inside a colour class
        sites = torch.tensor(rng.permutation(cls), dtype=torch.int32, device="cuda")
        gpu_ops.lattice_site_updates(act, x, sites, heat, SEED, 0, 9)
    assert torch.equal(x, ref)


# ---- the single-site heat-bath law -----------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.05, 0.5, 2.0, 8.0])
def test_single_site_heatbath_law(gpu_ops, beta):
    Mt = Mx = 4
    B = 1 << 16
    l = 1 * Mt + 2  # vertex (2, 1)
    a = np.empty((Mx, Mt, 2))
    rng = np.random.default_rng(5)
    a[..., 0] = np.arccos(rng.uniform(-1, 1, (Mx, Mt)))
    a[..., 1] = rng.uniform(-np.pi, np.pi, (Mx, Mt))
    phi = np.broadcast_to(a.reshape(1, -1), (B, 2 * Mt * Mx)).copy()
    act = _act(gpu_ops, Mt, Mx, beta)
    x = _dev(phi)
    gpu_ops.lattice_site_updates(act, x, l, 1, SEED, 0, 123)
    got = x.cpu().numpy()
    others = np.ones(2 * Mt * Mx, dtype=bool)
    others[2 * l:2 * l + 2] = False
    assert np.array_equal(got[:, others], phi[:, others])
    sig = sm.sigma_of(got[:, 2 * l:2 * l + 2])
    D = sm.delta(sm.sigma_of(a)[None])[0, 1, 2]
    nrm = np.linalg.norm(D)
    d = D / nrm
    s = beta * nrm
    x_par = sig @ d
    ks = _ks(x_par, lambda t: sm.compact_exp_cdf(s, t))
    assert ks < 1.95, f"KS of sigma . D^ at s = {s:.3g}: sqrt(n) D = {ks:.3f}"
    # azimuth about D^ uniform
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    az = np.arctan2(sig @ e2, sig @ e1)
    assert _ks(az, lambda t: (t + np.pi) / (2 * np.pi)) < 1.95
    if beta == 0.0:
        assert _ks(sig[:, 2], lambda t: (t + 1) / 2) < 1.95
        assert _ks(np.arctan2(sig[:, 1], sig[:, 0]), lambda t: (t + np.pi) / (2 * np.pi)) < 1.95


# ---- statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_ring_statistics_against_exact_answers(gpu_ops, beta):
    Mt, B, n_draw, burn = 2, 4096, 120, 10
    act = _act(gpu_ops, Mt, Mt, beta)
    x = gpu_ops.lattice_initialise(act, B, SEED)
    S, chi = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda")
    for d in range(n_draw):
        gpu_ops.lattice_sweep_draw(act, x, torch.empty_like(x), 3, 1, SEED, 0, 4 * d)
        if d >= burn:
            S += gpu_ops.lattice_evaluate(act, x)
            chi += gpu_ops.qoi_magnetic_susceptibility(x, Mt, Mt)
    S, chi = (S / (n_draw - burn)).cpu().numpy(), (chi / (n_draw - burn)).cpu().numpy()
    eS, echi = sm.ring_exact(beta)
    zcheck(f"sigma GPU 2x2 beta={beta} <S>", S.mean(), S.std(ddof=1) / math.sqrt(B), eS)
    zcheck(f"sigma GPU 2x2 beta={beta} <chi_m>", chi.mean(), chi.std(ddof=1) / math.sqrt(B), echi)


def test_free_spins_have_unit_susceptibility(gpu_ops):
    Mt, B = 64, 512
    act = _act(gpu_ops, Mt, Mt, 0.0)
    x = gpu_ops.lattice_initialise(act, B, SEED)
    src, w0, w1 = x, torch.empty_like(x), torch.empty_like(x)
    q_all = []
    for d in range(4):
        res, other, q = gpu_ops.lattice_sweep_draw_qoi(act, src, w0, w1, 2, 1, SEED, 0, 3 * d, 4)
        q_all.append(q.cpu().numpy())
        src, w0, w1 = res, other, src
    q = np.concatenate(q_all)  # at beta = 0 every heat-bath sweep draws fresh independent spins
    zcheck("sigma GPU 64^2 beta=0 <chi_m>", q.mean(), q.std(ddof=1) / math.sqrt(len(q)), 1.0)


def _batch_err(series, nb=20):
    m = len(series) // nb
    means = np.array([series[k * m:(k + 1) * m].mean() for k in range(nb)])
    return means.std(ddof=1) / math.sqrt(nb)


def test_device_chain_agrees_with_an_independent_cpu_chain(gpu_ops):
    Mt, beta, B, n_draw, burn = 8, 1.0, 256, 200, 20
    act = _act(gpu_ops, Mt, Mt, beta)
    x = gpu_ops.lattice_initialise(act, B, SEED)
    S, chi = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda")
    for d in range(n_draw):
        gpu_ops.lattice_sweep_draw(act, x, torch.empty_like(x), 3, 1, SEED, 0, 4 * d)
        if d >= burn:
            S += gpu_ops.lattice_evaluate(act, x)
            chi += gpu_ops.qoi_magnetic_susceptibility(x, Mt, Mt)
    S = (S / (n_draw - burn)).cpu().numpy() / (Mt * Mt)
    chi = (chi / (n_draw - burn)).cpu().numpy()
    cpu = np.array(list(sm.metropolis_chain(Mt, Mt, beta, 6000, np.random.default_rng(11))))[500:]
    zcheck("sigma 8x8 beta=1 <S>/N GPU vs CPU Metropolis", S.mean(), S.std(ddof=1) / math.sqrt(B), cpu[:, 0].mean(),
           _batch_err(cpu[:, 0]))
    zcheck("sigma 8x8 beta=1 <chi_m> GPU vs CPU Metropolis", chi.mean(), chi.std(ddof=1) / math.sqrt(B), cpu[:, 1].mean(),
           _batch_err(cpu[:, 1]))


# ---- errors, never faults ---------------------------------------------------------------------------------------------
def test_unsupported_operations_are_refused(gpu_ops):
    from mlmcpathintegral_amd import abi
    Mt = 8
    act = _act(gpu_ops, Mt, Mt, 1.0)
    x = gpu_ops.lattice_initialise(act, 2, SEED)
    with pytest.raises(abi.MlmcpiError, match="status -3.*HMC"):
        gpu_ops.LatticeHMC(act, 2, 5, 0.1)
    nb = C.c_size_t(0)
    with pytest.raises(abi.MlmcpiError, match="status -3"):
        abi.call("mlmcpi_lattice_hmc_draw", C.byref(act), gpu_ops._p(x), 2, 5, 0.1, 1, SEED, 0, 0, gpu_ops._p(x), gpu_ops._p(x),
                 None, gpu_ops._stream())
    coarse = _act(gpu_ops, Mt // 2, Mt // 2, 1.0)
    with pytest.raises(abi.MlmcpiError, match="status -3.*two-level"):
        abi.call("mlmcpi_lattice_twolevel_workspace_bytes", C.byref(act), C.byref(coarse), 2, C.byref(nb))
    y = torch.empty((2, 2 * (Mt // 2) ** 2), dtype=torch.float64, device="cuda")
    with pytest.raises(abi.MlmcpiError, match="status -3"):
        gpu_ops.lattice_copy_from_fine(act, 2, 2, x)
    with pytest.raises(abi.MlmcpiError, match="status -3"):
        abi.call("mlmcpi_lattice_copy_from_coarse", C.byref(act), 2, 2, gpu_ops._p(y), gpu_ops._p(x), 2, gpu_ops._stream())
    with pytest.raises(abi.MlmcpiError, match="status -3"):
        abi.call("mlmcpi_lattice_exact_workspace_bytes", C.byref(act), 2, C.byref(nb))
    # odd extents
    odd = _act(gpu_ops, 5, 4, 1.0)
    z = gpu_ops.lattice_initialise(odd, 2, SEED)
    with pytest.raises(abi.MlmcpiError, match="even"):
        gpu_ops.lattice_sweep_draw(odd, z, torch.empty_like(z), 1, 1, SEED, 0, 0)
    # QoI kinds of other actions on the sigma model, and 4 on other actions
    for k in (1, 2, 3):
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            gpu_ops.lattice_sweep_draw_qoi(act, x, torch.empty_like(x), torch.empty_like(x), 1, 1, SEED, 0, 0, k)
    for kind in (abi.SCHWINGER, abi.GFF):
        other = abi.lattice_action(kind, Mt, Mt, beta=1.0, mass=1.0)
        w = gpu_ops.lattice_initialise(other, 2, SEED)
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            gpu_ops.lattice_sweep_draw_qoi(other, w, torch.empty_like(w), torch.empty_like(w), 1, 1, SEED, 0, 0, 4)
    torch.cuda.synchronize()
