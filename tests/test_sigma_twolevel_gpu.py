"""GPU: the O(3) sigma model on the levels of its CoarsenRotate hierarchy (mlmcpi_sigma_level_*), its conditioned fine action
(mlmcpi_sigma_cfa_*) and the two-level Metropolis step (mlmcpi_sigma_twolevel_*) against the numpy model
(tests/sigma_level_model.py).  Tolerances are those of test_sigma_gpu.py: 1e-12 relative for sums, 1e-11 on unit vectors (the
angles themselves are ill-conditioned at the poles); sums of n terms that cancel are held to 1e-12 n."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sigma_level_model as lm
from conftest import zcheck

pytestmark = pytest.mark.gpu

SHAPES = [(2, 6), (4, 4), (6, 4), (66, 34), (130, 66)]   # wrap onto the same neighbour, transposition, odd planes, > one 64 x 32 tile
BETA = 1.3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _level(abi, L):
    return abi.sigma_level(L.Mt, L.Mx, L.rotated, L.beta)


def _close_sum(got, want, n=None):
    got, want = np.asarray(got), np.asarray(want)
    tol = 1e-12 * np.maximum(np.abs(want), 1.0) if n is None else 1e-12 * n
    assert np.all(np.abs(got - want) <= tol), float(np.max(np.abs(got - want) / tol))


def _close_spins(L, got, want):
    d = np.max(np.abs(lm.unit_vectors(L, got) - lm.unit_vectors(L, want)))
    assert d < 1e-11, d


@pytest.fixture(autouse=True)
def _reset_options():
    from mlmcpathintegral_amd import abi
    yield
    abi.set_option("MLMCPI_SIGMA_LEVEL_PLAN", "")
    abi.set_option("MLMCPI_SIGMA_TWOLEVEL_GROUPS", "")


@pytest.mark.parametrize("B", [3, 300])
@pytest.mark.parametrize("Mt,Mx", SHAPES)
def test_rotated_level_against_model(gpu_ops, Mt, Mx, B):
    """initialise, evaluate, QoI, the sweeps sweep by sweep (each from the device's previous state), both copies, the fill and the
    conditioned fine action on a ROTATED level"""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    L = lm.Level(Mt, Mx, True, BETA)
    lv = _level(abi, L)
    assert ops.sigma_level_size(lv) == 2 * L.n
    seed, chain0 = 31, 5
    x = ops.sigma_level_initialise(lv, B, seed, chain0)
    x0 = x.cpu().numpy()
    assert np.max(np.abs(x0 - lm.initialise(L, B, seed, chain0))) < 1e-13
    _close_sum(ops.sigma_level_evaluate(lv, x).cpu().numpy(), lm.evaluate(L, x0))
    _close_sum(ops.sigma_level_magnetic_susceptibility(lv, x).cpu().numpy(), lm.magnetic_susceptibility(L, x0))
    scratch = torch.empty_like(x)
    cur = x0
    for s, (n_or, n_hb) in enumerate([(1, 0), (0, 1), (1, 0), (0, 1)]):
        ops.sigma_level_sweep_draw(lv, x, scratch, n_or, n_hb, seed, chain0, 7 + s)
        got = x.cpu().numpy()
        _close_spins(L, got, lm.sweep_draw(L, cur, n_or, n_hb, seed, chain0, 7 + s))
        cur = got
    # the fill and its density (the O plane from the E plane)
    _close_sum(ops.sigma_cfa_evaluate(lv, x).cpu().numpy(), lm.cfa_evaluate(L, cur), n=L.n)
    ops.sigma_cfa_fill(lv, x, seed + 1, chain0, 3)
    got = x.cpu().numpy()
    want = lm.cfa_fill(L, cur, seed + 1, chain0, 3)
    _close_spins(L, got, want)
    coarse_entries = np.repeat(2 * L.fine2coarse[:, 0], 2) + np.tile([0, 1], len(L.fine2coarse))
    assert np.array_equal(got[:, coarse_entries], cur[:, coarse_entries])    # the fill touches fine-only vertices only
    # copies: the E plane <-> the coarse lattice, index for index
    c = ops.sigma_level_copy_from_fine(lv, x).cpu().numpy()
    assert np.array_equal(c, lm.copy_from_fine(L, got))
    cc = np.ascontiguousarray(c[:, ::-1])   # some other coarse state
    back = ops.sigma_level_copy_from_coarse(lv, _dev(cc), x).cpu().numpy()
    assert np.array_equal(back, lm.copy_from_coarse(L, cc, got))


@pytest.mark.parametrize("B", [3, 300])
@pytest.mark.parametrize("Mt,Mx", SHAPES)
def test_unrotated_level_against_model(gpu_ops, Mt, Mx, B):
    """the unrotated level through the level ABI: what it delegates (evaluate, QoI, sweeps) and what is new on it (the copies to
    and from the rotated partner, the fill and the conditioned fine action over the (i + j) odd vertices)"""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    L = lm.Level(Mt, Mx, False, BETA)
    lv = _level(abi, L)
    seed, chain0 = 32, 2
    x = ops.sigma_level_initialise(lv, B, seed, chain0)
    x0 = x.cpu().numpy()
    assert np.max(np.abs(x0 - lm.initialise(L, B, seed, chain0))) < 1e-13
    _close_sum(ops.sigma_level_evaluate(lv, x).cpu().numpy(), lm.evaluate(L, x0))
    _close_sum(ops.sigma_level_magnetic_susceptibility(lv, x).cpu().numpy(), lm.magnetic_susceptibility(L, x0))
    scratch = torch.empty_like(x)
    cur = x0
    for s, (n_or, n_hb) in enumerate([(1, 0), (0, 1)]):
        ops.sigma_level_sweep_draw(lv, x, scratch, n_or, n_hb, seed, chain0, 7 + s)
        got = x.cpu().numpy()
        _close_spins(L, got, lm.sweep_draw(L, cur, n_or, n_hb, seed, chain0, 7 + s))
        cur = got
    _close_sum(ops.sigma_cfa_evaluate(lv, x).cpu().numpy(), lm.cfa_evaluate(L, cur), n=L.n)
    ops.sigma_cfa_fill(lv, x, seed + 1, chain0, 3)
    got = x.cpu().numpy()
    _close_spins(L, got, lm.cfa_fill(L, cur, seed + 1, chain0, 3))
    coarse_entries = np.repeat(2 * L.fine2coarse[:, 0], 2) + np.tile([0, 1], len(L.fine2coarse))
    assert np.array_equal(got[:, coarse_entries], cur[:, coarse_entries])
    c = ops.sigma_level_copy_from_fine(lv, x).cpu().numpy()
    assert np.array_equal(c, lm.copy_from_fine(L, got))
    cc = np.ascontiguousarray(c[:, ::-1])
    back = ops.sigma_level_copy_from_coarse(lv, _dev(cc), x).cpu().numpy()
    assert np.array_equal(back, lm.copy_from_coarse(L, cc, got))


PLANS = ["", "8x8x256x1", "64x32x1024x3", "17x5x512x4", "33x17x256x2", "64x32x512x2", "3x2x256x5"]


@pytest.mark.parametrize("Mt,Mx", [(66, 34), (4, 4), (130, 66)])
def test_rotated_sweeps_bit_identical_across_plans(gpu_ops, Mt, Mx):
    """a 3 + 2 draw under every tile / workgroup / fuse setting, and split into two batches with chain0"""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    lv = abi.sigma_level(Mt, Mx, 1, BETA)
    B, seed = 5, 77
    x0 = ops.sigma_level_initialise(lv, B, seed, 0)
    results = []
    for plan in PLANS:
        abi.set_option("MLMCPI_SIGMA_LEVEL_PLAN", plan)
        x = x0.clone()
        ops.sigma_level_sweep_draw(lv, x, torch.empty_like(x), 3, 2, seed, 0, 11)
        results.append(x)
    for plan, r in zip(PLANS[1:], results[1:]):
        assert torch.equal(r, results[0]), plan
    assert not torch.equal(results[0], x0)
    abi.set_option("MLMCPI_SIGMA_LEVEL_PLAN", "")
    # 3 + 2 in one call = 3 + 0 and 0 + 2 in two; a batch split with chain0
    x = x0.clone()
    ops.sigma_level_sweep_draw(lv, x, torch.empty_like(x), 3, 0, seed, 0, 11)
    ops.sigma_level_sweep_draw(lv, x, torch.empty_like(x), 0, 2, seed, 0, 14)
    assert torch.equal(x, results[0])
    a, b = x0[:2].clone(), x0[2:].clone()
    ops.sigma_level_sweep_draw(lv, a, torch.empty_like(a), 3, 2, seed, 0, 11)
    ops.sigma_level_sweep_draw(lv, b, torch.empty_like(b), 3, 2, seed, 2, 11)
    assert torch.equal(torch.cat([a, b]), results[0])


def _twolevel_inputs(ops, abi, L, Lc, B, seed):
    """a current fine state and a coarse proposal, both after a few sweeps so that the three terms are of ordinary size"""
    lv, lc = _level(abi, L), _level(abi, Lc)
    theta = ops.sigma_level_initialise(lv, B, seed, 0)
    ops.sigma_level_sweep_draw(lv, theta, torch.empty_like(theta), 0, 3, seed, 0, 0)
    phi_c = ops.sigma_level_initialise(lc, B, seed + 1, 0)
    ops.sigma_level_sweep_draw(lc, phi_c, torch.empty_like(phi_c), 0, 3, seed + 1, 0, 0)
    # an independent proposal is never accepted on the larger lattices: every other chain proposes the restriction of its own
    # state instead, for which dS = F(theta_C) - F(theta_C) + 0 is rounding and the step accepts -- both branches on every shape
    phi_c[::2] = ops.sigma_level_copy_from_fine(lv, theta)[::2]
    return lv, lc, theta, phi_c


# fine level (Mt, Mx, rotated): both parities; 66 x 34 and 132 x 68 have more than one group of 256 fine-only vertices, none a
# multiple of 256; 4 x 4 and 8 x 4 wrap onto the same neighbour
TWOLEVEL = [(4, 4, 0, 300), (6, 4, 0, 3), (66, 34, 0, 300), (8, 4, 1, 300), (8, 12, 1, 3), (132, 68, 1, 300)]


@pytest.mark.parametrize("Mt,Mx,rot,B", TWOLEVEL)
def test_twolevel_draw_against_model(gpu_ops, Mt, Mx, rot, B):
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    L = lm.Level(Mt, Mx, rot, BETA)
    Lc = L.coarse(beta=0.9)        # beta_coarse != beta
    seed, step_no = 41, 6
    lv, lc, theta, phi_c = _twolevel_inputs(ops, abi, L, Lc, B, seed)
    theta0, phi_c0 = theta.cpu().numpy(), phi_c.cpu().numpy()
    want_new, want_acc, want_terms, want_trial, margin = lm.twolevel_draw(L, Lc, phi_c0, theta0, seed + 2, 0, step_no)
    decided = margin > 1e-9
    print(f"{Mt} x {Mx} rot {rot}: model acceptance {want_acc.mean():.3f}, undecided chains {(~decided).sum()} of {B}")
    assert (~decided).mean() <= 0.01   # the seed keeps the model alone within the share that may be left out

    def run(groups, lo=0, hi=B):
        abi.set_option("MLMCPI_SIGMA_TWOLEVEL_GROUPS", groups)
        st = ops.SigmaTwoLevelStep(lv, lc, hi - lo, seed=seed + 2, chain0=lo)
        st.set_state(theta[lo:hi])
        st.step = step_no
        st.draw(phi_c[lo:hi].contiguous())
        return st.theta.clone(), st.accept.clone(), st.terms.clone(), st.trial().clone()

    new, acc, terms, trial = run("")
    new_h, acc_h, terms_h, trial_h = (t.cpu().numpy() for t in (new, acc, terms, trial))
    _close_sum(terms_h, want_terms, n=L.n)
    assert np.array_equal(acc_h[decided] != 0, want_acc[decided])
    # the trial: the proposal on the coarse vertices bit for bit, the fill on the others
    assert np.array_equal(lm.copy_from_fine(L, trial_h), phi_c0)
    _close_spins(L, trial_h, want_trial)
    # accepted chains equal the trial, rejected chains are untouched, bit for bit
    a = acc_h != 0
    assert 0 < a.sum() < B or B < 10
    assert np.array_equal(new_h[a], trial_h[a]) and np.array_equal(new_h[~a], theta0[~a])
    # the decimation identity on the device's own output
    _close_sum(terms_h[:, 0] + terms_h[:, 2], lm.decimation_F(L, theta0) - lm.decimation_F(L, trial_h), n=L.n)
    # nothing depends on the launch plan or on the batch split
    for groups in ("3", "64"):
        for got, ref in zip(run(groups), (new, acc, terms, trial)):
            assert torch.equal(got, ref), groups
    if B >= 3:
        lo_part, hi_part = run("2", 0, 2), run("", 2, B)
        for p, q, ref in zip(lo_part, hi_part, (new, acc, terms, trial)):
            assert torch.equal(torch.cat([p, q]), ref)


def _edge_state(L, case):
    """[1, 2 n] states that put the conditioned fine action on its branches.  'zero': every fine-only vertex sees two spins
    (0, 0, 1), one sigma(pi, 0) and one sigma(-pi, 0), whose sum is exactly 0 in every order (sin(-pi) = -sin(pi), cos(+-pi) = -1);
    'aligned': all spins equal, so |Delta| = 4 and s = 4 beta."""
    a = np.zeros((L.n, 2))
    if case == "aligned":
        a[:, 0], a[:, 1] = 0.3, 0.5
    else:
        a[L.fineonly, 0], a[L.fineonly, 1] = 1.1, -0.7
        for l, _ in L.fine2coarse:
            i, j = L.coords[l]
            u, v = ((i // 2) % 2, (j // 2) % 2) if L.rotated else (((i + j) // 2) % 2, ((i - j) // 2) % 2)
            a[l, 0] = 0.0 if u == v else (math.pi if u == 0 else -math.pi)
    return a.reshape(1, 2 * L.n)


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("case,beta", [("zero", 1.3), ("aligned", 10.0), ("aligned", 2.5e-9)])
def test_cfa_branches_on_the_device(gpu_ops, rot, case, beta):
    """Delta = 0 (log 2 per vertex; the fill keeps the entry, the step takes the entry of d_theta), s = 40 and s = 1e-8"""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    L = lm.Level(8, 4, rot, beta)
    lv = _level(abi, L)
    h = _edge_state(L, case)
    D = lm.delta(L, lm.spins(L, h))[:, L.fineonly]
    s = beta * np.sqrt((D * D).sum(-1))
    assert np.all(s == 0.0) if case == "zero" else np.allclose(s, 4 * beta, rtol=1e-12)
    x = _dev(h)
    got = ops.sigma_cfa_evaluate(lv, x).cpu().numpy()
    want = lm.cfa_evaluate(L, h)
    assert np.all(np.isfinite(got)) and abs(got[0] - want[0]) <= 1e-12 * max(abs(want[0]), 1.0), (got, want)
    if case == "zero":
        assert abs(got[0] - len(L.fineonly) * math.log(2.0)) < 1e-12
    ops.sigma_cfa_fill(lv, x, 9, 0, 1)
    filled = x.cpu().numpy()
    if case == "zero":
        assert np.array_equal(filled, h)
    else:
        _close_spins(L, filled, lm.cfa_fill(L, h, 9, 0, 1))
    # the step with the restriction of the state as its proposal: the same neighbour sums
    Lc = L.coarse(beta)
    st = ops.SigmaTwoLevelStep(lv, _level(abi, Lc), 1, seed=9)
    st.set_state(_dev(h))
    st.draw(_dev(lm.copy_from_fine(L, h)))
    terms, trial = st.terms.cpu().numpy(), st.trial().cpu().numpy()
    assert np.all(np.isfinite(terms))
    if case == "zero":
        assert np.array_equal(trial, h) and np.all(terms == 0.0) and int(st.accept[0]) == 1
    else:
        want_new, want_acc, want_terms, want_trial, margin = lm.twolevel_draw(L, Lc, lm.copy_from_fine(L, h), h, 9, 0, 0)
        _close_sum(terms, want_terms, n=L.n * max(1.0, beta))
        _close_spins(L, trial, want_trial)
        assert margin[0] < 1e-9 or bool(st.accept[0]) == bool(want_acc[0])


def test_twolevel_chain_samples_the_fine_law(gpu_ops):
    """8 x 8, beta = 1, 4096 chains: a coarse heat-bath draw on the rotated level, then the two-level step, against the single-level
    10 + 1 draw; chi_m means across chains, |z| < 4.5.  Both levels start from 200 overrelaxation and 20 heat-bath sweeps of their
    own, so a valid step keeps the fine law from the first draw on (tests/test_sigma_level_model.py).
    The step is exact for proposals INDEPENDENT of the current state; the hierarchical chain proposes the successive states of one
    coarse chain, and what is left of their correlation is a bias of the algorithm (the reference's as well), not of the kernels.
    Measured at this shape with one 10 + 1 draw between proposals: z = +4.08 on the device (acceptance 0.17); on the numpy model
    z = +9.3 with one heat-bath sweep between proposals and +3.3 with eight.  The coarse draw here is therefore four 10 + 1 draws."""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    B, beta, n_meas = 4096, 1.0, 60
    lv = abi.sigma_level(8, 8, 0, beta)
    lc = lv.coarse(beta)
    single = ops.sigma_level_initialise(lv, B, 3, 0)
    fine = ops.sigma_level_initialise(lv, B, 4, 0)
    coarse = ops.sigma_level_initialise(lc, B, 5, 0)
    sf, sc = torch.empty_like(fine), torch.empty_like(coarse)
    ops.sigma_level_sweep_draw(lv, single, sf, 10 * 20, 20, 3, 0, 0)
    ops.sigma_level_sweep_draw(lv, fine, sf, 10 * 20, 20, 4, 0, 0)
    ops.sigma_level_sweep_draw(lc, coarse, sc, 10 * 20, 20, 5, 0, 0)
    step = ops.SigmaTwoLevelStep(lv, lc, B, seed=6)
    step.set_state(fine)
    tot_two = torch.zeros(B, dtype=torch.float64, device="cuda")
    tot_one = torch.zeros_like(tot_two)
    n_acc = torch.zeros(B, dtype=torch.float64, device="cuda")
    for k in range(n_meas):
        for r in range(4):
            ops.sigma_level_sweep_draw(lc, coarse, sc, 10, 1, 5, 0, 1000 + 11 * (4 * k + r))
        n_acc += step.draw(coarse)
        tot_two += ops.sigma_level_magnetic_susceptibility(lv, step.theta)
        ops.sigma_level_sweep_draw(lv, single, sf, 10, 1, 3, 0, 1000 + 11 * k)
        tot_one += ops.sigma_level_magnetic_susceptibility(lv, single)
    two, one = (tot_two / n_meas).cpu().numpy(), (tot_one / n_meas).cpu().numpy()
    rate = float(n_acc.sum()) / (B * n_meas)
    print(f"sigma two-level 8x8 beta=1: acceptance rate {rate:.4f}")
    assert 0.0 < rate < 1.0
    err = lambda v: v.std(ddof=1) / math.sqrt(B)
    zcheck("sigma two-level chain vs 10+1 heat bath, chi_m 8x8 beta=1", two.mean(), err(two), one.mean(), err(one), gate=4.5)


def test_errors_not_faults(gpu_ops):
    """bad levels and pairs are MLMCPI_ERR_INVALID with a message.  (A level carries no action kind: the kind-5 refusals of
    mlmcpi_lattice_copy_from_* / mlmcpi_lattice_twolevel_* stay as test_sigma_gpu.py pins them, and are repeated here.)"""
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    x = torch.zeros((2, 2 * 36), dtype=torch.float64, device="cuda")
    for Mt, Mx in ((3, 4), (4, 5), (0, 4), (4, 1)):
        for rot in (0, 1):
            bad = abi.sigma_level(Mt, Mx, rot, 1.0)
            with pytest.raises(abi.MlmcpiError, match="even extents"):
                abi.call("mlmcpi_sigma_level_evaluate", C.byref(bad), C.c_void_p(x.data_ptr()), 2, C.c_void_p(x.data_ptr()), None)
            with pytest.raises(abi.MlmcpiError, match="even extents"):
                abi.call("mlmcpi_sigma_cfa_fill", C.byref(bad), C.c_void_p(x.data_ptr()), 2, 1, 0, 0, None)
            with pytest.raises(abi.MlmcpiError, match="even extents"):
                abi.call("mlmcpi_sigma_level_sweep_draw", C.byref(bad), C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 2, 1, 1, 1, 0, 0, None)
    fine = abi.sigma_level(8, 8, 0, 1.0)
    partners = [abi.sigma_level(8, 8, 0, 1.0), abi.sigma_level(4, 4, 0, 1.0), abi.sigma_level(8, 4, 1, 1.0), abi.sigma_level(4, 4, 1, 1.0)]
    rfine = abi.sigma_level(8, 8, 1, 1.0)
    rpartners = [abi.sigma_level(8, 8, 0, 1.0), abi.sigma_level(4, 4, 1, 1.0), abi.sigma_level(4, 8, 0, 1.0), abi.sigma_level(8, 8, 1, 1.0)]
    p = C.c_void_p(x.data_ptr())
    for f, cs in ((fine, partners), (rfine, rpartners)):
        for c in cs:
            with pytest.raises(abi.MlmcpiError, match="not the CoarsenRotate partner"):
                abi.call("mlmcpi_sigma_twolevel_draw", C.byref(f), C.byref(c), p, p, 2, 1, 0, 0, p, p, None, None)
    # a rotated fine level whose partner would have odd extents
    with pytest.raises(abi.MlmcpiError, match="even extents"):
        abi.call("mlmcpi_sigma_twolevel_draw", C.byref(abi.sigma_level(6, 4, 1, 1.0)), C.byref(abi.sigma_level(3, 2, 0, 1.0)), p, p, 2, 1, 0, 0,
                 p, p, None, None)
    with pytest.raises(abi.MlmcpiError, match="bad arguments"):
        abi.call("mlmcpi_sigma_twolevel_draw", C.byref(fine), C.byref(fine.coarse()), None, p, 2, 1, 0, 0, p, p, None, None)
    for bad_option in ("0x8x256x1", "8x8x100x1", "8x8x256x0", "8x8x256x17", "128x128x256x16", "8x8x256"):
        with pytest.raises(abi.MlmcpiError, match="unknown option or value"):
            abi.set_option("MLMCPI_SIGMA_LEVEL_PLAN", bad_option)
    for bad_option in ("0", "65", "x"):
        with pytest.raises(abi.MlmcpiError, match="unknown option or value"):
            abi.set_option("MLMCPI_SIGMA_TWOLEVEL_GROUPS", bad_option)
    for name, args in (("mlmcpi_sigma_level_initialise", (p, 65536, 1, 0, None)), ("mlmcpi_sigma_level_evaluate", (p, 65536, p, None)),
                       ("mlmcpi_sigma_level_magnetic_susceptibility", (p, 65536, p, None)),
                       ("mlmcpi_sigma_level_copy_from_fine", (p, p, 65536, None)), ("mlmcpi_sigma_level_copy_from_coarse", (p, p, 65536, None)),
                       ("mlmcpi_sigma_twolevel_workspace_bytes", (65536, C.byref(C.c_size_t(0))))):
        with pytest.raises(abi.MlmcpiError, match="bad arguments"):   # a batch beyond the grid: a message, not a launch error
            abi.call(name, C.byref(fine), *args)
    sig = abi.lattice_action(abi.NONLINEAR_SIGMA, 8, 8, beta=1.0)
    with pytest.raises(abi.MlmcpiError, match="status -3"):
        abi.call("mlmcpi_lattice_copy_from_fine", C.byref(sig), 2, 2, p, p, 2, None)
