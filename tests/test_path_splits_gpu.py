"""GPU: the 1-D path units (path1d.hip, path_twolevel.hip, the statistics kernels of lattice_reduce.hip) past one split, one
pass and one block of chains.

tests/test_gpu_parity.py runs path_reduce_kernel with more than one workgroup per chain for the rotor only, at lengths the
split divides, and everything else here with one pass of each loop and a handful of chains.  The shapes below are the
smallest that reach each branch of choose_split (tests/path_cases.py SHAPES, mirrored launch arithmetic asserted in
tests/test_path_reference.py):

    (1025, 3)      2 splits of 513 and 512
    (2050, 2)      3 splits of 684, 684, 682: short last split, three passes of 256 threads with a tail
    (4100, 1500)   want = 2 < cap: 2 splits of 2050, 9 passes each
    (1100, 300)    2 splits and two blocks of path_finish_kernel, the second with 44 live threads
    (1100, 2100)   want = 1: one workgroup walks a chain of M > 1024 and finishes in the kernel

Reference: tests/path_reference.py, long double from the formulas, pinned on the CPU to the oracle and the survey's known
answers; the oracle itself (dev_initialise, dev_twolevel_draw, dev_hmc_trajectory, Statistics) where random streams are
involved.  Every chain has its own seeded data and every chain and every site is compared.  Tolerances are those of the
header of tests/test_gpu_parity.py: 1e-12 * max(1, |want|) for evaluate, force and <x^2>, 1e-10 for the susceptibility
and the two-level terms, 1e-12 for the two-level state; transfers, masked chains, accept flags, rotor initial states and
guard bands bit for bit.  All conditions on the inputs (distance from the branch cut of mod_2pi, both outcomes of the
two-level steps, both mask values on every level of the hierarchy) are properties of the oracle's numbers alone and are
asserted in tests/test_path_reference.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import path_cases as cases
import path_reference as ref

pytestmark = pytest.mark.gpu

SEED = cases.SEED
SENTINEL = -7.25
PAD = 4096     # doubles of guard band on either side of an output


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def make_action(kind, M, levels_down=0):
    """the action of cases.params(kind, M), or the one `levels_down` coarsenings below it (same T_final, M halved each time)"""
    from mlmcpathintegral_amd import abi
    p = cases.params(kind, M)
    M >>= levels_down
    return abi.path_action(cases.KINDS[kind], M, p["T_final"], p.get("m0", 1.0), p.get("mu2", 1.0), p.get("lam", 0.0), p.get("x0", 0.0))


def check(got, want, tol, what, where=None):
    """|got - want| <= tol * max(1, max |want|) on every entry, the maximum taken over the chain ([B, n]: per row) as
    assert_close of tests/test_gpu_parity.py is called there; names the worst entry"""
    got = np.asarray(got, dtype=np.float64)
    want64 = np.asarray(want, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = np.abs(got.astype(ref.LD) - np.asarray(want, dtype=ref.LD)).astype(np.float64)
    assert np.isfinite(err).all(), f"{what}: entry not finite at {np.argwhere(~np.isfinite(err))[0]}"
    bound = tol * np.maximum(1.0, np.max(np.abs(want64), axis=-1, keepdims=True)) * np.ones_like(err)
    worst = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    print(f"[path] {what}: worst |diff| = {err[worst]:.3e} (bound {bound[worst]:.3e})")
    assert (err <= bound).all(), (f"{what}: |diff| = {err[worst]:.3e} > {bound[worst]:.3e} at {worst}"
                                  + (f" ({where(worst)})" if where else "") + f"; {int((err > bound).sum())} entries beyond")


def check_per_chain(got, want, tol, what):
    """|got[b] - want[b]| <= tol * max(1, |want[b]|) for every chain b"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(ref.LD) - want).astype(np.float64)
    bound = tol * np.maximum(1.0, np.abs(np.asarray(want, dtype=np.float64)))
    assert np.isfinite(got).all(), f"{what}: chain {int(np.argmax(~np.isfinite(got)))} not finite"
    b = int(np.argmax(err / bound))
    print(f"[path] {what}: worst chain {b}: |diff| = {err[b]:.3e} (bound {bound[b]:.3e})")
    assert (err <= bound).all(), f"{what}: chain {b}: |diff| = {err[b]:.3e} > {bound[b]:.3e}; {int((err > bound).sum())} chains beyond"


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def guarded(n):
    """a sentinel-filled tensor of PAD + n + PAD doubles and its middle"""
    big = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    return big, big[PAD:PAD + n]


def assert_bands_untouched(big, n, what):
    band = torch.full((PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    assert bits_equal(big[:PAD], band), f"{what}: wrote in front of its output"
    assert bits_equal(big[PAD + n:], band), f"{what}: wrote behind its output"


def where_site(M, B):
    """(chain, site) -> the workgroup and pass of the grid-stride loop of path_force_kernel that writes it"""
    n = cases.choose_split(M, B)

    def f(idx):
        b, j = (int(i) for i in idx)
        return f"chain {b}, site {j}: workgroup {(j // 256) % n} of {n}, pass {j // (256 * n)}"
    return f


# ---- reductions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(cases.KINDS))
@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_evaluate_across_splits(gpu_ops, kind, M, B):
    """path_reduce_kernel<KIND, R_ENERGY> + path_finish_kernel; the last chain carries spikes on every split boundary"""
    x = cases.path_input(kind, M, B)
    S = gpu_ops.path_evaluate(make_action(kind, M), dev(x)).cpu().numpy()
    check_per_chain(S, cases.reference("action", kind, M, B), 1e-12, f"evaluate {kind} ({M}, {B})")


@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_qoi_across_splits(gpu_ops, M, B):
    """<x^2> on the harmonic input, the susceptibility on the rotor input (every chain: the inputs keep away from the
    branch cut of mod_2pi, tests/test_path_reference.py)"""
    X2 = gpu_ops.qoi_xsquared(dev(cases.path_input("harmonic", M, B))).cpu().numpy()
    check_per_chain(X2, cases.reference("xsquared", "harmonic", M, B), 1e-12, f"<x^2> ({M}, {B})")
    T = cases.params("rotor", M)["T_final"]
    chi = gpu_ops.qoi_susceptibility(dev(cases.path_input("rotor", M, B)), T).cpu().numpy()
    check_per_chain(chi, cases.reference("susceptibility", "rotor", M, B), 1e-10, f"susceptibility ({M}, {B})")


# ---- force, initialise, transfers: values and guard bands -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(cases.KINDS))
@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_force_across_passes(gpu_ops, kind, M, B):
    from mlmcpathintegral_amd import abi, ops
    act, x = make_action(kind, M), dev(cases.path_input(kind, M, B))
    big, f = guarded(B * M)
    abi.call("mlmcpi_path_force", C.byref(act), ops._p(x), ops._p(f), B, ops._stream())
    assert_bands_untouched(big, B * M, f"path_force_kernel {kind} ({M}, {B})")
    check(f.reshape(B, M).cpu().numpy(), cases.reference("force", kind, M, B), 1e-12, f"force {kind} ({M}, {B})", where_site(M, B))


@pytest.mark.parametrize("kind,M,B", [("rotor", 1025, 3), ("rotor", 1100, 300), ("quartic", 2050, 2)])
def test_initialise_across_passes(gpu_ops, orc, kind, M, B):
    from mlmcpathintegral_amd import abi, ops
    act = make_action(kind, M)
    A = orc.Action(cases.KINDS[kind], **cases.params(kind, M))
    big, x = guarded(B * M)
    abi.call("mlmcpi_path_initialise", C.byref(act), ops._p(x), B, SEED, 5, ops._stream())
    assert_bands_untouched(big, B * M, f"path_init_kernel {kind} ({M}, {B})")
    got = x.reshape(B, M).cpu().numpy()
    if kind != "rotor":
        assert (got == 0).all() and not np.signbit(got).any()
        return
    want = np.stack([A.dev_initialise(SEED, 5 + b) for b in range(B)])
    # (as test_path_initialise: the same uniform, -pi + 2 pi u with or without a fused multiply-add)
    assert (got == want).all() or np.max(np.abs(got - want)) < 1e-15, np.argwhere(got != want)[0]
    assert len({got[b].tobytes() for b in range(B)}) == B


@pytest.mark.parametrize("Mc,B", [(1025, 3), (2050, 3), (1100, 300)])
def test_transfers_across_passes(gpu_ops, Mc, B):
    from mlmcpathintegral_amd import abi, ops
    rng = np.random.default_rng(Mc + B)
    fine_h, coarse_h = rng.normal(size=(B, 2 * Mc)), rng.normal(size=(B, Mc))
    fine = dev(fine_h)
    big, coarse = guarded(B * Mc)
    abi.call("mlmcpi_path_copy_from_fine", ops._p(fine), ops._p(coarse), Mc, B, ops._stream())
    assert_bands_untouched(big, B * Mc, f"copy_from_fine ({Mc}, {B})")
    assert bits_equal(coarse.reshape(B, Mc), dev(ref.copy_from_fine(fine_h))), "copy_from_fine is fine[:, ::2]"
    assert bits_equal(fine, dev(fine_h)), "copy_from_fine leaves the fine paths alone"
    big, out = guarded(B * 2 * Mc)
    out.copy_(fine.reshape(-1))
    abi.call("mlmcpi_path_copy_from_coarse", ops._p(dev(coarse_h)), ops._p(out), Mc, B, ops._stream())
    assert_bands_untouched(big, B * 2 * Mc, f"copy_from_coarse ({Mc}, {B})")
    out = out.reshape(B, 2 * Mc)
    assert bits_equal(out[:, ::2], dev(coarse_h)), "copy_from_coarse sets the even sites"
    assert bits_equal(out[:, 1::2], fine[:, 1::2]), "copy_from_coarse leaves the odd sites alone"
    assert bits_equal(out, dev(ref.copy_from_coarse(coarse_h, fine_h)))


# ---- the two-level step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M,rough", cases.TWOLEVEL_CASES)
def test_twolevel_masked_draws(gpu_ops, kind, M, rough):
    """Six draws of twolevel_fused_kernel on 5 chains under masks that change from draw to draw, against the oracle's
    dev_twolevel_draw with chain id chain0 + b and the draw's step number -- for an unmasked chain as if no chain were
    masked: streams do not shift and the step counter advances for everyone.  Masked chains: theta bit for bit, accept 0,
    terms exactly 0.  Then one draw with d_terms = NULL: accept flags and state of the same draw with terms."""
    from mlmcpathintegral_amd import abi, ops
    B = cases.TWOLEVEL_B
    theta0, draws = cases.twolevel_run(kind, M, rough)
    fine, coarse = make_action(kind, M), make_action(kind, M, levels_down=1)
    step = gpu_ops.PathTwoLevelStep(fine, coarse, B, seed=SEED, chain0=cases.TWOLEVEL_CHAIN0)
    step.set_state(dev(theta0))
    for t, (xc, mask, accept, terms, theta) in enumerate(draws):
        step.terms.fill_(SENTINEL)
        step.accept.fill_(-1)
        before = step.theta.clone()
        acc = step.draw(dev(xc), mask=torch.as_tensor(mask, dtype=torch.int32).cuda()).cpu().numpy()
        got_terms, got_theta = step.terms.cpu().numpy(), step.theta
        off = torch.as_tensor(mask == 0).cuda()
        assert bits_equal(got_theta[off], before[off]), f"draw {t}: a masked chain moved"
        assert (acc[mask == 0] == 0).all() and (got_terms[mask == 0] == 0).all(), f"draw {t}: masked chains {acc}, {got_terms}"
        for b in np.flatnonzero(mask):
            check(got_terms[b], terms[b], 1e-10, f"{kind} M={M} draw {t} chain {b} terms")
        assert (acc == accept).all(), f"draw {t}: accept flags {acc} vs {accept} (mask {mask}, dS {terms.sum(axis=1)})"
        check(got_theta.cpu().numpy(), theta, 1e-12, f"{kind} M={M} state after draw {t}")
    # d_terms = NULL, straight through the ABI: the seventh draw twice from one state, with and without terms
    t, xc = len(draws), dev(draws[1][0])
    mask = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device="cuda")
    state = step.theta.clone()
    with_terms = step.draw(xc, mask=mask).clone()
    assert step.step == t + 1
    theta_with, theta_without = step.theta.clone(), state.clone()
    accept = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    abi.call("mlmcpi_path_twolevel_draw_masked", C.byref(fine), C.byref(coarse), ops._p(xc), ops._p(theta_without), B, SEED,
             cases.TWOLEVEL_CHAIN0, t, ops._p(step.work), ops._p(mask), ops._p(accept), None, ops._stream())
    assert torch.equal(accept, with_terms) and bits_equal(theta_without, theta_with)


def test_hierarchical_sampler_matches_the_oracle_composition(gpu_ops, orc):
    """mlmc.HierChain on the quartic action, levels 256 / 128 / 64, 8 chains: restriction, HMC on the coarsest level, masked
    two-level steps upwards, against the same composition written with the oracle (cases.hier_run; both mask values reach
    every level, tests/test_path_reference.py).  Accept flags exactly, states at the tolerance of
    test_config5_hierarchy_matches_oracle."""
    from mlmcpathintegral_amd import abi, mlmc
    H = cases.HIER
    acts = [abi.path_action(abi.QUARTIC, M, H["T_final"], 1.0, 1.0, 1.0, 1.0) for M in H["levels"]]
    L = len(acts)
    chain = mlmc.HierChain(acts, 0, H["B"], H["nt"], H["dt"], H["seed"], chain0=H["chain0"])
    chain.state[0].copy_(dev(cases.hier_start()))
    seen = {k: set() for k in range(L - 1)}
    for d, rec in enumerate(cases.hier_run()):
        out = chain.draw()
        assert out is chain.state[0]
        level_acc = {k: v.cpu().numpy().copy() for k, v in chain.level_accepted.items()}
        for k in range(L - 1, -1, -1):
            mask, accept, state = rec[k]
            got = (chain.hmc.accept if k == L - 1 else chain.steps[k].accept).cpu().numpy()
            assert (got == accept).all(), f"draw {d} level {k}: accept {got} vs {accept} (mask {mask})"
            check(chain.state[k].cpu().numpy(), state, 1e-9, f"draw {d} level {k} state")
            if k < L - 1:
                seen[k].update(mask.tolist())
            total = sum(r[k][1] for r in cases.hier_run()[:d + 1])
            assert (level_acc[k] == total).all()
    assert all(s == {0, 1} for s in seen.values()), seen


# ---- statistics kernels at B = 300 ------------------------------------------------------------------------------------------------
def ar1_series(n, B, seed):
    """[n, B]: AR(1) series with correlations 0 .. 0.9 across the chains around chain-dependent means"""
    rng = np.random.default_rng(seed)
    rho, mean = 0.9 * np.arange(B) / (B - 1), 0.3 + 0.01 * np.arange(B)
    s, v = np.zeros((n, B)), np.zeros(B)
    for j in range(n):
        v = rho * v + rng.normal(size=B)
        s[j] = mean + v
    return s


def test_stats_accumulate_two_blocks(gpu_ops):
    """stats_accumulate_kernel at B = 300 (two blocks, 44 live threads in the second), 25 samples, against the long-double
    power sums.  A sum takes at most n + 3 roundings of relative size 2^-53 (three products, n additions): 3.1e-15 of
    sum |q|^k; asserted at 1e-14 of it."""
    n, B = 25, 300
    series = ar1_series(n, B, 11)
    big, acc = guarded(5 * B)
    acc.zero_()
    for j in range(n):
        gpu_ops.stats_accumulate(acc, dev(series[j]))
    assert_bands_untouched(big, 5 * B, "stats_accumulate_kernel")
    got, want = acc.reshape(B, 5).cpu().numpy(), ref.power_sums(series)
    scale = ref.power_sums(np.abs(series)).astype(np.float64)
    err = np.abs(got.astype(ref.LD) - want).astype(np.float64)
    assert (got[:, 0] == n).all()
    assert (err <= 1e-14 * scale).all(), np.argwhere(err > 1e-14 * scale)[0]


def test_windowed_statistics_two_blocks(gpu_ops, orc):
    """stats_window_record_kernel and stats_window_tau_int at B = 300, window 5, against the oracle's Statistics per chain
    (tolerances of test_windowed_statistics_on_the_device_equal_the_oracle), and the pooled tau_int against the same
    quantity from the oracle's per-chain running sums."""
    n, B, W = 40, 300, 5
    series = ar1_series(n, B, 12)
    state = gpu_ops.stats_window_state(B, W)
    stats = [orc.Statistics(W) for _ in range(B)]
    for j in range(n):
        gpu_ops.stats_window_record(state, dev(series[j]))
        for b in range(B):
            stats[b].record(series[j, b])
        if j + 1 not in (3, 7, n):
            continue
        st = state.cpu().numpy()
        tau = gpu_ops.stats_window_tau_int(state, pooled=False).cpu().numpy()
        cov = np.zeros((B, W))
        for b in range(B):
            out = stats[b].get()
            nn, a1, S = stats[b].sums()
            assert st[b, 0] == j + 1 == out["samples"] == nn, b
            assert abs(st[b, 1] - out["average"]) < 1e-13, b
            assert abs(nn / (nn - 1.0) * (st[b, 2] - st[b, 1] ** 2) - out["variance"]) < 1e-12, b
            assert abs(tau[b] - out["tau_int"]) < 1e-10, (j, b, tau[b], out["tau_int"])
            cov[b] = (S - a1 * a1) * (1.0 - np.arange(W) / nn)
        c = cov.mean(axis=0)
        want = max(1.0, 1.0 + 2.0 * c[1:].sum() / c[0])
        pooled = float(gpu_ops.stats_window_tau_int(state, pooled=True))
        assert abs(pooled - want) < 1e-10, (j, pooled, want)


def test_rotor_draw_qoi_moments_two_blocks(gpu_ops):
    """mlmcpi_path_sweep_draw_qoi(acc=...) at B = 300: path_finish_kernel with d_acc in its second block.  rotor_sweeps.hip
    takes that path whenever a QoI is asked for, whatever the number of segments; M = 4 is the smallest even M whose charge
    can be non-zero (cases.SWEEP_QOI).  Three draws into one accumulator: the moments are those of stats_accumulate on the
    returned values, bit for bit, as test_rotor_draw_qoi_record_in_one_call_equals_the_three_steps asserts for B = 2..3."""
    from mlmcpathintegral_amd import abi
    c = cases.SWEEP_QOI
    M, B = c["M"], c["B"]
    act = abi.path_action(abi.ROTOR, M, c["T_final"], c["m0"])
    x = gpu_ops.path_initialise(act, B, SEED, c["chain0"])
    acc = torch.zeros((B, 5), dtype=torch.float64, device="cuda")
    want = torch.zeros((B, 5), dtype=torch.float64, device="cuda")
    for d in range(3):
        sweep0 = c["sweep0"] + d * (c["n_or"] + c["n_hb"])
        plain = x.clone()
        gpu_ops.path_sweep_draw(act, plain, torch.empty_like(plain), c["n_or"], c["n_hb"], SEED, c["chain0"], sweep0)
        src = x.clone()
        res, _, q = gpu_ops.path_sweep_draw_qoi(act, src, torch.empty_like(src), src, c["n_or"], c["n_hb"], SEED, c["chain0"], sweep0,
                                                acc=acc)
        assert torch.equal(res, plain), d
        chi = gpu_ops.qoi_susceptibility(plain, c["T_final"])
        assert float((q - chi).abs().max()) <= 1e-10
        if d == 0:
            tail = q[256:].cpu().numpy()
            assert (tail < 1e-20).any() and (tail > 0.1 / c["T_final"]).any(), "zero and non-zero charges in the second block"
        gpu_ops.stats_accumulate(want, q)
        assert torch.equal(acc, want), (d, int((acc != want).any(dim=1).nonzero()[0]))
        x = plain
