"""GPU: path_hmc.hip at every launch geometry plan_hmc can choose.

tests/test_gpu_parity.py reaches the register-resident plans at small B and at B = 2100, and four segmented ones (M = 330,
1000 with nt = 12, 32768, 65536).  The cases here (tests/path_hmc_cases.py, each with the plan it is meant to reach) are the
rest: paths shorter than their halo, the boundary M + 2 halo = 1024 of the short plan, the smallest multi-segment paths, the
longest nt either plan takes, workgroups of several waves with R > 1 chosen by the batch size, and hmc_chain_kernel with
R > 1 across waves (the double-buffered LDS exchange over repetitions, a rejected repetition and the extra exchange of the
susceptibility).  Every test first asserts the plan through mlmcpi_path_hmc_plan, so that a change of plan_hmc cannot
silently move a case to another kernel.

Reference: the oracle's dev_hmc_trajectory with the same Philox momenta and accept uniforms, chain by chain.  Bounds are those
of tests/test_gpu_parity.py: energies 1e-11, state 1e-10, accept flags and counts exact; mlmcpi_path_hmc_run against
repeated draws: counts exact, state 1e-12, QoI 1e-13.  The two long trajectories (nt = 479, 2015; nt * dt <= 2) are held
to 100 times the oracle's own sensitivity, the largest movement of its state when every site of the start moves by one
ulp (path_hmc_cases.ulp_sensitivity, measured where the test runs and never from the device's output: 1.2e-15 and 2.9e-15,
so 1.2e-13 and 2.9e-13; the factor covers FMA contraction on the device, which perturbs every step and not only the start).
No Metropolis test compared here is a near-tie: |u - exp(-dH)| > 1e-6 under the oracle, asserted in every test.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import path_hmc_cases as hc
from path_cases import SEED
from test_path_splits_gpu import SENTINEL, assert_bands_untouched, bits_equal, check, dev, guarded, make_action

pytestmark = pytest.mark.gpu


def align256(nbytes):
    return (nbytes + 255) // 256 * 256


def repeated_draws(ops, act, x, B, nt, dt, n_rep, chain0, n_draws, qoi_kind):
    """n_draws x (mlmcpi_path_hmc_draw, then the stand-alone QoI) on x in place: (QoI [B, n_draws], accepted draws [B])"""
    ref = ops.PathHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    qs, total = [], torch.zeros(B, dtype=torch.int32, device="cuda")
    for d in range(n_draws):
        total += ref.draw(x)
        qs.append(ops.qoi_susceptibility(x, act.T_final) if qoi_kind == 2 else ops.qoi_xsquared(x))
    return torch.stack(qs, dim=1), total


# ---- a. mlmcpi_path_hmc_draw on the segmented geometries ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(hc.SEGMENTED)), ids=lambda i: "{kind}-{M}-nt{nt}".format(**hc.SEGMENTED[i]))
def test_segmented_draws_match_oracle(gpu_ops, orc, i):
    """Two consecutive draws of three chains against the oracle; the chain in the middle drawn alone is row 1 of the batch
    bit for bit (the segmented plan does not depend on B); nothing is written outside x, x_trial and the partials: guard
    bands around the state and the workspace, the padding between the workspace's parts and the flags no one-repetition
    draw uses.  x_trial holds the new state of every chain that accepted, bit for bit, and the partials are laid out
    [B][nseg][4]: their second column sums, in segment order, to the kinetic energy the draw reports, and segment by
    segment it is the sum of the oracle's squared momenta over the sites the plan gives that segment (with one segment any
    rotation of the buffer around the ring computes the same draw; with several, this is what shows which sites each owns)."""
    from mlmcpathintegral_amd import abi
    ops, c = gpu_ops, hc.SEGMENTED[i]
    kind, M, nt, dt, B = c["kind"], c["M"], c["nt"], c["dt"], hc.SEG_B
    act = make_action(kind, M)
    plan = ops.path_hmc_plan(act, B, nt)
    assert plan == c["plan"] == ops.path_hmc_plan(act, 1, nt), (plan, c["what"])
    x0, flags, energies, states, margin = hc.segmented_run(i)
    assert margin > hc.MARGIN
    if c.get("long"):
        worst, counted = hc.ulp_sensitivity(i)
        assert counted == B * hc.SEG_DRAWS and 0 < worst < 1e-13
        bound = 100 * worst
    hmc = ops.PathHMC(act, B, nt, dt, n_rep=1, seed=SEED, chain0=hc.SEG_CHAIN0)
    solo = ops.PathHMC(act, 1, nt, dt, n_rep=1, seed=SEED, chain0=hc.SEG_CHAIN0 + 1)
    nwork, nseg = hmc.work.numel() // 8, plan["nseg"]
    off_partials = align256(B * M * 8) // 8
    end_partials = off_partials + B * nseg * 4
    assert hmc.work.numel() == align256(B * M * 8) + align256(B * nseg * 32) + align256(2 * B * 4)
    wbig, work = guarded(nwork)
    hmc.work = work
    xbig, x = guarded(B * M)
    x = x.view(B, M)
    x.copy_(dev(x0))
    xs = dev(x0[1:2])
    sentinel = torch.full((nwork,), SENTINEL, dtype=torch.float64, device="cuda")
    for d in range(hc.SEG_DRAWS):
        work.fill_(SENTINEL)
        acc = hmc.draw(x).cpu().numpy()
        en = hmc.energies.cpu().numpy()
        what = f"{kind} M={M} nt={nt} draw {d}"
        assert (acc == flags[:, d]).all(), f"{what}: accept flags {acc} vs {flags[:, d]}"
        for b in range(B):
            check(en[b], energies[b, d], 1e-11, f"{what} chain {b} energies")
        got = x.cpu().numpy()
        if c.get("long"):
            err = float(np.max(np.abs(got - states[d])))
            print(f"[hmc] {what}: max |state - oracle| = {err:.3e} (bound {bound:.3e} = 100 x {worst:.3e})")
            assert err <= bound, f"{what}: max |state - oracle| = {err:.3e} > {bound:.3e}"
        else:
            check(got, states[d], 1e-10, f"{what} state")
        # what the draw may write: x_trial [B * M] and the partials [B * nseg * 4], nothing else
        assert_bands_untouched(wbig, nwork, f"{what} workspace")
        assert_bands_untouched(xbig, B * M, f"{what} state")
        assert bits_equal(work[B * M:off_partials], sentinel[B * M:off_partials]), f"{what}: wrote behind x_trial"
        assert bits_equal(work[end_partials:], sentinel[end_partials:]), f"{what}: wrote behind the partials"
        x_trial, partials = work[:B * M].view(B, M), work[off_partials:end_partials].view(B, nseg, 4).cpu().numpy()
        assert not (x_trial == SENTINEL).any() and not (partials == SENTINEL).any(), f"{what}: a site or a partial not written"
        for b in np.flatnonzero(acc):
            assert bits_equal(x_trial[b], x[b]), f"{what}: x_trial of chain {b} is not the state it accepted"
        for b in range(B):
            t0 = 0.0
            for k in range(nseg):
                t0 += partials[b, k, 1]
            assert 0.5 * t0 == en[b, 1], f"{what}: partials of chain {b}"
            # segment k sums the sites the plan says it owns: its kinetic partial against the oracle's momenta there (a sum
            # of squares, at the energies' bound; a segment that owned other sites would be off by its whole value)
            p2 = hc.oracle_momenta(M, hc.SEG_CHAIN0 + b, d) ** 2
            check(partials[b, :, 1], [p2[lo:hi].sum() for lo, hi in hc.owned_ranges(plan, M)], 1e-11, f"{what} chain {b} partials by segment")
        # the chain in the middle on its own
        acc1 = solo.draw(xs)
        assert int(acc1[0]) == acc[1] and bits_equal(xs[0], x[1]) and bits_equal(solo.energies[0], hmc.energies[1]), what
    if "refused" in c:
        before = x.clone()
        with pytest.raises(abi.MlmcpiError, match="too long for the fused trajectory"):
            ops.PathHMC(act, B, c["refused"], dt, seed=SEED)
        hmc.nt = c["refused"]
        with pytest.raises(abi.MlmcpiError, match="too long for the fused trajectory"):
            hmc.draw(x)
        assert bits_equal(x, before)


# ---- b. draw and run at the geometries the batch size selects ----------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(hc.BATCH)), ids=lambda i: "{kind}-{M}-B{B}".format(**hc.BATCH[i]))
def test_batch_selected_geometries(gpu_ops, orc, i):
    """One draw, then mlmcpi_path_hmc_run (n_draws = 2, n_rep = 2) against repeated draws plus the stand-alone QoI with the
    assertions of test_hmc_run_one_wave_chains_equal_repeated_draws; chains 0, 1, B / 2 and B - 1 against the oracle."""
    ops, c = gpu_ops, hc.BATCH[i]
    kind, M, B, dt, nt = c["kind"], c["M"], c["B"], c["dt"], hc.BATCH_NT
    act = make_action(kind, M)
    assert ops.path_hmc_plan(act, B, nt) == c["plan"]
    assert B * M * 8 <= 16 * 2 ** 20
    chains = hc.batch_chains(B)
    counts_o, states_o, first, margin = hc.batch_outcomes(i, chains)
    assert margin > hc.MARGIN
    x0 = hc.batch_start(M, B)
    what = f"{kind} M={M} B={B}"
    xd = x0.cuda()
    hmc = ops.PathHMC(act, B, nt, dt, n_rep=1, seed=SEED, chain0=0)
    acc = hmc.draw(xd).cpu().numpy()
    for k, b in enumerate(chains):
        flag, e, s = first[k]
        assert acc[b] == flag, f"{what} draw: accept flag of chain {b}"
        check(hmc.energies[b].cpu().numpy(), e, 1e-11, f"{what} draw: energies of chain {b}")
        check(xd[b].cpu().numpy(), s, 1e-10, f"{what} draw: chain {b}")
    del xd
    qoi_kind = 2 if kind == "rotor" else 1
    xa, xb = x0.cuda(), x0.cuda()
    run = ops.PathHMC(act, B, nt, dt, n_rep=hc.BATCH_REP, seed=SEED, chain0=0)
    q, cnt = ops.path_hmc_run(run, xa, hc.BATCH_DRAWS, qoi_kind)
    qs, total = repeated_draws(ops, act, xb, B, nt, dt, hc.BATCH_REP, 0, hc.BATCH_DRAWS, qoi_kind)
    assert torch.equal(cnt, total), (cnt, total)
    check(xa.cpu().numpy(), xb.cpu().numpy(), 1e-12, f"{what} run: state after {hc.BATCH_DRAWS} draws")
    check(q.cpu().numpy(), qs.cpu().numpy(), 1e-13, f"{what} run: per-draw QoIs")
    counts = cnt.cpu().numpy()
    assert not (counts == 0).all() and not (counts == hc.BATCH_DRAWS).all(), "the batch should see both outcomes"
    for k, b in enumerate(chains):
        assert counts[b] == counts_o[k], f"{what} run: accepted draws of chain {b}"
        check(xa[b].cpu().numpy(), states_o[k], 1e-10, f"{what} run: chain {b} vs oracle")


# ---- c. mlmcpi_path_hmc_run with more than one wave and R > 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(hc.RUN)), ids=lambda i: "{kind}-{M}".format(**hc.RUN[i]))
def test_run_across_waves_with_several_sites_per_thread(gpu_ops, orc, i):
    """hmc_chain_kernel<KIND, R > 1> on 8 or 16 waves, n_draws = 3, n_rep = 2, with a rejected repetition and an accepted
    draw among the three chains: against repeated draws plus QoI, against the oracle, with qoi_kind = 0 and no QoI array,
    and as one call of 5 draws against calls of 2 and 3."""
    from mlmcpathintegral_amd import abi
    ops, c = gpu_ops, hc.RUN[i]
    kind, M, dt, qoi_kind = c["kind"], c["M"], c["dt"], c["qoi_kind"]
    B, nt, n_draws, n_rep, chain0 = hc.RUN_B, hc.RUN_NT, hc.RUN_DRAWS, hc.RUN_REP, hc.RUN_CHAIN0
    act = make_action(kind, M)
    assert ops.path_hmc_plan(act, B, nt) == c["plan"]
    x0, flags, x_oracle, q_oracle, rejected, margin, cut = hc.run_outcomes(i)
    assert margin > hc.MARGIN and rejected >= 1 and flags.any() and not flags.all()
    what = f"{kind} M={M}"
    xa, xb = dev(x0), dev(x0)
    run = ops.PathHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    q, cnt = ops.path_hmc_run(run, xa, n_draws, qoi_kind)
    qs, total = repeated_draws(ops, act, xb, B, nt, dt, n_rep, chain0, n_draws, qoi_kind)
    assert torch.equal(cnt, total), (cnt, total)
    check(xa.cpu().numpy(), xb.cpu().numpy(), 1e-12, f"{what}: state after {n_draws} draws")
    check(q.cpu().numpy(), qs.cpu().numpy(), 1e-13, f"{what}: per-draw QoIs")
    # the oracle; both outcomes: a draw with both repetitions rejected, and an accepted one
    counts = cnt.cpu().numpy()
    assert (counts == flags.sum(axis=1)).all(), (counts, flags)
    assert (counts < n_draws).any() and counts.sum() > 0, counts
    check(xa.cpu().numpy(), x_oracle, 1e-10, f"{what}: state vs oracle")
    if qoi_kind == 2:
        # the charge is a sum of differences that telescopes: it moves with the state only where a difference crosses the
        # branch cut of mod_2pi, and none comes closer to it than 1e-5; 1e-10 is the bound of test_path_evaluate_force_qoi
        assert cut > 1e-5
        check(q.cpu().numpy(), q_oracle, 1e-10, f"{what}: susceptibility vs oracle")
    else:
        # <x^2> of a state within 1e-10 max(1, |x|) of the oracle's moves by at most 2 |x| times that, plus the 1e-12 of the sum
        top = max(1.0, float(np.max(np.abs(x_oracle))))
        err = np.abs(q.cpu().numpy() - q_oracle)
        assert (err <= 1e-12 * np.maximum(1.0, np.abs(q_oracle)) + 2 * top * 1e-10 * top).all(), f"{what}: <x^2> vs oracle: {err.max():.3e}"
    # qoi_kind = 0 and no QoI array
    xc, cnt0 = dev(x0), torch.full((B,), -1, dtype=torch.int32, device="cuda")
    abi.call("mlmcpi_path_hmc_run", C.byref(act), ops._p(xc), B, nt, dt, n_rep, n_draws, 0, SEED, chain0, 0, ops._p(run.work),
             None, ops._p(cnt0), ops._stream())
    assert bits_equal(xc, xa) and torch.equal(cnt0, cnt), f"{what}: qoi_kind = 0"
    # 5 draws in one call, and in calls of 2 and 3 on one PathHMC (traj0 carries on)
    _, flags5, x5, _, _, margin5, _ = hc.run_outcomes(i, 5)
    assert margin5 > hc.MARGIN
    xe, xf = dev(x0), dev(x0)
    one = ops.PathHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    q5, c5 = ops.path_hmc_run(one, xe, 5, qoi_kind)
    two = ops.PathHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    q2, c2 = ops.path_hmc_run(two, xf, 2, qoi_kind)
    assert two.traj == 2 * n_rep
    q3, c3 = ops.path_hmc_run(two, xf, 3, qoi_kind)
    assert bits_equal(xe, xf) and torch.equal(c5, c2 + c3), f"{what}: 5 draws vs 2 + 3"
    assert bits_equal(q5, torch.cat([q2, q3], dim=1)), f"{what}: QoI columns of 5 draws vs 2 + 3"
    assert (c5.cpu().numpy() == flags5.sum(axis=1)).all(), (c5, flags5)
    check(xe.cpu().numpy(), x5, 1e-10, f"{what}: state after 5 draws vs oracle")


def test_small_segmented_run_equals_repeated_draws(gpu_ops):
    """mlmcpi_path_hmc_run on a segmented path (quartic M = 1000, nt = 12) issues the launches of n_draws calls of
    mlmcpi_path_hmc_draw, each followed by the QoI reduction: the same kernels on the same arguments in the same order, so
    state and counts are bit-identical; its QoI array is draw-major, [n_draws][B], as chain_major == 0 says."""
    from mlmcpathintegral_amd import abi
    ops, c = gpu_ops, hc.SEGMENTED_RUN
    kind, M, nt, dt, n_draws, n_rep, B, chain0 = c["kind"], c["M"], c["nt"], c["dt"], c["n_draws"], c["n_rep"], hc.RUN_B, hc.RUN_CHAIN0
    act = make_action(kind, M)
    plan = ops.path_hmc_plan(act, B, nt)
    assert plan == c["plan"] and plan["chain_major"] == 0
    layout = C.c_int32(-1)
    abi.call("mlmcpi_path_hmc_run_layout", C.byref(act), B, nt, C.byref(layout))
    assert layout.value == 0
    x0 = hc.start(kind, M, B, M + 1)
    xa, xb, xc = dev(x0), dev(x0), dev(x0)
    run = ops.PathHMC(act, B, nt, dt, n_rep=n_rep, seed=SEED, chain0=chain0)
    raw = torch.full((n_draws * B,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    abi.call("mlmcpi_path_hmc_run", C.byref(act), ops._p(xa), B, nt, dt, n_rep, n_draws, c["qoi_kind"], SEED, chain0, 0,
             ops._p(run.work), ops._p(raw), ops._p(cnt), ops._stream())
    qs, total = repeated_draws(ops, act, xb, B, nt, dt, n_rep, chain0, n_draws, c["qoi_kind"])
    assert bits_equal(xa, xb) and torch.equal(cnt, total), (cnt, total)
    assert int(total.sum()) > 0 and not torch.equal(xa, dev(x0))
    check(raw.view(n_draws, B).cpu().numpy(), qs.t().cpu().numpy(), 1e-13, "draw-major QoIs")
    assert len({float(v) for v in raw.cpu().numpy()}) == n_draws * B, "every (draw, chain) has its own value"
    q, cnt2 = ops.path_hmc_run(run, xc, n_draws, c["qoi_kind"])
    assert q.shape == (B, n_draws) and bits_equal(q, raw.view(n_draws, B).t().contiguous()) and torch.equal(cnt2, cnt)
