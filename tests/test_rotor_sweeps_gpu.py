"""GPU: rotor_sweeps.hip at both heat-bath samplers and at the limits of its LDS image.

tests/test_gpu_parity.py compares the rotor's sweeps with the oracle at 2 m0 / a = 4 only -- the step-envelope
instantiation rotor_sweep_kernel<true, true> in the middle of its range -- and at ring lengths away from every edge of
path_sweep_impl's segment arithmetic.  Here (cases and mirrored launch arithmetic: tests/rotor_sweep_cases.py, asserted on
the CPU in tests/test_rotor_sweep_cases.py):

    concentrations   flat 0.5, mid 4, top 16 (the last value of the step envelope), over 16.0000064 (the first values of the
                     wrapped Cauchy: rotor_sweep_kernel<true, false>, heatbath_cells<256, 4, true> with HbPool), peaked 64,
                     sharp 400
    M = 2, 4, 6      the halo wraps the ring many times; at M = 2 both neighbours are one site
    M = 1980 / 1976  one segment whose image is the full 2048 doubles, H2 = 1024 pairs in the closed form (without / with
                     the QoI launch's extra halo pair); 1982 / 1978 the first lengths with two segments, owned length
                     rounded up to even
    M = 2044 / 2046  the same two edges for a heat-bath-only launch: 1023 cells per colour phase against a retry pool of 256
    M = 5930         four segments with QoI, rounded owned length, short last segment
    M = 4096 (33,2)  four launches ending in the caller's buffer

Reference: the oracle's device-order sweeps applied one at a time with keys (SEED, CHAIN0 + b, SWEEP0 + s); every chain
and every site compared.  Tolerances are those of tests/test_gpu_parity.py and its header: HB_TOL[min(n_hb, 2)] through
assert_angles_close; closed form 1e-13; susceptibility 1e-10; everything that is the same arithmetic on the device twice
(fused against split launches, QoI draw against plain draw) bit for bit.  Every comparison with the oracle prints its
worst angular difference ("[rotor] ...") in front of its assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import path_reference as ref
import rotor_sweep_cases as cases
from test_gpu_parity import HB_TOL, assert_angles_close, assert_close
from test_path_splits_gpu import assert_bands_untouched, bits_equal, check_per_chain, guarded

pytestmark = pytest.mark.gpu

SEED, B, CHAIN0, SWEEP0 = cases.SEED, cases.B, cases.CHAIN0, cases.SWEEP0


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def make_action(scale, M):
    from mlmcpathintegral_amd import abi
    p = cases.params(scale, M)
    return abi.path_action(abi.ROTOR, M, p["T_final"], p["m0"])


def angle_err(got, want):
    d = np.asarray(got) - np.asarray(want)
    return np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi)))


def compare(got, want, tol, what):
    """print the worst angular difference and where it is, then assert_angles_close (bound 4 * tol)"""
    err = angle_err(got, want)
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"[rotor] {what}: worst angular diff = {err[worst]:.3e} at (chain, site) {tuple(int(i) for i in worst)}, "
          f"bound {4 * tol:.1e}, {int((err > 4 * tol).sum())} sites beyond")
    assert_angles_close(got, want, tol=tol, what=what)


def plain_draw(gpu_ops, act, x0, n_or, n_hb, chain0=CHAIN0, sweep0=SWEEP0):
    x = dev(x0)
    gpu_ops.path_sweep_draw(act, x, torch.empty_like(x), n_or, n_hb, SEED, chain0, sweep0)
    return x


class options:
    """library options for the length of a with block, reset behind it whatever happens"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from mlmcpathintegral_amd import abi
        try:
            for k, v in self.kw.items():
                abi.set_option(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from mlmcpathintegral_amd import abi
        for k in self.kw:
            abi.set_option(k, "")


# ---- parity with the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", cases.PARITY, ids=[cases.case_id(s, c) for s, c in cases.PARITY])
def test_sweeps_match_oracle(gpu_ops, orc, shape, scale):
    """mlmcpi_path_sweep_draw against the oracle's sweeps, one at a time.  (The rows marked QoI are the plain draw here; the
    launch with the QoI's halo is compared with this draw bit for bit in test_draw_with_qoi.)

    Measured on an MI355X (worst angular difference over all shapes, bound 4 * HB_TOL): no site differs at O(1) -- no accept
    decision is a tie.  Step envelope (flat, mid, top): <= 5.2e-14 everywhere, heat-bath-only draws bit for bit: the angle
    is a linear function of random bits.  Wrapped Cauchy, one heat-bath sweep (bound 2e-10): over 2.4e-11, peaked 4.1e-11,
    sharp 1.2e-10; two sweeps (bound 1e-8): 8.7e-12.  There the worst site of a case is the draw with the smallest angle
    |theta| about the centre (1.9e-6 at the 1.2e-10; decided with the oracle alone): theta = acos(f) turns the one or two
    ulps by which f = cos(theta) differs (cos(pi u) of libm against the device's) into (2e-16) / theta.  That is the
    amplification of the header of tests/test_gpu_parity.py at the other end: not a flat conditional but a draw at the
    mode of a peaked one; HB_TOL[1] holds for |theta| >= 1.1e-6."""
    M, n_or, n_hb, _ = shape
    x0, _, _, want = cases.oracle_run(M, n_or, n_hb, scale)
    got = plain_draw(gpu_ops, make_action(scale, M), x0, n_or, n_hb).cpu().numpy()
    assert np.isfinite(got).all() and (got >= -np.pi - 1e-15).all() and (got <= np.pi + 1e-15).all()
    compare(got, want, HB_TOL[min(n_hb, 2)], f"parity {cases.case_id(shape, scale)}")


@pytest.mark.parametrize("M", cases.CLOSED_FORM_M + (1984, 1986))
def test_overrelaxation_only_draws_match_closed_form_and_oracle(gpu_ops, orc, M):
    """n_hb == 0: the closed form of 16 and of 3 sweeps against its statement in numpy (1e-13) and against the oracle's
    sweeps; with 16 sweeps M = 1984 is the full image (H2 = 1024) and 1986 the first length with two segments"""
    from closed_form import angle_diff, rotor_overrelax_closed_form
    act = make_action("mid", M)
    for K in (16, 3):
        x0, _, _, want = cases.oracle_run(M, K, 0, "mid")
        got = plain_draw(gpu_ops, act, x0, K, 0).cpu().numpy()
        compare(got, want, HB_TOL[0], f"overrelaxation M={M} K={K}")
        worst = max(float(angle_diff(got[b], rotor_overrelax_closed_form(x0[b], K)).max()) for b in range(B))
        print(f"[rotor] closed form M={M} K={K}: worst = {worst:.3e} (bound 1e-13)")
        assert worst <= 1e-13, (M, K, worst)


# ---- sweep by sweep with a heat-bath sweep behind it -------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n_or,n_hb,scale", cases.BLOCK)
def test_sweep_by_sweep_with_heat_bath_matches_oracle(gpu_ops, orc, M, n_or, n_hb, scale):
    """MLMCPI_OR_KERNEL=block: 7 + 1 is one launch of eight sweeps, 8 + 1 two launches (the cap of 8 is full), 9 + 2 is
    8, 1 + heat, heat; each equals the oracle, and MLMCPI_OR_HEAT=split on top changes no bit"""
    act = make_action(scale, M)
    x0, _, _, want = cases.oracle_run(M, n_or, n_hb, scale)
    with options(MLMCPI_OR_KERNEL="block"):
        block = plain_draw(gpu_ops, act, x0, n_or, n_hb)
    with options(MLMCPI_OR_KERNEL="block", MLMCPI_OR_HEAT="split"):
        split = plain_draw(gpu_ops, act, x0, n_or, n_hb)
    compare(block.cpu().numpy(), want, HB_TOL[min(n_hb, 2)], f"block M={M} ({n_or},{n_hb}) {scale}")
    assert bits_equal(block, split), (M, n_or, n_hb, scale)


@pytest.mark.parametrize("M,scale", cases.FUSED_SPLIT)
def test_heat_bath_behind_the_last_overrelaxation_launch_at_both_samplers(gpu_ops, M, scale):
    """what test_rotor_heat_bath_behind_the_last_overrelaxation_launch asserts at 2 m0 / a = 4, at the top of the step
    envelope and with the wrapped Cauchy, on the full image, on two segments and on a ring shorter than the halo"""
    act = make_action(scale, M)
    for n_or, n_hb in cases.FUSED_SPLIT_DRAWS:
        x0 = cases.start(M, n_or, n_hb, scale)
        with options(MLMCPI_OR_HEAT="split"):
            split = plain_draw(gpu_ops, act, x0, n_or, n_hb)
        with options(MLMCPI_OR_HEAT="fused"):
            fused = plain_draw(gpu_ops, act, x0, n_or, n_hb)
        assert bits_equal(split, fused), (M, scale, n_or, n_hb)


# ---- the draw with its QoI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", cases.QOI, ids=[cases.case_id(s, c) for s, c in cases.QOI])
def test_draw_with_qoi(gpu_ops, shape, scale):
    """mlmcpi_path_sweep_draw_qoi with w1 == src and with three buffers: the state is the plain draw's bit for bit, chi is
    mlmcpi_qoi_susceptibility of it and the long-double susceptibility of it to 1e-10, and nothing is written outside the
    work buffers and the B values of chi"""
    from mlmcpathintegral_amd import abi, ops
    M, n_or, n_hb, _ = shape
    act, T = make_action(scale, M), cases.params(scale, M)["T_final"]
    x0 = cases.start(M, n_or, n_hb, scale)
    plain = plain_draw(gpu_ops, act, x0, n_or, n_hb)
    chi_dev = gpu_ops.qoi_susceptibility(plain, T).cpu().numpy()
    chi_ld = ref.susceptibility(plain.cpu().numpy(), T)
    for distinct in (False, True):
        what = f"draw + QoI {cases.case_id(shape, scale)} ({'three buffers' if distinct else 'w1 is src'})"
        big = [guarded(B * M) for _ in range(3 if distinct else 2)]
        bufs = [b[1].view(B, M) for b in big]
        bufs[0].copy_(dev(x0))
        src, w0, w1 = bufs[0], bufs[1], bufs[2 if distinct else 0]
        qbig, q = guarded(B)
        where = C.c_int32(-5)
        abi.call("mlmcpi_path_sweep_draw_qoi", C.byref(act), ops._p(src), ops._p(w0), ops._p(w1), B, n_or, n_hb, SEED, CHAIN0, SWEEP0,
                 ops._p(q), None, C.byref(where), ops._stream())
        assert where.value in (0, 1)
        res = w0 if where.value == 0 else w1
        for bb in big:
            assert_bands_untouched(bb[0], B * M, what)
        assert_bands_untouched(qbig, B, what + " chi")
        assert bits_equal(res, plain), what
        if distinct:
            assert bits_equal(src, dev(x0)), what + ": the source is read only"
        assert_close(q.cpu().numpy(), chi_dev, tol=1e-10, what=what + " against mlmcpi_qoi_susceptibility")
        check_per_chain(q.cpu().numpy(), chi_ld, 1e-10, what)


# ---- the retry pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,scale", cases.POOL)
def test_heat_bath_sweeps_equal_site_updates_over_the_colour_classes(gpu_ops, orc, M, scale):
    """Two heat-bath sweeps on two segments of 513 and 512 cells per colour phase, at the top of the step envelope (about a
    fifth of a phase's cells go through the pool of 256) and just above it.  Which cells wait in the pool and which lane
    finishes them must not show: every sweep equals the site-at-a-time updates (one thread per chain, no pool) walked over
    the even sites, then the odd ones, with the sweep's step -- the contract
    test_site_updates_over_the_colour_classes_equal_a_sweep states for the 2-D actions, at its 1e-12.  (A longer ring holding
    the same chains is no alternative: the ring's length enters the neighbours of sites 0 and M - 1.)"""
    act = make_action(scale, M)
    x0, _, _, want = cases.oracle_run(M, 0, 2, scale)
    both = plain_draw(gpu_ops, act, x0, 0, 2)
    compare(both.cpu().numpy(), want, HB_TOL[2], f"pool M={M} (0,2) {scale}")
    order = torch.from_numpy(np.concatenate([np.arange(0, M, 2), np.arange(1, M, 2)]).astype(np.int32)).cuda()
    state = dev(x0)
    for s in range(2):
        swept = state.clone()
        gpu_ops.path_sweep_draw(act, swept, torch.empty_like(swept), 0, 1, SEED, CHAIN0, SWEEP0 + s)
        walked = state.clone()
        gpu_ops.path_site_updates(act, walked, order, True, SEED, CHAIN0, SWEEP0 + s)
        err = angle_err(swept.cpu().numpy(), walked.cpu().numpy())
        print(f"[rotor] sweep {s} against site updates M={M} {scale}: worst = {err.max():.3e} (bound 1e-12)")
        assert err.max() < 1e-12, (s, np.unravel_index(int(np.argmax(err)), err.shape))
        state = swept
    assert bits_equal(state, both), "two draws of one heat-bath sweep are the draw of two"


# ---- site-at-a-time updates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,scale", cases.SITE)
@pytest.mark.parametrize("heat", [False, True])
def test_site_updates_in_a_second_block(gpu_ops, orc, M, scale, heat):
    """rotor_site_update_kernel at B = 70: 64 threads per block, 6 live threads in the second; a list with repeats and with
    sites 0 and M - 1 next to each other, then the single-site form on site M - 1"""
    act = make_action(scale, M)
    x0, want = cases.site_run(M, scale, heat)
    big, x = guarded(cases.SITE_B * M)
    x = x.view(cases.SITE_B, M)
    x.copy_(dev(x0))
    sites = torch.from_numpy(cases.site_list(M).view(np.int32)).cuda()
    gpu_ops.path_site_updates(act, x, sites, heat, SEED, CHAIN0, 21)
    gpu_ops.path_site_updates(act, x, M - 1, heat, SEED, CHAIN0, 22)
    assert_bands_untouched(big, cases.SITE_B * M, "rotor_site_update_kernel")
    compare(x.cpu().numpy(), want, HB_TOL[2] if heat else 1e-12, f"site updates M={M} {scale} heat={heat}")


# ---- errors, not launches ----------------------------------------------------------------------------------------------------------
def test_more_chains_than_a_grid_takes_is_an_error(gpu_ops):
    """the chains are gridDim.y of rotor_sweep_kernel: 65536 of them are refused by name, with and without QoI, and the
    state is left alone"""
    from mlmcpathintegral_amd import abi
    n, M = cases.GRID_Y_MAX + 1, 2
    act = make_action("mid", M)
    x = torch.full((n, M), 0.5, dtype=torch.float64, device="cuda")
    w = torch.full((n, M), 0.25, dtype=torch.float64, device="cuda")
    with pytest.raises(abi.MlmcpiError, match="65535"):
        gpu_ops.path_sweep_draw(act, x, w, 1, 1, SEED, 0, 0)
    with pytest.raises(abi.MlmcpiError, match="65535"):
        gpu_ops.path_sweep_draw_qoi(act, x, w, x, 0, 1, SEED, 0, 0)
    assert bool((x == 0.5).all()) and bool((w == 0.25).all())
    ok = x[:cases.GRID_Y_MAX].contiguous()
    gpu_ops.path_sweep_draw(act, ok, torch.empty_like(ok), 1, 1, SEED, 0, 0)   # the limit itself is a launch
    assert bool(torch.isfinite(ok).all()) and not bool((ok == 0.5).all())
