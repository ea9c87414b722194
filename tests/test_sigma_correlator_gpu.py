"""GPU: the time-slice correlators of the O(3) sigma model on the levels of its CoarsenRotate hierarchy
(mlmcpi_sigma_level_correlator, sigma_correlator.hip) against the long-double reference (tests/sigma_correlator_reference.py),
the sum identity against the device's own chi_m, bit identity over the batch split and the accumulation, the accumulated sums,
the refusals, the law on the 2 x 2 lattice and between two samplers at 16 x 16, and host/driver --correlator 1."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sigma_correlator_reference as ref
from conftest import zcheck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_EXTENT = 2048     # kCorrLdsExtent of sigma_correlator.hip: the correlator pass keeps the slice sums of a longer extent in
                      # global memory; (2048, 2) is the last level on the LDS path, (2050, 2) and (2, 2050) the first beyond it
# (Mt, Mx, chains): B = 300 up to (130, 70), so that the chain index runs past one of anything
SHAPES = [(2, 2, 300), (4, 2, 300), (2, 6, 300), (6, 4, 300), (16, 16, 300), (66, 34, 300), (130, 70, 300), (520, 20, 3), (20, 520, 3),
          (260, 260, 3), (1024, 1024, 2), (8192, 2, 2), (LDS_EXTENT, 2, 2), (LDS_EXTENT + 2, 2, 2), (2, LDS_EXTENT + 2, 2)]
CASES = [(Mt, Mx, B, rot, field) for Mt, Mx, B in SHAPES for rot in (0, 1) for field in ("hot", "planted")]
_cache = {}


def _level(Mt, Mx, rot, beta=1.0):
    from mlmcpathintegral_amd import abi
    return abi.sigma_level(Mt, Mx, rot, beta)


def _case(ops, Mt, Mx, B, rot, field):
    """state, device correlators and the reference of a case, computed once and shared by the tests that need them"""
    key = (Mt, Mx, B, rot, field)
    if key not in _cache:
        lv = _level(Mt, Mx, rot)
        if field == "hot":
            x = ops.sigma_level_initialise(lv, B, 1000 + Mt + 3 * Mx + rot)
        else:
            x = torch.from_numpy(ref.planted(Mt, Mx, rot, B, 7 + Mt + Mx + rot)).cuda()
        out = ops.sigma_level_correlator(lv, x)
        _cache[key] = (lv, x, out, ref.correlator(Mt, Mx, rot, x.cpu().numpy()))
    return _cache[key]


@pytest.mark.parametrize("Mt,Mx,B,rot,field", CASES)
def test_parity_with_the_long_double_reference(gpu_ops, Mt, Mx, B, rot, field):
    lv, x, out, want = _case(gpu_ops, Mt, Mx, B, rot, field)
    assert out.shape == (B, ref.n_out(Mt, Mx)) == (B, gpu_ops.sigma_level_correlator_size(lv))
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    tol = ref.tolerance(Mt, Mx, rot)
    print(f"({Mt}, {Mx}) rot {rot} {field}: max |C - ref| / bound = {np.max(err / tol):.3g}, max |C| = {np.max(np.abs(got)):.4g}")
    assert np.all(err <= tol), (np.max(err / tol), np.unravel_index(np.argmax(err / tol), err.shape))
    if field == "planted" and Mt >= 4 and Mx >= 4:   # the planted field tells the directions and the lags apart
        Ct, Cx = ref.split(want[0].astype(np.float64), Mt, Mx)
        assert abs(Ct[1] - Cx[1]) > 1e-3 * abs(Ct[0])


@pytest.mark.parametrize("Mt,Mx,B,rot,field", CASES)
def test_sum_identity_against_the_device_susceptibility(gpu_ops, Mt, Mx, B, rot, field):
    lv, x, out, _ = _case(gpu_ops, Mt, Mx, B, rot, field)
    chi = gpu_ops.sigma_level_magnetic_susceptibility(lv, x).cpu().numpy()
    Ct, Cx = ref.split(out.cpu().numpy().astype(np.longdouble), Mt, Mx)   # the weighted sum itself in long double: no error of its own
    tol = ref.tolerance(Mt, Mx, rot)
    for C_d, M, t in ((Ct, Mt, tol[0]), (Cx, Mx, tol[-1])):
        d = np.abs(ref.susceptibility(C_d, M) - chi).astype(np.float64)
        print(f"({Mt}, {Mx}) rot {rot} {field} M = {M}: max |sum w C - chi_m| / bound = {np.max(d) / t:.3g}")
        assert np.all(d <= t), np.max(d) / t


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, 0), (6, 4, 1), (66, 34, 0), (66, 34, 1), (520, 20, 0), (20, 520, 1), (260, 260, 1),
                                       (LDS_EXTENT + 2, 2, 0), (2, LDS_EXTENT + 2, 1)])
def test_bit_identity_over_the_batch_split_and_the_accumulation(gpu_ops, Mt, Mx, rot):
    lv = _level(Mt, Mx, rot)
    x = torch.from_numpy(ref.planted(Mt, Mx, rot, 7, 99)).cuda()
    whole = gpu_ops.sigma_level_correlator(lv, x)
    single = torch.cat([gpu_ops.sigma_level_correlator(lv, x[b:b + 1].contiguous()) for b in range(7)])
    assert torch.equal(whole, single)
    acc = torch.zeros(7, whole.shape[1], 2, dtype=torch.float64, device="cuda")
    assert torch.equal(gpu_ops.sigma_level_correlator(lv, x, acc=acc), whole)
    assert torch.equal(acc[..., 0], whole) and torch.equal(acc[..., 1], whole * whole)


GUARD, SENTINEL = 256, -12345.0   # doubles before and after every buffer (2 KiB: the workspace stays 256-byte aligned)


def _guarded(n):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return buf, C.c_void_p(buf.data_ptr() + 8 * GUARD)


def _untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, 1), (66, 34, 0), (130, 70, 1), (LDS_EXTENT + 2, 2, 0)])
def test_accumulation_and_guard_bands(gpu_ops, Mt, Mx, rot):
    from mlmcpathintegral_amd import abi
    lv, B = _level(Mt, Mx, rot), 5
    n_out = gpu_ops.sigma_level_correlator_size(lv)
    nbytes = C.c_size_t(0)
    abi.call("mlmcpi_sigma_level_correlator_workspace_bytes", C.byref(lv), B, C.byref(nbytes))
    assert nbytes.value % 8 == 0
    out_buf, p_out = _guarded(B * n_out)
    acc_buf, p_acc = _guarded(2 * B * n_out)
    work_buf, p_work = _guarded(nbytes.value // 8)
    acc_buf[GUARD:GUARD + 2 * B * n_out] = 0.0
    s1 = torch.zeros(B, n_out, dtype=torch.float64, device="cuda")
    s2 = torch.zeros_like(s1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in range(3):
        x = gpu_ops.sigma_level_initialise(lv, B, 50 + k)
        abi.call("mlmcpi_sigma_level_correlator", C.byref(lv), C.c_void_p(x.data_ptr()), B, p_out, p_acc, p_work, nbytes.value, stream)
        out = out_buf[GUARD:GUARD + B * n_out].reshape(B, n_out).clone()
        assert torch.equal(out, gpu_ops.sigma_level_correlator(lv, x))
        s1 += out
        s2 += out * out
    acc = acc_buf[GUARD:GUARD + 2 * B * n_out].reshape(B, n_out, 2)
    assert torch.equal(acc[..., 0], s1) and torch.equal(acc[..., 1], s2)
    assert _untouched(out_buf, B * n_out) and _untouched(acc_buf, 2 * B * n_out) and _untouched(work_buf, nbytes.value // 8)


def test_refusals_launch_nothing(gpu_ops):
    from mlmcpathintegral_amd import abi
    lv, B = _level(8, 8, 0), 2
    n_out = gpu_ops.sigma_level_correlator_size(lv)
    x = gpu_ops.sigma_level_initialise(lv, B, 1)
    work = gpu_ops.sigma_level_correlator_workspace(lv, B)
    out = torch.full((B, n_out), SENTINEL, dtype=torch.float64, device="cuda")
    px, po, pw = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr())
    status = "status -1"   # MLMCPI_ERR_INVALID
    for bad in ((7, 8), (8, 7), (0, 8), (8, 0)):
        for rot in (0, 1):
            with pytest.raises(abi.MlmcpiError, match="even extents") as e:
                abi.call("mlmcpi_sigma_level_correlator", C.byref(_level(*bad, rot)), px, B, po, None, pw, work.numel(), None)
            assert status in str(e.value)
            with pytest.raises(abi.MlmcpiError, match="even extents"):
                abi.call("mlmcpi_sigma_level_correlator_size", C.byref(_level(*bad, rot)), C.byref(C.c_uint32(0)))
            with pytest.raises(abi.MlmcpiError, match="even extents"):
                abi.call("mlmcpi_sigma_level_correlator_workspace_bytes", C.byref(_level(*bad, rot)), B, C.byref(C.c_size_t(0)))
    for args in ((None, px, B, po, None, pw, work.numel(), None), (C.byref(lv), None, B, po, None, pw, work.numel(), None),
                 (C.byref(lv), px, B, None, None, pw, work.numel(), None), (C.byref(lv), px, B, po, None, None, work.numel(), None)):
        with pytest.raises(abi.MlmcpiError, match=status):
            abi.call("mlmcpi_sigma_level_correlator", *args)
    with pytest.raises(abi.MlmcpiError, match="workspace is too small") as e:
        abi.call("mlmcpi_sigma_level_correlator", C.byref(lv), px, B, po, None, pw, work.numel() - 1, None)
    assert status in str(e.value)
    for big in (0, 65536):   # the launch geometry takes 1 .. 65535 chains (mlmcpi_hip.h): refused, never a truncated grid
        with pytest.raises(abi.MlmcpiError, match="65535 chains") as e:
            abi.call("mlmcpi_sigma_level_correlator", C.byref(lv), px, big, po, None, pw, work.numel(), None)
        assert status in str(e.value)
        with pytest.raises(abi.MlmcpiError, match=status):
            abi.call("mlmcpi_sigma_level_correlator_workspace_bytes", C.byref(lv), big, C.byref(C.c_size_t(0)))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def _chain_estimate(acc, n):
    """mean and chain-spread error per entry from the accumulated sums [B, n_out, 2] of n calls; the per-chain means as well"""
    means = (acc[..., 0] / n).cpu().numpy()
    return means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(means.shape[0]), means


def _xi_jackknife(means, M, lo, hi):
    """xi_2 of the mean correlator means[:, lo:hi] and its jackknife error over the chains (the arithmetic of SigmaCorrelator::xi)"""
    B, tot = means.shape[0], means[:, lo:hi].sum(axis=0)
    xi = ref.xi_second_moment(tot / B, M)
    leave = np.array([ref.xi_second_moment((tot - means[b, lo:hi]) / (B - 1), M) for b in range(B)])
    return float(xi), float(np.sqrt((B - 1) / B * np.sum((leave - leave.mean()) ** 2)))


def test_law_on_the_two_by_two_lattice(gpu_ops):
    """2 x 2, beta = 1, heat-bath draws of 10 + 1 sweeps, 4096 chains, 300 draws after 20 of burn-in, against C_t(0) = 1 + c1,
    C_t(1) = C_x(1) = c1 + c2 of the four-spin ring; chain-spread z-scores, gate 4.5 (profiles/sigma_correlator_zscores.json)"""
    lv, B, seed, n = _level(2, 2, 0, 1.0), 4096, 31, 300
    c1, c2 = ref.ring_c1_c2(1.0)
    x = gpu_ops.sigma_level_initialise(lv, B, seed)
    w = torch.empty_like(x)
    acc = torch.zeros(B, 4, 2, dtype=torch.float64, device="cuda")
    work = gpu_ops.sigma_level_correlator_workspace(lv, B)
    for d in range(20 + n):
        gpu_ops.sigma_level_sweep_draw(lv, x, w, 10, 1, seed, 0, 11 * d)
        if d >= 20:
            gpu_ops.sigma_level_correlator(lv, x, acc=acc, work=work)
    mean, err, _ = _chain_estimate(acc, n)
    for name, k, exact in (("C_t(0)", 0, 1.0 + c1), ("C_t(1)", 1, c1 + c2), ("C_x(1)", 3, c1 + c2)):
        zcheck(f"sigma correlator 2x2 beta=1 heat bath {name} vs ring", float(mean[k]), float(err[k]), exact, gate=4.5)


def test_law_swendsen_wang_against_heat_bath(gpu_ops):
    """16 x 16, beta = 1.5, 1024 chains each: 200 heat-bath draws of 10 + 1 sweeps after 50, and 200 draws of 2 Swendsen-Wang
    updates after 100 updates; the mean correlators agree at every lag, and xi_2 within its jackknife errors (gate 4.5)"""
    M, B, n = 16, 1024, 200
    lv = _level(M, M, 0, 1.5)
    n_out = gpu_ops.sigma_level_correlator_size(lv)
    work = gpu_ops.sigma_level_correlator_workspace(lv, B)
    est = {}
    x = gpu_ops.sigma_level_initialise(lv, B, 5)
    w = torch.empty_like(x)
    acc = torch.zeros(B, n_out, 2, dtype=torch.float64, device="cuda")
    for d in range(50 + n):
        gpu_ops.sigma_level_sweep_draw(lv, x, w, 10, 1, 5, 0, 11 * d)
        if d >= 50:
            gpu_ops.sigma_level_correlator(lv, x, acc=acc, work=work)
    est["hb"] = _chain_estimate(acc, n)
    x = gpu_ops.sigma_level_initialise(lv, B, 6)
    sw_work = gpu_ops.sigma_level_sw_workspace(lv, B)
    acc = torch.zeros(B, n_out, 2, dtype=torch.float64, device="cuda")
    gpu_ops.sigma_level_sw_draw(lv, x, 100, 6, 0, 0, outputs=False, work=sw_work)
    for d in range(n):
        gpu_ops.sigma_level_sw_draw(lv, x, 2, 6, 0, 100 + 2 * d, outputs=False, work=sw_work)
        gpu_ops.sigma_level_correlator(lv, x, acc=acc, work=work)
    est["sw"] = _chain_estimate(acc, n)
    for k in range(n_out):
        name = f"C_t({k})" if k <= M // 2 else f"C_x({k - M // 2 - 1})"
        zcheck(f"sigma correlator 16x16 beta=1.5 {name} Swendsen-Wang vs heat bath", float(est["sw"][0][k]), float(est["sw"][1][k]),
               float(est["hb"][0][k]), float(est["hb"][1][k]), gate=4.5)
    for d, (lo, hi) in enumerate(((0, M // 2 + 1), (M // 2 + 1, n_out))):
        xs, es = _xi_jackknife(est["sw"][2], M, lo, hi)
        xh, eh = _xi_jackknife(est["hb"][2], M, lo, hi)
        zcheck(f"sigma correlator 16x16 beta=1.5 xi_2 ({'tx'[d]}) Swendsen-Wang vs heat bath", xs, es, xh, eh, gate=4.5)


DRIVER = ["--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.5", "--sampler", "swendsenwang", "--n_updates", "1", "--n_samples", "500"]


def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def test_driver_prints_the_correlator_and_xi(gpu_ops):
    r = _driver(*DRIVER, "--batch", "64", "--correlator", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-3000:])
    lags = re.findall(r"^ C\(tau = (\d+)\): C_t = (\S+) \+/- (\S+) C_x = (\S+) \+/- (\S+) avg = (\S+) \+/- (\S+)$", r.stdout, re.M)
    assert [int(l[0]) for l in lags] == list(range(16 // 2 + 1))
    xi = re.findall(r"^ xi_2 \((t|x)\) = (\S+) \+/- (\S+) \(jackknife over chains\), xi_2 / M = (\S+)$", r.stdout, re.M)
    assert [d for d, *_ in xi] == ["t", "x"] and all(0.0 < float(v) < 16.0 and float(e) > 0.0 for _, v, e, _ in xi)
    q = re.search(r"Q: Avg \+/- Err = (\S+) \+/- ", r.stdout)
    chi = re.search(r"^ chi from C_t = (\S+), from C_x = (\S+)$", r.stdout, re.M)
    assert q and chi and chi.group(1) == chi.group(2) == q.group(1), (q and q.group(1), chi and chi.groups())
    assert re.search(r"^ F_t = \S+, F_x = \S+$", r.stdout, re.M)


def test_driver_without_the_option_prints_none_of_it(gpu_ops):
    r = _driver(*DRIVER, "--correlator", "0")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Single level MC" in r.stdout
    assert "C(tau" not in r.stdout and "xi_2" not in r.stdout and "correlator" not in r.stdout
