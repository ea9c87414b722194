"""GPU: mlmcpi_path_correlator against the long-double definition (tests/path_correlator_reference.py) at every launch
geometry, its determinism contract bit for bit, the accumulator, the refusals, and the law of <C(tau)> against the closed
forms of the periodic lattice (harmonic oscillator with the exact sampler, rotor with the overrelaxed heat bath).

Largest observed |error| / bound of the parity test: see DESIGN.md 4.2a.  The records of one run are
profiles/path_correlator_zscores.json (this module writes the z-scores and the parity ratios into the directory
MLMCPI_PATH_CORRELATOR_RECORDS names, if the variable is set)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import path_correlator_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
RECORDS = os.environ.get("MLMCPI_PATH_CORRELATOR_RECORDS")


def _act(kind, M, T_final=4.0, m0=1.0):
    from mlmcpathintegral_amd import abi
    return abi.path_action(kind, M, T_final, m0, 1.0, 1.0 if kind == 1 else 0.0, 0.0)


def _segmented_M(kind):
    """the shortest multiple of 100 whose plan at n_lag = 64 reports three segments or more"""
    M = 200
    while ref.plan(kind, M, 64, 2)[1]["nseg"] < 3:
        M += 100
    return M


def _shapes(kind):
    cap = ref.lag_cap(kind)
    return [(2, 2, 3), (7, 4, 5), (64, 33, 3), (128, 65, 300), (130, 66, 70), (1026, 514, 3), (4100, 17, 300), (_segmented_M(kind), 64, 2),
            (2 * (cap - 1), cap, 1), (8, 5, 70000)]


CASES = [(k, *s) for k in (0, 2) for s in _shapes(k)] + [(1, 130, 66, 70)]


def _inputs(kind, M, n_lag, B):
    """random paths, the spike path of the two ends, and spikes on every segment boundary the plan reports"""
    rng = np.random.default_rng(1000 * kind + M + n_lag)
    x = rng.uniform(-4 * np.pi, 4 * np.pi, (B, M)) if kind == ref.ROTOR else rng.standard_normal((B, M))
    amp = rng.uniform(0.5, 2.0, (min(B, 3), 4))
    ends = np.zeros((min(B, 3), M))
    ends[:, 0], ends[:, M - 1] = amp[:, 0], -amp[:, 1]
    p = ref.plan(kind, M, n_lag, B)[1]
    edges = np.zeros((min(B, 3), M))
    for s in range(p["nseg"]):
        edges[:, s * p["owned"]] = amp[:, 2] + s
        edges[:, (s * p["owned"] - 1) % M] = -amp[:, 3] - s
    return {"random": x, "ends": ends, "edges": edges}


RATIOS = {}


@pytest.mark.parametrize("kind,M,n_lag,B", CASES, ids=lambda v: str(v))
def test_parity_with_the_long_double_reference(gpu_ops, kind, M, n_lag, B):
    import torch
    from mlmcpathintegral_amd import ops
    act = _act(kind, M)
    rc, p = ref.plan(kind, M, n_lag, B)
    assert rc == 0 and ops.path_correlator_plan(act, n_lag, B) == p
    worst = 0.0
    for name, x in _inputs(kind, M, n_lag, B).items():
        got = ops.path_correlator(act, torch.from_numpy(x).cuda(), n_lag).cpu().numpy()
        want, bound = ref.correlator_and_bound(kind, x, n_lag)
        err = np.abs((got - want).astype(np.float64))
        assert got.shape == (x.shape[0], n_lag) and np.isfinite(got).all()
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
        print(f"[path correlator] kind {kind} M {M} n_lag {n_lag} B {B} {name}: nseg {p['nseg']} chains/wg {p['chains_per_workgroup']} "
              f"group {p['group']}: max |err| {err.max():.3e}, max err / bound {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    RATIOS[(kind, M, n_lag, B)] = worst
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        with open(os.path.join(RECORDS, "path_correlator_parity.json"), "w") as f:
            json.dump({"max_ratio_to_bound": max(RATIOS.values()), "cases": [{"case": list(k), "ratio": v} for k, v in RATIOS.items()]}, f, indent=1)


def test_the_case_list_reaches_every_geometry():
    plans = [ref.plan(*c)[1] for c in CASES]
    assert {(p["nseg"] > 1, p["chains_per_workgroup"]) for p in plans} == {(False, 4), (False, 1), (True, 1)}
    assert {p["group"] for p in plans} >= {1, 8, 16, 32, 64}
    assert max(p["nseg"] for p in plans) >= 3 and any(p["image_tiles"] - p["lag_tiles"] == 1 and p["nseg"] > 1 for p in plans)


@pytest.mark.parametrize("kind,M,n_lag", [(0, 128, 65), (2, 130, 66), (0, 9000, 64), (2, 4100, 17)])
def test_bit_identity_over_batch_split_and_stream(gpu_ops, kind, M, n_lag):
    import torch
    from mlmcpathintegral_amd import ops
    act = _act(kind, M)
    rng = np.random.default_rng(77 + M)
    x = torch.from_numpy(rng.standard_normal((300, M)) * (4.0 if kind == 2 else 1.0)).cuda()
    whole = ops.path_correlator(act, x, n_lag)
    assert torch.equal(ops.path_correlator(act, x[:70].contiguous(), n_lag)[5], ops.path_correlator(act, x[5:6].contiguous(), n_lag)[0])
    assert torch.equal(whole[5], ops.path_correlator(act, x[5:6].contiguous(), n_lag)[0])
    for cut in (1, 150):
        parts = torch.cat([ops.path_correlator(act, x[:cut].contiguous(), n_lag), ops.path_correlator(act, x[cut:].contiguous(), n_lag)])
        assert torch.equal(whole, parts), cut
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.path_correlator(act, x, n_lag)
    side.synchronize()
    assert torch.equal(whole, other)


def _guarded(n, fill=float("nan"), pad=64):
    """a tensor of n doubles between two bands of NaN: (whole buffer, the view)"""
    import torch
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[pad:pad + n]
    view.fill_(fill)
    return buf, view


def _bands_intact(buf, n, pad=64):
    import torch
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())


@pytest.mark.parametrize("kind,M,n_lag,B", [(0, 128, 65, 7), (2, 9000, 64, 3)])
def test_accumulator_and_guard_bands(gpu_ops, kind, M, n_lag, B):
    import torch
    from mlmcpathintegral_amd import abi, ops
    act = _act(kind, M)
    nbytes = C.c_size_t(0)
    abi.call("mlmcpi_path_correlator_workspace_bytes", C.byref(act), n_lag, B, C.byref(nbytes))
    assert nbytes.value % 8 == 0 and nbytes.value == ref.plan(kind, M, n_lag, B)[1]["work_bytes"]
    # the workspace is 256-byte aligned inside its guard: pad by 64 doubles from torch's 512-byte aligned allocation
    wbuf, work = _guarded(nbytes.value // 8)
    obuf, out = _guarded(B * n_lag)
    abuf, acc = _guarded(B * n_lag * 2, fill=0.0)
    assert work.data_ptr() % 256 == 0
    rng = np.random.default_rng(5)
    outs = []
    for k in range(3):
        x = torch.from_numpy(rng.standard_normal((B, M))).cuda()
        abi.call("mlmcpi_path_correlator", C.byref(act), C.c_void_p(x.data_ptr()), B, n_lag, C.c_void_p(out.data_ptr()), C.c_void_p(acc.data_ptr()),
                 C.c_void_p(work.data_ptr()), nbytes.value, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        outs.append(out.clone().reshape(B, n_lag))
        assert torch.equal(outs[-1], ops.path_correlator(act, x, n_lag))     # acc = None changes nothing else
    torch.cuda.synchronize()
    assert _bands_intact(wbuf, nbytes.value // 8) and _bands_intact(obuf, B * n_lag) and _bands_intact(abuf, B * n_lag * 2)
    a = acc.reshape(B, n_lag, 2).cpu().numpy()
    o = np.stack([t.cpu().numpy() for t in outs])
    eps = 2.0 ** -52
    assert np.all(np.abs(a[..., 0] - o.sum(axis=0)) <= 4 * eps * np.abs(o).sum(axis=0))
    assert np.all(np.abs(a[..., 1] - (o * o).sum(axis=0)) <= 4 * eps * (o * o).sum(axis=0))
    assert np.all(a[..., 1] > 0)


def test_refusals_touch_nothing(gpu_ops):
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    M, n_lag, B = 64, 33, 3
    act = _act(0, M)
    x = torch.zeros((B, M), dtype=torch.float64, device="cuda")
    out = torch.full((B * n_lag,), SENTINEL, dtype=torch.float64, device="cuda")
    acc = torch.full((B * n_lag * 2,), SENTINEL, dtype=torch.float64, device="cuda")
    work = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    pa = C.byref(act)

    def bad_action(kind, m):
        a = _act(0, M)
        a.kind, a.M = kind, m
        return C.byref(a)

    seg = _act(0, 9000)   # a segmented path needs B nseg n_lag doubles of workspace
    need = C.c_size_t(0)
    assert lib.mlmcpi_path_correlator_workspace_bytes(C.byref(seg), 64, 2, C.byref(need)) == 0 and need.value > 512
    xs = torch.zeros((2, 9000), dtype=torch.float64, device="cuda")
    calls = {
        "NULL act": (None, P(x), B, n_lag, P(out), P(acc), P(work), 512, None),
        "NULL d_x": (pa, None, B, n_lag, P(out), P(acc), P(work), 512, None),
        "NULL d_out": (pa, P(x), B, n_lag, None, P(acc), P(work), 512, None),
        "NULL d_work": (pa, P(x), B, n_lag, P(out), P(acc), None, 512, None),
        "kind -1": (bad_action(-1, M), P(x), B, n_lag, P(out), P(acc), P(work), 512, None),
        "kind 3": (bad_action(3, M), P(x), B, n_lag, P(out), P(acc), P(work), 512, None),
        "M = 0": (bad_action(0, 0), P(x), B, 1, P(out), P(acc), P(work), 512, None),
        "B = 0": (pa, P(x), 0, n_lag, P(out), P(acc), P(work), 512, None),
        "n_lag = 0": (pa, P(x), B, 0, P(out), P(acc), P(work), 512, None),
        "n_lag > M/2 + 1": (pa, P(x), B, n_lag + 1, P(out), P(acc), P(work), 512, None),
        "work_bytes too small": (pa, P(x), B, n_lag, P(out), P(acc), P(work), 255, None),
        "work_bytes too small, segmented": (C.byref(seg), P(xs), 2, 64, P(out), P(acc), P(work), need.value - 1, None),
    }
    for name, args in calls.items():
        assert lib.mlmcpi_path_correlator(*args) == ref.ERR_INVALID, name
        assert lib.mlmcpi_last_error(), name
    torch.cuda.synchronize()
    for t in (out, acc, work):
        assert bool((t == SENTINEL).all())
    # beyond the cap: MLMCPI_ERR_UNSUPPORTED, nothing touched either
    cap = ref.lag_cap(2)
    big = _act(2, 2 * cap)
    xb = torch.zeros((1, 2 * cap), dtype=torch.float64, device="cuda")
    assert lib.mlmcpi_path_correlator(C.byref(big), P(xb), 1, cap + 1, P(out), P(acc), P(work), 512, None) == ref.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((acc == SENTINEL).all())
    assert lib.mlmcpi_path_correlator(pa, P(x), B, n_lag, P(out), P(acc), P(work), 512, None) == 0   # and the same call, valid


def _law(name, mean, err, exact):
    z = (mean - exact) / err
    print(f"[path correlator law] {name}: z = {np.array2string(z, precision=2)}")
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        path = os.path.join(RECORDS, "path_correlator_zscores.json")
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = {"mean": mean.tolist(), "error": err.tolist(), "exact": exact.tolist(), "z": z.tolist(), "gate": 4.5}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
    assert float(np.max(np.abs(z))) < 4.5, z


def test_law_harmonic_oscillator(gpu_ops):
    """M = 16, T_final = 4, m0 = mu2 = 1, exact sampler (independent draws), 4096 chains x 20 draws through acc: the mean of C(tau)
    over chains against the closed form at all 9 lags, error = spread of the per-chain means"""
    import torch
    from mlmcpathintegral_amd import ops
    act, B, n_lag, n = _act(0, 16), 4096, 9, 20
    sampler = ops.HOExactSampler(act, B, seed=20261)
    acc = torch.zeros((B, n_lag, 2), dtype=torch.float64, device="cuda")
    work = ops.path_correlator_workspace(act, n_lag, B)
    x = None
    for _ in range(n):
        x = sampler.draw(x)
        ops.path_correlator(act, x, n_lag, acc=acc, work=work)
    means = (acc[:, :, 0] / n).cpu().numpy()
    _law("harmonic", means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(B), ref.ho_exact(16, 4.0, 1.0, 1.0, np.arange(n_lag)))


def test_law_rotor(gpu_ops):
    """M = 16, T_final = 4, m0 = 0.25 (kappa = m0 / a = 1), draws of 1 overrelaxation + 1 heat-bath sweep: 100 of burn-in, 200
    measured, 4096 chains, against the character expansion at all 9 lags"""
    import torch
    from mlmcpathintegral_amd import ops
    act, B, n_lag, seed = _act(2, 16, 4.0, 0.25), 4096, 9, 20262
    x = ops.path_initialise(act, B, seed)
    scratch = torch.empty_like(x)
    acc = torch.zeros((B, n_lag, 2), dtype=torch.float64, device="cuda")
    work = ops.path_correlator_workspace(act, n_lag, B)
    for d in range(300):
        ops.path_sweep_draw(act, x, scratch, 1, 1, seed, 0, 2 * d)
        if d >= 100:
            ops.path_correlator(act, x, n_lag, acc=acc, work=work)
    means = (acc[:, :, 0] / 200).cpu().numpy()
    err = means.std(axis=0, ddof=1) / np.sqrt(B)
    # lag 0 is the identity C(0) = 1, not a measurement: its spread is rounding, and its error the kernel's fp64 bound
    err[0] = max(err[0], (2 * (16 + 4) + 16) * ref.EPS)
    _law("rotor", means.mean(axis=0), err, ref.rotor_exact(16, 1.0, np.arange(n_lag)))
