"""GPU: mlmcpi_schwinger_wilson_loops against the long-double definition (tests/wilson_loops_reference.py) at every tile
geometry, single-link spikes on every tile boundary, the identities, its determinism contract bit for bit, the accumulator, the
refusals, and the law of <W(r, s)> against the exact series of the periodic lattice (overrelaxed heat bath at beta = 2, cluster
sampler at beta = 4).

Bound of the parity test, absolute and per entry: (24 r s + c_sum) eps, c_sum = (J + 6 + 4 + tiles + 2) / 2 from the summation
order built (derivation beside wilson_loops_reference.bound).  Largest observed |error| / bound: see DESIGN.md 4.1d.  The records
of one run are profiles/wilson_loops_zscores.json (this module writes the z-scores and the parity ratios into the directory
MLMCPI_WILSON_LOOPS_RECORDS names, if the variable is set)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import wilson_loops_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
RECORDS = os.environ.get("MLMCPI_WILSON_LOOPS_RECORDS")
TW, TH = ref.TILE, ref.TILE   # what the plan reports (asserted in every parity case)

# (Mt, Mx, R, S, B)
CASES = [(2, 2, 2, 2, 3), (2, 6, 2, 3, 3), (17, 9, 9, 9, 3), (17, 9, 9, 9, 70), (TW - 1, TH + 1, 16, 16, 3), (TW + 1, TH - 1, 16, 1, 3),
         (66, 34, 16, 16, 3), (130, 70, 7, 16, 3)]


def _theta(Mt, Mx, B, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, (B, 2 * Mt * Mx))


REFERENCE = {}


def _reference(case):
    """the random links of a case and their long-double W, computed once and shared"""
    if case not in REFERENCE:
        Mt, Mx, R, S, B = case
        th = _theta(Mt, Mx, B, 31 * Mt + Mx + R + S)
        W = ref.wilson_loops(th, Mt, Mx, R, S)
        th.setflags(write=False)
        W.setflags(write=False)
        REFERENCE[case] = (th, W)
    return REFERENCE[case]


def _record(name, payload):
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        path = os.path.join(RECORDS, "wilson_loops_zscores.json")
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = payload
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


RATIOS = {}


@pytest.mark.parametrize("case", CASES, ids=lambda v: "x".join(map(str, v)))
def test_parity_with_the_long_double_reference(gpu_ops, case):
    import torch
    from mlmcpathintegral_amd import ops
    Mt, Mx, R, S, B = case
    rc, p = ref.plan(Mt, Mx, R, S, B)
    assert rc == 0 and ops.wilson_loops_plan(Mt, Mx, R, S, B) == p and (p["tile_w"], p["tile_h"]) == (TW, TH)
    th, want = _reference(case)
    got = ops.wilson_loops(torch.tensor(th).cuda(), Mt, Mx, R, S).cpu().numpy()
    assert got.shape == (B, R, S) and np.isfinite(got).all()
    err = np.abs((got - want).astype(np.float64))
    ratio = float(np.max(err / ref.bound(p, R, S)[None]))
    print(f"[wilson loops] {Mt} x {Mx}, R {R} S {S} B {B}: tiles {p['tiles_w']} x {p['tiles_h']}, c_sum {ref.c_sum(p)}: "
          f"max |err| {err.max():.3e}, max err / bound {ratio:.4f}")
    RATIOS["x".join(map(str, case))] = ratio
    _record("parity", {"max_ratio_to_bound": max(RATIOS.values()), "cases": dict(RATIOS)})
    assert ratio <= 1.0, ratio


def test_the_case_list_reaches_every_geometry():
    plans = [ref.plan(*c)[1] for c in CASES]
    assert {(p["tiles_w"] > 1, p["tiles_h"] > 1) for p in plans} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(p["tiles_w"] >= 3 and p["tiles_h"] >= 3 for p in plans)                      # interior and edge tiles both ways
    assert {c[3] for c in CASES} >= {1, 2, 3, 9, 16} and any(c[0] % 2 and c[1] % 2 for c in CASES)
    assert any(c[2] == c[0] and c[3] == c[1] for c in CASES) and max(c[4] for c in CASES) > 64


def test_single_link_spikes_on_every_tile_boundary(gpu_ops):
    """a zero field with one link set to alpha, one chain per spike: W(r, s) = 1 - (2 r / V)(1 - cos alpha) for a theta0 link,
    2 s for a theta1 link (r < Mt, s < Mx), on both sides of every tile boundary, first and last row and column, the corners"""
    import torch
    from mlmcpathintegral_amd import ops
    Mt, Mx, R, S, alpha = 2 * TW + 2, TH + 2, 5, 4, 0.7
    p = ref.plan(Mt, Mx, R, S, 1)[1]
    cols = sorted({0, Mt - 1} | {e for r in ref.tile_ranges(p, Mt, Mx) for e in (r[0], (r[0] - 1) % Mt)})
    rows = sorted({0, Mx - 1} | {e for r in ref.tile_ranges(p, Mt, Mx) for e in (r[2], (r[2] - 1) % Mx)})
    assert cols == [0, TW - 1, TW, 2 * TW - 1, 2 * TW, Mt - 1] and rows == [0, TH - 1, TH, Mx - 1]
    spikes = [(i, j, mu) for j in rows for i in cols for mu in (0, 1)]
    th = np.zeros((len(spikes), Mx, Mt, 2))
    for b, (i, j, mu) in enumerate(spikes):
        th[b, j, i, mu] = alpha
    th = th.reshape(len(spikes), -1)
    got = ops.wilson_loops(torch.from_numpy(th).cuda(), Mt, Mx, R, S).cpu().numpy()
    r, s = np.arange(1, R + 1)[:, None], np.arange(1, S + 1)[None, :]
    closed = {0: 1 - 2 * r / (Mt * Mx) * (1 - np.cos(alpha)) + 0 * s, 1: 1 - 2 * s / (Mt * Mx) * (1 - np.cos(alpha)) + 0 * r}
    bound = ref.bound(p, R, S)
    want = ref.wilson_loops(th, Mt, Mx, R, S)
    for b, (i, j, mu) in enumerate(spikes):
        assert np.all(np.abs(got[b] - closed[mu]) <= bound), (i, j, mu)
        assert np.all(np.abs((got[b] - want[b]).astype(np.float64)) <= bound), (i, j, mu)


def test_wrapped_spikes_follow_the_reference(gpu_ops):
    """r = Mt or s = Mx: the loop's two edges along that direction coincide and cancel; the reference decides"""
    import torch
    from mlmcpathintegral_amd import ops
    Mt, Mx, R, S = 5, 3, 5, 3
    th = np.zeros((2, Mx, Mt, 2))
    th[0, 1, 2, 0] = th[1, 2, 4, 1] = 1.1
    th = th.reshape(2, -1)
    got = ops.wilson_loops(torch.from_numpy(th).cuda(), Mt, Mx, R, S).cpu().numpy()
    want = ref.wilson_loops(th, Mt, Mx, R, S)
    assert np.all(np.abs((got - want).astype(np.float64)) <= ref.bound(ref.plan(Mt, Mx, R, S, 2)[1], R, S))
    assert np.all(np.abs(got[:, Mt - 1, Mx - 1] - 1.0) <= ref.bound(ref.plan(Mt, Mx, R, S, 2)[1], R, S)[-1, -1])


@pytest.mark.parametrize("Mt,Mx", [(17, 9), (66, 34)])
def test_identities(gpu_ops, Mt, Mx):
    import torch
    from mlmcpathintegral_amd import ops
    R, S, B = min(Mt, 16), min(Mx, 16), 3
    bound = ref.bound(ref.plan(Mt, Mx, R, S, B)[1], R, S)
    th = _theta(Mt, Mx, B, 5 + Mt)
    W = ops.wilson_loops(torch.from_numpy(th).cuda(), Mt, Mx, R, S).cpu().numpy()
    plaq = ops.qoi_avg_plaquette(torch.from_numpy(th).cuda(), Mt, Mx).cpu().numpy()
    assert np.all(np.abs(W[:, 0, 0] - plaq) <= bound[0, 0])
    g = np.random.default_rng(6).uniform(-np.pi, np.pi, (B, Mx, Mt))
    Wg = ops.wilson_loops(torch.from_numpy(ref.gauge_transform(th, Mt, Mx, g)).cuda(), Mt, Mx, R, S).cpu().numpy()
    assert np.all(np.abs(Wg - W) <= 2 * bound[None])
    if R == Mt and S == Mx:
        assert np.all(np.abs(W[:, -1, -1] - 1.0) <= bound[-1, -1])


def test_the_whole_lattice_loop_is_one(gpu_ops):
    import torch
    from mlmcpathintegral_amd import ops
    for Mt, Mx in ((2, 2), (16, 16), (13, 7)):
        W = ops.wilson_loops(torch.from_numpy(_theta(Mt, Mx, 2, 9)).cuda(), Mt, Mx, Mt, Mx).cpu().numpy()
        assert np.all(np.abs(W[:, -1, -1] - 1.0) <= ref.bound(ref.plan(Mt, Mx, Mt, Mx, 2)[1], Mt, Mx)[-1, -1]), (Mt, Mx)


@pytest.mark.parametrize("Mt,Mx,R,S", [(17, 9, 9, 9), (70, 66, 6, 16)])
def test_bit_identity_over_batch_split_stream_and_accumulator(gpu_ops, Mt, Mx, R, S):
    import torch
    from mlmcpathintegral_amd import ops
    x = torch.from_numpy(_theta(Mt, Mx, 5, 77 + Mt)).cuda()
    whole = ops.wilson_loops(x, Mt, Mx, R, S)
    for b in range(5):
        assert torch.equal(whole[b], ops.wilson_loops(x[b:b + 1].contiguous(), Mt, Mx, R, S)[0]), b
    for cut in (1, 3):
        parts = torch.cat([ops.wilson_loops(x[:cut].contiguous(), Mt, Mx, R, S), ops.wilson_loops(x[cut:].contiguous(), Mt, Mx, R, S)])
        assert torch.equal(whole, parts), cut
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.wilson_loops(x, Mt, Mx, R, S)
    side.synchronize()
    assert torch.equal(whole, other)
    acc = torch.zeros((5, R, S, 2), dtype=torch.float64, device="cuda")
    assert torch.equal(whole, ops.wilson_loops(x, Mt, Mx, R, S, acc=acc))
    assert torch.equal(acc[..., 0], whole) and torch.equal(acc[..., 1], whole * whole)


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


@pytest.mark.parametrize("Mt,Mx,R,S,B", [(17, 9, 9, 9, 7), (70, 66, 6, 16, 3)])
def test_accumulator_and_guard_bands(gpu_ops, Mt, Mx, R, S, B):
    import torch
    from mlmcpathintegral_amd import abi, ops
    nbytes = C.c_size_t(0)
    abi.call("mlmcpi_schwinger_wilson_loops_workspace_bytes", Mt, Mx, R, S, B, C.byref(nbytes))
    assert nbytes.value % 256 == 0 and nbytes.value == ref.plan(Mt, Mx, R, S, B)[1]["work_bytes"]
    # the workspace is 256-byte aligned inside its guard: pad by 64 doubles from torch's 512-byte aligned allocation
    wbuf, work = _guarded(nbytes.value // 8)
    obuf, out = _guarded(B * R * S)
    abuf, acc = _guarded(B * R * S * 2, fill=0.0)
    assert work.data_ptr() % 256 == 0
    outs = []
    for k in range(2):
        x = torch.from_numpy(_theta(Mt, Mx, B, 40 + k)).cuda()
        keep = x.clone()
        abi.call("mlmcpi_schwinger_wilson_loops", C.c_void_p(x.data_ptr()), Mt, Mx, B, R, S, C.c_void_p(out.data_ptr()),
                 C.c_void_p(acc.data_ptr()), C.c_void_p(work.data_ptr()), nbytes.value, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        outs.append(out.clone().reshape(B, R, S))
        assert torch.equal(x, keep)                                              # the state is read only
        assert torch.equal(outs[-1], ops.wilson_loops(x, Mt, Mx, R, S))          # acc = None changes nothing else
    torch.cuda.synchronize()
    assert _bands_intact(wbuf, nbytes.value // 8) and _bands_intact(obuf, B * R * S) and _bands_intact(abuf, B * R * S * 2)
    a = acc.reshape(B, R, S, 2).cpu().numpy()
    o = np.stack([t.cpu().numpy() for t in outs])
    eps = 2.0 ** -52
    assert np.all(np.abs(a[..., 0] - o.sum(axis=0)) <= 2 * eps * np.abs(o).sum(axis=0))
    assert np.all(np.abs(a[..., 1] - (o * o).sum(axis=0)) <= 2 * eps * (o * o).sum(axis=0))


def test_refusals_touch_nothing(gpu_ops):
    import torch
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    Mt, Mx, R, S, B = 40, 20, 4, 3, 3
    x = torch.zeros((B, 2 * Mt * Mx), dtype=torch.float64, device="cuda")
    out = torch.full((B * 17 * 17,), SENTINEL, dtype=torch.float64, device="cuda")
    acc = torch.full((B * 17 * 17 * 2,), SENTINEL, dtype=torch.float64, device="cuda")
    need = C.c_size_t(0)
    assert lib.mlmcpi_schwinger_wilson_loops_workspace_bytes(Mt, Mx, R, S, B, C.byref(need)) == 0
    work = torch.full((B * 2 * 17 * 17 + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    big = work.numel() * 8
    invalid = {
        "NULL d_theta": (None, Mt, Mx, B, R, S, P(out), P(acc), P(work), big, None),
        "NULL d_out": (P(x), Mt, Mx, B, R, S, None, P(acc), P(work), big, None),
        "NULL d_work": (P(x), Mt, Mx, B, R, S, P(out), P(acc), None, big, None),
        "B = 0": (P(x), Mt, Mx, 0, R, S, P(out), P(acc), P(work), big, None),
        "R = 0": (P(x), Mt, Mx, B, 0, S, P(out), P(acc), P(work), big, None),
        "S = 0": (P(x), Mt, Mx, B, R, 0, P(out), P(acc), P(work), big, None),
        "R > Mt": (P(x), 3, Mx, B, 4, S, P(out), P(acc), P(work), big, None),
        "S > Mx": (P(x), Mt, 2, B, R, 3, P(out), P(acc), P(work), big, None),
        "Mt < 2": (P(x), 1, Mx, B, 1, S, P(out), P(acc), P(work), big, None),
        "Mx < 2": (P(x), Mt, 1, B, R, 1, P(out), P(acc), P(work), big, None),
        "Mt Mx > 2^30": (P(x), 2 ** 16, 2 ** 15, B, R, S, P(out), P(acc), P(work), big, None),
        "work_bytes too small": (P(x), Mt, Mx, B, R, S, P(out), P(acc), P(work), need.value - 1, None),
    }
    for name, args in invalid.items():
        assert lib.mlmcpi_schwinger_wilson_loops(*args) == ref.ERR_INVALID, name
        assert lib.mlmcpi_last_error(), name
    unsupported = {
        "R above the cap": (P(x), Mt, Mx, B, 17, S, P(out), P(acc), P(work), big, None),
        "S above the cap": (P(x), Mt, Mx, B, R, 17, P(out), P(acc), P(work), big, None),
        "both above the cap and the lattice": (P(x), 16, 16, B, 17, 17, P(out), P(acc), P(work), big, None),
    }
    for name, args in unsupported.items():
        assert lib.mlmcpi_schwinger_wilson_loops(*args) == ref.ERR_UNSUPPORTED, name
    torch.cuda.synchronize()
    for t in (out, acc, work):
        assert bool((t == SENTINEL).all())
    assert lib.mlmcpi_schwinger_wilson_loops(P(x), Mt, Mx, B, R, S, P(out), P(acc), P(work), need.value, None) == 0   # and the same call, valid
    torch.cuda.synchronize()
    assert bool(((out[:B * R * S] - 1.0).abs() <= 2.0 ** -52).all()) and bool((out[B * R * S:] == SENTINEL).all())


def _law(name, acc, n, exact):
    """z = (mean - exact) / (spread of the per-chain means / sqrt(B)), gate 4.5 (the path correlator's)"""
    means = (acc[..., 0] / n).cpu().numpy()
    B = means.shape[0]
    mean, err = means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(B)
    z = (mean - exact) / err
    print(f"[wilson loops law] {name}: W(4,4) = {mean[3, 3]:.6f} +/- {err[3, 3]:.6f} (exact {exact[3, 3]:.6f}); z =\n{np.array2string(z, precision=2)}")
    _record(name, {"mean": mean.tolist(), "error": err.tolist(), "exact": exact.tolist(), "z": z.tolist(), "gate": 4.5, "samples": n, "chains": B})
    assert err[3, 3] < 0.1 * exact[3, 3], (err[3, 3], exact[3, 3])
    assert float(np.max(np.abs(z))) < 4.5, z


N_DRAWS_HEATBATH = 400   # see test_law_heatbath
N_DRAWS_CLUSTER = 400    # the same count: W(4, 4) = 0.0964 at beta = 4 and its error 3.0e-4, far below a tenth


def test_law_heatbath(gpu_ops):
    """8 x 8, beta = 2, 1024 chains, draws of 10 overrelaxation + 1 heat-bath sweeps (ops.lattice_sweep_draw): 50 of warm-up, then
    N_DRAWS_HEATBATH measured through d_acc, W for r, s <= 4 against the exact series.  The count: W(4, 4) = 0.003158 exactly and its error
    has to be below a tenth of that; one sample of one chain spreads by 0.10 (measured: error 1.6e-4 over 1024 x 400), so 100 draws
    would just do and 400 leave a factor 2."""
    import torch
    from mlmcpathintegral_amd import abi, ops
    Mt, beta, B, seed = 8, 2.0, 1024, 20263
    act = abi.lattice_action(abi.SCHWINGER, Mt, Mt, beta=beta)
    x = ops.lattice_initialise(act, B, seed)
    scratch = torch.empty_like(x)
    acc = torch.zeros((B, 4, 4, 2), dtype=torch.float64, device="cuda")
    work = ops.wilson_loops_workspace(Mt, Mt, 4, 4, B)
    for d in range(50 + N_DRAWS_HEATBATH):
        ops.lattice_sweep_draw(act, x, scratch, 10, 1, seed, 0, 11 * d)
        if d >= 50:
            ops.wilson_loops(x, Mt, Mt, 4, 4, acc=acc, work=work)
    _law("heatbath_beta2", acc, N_DRAWS_HEATBATH, ref.wilson_loops_exact(beta, Mt, Mt, 4, 4))


def test_law_cluster(gpu_ops):
    """8 x 8, beta = 4, 1024 chains of the plaquette-path cluster sampler, links through ops.schwinger_cluster_links: 50 draws of
    warm-up, N_DRAWS_CLUSTER measured"""
    import torch
    from mlmcpathintegral_amd import abi, ops
    Mt, beta, B, seed = 8, 4.0, 1024, 20264
    act = abi.lattice_action(abi.SCHWINGER, Mt, Mt, beta=beta)
    sampler = ops.SchwingerClusterSampler(act, B, n_updates=10, seed=seed)
    theta = torch.empty((B, 2 * Mt * Mt), dtype=torch.float64, device="cuda")
    acc = torch.zeros((B, 4, 4, 2), dtype=torch.float64, device="cuda")
    work = ops.wilson_loops_workspace(Mt, Mt, 4, 4, B)
    for d in range(50 + N_DRAWS_CLUSTER):
        sampler.draw(theta)
        if d >= 50:
            links = ops.schwinger_cluster_links(act, sampler.psi, True, seed, 0, d)
            ops.wilson_loops(links, Mt, Mt, 4, 4, acc=acc, work=work)
    _law("cluster_beta4", acc, N_DRAWS_CLUSTER, ref.wilson_loops_exact(beta, Mt, Mt, 4, 4))
