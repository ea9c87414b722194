"""GPU: the geometric topological charge of the O(3) sigma model on the levels of its CoarsenRotate hierarchy
(mlmcpi_sigma_level_topological_charge, sigma_topology.hip) against the long-double reference (tests/sigma_topology_reference.py)
within the reference's per-chain bound, the integer cases, bit identity over batch size, batch split, stream and the outputs asked
for, guard bands, the accumulated moments, the chain edge of the launch grid, the refusals, and the law of Q at beta = 0 and at
beta = 1.2.  The records of one run are profiles/sigma_topology.json and profiles/sigma_topology_zscores.json (this module writes
the parity ratios and the z-scores into the directory MLMCPI_SIGMA_TOPOLOGY_RECORDS names, if the variable is set)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sigma_topology_reference as ref
from conftest import zcheck

pytestmark = pytest.mark.gpu

RECORDS = os.environ.get("MLMCPI_SIGMA_TOPOLOGY_RECORDS")
SENTINEL, PAD = -7.25, 64
ERR_INVALID = -1
Z_GATE = 5.0


def _record(file, name, payload):
    if RECORDS:
        os.makedirs(RECORDS, exist_ok=True)
        path = os.path.join(RECORDS, file)
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = payload
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


def _level(Mt, Mx, rot, beta=1.0):
    from mlmcpathintegral_amd import abi
    return abi.sigma_level(Mt, Mx, rot, beta)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


_device = {}


def _state(key):
    """the device copy of a reference input, uploaded once"""
    if key not in _device:
        _device[key] = torch.from_numpy(ref.gpu_case(*key)[0]).cuda()
    return _device[key]


RATIOS = {}


def _compare(name, c, Q, chi, sl=slice(None)):
    """Q within the per-chain bound of the reference, chi within the matching bound; returns the largest error over bound"""
    eq = np.abs(Q.cpu().numpy().astype(np.longdouble) - c.Q[sl]).astype(np.float64)
    ec = np.abs(chi.cpu().numpy().astype(np.longdouble) - c.chi[sl]).astype(np.float64)
    bq, bc = c.error_bound()[sl], c.chi_bound()[sl]
    rq, rc = float(np.max(eq / bq)), float(np.max(ec / bc))
    print(f"{name}: max |Q - ref| = {eq.max():.3e}, over bound {rq:.3g}; max |chi - ref| over bound {rc:.3g}; "
          f"charges {int(np.rint(c.Q[sl]).min())} .. {int(np.rint(c.Q[sl]).max())}")
    assert np.all(eq <= bq), (name, rq, int(np.argmax(eq / bq)))
    assert np.all(ec <= bc), (name, rc, int(np.argmax(ec / bc)))
    return max(rq, rc)


PARITY = [k for k in ref.gpu_cases() if k[3] != ref.EDGE_CHAINS]


@pytest.mark.parametrize("key", PARITY, ids=lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3]))
def test_parity_with_the_long_double_reference(gpu_ops, key):
    Mt, Mx, rot, B = key
    _, c = ref.gpu_case(*key)
    Q, chi = gpu_ops.sigma_level_topological_charge(_level(Mt, Mx, rot), _state(key))
    name = "%dx%d %s x %d" % (Mt, Mx, "rotated" if rot else "plain", B)
    RATIOS[name] = _compare(name, c, Q, chi)
    _record("sigma_topology.json", "parity_error_over_bound", {"largest": max(RATIOS.values()), "per_case": RATIOS})


@pytest.mark.parametrize("rot", [False, True])
def test_integer_cases(gpu_ops, rot):
    for Mt, Mx, lam, k in ref.INSTANTONS:
        for anti, want in ((False, k), (True, -k)):
            x = torch.from_numpy(ref.instanton(Mt, Mx, rot, lam, k, anti)).cuda()
            Q, chi = gpu_ops.sigma_level_topological_charge(_level(Mt, Mx, rot), x)
            n = Mt * Mx // 2 if rot else Mt * Mx
            assert np.rint(Q.item()) == want and abs(Q.item() - want) < 1e-12, (Mt, Mx, rot, lam, k, anti, Q.item())
            assert abs(chi.item() - want * want / n) < 1e-12
    for Mt, Mx in ref.PARITY_SHAPES:
        n = Mt * Mx // 2 if rot else Mt * Mx
        Q, chi = gpu_ops.sigma_level_topological_charge(_level(Mt, Mx, rot), torch.zeros((3, 2 * n), dtype=torch.float64, device="cuda"))
        assert Q.tolist() == [0.0] * 3 and chi.tolist() == [0.0] * 3        # the cold state: exactly zero


def _call(level, x, n_chains, q, chi, acc=None, stream=None):
    from mlmcpathintegral_amd import abi
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731
    return abi.load().mlmcpi_sigma_level_topological_charge(C.byref(level) if level is not None else None, p(x), n_chains, p(q), p(chi),
                                                            p(acc), C.c_void_p(stream or torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, False), (6, 4, True), (66, 34, False), (66, 34, True), (130, 70, False), (130, 70, True)])
def test_bit_identity(gpu_ops, Mt, Mx, rot):
    """chain b of the 300-chain call = the same chain alone = in a 7 + 293 split = on a second stream = with one output only"""
    lv, x = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 300))
    Q, chi = gpu_ops.sigma_level_topological_charge(lv, x)
    for b in (0, 6, 7, 255, 256, 299):
        q1, c1 = gpu_ops.sigma_level_topological_charge(lv, x[b:b + 1])
        assert _same_bits(q1, Q[b:b + 1]) and _same_bits(c1, chi[b:b + 1]), b
    qa, ca = gpu_ops.sigma_level_topological_charge(lv, x[:7])
    qb, cb = gpu_ops.sigma_level_topological_charge(lv, x[7:])
    assert _same_bits(torch.cat([qa, qb]), Q) and _same_bits(torch.cat([ca, cb]), chi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qs, cs = gpu_ops.sigma_level_topological_charge(lv, x)
    side.synchronize()
    assert _same_bits(qs, Q) and _same_bits(cs, chi)
    q_only, c_only = torch.empty_like(Q), torch.empty_like(chi)
    assert _call(lv, x, 300, q_only, None) == 0 and _call(lv, x, 300, None, c_only) == 0
    assert _same_bits(q_only, Q) and _same_bits(c_only, chi)


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, True), (66, 34, False), (130, 70, True)])
def test_guard_bands_and_the_state(gpu_ops, Mt, Mx, rot):
    lv, x, B = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 300)), 300
    before = x.clone()
    big = {k: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda") for k, n in (("q", B), ("chi", B), ("acc", 5 * B))}
    mid = {k: v[PAD:v.numel() - PAD] for k, v in big.items()}
    mid["acc"].zero_()
    assert _call(lv, x, B, mid["q"], mid["chi"], mid["acc"]) == 0
    torch.cuda.synchronize()
    band = torch.full((PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    for k, v in big.items():
        assert _same_bits(v[:PAD], band) and _same_bits(v[-PAD:], band), k
    assert _same_bits(x, before)
    Q, chi = gpu_ops.sigma_level_topological_charge(lv, x)
    assert _same_bits(mid["q"], Q) and _same_bits(mid["chi"], chi)


@pytest.mark.parametrize("rot", [False, True])
def test_accumulator_follows_stats_accumulate(gpu_ops, rot):
    """d_acc over three calls on three states = mlmcpi_stats_accumulate of the three chi, bit for bit"""
    lv, B = _level(66, 34, rot), 300
    states = [_state((66, 34, rot, 300)), _state((66, 34, rot, 300)).flip(0).contiguous(), _state((66, 34, rot, 300)).roll(5, 0).contiguous()]
    acc, want = (torch.zeros((B, 5), dtype=torch.float64, device="cuda") for _ in range(2))
    for x in states:
        _, chi = gpu_ops.sigma_level_topological_charge(lv, x, acc=acc)
        gpu_ops.stats_accumulate(want, chi)
    assert _same_bits(acc, want)
    assert acc[:, 0].tolist() == [3.0] * B and float(acc[:, 2].min()) >= 0.0


@pytest.mark.parametrize("rot", [False, True])
def test_chain_edge_of_the_launch_grid(gpu_ops, rot):
    """n_chains = 65535 and 65581 on (4, 4): every chain against the reference"""
    key = ref.EDGE_SHAPE + (rot, ref.EDGE_CHAINS)
    _, c = ref.gpu_case(*key)
    lv, x = _level(*ref.EDGE_SHAPE, rot), _state(key)
    Q, chi = gpu_ops.sigma_level_topological_charge(lv, x)
    _compare("4x4 %s x 65581" % ("rotated" if rot else "plain"), c, Q, chi)
    Q2, chi2 = gpu_ops.sigma_level_topological_charge(lv, x[:65535])
    _compare("4x4 %s x 65535" % ("rotated" if rot else "plain"), c, Q2, chi2, slice(0, 65535))
    assert _same_bits(Q2, Q[:65535]) and _same_bits(chi2, chi[:65535])


def test_refusals_write_nothing(gpu_ops):
    x = _state((4, 4, False, 3))
    out = {k: torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda") for k in ("q", "chi")}
    acc = torch.full((3, 5), SENTINEL, dtype=torch.float64, device="cuda")
    good = _level(4, 4, 0)
    bad = [("NULL level", None, x, 3, out["q"], out["chi"]), ("NULL state", good, None, 3, out["q"], out["chi"]),
           ("both outputs NULL", good, x, 3, None, None), ("no chains", good, x, 0, out["q"], out["chi"]),
           ("odd Mt", _level(3, 4, 0), x, 3, out["q"], out["chi"]), ("odd Mx", _level(4, 5, 1), x, 3, out["q"], out["chi"]),
           ("zero Mt", _level(0, 4, 0), x, 3, out["q"], out["chi"]), ("zero Mx", _level(4, 0, 1), x, 3, out["q"], out["chi"]),
           ("too large", _level(1 << 16, 1 << 15, 0), x, 3, out["q"], out["chi"]), ("too large, rotated", _level(1 << 15, 1 << 16, 1), x, 3, out["q"], out["chi"])]
    for name, lv, state, n, q, chi in bad:
        assert _call(lv, state, n, q, chi, acc) == ERR_INVALID, name
    torch.cuda.synchronize()
    for t in (out["q"], out["chi"], acc):
        assert _same_bits(t, torch.full_like(t, SENTINEL))
    assert _call(_level(1 << 15, 1 << 15, 0), None, 3, out["q"], out["chi"]) == ERR_INVALID   # 2^30 vertices pass the size check: NULL state
    assert _call(good, x, 3, out["q"], out["chi"]) == 0


def _mean_err(v):
    v = np.asarray(v, dtype=np.float64)
    return float(v.mean()), float(v.std(ddof=1) / np.sqrt(v.size))


@pytest.mark.parametrize("rot", [False, True])
def test_law_at_beta_zero(gpu_ops, rot):
    """mlmcpi_sigma_level_initialise draws uniform spins: <Q> and <Q^2> / n of 4096 chains at (8, 8) against the reference on
    independent numpy-uniform spins"""
    lv, B = _level(8, 8, rot), 4096
    Q, chi = gpu_ops.sigma_level_topological_charge(lv, gpu_ops.sigma_level_initialise(lv, B, 20261 + rot))
    c = ref.charge(8, 8, rot, ref.uniform_spins(8, 8, rot, B, seed=977 + rot))
    tag = "rotated" if rot else "plain"
    z = {}
    for what, got, want in (("<Q>", Q.cpu().numpy(), c.Q), ("<Q^2>/n", chi.cpu().numpy(), c.chi)):
        (g, ge), (w, we) = _mean_err(got), _mean_err(want)
        z[what] = zcheck(f"sigma topology beta = 0, 8x8 {tag}: {what}", g, ge, w, we, gate=Z_GATE)
    _record("sigma_topology_zscores.json", f"beta0_8x8_{tag}", z)


def test_law_at_finite_beta(gpu_ops):
    """<Q^2> / n at (8, 8), beta = 1.2, from heat-bath draws and from Swendsen-Wang updates: two independent code paths, 4096
    independent chains each from their own hot start, compared by the spread of the per-chain means (valid whatever tau_int is).
    Burn-in: DESIGN 7.5 records tau_int of chi_m on the far larger 64 x 64 lattice, at most 2.34 heat-bath draws (10 + 1 sweeps) and
    7.08 SW updates up to beta = 1.5; 40 draws and 150 updates are some twenty of those.  It records none for chi_t at this size,
    so the eight measured states a chain contributes, a draw (five updates) apart, also give tau_int of chi_t by the pooled
    autocovariance over the chains, written beside the z-score."""
    from mlmcpathintegral_amd import abi
    beta, B, n_meas = 1.2, 4096, 8
    lv, act = _level(8, 8, 0, beta), abi.lattice_action(abi.NONLINEAR_SIGMA, 8, 8, beta=beta)
    series = {}
    x = gpu_ops.sigma_level_initialise(lv, B, 31337)
    scratch = torch.empty_like(x)
    for k in range(40):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 11 * k)
    hb = []
    for k in range(n_meas):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 440 + 11 * k)
        hb.append(gpu_ops.sigma_level_topological_charge(lv, x)[1].cpu().numpy())
    series["heatbath"] = np.stack(hb, axis=1)
    y = gpu_ops.sigma_level_initialise(lv, B, 4242, chain0=B)
    work = gpu_ops.sigma_sw_workspace(act, B)
    gpu_ops.sigma_sw_draw(act, y, 150, 4242, B, 0, outputs=False, work=work)
    sw = []
    for k in range(n_meas):
        gpu_ops.sigma_sw_draw(act, y, 5, 4242, B, 150 + 5 * k, outputs=False, work=work)
        sw.append(gpu_ops.sigma_level_topological_charge(lv, y)[1].cpu().numpy())
    series["swendsenwang"] = np.stack(sw, axis=1)
    rec = {}
    for name, s in series.items():
        d = s - s.mean()
        rho = [float((d[:, :n_meas - t] * d[:, t:]).mean() / (d * d).mean()) for t in range(1, 4)]
        rec[name] = {"mean": _mean_err(s.mean(axis=1))[0], "error": _mean_err(s.mean(axis=1))[1], "rho_1_2_3": rho,
                     "tau_int_window_3": 0.5 + sum(rho)}
        print(f"chi_t 8x8 beta 1.2 {name}: {rec[name]}")
    (h, he), (s, se) = _mean_err(series["heatbath"].mean(axis=1)), _mean_err(series["swendsenwang"].mean(axis=1))
    rec["z"] = zcheck("sigma topology beta = 1.2, 8x8: chi_t heat bath vs Swendsen-Wang", h, he, s, se, gate=Z_GATE)
    _record("sigma_topology_zscores.json", "beta1.2_8x8_heatbath_vs_sw", rec)
    assert h > 0.0 and s > 0.0
