"""GPU: cooling of the O(3) sigma model on the levels of its CoarsenRotate hierarchy and the cooled charge, susceptibility and
energy by depth (mlmcpi_sigma_level_cooled_charge, sigma_cooling.hip) against the long-double model
(tests/sigma_cooling_reference.py) within the bounds derived there; bit identity over depth lists, launch plans, batch split,
stream and the outputs asked for; the state and guard bands; the chain edge of the launch grid; the refusals and the plan query;
the instanton tables; and the law of chi_t by depth at beta = 1.2.  The records of one run are profiles/sigma_cooling.json and
profiles/sigma_cooling_zscores.json (this module writes them into the directory MLMCPI_SIGMA_COOLING_RECORDS names, if set)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

import sigma_cooling_reference as ref
import sigma_topology_reference as topo
from conftest import zcheck

pytestmark = pytest.mark.gpu

RECORDS = os.environ.get("MLMCPI_SIGMA_COOLING_RECORDS")
SENTINEL, PAD = -7.25, 64
ERR_INVALID = -1
Z_GATE = 4.0
PLAN = "MLMCPI_SIGMA_COOL_PLAN"


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
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _all_same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.fixture
def set_plan():
    from mlmcpathintegral_amd import abi

    def go(value):
        abi.set_option(PLAN, value)
    yield go
    go("")


_device = {}


def _state(key):
    """the device copy of a reference input, uploaded once"""
    if key not in _device:
        _device[key] = torch.from_numpy(ref.gpu_input(*key)).cuda()
    return _device[key]


def _tag(key):
    return "%dx%d %s x %d" % (key[0], key[1], "rotated" if key[2] else "plain", key[3])


RATIOS = {}


def _compare(name, c, Q, chi, E, cooled, rows=slice(None)):
    """device outputs of the chains `rows` against the model c of exactly those chains; returns the largest error over bound"""
    ld = lambda t: t.cpu().numpy().astype(np.longdouble)   # noqa: E731
    eq = np.abs(ld(Q)[rows] - c.Q).astype(np.float64)
    ec = np.abs(ld(chi)[rows] - c.chi).astype(np.float64)
    ee = np.abs(ld(E)[rows] - c.E).astype(np.float64)
    ev = float(np.abs(ref.sigma_of(cooled.cpu().numpy()[rows], c.n, np.longdouble) - c.sig).max())
    r = {"Q": float(np.max(eq / c.q_bound())), "chi": float(np.max(ec / c.chi_bound())), "E": float(np.max(ee / c.e_bound())),
         "vectors": ev / float(c.tau()[-1])}
    print(f"{name}: max |Q - ref| = {eq.max():.3e}, |E - ref| = {ee.max():.3e}, |sigma - ref| = {ev:.3e} (tau = {c.tau()[-1]:.3e}, "
          f"dev64 = {c.dev64.max():.3e}); error over bound {r}; min |Delta| = {c.min_delta:.3g}, margin = {c.margin.min():.3g}")
    assert ev <= c.tau()[-1], (name, r)
    assert np.all(eq <= c.q_bound()) and np.all(ec <= c.chi_bound()) and np.all(ee <= c.e_bound()), (name, r)
    return max(r.values())


PARITY = [k for k in ref.gpu_cases() if k[3] != topo.EDGE_CHAINS]


@pytest.mark.parametrize("key", PARITY, ids=lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3]))
def test_parity_with_the_long_double_model(gpu_ops, key):
    """parity shapes x 3 and 300 chains at depths [0, 1, 2, 3, 7, 10] and the large case at [0, 2, 5]; E_d never rises"""
    Mt, Mx, rot, B = key
    _, c = ref.gpu_case(*key)
    before = _state(key).clone()
    Q, chi, E, cooled = gpu_ops.sigma_level_cooled_charge(_level(Mt, Mx, rot), _state(key), ref.case_depths(key), energy=True, cooled=True)
    RATIOS[_tag(key)] = _compare(_tag(key), c, Q, chi, E, cooled)
    assert _same_bits(_state(key), before)
    assert bool(torch.all(E[:, 1:] - E[:, :-1] <= 1e-12 * c.n))
    _record("sigma_cooling.json", "parity_error_over_bound", {"largest": max(RATIOS.values()), "per_case": RATIOS})


def _plans(Mt, Mx):
    plans = ["", "1x1x256x1", "8x4x256x4", "48x48x1024x1"]   # the default, single sites, K = 4, larger than the level
    if (Mt, Mx) in ((66, 34), (130, 70)):
        plans.append("7x5x512x3")   # an odd tile
    return plans


@pytest.mark.parametrize("Mt,Mx,rot", [(s[0], s[1], r) for s in topo.PARITY_SHAPES for r in (False, True)])
def test_bit_identity(gpu_ops, set_plan, Mt, Mx, rot):
    """Q_0 = the charge; [10] = [0, 1, 2, 3, 7, 10] = [7, 10]; every plan; 300 = 7 + 293; a second stream; every subset of outputs"""
    lv, x, full = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 300)), ref.PARITY_DEPTHS
    want = gpu_ops.sigma_level_cooled_charge(lv, x, full, energy=True, cooled=True)
    Q0, chi0 = gpu_ops.sigma_level_topological_charge(lv, x)
    assert _same_bits(want[0][:, 0].contiguous(), Q0) and _same_bits(want[1][:, 0].contiguous(), chi0)
    small = x[:20].contiguous()   # single-site tiles: 20 chains keep the launch small
    want_small = [t[:20].contiguous() for t in want]
    for plan in _plans(Mt, Mx):
        set_plan(plan)
        xs, ws = (small, want_small) if plan == "1x1x256x1" else (x, want)
        assert _all_same(gpu_ops.sigma_level_cooled_charge(lv, xs, full, energy=True, cooled=True), ws), plan
        last = gpu_ops.sigma_level_cooled_charge(lv, xs, [10], energy=True, cooled=True)
        assert all(_same_bits(a[:, 0], b[:, -1]) for a, b in zip(last[:3], ws[:3])) and _same_bits(last[3], ws[3]), plan
        two = gpu_ops.sigma_level_cooled_charge(lv, xs, [7, 10], energy=True, cooled=True)
        assert all(_same_bits(a, b[:, -2:]) for a, b in zip(two[:3], ws[:3])) and _same_bits(two[3], ws[3]), plan
    set_plan("")
    a = gpu_ops.sigma_level_cooled_charge(lv, x[:7], full, energy=True, cooled=True)
    b = gpu_ops.sigma_level_cooled_charge(lv, x[7:], full, energy=True, cooled=True)
    assert _all_same([torch.cat([s, t]) for s, t in zip(a, b)], want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = gpu_ops.sigma_level_cooled_charge(lv, x, full, energy=True, cooled=True, stream=side)
    side.synchronize()
    assert _all_same(on_side, want)
    work = gpu_ops.sigma_level_cooling_workspace(lv, 300)
    for use in itertools.product((False, True), repeat=4):
        if not any(use[:3]):
            continue
        out = [torch.empty_like(t) if u else None for t, u in zip(want, use)]
        assert _call(lv, x, 300, full, *out, work) == 0
        assert all(o is None or _same_bits(o, t) for o, t in zip(out, want)), use


def _call(level, x, n_chains, depths, q, chi, e, cooled, work, work_bytes=None, stream=None):
    from mlmcpathintegral_amd import abi
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731
    d = None if depths is None else (C.c_uint32 * max(1, len(depths)))(*depths)
    return abi.load().mlmcpi_sigma_level_cooled_charge(
        C.byref(level) if level is not None else None, p(x), n_chains, d, 0 if depths is None else len(depths), p(q), p(chi), p(e),
        p(cooled), p(work), (0 if work is None else work.numel()) if work_bytes is None else work_bytes,
        C.c_void_p(stream or torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, True), (66, 34, False), (130, 70, True)])
def test_guard_bands_and_the_state(gpu_ops, Mt, Mx, rot):
    lv, x, B, depths = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 300)), 300, ref.PARITY_DEPTHS
    before, nd = x.clone(), len(depths)
    nwork = gpu_ops.sigma_level_cooling_workspace(lv, B).numel()
    assert nwork % 8 == 0
    sizes = {"q": B * nd, "chi": B * nd, "e": B * nd, "cooled": x.numel(), "work": nwork // 8}
    big = {k: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda") for k, n in sizes.items()}
    mid = {k: v[PAD:v.numel() - PAD] for k, v in big.items()}
    assert mid["work"].data_ptr() % 256 == 0
    assert _call(lv, x, B, depths, mid["q"], mid["chi"], mid["e"], mid["cooled"], mid["work"], work_bytes=nwork) == 0
    torch.cuda.synchronize()
    band = torch.full((PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    for k, v in big.items():
        assert _same_bits(v[:PAD], band) and _same_bits(v[-PAD:], band), k
    assert _same_bits(x, before)
    want = gpu_ops.sigma_level_cooled_charge(lv, x, depths, energy=True, cooled=True)
    assert _all_same([mid["q"].view(B, nd), mid["chi"].view(B, nd), mid["e"].view(B, nd), mid["cooled"].view_as(x)], want)


@pytest.mark.parametrize("rot", [False, True])
def test_chain_edge_of_the_launch_grid(gpu_ops, rot):
    """n_chains = 65535 and 65581 on (4, 4) at depths [0, 2]: every chain against the split batch, six against the model"""
    key = topo.EDGE_SHAPE + (rot, topo.EDGE_CHAINS)
    _, c = ref.gpu_case(*key)
    lv, x = _level(*topo.EDGE_SHAPE, rot), _state(key)
    full = gpu_ops.sigma_level_cooled_charge(lv, x, ref.EDGE_DEPTHS, energy=True, cooled=True)
    _compare(_tag(key), c, *full, rows=ref.EDGE_PINNED)
    a = gpu_ops.sigma_level_cooled_charge(lv, x[:65535], ref.EDGE_DEPTHS, energy=True, cooled=True)
    assert _all_same(a, [t[:65535] for t in full])
    b = gpu_ops.sigma_level_cooled_charge(lv, x[65535:], ref.EDGE_DEPTHS, energy=True, cooled=True)
    assert _all_same(b, [t[65535:] for t in full])


def test_refusals_write_nothing(gpu_ops):
    from mlmcpathintegral_amd import abi
    x, good = _state((4, 4, False, 3)), _level(4, 4, 0)
    work = gpu_ops.sigma_level_cooling_workspace(good, 3)
    out = {k: torch.full((3, 2), SENTINEL, dtype=torch.float64, device="cuda") for k in ("q", "chi", "e")}
    cooled = torch.full_like(x, SENTINEL)
    o = (out["q"], out["chi"], out["e"], cooled)
    bad = [("level is NULL", None, x, 3, [0, 2], o, work, None), ("d_state is NULL", good, None, 3, [0, 2], o, work, None),
           ("depths is NULL", good, x, 3, None, o, work, None), ("d_work is NULL", good, x, 3, [0, 2], o, None, None),
           ("all three are NULL", good, x, 3, [0, 2], (None, None, None, cooled), work, None),
           ("even extents", _level(3, 4, 0), x, 3, [0, 2], o, work, None), ("even extents", _level(4, 5, 1), x, 3, [0, 2], o, work, None),
           ("even extents", _level(0, 4, 0), x, 3, [0, 2], o, work, None), ("even extents", _level(4, 0, 1), x, 3, [0, 2], o, work, None),
           ("too large", _level(1 << 16, 1 << 15, 0), x, 3, [0, 2], o, work, None),
           ("n_chains > 0", good, x, 0, [0, 2], o, work, None),
           ("strictly ascending", good, x, 3, [2, 2], o, work, None), ("strictly ascending", good, x, 3, [3, 1], o, work, None),
           ("at most 4096", good, x, 3, [0, 4097], o, work, None), ("1 .. 32 depths", good, x, 3, [], o, work, None),
           ("1 .. 32 depths", good, x, 3, list(range(33)), o, work, None),
           ("workspace is too small", good, x, 3, [0, 2], o, work, work.numel() - 1)]
    for msg, lv, state, n, depths, outs, w, wb in bad:
        assert _call(lv, state, n, depths, *outs, w, work_bytes=wb) == ERR_INVALID, msg
        err = abi.load().mlmcpi_last_error().decode()
        assert msg in err, (msg, err)
    torch.cuda.synchronize()
    for t in o:
        assert _same_bits(t, torch.full_like(t, SENTINEL))
    assert _call(good, x, 3, [0, 2], *o, work) == 0


@pytest.mark.parametrize("plan", ["", "1x1x256x1", "8x4x256x4", "16x16x512x16", "7x5x512x3"])
@pytest.mark.parametrize("rot", [False, True])
def test_plan_query(gpu_ops, set_plan, plan, rot):
    """the plan query against the launch arithmetic restated here: the launches' sweeps sum to the last depth and no launch
    crosses a listed depth"""
    set_plan(plan)
    tw, th, nt, K = (int(v) for v in plan.split("x")) if plan else (32, 32, 512, 2)
    lv = _level(66, 34, rot)
    PW, PH = (33, 17) if rot else (66, 34)
    for depths in ([0], [1], [10], [0, 1, 2, 3, 7, 10], [7, 10], [5, 4096]):
        p = gpu_ops.sigma_level_cooling_plan(lv, 300, depths)
        want, done = [], 0
        for d in depths:
            while done < d:
                want.append(min(K, d - done))
                done += want[-1]
        got = list(p.launch_sweeps[:p.n_launches])
        assert got == want and sum(got) == depths[-1] and p.n_measurements == len(depths)
        edges = set(np.cumsum(got).tolist())
        assert all(d in edges for d in depths if d > 0)
        etw, eth = min(tw, PW), min(th, PH)
        assert (p.tw, p.th, p.nt, p.fuse) == (etw, eth, nt, K)
        assert p.tiles == -(-PW // etw) * -(-PH // eth)
        deepest = max(got, default=0)
        halo = deepest if rot else 2 * deepest
        assert p.lds_bytes == ((etw + 2 * halo) * (eth + 2 * halo) * (48 if rot else 24) if deepest else 0)
        assert p.lds_bytes <= 160 * 1024 - 512


def test_the_knob_refuses_what_does_not_fit(gpu_ops, set_plan):
    from mlmcpathintegral_amd import abi
    for bad in ("0x4x256x1", "4x4x128x1", "4x4x256x0", "4x4x256x17", "64x64x256x1x", "20x20x256x16", "129x1x256x1"):
        assert abi.load().mlmcpi_set_option(PLAN.encode(), bad.encode()) == ERR_INVALID, bad


@pytest.mark.parametrize("rot", [False, True])
def test_instanton_tables(gpu_ops, rot):
    """the Q-by-depth and E-by-depth tables of the CPU test, on the device"""
    four_pi = 4 * np.pi
    for Mt, Mx, lam, k in ref.INSTANTON_CASES:
        wantQ, wantE = ref.instanton_table(Mt, Mx, rot, lam, k)
        x = torch.from_numpy(topo.instanton(Mt, Mx, rot, lam, k)).cuda()
        Q, _, E = gpu_ops.sigma_level_cooled_charge(_level(Mt, Mx, rot), x, ref.INSTANTON_DEPTHS, energy=True)
        Q, E = Q[0].cpu().numpy(), E[0].cpu().numpy() / four_pi
        assert np.array_equal(np.rint(Q), np.rint(wantQ)), (Mt, Mx, rot, k, Q, wantQ)
        assert np.abs(Q - wantQ).max() < 1e-10 and np.abs(E - wantE).max() < 1e-10, (Mt, Mx, rot, k)
    zero = torch.zeros((3, 2 * ref.n_vertices(6, 4, rot)), dtype=torch.float64, device="cuda")
    Q, chi, E = gpu_ops.sigma_level_cooled_charge(_level(6, 4, rot), zero, [0, 3], energy=True)
    assert not Q.any() and not chi.any() and not E.any()   # the cold state: a fixed point, exactly zero


def _mean_err(v):
    v = np.asarray(v, dtype=np.float64)
    return float(v.mean()), float(v.std(ddof=1) / np.sqrt(v.size))


def test_law_at_finite_beta(gpu_ops):
    """chi_t at depths 0, 1, 3 at (8, 8), beta = 1.2, from heat-bath draws and from Swendsen-Wang updates: chain counts, burn-in and
    spacing of test_sigma_topology_gpu.py::test_law_at_finite_beta (the depth-0 values are those of that test), |z| <= 4 per depth"""
    from mlmcpathintegral_amd import abi
    beta, B, n_meas, depths = 1.2, 4096, 8, [0, 1, 3]
    lv, act = _level(8, 8, 0, beta), abi.lattice_action(abi.NONLINEAR_SIGMA, 8, 8, beta=beta)
    cwork = gpu_ops.sigma_level_cooling_workspace(lv, B)
    series = {}
    x = gpu_ops.sigma_level_initialise(lv, B, 31337)
    scratch = torch.empty_like(x)
    for k in range(40):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 11 * k)
    hb = []
    for k in range(n_meas):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 440 + 11 * k)
        hb.append(gpu_ops.sigma_level_cooled_charge(lv, x, depths, work=cwork)[1].cpu().numpy())
    assert _same_bits(torch.from_numpy(hb[-1][:, 0].copy()), gpu_ops.sigma_level_topological_charge(lv, x)[1].cpu())
    series["heatbath"] = np.stack(hb, axis=1)   # [B, n_meas, n_depths]
    y = gpu_ops.sigma_level_initialise(lv, B, 4242, chain0=B)
    work = gpu_ops.sigma_sw_workspace(act, B)
    gpu_ops.sigma_sw_draw(act, y, 150, 4242, B, 0, outputs=False, work=work)
    sw = []
    for k in range(n_meas):
        gpu_ops.sigma_sw_draw(act, y, 5, 4242, B, 150 + 5 * k, outputs=False, work=work)
        sw.append(gpu_ops.sigma_level_cooled_charge(lv, y, depths, work=cwork)[1].cpu().numpy())
    series["swendsenwang"] = np.stack(sw, axis=1)
    rec = {}
    for j, d in enumerate(depths):
        (h, he), (s, se) = _mean_err(series["heatbath"][:, :, j].mean(axis=1)), _mean_err(series["swendsenwang"][:, :, j].mean(axis=1))
        z = zcheck(f"sigma cooling beta = 1.2, 8x8, depth {d}: chi_t heat bath vs Swendsen-Wang", h, he, s, se, gate=Z_GATE)
        rec[f"depth_{d}"] = {"heatbath": [h, he], "swendsenwang": [s, se], "z": z}
        assert h > 0.0 and s > 0.0
    _record("sigma_cooling_zscores.json", "beta1.2_8x8_heatbath_vs_sw", rec)
