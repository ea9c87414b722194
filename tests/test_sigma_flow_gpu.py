"""GPU: the gradient flow of the O(3) sigma model on the levels of its CoarsenRotate hierarchy and the flowed charge,
susceptibility and energy by step count (mlmcpi_sigma_level_flowed_charge, sigma_flow.hip) against the long-double model
(tests/sigma_flow_reference.py) within the bounds derived there; bit identity over step lists, launch plans, batch split, stream
and the outputs asked for; the state and guard bands; the chain edge of the launch grid; the refusals and the plan query; the
instanton and dislocation tables; and the law of chi_t by flow time at beta = 1.2.  The records of one run are
profiles/sigma_flow.json and profiles/sigma_flow_zscores.json (written into the directory MLMCPI_SIGMA_FLOW_RECORDS names, if
set)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sigma_cooling_reference as cool
import sigma_flow_reference as ref
import sigma_topology_reference as topo
from conftest import zcheck

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -7.25, 64
ERR_INVALID = -1
Z_GATE = 4.0
PLAN = "MLMCPI_SIGMA_FLOW_PLAN"
LDS_MAX = 160 * 1024 - 512
EPS, STEPS = ref.RUNS[0]


def _level(Mt, Mx, rot, beta=1.0):
    from mlmcpathintegral_amd import abi
    return abi.sigma_level(Mt, Mx, rot, beta)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _all_same(a, b):
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


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


def _tag(key, eps):
    return "%dx%d %s x %d eps %g" % (key[0], key[1], "rotated" if key[2] else "plain", key[3], eps)


RATIOS = {}


def _compare(name, c, Q, chi, E, flowed, rows=slice(None)):
    """device outputs of the chains `rows` against the model c of exactly those chains; returns the largest error over bound"""
    ld = lambda t: t.cpu().numpy().astype(np.longdouble)   # noqa: E731
    eq = np.abs(ld(Q)[rows] - c.Q).astype(np.float64)
    ec = np.abs(ld(chi)[rows] - c.chi).astype(np.float64)
    ee = np.abs(ld(E)[rows] - c.E).astype(np.float64)
    ev = float(np.abs(cool.sigma_of(flowed.cpu().numpy()[rows], c.n, np.longdouble) - c.sig).max())
    r = {"Q": float(np.max(eq / c.q_bound())), "chi": float(np.max(ec / c.chi_bound())), "E": float(np.max(ee / c.e_bound())),
         "vectors": ev / float(c.tau()[-1])}
    print(f"{name}: max |Q - ref| = {eq.max():.3e}, |E - ref| = {ee.max():.3e}, |sigma - ref| = {ev:.3e} (tau = {c.tau()[-1]:.3e}, "
          f"dev64 = {c.dev64.max():.3e}); error over bound {r}; min |Y| = {c.min_norm:.3g}, margin = {c.margin.min():.3g}")
    assert ev <= c.tau()[-1], (name, r)
    assert np.all(eq <= c.q_bound()) and np.all(ec <= c.chi_bound()) and np.all(ee <= c.e_bound()), (name, r)
    return max(r.values())


@pytest.mark.parametrize("key", ref.parity_cases(), ids=lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3]))
def test_parity_with_the_long_double_model(gpu_ops, key):
    """(2, 2) .. (18, 10) x 3 and 300 chains, (66, 34) and (130, 70) x 3 chains, both layouts, at steps [0, 1, 2, 3, 7, 10] of
    eps = 0.05 and [0, 4] of eps = 0.25; E_s never rises; the largest error over bound is recorded and is at most 1"""
    Mt, Mx, rot, B = key
    _, runs = ref.gpu_case(*key)
    before = _state(key).clone()
    for c in runs:
        Q, chi, E, flowed = gpu_ops.sigma_level_flowed_charge(_level(Mt, Mx, rot), _state(key), c.eps, c.depths, energy=True, flowed=True)
        RATIOS[_tag(key, c.eps)] = _compare(_tag(key, c.eps), c, Q, chi, E, flowed)
        assert _same_bits(_state(key), before)
        assert bool(torch.all(E[:, 1:] - E[:, :-1] <= 1e-12 * c.n))
    ref.record("sigma_flow.json", "parity_error_over_bound", {"largest": max(RATIOS.values()), "per_case": RATIOS})
    assert max(RATIOS.values()) <= 1.0


def _largest_fuse(tw, th):
    return max(k for k in range(1, 17) if (tw + 6 * k) * (th + 6 * k) * 144 <= LDS_MAX)


def _plans():
    # the default, single sites, K = 2, an odd tile at K = 3, and the largest K whose images fit (on a 2 x 2 tile: 5)
    return ["", "1x1x256x1", "8x4x256x2", "7x5x512x3", "2x2x1024x%d" % _largest_fuse(2, 2)]


@pytest.mark.parametrize("Mt,Mx,rot", [(s[0], s[1], r) for s in ref.SMALL_SHAPES for r in (False, True)])
def test_bit_identity(gpu_ops, set_plan, Mt, Mx, rot):
    """Q_0 = the charge; [10] = [0, 1, 2, 3, 7, 10]; [3, 7] against [7]; every plan; 300 = 1 + 299; a second stream; every subset of
    outputs"""
    assert _largest_fuse(2, 2) == 5 and (2 + 36) * (2 + 36) * 144 > LDS_MAX
    lv, x, full = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 300)), STEPS
    want = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, full, energy=True, flowed=True)
    Q0, chi0 = gpu_ops.sigma_level_topological_charge(lv, x)
    assert _same_bits(want[0][:, 0].contiguous(), Q0) and _same_bits(want[1][:, 0].contiguous(), chi0)
    for plan in _plans():
        set_plan(plan)
        assert _all_same(gpu_ops.sigma_level_flowed_charge(lv, x, EPS, full, energy=True, flowed=True), want), plan
        last = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [10], energy=True, flowed=True)
        assert all(_same_bits(a[:, 0], b[:, -1]) for a, b in zip(last[:3], want[:3])) and _same_bits(last[3], want[3]), plan
        two = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [3, 7], energy=True, flowed=True)
        one = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [7], energy=True, flowed=True)
        assert all(_same_bits(a[:, 1], b[:, 0]) for a, b in zip(two[:3], one[:3])) and _same_bits(two[3], one[3]), plan
        assert all(_same_bits(a, b[:, 3:5]) for a, b in zip(two[:3], want[:3])), plan
    set_plan("")
    a = gpu_ops.sigma_level_flowed_charge(lv, x[:1], EPS, full, energy=True, flowed=True)
    b = gpu_ops.sigma_level_flowed_charge(lv, x[1:], EPS, full, energy=True, flowed=True)
    assert _all_same([torch.cat([s, t]) for s, t in zip(a, b)], want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, full, energy=True, flowed=True, stream=side)
    side.synchronize()
    assert _all_same(on_side, want)
    work = gpu_ops.sigma_level_flow_workspace(lv, 300)
    for use in itertools.product((False, True), repeat=4):
        if not any(use[:3]):
            continue
        out = [torch.empty_like(t) if u else None for t, u in zip(want, use)]
        assert _call(lv, x, 300, EPS, full, *out, work) == 0
        assert all(o is None or _same_bits(o, t) for o, t in zip(out, want)), use


@pytest.mark.parametrize("Mt,Mx,rot", [(s[0], s[1], r) for s in ref.LARGE_SHAPES for r in (False, True)])
def test_bit_identity_over_plans_past_one_tile(gpu_ops, set_plan, Mt, Mx, rot):
    """the plans on levels of many tiles, tiles that do not divide the plane and halos that wrap: 3 chains"""
    lv, x = _level(Mt, Mx, rot), _state((Mt, Mx, rot, 3))
    want = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, STEPS, energy=True, flowed=True)
    for plan in _plans()[1:] + ["32x8x512x2"]:
        set_plan(plan)
        assert _all_same(gpu_ops.sigma_level_flowed_charge(lv, x, EPS, STEPS, energy=True, flowed=True), want), plan
        two = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [3, 7], energy=True)
        assert all(_same_bits(a, b[:, 3:5]) for a, b in zip(two, want[:3])), plan


@pytest.mark.parametrize("Mt,Mx,rot", [(6, 4, True), (18, 10, False), (130, 70, True)])
def test_flowed_fed_back_in_continues_within_the_parity_bound(gpu_ops, Mt, Mx, rot):
    """the angles of step 3 as a state: its steps 4 and 7 are steps 7 and 10 of the input within the bounds of the comparison (the
    atan2 / sincos round trip is not bit-exact, and is what the factor 8 of tau allows for)"""
    key = (Mt, Mx, rot, 3)
    _, runs = ref.gpu_case(*key)
    c = runs[0]
    lv, x = _level(Mt, Mx, rot), _state(key)
    flowed3 = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [3], flowed=True)[2]
    Q, chi, E, flowed = gpu_ops.sigma_level_flowed_charge(lv, flowed3, EPS, [4, 7], energy=True, flowed=True)
    sub = ref.Flowed(c.n, [7, 10], c.eps)
    for k in ("Q", "chi", "E", "margin", "weight"):
        setattr(sub, k, getattr(c, k)[:, 4:6])
    sub.dev64, sub.sig, sub.min_norm = c.dev64[4:6], c.sig, c.min_norm
    _compare(_tag(key, EPS) + " (resumed at step 3)", sub, Q, chi, E, flowed)


def _call(level, x, n_chains, eps, steps, q, chi, e, flowed, work, work_bytes=None, stream=None):
    from mlmcpathintegral_amd import abi
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731
    d = None if steps is None else (C.c_uint32 * max(1, len(steps)))(*steps)
    return abi.load().mlmcpi_sigma_level_flowed_charge(
        C.byref(level) if level is not None else None, p(x), n_chains, eps, d, 0 if steps is None else len(steps), p(q), p(chi), p(e),
        p(flowed), p(work), (0 if work is None else work.numel()) if work_bytes is None else work_bytes,
        C.c_void_p(stream or torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("Mt,Mx,rot,B", [(6, 4, True, 300), (66, 34, False, 3), (130, 70, True, 3)])
def test_guard_bands_and_the_state(gpu_ops, Mt, Mx, rot, B):
    lv, x, steps = _level(Mt, Mx, rot), _state((Mt, Mx, rot, B)), STEPS
    before, nd = x.clone(), len(steps)
    nwork = gpu_ops.sigma_level_flow_workspace(lv, B).numel()
    assert nwork % 8 == 0
    sizes = {"q": B * nd, "chi": B * nd, "e": B * nd, "flowed": x.numel(), "work": nwork // 8}
    big = {k: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda") for k, n in sizes.items()}
    mid = {k: v[PAD:v.numel() - PAD] for k, v in big.items()}
    assert mid["work"].data_ptr() % 256 == 0
    assert _call(lv, x, B, EPS, steps, mid["q"], mid["chi"], mid["e"], mid["flowed"], mid["work"], work_bytes=nwork) == 0
    torch.cuda.synchronize()
    band = torch.full((PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    for k, v in big.items():
        assert _same_bits(v[:PAD], band) and _same_bits(v[-PAD:], band), k
    assert _same_bits(x, before)
    want = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, steps, energy=True, flowed=True)
    assert _all_same([mid["q"].view(B, nd), mid["chi"].view(B, nd), mid["e"].view(B, nd), mid["flowed"].view_as(x)], want)


@pytest.mark.parametrize("rot", [False, True])
def test_chain_edge_of_the_launch_grid(gpu_ops, rot):
    """n_chains = 65535 and 65581 on (2, 2) at steps [0, 2]: every chain against the split batch, six against the model"""
    key = ref.EDGE_SHAPE + (rot, ref.EDGE_CHAINS)
    _, (c,) = ref.gpu_case(*key)
    lv, x = _level(*ref.EDGE_SHAPE, rot), _state(key)
    full = gpu_ops.sigma_level_flowed_charge(lv, x, c.eps, c.depths, energy=True, flowed=True)
    _compare(_tag(key, c.eps), c, *full, rows=ref.EDGE_PINNED)
    a = gpu_ops.sigma_level_flowed_charge(lv, x[:65535], c.eps, c.depths, energy=True, flowed=True)
    assert _all_same(a, [t[:65535] for t in full])
    b = gpu_ops.sigma_level_flowed_charge(lv, x[65535:], c.eps, c.depths, energy=True, flowed=True)
    assert _all_same(b, [t[65535:] for t in full])


def test_refusals_write_nothing(gpu_ops):
    from mlmcpathintegral_amd import abi
    x, good = _state((6, 4, False, 3)), _level(6, 4, 0)
    work = gpu_ops.sigma_level_flow_workspace(good, 3)
    out = {k: torch.full((3, 2), SENTINEL, dtype=torch.float64, device="cuda") for k in ("q", "chi", "e")}
    flowed = torch.full_like(x, SENTINEL)
    o = (out["q"], out["chi"], out["e"], flowed)
    s = [0, 2]
    bad = [("level is NULL", None, x, 3, EPS, s, o, work, None), ("d_state is NULL", good, None, 3, EPS, s, o, work, None),
           ("steps is NULL", good, x, 3, EPS, None, o, work, None), ("d_work is NULL", good, x, 3, EPS, s, o, None, None),
           ("all three are NULL", good, x, 3, EPS, s, (None, None, None, flowed), work, None),
           ("even extents", _level(3, 4, 0), x, 3, EPS, s, o, work, None), ("even extents", _level(4, 5, 1), x, 3, EPS, s, o, work, None),
           ("even extents", _level(0, 4, 0), x, 3, EPS, s, o, work, None), ("too large", _level(1 << 16, 1 << 15, 0), x, 3, EPS, s, o, work, None),
           ("n_chains > 0", good, x, 0, EPS, s, o, work, None),
           ("0 < eps <= 0.25", good, x, 3, 0.0, s, o, work, None), ("0 < eps <= 0.25", good, x, 3, -0.05, s, o, work, None),
           ("0 < eps <= 0.25", good, x, 3, 0.2500001, s, o, work, None), ("0 < eps <= 0.25", good, x, 3, float("nan"), s, o, work, None),
           ("0 < eps <= 0.25", good, x, 3, float("inf"), s, o, work, None),
           ("strictly ascending", good, x, 3, EPS, [2, 2], o, work, None), ("strictly ascending", good, x, 3, EPS, [3, 1], o, work, None),
           ("at most 4096", good, x, 3, EPS, [0, 4097], o, work, None), ("1 .. 32 step counts", good, x, 3, EPS, [], o, work, None),
           ("1 .. 32 step counts", good, x, 3, EPS, list(range(33)), o, work, None),
           ("workspace is too small", good, x, 3, EPS, s, o, work, work.numel() - 1),
           # 2^22 groups of 256 vertices x 2^20 chains > 2^23 x 65535 workgroups
           ("workgroups per launch", _level(1 << 15, 1 << 15, 0), x, 1 << 20, EPS, s, o, work, None)]
    for msg, lv, state, n, eps, steps, outs, w, wb in bad:
        assert _call(lv, state, n, eps, steps, *outs, w, work_bytes=wb) == ERR_INVALID, msg
        err = abi.load().mlmcpi_last_error().decode()
        assert msg in err, (msg, err)
    torch.cuda.synchronize()
    for t in o:
        assert _same_bits(t, torch.full_like(t, SENTINEL))
    assert _call(good, x, 3, 0.25, s, *o, work) == 0


@pytest.mark.parametrize("plan", ["", "1x1x256x1", "8x4x256x2", "7x5x512x3", "2x2x1024x5", "16x16x512x2"])
@pytest.mark.parametrize("rot", [False, True])
def test_plan_query(gpu_ops, set_plan, plan, rot):
    """the plan query against the launch arithmetic restated here: the launches' steps sum to the last step count, no launch
    crosses a listed one, and lds_bytes = (tw + 6 K)(th + 6 K) x 72 B (rotated 144 B) at the deepest launch"""
    set_plan(plan)
    tw, th, nt, K = (int(v) for v in plan.split("x")) if plan else (16, 16, 512, 1)
    lv = _level(66, 34, rot)
    PW, PH = (33, 17) if rot else (66, 34)
    for steps in ([0], [1], [10], [0, 1, 2, 3, 7, 10], [3, 7], [5, 4096]):
        p = gpu_ops.sigma_level_flow_plan(lv, 300, EPS, steps)
        want, done = [], 0
        for d in steps:
            while done < d:
                want.append(min(K, d - done))
                done += want[-1]
        got = list(p.launch_steps[:p.n_launches])
        assert got == want and sum(got) == steps[-1] and p.n_measurements == len(steps)
        edges = set(np.cumsum(got).tolist())
        assert all(d in edges for d in steps if d > 0)
        etw, eth = min(tw, PW), min(th, PH)
        assert (p.tw, p.th, p.nt, p.fuse) == (etw, eth, nt, K)
        assert p.tiles == -(-PW // etw) * -(-PH // eth)
        deepest = max(got, default=0)
        assert p.lds_bytes == ((etw + 6 * deepest) * (eth + 6 * deepest) * (144 if rot else 72) if deepest else 0)
        assert p.lds_bytes <= LDS_MAX
    from mlmcpathintegral_amd import abi
    plan_out = abi.SigmaFlowPlan()
    d = (C.c_uint32 * 1)(3)
    assert abi.load().mlmcpi_sigma_level_flow_plan(C.byref(lv), 300, 0.3, d, 1, C.byref(plan_out)) == ERR_INVALID
    assert "0 < eps <= 0.25" in abi.load().mlmcpi_last_error().decode()


def test_the_knob_refuses_what_does_not_fit(gpu_ops, set_plan):
    from mlmcpathintegral_amd import abi
    for bad in ("0x4x256x1", "4x4x128x1", "4x4x256x0", "4x4x256x17", "16x16x256x1x", "2x2x256x6", "32x32x512x1", "129x1x256x1"):
        assert abi.load().mlmcpi_set_option(PLAN.encode(), bad.encode()) == ERR_INVALID, bad
    for good in ("2x2x256x5", "27x27x512x1", "128x1x1024x1"):
        set_plan(good)


@pytest.mark.parametrize("rot", [False, True])
def test_instanton_and_dislocation_tables(gpu_ops, rot):
    """the Q-by-step and E-by-step tables of the CPU test, on the device; the dislocation loses its charge at the model's step"""
    four_pi = 4 * np.pi
    cases = [(c, ref.INSTANTON_STEPS) for c in ref.INSTANTON_CASES] + [(ref.DISLOCATION, ref.DISLOCATION_STEPS)]
    for (Mt, Mx, lam, k), steps in cases:
        wantQ, wantE = ref.instanton_table(Mt, Mx, rot, lam, k, tuple(steps))
        x = torch.from_numpy(topo.instanton(Mt, Mx, rot, lam, k)).cuda()
        Q, _, E = gpu_ops.sigma_level_flowed_charge(_level(Mt, Mx, rot), x, ref.TABLE_EPS, steps, energy=True)
        Q, E = Q[0].cpu().numpy(), E[0].cpu().numpy() / four_pi
        assert np.array_equal(np.rint(Q), np.rint(wantQ)), (Mt, Mx, rot, k, Q, wantQ)
        assert np.abs(Q - wantQ).max() < 1e-10 and np.abs(E - wantE).max() < 1e-10, (Mt, Mx, rot, k)
        if (Mt, Mx, lam, k) == ref.DISLOCATION:
            assert steps[ref.charge_loss_step(Q)] == ref.DISLOCATION_LOSS_STEP[rot]
        elif not rot:
            assert np.all(np.rint(Q) == k)
    zero = torch.zeros((3, 2 * cool.n_vertices(6, 4, rot)), dtype=torch.float64, device="cuda")
    Q, chi, E = gpu_ops.sigma_level_flowed_charge(_level(6, 4, rot), zero, 0.25, [0, 3], energy=True)
    assert not Q.any() and not chi.any() and not E.any()   # the cold state: a fixed point, exactly zero


def _mean_err(v):
    v = np.asarray(v, dtype=np.float64)
    return float(v.mean()), float(v.std(ddof=1) / np.sqrt(v.size))


def test_law_at_finite_beta(gpu_ops):
    """chi_t at t = 0, 0.25, 1 (eps = 0.05) at (8, 8), beta = 1.2, from heat-bath draws and from Swendsen-Wang updates: chain
    counts, burn-in and spacing of test_sigma_cooling_gpu.py::test_law_at_finite_beta, |z| < 4 per flow time"""
    from mlmcpathintegral_amd import abi
    beta, B, n_meas, steps = 1.2, 4096, 8, [0, 5, 20]
    lv, act = _level(8, 8, 0, beta), abi.lattice_action(abi.NONLINEAR_SIGMA, 8, 8, beta=beta)
    fwork = gpu_ops.sigma_level_flow_workspace(lv, B)
    series = {}
    x = gpu_ops.sigma_level_initialise(lv, B, 31337)
    scratch = torch.empty_like(x)
    for k in range(40):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 11 * k)
    hb = []
    for k in range(n_meas):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 31337, 0, 440 + 11 * k)
        hb.append(gpu_ops.sigma_level_flowed_charge(lv, x, EPS, steps, work=fwork)[1].cpu().numpy())
    assert _same_bits(torch.from_numpy(hb[-1][:, 0].copy()), gpu_ops.sigma_level_topological_charge(lv, x)[1].cpu())
    series["heatbath"] = np.stack(hb, axis=1)   # [B, n_meas, n_steps]
    y = gpu_ops.sigma_level_initialise(lv, B, 4242, chain0=B)
    work = gpu_ops.sigma_sw_workspace(act, B)
    gpu_ops.sigma_sw_draw(act, y, 150, 4242, B, 0, outputs=False, work=work)
    sw = []
    for k in range(n_meas):
        gpu_ops.sigma_sw_draw(act, y, 5, 4242, B, 150 + 5 * k, outputs=False, work=work)
        sw.append(gpu_ops.sigma_level_flowed_charge(lv, y, EPS, steps, work=fwork)[1].cpu().numpy())
    series["swendsenwang"] = np.stack(sw, axis=1)
    rec = {}
    for j, s in enumerate(steps):
        (h, he), (w, we) = _mean_err(series["heatbath"][:, :, j].mean(axis=1)), _mean_err(series["swendsenwang"][:, :, j].mean(axis=1))
        z = zcheck(f"sigma flow beta = 1.2, 8x8, t = {s * EPS:g}: chi_t heat bath vs Swendsen-Wang", h, he, w, we, gate=Z_GATE)
        rec[f"t_{s * EPS:g}"] = {"heatbath": [h, he], "swendsenwang": [w, we], "z": z}
        assert h > 0.0 and w > 0.0
    ref.record("sigma_flow_zscores.json", "beta1.2_8x8_heatbath_vs_sw", rec)
