"""GPU: the Swendsen-Wang multi-cluster update of the O(3) sigma model on the levels of its CoarsenRotate hierarchy
(mlmcpi_sigma_level_sw_draw, sigma_sw.hip) against its numpy restatement (tests/sigma_level_sw_model.py) update by
update, its invariances bit for bit (call split, batch split, launch plan, tile, outputs asked for or not), the delegation of an
unrotated level, its law and its improved estimator against the device's rotated heat bath and the CPU model, the hierarchical
chain it is there for, and host/driver --coarsesampler levelsw."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sigma_level_model as slm
import sigma_level_sw_model as slsw
from conftest import zcheck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_MAX_N = 7552      # the chain plan's LDS bound
# Swendsen-Wang updates per coarse draw of the hierarchical chain at 8 x 8, beta = 1.  DESIGN.md 7.6 found 20 level-Wolff updates
# between proposals sufficient there.  On the CPU, with the numpy models (tools/exp_sigma_level_sw_model.py,
# profiles/sigma_level_sw_model.json: rotated 8 x 8 level, beta = 1, 512 chains x 200 draws), the lag-1 autocorrelation of chi_m
# between successive draws is 0.0780 +- 0.0029 under 20 level-Wolff updates per draw and 0.842, 0.522, 0.293, 0.0962 +- 0.0034,
# 0.0827 +- 0.0026, 0.0735 +- 0.0022, 0.0505 +- 0.0034 under k = 1, 4, 8, 16, 17, 18, 20 Swendsen-Wang updates per draw (a factor
# 0.85 per update: at beta = 1 the clusters are small and one update moves the component of M along one normal only): k = 18 is
# the smallest k whose autocorrelation is no larger.
K_HIER = 18


def _level(Mt, Mx, rot, beta):
    from mlmcpathintegral_amd import abi
    return abi.sigma_level(Mt, Mx, rot, beta)


def _thermalised(ops, lv, B, seed, draws=2, aligned=False):
    """device states with some order in them: a random (or all-aligned) start, then `draws` heat-bath draws of 10 + 1 sweeps"""
    x = ops.sigma_level_initialise(lv, B, seed)
    if aligned:
        x[:, 0::2] = 0.5 * math.pi
        x[:, 1::2] = 0.25
    w = torch.empty_like(x)
    for d in range(draws):
        ops.sigma_level_sweep_draw(lv, x, w, 10, 1, seed, 0, 11 * d)
    return x


class _plan:
    """a launch plan forced through mlmcpi_set_option, the defaults restored on exit"""

    def __init__(self, plan="", tile=""):
        self.plan, self.tile = plan, tile

    def __enter__(self):
        from mlmcpathintegral_amd import abi
        abi.set_option("MLMCPI_SIGMA_SW_PLAN", self.plan)
        abi.set_option("MLMCPI_SIGMA_SW_TILE", self.tile)

    def __exit__(self, *exc):
        from mlmcpathintegral_amd import abi
        abi.set_option("MLMCPI_SIGMA_SW_PLAN", "")
        abi.set_option("MLMCPI_SIGMA_SW_TILE", "")


def _draw_into(ops, lv, x, n, seed, chain0, update0, out, work=None):
    """mlmcpi_sigma_level_sw_draw ADDING to the caller's accumulators out = (flipped, clusters, improved)"""
    from mlmcpathintegral_amd import abi
    B = x.shape[0]
    work = ops.sigma_level_sw_workspace(lv, B) if work is None else work
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    abi.call("mlmcpi_sigma_level_sw_draw", C.byref(lv), p(x), B, n, seed, chain0, update0, p(out[0]), p(out[1]), p(out[2]), p(work),
             C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _zeros(B):
    return (torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
            torch.zeros(B, dtype=torch.float64, device="cuda"))


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


# ---- parity, update by update ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "tiled8x8"])
@pytest.mark.parametrize("beta", [1.0, 1.5])
@pytest.mark.parametrize("Mt,Mx,B,n", [(2, 2, 5, 8), (2, 6, 5, 8), (4, 6, 5, 8), (16, 16, 4, 6), (66, 34, 3, 4), (130, 70, 3, 3)])
def test_every_update_equals_the_model(gpu_ops, Mt, Mx, B, n, beta, mode):
    """each device update on a rotated level against the model applied to the device's own previous state: the same set of
    changed vertices, the same flipped and cluster counts, unit vectors to 1e-11, the improved value to 1e-9 relative (one ulp in
    a between two libms can move q(a) by one unit).  A bond whose uniform lies within 1e-10 of its probability could flip
    between two libms: the margin is asserted never to be that small, not skipped.  The seeds (3000 + Mt + 10 beta) were run
    through the model on the CPU first, from the model's own two 10 + 1 draws: every case clears the margin (smallest:
    5.1e-6, rotated (16, 16) at beta = 1.5), holds a cluster larger than 1 and an update with at least two clusters.  Tiles
    of 8 x 8 cells: (66, 34) has planes of 33 x 17, so 5 x 3 tiles with masked edges; (130, 70) 9 x 5; on the small levels one
    masked tile whose wrap links all cross."""
    ops = gpu_ops
    L = slm.Level(Mt, Mx, True, beta)
    lv = _level(Mt, Mx, 1, beta)
    seed, chain0, update0 = 3000 + Mt + int(10 * beta), 3, 40
    x = _thermalised(ops, lv, B, seed)
    work = ops.sigma_level_sw_workspace(lv, B)
    largest, most = 0, 0
    with _plan(*(("", "") if mode == "default" else ("tiled", "8x8"))):
        for k in range(n):
            before = x.cpu().numpy()
            flipped, clusters, improved = (t.cpu().numpy() for t in ops.sigma_level_sw_draw(lv, x, 1, seed, chain0, update0 + k, work=work))
            after = x.cpu().numpy()
            for b in range(B):
                want, info = slsw.dev_update(L, before[b], seed, chain0 + b, update0 + k)
                sizes = np.bincount(info["labels"])
                print(f"rotated {Mt}x{Mx} beta={beta} update {k} chain {b}: {info['clusters']} clusters, largest {sizes.max()}, "
                      f"{len(info['flipped'])} flipped, margin {info['margin']:.3g}, improved {improved[b]:.12g} vs {info['improved']:.12g}")
                assert info["margin"] > 1e-10, "a bond decision within 1e-10 of its uniform: change the seed"
                changed = np.nonzero(np.any(after[b].reshape(L.n, 2) != before[b].reshape(L.n, 2), axis=1))[0]
                assert np.array_equal(changed, info["flipped"]), (k, b, len(changed), len(info["flipped"]))
                assert flipped[b] == len(info["flipped"]) and clusters[b] == info["clusters"]
                d = np.abs(slm.unit_vectors(L, after[b][None]) - slm.unit_vectors(L, want[None])).max()
                assert d < 1e-11, (k, b, d)
                assert abs(improved[b] - info["improved"]) <= 1e-9 * info["improved"], (k, b, improved[b], info["improved"])
                largest, most = max(largest, int(sizes.max())), max(most, info["clusters"])
    assert largest > 1 and most >= 2, "a kernel that bonds nothing, or everything, must not pass"


# ---- invariances, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B,beta", [(2, 2, 8, 1.5), (16, 16, 8, 1.0), (130, 70, 4, 1.5), (512, 300, 4, 1.5), (1024, 1024, 4, 1.5)])
def test_call_split_batch_split_plans_tiles_and_outputs_give_the_same_bits(gpu_ops, Mt, Mx, B, beta):
    """rotated levels; (512, 300) has planes of 256 x 150 and n = 76 800, beyond the chain plan: 150 is no multiple of 8, 32 or
    64, so every tile column ends in a masked tile; (1024, 1024) has n = 524 288 and starts aligned, so that clusters span many
    tiles"""
    ops = gpu_ops
    lv = _level(Mt, Mx, 1, beta)
    nv, n = Mt * Mx // 2, 10
    seed, chain0, update0 = 191 + Mt, 5, 1000
    x0 = _thermalised(ops, lv, B, seed, aligned=Mt == 1024)
    ref, out = x0.clone(), _zeros(B)
    _draw_into(ops, lv, ref, n, seed, chain0, update0, out)
    print(f"rotated {Mt} x {Mx} beta = {beta}: per update {out[0].double().mean().item() / n:.1f} flipped, "
          f"{out[1].double().mean().item() / n:.1f} clusters, improved chi_m {out[2].mean().item() / n:.6g}")
    assert not torch.equal(ref, x0) and (out[1] >= n).all() and (out[2] > 0).all()

    a, acc = x0.clone(), _zeros(B)                                   # 10 updates = 5 + 5, into the same accumulators
    _draw_into(ops, lv, a, 5, seed, chain0, update0, acc)
    _draw_into(ops, lv, a, 5, seed, chain0, update0 + 5, acc)
    assert torch.equal(a, ref) and _same(acc, out)

    h = B // 2                                                       # the batch in two halves
    lo, hi, olo, ohi = x0[:h].clone(), x0[h:].clone(), _zeros(h), _zeros(B - h)
    _draw_into(ops, lv, lo, n, seed, chain0, update0, olo)
    _draw_into(ops, lv, hi, n, seed, chain0 + h, update0, ohi)
    assert torch.equal(torch.cat([lo, hi]), ref) and _same([torch.cat(p) for p in zip(olo, ohi)], out)

    plans = [("tiled", t) for t in ("8x8", "16x32", "64x64")] + ([("chain", "")] if nv <= CHAIN_MAX_N else [])
    for plan, tile in plans:
        with _plan(plan, tile):
            y, o = x0.clone(), _zeros(B)
            _draw_into(ops, lv, y, n, seed, chain0, update0, o)
        assert torch.equal(y, ref) and _same(o, out), (plan, tile)
        with _plan(plan, tile):                                      # and without outputs: the same state
            y = x0.clone()
            assert ops.sigma_level_sw_draw(lv, y, n, seed, chain0, update0, outputs=False) is None
        assert torch.equal(y, ref), (plan, tile, "no outputs")


def test_the_chain_plan_beyond_its_capacity_is_refused(gpu_ops):
    from mlmcpathintegral_amd import abi
    ops = gpu_ops
    lv = _level(512, 300, 1, 1.5)
    x = ops.sigma_level_initialise(lv, 1, 3)
    x0 = x.clone()
    with _plan("chain", ""):
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            ops.sigma_level_sw_draw(lv, x, 1, 1, 0, 0)
    assert torch.equal(x, x0)


# ---- guard bands ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,tile", [("chain", ""), ("tiled", "8x8")])
@pytest.mark.parametrize("rot", [1, 0])
def test_nothing_outside_the_workspace_is_written_and_its_content_at_entry_is_ignored(gpu_ops, rot, plan, tile):
    """(12, 10), three chains, three updates; tiles of 8 x 8: 2 x 2 masked tiles on the lattice, one tile of 6 x 5 cells whose wrap
    links all cross on the level.  The workspace sits in a buffer of 0xA5 with 256 B either side: both bands stay, and the state
    and outputs are the bits of a run on a zeroed workspace of exactly the queried size."""
    ops, B, n = gpu_ops, 3, 3
    lv = _level(12, 10, rot, 1.5)
    x0 = _thermalised(ops, lv, B, 9)
    need = ops.sigma_level_sw_workspace(lv, B).numel()
    with _plan(plan, tile):
        ref, want = x0.clone(), _zeros(B)
        _draw_into(ops, lv, ref, n, 10, 1, 3, want, work=torch.zeros(need, dtype=torch.uint8, device="cuda"))
        wbuf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        x, out = x0.clone(), _zeros(B)
        _draw_into(ops, lv, x, n, 10, 1, 3, out, work=wbuf[256:256 + need])
    assert (wbuf[:256] == 0xA5).all() and (wbuf[256 + need:] == 0xA5).all()
    assert torch.equal(x, ref) and _same(out, want)
    assert not torch.equal(ref, x0) and (want[1] > 0).all()


# ---- an unrotated level is mlmcpi_sigma_sw_draw -----------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx", [(16, 16), (130, 70)])
def test_unrotated_level_gives_the_bits_and_the_workspace_of_the_lattice_entry_point(gpu_ops, Mt, Mx):
    from mlmcpathintegral_amd import abi
    ops, B, beta = gpu_ops, 6, 1.5
    lv = _level(Mt, Mx, 0, beta)
    act = abi.lattice_action(abi.NONLINEAR_SIGMA, Mt, Mx, beta=beta)
    x0 = _thermalised(ops, lv, B, 50 + Mt)
    a, b = x0.clone(), x0.clone()
    assert ops.sigma_level_sw_workspace(lv, B).numel() == ops.sigma_sw_workspace(act, B).numel()
    oa = ops.sigma_level_sw_draw(lv, a, 10, 9, 2, 30)
    ob = ops.sigma_sw_draw(act, b, 10, 9, 2, 30)
    assert torch.equal(a, b) and _same(oa, ob) and not torch.equal(a, x0)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _chain_means(samples, B):
    m = torch.stack(samples).mean(dim=0).cpu().numpy()
    return float(m.mean()), float(m.std(ddof=1) / math.sqrt(B))


@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_chi_m_and_the_improved_estimator_agree_with_the_rotated_heat_bath_and_the_cpu_model(gpu_ops, beta):
    ops = gpu_ops
    Mt = Mx = 16
    lv = _level(Mt, Mx, 1, beta)
    L = slm.Level(Mt, Mx, True, beta)
    B, burn, meas = 512, 100, 300

    x = ops.sigma_level_initialise(lv, B, 41)
    work = ops.sigma_level_sw_workspace(lv, B)
    chi, imp = [], []
    for d in range(burn + meas):
        out = ops.sigma_level_sw_draw(lv, x, 1, 42, 0, d, work=work)
        if d >= burn:
            chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
            imp.append(out[2])
    (w, w_err), (im, im_err) = _chain_means(chi, B), _chain_means(imp, B)

    x = ops.sigma_level_initialise(lv, B, 44)
    scratch = torch.empty_like(x)
    chi = []
    for d in range(burn + meas):
        ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 45, 0, 11 * d)
        if d >= burn:
            chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
    h, h_err = _chain_means(chi, B)
    zcheck(f"sigma level SW chi_m rotated 16x16 beta={beta}: device SW vs device heat bath", w, w_err, h, h_err)
    zcheck(f"sigma level SW rotated 16x16 beta={beta}: improved estimator vs plain chi_m", im, im_err, w, w_err)

    Bc = 48
    phi = slm.initialise(L, Bc, 46)
    chi = []
    for step in range(700):
        phi, _ = slsw.dev_update_batch(L, phi, 47, 0, step)
        if step >= 200:
            chi.append(slm.magnetic_susceptibility(L, phi))
    c = np.mean(chi, axis=0)
    zcheck(f"sigma level SW chi_m rotated 16x16 beta={beta}: device SW vs CPU model chain", w, w_err, float(c.mean()),
           float(c.std(ddof=1) / math.sqrt(Bc)))


def test_hierarchical_chain_with_a_swendsen_wang_coarse_sampler_samples_the_fine_law(gpu_ops):
    """The reason for the feature.  8 x 8, beta = beta_coarse = 1, 4096 chains: the coarse proposals are the successive states of
    one rotated-level Swendsen-Wang chain, ONE draw of K_HIER updates between proposals, then the two-level step, against the
    single-level 10 + 1 heat-bath draw of the same run; zcheck of the two device chains.  Both levels start from 200
    overrelaxation and 20 heat-bath sweeps of their own, so a valid step keeps the fine law from the first draw on.  K_HIER: on
    the CPU models the lag-1 autocorrelation of chi_m on the rotated 8 x 8 level is 0.0780 +- 0.0029 under 20 level-Wolff updates
    per draw (the setting DESIGN.md 7.6 found sufficient) and 0.0827 +- 0.0026 / 0.0735 +- 0.0022 under 17 / 18 Swendsen-Wang
    updates: 18 is the smallest k that is no larger."""
    ops = gpu_ops
    B, beta, n_meas = 4096, 1.0, 60
    lv = _level(8, 8, 0, beta)
    lc = _level(8, 8, 1, beta)
    single = ops.sigma_level_initialise(lv, B, 3, 0)
    fine = ops.sigma_level_initialise(lv, B, 4, 0)
    coarse = ops.sigma_level_initialise(lc, B, 5, 0)
    sf, sc = torch.empty_like(fine), torch.empty_like(coarse)
    ops.sigma_level_sweep_draw(lv, single, sf, 10 * 20, 20, 3, 0, 0)
    ops.sigma_level_sweep_draw(lv, fine, sf, 10 * 20, 20, 4, 0, 0)
    ops.sigma_level_sweep_draw(lc, coarse, sc, 10 * 20, 20, 5, 0, 0)
    work = ops.sigma_level_sw_workspace(lc, B)
    step = ops.SigmaTwoLevelStep(lv, lc, B, seed=6)
    step.set_state(fine)
    tot_two = torch.zeros(B, dtype=torch.float64, device="cuda")
    tot_one = torch.zeros_like(tot_two)
    n_acc = torch.zeros(B, dtype=torch.float64, device="cuda")
    clusters = torch.zeros(B, dtype=torch.float64, device="cuda")
    for k in range(n_meas):
        clusters += ops.sigma_level_sw_draw(lc, coarse, K_HIER, 5, 0, K_HIER * k, work=work)[1]
        n_acc += step.draw(coarse)
        tot_two += ops.sigma_level_magnetic_susceptibility(lv, step.theta)
        ops.sigma_level_sweep_draw(lv, single, sf, 10, 1, 3, 0, 1000 + 11 * k)
        tot_one += ops.sigma_level_magnetic_susceptibility(lv, single)
    two, one = (tot_two / n_meas).cpu().numpy(), (tot_one / n_meas).cpu().numpy()
    rate = float(n_acc.sum()) / (B * n_meas)
    print(f"sigma hierarchical chain 8x8 beta=1, {K_HIER} SW updates per coarse draw: acceptance rate {rate:.4f}, "
          f"{float(clusters.sum()) / (B * n_meas * K_HIER):.2f} clusters per update on 32 vertices")
    assert 0.0 < rate < 1.0
    err = lambda v: v.std(ddof=1) / math.sqrt(B)  # noqa: E731
    zcheck(f"sigma hierarchical chain, {K_HIER} rotated SW updates per proposal, vs 10+1 heat bath, chi_m 8x8 beta=1", two.mean(),
           err(two), one.mean(), err(one))


# ---- driver ---------------------------------------------------------------------------------------------------------------
COMMON = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1"]
COARSE = ["--coarsening", "rotate", "--coarsesampler", "levelsw", "--n_updates", str(K_HIER)]


def _driver(*args):
    exe = os.path.join(ROOT, "host", "driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


def _avg_err(out):
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


def test_driver_hierarchical_with_levelsw_agrees_with_the_heat_bath_sampler():
    h = _driver(*COMMON, *COARSE, "--sampler", "hierarchical", "--n_level", "2", "--n_samples", "6000", "--n_burnin", "200", "--n_meas", "20")
    assert h.returncode == 0, h.stdout[-2000:] + h.stderr[-2000:]
    s = _driver(*COMMON, "--sampler", "heatbath", "--n_samples", "4000", "--n_burnin", "100")
    assert s.returncode == 0, s.stdout[-2000:] + s.stderr[-2000:]
    (ha, he), (sa, se) = _avg_err(h.stdout), _avg_err(s.stdout)
    zcheck(f"host/driver chi_m 8x8 beta=1: hierarchical over levelsw ({K_HIER} updates) vs --sampler heatbath", ha, he, sa, se)


def test_driver_levelsw_on_three_levels_and_in_the_twolevel_method():
    # three levels: 8 x 8, rotated 8 x 8, 4 x 4 -- the Swendsen-Wang sampler runs on the unrotated 4 x 4 level
    k = _driver(*COMMON, *COARSE, "--sampler", "hierarchical", "--n_level", "3", "--n_samples", "200", "--n_burnin", "20", "--n_meas", "10")
    assert k.returncode == 0, k.stdout[-2000:] + k.stderr[-2000:]
    assert "level 2" in k.stdout
    r = _driver(*COMMON, *COARSE, "--sampler", "heatbath", "--method", "twolevel", "--n_samples", "300", "--n_burnin", "50", "--n_meas", "20")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for what in ("QoI[fine]", "QoI[coarse]", "acceptance probability"):
        assert what in r.stdout, (what, r.stdout[-2000:])
    rate = float(re.findall(r"acceptance probability\s+p = ([0-9.]+)", r.stdout)[-1])
    print("two-level acceptance rate over levelsw", rate)
    assert 0.0 < rate < 1.0


def test_driver_swendsenwang_on_an_unrotated_lattice_prints_what_it_printed():
    r = _driver("--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1", "--n_samples", "500", "--n_burnin", "50", "--sampler",
                "swendsenwang", "--n_updates", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _avg_err(r.stdout)
    mi = re.search(r"improved chi_m = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", r.stdout)
    mc = re.search(r"mean clusters per update = ([0-9.eE+-]+)", r.stdout)
    assert mi and mc and "cluster updates per draw = 2" in r.stdout, r.stdout[-2000:]
    assert float(mi.group(1)) > 0 and float(mc.group(1)) > 1.0
