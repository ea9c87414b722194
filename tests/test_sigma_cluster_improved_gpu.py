"""GPU: the improved estimators of the Wolff single-cluster update (mlmcpi_sigma_level_cluster_improved_draw, sigma_cluster.hip)
against their long double reference update by update (tests/sigma_cluster_improved_reference.py), the state against the plain
draw bit for bit, the two identities, the invariances bit for bit, accumulation and guard bands, the argument checks, and the
law against the plain estimators of the same run."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sigma_cluster_improved_reference as wir
import sigma_correlator_reference as cref
import sigma_level_cluster_model as slcm
import sigma_level_model as slm
from conftest import zcheck
from test_sigma_level_cluster_gpu import PLANS, _level, _plan, _thermalised

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _zeros(B, n_out):
    return (torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda"),
            torch.zeros(B, 2, dtype=torch.float64, device="cuda"), torch.zeros(B, n_out, dtype=torch.float64, device="cuda"))


def _draw_into(ops, lv, x, n, seed, chain0, update0, out, work=None, work_bytes=None, structure=True, corr=True, improved=True):
    """mlmcpi_sigma_level_cluster_improved_draw ADDING to out = (sites, improved, structure, corr)"""
    from mlmcpathintegral_amd import abi
    B = x.shape[0]
    work = ops.sigma_level_cluster_improved_workspace(lv, B) if work is None else work
    abi.call("mlmcpi_sigma_level_cluster_improved_draw", C.byref(lv), _p(x), B, n, seed, chain0, update0, _p(out[0]),
             _p(out[1] if improved else None), _p(out[2] if structure else None), _p(out[3] if corr else None), _p(work),
             work.numel() if work_bytes is None else work_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


# ---- parity, update by update, and the two identities ---------------------------------------------------------------------
# singletons (beta so small that no link bonds), mixed (a heat-bath start at beta = 1.5), spanning (an aligned start at beta = 4)
REGIMES = [("singletons", 1e-6), ("mixed", 1.5), ("spanning", 4.0)]


@pytest.mark.parametrize("regime,beta", REGIMES)
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Mt,Mx,B,n", [(2, 2, 4, 4), (2, 6, 4, 4), (6, 2, 4, 4), (4, 4, 4, 4), (16, 16, 3, 3), (66, 34, 3, 2), (130, 70, 3, 2)])
def test_every_update_equals_the_reference(gpu_ops, Mt, Mx, B, n, rot, regime, beta):
    """each device update on the device's own previous state: the state and the count are the bits of the plain draw, the flipped
    set is the model's cluster, and chi^W, F_d^W and every lag of C_d^W lie within the bounds of the reference (absolute, from the
    roundings: 1.5 x 2^-32 per member in a slice sum, the double products and conversions, 2^-(s + 1) per pair of slices).  The two
    identities, sum_tau w C = chi and sum_tau w C cos(2 pi tau / M_d) = F_d, hold within the summed bounds.
    Largest observed |device - reference| / bound: see DESIGN.md 4.6a (a record, not a gate)."""
    ops = gpu_ops
    L = slm.Level(Mt, Mx, rot, beta)
    lv = _level(Mt, Mx, int(rot), beta)
    seed, chain0, update0 = 5000 + Mt + Mx, 3, 40
    if regime == "spanning":
        x = ops.sigma_level_initialise(lv, B, seed)
        x[:, 0::2], x[:, 1::2] = 0.5 * math.pi, 0.25
    elif regime == "singletons":
        x = ops.sigma_level_initialise(lv, B, seed)
    else:
        x = _thermalised(ops, lv, B, seed)
    work = ops.sigma_level_cluster_improved_workspace(lv, B)
    largest, smallest, worst = 0, L.n, 0.0
    for k in range(n):
        before = x.cpu().numpy()
        y = x.clone()
        plain = ops.sigma_level_cluster_draw(lv, y, 1, seed, chain0, update0 + k)
        sites, chi, F, corr = (t.cpu().numpy() for t in ops.sigma_level_cluster_improved_draw(lv, x, 1, seed, chain0, update0 + k, work=work,
                                                                                            structure=True, correlator=True))
        assert torch.equal(x, y) and np.array_equal(sites, plain.cpu().numpy())
        after = x.cpu().numpy()
        for b in range(B):
            _, info = slcm.dev_update(L, before[b], seed, chain0 + b, update0 + k)
            assert info["margin"] > 1e-10, "a bond decision within 1e-10 of its uniform: change the seed"
            members = info["sites"]
            changed = np.nonzero(np.any(after[b].reshape(L.n, 2) != before[b].reshape(L.n, 2), axis=1))[0]
            assert np.array_equal(changed, members), (k, b, len(changed), len(members))
            assert sites[b] == len(members)
            a = wir.dots(L, before[b], info["r"])
            rchi, rF, rC = wir.estimators(L, a, members)
            bchi, bC = wir.susceptibility_bound(L, a, members), wir.device_bound(L, a, members)
            bF = [wir.structure_bound(L, a, members, d) for d in range(2)]
            err = np.abs(corr[b].astype(LD) - rC).astype(np.float64)
            ratios = [abs(float(LD(chi[b]) - rchi)) / bchi] + [abs(float(LD(F[b, d]) - rF[d])) / bF[d] for d in range(2)]
            ratios.append(float(np.divide(err, bC, out=np.zeros_like(err), where=bC > 0).max()))   # bound = 0: the cluster reaches no such lag
            worst = max(worst, max(ratios))
            print(f"rot={rot} {Mt}x{Mx} {regime} update {k} chain {b}: cluster {len(members)}, chi {chi[b]:.15g} vs {float(rchi):.15g}, "
                  f"|diff| / bound: chi {ratios[0]:.3g}, F {max(ratios[1:3]):.3g}, C {ratios[3]:.3g}")
            assert ratios[0] <= 1.0 and ratios[1] <= 1.0 and ratios[2] <= 1.0, (k, b, chi[b], rchi, F[b], rF)
            assert np.all(err <= bC), (k, b, corr[b], rC, bC)
            if regime == "singletons":
                assert abs(chi[b] - 3.0 * a[members[0]] ** 2) <= bchi
            for d, (M, lo) in enumerate(((Mt, 0), (Mx, Mt // 2 + 1))):
                w = cref.weights(M).astype(LD)
                cos = wir.slice_phases(M)[0][:M // 2 + 1]
                Cd, bd = corr[b, lo:lo + M // 2 + 1].astype(LD), bC[lo:lo + M // 2 + 1]
                assert abs(float((w * Cd).sum() - LD(chi[b]))) <= float((w * bd).sum()) + bchi, (k, b, d)
                assert abs(float((w * Cd * cos).sum() - LD(F[b, d]))) <= float((w * bd * np.abs(cos)).sum()) + bF[d], (k, b, d)
            largest, smallest = max(largest, len(members)), min(smallest, len(members))
    print(f"[wolff improved] rot={rot} {Mt}x{Mx} {regime}: largest |device - reference| / bound = {worst:.4f}")
    if regime == "singletons":
        assert largest == 1, "every cluster a single vertex"
    elif regime == "spanning":
        assert largest > L.n // 2, "a cluster across the level"
    elif L.n > 2:
        assert largest > 1 and smallest < L.n, "a kernel that bonds nothing, or everything, must not pass"


# ---- invariances, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B,beta,rot", [(16, 16, 8, 1.0, 1), (66, 34, 4, 1.5, 1), (16, 16, 8, 1.5, 0), (66, 34, 4, 1.5, 0)])
def test_plans_call_split_batch_split_and_optional_outputs_give_the_same_bits(gpu_ops, Mt, Mx, B, beta, rot):
    ops = gpu_ops
    lv = _level(Mt, Mx, rot, beta)
    n, n_out = 10, cref.n_out(Mt, Mx)
    seed, chain0, update0 = 291 + Mt, 5, 1000
    x0 = _thermalised(ops, lv, B, seed)
    ref, out = x0.clone(), _zeros(B, n_out)
    _draw_into(ops, lv, ref, n, seed, chain0, update0, out)
    assert not torch.equal(ref, x0) and (out[1] > 0).all() and (out[3][:, 0] > 0).all()

    y = x0.clone()                                                   # the plain draw: the same state and count
    assert torch.equal(ops.sigma_level_cluster_draw(lv, y, n, seed, chain0, update0), out[0]) and torch.equal(y, ref)

    for first in (5, 1):                                             # 10 = 5 + 5 and 4 = 1 + 3 (+ 6), into the same accumulators
        a, acc, k = x0.clone(), _zeros(B, n_out), 0
        for part in ((5, 5) if first == 5 else (1, 3, 6)):
            _draw_into(ops, lv, a, part, seed, chain0, update0 + k, acc)
            k += part
        assert torch.equal(a, ref) and _same(acc, out), first

    h = B // 2 - 1                                                   # the batch in two parts, the second at its chain0 offset
    lo, hi, olo, ohi = x0[:h].clone(), x0[h:].clone(), _zeros(h, n_out), _zeros(B - h, n_out)
    _draw_into(ops, lv, lo, n, seed, chain0, update0, olo)
    _draw_into(ops, lv, hi, n, seed, chain0 + h, update0, ohi)
    assert torch.equal(torch.cat([lo, hi]), ref) and _same([torch.cat(p) for p in zip(olo, ohi)], out)

    for team, bitmap in PLANS:                                       # the wave team forced by the knob: B is far below its threshold
        with _plan(team, bitmap):
            y, o = x0.clone(), _zeros(B, n_out)
            _draw_into(ops, lv, y, n, seed, chain0, update0, o)
        assert torch.equal(y, ref) and _same(o, out), (team, bitmap)

    for structure, corr in ((False, False), (True, False), (False, True)):   # without the optional outputs: the others unchanged
        y, o = x0.clone(), _zeros(B, n_out)
        _draw_into(ops, lv, y, n, seed, chain0, update0, o, structure=structure, corr=corr)
        assert torch.equal(y, ref) and torch.equal(o[0], out[0]) and torch.equal(o[1], out[1])
        assert torch.equal(o[2], out[2] if structure else torch.zeros_like(o[2]))
        assert torch.equal(o[3], out[3] if corr else torch.zeros_like(o[3]))
    got = ops.sigma_level_cluster_improved_draw(lv, x0.clone(), n, seed, chain0, update0, structure=True, correlator=True)
    assert _same(got, out)
    assert len(ops.sigma_level_cluster_improved_draw(lv, x0.clone(), n, seed, chain0, update0)) == 2


@pytest.mark.parametrize("Mt,Mx,rot", [(16, 16, 0), (16, 16, 1), (66, 34, 0), (66, 34, 1)])
def test_three_hundred_chains_in_one_call_equal_seven_and_the_rest(gpu_ops, Mt, Mx, rot):
    ops, B = gpu_ops, 300
    lv = _level(Mt, Mx, rot, 1.5)
    n_out = cref.n_out(Mt, Mx)
    x0 = _thermalised(ops, lv, B, 17)
    ref, out = x0.clone(), _zeros(B, n_out)
    _draw_into(ops, lv, ref, 2, 18, 2, 7, out)
    lo, hi, olo, ohi = x0[:7].clone(), x0[7:].clone(), _zeros(7, n_out), _zeros(B - 7, n_out)
    _draw_into(ops, lv, lo, 2, 18, 2, 7, olo)
    _draw_into(ops, lv, hi, 2, 18, 2 + 7, 7, ohi)
    assert torch.equal(torch.cat([lo, hi]), ref) and _same([torch.cat(p) for p in zip(olo, ohi)], out)
    with _plan("wave", "lds"):
        y, o = x0.clone(), _zeros(B, n_out)
        _draw_into(ops, lv, y, 2, 18, 2, 7, o)
    assert torch.equal(y, ref) and _same(o, out)


# ---- accumulation and guard bands -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("team", ["wave", "block"])
@pytest.mark.parametrize("rot", [1, 0])
def test_the_accumulators_are_added_to_and_nothing_else_is_written(gpu_ops, rot, team):
    """guard bands round every output and the workspace, the workspace full of 0xA5 at entry; two calls of one update each into the
    same arrays (one add per update to the count, chi and every lag, so start + first + second in that order is what the device forms)"""
    ops, B, G = gpu_ops, 5, 512
    lv = _level(6, 10, rot, 1.5)
    n_out = cref.n_out(6, 10)
    x0 = _thermalised(ops, lv, B, 9)
    need = ops.sigma_level_cluster_improved_workspace(lv, B).numel()
    with _plan(team, ""):
        first = ops.sigma_level_cluster_improved_draw(lv, x0.clone(), 1, 10, 1, 3, structure=True, correlator=True)
        x1 = x0.clone()
        ops.sigma_level_cluster_draw(lv, x1, 1, 10, 1, 3)
        second = ops.sigma_level_cluster_improved_draw(lv, x1.clone(), 1, 10, 1, 4, structure=True, correlator=True)
        sizes = (B, B, 2 * B, B * n_out)
        bufs = [torch.full((G + s + G,), -7.25 if i else -7, dtype=torch.float64 if i else torch.int32, device="cuda") for i, s in enumerate(sizes)]
        views = [b[G:G + s] for b, s in zip(bufs, sizes)]
        starts = []
        for i, v in enumerate(views):
            v.copy_((torch.arange(v.numel(), device="cuda") * (0.125 if i else 3)).to(v.dtype))
            starts.append(v.clone())
        out = (views[0], views[1], views[2].view(B, 2), views[3].view(B, n_out))
        wbuf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        x = x0.clone()
        _draw_into(ops, lv, x, 1, 10, 1, 3, out, work=wbuf[256:256 + need])
        _draw_into(ops, lv, x, 1, 10, 1, 4, out, work=wbuf[256:256 + need])
    for i, (v, s, f1, f2) in enumerate(zip(views, starts, first, second)):
        want = (s + f1.reshape(-1)) + f2.reshape(-1)
        if i == 2:    # F takes two adds an update (cos, then sin): four adds here against two, each within 2^-53 of its partial sum
            assert ((v - want).abs() <= 8 * 2.0 ** -53 * (s.abs() + f1.reshape(-1) + f2.reshape(-1))).all()
        else:
            assert torch.equal(v, want), i
    for b, s in zip(bufs, sizes):
        fill = -7.25 if b.dtype == torch.float64 else -7
        assert (b[:G] == fill).all() and (b[G + s:] == fill).all()
    assert (wbuf[:256] == 0xA5).all() and (wbuf[256 + need:] == 0xA5).all()


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing(gpu_ops):
    from mlmcpathintegral_amd import abi
    ops, B = gpu_ops, 3
    lv = _level(16, 16, 1, 1.0)
    n_out = cref.n_out(16, 16)
    x = ops.sigma_level_initialise(lv, B, 3)
    x0 = x.clone()
    work = ops.sigma_level_cluster_improved_workspace(lv, B)
    plain = ops.sigma_level_cluster_workspace(lv, B).numel()
    a256 = lambda v: -(-v // 256) * 256  # noqa: E731
    assert work.numel() == plain + a256(B * 32 * 8) + a256(B * (5 + n_out) * 8) + a256(B * 32 * 4) + a256(B * 32 * 16)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(level, state, nb, n, update0, improved, wk, wbytes, out):
        with pytest.raises(abi.MlmcpiError, match="status -1"):
            abi.call("mlmcpi_sigma_level_cluster_improved_draw", C.byref(level) if level is not None else None, _p(state), nb, n, 1, 0,
                     update0, _p(out[0]), _p(improved), _p(out[2]), _p(out[3]), _p(wk), wbytes, stream)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and _same(out, _zeros(B, n_out))           # nothing was launched

    out = _zeros(B, n_out)
    refused(lv, x, B, 1, 0, None, work, work.numel(), out)                   # NULL d_improved
    refused(lv, x, B, 1, 0, out[1], work, work.numel() - 1, out)             # a short workspace
    refused(lv, x, B, 1, 0, out[1], work, plain, out)                        # the plain draw's workspace
    refused(lv, x, B, 1, 0, out[1], None, work.numel(), out)                 # no workspace
    refused(lv, None, B, 1, 0, out[1], work, work.numel(), out)              # no state
    refused(lv, x, 0, 1, 0, out[1], work, work.numel(), out)                 # B = 0
    refused(lv, x, B, 2, 0xFFFFFFFF, out[1], work, work.numel(), out)        # the update counter overflows
    refused(None, x, B, 1, 0, out[1], work, work.numel(), out)               # NULL level
    for Mt, Mx, beta in ((15, 16, 1.0), (16, 15, 1.0), (0, 16, 1.0), (16, 16, 0.0), (16, 16, -1.0)):
        for rot in (0, 1):
            refused(_level(Mt, Mx, rot, beta), x, B, 1, 0, out[1], work, work.numel(), out)
            with pytest.raises(abi.MlmcpiError, match="status -1"):
                abi.call("mlmcpi_sigma_level_cluster_improved_workspace_bytes", C.byref(_level(Mt, Mx, rot, beta)), B, C.byref(C.c_size_t(0)))


# ---- statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot,beta", [(0, 1.0), (1, 1.5)])
def test_the_improved_estimators_have_the_law_of_the_plain_ones(gpu_ops, rot, beta):
    """16 x 16 (beta = 1) and its rotated partner (beta = 1.5), 256 chains, seed 52, 100 + 200 draws of 10 updates: per chain the mean
    over the run of the improved chi_m and C_t(tau) (per update) and of the plain estimators (mlmcpi_sigma_level_magnetic_
    susceptibility, mlmcpi_sigma_level_correlator) on the state before each draw; chi_m and each of the 9 lags within 5 combined
    standard errors, the errors from the spread over the chains.  The ratio of the spreads is printed and recorded in DESIGN.md
    7.10, not asserted."""
    ops = gpu_ops
    Mt = Mx = 16
    lv = _level(Mt, Mx, rot, beta)
    B, burn, meas, per = 256, 100, 200, 10
    x = ops.sigma_level_initialise(lv, B, 51)
    work = ops.sigma_level_cluster_improved_workspace(lv, B)
    n_out = cref.n_out(Mt, Mx)
    imp_c, pl_c = (torch.zeros(B, n_out, dtype=torch.float64, device="cuda") for _ in range(2))
    imp_chi, pl_chi = (torch.zeros(B, dtype=torch.float64, device="cuda") for _ in range(2))
    for d in range(burn + meas):
        if d >= burn:
            pl_c += ops.sigma_level_correlator(lv, x)
            pl_chi += ops.sigma_level_magnetic_susceptibility(lv, x)
        out = ops.sigma_level_cluster_improved_draw(lv, x, per, 52, 0, per * d, work=work, correlator=True)
        if d >= burn:
            imp_chi += out[1] / per
            imp_c += out[2] / per
    imp_c, pl_c, imp_chi, pl_chi = ((t / meas).cpu().numpy() for t in (imp_c, pl_c, imp_chi, pl_chi))
    err = lambda v: float(v.std(ddof=1) / math.sqrt(B))  # noqa: E731
    tag = f"sigma Wolff improved {'rotated' if rot else 'unrotated'} 16x16 beta={beta}"
    print(f"{tag}: chain spread of chi_m, improved / plain = {imp_chi.std(ddof=1) / pl_chi.std(ddof=1):.4f}")
    for k in range(Mt // 2 + 1):
        print(f"{tag}: chain spread of C_t({k}), improved / plain = {imp_c[:, k].std(ddof=1) / pl_c[:, k].std(ddof=1):.4f}")
    zcheck(f"{tag}: improved vs plain chi_m", float(imp_chi.mean()), err(imp_chi), float(pl_chi.mean()), err(pl_chi), gate=5.0)
    for k in range(Mt // 2 + 1):
        zcheck(f"{tag}: improved vs plain C_t({k})", float(imp_c[:, k].mean()), err(imp_c[:, k]), float(pl_c[:, k].mean()), err(pl_c[:, k]), gate=5.0)
