"""GPU: the cluster-improved structure factor of the Swendsen-Wang update (mlmcpi_sigma_level_sw_structure_draw, sigma_sw.hip)
against its long double reference update by update (tests/sigma_sw_structure_reference.py), its invariances bit for bit, the
chain plan at its capacity, its argument checks and its law against the plain structure factor of the time-slice correlator."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sigma_level_model as slm
import sigma_level_sw_model as slsw
import sigma_sw_structure_reference as ssr
from conftest import zcheck
from test_sigma_level_sw_gpu import CHAIN_MAX_N, _level, _plan, _same, _thermalised

pytestmark = pytest.mark.gpu


def _draw_into(ops, lv, x, n, seed, chain0, update0, out, work=None, work_bytes=None, structure=True):
    """mlmcpi_sigma_level_sw_structure_draw ADDING to out = (flipped, clusters, improved, structure)"""
    from mlmcpathintegral_amd import abi
    B = x.shape[0]
    work = ops.sigma_level_sw_structure_workspace(lv, B) if work is None else work
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
    abi.call("mlmcpi_sigma_level_sw_structure_draw", C.byref(lv), p(x), B, n, seed, chain0, update0, p(out[0]), p(out[1]), p(out[2]),
             p(out[3] if structure else None), p(work), work.numel() if work_bytes is None else work_bytes,
             C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _zeros(B):
    return (torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
            torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, 2, dtype=torch.float64, device="cuda"))


# ---- parity, update by update ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "tiled8x8"])
@pytest.mark.parametrize("beta", [1.0, 1.5])
@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("Mt,Mx,B,n", [(2, 2, 5, 8), (2, 6, 5, 8), (4, 6, 5, 8), (16, 16, 4, 6), (66, 34, 3, 4), (130, 70, 3, 3)])
def test_every_update_equals_the_reference(gpu_ops, Mt, Mx, B, n, rot, beta, mode):
    """each device update against the reference on the model's clusters of the device's own previous state.  The bound is
    absolute and comes from the fixed point (ssr.device_bound, where the derivation is): per vertex half a unit 2^-32 of rounding
    and one unit where a libm ulp moves it, so a cluster sum is off by at most 1.5 n_C 2^-32 and a direction by
    3 x (3 / n) sum_C n_C sum_C |a| 2^-31 plus second order and the rounding of the double sums.  The seeds (3000 + Mt + 10 beta, those
    of the update's own parity test) clear the margin 1e-10 in every case, which is asserted, not skipped.  The state and the
    three old outputs are asserted against the model as that test asserts them.  Largest observed |device - reference| / bound
    over the 48 cases: 0.151 (one run on an MI355X)."""
    ops = gpu_ops
    L = slm.Level(Mt, Mx, rot, beta)
    lv = _level(Mt, Mx, int(rot), beta)
    seed, chain0, update0 = 3000 + Mt + int(10 * beta), 3, 40
    x = _thermalised(ops, lv, B, seed)
    work = ops.sigma_level_sw_structure_workspace(lv, B)
    largest, most, worst = 0, 0, 0.0
    with _plan(*(("", "") if mode == "default" else ("tiled", "8x8"))):
        for k in range(n):
            before = x.cpu().numpy()
            flipped, clusters, improved, F = (t.cpu().numpy() for t in ops.sigma_level_sw_draw(lv, x, 1, seed, chain0, update0 + k, work=work,
                                                                                              structure=True))
            after = x.cpu().numpy()
            for b in range(B):
                want, info = slsw.dev_update(L, before[b], seed, chain0 + b, update0 + k)
                sizes = np.bincount(info["labels"])
                assert info["margin"] > 1e-10, "a bond decision within 1e-10 of its uniform: change the seed"
                changed = np.nonzero(np.any(after[b].reshape(L.n, 2) != before[b].reshape(L.n, 2), axis=1))[0]
                assert np.array_equal(changed, info["flipped"]), (k, b, len(changed), len(info["flipped"]))
                assert flipped[b] == len(info["flipped"]) and clusters[b] == info["clusters"]
                assert abs(improved[b] - info["improved"]) <= 1e-9 * info["improved"]
                for d in range(2):
                    ref, bound = float(ssr.improved(L, info["a"], info["labels"], d)), ssr.device_bound(L, info["a"], info["labels"], d)
                    err = abs(F[b, d] - ref)
                    worst = max(worst, err / bound)
                    print(f"rot={rot} {Mt}x{Mx} beta={beta} update {k} chain {b} d={d}: F {F[b, d]:.15g} vs {ref:.15g}, |diff| {err:.3g}, "
                          f"bound {bound:.3g}, {info['clusters']} clusters, largest {sizes.max()}")
                    assert err <= bound, (k, b, d, F[b, d], ref, bound)
                largest, most = max(largest, int(sizes.max())), max(most, info["clusters"])
    print(f"[structure] rot={rot} {Mt}x{Mx} beta={beta} {mode}: largest |device - reference| / bound = {worst:.4f}")
    assert largest > 1 and most >= 2, "a kernel that bonds nothing, or everything, must not pass"


# ---- invariances, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mt,Mx,B,beta,rot", [(2, 2, 8, 1.5, 1), (16, 16, 8, 1.0, 1), (130, 70, 4, 1.5, 1), (512, 300, 4, 1.5, 1),
                                              (1024, 1024, 4, 1.5, 1), (16, 16, 8, 1.5, 0), (130, 70, 4, 1.5, 0)])
def test_call_split_batch_split_plans_and_tiles_give_the_same_bits(gpu_ops, Mt, Mx, B, beta, rot):
    ops = gpu_ops
    lv = _level(Mt, Mx, rot, beta)
    nv, n = (Mt * Mx // 2 if rot else Mt * Mx), 10
    seed, chain0, update0 = 191 + Mt, 5, 1000
    x0 = _thermalised(ops, lv, B, seed, aligned=Mt == 1024)
    ref, out = x0.clone(), _zeros(B)
    _draw_into(ops, lv, ref, n, seed, chain0, update0, out)
    print(f"rot={rot} {Mt} x {Mx} beta = {beta}: per update improved chi_m {out[2].mean().item() / n:.6g}, F_t {out[3][:, 0].mean().item() / n:.6g}, "
          f"F_x {out[3][:, 1].mean().item() / n:.6g}")
    assert not torch.equal(ref, x0) and (out[3] > 0).all()

    y = x0.clone()                                                   # the update without structure: the same state and outputs
    old = ops.sigma_level_sw_draw(lv, y, n, seed, chain0, update0)
    assert torch.equal(y, ref) and _same(old, out[:3])

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


# ---- the chain plan at its capacity ---------------------------------------------------------------------------------------
def test_the_chain_plan_runs_at_its_capacity_and_is_refused_beyond(gpu_ops):
    from mlmcpathintegral_amd import abi
    ops, B = gpu_ops, 2
    lv = _level(122, 122, 1, 1.5)                                    # n = 7442 of 7552
    x0 = _thermalised(ops, lv, B, 7)
    res = {}
    for plan in ("chain", "tiled"):
        with _plan(plan, ""):
            y, o = x0.clone(), _zeros(B)
            _draw_into(ops, lv, y, 3, 8, 1, 20, o)
        res[plan] = (y, o)
    assert torch.equal(res["chain"][0], res["tiled"][0]) and _same(res["chain"][1], res["tiled"][1])
    assert not torch.equal(res["chain"][0], x0) and (res["chain"][1][3] > 0).all()

    lv = _level(512, 300, 1, 1.5)
    x = ops.sigma_level_initialise(lv, 1, 3)
    x0 = x.clone()
    with _plan("chain", ""):
        with pytest.raises(abi.MlmcpiError, match="status -3"):
            ops.sigma_level_sw_draw(lv, x, 1, 1, 0, 0, structure=True)
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
    need = ops.sigma_level_sw_structure_workspace(lv, B).numel()
    with _plan(plan, tile):
        ref, want = x0.clone(), _zeros(B)
        _draw_into(ops, lv, ref, n, 10, 1, 3, want, work=torch.zeros(need, dtype=torch.uint8, device="cuda"))
        wbuf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        x, out = x0.clone(), _zeros(B)
        _draw_into(ops, lv, x, n, 10, 1, 3, out, work=wbuf[256:256 + need])
    assert (wbuf[:256] == 0xA5).all() and (wbuf[256 + need:] == 0xA5).all()
    assert torch.equal(x, ref) and _same(out, want)
    assert not torch.equal(ref, x0) and (want[3] > 0).all()


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_a_short_workspace_and_a_null_accumulator_are_invalid(gpu_ops):
    from mlmcpathintegral_amd import abi
    ops, B = gpu_ops, 3
    lv = _level(16, 16, 1, 1.0)
    x = ops.sigma_level_initialise(lv, B, 3)
    x0 = x.clone()
    work = ops.sigma_level_sw_structure_workspace(lv, B)
    assert work.numel() == ops.sigma_level_sw_workspace(lv, B).numel() + 4 * (-(-B * 128 * 8 // 256) * 256)
    for kwargs in ({"work_bytes": ops.sigma_level_sw_workspace(lv, B).numel()}, {"structure": False}):
        out = _zeros(B)
        with pytest.raises(abi.MlmcpiError, match="status -1"):
            _draw_into(ops, lv, x, 1, 1, 0, 0, out, work=work, **kwargs)
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and _same(out, _zeros(B)), kwargs                # nothing was launched


# ---- statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [1.0, 1.5])
@pytest.mark.parametrize("rot", [1, 0])
def test_the_improved_structure_factor_and_xi_agree_with_the_plain_ones(gpu_ops, rot, beta):
    """16 x 16, 512 chains, 100 + 300 updates: the mean improved F_d against the plain F_d = sum_tau w C_d(tau) cos(2 pi tau / M) of
    mlmcpi_sigma_level_correlator on the state before each update, and xi_2 = sqrt(chi / F - 1) / (2 sin(pi / M)) from the
    chain-averaged improved (chi, F) against that from the plain ones, each with a jackknife over the chains"""
    import sigma_correlator_reference as cref
    ops = gpu_ops
    Mt = Mx = 16
    lv = _level(Mt, Mx, rot, beta)
    B, burn, meas = 512, 100, 300
    x = ops.sigma_level_initialise(lv, B, 41)
    work = ops.sigma_level_sw_structure_workspace(lv, B)
    w = torch.tensor(cref.weights(Mt), device="cuda")
    cosw = w * torch.cos(2.0 * math.pi * torch.arange(Mt // 2 + 1, device="cuda", dtype=torch.float64) / Mt)
    acc = torch.zeros(6, B, dtype=torch.float64, device="cuda")      # improved chi, F_t, F_x; plain chi, F_t, F_x
    for d in range(burn + meas):
        if d >= burn:
            Ct, Cx = cref.split(ops.sigma_level_correlator(lv, x), Mt, Mx)
            acc[3] += (Ct * w).sum(dim=1)
            acc[4] += (Ct * cosw).sum(dim=1)
            acc[5] += (Cx * cosw).sum(dim=1)
        out = ops.sigma_level_sw_draw(lv, x, 1, 42, 0, d, work=work, structure=True)
        if d >= burn:
            acc[0] += out[2]
            acc[1:3] += out[3].T
    m = (acc / meas).cpu().numpy()
    err = lambda v: float(v.std(ddof=1) / math.sqrt(B))  # noqa: E731

    def xi(chi, F):
        """xi_2 of the chain means and its jackknife error over the chains"""
        f = lambda c, g: math.sqrt(c / g - 1.0) / (2.0 * math.sin(math.pi / Mt))  # noqa: E731
        full = f(chi.mean(), F.mean())
        jk = np.array([f((chi.sum() - chi[b]) / (B - 1), (F.sum() - F[b]) / (B - 1)) for b in range(B)])
        return full, math.sqrt((B - 1) / B * ((jk - jk.mean()) ** 2).sum())

    tag = f"sigma SW structure {'rotated' if rot else 'unrotated'} 16x16 beta={beta}"
    zcheck(f"{tag}: improved chi_m vs plain", float(m[0].mean()), err(m[0]), float(m[3].mean()), err(m[3]))
    for d, name in ((1, "t"), (2, "x")):
        zcheck(f"{tag}: improved F_{name} vs plain F_{name}", float(m[d].mean()), err(m[d]), float(m[3 + d].mean()), err(m[3 + d]))
        (xi_i, e_i), (xi_p, e_p) = xi(m[0], m[d]), xi(m[3], m[3 + d])
        print(f"{tag}: xi_2({name}) improved {xi_i:.5f} +- {e_i:.2g}, plain {xi_p:.5f} +- {e_p:.2g}")
        zcheck(f"{tag}: improved xi_2({name}) vs plain", xi_i, e_i, xi_p, e_p)
