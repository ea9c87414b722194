"""First measurements of the Wolff single-cluster update on ROTATED levels of the O(3) sigma model
(mlmcpi_sigma_level_cluster_draw, sigma_cluster.hip), one process on one GPU, after the pattern of
tools/exp_sigma_cluster.py.  Shapes: the rotated partner of 64^2 x 4096 chains (n = 2048 vertices) and of 1024^2 x 32 chains
(n = 524 288), beta = 1.0 and 1.5, states thermalised with rotated heat-bath draws and then cluster draws.  Per setting: ms
per draw of k = 10 updates (HIP events, median of 20 draws after 5 warm-up draws), flipped vertices per update, vertex flips
per second, and for the Wolff draw and the rotated 10 + 1 sweep draw the integrated autocorrelation time of chi_m
(autocovariances pooled over the chains, summed up to a window of 6 tau; a lower bound where the window is cut) and tau_int x
ms per draw, the time per independent chi_m sample.  Writes profiles/sigma_level_cluster.json.  Records, not gates.

  python tools/exp_sigma_level_cluster.py [--out profiles/sigma_level_cluster.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

SEED, N_UPDATES, N_OR, N_HB, WARMUP, DRAWS = 20240911, 10, 10, 1, 5, 20


def timed(fn, first, warmup=WARMUP, draws=DRAWS):
    for d in range(first, first + warmup):
        fn(d)
    torch.cuda.synchronize()
    ms = []
    for d in range(first + warmup, first + warmup + draws):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(d)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_per_draw": statistics.median(ms), "min": min(ms), "max": max(ms), "draws": draws, "warmup": warmup}


def tau_int(series):
    """series [draws, chains] -> (tau_int, window, cut): autocovariances averaged over the chains, tau = 1 + 2 sum_{k <= W} rho(k),
    W the first lag with W >= 6 tau(W); cut = the window reached a quarter of the run first (tau is then a lower bound)"""
    x = series - series.mean(dim=0, keepdim=True)
    n = x.shape[0]
    c0 = (x * x).mean().item()
    tau, k = 1.0, 0
    for k in range(1, n // 4):
        tau += 2.0 * (x[:-k] * x[k:]).mean().item() / c0
        if k >= 6.0 * tau:
            return tau, k, False
    return tau, k, True


def setting(M, B, beta, therm_draws, tau_draws):
    lv = abi.sigma_level(M, M, 1, beta)
    nvert = M * M // 2
    x = ops.sigma_level_initialise(lv, B, SEED)
    scratch = torch.empty_like(x)
    work = ops.sigma_level_cluster_workspace(lv, B)
    for d in range(therm_draws):
        ops.sigma_level_sweep_draw(lv, x, scratch, N_OR, N_HB, SEED, 0, 11 * d)
    heat = lambda d: ops.sigma_level_sweep_draw(lv, x, scratch, N_OR, N_HB, SEED, 0, 11 * d)  # noqa: E731
    wolff = lambda d: ops.sigma_level_cluster_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, count=False, work=work)  # noqa: E731
    for d in range(50):
        wolff(d)
    rec = {"Mt": M, "Mx": M, "rotated": True, "vertices": nvert, "chains": B, "beta": beta, "updates_per_draw": N_UPDATES, "thermalisation_heatbath_draws": therm_draws}
    rec["wolff"] = timed(wolff, 50)
    count = torch.zeros(B, dtype=torch.int64, device="cuda")
    first, n = 50 + WARMUP + DRAWS, 20
    for d in range(first, first + n):
        count += ops.sigma_level_cluster_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=work).long()
    per_update = count.double().mean().item() / (n * N_UPDATES)
    rec["flipped_vertices_per_update"] = per_update
    rec["share_of_level_per_update"] = per_update / nvert
    rec["vertex_flips_per_s"] = per_update * N_UPDATES * B / (rec["wolff"]["ms_per_draw"] * 1e-3)
    rec["heatbath_10_plus_1"] = timed(heat, therm_draws)
    if tau_draws:
        for name, fn, first in (("wolff", wolff, first + n), ("heatbath_10_plus_1", heat, therm_draws + WARMUP + DRAWS)):
            chi = torch.stack([(fn(d), ops.sigma_level_magnetic_susceptibility(lv, x))[1] for d in range(first, first + tau_draws)])
            tau, window, cut = tau_int(chi)
            rec[name]["chi_m_mean"] = chi.mean().item()
            rec[name]["tau_int_chi_m_draws"] = tau
            rec[name]["tau_window_draws"] = window
            rec[name]["tau_is_lower_bound"] = cut
            rec[name]["tau_draws_recorded"] = tau_draws
            rec[name]["tau_int_x_ms_per_draw"] = tau * rec[name]["ms_per_draw"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_level_cluster.json"))
    ap.add_argument("--quick", action="store_true", help="small chain counts and short runs (a functional check, not a measurement)")
    a = ap.parse_args()
    q = 16 if a.quick else 1
    settings = [(64, 4096 // q, beta, 40 // q + 2, 600 // q) for beta in (1.0, 1.5)] + [(1024, 32 // q, beta, 20 // q + 2, 240 // q) for beta in (1.0, 1.5)]
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "hip events, median of %d draws after %d warm-up draws, one process; first measurements, records not gates" % (DRAWS, WARMUP),
           "settings": [setting(*s) for s in settings]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
