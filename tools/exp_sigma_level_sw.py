"""First measurements of the Swendsen-Wang update on ROTATED levels of the O(3) sigma model (mlmcpi_sigma_level_sw_draw,
sigma_sw.hip), one process on one GPU, after the pattern of tools/exp_sigma_level_cluster.py.  Shapes: the rotated
partner of 64^2 x 4096 chains (n = 2048 vertices, chain plan) and of 1024^2 x 32 chains (n = 524 288, tiled plan), beta = 1.0
and 1.5, states thermalised with rotated heat-bath draws and then Swendsen-Wang updates.  Per setting, for a draw of ONE
Swendsen-Wang update (outputs asked for), a draw of 10 level-Wolff updates and the rotated 10 + 1 sweep draw: ms per draw (HIP
events, median of 20 draws after 5 warm-up draws), the integrated autocorrelation time of chi_m in draws (autocovariances
pooled over the chains, summed up to a window of 6 tau; a lower bound where the window is cut) and tau_int x ms per draw, the
time per independent chi_m sample; for the Swendsen-Wang draw the same for its improved estimator, and clusters and flipped
vertices per update.  Writes profiles/sigma_level_sw.json.  Records, not gates.

  python tools/exp_sigma_level_sw.py [--out profiles/sigma_level_sw.json] [--quick]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402
from exp_sigma_level_cluster import DRAWS, WARMUP, tau_int, timed  # noqa: E402

SEED, N_WOLFF, N_OR, N_HB = 20240912, 10, 10, 1


def setting(M, B, beta, therm_draws, tau_draws):
    lv = abi.sigma_level(M, M, 1, beta)
    nvert = M * M // 2
    x = ops.sigma_level_initialise(lv, B, SEED)
    scratch = torch.empty_like(x)
    work_sw = ops.sigma_level_sw_workspace(lv, B)
    work_wolff = ops.sigma_level_cluster_workspace(lv, B)
    last = {}

    def heat(d):
        ops.sigma_level_sweep_draw(lv, x, scratch, N_OR, N_HB, SEED, 0, 11 * d)

    def wolff(d):
        ops.sigma_level_cluster_draw(lv, x, N_WOLFF, SEED + 1, 0, N_WOLFF * d, count=False, work=work_wolff)

    def sw(d):
        last["out"] = ops.sigma_level_sw_draw(lv, x, 1, SEED + 2, 0, d, work=work_sw)

    for d in range(therm_draws):
        heat(d)
    for d in range(50):
        sw(d)
    rec = {"Mt": M, "Mx": M, "rotated": True, "vertices": nvert, "chains": B, "beta": beta, "thermalisation_heatbath_draws": therm_draws}
    first = {"swendsenwang_1_update": 50, "wolff_10_updates": 0, "heatbath_10_plus_1": therm_draws}
    for name, fn in (("swendsenwang_1_update", sw), ("wolff_10_updates", wolff), ("heatbath_10_plus_1", heat)):
        r = timed(fn, first[name])
        start = first[name] + WARMUP + DRAWS
        chi, imp, flipped, clusters = [], [], 0.0, 0.0
        for d in range(start, start + tau_draws):
            fn(d)
            chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
            if fn is sw:
                imp.append(last["out"][2])
                flipped += last["out"][0].double().mean().item()
                clusters += last["out"][1].double().mean().item()
        series = {"chi_m": torch.stack(chi)}
        if imp:
            series["improved"] = torch.stack(imp)
            r["flipped_vertices_per_update"] = flipped / tau_draws
            r["clusters_per_update"] = clusters / tau_draws
        for key, s in series.items():
            tau, window, cut = tau_int(s)
            r[key] = {"mean": s.mean().item(), "tau_int_draws": tau, "tau_window_draws": window, "tau_is_lower_bound": cut,
                      "tau_draws_recorded": tau_draws, "ms_per_independent_sample": tau * r["ms_per_draw"]}
        rec[name] = r
    rec["swendsenwang_1_update"]["ms_per_update"] = rec["swendsenwang_1_update"]["ms_per_draw"]
    rec["wolff_10_updates"]["ms_per_update"] = rec["wolff_10_updates"]["ms_per_draw"] / N_WOLFF
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_level_sw.json"))
    ap.add_argument("--quick", action="store_true", help="small chain counts and short runs (a functional check, not a measurement)")
    a = ap.parse_args()
    q = 16 if a.quick else 1
    settings = [(64, 4096 // q, beta, 40 // q + 2, 400 // q) for beta in (1.0, 1.5)] + [(1024, 32 // q, beta, 20 // q + 2, 160 // q) for beta in (1.0, 1.5)]
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "hip events, median of %d draws after %d warm-up draws, one process; first measurements, records not gates" % (DRAWS, WARMUP),
           "settings": []}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for s in settings:
        out["settings"].append(setting(*s))
        with open(a.out, "w") as f:        # after every setting: a run that is cut short leaves what it measured
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
