"""First measurements of the improved Wolff draw (mlmcpi_sigma_level_cluster_improved_draw), one process
on one GPU, beside the plain Wolff draw of the same build.  One run each: records, not gates.  Writes
profiles/sigma_cluster_improved.json.

Cost: ms per draw of 10 updates (HIP events, median of 20 draws after 5 warm-up draws, as tools/exp_sigma_cluster.py) of the plain
draw and of the improved draw with chi only, with the structure factor, and with the correlator, at 64^2 x 4096 chains, beta = 1
and 1.5, and on the rotated partner of 1024^2 x 32 chains; states thermalised with heat-bath draws.
Independent samples (64^2): the integrated autocorrelation time, in draws, and the variance per draw of the plain chi_m after each
draw and of the draw's improved chi_m, and tau_int x ms per draw, to set beside profiles/sigma_cluster.json and
profiles/sigma_sw.json.
Lags: 64^2, beta = 1.5, 512 chains, draws of one update: per lag the error (spread over the chains of the run mean) of the plain
C_t on the state before each update over that of the improved C_t, equal samples.

  python tools/exp_sigma_cluster_improved.py [--out profiles/sigma_cluster_improved.json] [--quick]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from exp_sigma_cluster import DRAWS, N_HB, N_OR, N_UPDATES, SEED, WARMUP, tau_int, timed  # noqa: E402
from mlmcpathintegral_amd import abi, ops  # noqa: E402


def setting(M, rot, B, beta, therm_draws, tau_draws):
    lv = abi.sigma_level(M, M, rot, beta)
    x = ops.sigma_level_initialise(lv, B, SEED)
    scratch = torch.empty_like(x)
    for d in range(therm_draws):
        ops.sigma_level_sweep_draw(lv, x, scratch, N_OR, N_HB, SEED, 0, 11 * d)
    plain_work, work = ops.sigma_level_cluster_workspace(lv, B), ops.sigma_level_cluster_improved_workspace(lv, B)
    draws = {"plain": lambda d: ops.sigma_level_cluster_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=plain_work),
             "improved_chi": lambda d: ops.sigma_level_cluster_improved_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=work),
             "improved_chi_structure": lambda d: ops.sigma_level_cluster_improved_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=work,
                                                                                       structure=True),
             "improved_chi_correlator": lambda d: ops.sigma_level_cluster_improved_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=work,
                                                                                        correlator=True),
             "improved_all": lambda d: ops.sigma_level_cluster_improved_draw(lv, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, work=work,
                                                                             structure=True, correlator=True)}
    rec = {"Mt": M, "Mx": M, "rotated": bool(rot), "chains": B, "beta": beta, "updates_per_draw": N_UPDATES,
           "thermalisation_heatbath_draws": therm_draws, "workspace_bytes": {"plain": plain_work.numel(), "improved": work.numel()}}
    first = 0
    for name, fn in draws.items():
        rec[name] = timed(fn, first)
        first += WARMUP + DRAWS
    for name in list(draws)[1:]:
        rec[name]["over_plain"] = rec[name]["ms_per_draw"] / rec["plain"]["ms_per_draw"]
    sites = torch.zeros(B, dtype=torch.int64, device="cuda")
    for d in range(first, first + 20):
        sites += draws["plain"](d).long()
    first += 20
    rec["flipped_vertices_per_update"] = sites.double().mean().item() / (20 * N_UPDATES)
    if tau_draws:
        chi, imp = [], []
        for d in range(first, first + tau_draws):
            imp.append(draws["improved_chi"](d)[1] / N_UPDATES)
            chi.append(ops.sigma_level_magnetic_susceptibility(lv, x))
        for name, s, ms in (("plain_chi_m", torch.stack(chi), rec["plain"]["ms_per_draw"]),
                            ("improved_chi_m", torch.stack(imp), rec["improved_chi"]["ms_per_draw"])):
            tau, window, cut = tau_int(s)
            rec[name] = {"mean": s.mean().item(), "variance_per_draw": s.var(dim=0).mean().item(), "tau_int_draws": tau,
                         "tau_window_draws": window, "tau_is_lower_bound": cut, "tau_draws_recorded": tau_draws, "tau_int_x_ms_per_draw": tau * ms,
                         "variance_x_tau_int_x_ms": s.var(dim=0).mean().item() * tau * ms}
    print(json.dumps(rec), flush=True)
    return rec


def lags(M, beta, B, therm_draws, burn, meas):
    lv = abi.sigma_level(M, M, 0, beta)
    x = ops.sigma_level_initialise(lv, B, SEED + 3)
    scratch = torch.empty_like(x)
    for d in range(therm_draws):
        ops.sigma_level_sweep_draw(lv, x, scratch, N_OR, N_HB, SEED + 3, 0, 11 * d)
    work = ops.sigma_level_cluster_improved_workspace(lv, B)
    nt = M // 2 + 1
    imp, pl = torch.zeros(B, nt, dtype=torch.float64, device="cuda"), torch.zeros(B, nt, dtype=torch.float64, device="cuda")
    for d in range(burn + meas):
        if d >= burn:
            pl += ops.sigma_level_correlator(lv, x)[:, :nt]
        out = ops.sigma_level_cluster_improved_draw(lv, x, 1, SEED + 4, 0, d, work=work, correlator=True)
        if d >= burn:
            imp += out[2][:, :nt]
    imp, pl = (imp / meas).cpu().numpy(), (pl / meas).cpu().numpy()
    err = lambda v: (v.std(axis=0, ddof=1) / math.sqrt(B)).tolist()  # noqa: E731
    e_i, e_p = err(imp), err(pl)
    rec = {"M": M, "beta": beta, "chains": B, "burn_in_updates": burn, "samples_per_chain": meas, "direction": "t",
           "C_improved": imp.mean(axis=0).tolist(), "error_improved": e_i, "C_plain": pl.mean(axis=0).tolist(), "error_plain": e_p,
           "error_ratio_plain_over_improved": [p / i for p, i in zip(e_p, e_i)]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_cluster_improved.json"))
    ap.add_argument("--quick", action="store_true", help="small chain counts and short runs (a functional check, not a measurement)")
    a = ap.parse_args()
    q = 16 if a.quick else 1
    settings = [(64, 0, 4096 // q, beta, 40 // q + 2, 600 // q) for beta in (1.0, 1.5)] + [(1024, 1, 32 // q, beta, 20 // q + 2, 0) for beta in (1.0, 1.5)]
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "hip events, median of %d draws after %d warm-up draws, one process; first measurements, one run each, records not gates"
                     % (DRAWS, WARMUP),
           "settings": [setting(*s) for s in settings], "lags": lags(64, 1.5, 512 // q, 40 // q + 2, 200 // q, 400 // q)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
