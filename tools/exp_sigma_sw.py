"""First measurements of the Swendsen-Wang multi-cluster update of the O(3) sigma model (mlmcpi_sigma_sw_draw), one process on
one GPU, beside the Wolff draw (10 updates) and the heat-bath draw (10 overrelaxation + 1 heat-bath sweeps) timed in the same
process.  Shapes 64^2 x 4096 chains and 1024^2 x 32 chains, beta = 1.0 and 1.5, states thermalised with heat-bath draws.  Per
setting: ms per SW update (a draw of one update, without and with its outputs; HIP events, median of 20 draws after 5 warm-up
draws, with min and max), clusters per update, ms per Wolff draw and per heat-bath draw; on 64^2 the integrated
autocorrelation time, in draws, of plain chi_m under each sampler and of the improved chi_m under SW (autocovariances pooled
over the chains, summed up to a window of 6 tau) and tau_int x ms per draw.  Writes profiles/sigma_sw.json.  Records, not
gates.

  python tools/exp_sigma_sw.py [--out profiles/sigma_sw.json] [--quick]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from exp_sigma_cluster import DRAWS, N_HB, N_OR, N_UPDATES, SEED, WARMUP, tau_int, timed  # noqa: E402
from mlmcpathintegral_amd import abi, ops  # noqa: E402


def setting(M, B, beta, therm_draws, tau_draws):
    act = abi.lattice_action(abi.NONLINEAR_SIGMA, M, M, beta=beta)
    x = ops.lattice_initialise(act, B, SEED)
    scratch = torch.empty_like(x)
    sw_work, wolff_work = ops.sigma_sw_workspace(act, B), ops.sigma_cluster_workspace(act, B)
    heat = lambda d: ops.lattice_sweep_draw(act, x, scratch, N_OR, N_HB, SEED, 0, 11 * d)  # noqa: E731
    wolff = lambda d: ops.sigma_cluster_draw(act, x, N_UPDATES, SEED + 1, 0, N_UPDATES * d, count=False, work=wolff_work)  # noqa: E731
    sw = lambda d: ops.sigma_sw_draw(act, x, 1, SEED + 2, 0, d, outputs=False, work=sw_work)  # noqa: E731
    sw_out = lambda d: ops.sigma_sw_draw(act, x, 1, SEED + 2, 0, d, work=sw_work)  # noqa: E731
    for d in range(therm_draws):
        heat(d)
    rec = {"Mt": M, "Mx": M, "chains": B, "beta": beta, "thermalisation_heatbath_draws": therm_draws,
           "sw_plan": "chain" if M * M <= 7552 and B >= 256 else "tiled 64x32"}
    first = therm_draws
    for name, fn in (("swendsenwang_1_update", sw), ("swendsenwang_1_update_with_outputs", sw_out), ("wolff_10_updates", wolff),
                     ("heatbath_10_plus_1", heat)):
        rec[name] = timed(fn, first)
        first += WARMUP + DRAWS
    clusters = torch.zeros(B, dtype=torch.int64, device="cuda")
    for d in range(first, first + 20):
        clusters += sw_out(d)[1].long()
    first += 20
    rec["clusters_per_update"] = clusters.double().mean().item() / 20
    rec["vertices_per_cluster"] = M * M / rec["clusters_per_update"]
    if tau_draws:
        chi, imp = [], []
        for d in range(first, first + tau_draws):
            imp.append(sw_out(d)[2])
            chi.append(ops.qoi_magnetic_susceptibility(x, M, M))
        first += tau_draws
        series = {"swendsenwang_1_update": torch.stack(chi), "swendsenwang_improved": torch.stack(imp)}
        for name, fn in (("wolff_10_updates", wolff), ("heatbath_10_plus_1", heat)):
            series[name] = torch.stack([(fn(d), ops.qoi_magnetic_susceptibility(x, M, M))[1] for d in range(first, first + tau_draws)])
            first += tau_draws
        for name, s in series.items():
            tau, window, cut = tau_int(s)
            ms = rec["swendsenwang_1_update_with_outputs" if name == "swendsenwang_improved" else name]["ms_per_draw"]
            r = rec.setdefault(name, {})
            r.update({"chi_m_mean": s.mean().item(), "variance_per_draw": s.var(dim=0).mean().item(), "tau_int_draws": tau,
                      "tau_window_draws": window, "tau_is_lower_bound": cut, "tau_draws_recorded": tau_draws, "tau_int_x_ms": tau * ms})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_sw.json"))
    ap.add_argument("--quick", action="store_true", help="small chain counts and short runs (a functional check, not a measurement)")
    a = ap.parse_args()
    q = 16 if a.quick else 1
    settings = [(64, 4096 // q, beta, 40 // q + 2, 400 // q) for beta in (1.0, 1.5)] + [(1024, 32 // q, beta, 20 // q + 2, 0) for beta in (1.0, 1.5)]
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "hip events, median of %d draws after %d warm-up draws, one process; first measurements, records not gates" % (DRAWS, WARMUP),
           "settings": [setting(*s) for s in settings]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
