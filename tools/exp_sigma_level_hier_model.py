#!/usr/bin/env python3
"""How many Wolff updates between coarse proposals does the hierarchical chain of the sigma model need?  On the CPU, with the
numpy models of tests/ (no device): 8 x 8, beta = beta_coarse = 1; the coarse proposals are the successive states of ONE
rotated-level Wolff chain (tests/sigma_level_cluster_model.py), one draw of k updates between proposals, fed to
sigma_level_model.twolevel_draw; chi_m of the fine chain against the model's single-level 10 + 1 heat-bath chain.  Both levels
start from sweeps of their own law, so a valid step keeps the fine law from the first draw on.  Means across chains; the
chain's error must be at or below 0.7 % of chi_m (the bias with one 10 + 1 heat-bath draw between proposals is 2.6 %, DESIGN
7.6).  The k to use is the smallest of {10, 20, 40, 80} whose chain lies within 3 of its own sigma of the heat-bath value.

    python tools/exp_sigma_level_hier_model.py [--B 512] [--steps 120] [--out profiles/sigma_level_hier_model.json]
"""
import argparse, json, math, multiprocessing as mp, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sigma_level_cluster_model as slcm   # noqa: E402
import sigma_level_model as slm            # noqa: E402

KS = (10, 20, 40, 80)


def stat(v):
    return float(v.mean()), float(v.std(ddof=1) / math.sqrt(len(v)))


def heatbath(a):
    L = slm.Level(8, 8, False, 1.0)
    x = slm.sweep_draw(L, slm.initialise(L, a.B, 3), 40, 20, seed=3)
    tot = np.zeros(a.B)
    for s in range(a.steps):
        x = slm.sweep_draw(L, x, 10, 1, seed=3, sweep0=1000 + 11 * s)
        tot += slm.magnetic_susceptibility(L, x)
    m, e = stat(tot / a.steps)
    return {"sampler": "single-level 10 + 1 heat bath", "chi_m": m, "error": e}


def hierarchical(args):
    a, k = args
    t0 = time.time()
    L = slm.Level(8, 8, False, 1.0)
    Lc = L.coarse(1.0)
    theta = slm.sweep_draw(L, slm.initialise(L, a.B, 4), 40, 20, seed=4)
    coarse = slm.sweep_draw(Lc, slm.initialise(Lc, a.B, 5), 40, 20, seed=5)
    tot, acc, sizes = np.zeros(a.B), 0.0, 0.0
    for s in range(a.steps):
        for j in range(k):
            coarse, size = slcm.dev_update_batch(Lc, coarse, 5, 0, k * s + j)
            sizes += size.mean()
        theta, accept, _, _, _ = slm.twolevel_draw(L, Lc, coarse, theta, 6, 0, s)
        acc += accept.mean()
        tot += slm.magnetic_susceptibility(L, theta)
    m, e = stat(tot / a.steps)
    return {"k": k, "chi_m": m, "error": e, "acceptance": acc / a.steps, "mean_cluster_size": sizes / (k * a.steps),
            "seconds": time.time() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_level_hier_model.json"))
    a = ap.parse_args()
    with mp.get_context("fork").Pool(min(len(KS) + 1, os.cpu_count() or 1)) as pool:
        hb = pool.apply_async(heatbath, (a,))
        rows = pool.map(hierarchical, [(a, k) for k in KS])
        hb = hb.get()
    chosen = None
    for r in rows:
        r["z_own_sigma"] = (r["chi_m"] - hb["chi_m"]) / r["error"]
        r["z"] = (r["chi_m"] - hb["chi_m"]) / math.hypot(r["error"], hb["error"])
        r["error_over_chi_m"] = r["error"] / r["chi_m"]
        if chosen is None and abs(r["z_own_sigma"]) < 3.0 and r["error_over_chi_m"] <= 0.007:
            chosen = r["k"]
    res = {"what": "numpy model, 8 x 8, beta = beta_coarse = 1: hierarchical chain with k rotated-level Wolff updates between "
                   "proposals against the single-level 10 + 1 heat bath; one run", "B": a.B, "steps": a.steps, "heatbath": hb,
           "hierarchical": rows, "smallest_k_within_3_own_sigma": chosen}
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
