#!/usr/bin/env python3
"""How many Swendsen-Wang updates between coarse proposals stand for the 20 rotated-level Wolff updates DESIGN 7.6 found
sufficient for the hierarchical chain at 8 x 8, beta = 1?  On the CPU, with the numpy models of tests/ (no device): the rotated
8 x 8 level (n = 32), beta = 1, B chains thermalised with heat-bath sweeps and then with the sampler itself; one DRAW is 20
level-Wolff updates (tests/sigma_level_cluster_model.py) or k Swendsen-Wang updates (tests/sigma_level_sw_model.py); chi_m is
recorded after every draw and its lag-1 autocorrelation between successive draws is estimated from the autocovariances pooled
over the chains, with the error from a jackknife over 16 blocks of chains.  The k to use is the smallest whose
autocorrelation is no larger than that of the 20 Wolff updates.

    python tools/exp_sigma_level_sw_model.py [--B 512] [--draws 200] [--out profiles/sigma_level_sw_model.json]
"""
import argparse, json, multiprocessing as mp, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sigma_level_cluster_model as slcm   # noqa: E402
import sigma_level_model as slm            # noqa: E402
import sigma_level_sw_model as slsw        # noqa: E402

K_WOLFF = 20
KS = (1, 2, 4, 8, 12, 13, 14, 15, 16, 17, 18, 20, 24)


def lag1(series):
    """series [draws, chains] -> (rho(1), jackknife error over 16 blocks of chains)"""
    def rho(x):
        x = x - x.mean(axis=0, keepdims=True)
        return float((x[:-1] * x[1:]).mean() / (x * x).mean())
    blocks = np.array_split(np.arange(series.shape[1]), 16)
    jack = np.array([rho(np.delete(series, blk, axis=1)) for blk in blocks])
    return rho(series), float(np.sqrt((len(jack) - 1) * ((jack - jack.mean()) ** 2).mean()))


def run(args):
    a, name, k = args
    t0 = time.time()
    L = slm.Level(8, 8, True, 1.0)
    update = slcm.dev_update_batch if name == "wolff" else slsw.dev_update_batch
    x = slm.sweep_draw(L, slm.initialise(L, a.B, 11), 40, 20, seed=11)
    chi, step = [], 0
    for d in range(20 + a.draws):
        for _ in range(k):
            x, _ = update(L, x, 12, 0, step)
            step += 1
        if d >= 20:
            chi.append(slm.magnetic_susceptibility(L, x))
    chi = np.array(chi)
    r, e = lag1(chi)
    return {"sampler": name, "updates_per_draw": k, "chi_m": float(chi.mean()), "lag1_autocorrelation": r, "error": e,
            "seconds": time.time() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_level_sw_model.json"))
    a = ap.parse_args()
    jobs = [(a, "wolff", K_WOLFF)] + [(a, "swendsenwang", k) for k in KS]
    with mp.get_context("fork").Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        rows = pool.map(run, jobs)
    wolff, sw = rows[0], rows[1:]
    chosen = next((r["updates_per_draw"] for r in sw if r["lag1_autocorrelation"] <= wolff["lag1_autocorrelation"]), None)
    res = {"what": "numpy model, rotated 8 x 8 level, beta = 1: lag-1 autocorrelation of chi_m between successive draws, a draw = 20 "
                   "level-Wolff updates or k Swendsen-Wang updates; one run", "B": a.B, "draws": a.draws, "wolff": wolff,
           "swendsenwang": sw, "smallest_k_no_larger_than_wolff": chosen}
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
