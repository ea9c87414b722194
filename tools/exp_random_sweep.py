"""Times the parallel random-order sweep against the two paths that existed before it, in one process on one GPU:
ms per draw of 10 overrelaxation + 1 heat-bath sweeps (event-timed, median of 10 draws after 3 warm-up draws) for
  new        mlmcpi_lattice_random_sweep_draw (device order, parallel rounds, one launch per draw)
  site_loop  mlmcpi_lattice_site_updates with a host permutation per sweep (what random_order = true ran before)
  multicolour  mlmcpi_lattice_sweep_draw
and the rounds per sweep read from mlmcpi_lattice_random_sweep_order.  Writes profiles/random_order_parallel.json.

  python tools/exp_random_sweep.py [--out profiles/random_order_parallel.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

SEED, N_OR, N_HB, WARMUP, DRAWS = 20240607, 10, 1, 3, 10


def timed(fn, warmup=WARMUP, draws=DRAWS):
    for d in range(warmup):
        fn(d)
    torch.cuda.synchronize()
    ms = []
    for d in range(warmup, warmup + draws):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(d)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_per_draw": statistics.median(ms), "min": min(ms), "max": max(ms), "draws": draws, "warmup": warmup}


def shape(name, kind, M, B, coupling, site_loop=True):
    act = abi.lattice_action(kind, M, M, beta=coupling) if kind != abi.GFF else abi.lattice_action(kind, M, M, mass=coupling)
    n = (2 if kind == abi.SCHWINGER else 1) * M * M
    x = ops.lattice_initialise(act, B, SEED)
    work = ops.lattice_random_sweep_workspace(act, B)
    rec = {"shape": name, "Mt": M, "Mx": M, "chains": B, "sweeps": [N_OR, N_HB]}
    rec["new"] = timed(lambda d: ops.lattice_random_sweep_draw(act, x, N_OR, N_HB, SEED, 0, d * 11, work=work))
    scratch = torch.empty_like(x)
    rec["multicolour"] = timed(lambda d: ops.lattice_sweep_draw(act, x, scratch, N_OR, N_HB, SEED, 0, d * 11))
    if site_loop:
        rng = np.random.default_rng(1)
        perm = torch.empty(n, dtype=torch.int32, device="cuda")

        def loop(d):
            for s in range(N_OR + N_HB):
                perm.copy_(torch.from_numpy(rng.permutation(n).astype(np.int32)))
                ops.lattice_site_updates(act, x, perm, s >= N_OR, SEED, 0, d * 11 + s)
        rec["site_loop"] = timed(loop)
        rec["speedup_over_site_loop"] = rec["site_loop"]["ms_per_draw"] / rec["new"]["ms_per_draw"]
    else:
        rec["site_loop"] = None  # one thread per chain over 2 10^6 links per sweep: minutes per draw
    rec["ratio_to_multicolour"] = rec["new"]["ms_per_draw"] / rec["multicolour"]["ms_per_draw"]
    _, rnd = ops.lattice_random_sweep_order(act, min(B, 8), SEED, 0, 0)
    per = rnd.max(dim=1).values.double()
    rec["rounds"] = {"mean": float(per.mean()), "max": int(per.max()), "mean_round_of_an_index": float(rnd.double().mean()),
                     "orders": int(per.numel())}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "random_order_parallel.json"))
    ap.add_argument("--quick", action="store_true", help="small chain counts (a functional check, not a measurement)")
    a = ap.parse_args()
    q = 16 if a.quick else 1
    shapes = [("schwinger_64x64", abi.SCHWINGER, 64, 4096 // q, 1.0, True), ("schwinger_16x16", abi.SCHWINGER, 16, 16384 // q, 1.0, True),
              ("schwinger_1024x1024_global", abi.SCHWINGER, 1024, 32 // q, 1.0, False), ("gff_64x64", abi.GFF, 64, 4096 // q, 10.0, True),
              ("sigma_64x64", abi.NONLINEAR_SIGMA, 64, 1024 // q, 1.0, True)]
    out = {"device": torch.cuda.get_device_name(0), "timing": "hip events, median of 10 draws after 3 warm-up draws, one process",
           "shapes": [shape(*s) for s in shapes]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
