#!/usr/bin/env python3
"""First timings of sigma-model cooling (records, not gates).

    python tools/time_sigma_cooling.py [--out profiles/sigma_cooling.json] [--reps 10] [--rounds 3]

Per shape (1024^2 x 32 chains and 64^2 x 4096 chains, unrotated and rotated) one mlmcpi_sigma_level_cooled_charge call (Q, chi and E
asked for, the workspace allocated beforehand) for each of the depth lists [1], [5], [10], [20] and [0, 1, 2, 5, 10, 20], and on the
same states one mlmcpi_sigma_level_topological_charge call and one draw of a single overrelaxation sweep
(mlmcpi_sigma_level_sweep_draw, n_overrelax = 1, n_heatbath = 0: the sweep of DESIGN.md 7.1 on a plain level, of 7.6 on a rotated
one).  The calls are timed in turn, `rounds` times, each time the median of `reps` calls between device events after 5 warm-up
calls; the record keeps every round.  ms per cooling sweep is the difference between depth lists, (t[20] - t[10]) / 10 and
(t[10] - t[5]) / 5: staging, the one measurement and the launch overheads the lists share cancel.  The expectation to check: a
cooling sweep costs no more than an overrelaxation sweep (the same LDS traffic and fp64 work minus the reflection, no sincos or
atan2 and no angle write-out).  An existing --out file is updated (the GPU tests write their parity record into the same file).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

DEPTH_LISTS = [[1], [5], [10], [20], [0, 1, 2, 5, 10, 20]]


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_cooling.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    plan = os.environ.get("MLMCPI_SIGMA_COOL_PLAN", "")
    timing = {"device": torch.cuda.get_device_name(0), "plan": plan or "default (32x32x512x2)",
              "note": "first measurements, one process; records, not gates; uniform random spins (mlmcpi_sigma_level_initialise)",
              "shapes": []}
    name = lambda d: ",".join(str(v) for v in d)   # noqa: E731
    for M, B in ((1024, 32), (64, 4096)):
        for rot in (0, 1):
            lv = abi.sigma_level(M, M, rot, 1.0)
            x = ops.sigma_level_initialise(lv, B, 1)
            y, scratch = x.clone(), torch.empty_like(x)
            work = ops.sigma_level_cooling_workspace(lv, B)
            rounds = []
            for _ in range(args.rounds):   # the calls in turn: what drifts, drifts for all
                r = {name(d): timed(lambda d=d: ops.sigma_level_cooled_charge(lv, x, d, energy=True, work=work), args.reps) for d in DEPTH_LISTS}
                r["topological_charge"] = timed(lambda: ops.sigma_level_topological_charge(lv, x), args.reps)
                r["overrelaxation_sweep"] = timed(lambda: ops.sigma_level_sweep_draw(lv, y, scratch, 1, 0, 1, 0, 0), args.reps)
                rounds.append(r)
            med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in rounds[0]}
            sweep = (med["20"] - med["10"]) / 10
            rec = {"Mt": M, "Mx": M, "rotated": rot, "chains": B, "vertices": x.numel() // 2, "rounds": rounds, "ms_per_call": med,
                   "ms_per_sweep_20_minus_10": sweep, "ms_per_sweep_10_minus_5": (med["10"] - med["5"]) / 5,
                   "ratio_call_to_topological_charge": {name(d): med[name(d)] / med["topological_charge"] for d in DEPTH_LISTS},
                   "ratio_sweep_to_overrelaxation_sweep": sweep / med["overrelaxation_sweep"]}
            timing["shapes"].append(rec)
            print(json.dumps({k: v for k, v in rec.items() if k != "rounds"}))
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["timing"] = timing
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
