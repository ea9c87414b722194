#!/usr/bin/env python3
"""First timings of the sigma-model gradient flow (records, not gates).

    python tools/time_sigma_flow.py [--out profiles/sigma_flow.json] [--reps 10] [--rounds 3]

Per shape (64^2 x 4096 chains and 1024^2 x 32 chains, unrotated and rotated) one mlmcpi_sigma_level_flowed_charge call (Q, chi and
E asked for, eps = 0.05, the workspace allocated beforehand) for each of the step lists [5], [10] and [20], and on the same states
one mlmcpi_sigma_level_cooled_charge call for the depth lists [5], [10] and [20]: the marginal cooling sweep of DESIGN.md 7.15
re-measured in the same run.  The calls are timed in turn, `rounds` times, each time the median of `reps` calls between device
events after 5 warm-up calls; the record keeps every round.  ms per flow step is the difference between step lists, (t[20] -
t[10]) / 10 and (t[10] - t[5]) / 5: staging, the one measurement and the launch overheads the lists share cancel; ms per cooling
sweep likewise.  The expectation to compare with: a step is three all-site stages, about three cooling sweeps.  An existing --out
file is updated (the tests write their records into the same file).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

LISTS = [[5], [10], [20]]
EPS = 0.05


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
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_flow.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    timing = {"device": torch.cuda.get_device_name(0), "eps": EPS,
              "flow_plan": os.environ.get("MLMCPI_SIGMA_FLOW_PLAN", "") or "default (16x16x512x1)",
              "cool_plan": os.environ.get("MLMCPI_SIGMA_COOL_PLAN", "") or "default (32x32x512x2)",
              "note": "first measurements, one process; records, not gates; uniform random spins (mlmcpi_sigma_level_initialise)",
              "shapes": []}
    for M, B in ((64, 4096), (1024, 32)):
        for rot in (0, 1):
            lv = abi.sigma_level(M, M, rot, 1.0)
            x = ops.sigma_level_initialise(lv, B, 1)
            fwork, cwork = ops.sigma_level_flow_workspace(lv, B), ops.sigma_level_cooling_workspace(lv, B)
            rounds = []
            for _ in range(args.rounds):   # the calls in turn: what drifts, drifts for all
                r = {"flow_%d" % d[0]: timed(lambda d=d: ops.sigma_level_flowed_charge(lv, x, EPS, d, energy=True, work=fwork), args.reps) for d in LISTS}
                r.update({"cool_%d" % d[0]: timed(lambda d=d: ops.sigma_level_cooled_charge(lv, x, d, energy=True, work=cwork), args.reps) for d in LISTS})
                rounds.append(r)
            med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in rounds[0]}
            step, sweep = (med["flow_20"] - med["flow_10"]) / 10, (med["cool_20"] - med["cool_10"]) / 10
            rec = {"Mt": M, "Mx": M, "rotated": rot, "chains": B, "vertices": x.numel() // 2, "rounds": rounds, "ms_per_call": med,
                   "ms_per_flow_step_20_minus_10": step, "ms_per_flow_step_10_minus_5": (med["flow_10"] - med["flow_5"]) / 5,
                   "ms_per_cooling_sweep_20_minus_10": sweep, "ms_per_cooling_sweep_10_minus_5": (med["cool_10"] - med["cool_5"]) / 5,
                   "ratio_flow_step_to_cooling_sweep": step / sweep,
                   "ns_per_vertex_and_flow_step": 1e6 * step / (x.numel() // 2)}
            timing["shapes"].append(rec)
            print(json.dumps({k: v for k, v in rec.items() if k != "rounds"}), flush=True)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["timing"] = timing
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
