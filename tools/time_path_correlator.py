#!/usr/bin/env python3
"""First timings of the time correlator of the 1-D paths (records, not gates).

    python tools/time_path_correlator.py [--out profiles/path_correlator.json] [--reps 20]

Per shape (M, n_lag, B) and kind (0 harmonic, 2 rotor): one mlmcpi_path_correlator call and, on the same states, one
mlmcpi_qoi_xsquared call -- the cheapest read of the same bytes.  The floor is M n_lag components fp64 FMAs per chain at the
device's fp64 vector rate (78.6 TFLOP/s = 39.3e12 FMA/s).  Times are medians of `reps` calls between device events after 5
warm-up calls.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

FMA_PER_S = 78.6e12 / 2
SHAPES = ((128, 65, 4096), (1024, 64, 2048), (4096, 2049, 256))


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
    ap.add_argument("--out", default=os.path.join("profiles", "path_correlator.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "box": os.uname().nodename, "fp64_fma_per_s": FMA_PER_S,
           "note": "first measurements, one run; records, not gates", "shapes": []}
    for M, n_lag, B in SHAPES:
        for kind in (abi.HARMONIC, abi.ROTOR):
            act = abi.path_action(kind, M, M / 32.0, 1.0 if kind == abi.HARMONIC else 0.25)
            gen = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn((B, M), dtype=torch.float64, device="cuda", generator=gen) * (4.0 if kind == abi.ROTOR else 1.0)
            work = ops.path_correlator_workspace(act, n_lag, B)
            acc = torch.zeros(B, n_lag, 2, dtype=torch.float64, device="cuda")
            plan = ops.path_correlator_plan(act, n_lag, B)
            ncomp = plan["components"]
            rec = {"kind": int(kind), "M": M, "n_lag": n_lag, "chains": B, "plan": plan,
                   "correlator": timed(lambda: ops.path_correlator(act, x, n_lag, acc=acc, work=work), args.reps),
                   "xsquared": timed(lambda: ops.qoi_xsquared(x), args.reps)}
            floor_ms = 1e3 * B * M * n_lag * ncomp / FMA_PER_S
            rec["fma_floor_ms"] = floor_ms
            rec["ratio_to_xsquared"] = rec["correlator"]["median_ms"] / rec["xsquared"]["median_ms"]
            rec["ratio_to_fma_floor"] = rec["correlator"]["median_ms"] / floor_ms
            rec["closer_to"] = "fma_floor" if rec["ratio_to_fma_floor"] < rec["ratio_to_xsquared"] else "xsquared"
            out["shapes"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
