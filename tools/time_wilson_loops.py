#!/usr/bin/env python3
"""First timings of the Wilson loops of the quenched Schwinger model (records, not gates).

    python tools/time_wilson_loops.py [--out profiles/wilson_loops.json] [--reps 20]

Per shape (Mt = Mx, R = S, B): one mlmcpi_schwinger_wilson_loops call and, on the same states, one mlmcpi_qoi_avg_plaquette call --
the cheapest read of the same bytes.  Two floors, both arithmetic and not measurements:
  valu_floor_ms  V B R (5 S + 4) fp64 vector instructions per lane-element (4 per strip multiply, 5 per loop product and its add) at
                 the device's fp64 vector rate (78.6 TFLOP/s = 39.3e12 instructions/s)
  lds_floor_ms   what a kernel with ONE 16-byte LDS read per loop product would need: V B R S 16 bytes at 256 CUs x 256 B/clk x 2.4 GHz.
                 The kernel as built reads (J + S - 1) / (J S) of that (lds_bytes_as_built).
Times are medians of `reps` calls between device events after 5 warm-up calls.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

FP64_INSTR_PER_S = 78.6e12 / 2
LDS_BYTES_PER_S = 256 * 256 * 2.4e9
SHAPES = ((1024, 1, 32), (1024, 4, 32), (1024, 8, 32), (1024, 16, 32), (64, 8, 4096))


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
    ap.add_argument("--out", default=os.path.join("profiles", "wilson_loops.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "box": os.uname().nodename, "fp64_instr_per_s": FP64_INSTR_PER_S,
           "lds_bytes_per_s": LDS_BYTES_PER_S, "note": "first measurements, one run; records, not gates; the floors are arithmetic",
           "shapes": []}
    for M, R, B in SHAPES:
        S, V = R, M * M
        act = abi.lattice_action(abi.SCHWINGER, M, M, beta=1.0)
        x = ops.lattice_initialise(act, B, 1)
        work = ops.wilson_loops_workspace(M, M, R, S, B)
        acc = torch.zeros(B, R, S, 2, dtype=torch.float64, device="cuda")
        plan = ops.wilson_loops_plan(M, M, R, S, B)
        rec = {"Mt": M, "Mx": M, "R": R, "S": S, "chains": B, "plan": plan,
               "wilson_loops": timed(lambda: ops.wilson_loops(x, M, M, R, S, acc=acc, work=work), args.reps),
               "avg_plaquette": timed(lambda: ops.qoi_avg_plaquette(x, M, M), args.reps)}
        rec["valu_floor_ms"] = 1e3 * V * B * R * (5 * S + 4) / FP64_INSTR_PER_S
        rec["lds_floor_ms"] = 1e3 * V * B * R * S * 16 / LDS_BYTES_PER_S
        rec["lds_bytes_as_built"] = V * B * R * (plan["J"] + S - 1) * 16 // plan["J"]
        rec["state_bytes"] = V * B * 16
        rec["ratio_to_avg_plaquette"] = rec["wilson_loops"]["median_ms"] / rec["avg_plaquette"]["median_ms"]
        rec["ratio_to_valu_floor"] = rec["wilson_loops"]["median_ms"] / rec["valu_floor_ms"]
        rec["ratio_to_lds_floor"] = rec["wilson_loops"]["median_ms"] / rec["lds_floor_ms"]
        out["shapes"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
