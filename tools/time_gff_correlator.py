#!/usr/bin/env python3
"""First timings of the momentum-projected GFF slice correlators (records, not gates).

    python tools/time_gff_correlator.py [--out profiles/gff_correlator.json] [--reps 20]

Per shape (Mt = Mx, P, chains, unrotated): one mlmcpi_gff_correlator call and, on the same states in the same process, one
mlmcpi_qoi_phi_squared call -- the existing kernel that makes the same single read.  Floors, all arithmetic and not measurements:
  hbm_floor_ms   the state once (V chains 8 bytes) plus the partials the projection writes and the gather reads back
                 (2 x 16 bytes x P x (bands W + chunks H) per chain) at 8 TB/s
  valu_floor_ms  4 P fp64 FMAs per vertex (2 directions x 2 parts) at the device's fp64 vector rate (39.3e12 instructions/s)
  lds_floor_ms   the LDS reads of the projection as built: per vertex and momentum one 8-byte and one 16-byte read in each direction
                 (48 P bytes; the 16-byte twiddle reads are wave-uniform but still issued) at 256 CUs x 128 B/clk x 2.4 GHz
Times are medians of `reps` calls between device events after 5 warm-up calls; the clocks are what the device reports at the
start; one run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP64_INSTR_PER_S = 78.6e12 / 2
LDS_BYTES_PER_S = 256 * 128 * 2.4e9
SHAPES = ((1024, 1, 32), (1024, 4, 32), (1024, 8, 32), (64, 1, 4096), (64, 8, 4096))


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


def clocks():
    try:
        p = torch.cuda.get_device_properties(0)
        return {"clock_rate_khz": getattr(p, "clock_rate", None), "memory_clock_rate_khz": getattr(p, "memory_clock_rate", None),
                "compute_units": p.multi_processor_count}
    except Exception as e:  # noqa: BLE001
        return {"error": str(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gff_correlator.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "box": os.uname().nodename, "clocks": clocks(), "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "fp64_instr_per_s": FP64_INSTR_PER_S, "lds_bytes_per_s": LDS_BYTES_PER_S,
           "note": "first measurements, one run; records, not gates; the floors are arithmetic", "shapes": []}
    for M, P, B in SHAPES:
        V = M * M
        act = abi.lattice_action(abi.GFF, M, M, mass=4.0)
        x = ops.lattice_initialise(act, B, 1)
        work = ops.gff_correlator_workspace(M, M, P, B)
        acc = torch.zeros(B, ops.gff_correlator_size(M, M, P), 2, dtype=torch.float64, device="cuda")
        plan = ops.gff_correlator_plan(M, M, P, False, B)
        rec = {"Mt": M, "Mx": M, "P": P, "chains": B, "rotated": 0, "plan": plan,
               "gff_correlator": timed(lambda: ops.gff_correlator(x, M, M, P, acc=acc, work=work), args.reps),
               "phi_squared": timed(lambda: ops.qoi_phi_squared(x), args.reps)}
        partial_bytes = 2 * 16 * P * (plan["bands"] * plan["plane_w"] + plan["chunks"] * plan["plane_h"]) * B
        rec["state_bytes"] = V * B * 8
        rec["partial_bytes_written_and_read"] = partial_bytes
        rec["hbm_floor_ms"] = 1e3 * (V * B * 8 + partial_bytes) / HBM_BYTES_PER_S
        rec["valu_floor_ms"] = 1e3 * V * B * 4 * P / FP64_INSTR_PER_S
        rec["lds_floor_ms"] = 1e3 * V * B * 48 * P / LDS_BYTES_PER_S
        rec["ratio_to_phi_squared"] = rec["gff_correlator"]["median_ms"] / rec["phi_squared"]["median_ms"]
        rec["phi_squared_fraction_of_hbm"] = 1e3 * V * B * 8 / HBM_BYTES_PER_S / rec["phi_squared"]["median_ms"]
        for floor in ("hbm", "valu", "lds"):
            rec["ratio_to_%s_floor" % floor] = rec["gff_correlator"]["median_ms"] / rec["%s_floor_ms" % floor]
        out["shapes"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
