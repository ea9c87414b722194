#!/usr/bin/env python3
"""First timings of the sigma model's topological charge (records, not gates).

    python tools/time_sigma_topology.py [--out profiles/sigma_topology.json] [--reps 30] [--rounds 3]

Per shape (1024^2 x 32 chains and 64^2 x 4096 chains, unrotated and rotated): one mlmcpi_sigma_level_topological_charge call (its
two launches) and, on the same states, one mlmcpi_sigma_level_magnetic_susceptibility call -- both read the state once and pay one
sincos pair per vertex, so chi_m (device code this build does not touch) is the yardstick.  The two are timed alternately, `rounds`
times, each time the median of `reps` calls between device events after 5 warm-up calls; the record keeps every round, so the
spread is there to see.  An existing --out file is updated (the GPU tests write their parity record into the same file).

The instruction-count floor.  The vector work a vertex cannot avoid is 2 sincos (its own angles, staged once) and 2 atan2 (n faces of
two triangles for n vertices).  Counted in the gfx950 ISA hipcc -O3 emits for a kernel that calls the routine once (ROCm's ocml):
atan2 is branch-free, 106 vector instructions, 44 of them fp64; sincos is 155, 108 of them fp64, and that count includes its
large-argument reduction behind two branches, so for angles in [-pi, pi] it is an upper estimate.  A wave64 vector instruction
issues in 2 cycles on a SIMD-32, an fp64 one in 4 (the part's 78.6 TFLOP/s of vector fp64 are half its fp32 rate); 1024 SIMDs at
2.4 GHz.  `floor_atan2_only` uses the exact atan2 count alone and is a true lower bound; `estimate_sincos_atan2` adds the sincos
count and is what the kernel should be compared with.  The halo (33^2 / 32^2 staged vertices per tile), the dot and triple products,
the LDS traffic and the sums come on top.  The HBM floor counts the 16 bytes per vertex at the measured 6.29 TB/s copy rate.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402

ATAN2 = {"valu": 106, "fp64": 44}
SINCOS = {"valu": 155, "fp64": 108}
SIMDS, CLOCK_HZ, HBM_BPS = 1024, 2.4e9, 6.29e12


def wave_cycles(c):
    return 4 * c["fp64"] + 2 * (c["valu"] - c["fp64"])


def floors_ms(vertices):
    per_simd_waves = vertices / 64 / SIMDS
    return {"floor_atan2_only_ms": 1e3 * per_simd_waves * 2 * wave_cycles(ATAN2) / CLOCK_HZ,
            "estimate_sincos_atan2_ms": 1e3 * per_simd_waves * 2 * (wave_cycles(ATAN2) + wave_cycles(SINCOS)) / CLOCK_HZ,
            "hbm_floor_ms": 1e3 * 16 * vertices / HBM_BPS}


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
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_topology.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    timing = {"device": torch.cuda.get_device_name(0), "box": os.uname().nodename,
              "note": "first measurements, one process; records, not gates; chi_m is the kernel of this same build (unchanged device code); "
                      "uniform random spins (mlmcpi_sigma_level_initialise)",
              "instruction_counts_per_call": {"atan2": ATAN2, "sincos": SINCOS}, "shapes": []}
    for M, B in ((1024, 32), (64, 4096)):
        for rot in (0, 1):
            lv = abi.sigma_level(M, M, rot, 1.0)
            x = ops.sigma_level_initialise(lv, B, 1)
            vertices = x.numel() // 2
            rounds = []
            for _ in range(args.rounds):   # alternate the two calls: what drifts, drifts for both
                rounds.append({"topological_charge": timed(lambda: ops.sigma_level_topological_charge(lv, x), args.reps),
                               "chi_m": timed(lambda: ops.sigma_level_magnetic_susceptibility(lv, x), args.reps)})
            t = statistics.median(r["topological_charge"]["median_ms"] for r in rounds)
            c = statistics.median(r["chi_m"]["median_ms"] for r in rounds)
            rec = {"Mt": M, "Mx": M, "rotated": rot, "chains": B, "vertices": vertices, "rounds": rounds,
                   "topological_charge_ms": t, "chi_m_ms": c, "ratio_topological_charge_to_chi_m": t / c,
                   "ratio_per_round": [r["topological_charge"]["median_ms"] / r["chi_m"]["median_ms"] for r in rounds]}
            rec.update(floors_ms(vertices))
            rec["estimate_over_measured"] = rec["estimate_sincos_atan2_ms"] / t
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
