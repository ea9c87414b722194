#!/usr/bin/env python3
"""First timings of the sigma model's two-level step and rotated-level sweeps (records, not gates).

    python tools/time_sigma_twolevel.py [--out profiles/sigma_twolevel.json] [--reps 20]

Per shape (64^2 x 4096 chains, 1024^2 x 32 chains; beta = 1): one mlmcpi_sigma_twolevel_draw (fine level unrotated M x M, coarse
partner the rotated M x M) and one 10 + 1 draw of mlmcpi_sigma_level_sweep_draw on that rotated level, beside the unrotated
level's own 10 + 1 draw.  Times are medians of `reps` calls between device events after 5 warm-up calls; min and max recorded.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlmcpathintegral_amd import abi, ops  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_twolevel.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "beta": 1.0, "note": "first measurements, one run; records, not gates", "shapes": []}
    for M, B in ((64, 4096), (1024, 32)):
        fine = abi.sigma_level(M, M, 0, 1.0)
        rot = fine.coarse(1.0)
        theta = ops.sigma_level_initialise(fine, B, 1)
        ops.sigma_level_sweep_draw(fine, theta, torch.empty_like(theta), 0, 2, 1, 0, 0)
        phi = ops.sigma_level_initialise(rot, B, 2)
        scratch = torch.empty_like(phi)
        ops.sigma_level_sweep_draw(rot, phi, scratch, 0, 2, 2, 0, 0)
        step = ops.SigmaTwoLevelStep(fine, rot, B, seed=3)
        step.set_state(theta)
        counter = [100]

        def rot_draw():
            ops.sigma_level_sweep_draw(rot, phi, scratch, 10, 1, 2, 0, counter[0])
            counter[0] += 11

        fscratch = torch.empty_like(theta)

        def fine_draw():
            ops.sigma_level_sweep_draw(fine, theta, fscratch, 10, 1, 1, 0, counter[0])
            counter[0] += 11

        rec = {"Mt": M, "Mx": M, "chains": B,
               "twolevel_draw": timed(lambda: step.draw(phi), args.reps),
               "rotated_level_draw_10_1": timed(rot_draw, args.reps),
               "unrotated_level_draw_10_1": timed(fine_draw, args.reps)}
        n_fine, n_rot = M * M * B, M * M // 2 * B
        rec["twolevel_draw"]["fine_vertices_per_s"] = n_fine / (rec["twolevel_draw"]["median_ms"] * 1e-3)
        rec["rotated_level_draw_10_1"]["vertex_updates_per_s"] = 11 * n_rot / (rec["rotated_level_draw_10_1"]["median_ms"] * 1e-3)
        rec["unrotated_level_draw_10_1"]["vertex_updates_per_s"] = 11 * n_fine / (rec["unrotated_level_draw_10_1"]["median_ms"] * 1e-3)
        rec["twolevel_acceptance_of_last_draw"] = float(step.accept.double().mean())
        out["shapes"].append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
