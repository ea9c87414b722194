#!/usr/bin/env python3
"""First timings of the sigma model's time-slice correlator (records, not gates).

    python tools/time_sigma_correlator.py [--out profiles/sigma_correlator.json] [--reps 20]

Per shape (1024^2 x 32 chains and 64^2 x 4096 chains, unrotated and rotated): one mlmcpi_sigma_level_correlator call (its three
launches) and, on the same states, one mlmcpi_sigma_level_magnetic_susceptibility call -- both read the state once and pay one
sincos pair per vertex, so chi_m is the yardstick.  The fraction of 8 TB/s counts the 16 bytes per vertex of the state against
the time of the WHOLE correlator call, so it is a lower bound for the slice-sum pass alone.  At 64^2 x 4096 one Swendsen-Wang
update of the same states is timed beside them.  Times are medians of `reps` calls between device events after 5 warm-up calls.
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
    ap.add_argument("--out", default=os.path.join("profiles", "sigma_correlator.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "box": os.uname().nodename, "beta": 1.5,
           "note": "first measurements, one run; records, not gates; chi_m is the kernel of this same build (unchanged device code)",
           "shapes": []}
    for M, B in ((1024, 32), (64, 4096)):
        for rot in (0, 1):
            lv = abi.sigma_level(M, M, rot, 1.5)
            x = ops.sigma_level_initialise(lv, B, 1)
            ops.sigma_level_sweep_draw(lv, x, torch.empty_like(x), 0, 2, 1, 0, 0)
            work = ops.sigma_level_correlator_workspace(lv, B)
            acc = torch.zeros(B, ops.sigma_level_correlator_size(lv), 2, dtype=torch.float64, device="cuda")
            rec = {"Mt": M, "Mx": M, "rotated": rot, "chains": B, "workspace_bytes": work.numel(),
                   "correlator": timed(lambda: ops.sigma_level_correlator(lv, x, acc=acc, work=work), args.reps),
                   "chi_m": timed(lambda: ops.sigma_level_magnetic_susceptibility(lv, x), args.reps)}
            state_bytes = x.numel() * 8
            rec["ratio_correlator_to_chi_m"] = rec["correlator"]["median_ms"] / rec["chi_m"]["median_ms"]
            rec["correlator"]["fraction_of_8TBps_whole_call"] = state_bytes / (rec["correlator"]["median_ms"] * 1e-3) / 8e12
            rec["chi_m"]["fraction_of_8TBps"] = state_bytes / (rec["chi_m"]["median_ms"] * 1e-3) / 8e12
            if M == 64:
                sw_work = ops.sigma_level_sw_workspace(lv, B)
                counter = [0]

                def sw():
                    ops.sigma_level_sw_draw(lv, x, 1, 9, 0, counter[0], outputs=False, work=sw_work)
                    counter[0] += 1

                rec["swendsen_wang_update"] = timed(sw, args.reps)
                rec["ratio_correlator_to_swendsen_wang_update"] = rec["correlator"]["median_ms"] / rec["swendsen_wang_update"]["median_ms"]
            out["shapes"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
