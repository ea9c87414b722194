#!/usr/bin/env python3
"""Records of the cluster-improved time-slice correlator of the Swendsen-Wang update: what the correlator
output costs, and what it buys per lag.  One run each, not gates.  Writes profiles/sigma_sw_correlator.json.

Cost: the time of an update through mlmcpi_sigma_level_sw_correlator_draw against the same update through
mlmcpi_sigma_level_sw_draw and mlmcpi_sigma_level_sw_structure_draw (all outputs asked for), events around `reps` calls after
warm-up, at 64 x 64 x 4096 chains (chain plan) and the rotated partner of 1024 x 1024 x 32 chains (tiled plan), beta = 1 and 1.5,
in calls of 1 update (what the sampler issues).  Variance: 64 x 64, beta = 1.5, per lag the spread over the chains of the mean
plain C_t (mlmcpi_sigma_level_correlator on the state before each update) over that of the improved C_t, equal samples.

    python tools/time_sigma_sw_correlator.py [--out profiles/sigma_sw_correlator.json] [--only cost|variance]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mlmcpathintegral_amd import abi, ops  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def cost(Mt, Mx, rot, B, beta, reps):
    lv = abi.sigma_level(Mt, Mx, rot, beta)
    x = ops.sigma_level_initialise(lv, B, 11)
    x[:, 0::2] = 0.5 * math.pi        # an aligned start, then cluster updates: clusters of the size the law has
    x[:, 1::2] = 0.25
    work = {"plain": ops.sigma_level_sw_workspace(lv, B), "structure": ops.sigma_level_sw_structure_workspace(lv, B),
            "correlator": ops.sigma_level_sw_correlator_workspace(lv, B)}
    counter = [0]

    def run(n, kind):
        ops.sigma_level_sw_draw(lv, x, n, 12, 0, counter[0], work=work[kind], structure=kind == "structure", correlator=kind == "correlator")
        counter[0] += n

    for _ in range(6):
        run(10, "plain")
    row = {"Mt": Mt, "Mx": Mx, "rotated": bool(rot), "chains": B, "beta": beta, "reps": reps,
           "workspace_bytes": {k: v.numel() for k, v in work.items()}}
    ms = {kind: timed(lambda: run(1, kind), reps) for kind in ("plain", "structure", "correlator")}
    ms["correlator_over_plain"] = ms["correlator"] / ms["plain"]
    ms["correlator_over_structure"] = ms["correlator"] / ms["structure"]
    row["ms_per_update_calls_of_1"] = ms
    return row


def variance(M, beta, B, burn, meas):
    lv = abi.sigma_level(M, M, 0, beta)
    x = ops.sigma_level_initialise(lv, B, 41)
    work = ops.sigma_level_sw_correlator_workspace(lv, B)
    nt = M // 2 + 1
    imp, pl = torch.zeros(B, nt, dtype=torch.float64, device="cuda"), torch.zeros(B, nt, dtype=torch.float64, device="cuda")
    for d in range(burn + meas):
        if d >= burn:
            pl += ops.sigma_level_correlator(lv, x)[:, :nt]
        out = ops.sigma_level_sw_draw(lv, x, 1, 42, 0, d, work=work, correlator=True)
        if d >= burn:
            imp += out[3][:, :nt]
    imp, pl = (imp / meas).cpu().numpy(), (pl / meas).cpu().numpy()
    err = lambda v: (v.std(axis=0, ddof=1) / math.sqrt(B)).tolist()  # noqa: E731
    e_i, e_p = err(imp), err(pl)
    return {"M": M, "beta": beta, "chains": B, "burn_in": burn, "samples_per_chain": meas, "direction": "t",
            "C_improved": imp.mean(axis=0).tolist(), "error_improved": e_i, "C_plain": pl.mean(axis=0).tolist(), "error_plain": e_p,
            "error_ratio_plain_over_improved": [p / i for p, i in zip(e_p, e_i)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_sw_correlator.json"))
    ap.add_argument("--only", choices=["cost", "variance"], default=None)
    args = ap.parse_args()
    rec = {"note": "one run each on one MI355X; records, not gates", "device": torch.cuda.get_device_name(0), "cost": [], "variance": None}
    if args.only != "variance":
        for beta in (1.0, 1.5):
            rec["cost"].append(cost(64, 64, 0, 4096, beta, 20))
            rec["cost"].append(cost(1024, 1024, 1, 32, beta, 10))
            print(json.dumps(rec["cost"][-2:]), flush=True)
    if args.only != "cost":
        rec["variance"] = variance(64, 1.5, 512, 200, 400)
        print(json.dumps(rec["variance"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
