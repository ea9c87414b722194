#!/usr/bin/env python3
"""Records of the cluster-improved structure factor of the Swendsen-Wang update: what the structure
outputs cost, and what they buy for xi_2.  One run each, not gates.  Writes profiles/sigma_sw_structure.json.

Cost: the time of an update through mlmcpi_sigma_level_sw_structure_draw against the same update through
mlmcpi_sigma_level_sw_draw (all outputs asked for), events around `reps` calls after warm-up, at 64 x 64 x 4096 chains (chain
plan) and the rotated partner of 1024 x 1024 x 32 chains (tiled plan), beta = 1 and 1.5, in calls of 1 update (what the sampler
issues) and of 10 updates.  Variance: 64 x 64, beta = 1.5, the jackknife error over the chains of xi_2 from the improved (chi, F)
against that from the plain ones of mlmcpi_sigma_level_correlator on the same states, equal samples.

    python tools/time_sigma_sw_structure.py [--out profiles/sigma_sw_structure.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
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
    plain, struct = ops.sigma_level_sw_workspace(lv, B), ops.sigma_level_sw_structure_workspace(lv, B)
    counter = [0]

    def run(n, structure):
        ops.sigma_level_sw_draw(lv, x, n, 12, 0, counter[0], work=struct if structure else plain, structure=structure)
        counter[0] += n

    for _ in range(6):
        run(10, False)
    row = {"Mt": Mt, "Mx": Mx, "rotated": bool(rot), "chains": B, "beta": beta, "reps": reps}
    for n in (1, 10):
        a = timed(lambda: run(n, False), reps) / n
        b = timed(lambda: run(n, True), reps) / n
        row[f"ms_per_update_calls_of_{n}"] = {"plain": a, "structure": b, "ratio": b / a}
    return row


def variance(M, beta, B, burn, meas):
    lv = abi.sigma_level(M, M, 0, beta)
    x = ops.sigma_level_initialise(lv, B, 41)
    work = ops.sigma_level_sw_structure_workspace(lv, B)
    w = torch.full((M // 2 + 1,), 2.0, dtype=torch.float64, device="cuda")
    w[0] = w[-1] = 1.0
    cosw = w * torch.cos(2.0 * math.pi * torch.arange(M // 2 + 1, device="cuda", dtype=torch.float64) / M)
    acc = torch.zeros(4, B, dtype=torch.float64, device="cuda")      # improved chi, F_t; plain chi, F_t
    for d in range(burn + meas):
        if d >= burn:
            Ct = ops.sigma_level_correlator(lv, x)[:, :M // 2 + 1]
            acc[2] += (Ct * w).sum(dim=1)
            acc[3] += (Ct * cosw).sum(dim=1)
        out = ops.sigma_level_sw_draw(lv, x, 1, 42, 0, d, work=work, structure=True)
        if d >= burn:
            acc[0] += out[2]
            acc[1] += out[3][:, 0]
    m = (acc / meas).cpu().numpy()

    def xi(chi, F):
        f = lambda c, g: math.sqrt(c / g - 1.0) / (2.0 * math.sin(math.pi / M))  # noqa: E731
        jk = np.array([f((chi.sum() - chi[b]) / (B - 1), (F.sum() - F[b]) / (B - 1)) for b in range(B)])
        return f(chi.mean(), F.mean()), math.sqrt((B - 1) / B * ((jk - jk.mean()) ** 2).sum())

    (xi_i, e_i), (xi_p, e_p) = xi(m[0], m[1]), xi(m[2], m[3])
    return {"M": M, "beta": beta, "chains": B, "burn_in": burn, "samples_per_chain": meas, "direction": "t",
            "xi2_improved": xi_i, "error_improved": e_i, "xi2_plain": xi_p, "error_plain": e_p, "error_ratio_plain_over_improved": e_p / e_i,
            "variance_ratio": (e_p / e_i) ** 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_sw_structure.json"))
    args = ap.parse_args()
    rec = {"note": "one run each on one MI355X; records, not gates", "device": torch.cuda.get_device_name(0), "cost": [], "variance": None}
    for beta in (1.0, 1.5):
        rec["cost"].append(cost(64, 64, 0, 4096, beta, 20))
        rec["cost"].append(cost(1024, 1024, 1, 32, beta, 10))
        print(json.dumps(rec["cost"][-2:]), flush=True)
    rec["variance"] = variance(64, 1.5, 512, 200, 400)
    print(json.dumps(rec["variance"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
