#!/usr/bin/env python3
"""Draw time of the O(3) sigma model at 1024^2 x 32 chains (10 overrelaxation + 1 heat-bath sweeps + the fused chi_m, one
ops.lattice_sweep_draw_qoi call) by fuse depth and sweep tile (MLMCPI_SWEEP_TILE), event-timed; HBM floor = state read +
written once per launch (16 B per vertex each way).   python tools/exp_sigma_time.py [out.json]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mlmcpathintegral_amd import abi, ops
abi.load()
N, B, n_or, n_hb = 1024, 32, 10, 1
act = abi.lattice_action(abi.NONLINEAR_SIGMA, N, N, beta=1.0)
src = ops.lattice_initialise(act, B, 7)
w0, w1 = torch.empty_like(src), torch.empty_like(src)
floor_ms = 2 * 8 * src.numel() / 8e12 * 1e3  # one launch's read + write at 8 TB/s
rows = []
for tile in ("", "32x32x256", "32x32x512", "64x64x256", "64x64x512", "64x32x256"):
    abi.set_option("MLMCPI_SWEEP_TILE", tile)
    for fuse in (1, 2, 3, 4):
        sweep = 0
        def draw():
            global src, w0, w1, sweep
            res, other, q = ops.lattice_sweep_draw_qoi(act, src, w0, w1, n_or, n_hb, 7, 0, sweep, 4, fuse=fuse)
            src, w0, w1 = res, other, src
            sweep += n_or + n_hb
        for _ in range(3):
            draw()
        times = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); draw(); e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        launches = -(-(n_or + n_hb) // fuse)
        row = {"tile": tile or "default", "fuse": fuse, "ms_per_draw_median": statistics.median(times), "ms_per_draw_min": min(times),
               "launches": launches, "vertex_updates_per_s": N * N * B * (n_or + n_hb) / (statistics.median(times) * 1e-3),
               "hbm_floor_ms_per_draw": floor_ms * launches}
        rows.append(row)
        print(json.dumps(row), flush=True)
abi.set_option("MLMCPI_SWEEP_TILE", "")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"shape": [N, N], "batch": B, "n_overrelax": n_or, "n_heatbath": n_hb, "rows": rows}, f, indent=1)
