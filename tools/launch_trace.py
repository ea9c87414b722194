#!/usr/bin/env python3
"""The kernel launches of a fixed list of mlmcpi_lattice_sweep_draw* calls, as the GPU saw them.

    python tools/launch_trace.py --commit <hash> > tests/golden/sweep_launch_trace.json

The parent process runs `rocprofv3 --kernel-trace` over a fresh child python (this file with --child) and writes, per
case, the ordered rows [kernel name, grid x, grid y, workgroup size, LDS_Block_Size] of the library's kernels (grid in
workgroups; LDS_Block_Size is static + dynamic LDS after allocation rounding).  The child initialises every state first and
then puts a one-element int16 fill in front of every case; the parent splits the trace on those fills, so which rows belong
to a case does not depend on the library's launch plan.  The tail copy of a draw is not a kernel and does not show.

A refactor of the launch path takes the trace of its parent (build the parent's library as a variant, tools/build_variant.sh,
and run this with MLMCPI_LIB_VARIANT set), commits it as the fixture, and shows that its own trace equals it row for row;
tests/test_sweep_plan.py holds mlmcpi_lattice_sweep_plan against the same fixture without a GPU.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = "FillFunctor<short>"   # the one-element int16 fill between cases
QOI_OF = {"schwinger": 1, "gff": 3, "sigma": 4}


def case(kind, Mt, Mx, n_or, n_hb, B=2, beta=1.0, fuse=0, option=None, entry="draw"):
    name = f"{kind} {Mt}x{Mx} B={B} beta={beta:g} ({n_or},{n_hb}) fuse={fuse}"
    if option:
        name += " " + "=".join(option)
    if entry != "draw":
        name += " " + entry
    return dict(name=name, kind=kind, Mt=Mt, Mx=Mx, B=B, beta=beta, n_overrelax=n_or, n_heatbath=n_hb, fuse=fuse,
                option=list(option) if option else None, entry=entry)


def cases():
    out = []
    for B in (1, 65):   # wide / narrow workgroups of the fused closed-form launch
        for n_or in (7, 10, 13):
            out.append(case("schwinger", 128, 128, n_or, 1, B=B))
    out.append(case("schwinger", 128, 128, 10, 0))
    out += [case("schwinger", 128, 64, 0, 1, beta=beta) for beta in (1.0, 10.0)]   # step / wrapped-Cauchy sampler
    out += [case("schwinger", Mt, Mx, 10, 1) for Mt, Mx in ((64, 64), (64, 32), (130, 70), (66, 34), (16, 16), (4, 4))]
    out.append(case("schwinger", 66, 34, 16, 0, fuse=16))   # the fused count shrinks until tile + halo fits in LDS
    for M in (32, 64, 66, 96, 100, 128):
        out += [case("gff", M, M, n_or, n_hb) for n_or, n_hb in ((10, 1), (6, 1), (5, 0), (13, 0))]
    for Mt, Mx in ((16, 16), (64, 64), (130, 70)):
        for fuse in (0, 1, 5):
            out += [case("sigma", Mt, Mx, n_or, 1, fuse=fuse) for n_or in (10, 0)]
    options = [("MLMCPI_OR_KERNEL", "block"), ("MLMCPI_OR_HEAT", "split"), ("MLMCPI_OR_HEAT", "wide"),
               ("MLMCPI_OR_HEAT", "narrow"), ("MLMCPI_SWEEP_TILE", "32x32x512"), ("MLMCPI_SWEEP_TILE", "64x32x1024")]
    for kind, M in (("schwinger", 128), ("gff", 128), ("sigma", 64)):
        for entry in ("draw", "qoi", "qoi_record"):
            out += [case(kind, M, M, 10, 1, option=o, entry=entry) for o in options]
            out += [case(kind, M, M, 10, 1, fuse=f, entry=entry) for f in (0, 2, 4, 6)]
    return list({c["name"]: c for c in out}.values())   # (the default-fuse draws of the last block repeat two table cases)


def action_of(c):
    from mlmcpathintegral_amd import abi
    if c["kind"] == "gff":
        return abi.lattice_action(abi.GFF, c["Mt"], c["Mx"], mass=3.0)
    return abi.lattice_action(abi.SCHWINGER if c["kind"] == "schwinger" else abi.NONLINEAR_SIGMA, c["Mt"], c["Mx"], beta=c["beta"])


def child():
    sys.path.insert(0, ROOT)
    import torch
    from mlmcpathintegral_amd import abi, ops
    todo, states = [], {}
    for c in cases():   # every allocation and initialisation first: nothing but the draw follows a marker
        act = action_of(c)
        key = (c["kind"], c["Mt"], c["Mx"], c["B"], c["beta"])
        if key not in states:
            states[key] = ops.lattice_initialise(act, c["B"], 3)
        x = states[key]
        acc = torch.zeros((c["B"], 5), dtype=torch.float64, device=x.device)
        todo.append((c, act, x, torch.empty_like(x), torch.empty_like(x), acc))
    marker = torch.empty(1, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for i, (c, act, x, w0, w1, acc) in enumerate(todo):
        marker.fill_(i)
        if c["option"]:
            abi.set_option(*c["option"])
        try:
            if c["entry"] == "draw":
                ops.lattice_sweep_draw(act, x, w0, c["n_overrelax"], c["n_heatbath"], 3, 0, 0, c["fuse"])
            else:
                ops.lattice_sweep_draw_qoi(act, x, w0, w1, c["n_overrelax"], c["n_heatbath"], 3, 0, 0, QOI_OF[c["kind"]], c["fuse"],
                                           acc=acc if c["entry"] == "qoi_record" else None)
        finally:
            if c["option"]:
                abi.set_option(c["option"][0], "")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", action="store_true", help="run the draws (what the parent process traces)")
    ap.add_argument("--commit", default="", help="the commit the traced library was built from (recorded in the output)")
    args = ap.parse_args()
    if args.child:
        return child()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                        os.path.abspath(__file__), "--child"], check=True, stdout=sys.stderr)
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_case = []
    for r in rows:
        if MARKER in r["Kernel_Name"]:
            per_case.append([])
        elif per_case and "mlmcpi::" in r["Kernel_Name"]:
            wg = int(r["Workgroup_Size_X"])
            per_case[-1].append([r["Kernel_Name"], int(r["Grid_Size_X"]) // wg, int(r["Grid_Size_Y"]), wg, int(r["LDS_Block_Size"])])
    todo = cases()
    if len(per_case) != len(todo):
        sys.exit(f"launch_trace: {len(per_case)} markers in the trace for {len(todo)} cases")
    for c, launches in zip(todo, per_case):
        c["launches"] = launches
    json.dump({"commit": args.commit, "variant": os.environ.get("MLMCPI_LIB_VARIANT", ""),
               "how": "tools/launch_trace.py: rows are [kernel name, grid x, grid y, workgroup size, LDS_Block_Size]",
               "cases": todo}, sys.stdout, indent=0)
    print()


if __name__ == "__main__":
    main()
