"""mlmcpi_lattice_sweep_plan (the planner the draws of mlmcpi_lattice_sweep_draw* run, lattice2d.hip: make_sweep_plan,
next_launch) against the launches of the parent of the planner/executor split as a GPU traced them:
tests/golden/sweep_launch_trace.json, written by tools/launch_trace.py (rows [kernel name, grid x, grid y, workgroup
size, LDS_Block_Size]).  Only the last test needs a device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from mlmcpathintegral_amd import abi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = json.load(open(os.path.join(ROOT, "tests", "golden", "sweep_launch_trace.json")))
KINDS = {"schwinger": abi.SCHWINGER, "gff": abi.GFF, "sigma": abi.NONLINEAR_SIGMA}


def action_of(c):
    if c["kind"] == "gff":
        return abi.lattice_action(abi.GFF, c["Mt"], c["Mx"], mass=3.0)
    return abi.lattice_action(KINDS[c["kind"]], c["Mt"], c["Mx"], beta=c["beta"])


def plan_of(c):
    if c["option"]:
        abi.set_option(*c["option"])
    try:
        return ops.lattice_sweep_plan(action_of(c), c["B"], c["n_overrelax"], c["n_heatbath"], c["fuse"])
    finally:
        if c["option"]:
            abi.set_option(c["option"][0], "")


def instantiation(traced_name):
    """`void mlmcpi::kernel<args>(parameters) [clone .kd]` -> `kernel<args>`"""
    return re.sub(r"^void\s+", "", traced_name).split("(")[0].replace("mlmcpi::", "").replace(".kd", "").strip()


def test_the_fixture_names_its_commit_and_covers_the_kernel_families():
    assert re.fullmatch(r"[0-9a-f]{40}", TRACE["commit"])
    seen = {instantiation(row[0]).split("<")[0] for c in TRACE["cases"] for row in c["launches"]}
    assert {"schwinger_sweep_kernel", "gff_sweep_kernel", "schwinger_or_block_kernel", "gff_or_block_kernel", "gff_or_heat_kernel",
            "schwinger_perm_kernel", "schwinger_perm_heat_kernel", "sigma_sweep_kernel"} <= seen


@pytest.mark.parametrize("case", [c for c in TRACE["cases"] if c["entry"] == "draw"], ids=lambda c: c["name"])
def test_plan_names_the_launches_the_parent_made(case):
    plan = plan_of(case)
    traced = case["launches"]
    assert [l["instantiation"] for l in plan] == [instantiation(row[0]) for row in traced]
    assert [(l["grid_x"], case["B"], l["threads"]) for l in plan] == [tuple(row[1:4]) for row in traced]
    # LDS_Block_Size of the trace is the kernel's STATIC LDS in 512-byte granules (0 or 512 in all 529 rows of the fixture, under
    # launches that asked for up to 156 KiB): the dynamic bytes of a launch do not show in it, so it cannot bound them from
    # above.  What the two figures must do together is fit the 160 KiB of a CU.
    for l, row in zip(plan, traced):
        assert 0 < l["lds_bytes"] and l["lds_bytes"] + row[4] <= 160 * 1024, (l, row)
    # the records tile the draw: overrelaxation sweeps first, then the heat bath, no gap and no overlap
    s = 0
    for l in plan:
        assert l["n_overrelax"] + l["n_heatbath"] >= 1
        assert l["n_overrelax"] == min(l["n_overrelax"] + l["n_heatbath"], max(case["n_overrelax"] - s, 0))
        s += l["n_overrelax"] + l["n_heatbath"]
    assert s == case["n_overrelax"] + case["n_heatbath"]


def _raw_plan(act, B, n_or, n_hb, fuse, capacity):
    recs, count = (abi.SweepLaunch * max(capacity, 1))(), C.c_uint32(0)
    rc = abi.load().mlmcpi_lattice_sweep_plan(C.byref(act), B, n_or, n_hb, fuse, recs, capacity, C.byref(count))
    return rc, count.value


def test_plan_refuses_what_a_draw_refuses():
    INVALID = -1
    assert _raw_plan(abi.lattice_action(abi.SCHWINGER, 65, 64, beta=1.0), 2, 10, 1, 0, 16)[0] == INVALID   # odd extent
    assert _raw_plan(abi.lattice_action(abi.NONLINEAR_SIGMA, 64, 33, beta=1.0), 2, 10, 1, 0, 16)[0] == INVALID
    assert _raw_plan(abi.lattice_action(abi.GFF, 64, 32, mass=3.0), 2, 10, 1, 0, 16)[0] == INVALID         # GFF: square only
    assert _raw_plan(abi.lattice_action(abi.GFF, 64, 64, mass=3.0), 0, 10, 1, 0, 16)[0] == INVALID         # no chains
    assert _raw_plan(abi.lattice_action(abi.ROTOR, 64, 64), 2, 10, 1, 0, 16)[0] == INVALID                  # not a 2-D action
    act = abi.lattice_action(abi.GFF, 64, 64, mass=3.0)   # 10 + 1 sweeps: 5 | 5 + heat bath
    assert _raw_plan(act, 2, 10, 1, 0, 2) == (0, 2)
    assert _raw_plan(act, 2, 10, 1, 0, 1) == (INVALID, 2) and b"capacity" in abi.load().mlmcpi_last_error()
    assert _raw_plan(act, 2, 10, 1, 0, 0) == (INVALID, 2)
    assert _raw_plan(act, 2, 0, 0, 0, 0) == (0, 0)


def test_plan_needs_no_device():
    """a fresh process that sees no GPU at all (this is what the test is about: the parent process may have one)"""
    code = ("from mlmcpathintegral_amd import abi, ops\n"
            "p = ops.lattice_sweep_plan(abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0), 1, 10, 1)\n"
            "print([l['instantiation'] for l in p])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "['schwinger_perm_heat_kernel<1024, true>']"


def _draw_from(ops, act, src, w0, w1, n_or, n_hb, sweep0, fuse):
    where = C.c_int32(-2)
    abi.call("mlmcpi_lattice_sweep_draw_from", C.byref(act), ops._p(src), ops._p(w0), ops._p(w1), src.shape[0], n_or, n_hb, 11, 0,
             sweep0, fuse, C.byref(where), ops._stream())
    return where.value


@pytest.mark.gpu
def test_draws_follow_the_plan(gpu_ops):
    """Six cases of the fixture, one per kernel family: closed form (13 + 1 sweeps: 7, then 6 with the heat bath), Schwinger register blocks, the
    generic Schwinger and GFF tile kernels, GFF register blocks, sigma model.  The draw ends in the work buffer the number of
    planned launches says, and equals -- bit for bit -- the same sweeps issued launch by launch from the plan's depths."""
    import torch
    ops = gpu_ops
    names = ("schwinger 128x128 B=1 beta=1 (13,1) fuse=0", "schwinger 128x128 B=2 beta=1 (10,1) fuse=0 MLMCPI_OR_KERNEL=block",
             "schwinger 66x34 B=2 beta=1 (10,1) fuse=0", "gff 64x64 B=2 beta=1 (10,1) fuse=0", "gff 32x32 B=2 beta=1 (10,1) fuse=0",
             "sigma 64x64 B=2 beta=1 (10,1) fuse=0")
    for case in (c for c in TRACE["cases"] if c["name"] in names):
        option, n_or, B = case["option"], case["n_overrelax"], case["B"]
        act, plan = action_of(case), plan_of(case)
        assert len(plan) >= 2
        x0 = ops.lattice_initialise(act, B, 5)
        w0, w1, u, v = (torch.empty_like(x0) for _ in range(4))
        if option:
            abi.set_option(*option)
        try:
            where = _draw_from(ops, act, x0, w0, w1, n_or, 1, 3, 0)
            assert where == (len(plan) - 1) % 2, (case, where, len(plan))
            src, s = x0, 0
            for l in plan:   # a draw of the launch's own sweeps is that one launch, and writes its first work buffer
                assert ops.lattice_sweep_plan(act, B, l["n_overrelax"], l["n_heatbath"]) == [l], (case, l)
                assert _draw_from(ops, act, src, u, v, l["n_overrelax"], l["n_heatbath"], 3 + s, 0) == 0
                src, u, v, s = u, v, u, s + l["n_overrelax"] + l["n_heatbath"]
        finally:
            if option:
                abi.set_option(option[0], "")
        assert torch.equal(src, w1 if where else w0), case
    assert sum(c["name"] in names for c in TRACE["cases"]) == len(names)
