"""mlmcpi_path_hmc_plan (host only: the geometry plan_hmc of path_hmc.hip chooses from (kind, M, B, nt)) against the rule as
tests/path_hmc_cases.py restates it, the invariants every plan must keep, and the conditions the cases of
tests/test_path_hmc_geometry_gpu.py rely on, which are properties of the plan and of the oracle's numbers alone: each case
reaches the geometry it names, both Metropolis outcomes occur where a test asserts them, and no accept test the GPU tests
assert on is a near-tie.  Nothing here needs a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import path_hmc_cases as hc
from path_cases import KINDS, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_plan(kind, M, B, nt):
    """(status, plan or None) straight through the ABI"""
    from mlmcpathintegral_amd import abi
    act = abi.path_action(KINDS[kind], M, M / 8.0, 1.0, 1.0, 1.0, 1.0)
    info = abi.PathHmcPlan(*([0xFFFFFFFF] * 5), -1)
    rc = abi.load().mlmcpi_path_hmc_plan(C.byref(act), B, nt, C.byref(info))
    return rc, ({n: getattr(info, n) for n in hc.FIELDS} if rc == 0 else None)


@pytest.fixture(scope="module")
def grid():
    """{(kind, M, B, nt): (status, plan)} from the ABI over the whole grid"""
    return {(k, M, B, nt): raw_plan(k, M, B, nt) for k in KINDS for M in hc.GRID_M for B in hc.GRID_B for nt in hc.GRID_NT}


def test_the_grid_is_the_one_asked_for():
    assert hc.GRID_M[:70] == list(range(1, 71)) and hc.GRID_M[70:-5] == [64 * k for k in range(2, 129)]
    assert hc.GRID_M[-5:] == [8193, 8200, 12000, 32768, 65536]
    assert hc.GRID_B == (1, 2, 255, 256, 512, 1024, 2048, 2100) and hc.GRID_NT == (1, 5, 100, 479, 480, 2015, 2016)


def test_query_equals_the_restated_rule(grid):
    refused = 0
    for key, got in grid.items():
        assert got == hc.plan(*key), (key, got, hc.plan(*key))
        refused += got[0] != 0
    # M = 1 is no path; nt too long for the buffer: both MLMCPI_ERR_INVALID
    assert all(grid[(k, 1, B, nt)][0] == hc.ERR_INVALID for k in KINDS for B in hc.GRID_B for nt in hc.GRID_NT)
    assert refused > 3 * 8 * 7 and len(grid) - refused > 10000
    assert grid[("quartic", 10, 2, 479)][0] == 0 and grid[("quartic", 10, 2, 480)][0] == hc.ERR_INVALID
    assert grid[("rotor", 8200, 2, 2015)][0] == 0 and grid[("rotor", 8200, 2, 2016)][0] == hc.ERR_INVALID


def test_refusal_is_the_one_the_draw_gives():
    from mlmcpathintegral_amd import abi
    lib, size, info = abi.load(), C.c_size_t(0), abi.PathHmcPlan()
    act = abi.path_action(abi.HARMONIC, 10, 1.25)
    assert lib.mlmcpi_path_hmc_plan(C.byref(act), 3, 480, C.byref(info)) == hc.ERR_INVALID
    message = lib.mlmcpi_last_error()
    assert b"nt = 480 too long" in message and b"max 479" in message
    assert lib.mlmcpi_path_hmc_workspace_bytes(C.byref(act), 3, 480, C.byref(size)) == hc.ERR_INVALID
    assert lib.mlmcpi_last_error() == message
    # nothing is launched for a refused nt: the draw returns the same status before it touches its buffers (host memory here)
    work = (C.c_char * 4096)()
    assert lib.mlmcpi_path_hmc_draw(C.byref(act), work, 3, 480, 0.004, 1, 1, 0, 0, work, None, None, None) == hc.ERR_INVALID
    assert lib.mlmcpi_last_error() == message
    assert lib.mlmcpi_path_hmc_plan(C.byref(act), 0, 5, C.byref(info)) == hc.ERR_INVALID      # no chains
    assert lib.mlmcpi_path_hmc_plan(C.byref(act), 3, 5, None) == hc.ERR_INVALID                # nowhere to write
    assert lib.mlmcpi_path_hmc_plan(None, 3, 5, C.byref(info)) == hc.ERR_INVALID
    lat = abi.path_action(abi.GFF, 64, 8.0)
    assert lib.mlmcpi_path_hmc_plan(C.byref(lat), 3, 5, C.byref(info)) == hc.ERR_INVALID      # not a 1-D path action


def test_plans_keep_their_invariants(grid):
    for (kind, M, B, nt), (rc, p) in grid.items():
        if rc:
            continue
        key = (kind, M, B, nt, p)
        assert p["NT"] % 64 == 0 and p["NT"] <= (512 if p["R"] >= 8 else 1024), key
        assert p["R"] in (1, 2, 4, 8, 16) and (kind != "rotor" or p["R"] <= 8), key
        assert p["chain_major"] == (1 if p["halo"] == 0 else 0), key
        if p["halo"] == 0:
            assert p["NT"] * p["R"] == M and p["nseg"] == 1 and p["owned_len"] == M, key
        else:
            assert p["halo"] == nt + 1 and p["owned_len"] + 2 * p["halo"] <= p["NT"] * p["R"], key
            assert (p["nseg"] - 1) * p["owned_len"] < M <= p["nseg"] * p["owned_len"], key
        # the owned ranges tile [0, M) exactly once
        ranges = hc.owned_ranges(p, M)
        assert ranges[0][0] == 0 and ranges[-1][1] == M and all(lo < hi for lo, hi in ranges), key
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), key


def test_run_layout_agrees_with_chain_major(grid):
    from mlmcpathintegral_amd import abi
    lib = abi.load()
    for (kind, M, B, nt), (rc, p) in grid.items():
        if M > 200 and B not in (2, 2100) or nt not in (5, 480, 2016):
            continue
        act, layout = abi.path_action(KINDS[kind], M, M / 8.0), C.c_int32(-1)
        assert lib.mlmcpi_path_hmc_run_layout(C.byref(act), B, nt, C.byref(layout)) == rc, (kind, M, B, nt)
        assert rc or layout.value == p["chain_major"], (kind, M, B, nt)


def _cases():
    for c in hc.SEGMENTED:
        yield c["kind"], c["M"], hc.SEG_B, c["nt"], c["plan"]
        yield c["kind"], c["M"], 1, c["nt"], c["plan"]            # the plan of a segmented path does not depend on B
    for c in hc.BATCH:
        yield c["kind"], c["M"], c["B"], hc.BATCH_NT, c["plan"]
    for c in hc.RUN:
        yield c["kind"], c["M"], hc.RUN_B, hc.RUN_NT, c["plan"]
    c = hc.SEGMENTED_RUN
    yield c["kind"], c["M"], hc.RUN_B, c["nt"], c["plan"]


def test_every_case_reaches_the_geometry_it_names():
    for kind, M, B, nt, want in _cases():
        assert raw_plan(kind, M, B, nt) == (0, want), (kind, M, B, nt)
    for c in hc.SEGMENTED:
        if "refused" in c:
            assert raw_plan(c["kind"], c["M"], hc.SEG_B, c["refused"] - 1)[0] == 0 and c["refused"] == c["nt"] + 1
            assert raw_plan(c["kind"], c["M"], hc.SEG_B, c["refused"]) == (hc.ERR_INVALID, None)
    # what the issue lists as never run, by the plan that shows it is reached
    seg = {(c["kind"], c["M"], c["nt"]): c["plan"] for c in hc.SEGMENTED}
    assert all(p["halo"] > M for (k, M, nt), p in seg.items() if M <= 16)                              # 1. shorter than the halo
    assert seg[("quartic", 1000, 11)]["R"] == 4 and 1000 + 2 * seg[("quartic", 1000, 11)]["halo"] == 1024   # 2. the branch boundary
    assert (seg[("rotor", 1000, 12)]["R"], seg[("rotor", 1000, 12)]["NT"], seg[("rotor", 1000, 12)]["nseg"]) == (8, 512, 1)
    assert seg[("quartic", 8200, 10)]["nseg"] == 3 and seg[("rotor", 4160, 10)]["nseg"] == 2             # 3. smallest multi-segment
    assert hc.owned_ranges(seg[("quartic", 8200, 10)], 8200)[-1] == (5468, 8200)
    assert 2 * seg[("harmonic", 10, 479)]["halo"] + 64 == 1024 and 2 * seg[("quartic", 1000, 2015)]["halo"] + 64 == 4096   # 4. the nt limit
    assert {(c["plan"]["R"], c["plan"]["NT"]) for c in hc.BATCH} == {(2, 512), (4, 256), (8, 128), (16, 128)}      # 5. batch-selected
    assert {(c["kind"], c["plan"]["R"], c["plan"]["NT"]) for c in hc.RUN} == {
        ("quartic", 2, 1024), ("quartic", 4, 1024), ("quartic", 16, 512), ("rotor", 2, 1024), ("rotor", 4, 1024)}   # 6. multi-wave R > 1
    # memory: the largest case is 1024 x 2048 doubles
    assert max(c["M"] * c["B"] * 8 for c in hc.BATCH) == 16 * 2 ** 20


def test_new_symbol_is_declared_exported_and_bound():
    from mlmcpathintegral_amd import abi, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlmcpi_hip.h")).read(), flags=re.S)
    lib = abi.load()
    assert re.search(r"\bmlmcpi_path_hmc_plan\s*\(", header), "mlmcpi_path_hmc_plan is not declared"
    assert hasattr(lib, "mlmcpi_path_hmc_plan") and "mlmcpi_path_hmc_plan" in abi.SIGNATURES
    # the struct of the header, field by field
    body = re.search(r"typedef struct mlmcpi_path_hmc_plan_info \{(.*?)\} mlmcpi_path_hmc_plan_info;", header, flags=re.S).group(1)
    declared = [(t, n.strip()) for t, names in re.findall(r"(uint32_t|int32_t)\s+([^;]+);", body) for n in names.split(",")]
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in declared] == list(abi.PathHmcPlan._fields_)
    assert tuple(n for n, _ in abi.PathHmcPlan._fields_) == hc.FIELDS
    assert lib.mlmcpi_abi_version() == 1
    act = abi.path_action(abi.ROTOR, 4160, 520.0, 0.25)
    assert ops.path_hmc_plan(act, 3, 10) == hc.plan("rotor", 4160, 3, 10)[1]
    with pytest.raises(abi.MlmcpiError, match="too long for the fused trajectory"):
        ops.path_hmc_plan(act, 3, 2016)


def test_plan_needs_no_device():
    """a fresh process that sees no GPU at all (this is what the test is about: the parent process may have one): the
    query answers as it does here, MLMCPI_OK and MLMCPI_ERR_INVALID, where a call that needs the device reports that there
    is none"""
    code = ("import ctypes as C\n"
            "from mlmcpathintegral_amd import abi, ops\n"
            "act = abi.path_action(abi.QUARTIC, 8200, 1025.0, 1.0, 1.0, 1.0, 1.0)\n"
            "p = ops.path_hmc_plan(act, 3, 10)\n"
            "info, n = abi.PathHmcPlan(), C.c_int(-1)\n"
            "print([p[k] for k in ('R', 'NT', 'nseg', 'owned_len', 'halo', 'chain_major')],\n"
            "      abi.load().mlmcpi_path_hmc_plan(C.byref(act), 3, 2016, C.byref(info)), abi.load().mlmcpi_device_count(C.byref(n)))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "[16, 256, 3, 2734, 11, 0] -1 -4"


# ---- what the GPU cases rely on, from the oracle alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(hc.SEGMENTED)), ids=lambda i: "{kind}-{M}-{nt}".format(**hc.SEGMENTED[i]))
def test_segmented_cases_under_the_oracle(orc, i):
    c = hc.SEGMENTED[i]
    x0, flags, energies, states, margin = hc.segmented_run(i)
    assert margin > hc.MARGIN, (c, margin)
    assert flags.shape == (hc.SEG_B, hc.SEG_DRAWS) and flags.any()
    assert len({x0[b].tobytes() for b in range(hc.SEG_B)}) == hc.SEG_B
    if c.get("long"):
        assert c["nt"] * c["dt"] <= 2.0
        worst, counted = hc.ulp_sensitivity(i)
        assert counted == hc.SEG_B * hc.SEG_DRAWS and 0 < worst < 1e-13, (worst, counted)
        print(f"[hmc] {c['kind']} M={c['M']} nt={c['nt']}: one ulp at the start moves the oracle's state by {worst:.3e}; "
              f"bound of the GPU test {100 * worst:.3e}")
    else:
        assert c["nt"] <= 100


@pytest.mark.parametrize("i", range(len(hc.BATCH)), ids=lambda i: "{kind}-{M}-{B}".format(**hc.BATCH[i]))
def test_batch_cases_under_the_oracle(orc, i):
    """both outcomes among the first 48 chains (the table's counts), and no near-tie on the chains compared with the oracle"""
    c = hc.BATCH[i]
    counts, _, _, _ = hc.batch_outcomes(i, tuple(range(48)))
    hist = np.bincount(counts, minlength=hc.BATCH_DRAWS + 1).tolist()
    print(f"[hmc] {c['kind']} M={c['M']} B={c['B']} dt={c['dt']}: accepted draws 0/1/2 of 48 chains: {hist}")
    assert hist[hc.BATCH_DRAWS] < 48 and hist[0] < 48
    assert hc.batch_outcomes(i, hc.batch_chains(c["B"]))[3] > hc.MARGIN


@pytest.mark.parametrize("i", range(len(hc.RUN)), ids=lambda i: "{kind}-{M}".format(**hc.RUN[i]))
def test_run_cases_under_the_oracle(orc, i):
    """a rejected repetition and an accepted draw among the three chains, for the 3-draw and the 5-draw run; no near-tie;
    the rotor's neighbour differences keep away from the branch cut of mod_2pi (its QoI is compared with the oracle's)"""
    c = hc.RUN[i]
    for n in (hc.RUN_DRAWS, 5):
        _, flags, _, q, rejected, margin, cut = hc.run_outcomes(i, n)
        print(f"[hmc] {c['kind']} M={c['M']} dt={c['dt']} {n} draws: accepted {flags.sum(axis=1).tolist()}, {rejected} rejected repetitions")
        assert rejected >= 1 and flags.any() and not flags.all(), (c, flags)
        assert margin > hc.MARGIN and np.isfinite(q).all()
        if c["kind"] == "rotor":
            assert cut > 1e-5, cut
            assert (q > 1e-3).any(), "some charge is not zero"
    assert params(c["kind"], c["M"])["T_final"] == c["M"] / 8.0
