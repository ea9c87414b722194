"""CPU: mlmcpi_set_option and the environment loading of the tuning knobs (options.hip), knob by knob: every accepted
spelling, a set of refused ones, the status and message of a refusal, and -- for the three knobs whose effect shows in the
host-only mlmcpi_lattice_sweep_plan -- that a refused value and "" both put the knob back to its default.  The library
loads without a GPU; nothing here touches one."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from mlmcpathintegral_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # MLMCPI_ERR_INVALID

# name -> (accepted spellings, refused spellings).  "" (the default) is accepted by every knob.
KNOBS = {
    "MLMCPI_SWEEP_TILE": (["", "64x32x256", "128x64x512", "2x2x1024", "32x32x512"],
                          ["63x32x256", "64x31x256", "0x32x256", "64x0x256", "64x32x100", "64x32x0", "64x32", "64", "x", "auto",
                           "64X32X256", "1x32x256"]),
    "MLMCPI_OR_KERNEL": (["", "block", "perm"], ["auto", "blocks", "Block", "lds", "patch", "block ", "0"]),
    "MLMCPI_OR_HEAT": (["", "split", "fused", "wide", "narrow"], ["auto", "sideways", "Split", "wide ", "1"]),
    "MLMCPI_RANDOM_SWEEP_HOME": (["", "global", "lds"], ["auto", "Global", "hbm", "lds ", "1"]),
    "MLMCPI_RANDOM_SWEEP_CHUNK": (["", "1", "100", "254"], ["0", "255", "1000", "abc", "x7", "-1"]),
    "MLMCPI_SIGMA_CLUSTER_TEAM": (["", "auto", "wave", "block"], ["Wave", "waves", "thread", "auto ", "2"]),
    "MLMCPI_SIGMA_CLUSTER_BITMAP": (["", "global", "lds"], ["auto", "Global", "workspace", " lds", "1"]),
    "MLMCPI_SIGMA_SW_PLAN": (["", "auto", "chain", "tiled"], ["Chain", "tile", "chains", "tiled ", "1"]),
    "MLMCPI_SIGMA_SW_TILE": (["", "8x8", "16x64", "64x32", "32x32", "64x64"],
                             ["8x8x", "8x8 ", "8x12", "12x8", "128x8", "8x128", "4x8", "0x0", "8", "8x", "x8", "auto", "64x32x256"]),
    "MLMCPI_SIGMA_LEVEL_PLAN": (["", "32x32x512x2", "1x1x256x1", "128x1x1024x1", "26x26x256x16", "64x32x512x1"],
                                ["32x32x512x2z", "32x32x512x2 ", "32x32x512", "0x32x512x2", "32x0x512x2", "129x1x256x1", "1x129x256x1",
                                 "32x32x100x2", "32x32x512x0", "32x32x512x17", "27x26x256x16", "128x128x256x1", "auto"]),
    # the spellings of test_sigma_cooling_gpu.py / test_sigma_flow_gpu.py (their plans and test_the_knob_refuses_what_does_not_fit),
    # and the trailing-character and field-count cases of _LEVEL_PLAN
    "MLMCPI_SIGMA_COOL_PLAN": (["", "32x32x512x2", "1x1x256x1", "8x4x256x4", "48x48x1024x1", "7x5x512x3", "16x16x512x16", "128x1x1024x1"],
                               ["0x4x256x1", "4x4x128x1", "4x4x256x0", "4x4x256x17", "64x64x256x1x", "20x20x256x16", "129x1x256x1",
                                "1x129x256x1", "32x32x512x2z", "32x32x512x2 ", "32x32x512", "32x32x512x2x1", "auto"]),
    "MLMCPI_SIGMA_FLOW_PLAN": (["", "16x16x512x1", "2x2x256x5", "27x27x512x1", "128x1x1024x1", "1x1x256x1", "8x4x256x2", "7x5x512x3"],
                               ["0x4x256x1", "4x4x128x1", "4x4x256x0", "4x4x256x17", "16x16x256x1x", "2x2x256x6", "32x32x512x1",
                                "129x1x256x1", "1x129x256x1", "16x16x512x1z", "16x16x512x1 ", "16x16x512", "16x16x512x1x1", "auto"]),
    "MLMCPI_SIGMA_TWOLEVEL_GROUPS": (["", "1", "7", "64"], ["0", "65", "7x", "7 ", "abc", "-1", "auto"]),
}


def set_raw(name, value):
    """(status, message) of mlmcpi_set_option, not turned into an exception"""
    lib = abi.load()
    rc = lib.mlmcpi_set_option(None if name is None else name.encode(), None if value is None else value.encode())
    return rc, lib.mlmcpi_last_error().decode()


def refused(name, value):
    rc, msg = set_raw(name, value)
    show = lambda s: "(null)" if s is None else s
    return rc == INVALID and msg == "unknown option or value: %s=%s" % (show(name), show(value)), (name, value, rc, msg)


def test_the_table_covers_the_thirteen_knobs():
    assert len(KNOBS) == 13
    for name, (good, bad) in KNOBS.items():
        assert "" in good and len(good) >= 3 and len(bad) >= 5 and not set(good) & set(bad), name


@pytest.mark.parametrize("name", sorted(KNOBS))
def test_every_accepted_spelling_is_accepted_and_the_rest_refused(name):
    good, bad = KNOBS[name]
    try:
        for v in good:
            assert set_raw(name, v)[0] == 0, (name, v, set_raw(name, v))
        for v in bad:
            ok, what = refused(name, v)
            assert ok, what
        assert set_raw(name, None)[0] == 0   # a NULL value is the empty one
    finally:
        abi.set_option(name, "")


def test_unknown_names_are_refused():
    for name in ("MLMCPI_NO_SUCH_KNOB", "MLMCPI_OR_THREADS", "mlmcpi_sweep_tile", "MLMCPI_SWEEP_TILE ", "SWEEP_TILE", "", None):
        for v in ("", "1", "block", None):
            ok, what = refused(name, v)
            assert ok, what


def test_trailing_characters_the_parent_lets_through():
    """Two quirks, pinned as they are and not fixed: the formats of MLMCPI_SWEEP_TILE and MLMCPI_RANDOM_SWEEP_CHUNK end without
    the %c that the other numeric knobs use to refuse trailing characters, so whatever follows the last number is ignored."""
    act = abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0)
    try:
        # quirk, not a promise: "64x32x256z" is taken as 64x32x256
        assert set_raw("MLMCPI_SWEEP_TILE", "64x32x256z")[0] == 0
        with_z = _launches(act, 1)
        assert set_raw("MLMCPI_SWEEP_TILE", "64x32x256")[0] == 0
        assert with_z == _launches(act, 1) and with_z[0][2:4] == (64, 32)
        assert set_raw("MLMCPI_SWEEP_TILE", "64x32x256x9")[0] == 0
        # quirk, not a promise: "12abc" is taken as 12 (no host-only call shows the chunk, so only the status is pinned)
        assert set_raw("MLMCPI_RANDOM_SWEEP_CHUNK", "12abc")[0] == 0
        assert set_raw("MLMCPI_RANDOM_SWEEP_CHUNK", "254 ")[0] == 0
        ok, what = refused("MLMCPI_RANDOM_SWEEP_CHUNK", "255abc")   # (the number itself is still checked)
        assert ok, what
    finally:
        abi.set_option("MLMCPI_SWEEP_TILE", "")
        abi.set_option("MLMCPI_RANDOM_SWEEP_CHUNK", "")


# ---- the three knobs that show in mlmcpi_lattice_sweep_plan ----------------------------------------------------------
def _launches(act, B):
    """(kernel, threads, tile_w, tile_h, n_overrelax, n_heatbath) of every launch of a 10 + 1 draw under the options in force"""
    recs, count = (abi.SweepLaunch * 16)(), C.c_uint32(0)
    abi.call("mlmcpi_lattice_sweep_plan", C.byref(act), B, 10, 1, 0, recs, 16, C.byref(count))
    return [(r.kernel, r.threads, r.tile_w, r.tile_h, r.n_overrelax, r.n_heatbath) for r in recs[:count.value]]


def _probe():
    """Schwinger 128 x 128, 10 + 1 sweeps, at 1 chain (4 workgroups: the fused launch is wide by default) and at 100 chains (400
    workgroups: narrow by default), so that each value of MLMCPI_OR_HEAT differs from the default in one of the two."""
    act = abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0)
    return _launches(act, 1), _launches(act, 100)


K_SWEEP, K_OR_BLOCK, K_PERM, K_PERM_HEAT = 0, 2, 5, 6   # mlmcpi_sweep_kernel


# knob -> [(value, what the probe must show under it)], every value one that changes the plan
PLAN_KNOBS = {
    "MLMCPI_SWEEP_TILE": [("32x32x512", lambda one, many: {l[:4] for l in one} == {(K_SWEEP, 512, 32, 32)}),
                          ("64x32x1024", lambda one, many: {l[:4] for l in one} == {(K_SWEEP, 1024, 64, 32)})],
    "MLMCPI_OR_KERNEL": [("block", lambda one, many: one[0][0] == K_OR_BLOCK and one[-1][0] == K_SWEEP)],
    "MLMCPI_OR_HEAT": [("split", lambda one, many: [l[0] for l in one] == [K_PERM, K_SWEEP]),
                       ("narrow", lambda one, many: one == [(K_PERM_HEAT, 512, 64, 64, 10, 1)]),
                       ("wide", lambda one, many: many == [(K_PERM_HEAT, 1024, 64, 64, 10, 1)])],
}


def test_the_default_plan_of_the_probe():
    assert _probe() == ([(K_PERM_HEAT, 1024, 64, 64, 10, 1)], [(K_PERM_HEAT, 512, 64, 64, 10, 1)])


@pytest.mark.parametrize("name", sorted(PLAN_KNOBS))
def test_a_refused_value_and_the_empty_one_reset_the_knob(name):
    """The parent clears a knob's fields before it parses the value: a refused value leaves the knob at its DEFAULT, not at the
    value it had, and so does ""."""
    default = _probe()
    try:
        for value, shows in PLAN_KNOBS[name]:
            for reset in (KNOBS[name][1][0], "", None):
                abi.set_option(name, value)
                assert _probe() != default and shows(*_probe()), (name, value, _probe())
                rc, _ = set_raw(name, reset)
                assert rc == (0 if not reset else INVALID), (name, reset, rc)
                assert _probe() == default, (name, value, reset, _probe())
        # the accepted spellings that name the default leave the plan where it is
        for value in {"MLMCPI_OR_KERNEL": ["perm"], "MLMCPI_OR_HEAT": ["fused"]}.get(name, []):
            abi.set_option(name, value)
            assert _probe() == default, (name, value)
    finally:
        abi.set_option(name, "")


# ---- the environment ---------------------------------------------------------------------------------------------------
_CHILD = """
import ctypes as C
from mlmcpathintegral_amd import abi
act = abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0)
for B in (1, 100):
    recs, count = (abi.SweepLaunch * 16)(), C.c_uint32(0)
    abi.call("mlmcpi_lattice_sweep_plan", C.byref(act), B, 10, 1, 0, recs, 16, C.byref(count))
    print([(r.kernel, r.threads, r.tile_w, r.tile_h, r.n_overrelax, r.n_heatbath) for r in recs[:count.value]])
"""


def _child_probe(**knobs):
    """the probe in a fresh process that finds `knobs` in its environment (and none of the others)"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    one, many = (eval(line) for line in r.stdout.strip().splitlines())
    return one, many


@pytest.mark.parametrize("name", sorted(PLAN_KNOBS))
def test_a_knob_in_the_environment_is_loaded(name):
    value, shows = PLAN_KNOBS[name][-1]
    probe = _child_probe(**{name: value})
    assert shows(*probe), (name, value, probe)
    abi.set_option(name, value)
    try:
        assert probe == _probe()   # the same as setting it by call
    finally:
        abi.set_option(name, "")


def test_a_refused_value_in_the_environment_is_the_default_and_no_error():
    """(the environment is read without a caller to report to: a refused value there leaves the default in force)"""
    default = _probe()
    assert _child_probe() == default
    assert _child_probe(MLMCPI_OR_KERNEL="blocks", MLMCPI_SWEEP_TILE="63x32x256", MLMCPI_OR_HEAT="sideways") == default
