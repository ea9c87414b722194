"""CPU: the plan queries of the two smoothers of the O(3) sigma model, mlmcpi_sigma_level_cooling_plan and
mlmcpi_sigma_level_flow_plan (sigma_smooth.hip drives both), which touch no device: the launch arithmetic of the GPU modules'
test_plan_query restated against both, every refusal a plan query shares with its call, and the one bound on the workgroups of a
launch -- vertex groups, smoothing tiles and charge tiles -- that both smoothers answer alike."""
import ctypes as C

import numpy as np
import pytest

from mlmcpathintegral_amd import abi

ERR_INVALID = -1
LDS_MAX = 160 * 1024 - 512
EPS = 0.05


class Smoother:
    def __init__(self, name, knob, query, plan_type, launches, default, lst, items, flow):
        self.name, self.knob, self.query, self.plan_type, self.launches = name, knob, query, plan_type, launches
        self.default, self.lst, self.items, self.flow = default, lst, items, flow

    def lds(self, tw, th, K, rot):
        """the LDS image of a launch of K fused units"""
        if self.flow:
            return (tw + 6 * K) * (th + 6 * K) * (144 if rot else 72)
        halo = K if rot else 2 * K
        return (tw + 2 * halo) * (th + 2 * halo) * (48 if rot else 24)

    def raw(self, level, n_chains, counts, plan="new", eps=EPS):
        """(status, message, plan) of the plan query, not turned into an exception; counts None: a NULL list of length 2"""
        lib = abi.load()
        out = self.plan_type() if plan == "new" else plan
        lst = None if counts is None else (C.c_uint32 * max(len(counts), 1))(*counts)
        n = 2 if counts is None else len(counts)
        args = (None if level is None else C.byref(level), n_chains) + ((eps,) if self.flow else ()) + (lst, n)
        rc = getattr(lib, self.query)(*args, None if out is None else C.byref(out))
        return rc, lib.mlmcpi_last_error().decode(), out


COOLING = Smoother("cooling", "MLMCPI_SIGMA_COOL_PLAN", "mlmcpi_sigma_level_cooling_plan", abi.SigmaCoolingPlan, "launch_sweeps",
                   (32, 32, 512, 2), "depths", "depths", False)
FLOW = Smoother("flow", "MLMCPI_SIGMA_FLOW_PLAN", "mlmcpi_sigma_level_flow_plan", abi.SigmaFlowPlan, "launch_steps",
                (16, 16, 512, 1), "steps", "step counts", True)
SMOOTHERS = [COOLING, FLOW]
# the plans and lists of test_sigma_cooling_gpu.py::test_plan_query and test_sigma_flow_gpu.py::test_plan_query
PLANS = {"cooling": ["", "1x1x256x1", "8x4x256x4", "16x16x512x16", "7x5x512x3"],
         "flow": ["", "1x1x256x1", "8x4x256x2", "7x5x512x3", "2x2x1024x5", "16x16x512x2"]}
LISTS = {"cooling": ([0], [1], [10], [0, 1, 2, 3, 7, 10], [7, 10], [5, 4096]),
         "flow": ([0], [1], [10], [0, 1, 2, 3, 7, 10], [3, 7], [5, 4096])}


def _level(Mt, Mx, rot, beta=1.0):
    return abi.sigma_level(Mt, Mx, rot, beta)


@pytest.fixture
def set_plan():
    def go(s, value):
        abi.set_option(s.knob, value)
    yield go
    for s in SMOOTHERS:
        abi.set_option(s.knob, "")


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("s", SMOOTHERS, ids=lambda s: s.name)
def test_plan_query(set_plan, s, rot):
    """the launches' units sum to the last entry of the list, no launch crosses a listed entry, and lds_bytes is the image of the
    deepest launch"""
    lv = _level(66, 34, rot)
    PW, PH = (33, 17) if rot else (66, 34)
    for plan in PLANS[s.name]:
        set_plan(s, plan)
        tw, th, nt, K = (int(v) for v in plan.split("x")) if plan else s.default
        for counts in LISTS[s.name]:
            rc, msg, p = s.raw(lv, 300, counts)
            assert rc == 0, (plan, counts, msg)
            want, done = [], 0
            for d in counts:
                while done < d:
                    want.append(min(K, d - done))
                    done += want[-1]
            got = list(getattr(p, s.launches)[:p.n_launches])
            assert got == want and sum(got) == counts[-1] and p.n_measurements == len(counts)
            edges = set(np.cumsum(got).tolist())
            assert all(d in edges for d in counts if d > 0)
            etw, eth = min(tw, PW), min(th, PH)
            assert (p.tw, p.th, p.nt, p.fuse) == (etw, eth, nt, K)
            assert p.tiles == -(-PW // etw) * -(-PH // eth)
            deepest = max(got, default=0)
            assert p.lds_bytes == (s.lds(etw, eth, deepest, rot) if deepest else 0)
            assert p.lds_bytes <= LDS_MAX


@pytest.mark.parametrize("s", SMOOTHERS, ids=lambda s: s.name)
def test_refusals_shared_with_the_call(s):
    """every refusal of the call that does not need a device pointer; a refused query leaves the plan as it was"""
    good, counts = _level(6, 4, 0), [0, 2]
    bad = [("level is NULL", None, 3, counts), ("%s is NULL" % s.lst, good, 3, None),
           ("even extents", _level(3, 4, 0), 3, counts), ("even extents", _level(4, 5, 1), 3, counts),
           ("even extents", _level(0, 4, 0), 3, counts), ("even extents", _level(4, 0, 1), 3, counts),
           ("too large", _level(1 << 16, 1 << 15, 0), 3, counts), ("n_chains > 0", good, 0, counts),
           ("strictly ascending", good, 3, [2, 2]), ("strictly ascending", good, 3, [3, 1]), ("at most 4096", good, 3, [0, 4097]),
           ("1 .. 32 %s" % s.items, good, 3, []), ("1 .. 32 %s" % s.items, good, 3, list(range(33))),
           # 2^22 groups of 256 vertices x 2^20 chains > 2^23 x 65535 workgroups
           ("workgroups per launch", _level(1 << 15, 1 << 15, 0), 1 << 20, counts)]
    for msg, lv, n, lst in bad:
        mark = s.plan_type(tw=77, n_launches=5)
        rc, err, p = s.raw(lv, n, lst, plan=mark)
        assert rc == ERR_INVALID and msg in err, (msg, rc, err)
        assert (p.tw, p.n_launches) == (77, 5), msg
    rc, err, _ = s.raw(good, 3, counts, plan=None)
    assert rc == ERR_INVALID and "plan is NULL" in err, err
    if s.flow:
        for eps in (0.0, -0.05, 0.2500001, 0.3, float("nan"), float("inf")):
            rc, err, _ = s.raw(good, 3, counts, eps=eps)
            assert rc == ERR_INVALID and "0 < eps <= 0.25" in err, (eps, err)
        assert s.raw(good, 3, counts, eps=0.25)[0] == 0
    assert s.raw(good, 3, counts)[0] == 0


@pytest.mark.parametrize("s", SMOOTHERS, ids=lambda s: s.name)
def test_the_charge_launch_counts_in_the_workgroup_bound(set_plan, s):
    """A rotated level (2^29, 2) is a plane of 2^28 x 1 cells: 2^21 groups of 256 vertices, under the plan 128x1x256x1 2^21
    smoothing tiles, but 2^23 charge tiles of 32 x 32.  With 2^17 chains the charge launch alone passes the 2^23 x 65535
    workgroups of a grid, and both smoothers refuse; with 2^15 chains every launch fits."""
    set_plan(s, "128x1x256x1")
    lv = _level(1 << 29, 2, 1)
    rc, err, p = s.raw(lv, 1 << 15, [1])
    assert rc == 0 and p.tiles == 1 << 21, err
    rc, err, _ = s.raw(lv, 1 << 17, [1])
    assert rc == ERR_INVALID and "workgroups per launch" in err, (rc, err)
    assert str((1 << 17) * (1 << 23)) in err   # the need it reports is that of the charge launch
