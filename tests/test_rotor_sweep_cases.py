"""CPU: the cases of tests/test_rotor_sweeps_gpu.py reach what they are named for.  tests/rotor_sweep_cases.py mirrors the
launch arithmetic of path_sweep_impl (rotor_sweeps.hip); asserted here, with no device:

  * the concentrations: which sampler each selects, that `top` is 16 exactly and `over` the wrapped Cauchy's side of it, and
    that a = T_final / M is exact where 1 / a is a power of two;
  * the geometry of every shape: segments, rounding of the owned length, the full LDS image, the halo against the ring;
  * the launch plans: closed form against sweep by sweep, the heat-bath sweep behind the last overrelaxation launch;
  * the inputs: the cells of the first heat-bath sweep of every multi-segment case lie in all eight classes of the step
    envelope, and at `top` reach concentrations below 0.5 and above 15 (oracle sweeps up to there, no device).
"""
import numpy as np
import pytest

import rotor_sweep_cases as cases


def plan(shape, **kw):
    M, n_or, n_hb, qoi = shape
    return cases.launches(M, n_or, n_hb, with_qoi=qoi, **kw)


def shape_of(M, qoi=None):
    (s,) = [s for s in cases.EDGES if s[0] == M and (qoi is None or s[3] == qoi)]
    return s


# ---- concentrations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sorted({s[0] for s in cases.SHAPES} | {34}))
def test_concentrations_select_their_sampler(M):
    want = dict(flat=0.5, mid=4.0, top=16.0, peaked=64.0)
    for scale in cases.SCALES:
        p = cases.params(scale, M)
        v = cases.sig_scale(p)
        assert (v <= cases.VS_KAPPA_MAX) == (cases.SAMPLER[scale] == "step"), (scale, v)
        if scale in want:      # 1 / a a power of two: T_final and a carry no rounding
            assert p["T_final"] * cases.SCALES[scale][1] == M and p["T_final"] / M == 1.0 / cases.SCALES[scale][1]
            assert v == want[scale]
    over = cases.sig_scale(cases.params("over", M))
    assert 16.0 < over < 16.00001
    assert abs(cases.sig_scale(cases.params("sharp", M)) - 400.0) < 1e-10


def test_sharp_is_the_cluster_tests_rotor():
    """_rotor(M, 400.0) of tests/test_cluster_gpu.py: T_final = M * 2.0 * M0 / kappa2 with M0 = 0.25"""
    assert cases.params("sharp", 1982) == dict(M=1982, T_final=1982 * 2.0 * 0.25 / 400.0, m0=0.25)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def test_full_image_in_one_segment():
    for M, qoi, halo in ((1980, False, 34), (1976, True, 36)):
        (l,) = plan(shape_of(M))
        assert (l["n"], l["n_closed"], l["kinds"], l["halo"], l["qoi"]) == (17, 16, 1 << 16, halo, qoi)
        assert l["nseg2"] == 1 and l["L"] == [cases.LDS_IMAGE] and l["L"][0] // 2 == 4 * 256 and not l["rounded"]
    (l,) = plan(shape_of(2044))
    assert (l["n"], l["n_closed"], l["kinds"], l["halo"]) == (1, 0, 1, 2)
    assert l["L"] == [cases.LDS_IMAGE] and l["cells"] == [(1023, 1023)] and l["cells"][0][0] > 3 * cases.POOL_CAP


def test_first_lengths_with_two_segments():
    for M, olen in ((1982, [992, 990]), (1978, [990, 988]), (2046, [1024, 1022])):
        shape = shape_of(M)
        (l,) = plan(shape)
        assert l["nseg2"] == 2 and l["olen"] == olen and l["rounded"], (M, l)
        assert max(l["L"]) <= cases.LDS_IMAGE
        (before,) = plan((M - 2,) + shape[1:])
        assert before["nseg2"] == 1 and before["L"] == [cases.LDS_IMAGE], "M - 2 is the full image in one segment"
    # without the QoI's halo pair the QoI shapes are one segment: the extra pair is what splits them
    assert [l["nseg2"] for l in cases.launches(1978, 16, 1)] == [1]
    assert plan(shape_of(2046))[0]["cells"] == [(513, 513), (512, 512)]


def test_four_segments_with_a_short_last_one():
    (l,) = plan(shape_of(5930))
    assert l["qoi"] and l["halo"] == 36 and l["rounded"] and l["owned"] == 1484
    assert l["olen"] == [1484, 1484, 1484, 1478]


def test_four_launches_end_in_the_callers_buffer():
    p = plan(shape_of(4096))
    assert [(l["n"], l["n_closed"], l["kinds"]) for l in p] == [(16, 16, 0), (16, 16, 0), (2, 1, 2), (1, 0, 1)]
    assert [l["sampler"] for l in p] == [None, None, "step", "step"]
    assert cases.lands_in_callers_buffer(p)
    assert all(l["nseg2"] == 3 for l in p[:2]) and p[0]["olen"] == [1366, 1366, 1364]
    assert [l["sampler"] for l in plan(shape_of(4096), scale=400.0)] == [None, None, "cauchy", "cauchy"]


@pytest.mark.parametrize("shape", cases.SMALL, ids=cases.case_id)
def test_rings_shorter_than_the_halo(shape):
    M, n_or, n_hb, qoi = shape
    p = plan(shape)
    assert sum(l["n"] for l in p) == n_or + n_hb and p[-1]["qoi"] == qoi and not any(l["qoi"] for l in p[:-1])
    for l in p:
        assert l["nseg2"] == 1 and l["olen"] == [M] and l["L"] == [M + 2 * l["halo"]]
        assert l["halo"] >= M or (M, l["halo"]) in ((4, 2), (6, 2), (6, 4)), "the halo wraps the ring"
    if (n_or, n_hb) == (16, 1):
        assert [l["halo"] for l in p] == [36 if qoi else 34]
    if (n_or, n_hb) == (3, 2):
        assert [(l["n"], l["kinds"], l["halo"]) for l in p] == [(4, 8, 8), (1, 1, 4 if qoi else 2)]


def test_halo_not_a_multiple_of_the_ring_at_six_sites():
    halos = {l["halo"] for s in cases.SMALL if s[0] == 6 for l in plan(s)}
    assert halos == {34, 36, 8, 2, 4} and {h % 6 for h in halos} == {4, 0, 2}
    assert all(l["halo"] % 2 == 0 for s in cases.SMALL if s[0] == 2 for l in plan(s))


# ---- launch plans --------------------------------------------------------------------------------------------------------------
def test_sweep_by_sweep_takes_the_heat_bath_along_below_its_cap_only():
    """(n < cap || closed): 7 + 1 is one launch of 8 sweeps, 8 + 1 is two launches, 9 + 2 is 8, 1 + 1, 1"""
    def nk(n_or, n_hb, **kw):
        return [(l["n"], l["n_closed"], l["kinds"]) for l in cases.launches(1982, n_or, n_hb, **kw)]
    assert nk(7, 1, block_mode=True) == [(8, 0, 1 << 7)]
    assert nk(8, 1, block_mode=True) == [(8, 0, 0), (1, 0, 1)]
    assert nk(9, 2, block_mode=True) == [(8, 0, 0), (2, 0, 2), (1, 0, 1)]
    assert nk(7, 1, block_mode=True, split_heat=True) == [(7, 0, 0), (1, 0, 1)]
    assert nk(9, 2, block_mode=True, split_heat=True) == [(8, 0, 0), (1, 0, 0), (1, 0, 1), (1, 0, 1)]
    assert nk(8, 1) == [(9, 8, 1 << 8)] and nk(16, 1) == [(17, 16, 1 << 16)] and nk(17, 1) == [(16, 16, 0), (2, 1, 2)]
    assert nk(16, 1, split_heat=True) == [(16, 16, 0), (1, 0, 1)]
    # (eight sweeps need a halo of 16 only: M = 1982 is one segment here, the ring of 6 sites is wrapped five times)
    assert [(l["nseg2"], l["L"]) for l in cases.launches(1982, 7, 1, block_mode=True)] == [(1, [2014])]
    assert [l["L"] for l in cases.launches(6, 7, 1, block_mode=True)] == [[38]]
    assert {(M, s) for M, _, _, s in cases.BLOCK} == {(M, s) for M in (1982, 6) for s in ("mid", "over")}


def test_fused_and_split_draws_differ_in_their_launches():
    for M, scale in cases.FUSED_SPLIT:
        v = cases.sig_scale(cases.params(scale, M))
        for n_or, n_hb in cases.FUSED_SPLIT_DRAWS:
            fused, split = cases.launches(M, n_or, n_hb, scale=v), cases.launches(M, n_or, n_hb, split_heat=True, scale=v)
            assert len(split) == len(fused) + 1
            assert any(l["n_closed"] and l["kinds"] for l in fused) and not any(l["n_closed"] and l["kinds"] for l in split)
            assert {l["sampler"] for l in fused if l["kinds"]} == {cases.SAMPLER[scale]}
    # of the draws only (16, 1) is deep enough for the edges the two lengths are named for
    assert (16, 1) in cases.FUSED_SPLIT_DRAWS
    assert [l["nseg2"] for l in cases.launches(1982, 10, 1)] == [1] and [l["nseg2"] for l in cases.launches(1982, 16, 1)] == [2]
    assert [l["L"] for l in cases.launches(1980, 16, 1)] == [[cases.LDS_IMAGE]]
    assert [l["L"] for l in cases.launches(1980, 16, 1, split_heat=True)] == [[2044], [1984]]


def test_every_parity_case_runs_the_sampler_of_its_name():
    seen = set()
    for shape, scale in cases.PARITY:
        M = shape[0]
        v = cases.sig_scale(cases.params(scale, M))
        p = plan(shape, scale=v)
        assert {l["sampler"] for l in p if l["kinds"]} == {cases.SAMPLER[scale]}
        assert all(max(l["L"]) <= cases.LDS_IMAGE and all(o % 2 == 0 for o in l["olen"]) for l in p)
        seen.add((shape, scale))
    assert len(seen) == len(cases.PARITY) == 4 * len(cases.SHAPES) + 2 * len(cases.TWO_SEGMENT)
    assert all(plan(s)[-1]["nseg2"] == 2 for s in cases.TWO_SEGMENT) and all(plan(s)[-1]["nseg2"] >= 2 for s in cases.MULTI_SEGMENT)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def test_starts_are_per_chain_and_in_range():
    for shape, scale in cases.PARITY[:8] + cases.PARITY[-6:]:
        x = cases.start(*shape[:3], scale)
        assert x.shape == (cases.B, shape[0]) and (x >= -np.pi).all() and (x < np.pi).all()
        assert len({x[b].tobytes() for b in range(cases.B)}) == cases.B
    assert cases.CHAIN0 != 0 and cases.SWEEP0 != 0 and cases.B == 3


@pytest.mark.parametrize("shape", cases.MULTI_SEGMENT, ids=cases.case_id)
@pytest.mark.parametrize("scale", ["flat", "mid", "top"])
def test_first_heat_bath_sweep_meets_every_class_of_the_step_envelope(orc, shape, scale):
    M, n_or, n_hb, _ = shape
    _, pre, post, _ = cases.oracle_run(M, n_or, n_hb, scale)
    xp, xm = cases.first_heat_cells(pre, post)
    cls = cases.step_class(xp, xm)
    v = cases.sig_scale(cases.params(scale, M))
    k = cases.kappa(v, xp, xm)
    for b in range(cases.B):
        assert set(cls[b].tolist()) == set(range(cases.VS_CLASSES)), (b, np.bincount(cls[b]))
        if scale == "top":
            assert k[b].min() < 0.5 and k[b].max() > 15.0, (b, k[b].min(), k[b].max())
    # the classes are ranges of the concentration: class c holds kappa in scale * [sin(2 pi c / 32), sin(2 pi (c + 1) / 32)]
    lo, hi = v * np.sin(2 * np.pi * cls / 32.0), v * np.sin(2 * np.pi * (cls + 1) / 32.0)
    assert (k >= lo - 1e-9).all() and (k <= hi + 1e-9).all()


def test_first_heat_cells_are_the_neighbours_the_sweep_reads(orc):
    """the helper against the oracle itself: one heat-bath sweep by single-site updates in colour order, reading the
    neighbours the helper names"""
    M, scale = 6, "mid"
    _, pre, post, _ = cases.oracle_run(M, 0, 1, scale)
    xp, xm = cases.first_heat_cells(pre, post)
    x = pre[0].copy()
    for l in list(range(0, M, 2)) + list(range(1, M, 2)):
        assert x[(l + 1) % M] == xp[0, l] and x[(l - 1) % M] == xm[0, l]
        x[l] = post[0, l]


def test_site_lists():
    for M, _ in cases.SITE:
        s = cases.site_list(M).tolist()
        assert set(s) == set(range(M)) and len(s) > M and all(0 <= l < M for l in s)
        pairs = list(zip(s, s[1:]))
        assert (0, M - 1) in pairs and (M - 1, 0) in pairs and any(a == b for a, b in pairs)
    assert cases.SITE_B == 64 + 6
