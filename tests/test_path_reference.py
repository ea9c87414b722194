"""CPU: tests/path_reference.py (the long-double restatement of the 1-D path formulas) against the oracle and the survey's
known answers, and the conditions tests/test_path_splits_gpu.py relies on, all decided here with no device:

  * every rotor input keeps |mod_2pi(d)| at least BRANCH_MARGIN from pi, so the susceptibility is compared on every chain;
  * the shapes reach the splits they are named for, and the spikes sit on the split boundaries;
  * over the six masked two-level draws the unmasked quartic and rotor chains see both outcomes, at every size -- the
    coarse path of 2 sites (M = 4) included, which the oracle accepts;
  * in the hierarchical composition both mask values reach every level;
  * the rotor draw + QoI case has zero and non-zero susceptibilities among the chains of path_finish_kernel's second block.

Bounds against the oracle (fp64, sequential sums of M positive terms; the long-double side is 2^-11 of that): 1e-12
relative for the sums (M eps = 9e-13 at M = 4100 is the worst case of a sequential sum), 1e-13 * scale for the force (a
handful of operations per site), 1e-10 for the susceptibility as everywhere in the suite.
"""
import numpy as np
import pytest

import path_cases as cases
import path_reference as ref
from path_reference import LD, PI


def oracle_action(orc, kind, M):
    return orc.Action(cases.KINDS[kind], **cases.params(kind, M))


def test_long_double_is_extended():
    assert np.finfo(LD).eps <= 2.0 ** -63
    assert abs(ref.winding(np.array([0.0, 2.0, 4.0, 2.0]))) < 1e-17              # -2 + 2 + 2 - 2: there and back
    x = np.array([0.0, 2.0, 4.0, 6.0])                                        # 2 + 2 + 2 + (-6 + 2 pi): one turn
    assert abs(ref.winding(x) - 2 * PI) < 1e-17
    assert abs(ref.susceptibility(x, 0.5) - 2) < 1e-17
    assert abs(ref.distance_to_branch_cut(np.array([0.0, np.pi - 1e-3])) - 1e-3) < 1e-12


@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_shapes_reach_their_splits(M, B):
    lens = [hi - lo for lo, hi in cases.split_bounds(M, B)]
    assert lens == {(1025, 3): [513, 512], (2050, 2): [684, 684, 682], (4100, 1500): [2050, 2050], (1100, 300): [550, 550],
                    (1100, 2100): [1100]}[(M, B)]
    sites = cases.spike_sites(M, B)
    assert sites[0] == 0 and sites[-1] == M - 1 and len(sites) == 2 * len(lens)
    x = cases.path_input("quartic", M, B)
    assert (np.abs(x[B - 1, sites]) >= 6.0).all() and (np.abs(x[: B - 1]) <= 3.0).all()
    assert len({x[b].tobytes() for b in range(min(B, 64))}) == min(B, 64), "every chain its own data"


@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_rotor_inputs_keep_away_from_the_branch_cut(M, B):
    x = cases.path_input("rotor", M, B)
    assert float(np.min(ref.distance_to_branch_cut(x))) >= cases.BRANCH_MARGIN
    Q = ref.winding(x) / (2 * PI)
    assert np.max(np.abs(Q - np.rint(Q))) < 1e-12, "Q / 2 pi is an integer"
    assert len(set(np.rint(Q).astype(int))) > 1 or B < 3, "the chains do not share one charge"


@pytest.mark.parametrize("kind", list(cases.KINDS))
@pytest.mark.parametrize("M,B", cases.SHAPES)
def test_formulas_equal_the_oracle_at_the_gpu_shapes(orc, kind, M, B):
    A = oracle_action(orc, kind, M)
    x = cases.path_input(kind, M, B)
    S, F = cases.reference("action", kind, M, B), cases.reference("force", kind, M, B)
    L = orc.lib()
    X2 = cases.reference("xsquared", kind, M, B) if kind == "harmonic" else None
    chi = cases.reference("susceptibility", kind, M, B) if kind == "rotor" else None
    T = cases.params(kind, M)["T_final"]
    chains = range(B) if B <= 300 else list(range(0, B, 37)) + [B - 1]   # every 37th chain and the spike chain B - 1 (the device test compares all)
    for b in chains:
        xb = np.ascontiguousarray(x[b])
        assert abs(S[b] - A.evaluate(xb)) <= 1e-12 * max(1.0, float(S[b])), (b, S[b])
        want = A.force(xb)
        assert np.max(np.abs(F[b] - want)) <= 1e-13 * max(1.0, float(np.max(np.abs(want)))), b
        if X2 is not None:
            assert abs(X2[b] - L.orc_qoi_xsquared(xb, M)) <= 1e-12 * max(1.0, float(X2[b]))
        if chi is not None:
            assert abs(chi[b] - L.orc_qoi_susceptibility(xb, M, T)) <= 1e-10 * max(1.0, float(chi[b]))


def test_known_answers(golden):
    x = np.sin(np.arange(16) + 1.0)
    for name, kind in (("rotor_M16", "rotor"), ("quartic_M16", "quartic")):
        g = golden[name]
        p = dict(g["params"])
        assert abs(ref.action(kind, p, x) - g["S"]) <= 1e-13 * g["S"]
        assert np.max(np.abs(ref.force(kind, p, x)[:4] - np.array(g["force_0_3"]))) <= 1e-13 * 5
    assert abs(ref.xsquared(x) - golden["quartic_M16"]["X2"]) <= 1e-14


def test_force_is_the_gradient_of_the_action():
    """central differences in long double, h = 1e-6: truncation ~ h^2 |S'''| / 6 <= 1e-10 here, rounding 2^-63 S / h ~ 1e-11"""
    rng = np.random.default_rng(3)
    x, h = rng.uniform(-1.5, 1.5, 10), LD(1e-6)
    for kind in cases.KINDS:
        p = cases.params(kind, 10)
        F = ref.force(kind, p, x)
        for j in (0, 4, 9):
            e = np.zeros(10, dtype=LD)
            e[j] = h
            g = (ref.action(kind, p, x + e) - ref.action(kind, p, x - e)) / (2 * h)
            assert abs(g - F[j]) < 1e-8, (kind, j, g, F[j])


def test_transfers():
    rng = np.random.default_rng(4)
    fine, coarse = rng.normal(size=(3, 10)), rng.normal(size=(3, 5))
    assert (ref.copy_from_fine(fine) == fine[:, ::2]).all()
    out = ref.copy_from_coarse(coarse, fine)
    assert (out[:, ::2] == coarse).all() and (out[:, 1::2] == fine[:, 1::2]).all()


def test_power_sums():
    rng = np.random.default_rng(5)
    q = rng.normal(0.3, 1.0, (25, 7))
    want = ref.power_sums(q)
    assert (want[:, 0] == 25).all()
    for k in (1, 2, 3, 4):
        assert np.max(np.abs(want[:, k] - np.sum(q ** k, axis=0))) < 1e-12 * np.max(np.abs(want[:, k]))


@pytest.mark.parametrize("kind,M,rough", cases.TWOLEVEL_CASES)
def test_masked_twolevel_draws_see_both_outcomes(orc, kind, M, rough):
    """the conditions of test_twolevel_masked_draws, on the oracle alone; M = 4 is in: dev_twolevel_draw takes a coarse
    path of 2 sites (its two neighbours are one site) and gives finite terms"""
    theta0, draws = cases.twolevel_run(kind, M, rough)
    before, seen = theta0, set()
    for xc, mask, accept, terms, theta in draws:
        off = mask == 0
        assert (theta[off] == before[off]).all() and (accept[off] == 0).all() and (terms[off] == 0).all()
        assert np.isfinite(terms).all() and np.isfinite(theta).all()
        for b in np.flatnonzero(mask):
            seen.add(int(accept[b]))
            assert (theta[b] == before[b]).all() == (accept[b] == 0) or kind == "harmonic"
        before = theta
    if kind != "harmonic":
        assert seen == {0, 1}
    # streams do not shift: chain 2 of draw 0 (mask 1, 0, 1, 0, 0) is the draw of stream chain0 + 2, step 0, on its own
    F, Cc = cases.twolevel_actions(orc, kind, M)
    xc, _, accept, terms, theta = draws[0]
    alone = theta0[2].copy()
    a, t = F.dev_twolevel_draw(Cc, xc[2], alone, cases.SEED, cases.TWOLEVEL_CHAIN0 + 2, 0)
    assert a == accept[2] and (t == terms[2]).all() and (alone == theta[2]).all()


def test_coarse_path_of_two_sites(orc):
    """the M = 4 decision: the oracle's actions on 2 sites are the formulas (d_0 = -d_1: each link counted twice)"""
    x = np.array([0.3, -1.1])
    for kind in cases.KINDS:
        A = oracle_action(orc, kind, 2)
        assert abs(ref.action(kind, cases.params(kind, 2), x) - A.evaluate(x)) < 1e-14 * max(1.0, abs(A.evaluate(x)))


def test_hierarchy_reaches_every_level_with_both_masks():
    draws = cases.hier_run()
    L = len(cases.HIER["levels"])
    for k in range(L - 1):
        masks = np.concatenate([rec[k][0] for rec in draws])
        assert set(masks.tolist()) == {0, 1}, f"mask into level {k}"
    assert set(np.concatenate([rec[0][1] for rec in draws]).tolist()) == {0, 1}
    # a two-level step that refuses a chain the level below accepted happens too (the mask is not the whole story)
    assert any(((rec[k][0] == 1) & (rec[k][1] == 0)).any() for rec in draws for k in range(L - 1))


def test_sweep_qoi_case_has_zero_and_nonzero_charges(orc):
    """cases.SWEEP_QOI: chains 256 .. 299 (path_finish_kernel's second block) hold both chi = 0 and chi > 0 after the draw"""
    c = cases.SWEEP_QOI
    A = orc.Action(orc.ROTOR, M=c["M"], T_final=c["T_final"], m0=c["m0"])
    chi = np.zeros(c["B"])
    for b in range(c["B"]):
        x = A.dev_initialise(cases.SEED, c["chain0"] + b)
        for s in range(c["n_or"] + c["n_hb"]):
            A.dev_sweep(x, s >= c["n_or"], cases.SEED, c["chain0"] + b, c["sweep0"] + s)
        chi[b] = orc.lib().orc_qoi_susceptibility(x, c["M"], c["T_final"])
    tail = chi[256:]
    assert (tail < 1e-20).any() and (tail > 0.1 / c["T_final"]).any(), tail
