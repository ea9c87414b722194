"""Gaussian free field multilevel glue: GFFAction on the levels of a coarsening hierarchy (rotated levels,
Gibbs-smoothed coarse actions), GFFConditionedFineAction and the two-level step between GFF levels.
CPU: vertex lists against the compiled reference (its recorded output), the library's dense matrices against the oracle's
independent construction and against the defining properties (n_gibbs = 0 gives the plain precision matrix, many sweeps
give the exact marginal of the finer level).  GPU: evaluate / draw / fill-in / two-level step against the oracle, and the
hierarchical chain against the closed form of <phi^2>."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTATE, BOTH = 4, 0


class Level:
    """library-side level handle (host functions work without a GPU)"""

    def __init__(self, Mt, ctype, level, mass, n_gibbs=0, omega=1.0):
        from mlmcpathintegral_amd import abi
        self.abi = abi
        self.h = C.c_void_p()
        abi.call("mlmcpi_gff_level_create", Mt, Mt, ctype, level, float(mass), n_gibbs, float(omega), C.byref(self.h))
        n, nc, mtc, mxc, mu2 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
        abi.call("mlmcpi_gff_level_info", self.h, C.byref(n), C.byref(nc), C.byref(mtc), C.byref(mxc), C.byref(mu2))
        self.N, self.n_coarse, self.Mt_c, self.mu2 = n.value, nc.value, mtc.value, mu2.value
        self.Mt, self.n_gibbs, self.rotated = Mt, n_gibbs, ctype == ROTATE and level % 2 == 1

    def nb(self):
        return _neighbours(self.Mt, self.rotated)

    def tables(self):
        pairs = np.zeros(2 * self.n_coarse, dtype=np.uint32)
        fineonly = np.zeros(self.N - self.n_coarse, dtype=np.uint32)
        self.abi.call("mlmcpi_gff_level_tables", self.h, pairs.ctypes.data_as(C.c_void_p), fineonly.ctypes.data_as(C.c_void_p))
        return pairs, fineonly

    def matrix(self, which):
        out = np.zeros((self.N, self.N))
        self.abi.call("mlmcpi_gff_level_matrix", self.h, which, out.ctypes.data_as(C.c_void_p))
        return out

    def __del__(self):
        try:
            self.abi.call("mlmcpi_gff_level_destroy", self.h)
        except Exception:
            pass


class OLevel:
    def __init__(self, orc, Mt, ctype, level, mass, n_gibbs=0, omega=1.0):
        self.L = orc.lib()
        self.h = self.L.orc_gff_level_new(Mt, Mt, ctype, level, float(mass), n_gibbs, float(omega))
        self.N, self.n_coarse = self.L.orc_gff_level_size(self.h), self.L.orc_gff_level_n_coarse(self.h)

    def tables(self):
        pairs = np.zeros(2 * self.n_coarse, dtype=np.uint32)
        fineonly = np.zeros(self.N - self.n_coarse, dtype=np.uint32)
        self.L.orc_gff_level_tables(self.h, pairs.ctypes.data_as(C.c_void_p), fineonly.ctypes.data_as(C.c_void_p))
        return pairs, fineonly

    def matrix(self, which):
        out = np.zeros((self.N, self.N))
        self.L.orc_gff_level_matrix(self.h, which, out)
        return out

    def __del__(self):
        self.L.orc_gff_level_free(self.h)


@pytest.mark.parametrize("Mt,ctype,level", [(8, ROTATE, 0), (8, ROTATE, 1), (16, ROTATE, 0), (16, ROTATE, 1), (8, BOTH, 0), (4, ROTATE, 0),
                                            (32, ROTATE, 1)])
def test_vertex_lists_match_compiled_reference(compiled_ref, orc, Mt, ctype, level):
    """coarse / fine-only vertices and the fine -> coarse map of Lattice2D (lattice2d.cc:82-134), rotated levels included:
    library == oracle == the reference's own class (its recorded output), bit for bit"""
    rec = compiled_ref["vertex_lists"][f"{Mt} {ctype} {level}"]
    want_f, want_p = np.array(rec["fineonly"], dtype=np.uint32), np.array(rec["fine2coarse"], dtype=np.uint32)
    nf, nc = want_f.size, want_p.size // 2
    for lv in (Level(Mt, ctype, level, 1.0), OLevel(orc, Mt, ctype, level, 1.0)):
        assert lv.n_coarse == nc and lv.N - lv.n_coarse == nf
        pairs, fineonly = lv.tables()
        assert np.array_equal(pairs, want_p) and np.array_equal(fineonly, want_f)


@pytest.mark.parametrize("Mt,level,n_gibbs,omega", [(4, 0, 2, 1.0), (4, 1, 2, 1.0), (8, 1, 2, 1.0), (8, 1, 1, 1.3), (8, 0, 3, 0.8), (8, 1, 0, 1.0),
                                                    (24, 1, 2, 1.0), (17, 0, 1, 1.0)])
def test_dense_matrices_match_oracle(orc, Mt, level, n_gibbs, omega):
    """Qhat of gffaction.cc:126-173 and the factor of the exact sampler: the library (Cholesky-based inverses) against the
    oracle (Gauss-Jordan), independent constructions of the same dense algebra.  (24, level 1) is the 288-vertex level the
    GPU cases beyond one workgroup pass rest on; 17 x 17 has odd extents, which only CoarsenBoth level 0 may have.)"""
    ctype = BOTH if Mt % 2 else ROTATE
    a, b = Level(Mt, ctype, level, 10.0, n_gibbs, omega), OLevel(orc, Mt, ctype, level, 10.0, n_gibbs, omega)
    for which in (0, 1):
        A, Bm = a.matrix(which), b.matrix(which)
        assert np.max(np.abs(A - Bm)) < 1e-11 * np.max(np.abs(Bm)), which
    Q = a.matrix(0)
    assert np.allclose(Q, Q.T, rtol=0, atol=1e-12 * np.abs(Q).max()) and np.all(np.linalg.eigvalsh(Q) > 0)
    Linv = a.matrix(1)
    # L^-T L^-1 = Q^-1 with Q the plain stencil of the level
    nb = _neighbours(Mt, level % 2 == 1)
    Qp = _stencil_matrix(nb, [4.0 + a.mu2, -1.0])
    assert np.allclose(Linv.T @ Linv @ Qp, np.eye(a.N), atol=1e-10)


def _neighbours(Mt, rotated):
    from mlmcpathintegral_amd import abi
    n = Mt * Mt // 2 if rotated else Mt * Mt
    out = np.zeros(8 * n, dtype=np.uint32)
    abi.call("mlmcpi_neighbours_2d", Mt, Mt, int(rotated), out.ctypes.data_as(C.c_void_p))
    return out.reshape(n, 8)


def _stencil_matrix(nb, stencil):
    n = nb.shape[0]
    Q = np.zeros((n, n))
    for l in range(n):
        Q[l, l] += stencil[0]
        for s in range(len(stencil) - 1):
            for k in range(4):
                Q[l, nb[l, 4 * s + k]] += stencil[s + 1]
    return Q


def test_smoothed_coarse_action_interpolates_between_plain_and_exact_marginal():
    """What the coarse GFF action IS: with no smoothing it is the plain stencil of the coarse lattice; with many Gibbs
    sweeps it becomes the exact marginal of the fine action on the coarse vertices (the Schur complement, which is what the
    fill-in of GFFConditionedFineAction assumes) -- checked against the marginal computed from the FINE level's precision
    matrix, so the factor sqrt(2) in the lattice spacing of the rotated level, the 9-point stencil and the vertex maps all
    have to be right."""
    Mt, mass = 8, 10.0
    fine = Level(Mt, ROTATE, 0, mass)
    pairs, _ = fine.tables()
    Qf = _stencil_matrix(_neighbours(Mt, False), [4.0 + fine.mu2, -1.0])
    cov = np.linalg.inv(Qf)
    fidx, cidx = pairs[0::2], pairs[1::2]
    marg = np.zeros((fine.n_coarse, fine.n_coarse))
    marg[np.ix_(cidx, cidx)] = cov[np.ix_(fidx, fidx)]      # covariance of the coarse vertices, in coarse numbering
    Q_marginal = np.linalg.inv(marg)
    plain = Level(Mt, ROTATE, 1, mass, 0).matrix(0)
    assert np.allclose(plain, _stencil_matrix(_neighbours(Mt, True), [4.0 + 2.0 * fine.mu2, -1.0]), atol=1e-12)
    err = [np.max(np.abs(Level(Mt, ROTATE, 1, mass, n).matrix(0) - Q_marginal)) for n in (0, 2, 8, 60)]
    assert err[0] > err[1] > err[2] > err[3] and err[3] < 1e-9 * np.abs(Q_marginal).max(), err


# ---- the reference author's own numpy construction (tests/golden/gff_qhat.json, made by make_gff_qhat_fixture.py) --------
def _qhat_fixture():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "gff_qhat.json")) as f:
        return json.load(f)


def _fixture_fields(Mlat):
    """the three deterministic fields of make_gff_qhat_fixture.py (Cartesian coordinates: permutation-free)"""
    i, j = np.meshgrid(np.arange(Mlat), np.arange(Mlat), indexing="ij")
    return [np.sin(0.7 * i + 1.3 * j + 0.2), np.cos(2.0 * np.pi * i / Mlat) * (1.0 + 0.1 * j), ((3 * i + 5 * j) % 7) / 7.0 - 0.4]


def _rotated_coords(Mt, n):
    from mlmcpathintegral_amd import abi
    out = []
    for ell in range(n):
        i, j = C.c_int(), C.c_int()
        abi.load().mlmcpi_vertex_lin2cart(Mt, Mt, 1, ell, C.byref(i), C.byref(j))
        out.append((i.value, j.value))
    return out


@pytest.mark.parametrize("case", [c for c in _qhat_fixture()["qhat"] if c["order"] == "lattice2d" or c["nsmooth"] == 0],
                         ids=lambda c: f"M{c['Mlat']}-n{c['nsmooth']}-{c['order']}")
def test_qhat_matches_the_reference_authors_numpy_construction(orc, case):
    """Q-hat of the first rotated level, Sigma_iter = Sigma + G^n (Sigma_initial - Sigma) G^n^T inverted
    (gffaction.cc:133-166), against /root/reference/python/gibbs_smoother.py:41-55 run by the fixture generator -- the
    reference author's own construction of the same object, with the same stencils (coarse mu2 = 2 x fine).  Library
    (mlmcpi_gff_level_matrix) and oracle both reproduce 1/2 phi^T Q-hat phi for three fields and the diagonal and one row
    of Sigma_iter = Q-hat^-1.  For nsmooth > 0 the matrix depends on the order of the Gibbs sweep: the cases compared are
    the ones the generator built in Lattice2D's numbering of the rotated vertices (order = lattice2d)."""
    Mlat, n = case["Mlat"], case["nsmooth"]
    for lv in (Level(Mlat, ROTATE, 1, case["mass"], n), OLevel(orc, Mlat, ROTATE, 1, case["mass"], n)):
        Q = lv.matrix(0)
        coords = _rotated_coords(Mlat, lv.N)
        for f, want in zip(_fixture_fields(Mlat), case["energies"]):
            phi = np.array([f[i, j] for i, j in coords])
            assert abs(0.5 * phi @ Q @ phi - want) < 1e-10 * max(1.0, abs(want))
        Sigma = np.linalg.inv(Q)
        lin = {c: l for l, c in enumerate(coords)}
        for i, j, v in case["sigma_iter_diag"]:
            assert abs(Sigma[lin[(i, j)], lin[(i, j)]] - v) < 1e-10 * abs(v)
        for i, j, v in case["sigma_iter_row0"]:
            assert abs(Sigma[lin[(0, 0)], lin[(i, j)]] - v) < 1e-11


def test_gibbs_sweep_order_matters_for_qhat():
    """why only the lattice2d-ordered cases can be compared for nsmooth > 0: the same construction swept in the Python
    class's own vertex order gives a different Q-hat (energies differ in the 3rd-4th digit), and the same one for nsmooth = 0"""
    cases = {(c["Mlat"], c["nsmooth"], c["order"]): c for c in _qhat_fixture()["qhat"]}
    for Mlat in (8, 16):
        a, b = cases[(Mlat, 0, "python")], cases[(Mlat, 0, "lattice2d")]
        assert np.allclose(a["energies"], b["energies"], rtol=1e-12)
        a, b = cases[(Mlat, 2, "python")], cases[(Mlat, 2, "lattice2d")]
        assert not np.allclose(a["energies"], b["energies"], rtol=1e-6)


@pytest.mark.parametrize("case", _qhat_fixture()["twolevel_terms"], ids=lambda c: f"M{c['Mlat']}-m{c['mass']}-n{c['nsmooth']}")
def test_two_level_terms_match_the_reference_authors_python(orc, case):
    """The three actions of TwoLevelMetropolisStep::draw for the GFF (twolevelmetropolisstep.cc:35-89 with GFFAction::evaluate,
    gffaction.cc:8-30, the smoothed coarse action, :133-166, and GFFConditionedFineAction::evaluate,
    gffconditionedfineaction.cc:7-49), against /root/reference/python/gff_twolevel.py (GFFAction.evaluate, evaluate_fillin,
    CoarseGibbsSmoother.evaluate, TwoLevelSampler.step), run by the fixture generator on two deterministic fields: the
    oracle reproduces S_fine, S_fillin, S_coarse of each field and Delta S of the pair to 1e-10 -- the vertex maps, the
    restriction to the rotated level, the fill-in's neighbour sums and variance included."""
    L = orc.lib()
    Mlat, mass, n = case["Mlat"], case["mass"], case["nsmooth"]
    F, Cl = OLevel(orc, Mlat, ROTATE, 0, mass, 0), OLevel(orc, Mlat, ROTATE, 1, mass, n)
    f = _fixture_fields(Mlat)
    got = {}
    for name, field in (("current", f[0]), ("proposal", f[2])):
        phi = np.array([field[l % Mlat, l // Mlat] for l in range(Mlat * Mlat)])   # vertex l = Mt j + i
        coarse = np.zeros(Cl.N)
        L.orc_gff_copy(F.h, phi, coarse, 1)
        got[name] = {"S_fine": L.orc_gff_level_evaluate(F.h, phi), "S_fillin": L.orc_gff_cfa_evaluate(F.h, phi),
                     "S_coarse": L.orc_gff_level_evaluate(Cl.h, coarse)}
        for k, v in case["terms"][name].items():
            assert abs(got[name][k] - v) < 1e-10 * max(1.0, abs(v)), (name, k, got[name][k], v)
    dS = (got["proposal"]["S_fine"] - got["current"]["S_fine"]) + (got["current"]["S_coarse"] - got["proposal"]["S_coarse"]) \
        + (got["current"]["S_fillin"] - got["proposal"]["S_fillin"])
    assert abs(dS - case["DeltaS"]) < 1e-9


def test_phi_squared_closed_form_matches_the_reference_authors_python(orc):
    """gff_phi_squared_analytical (auxilliary.cc:197-209) against QoISquaredField.exact_value of gff_twolevel.py:186-193"""
    for c in _qhat_fixture()["phi_squared_exact"]:
        got = orc.lib().orc_gff_phi_squared_analytical(c["mass"], c["Mlat"], c["Mlat"])
        assert abs(got - c["phi_squared"]) < 1e-12 * c["phi_squared"], (c, got)


def test_three_level_acceptance_is_the_plain_vs_marginal_mismatch():
    """with three GFF levels (16 x 16 -> rotated -> 8 x 8) the lower two-level step accepts about 8 %.  The
    reading: the fill-in of the rotated level (gffconditionedfineaction.cc:7-25) is exact for the PLAIN stencil there, so
    a proposal on that level is distributed (nearly) like the plain stencil's Gaussian, while the level's action is the
    Gibbs-smoothed Q-hat, close to the 9-point marginal of the finer level: an independence Metropolis test between the two.
    (a) numpy, with the library's own matrices: the expected acceptance of exactly that step is 0.05 ... 0.12;
    (b) the reference author's Python experiment of the same test (GFFAction.draw_5pt / draw_9pt / evaluate_*,
        gff_twolevel_coarse.py:8-152, run by the fixture generator at the same mu2 on square lattices of 64 and 144
        vertices) brackets it: 0.20 at 64, 0.055 at 144 vertices; the rotated level has 128."""
    rng = np.random.default_rng(7)
    Mt, mass, n_gibbs = 16, 10.0, 2
    # (a level handle takes the extents of ITS lattice: level 2 of the 16 x 16 hierarchy is the unrotated 8 x 8 lattice)
    l1, l2 = Level(Mt, ROTATE, 1, mass, n_gibbs), Level(Mt // 2, ROTATE, 2, mass, n_gibbs)
    assert l2.N == l1.n_coarse and abs(l2.mu2 - 2.0 * l1.mu2) < 1e-14
    Q1, Q2 = l1.matrix(0), l2.matrix(0)
    pairs, fineonly = l1.tables()
    fidx, cidx = pairs[0::2], pairs[1::2]
    nb = _neighbours(Mt, True)
    kappa = 4.0 + l1.mu2
    C1, C2 = np.linalg.cholesky(np.linalg.inv(Q1)), np.linalg.cholesky(np.linalg.inv(Q2))

    def cfa(theta):  # -log density of the fine-only vertices given the coarse ones (up to a constant)
        mean = theta[nb[fineonly, :4]].sum(axis=1) / kappa
        return 0.5 * kappa * np.sum((theta[fineonly] - mean) ** 2)

    acc = []
    for _ in range(4000):
        theta = C1 @ rng.standard_normal(l1.N)                      # current state ~ the level's action
        x_new = C2 @ rng.standard_normal(l2.N)                      # coarse proposal ~ the coarser level's action
        prop = np.zeros(l1.N)
        prop[fidx] = x_new[cidx]
        prop[fineonly] = prop[nb[fineonly, :4]].sum(axis=1) / kappa + rng.standard_normal(len(fineonly)) / math.sqrt(kappa)
        x_old = np.zeros(l2.N)
        x_old[cidx] = theta[fidx]
        dS = (0.5 * prop @ Q1 @ prop - 0.5 * theta @ Q1 @ theta) - (0.5 * x_new @ Q2 @ x_new - 0.5 * x_old @ Q2 @ x_old) \
            - (cfa(prop) - cfa(theta))
        acc.append(min(1.0, math.exp(-dS)))
    p = float(np.mean(acc))
    ref = {a["ndof"]: a["mean_acceptance_probability"] for a in _qhat_fixture()["independence_acceptance_5pt_vs_9pt"]}
    assert ref[144] < p < ref[64], (p, ref)
    assert 0.05 < p < 0.12, p


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _dev(abi, name, *args):
    abi.call(name, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,level,n_gibbs", [(8, 0, 0), (8, 1, 2), (16, 1, 2), (16, 0, 0), (8, 1, 0)])
def test_level_evaluate_and_draw_match_oracle(gpu_ops, orc, Mt, level, n_gibbs):
    import torch
    from mlmcpathintegral_amd import abi
    a, b = Level(Mt, ROTATE, level, 10.0, n_gibbs), OLevel(orc, Mt, ROTATE, level, 10.0, n_gibbs)
    B, seed = 5, 31
    phi = torch.zeros((B, a.N), dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_level_draw", a.h, C.c_void_p(phi.data_ptr()), B, seed, 3, 7, None)
    S = torch.zeros(B, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_level_evaluate", a.h, C.c_void_p(phi.data_ptr()), B, C.c_void_p(S.data_ptr()), None)
    got, gotS = phi.cpu().numpy(), S.cpu().numpy()
    for c in range(B):
        want = np.zeros(a.N)
        b.L.orc_gff_level_dev_draw(b.h, want, seed, 3 + c, 7)
        assert np.max(np.abs(got[c] - want)) < 1e-11 * max(1.0, np.abs(want).max())
        assert abs(gotS[c] - b.L.orc_gff_level_evaluate(b.h, want)) < 1e-10 * max(1.0, abs(gotS[c]))


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,level", [(8, 0), (8, 1), (16, 0), (16, 1)])
def test_gff_twolevel_step_matches_oracle(gpu_ops, orc, Mt, level):
    """fill-in, conditioned fine action, the three action differences and the accept decision of the two-level step
    between a GFF level and its coarsening (unrotated -> rotated and rotated -> unrotated), against the oracle"""
    import torch
    from mlmcpathintegral_amd import abi
    mass = 10.0
    fine, coarse = Level(Mt, ROTATE, level, mass, 0 if level == 0 else 2), None
    Mt_c = fine.Mt_c
    coarse = Level(Mt_c, ROTATE, level + 1, mass, 2)
    ofine, ocoarse = OLevel(orc, Mt, ROTATE, level, mass, 0 if level == 0 else 2), OLevel(orc, Mt_c, ROTATE, level + 1, mass, 2)
    B, seed = 6, 77
    rng = np.random.default_rng(5)
    theta0 = 0.3 * rng.normal(size=(B, fine.N))
    phic0 = 0.3 * rng.normal(size=(B, coarse.N))
    theta = torch.tensor(theta0, device="cuda")
    phic = torch.tensor(phic0, device="cuda")
    nbytes = C.c_size_t()
    abi.call("mlmcpi_gff_twolevel_workspace_bytes", fine.h, B, C.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    terms = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_twolevel_draw", fine.h, coarse.h, C.c_void_p(phic.data_ptr()), C.c_void_p(theta.data_ptr()), B, seed, 2, 9,
             C.c_void_p(work.data_ptr()), C.c_void_p(acc.data_ptr()), C.c_void_p(terms.data_ptr()), None)
    got, gacc, gterms = theta.cpu().numpy(), acc.cpu().numpy(), terms.cpu().numpy()
    n_acc = 0
    for c in range(B):
        want = theta0[c].copy()
        t = np.zeros(3)
        a = ofine.L.orc_gff_dev_twolevel_draw(ofine.h, ocoarse.h, np.ascontiguousarray(phic0[c]), want, seed, 2 + c, 9, t)
        assert np.allclose(gterms[c], t, rtol=1e-9, atol=1e-9), (gterms[c], t)
        assert a == gacc[c]
        assert np.max(np.abs(got[c] - want)) < 1e-11
        n_acc += a
    # conditioned fine action on its own
    S = torch.zeros(B, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_cfa_evaluate", fine.h, C.c_void_p(theta.data_ptr()), B, C.c_void_p(S.data_ptr()), None)
    for c in range(B):
        assert abs(S[c].item() - ofine.L.orc_gff_cfa_evaluate(ofine.h, np.ascontiguousarray(got[c]))) < 1e-10


@pytest.mark.gpu
def test_gff_two_level_chain_samples_the_fine_distribution(gpu_ops, orc):
    """16 x 16 GFF (mass 10, CoarsenRotate): coarse samples from the smoothed coarse action's own exact sampler
    (GFFAction::draw with n_gibbs_smooth = 2, the reference's GFFSamplerFactory), filled in and accepted by the two-level
    step: <phi^2> of the fine chain against gff_phi_squared_analytical, and a high acceptance rate (the coarse action is
    two Gibbs sweeps away from the exact marginal)."""
    import torch
    from conftest import zcheck
    from mlmcpathintegral_amd import abi
    Mt, mass, B, n_burn, n = 16, 10.0, 512, 20, 200
    fine, coarse = Level(Mt, ROTATE, 0, mass, 0), Level(Mt, ROTATE, 1, mass, 2)
    theta = torch.zeros((B, fine.N), dtype=torch.float64, device="cuda")
    phic = torch.zeros((B, coarse.N), dtype=torch.float64, device="cuda")
    nbytes = C.c_size_t()
    abi.call("mlmcpi_gff_twolevel_workspace_bytes", fine.h, B, C.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    vals, n_acc = [], 0
    for k in range(n_burn + n):
        abi.call("mlmcpi_gff_level_draw", coarse.h, C.c_void_p(phic.data_ptr()), B, 5, 0, k, None)
        abi.call("mlmcpi_gff_twolevel_draw", fine.h, coarse.h, C.c_void_p(phic.data_ptr()), C.c_void_p(theta.data_ptr()), B, 5, 0, k,
                 C.c_void_p(work.data_ptr()), C.c_void_p(acc.data_ptr()), None, None)
        if k >= n_burn:
            vals.append(gpu_ops.qoi_phi_squared(theta))
            n_acc += int(acc.sum().item())
    v = torch.stack(vals).mean(dim=0)
    m, e = float(v.mean()), float(v.std(unbiased=True)) / math.sqrt(B)
    exact = orc.lib().orc_gff_phi_squared_analytical(mass, Mt, Mt)
    p_acc = n_acc / (n * B)
    print(f"GFF two-level chain 16^2: <phi^2> = {m:.6f} +- {e:.6f} (exact {exact:.6f}), acceptance {p_acc:.3f}")
    zcheck("GFF two-level chain 16^2: <phi^2> vs closed form", m, e, exact)
    # the acceptance rate expected from the reference author's matrices with Lattice2D's order of the Gibbs sweep
    # (tests/golden/gff_qhat.json: 0.9863 +- 0.0001; the Python class's own sweep order would give 0.9910)
    want = next(a for a in _qhat_fixture()["twolevel_expected_acceptance"] if a["order"] == "lattice2d")
    zcheck("GFF two-level chain 16^2: acceptance vs the reference author's matrices", p_acc,
           math.sqrt(p_acc * (1.0 - p_acc) / (n * B)) * 3.0, want["mean"], want["error"])   # (x 3: successive steps of a chain are correlated)
    assert p_acc > 0.5


# ---- beyond one workgroup pass ----------------------------------------------------------------------------------------------
# Every kernel of gff_levels.hip runs 256 threads over a chain with a stride loop.  The cases above have at most 256
# vertices per chain, so no loop there takes a second pass, no accumulator a second term, no copy a second block.  The
# shapes here are the smallest at which each loop does something new:
#   24 x 24 level 0   576 = 2 * 256 + 64 vertices: three passes, the last one ragged; three blocks in the copy / accept kernels
#   24 x 24 level 1   288 = 256 + 32 (rotated): two passes, ragged
#   32 x 32 level 1   512 (rotated), coarse level 256: exact multiples of the block, both levels dense
#   17 x 17           289, odd, not coarsenable (CoarsenBoth level 0): the odd tail of the normals on the 145th pair
#   3 x 3             9: the odd tail inside one pass
# held to the long-double restatement (tests/gff_level_reference.py) and to the oracle.  Dense levels above 1024 vertices
# (kMaxDense = 4096) stay untested.
import functools

import gff_level_reference as ref

MASS = 10.0
BIG = [(24, ROTATE, 0), (24, ROTATE, 1), (32, ROTATE, 1)]
ODD = [(17, BOTH, 0), (3, BOTH, 0)]


@functools.lru_cache(maxsize=None)
def _pair(Mt, ctype, level, n_gibbs, omega=1.0):
    """library and oracle handles of one level, made once per session (the dense set-up of 576 vertices takes 0.7 s each)"""
    import oracle
    return Level(Mt, ctype, level, MASS, n_gibbs, omega), OLevel(oracle, Mt, ctype, level, MASS, n_gibbs, omega)


def _ref_energy(lv):
    if lv.n_gibbs == 0:
        nb = lv.nb()
        return lambda phi: ref.stencil_energy(phi, nb, lv.mu2)
    Q = lv.matrix(0)
    return lambda phi: ref.dense_energy(phi, Q)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_coarsen_rotate_with_odd_extents_has_no_coarse_level():
    """An unrotated CoarsenRotate level coarsens to a rotated lattice, which needs even extents (lattice2d.cc:13-15).  A
    17 x 17 level used to report the 145 vertices with i + j even as coarse vertices -- mapped onto 128 distinct indices of
    a coarse lattice that cannot exist, next to a coarse buffer of 17 * 17 / 2 = 144 entries.  Now it has no coarse level,
    and the copies refuse before any launch (host checks only: no device is touched)."""
    from mlmcpathintegral_amd import abi
    lv = Level(17, ROTATE, 0, 1.0)
    assert lv.N == 289 and lv.n_coarse == 0 and lv.Mt_c == 0
    dummy = np.zeros(289)
    p = dummy.ctypes.data_as(C.c_void_p)
    for name in ("mlmcpi_gff_copy_from_fine", "mlmcpi_gff_copy_from_coarse"):
        with pytest.raises(abi.MlmcpiError, match="the lattice has no coarse level"):
            abi.call(name, lv.h, p, p, 1, None)
    with pytest.raises(abi.MlmcpiError, match="the lattice has no coarse level"):
        abi.call("mlmcpi_gff_cfa_fill", lv.h, p, 1, 1, 0, 0, p, None)
    nbytes = C.c_size_t()
    with pytest.raises(abi.MlmcpiError):
        abi.call("mlmcpi_gff_twolevel_workspace_bytes", lv.h, 1, C.byref(nbytes))
    # even extents coarsen as before; CoarsenBoth with odd extents never did
    assert Level(18, ROTATE, 0, 1.0).n_coarse == 162 and Level(17, BOTH, 0, 1.0).n_coarse == 0


def _eval_cases():
    out = [(Mt, ct, lv, ng) for Mt, ct, lv in BIG for ng in (0, 2)]
    return out + [(Mt, ct, lv, ng) for Mt, ct, lv in ODD for ng in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,ctype,level,n_gibbs", _eval_cases())
def test_level_evaluate_beyond_one_pass(gpu_ops, Mt, ctype, level, n_gibbs):
    """mlmcpi_gff_level_evaluate, table kernel (n_gibbs = 0) and dense kernel: four seeded fields that no draw made, and one
    that is non-zero at a single vertex of the last pass, whose action is 1/2 Q_ll v^2 (a kernel that stops after the first
    pass returns 0)."""
    import torch
    from mlmcpathintegral_amd import abi
    a, b = _pair(Mt, ctype, level, n_gibbs)
    n = a.N
    phi = np.zeros((5, n))
    phi[:4] = 0.3 * np.random.default_rng(n + n_gibbs).normal(size=(4, n))
    l, v = n - 7, 1.5
    assert n <= 256 or l >= 256
    phi[4, l] = v
    d = torch.tensor(phi, device="cuda")
    S = torch.full((5,), -1.0, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_level_evaluate", a.h, _ptr(d), 5, _ptr(S), None)
    got, want = S.cpu().numpy(), _ref_energy(a)(phi)
    single = 0.5 * (4.0 + a.mu2 if n_gibbs == 0 else a.matrix(0)[l, l]) * v * v
    assert single > 1.0 and abs(float(want[4]) - single) < 1e-13 * single
    for c in range(5):
        print(f"evaluate {Mt} level {level} n_gibbs {n_gibbs} field {c}: S = {got[c]:.15g}, device - reference = {float(got[c] - want[c]):.2e}")
        assert abs(got[c] - want[c]) < 1e-10 * max(1.0, abs(float(want[c])))
        wo = b.L.orc_gff_level_evaluate(b.h, phi[c])
        assert abs(got[c] - wo) < 1e-10 * max(1.0, abs(wo))


def _draw_want(a, b, orc, seed, chains, step, n_gibbs, omega):
    """reference and oracle draws of the given chains: ([len(chains), N] long double, the same from the oracle)"""
    n, m = a.N, (a.N + 1) // 2
    psi = np.stack([ref.pair_normals(ref.oracle_random(orc, seed, c, step, ref.P_GFF_EXACT, 0, m), n) for c in chains])
    gibbs = np.zeros((n_gibbs, len(chains), n), dtype=ref.LD)
    for k in range(n_gibbs):
        for i, c in enumerate(chains):
            gibbs[k, i] = ref.pair_normals(ref.oracle_random(orc, seed, c, step, ref.P_GFF_GIBBS, k, m), n)
    want = ref.level_draw(psi, a.matrix(1), a.nb(), a.mu2, omega, gibbs)
    wo = np.zeros((len(chains), n))
    for i, c in enumerate(chains):
        b.L.orc_gff_level_dev_draw(b.h, wo[i], seed, c, step)
    return want, wo


def _draw_cases():
    out = []
    for Mt, ct, lv in BIG + ODD:
        ng = 2 if (Mt, ct, lv) in BIG else 1
        out += [(Mt, ct, lv, 0, 1.0), (Mt, ct, lv, ng, 1.0), (Mt, ct, lv, ng, 1.3)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,ctype,level,n_gibbs,omega", _draw_cases())
def test_level_draw_beyond_one_pass(gpu_ops, orc, Mt, ctype, level, n_gibbs, omega):
    """mlmcpi_gff_level_draw: white noise over more than 128 pairs (and an odd last one), the triangular product with more
    than one row per thread, Gibbs sweeps over the whole level; chain0 != 0; every vertex of every chain."""
    import torch
    from mlmcpathintegral_amd import abi
    a, b = _pair(Mt, ctype, level, n_gibbs, omega)
    B, seed, chain0, step = 5, 31, 3, 7
    phi = torch.full((B, a.N), 99.0, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_level_draw", a.h, _ptr(phi), B, seed, chain0, step, None)
    got = phi.cpu().numpy()
    want, wo = _draw_want(a, b, orc, seed, range(chain0, chain0 + B), step, n_gibbs, omega)
    for c in range(B):
        scale = max(1.0, float(np.abs(want[c]).max()))
        print(f"draw {Mt} level {level} n_gibbs {n_gibbs} omega {omega} chain {c}: device - reference = "
              f"{float(np.max(np.abs(got[c] - want[c]))):.2e}, max|phi| = {scale:.3f}")
        assert np.max(np.abs(got[c] - want[c])) < 1e-11 * scale
        assert np.max(np.abs(got[c] - wo[c])) < 1e-11 * scale


@pytest.mark.gpu
def test_level_draw_chain_index_past_a_byte(gpu_ops, orc):
    """300 chains in one launch (key.chain += b with b > 255), 8 x 8 rotated level with two Gibbs sweeps"""
    import torch
    from mlmcpathintegral_amd import abi
    a, b = _pair(8, ROTATE, 1, 2)
    B, seed, chain0, step = 300, 31, 3, 2
    phi = torch.full((B, a.N), 99.0, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_level_draw", a.h, _ptr(phi), B, seed, chain0, step, None)
    got = phi.cpu().numpy()
    spots = [0, 1, 255, 256, 299]
    want, wo = _draw_want(a, b, orc, seed, [chain0 + c for c in spots], step, 2, 1.0)
    for i, c in enumerate(spots):
        scale = max(1.0, float(np.abs(want[i]).max()))
        assert np.max(np.abs(got[c] - want[i])) < 1e-11 * scale and np.max(np.abs(got[c] - wo[i])) < 1e-11 * scale
    assert not np.any(got == 99.0)


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,ctype,level", BIG)
def test_copies_and_fill_in_beyond_one_block(gpu_ops, orc, Mt, ctype, level):
    """mlmcpi_gff_copy_from_fine / copy_from_coarse / cfa_fill / cfa_evaluate as calls of their own: copies bit for bit (more
    than 256 pairs: a second block of gff_pairs_copy_kernel), vertices that a call must not write left as they were"""
    import torch
    from mlmcpathintegral_amd import abi
    ng = 0 if level == 0 else 2
    a, b = _pair(Mt, ctype, level, ng)
    nb, (pairs, fineonly) = a.nb(), a.tables()
    fidx, n, nc, B = pairs[0::2], a.N, a.n_coarse, 3
    assert len(fineonly) == n - nc and (nc > 256 or (Mt, level) != (24, 0))   # 288 pairs at 24 x 24 level 0: a second block
    rng = np.random.default_rng(n)
    fine0, coarse0 = rng.normal(size=(B, n)), rng.normal(size=(B, nc))
    # fine -> coarse
    dc = torch.full((B, nc), -7.25, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_copy_from_fine", a.h, _ptr(torch.tensor(fine0, device="cuda")), _ptr(dc), B, None)
    got = dc.cpu().numpy()
    assert np.array_equal(got, ref.copy_from_fine(fine0, pairs, nc))
    for c in range(B):
        want = np.zeros(nc)
        b.L.orc_gff_copy(b.h, fine0[c].copy(), want, 1)
        assert np.array_equal(got[c], want)
    # coarse -> fine: the fine-only vertices keep their sentinel
    df = torch.full((B, n), -7.25, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_copy_from_coarse", a.h, _ptr(torch.tensor(coarse0, device="cuda")), _ptr(df), B, None)
    got = df.cpu().numpy()
    assert np.array_equal(got, ref.copy_from_coarse(coarse0, pairs, np.full((B, n), -7.25)))
    assert np.all(got[:, fineonly] == -7.25) and not np.any(got[:, fidx] == -7.25)
    # fill-in: coarse vertices untouched, fine-only ones and S_cfa against the reference and the oracle
    seed, chain0, step = 77, 2, 9
    state0 = 0.3 * rng.normal(size=(B, n))
    ds = torch.tensor(state0, device="cuda")
    S = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    abi.call("mlmcpi_gff_cfa_fill", a.h, _ptr(ds), B, seed, chain0, step, _ptr(S), None)
    got, gotS = ds.cpu().numpy(), S.cpu().numpy()
    assert np.array_equal(got[:, fidx], state0[:, fidx])
    normals = np.stack([ref.oracle_random(orc, seed, chain0 + c, step, ref.P_FILLIN, 0, n)[:, 2] for c in range(B)])
    want, wantS = ref.cfa_fill(state0, nb, fineonly, a.mu2, normals)
    for c in range(B):
        assert np.max(np.abs(got[c] - want[c])) < 1e-11 * max(1.0, float(np.abs(want[c]).max()))
        assert abs(gotS[c] - wantS[c]) < 1e-10 * max(1.0, float(wantS[c]))
        wo = state0[c].copy()
        So = b.L.orc_gff_cfa_dev_fill(b.h, wo, seed, chain0 + c, step)
        assert np.max(np.abs(got[c] - wo)) < 1e-11 * max(1.0, np.abs(wo).max()) and abs(gotS[c] - So) < 1e-10 * max(1.0, So)
    # conditioned fine action of a state that no fill-in made
    abi.call("mlmcpi_gff_cfa_evaluate", a.h, _ptr(torch.tensor(state0, device="cuda")), B, _ptr(S), None)
    gotS, wantS = S.cpu().numpy(), ref.cfa_action(state0, nb, fineonly, a.mu2)
    for c in range(B):
        assert abs(gotS[c] - wantS[c]) < 1e-10 * max(1.0, float(wantS[c]))
        assert abs(gotS[c] - b.L.orc_gff_cfa_evaluate(b.h, state0[c])) < 1e-10 * max(1.0, float(wantS[c]))


@functools.lru_cache(maxsize=None)
def _twolevel_case(Mt, level):
    """Inputs of the two-level cases and what the oracle makes of them.  Current fine states: chains 0-3 are samples of the
    fine level's plain stencil (numpy normals through the library's host matrix), chains 4-7 seeded normals of amplitude 3
    (far from a sample).  Coarse proposals: for the even chains the coarse vertices of the current state plus noise of 1e-3
    (the step then only replaces the fill-in), for the odd ones rough, unit-variance noise -- the construction of
    test_twolevel_step_matches_oracle for the paths.  The Gaussian fill-in is exact and the smoothed coarse action close to
    the marginal, so a step from a sample is accepted nearly always; the steps from the far states supply the rejections."""
    B, seed, chain0, step = 8, 78, 2, 9   # (seed 77 accepts all eight chains of 24 x 24 level 0)
    fine, ofine = _pair(Mt, ROTATE, level, 0 if level == 0 else 2)
    coarse, ocoarse = _pair(fine.Mt_c, ROTATE, level + 1, 2)
    pairs, _ = fine.tables()
    rng = np.random.default_rng(100 * Mt + level)
    theta0 = rng.normal(size=(B, fine.N))
    theta0[:4] = theta0[:4] @ np.tril(fine.matrix(1))
    theta0[4:] *= 3.0
    phic0 = ref.copy_from_fine(theta0, pairs, coarse.N)
    phic0[0::2] += 1e-3 * rng.normal(size=phic0[0::2].shape)
    phic0[1::2] = rng.normal(size=phic0[1::2].shape)
    want, terms, acc = theta0.copy(), np.zeros((B, 3)), np.zeros(B, dtype=np.int32)
    for c in range(B):
        acc[c] = ofine.L.orc_gff_dev_twolevel_draw(ofine.h, ocoarse.h, np.ascontiguousarray(phic0[c]), want[c], seed, chain0 + c, step, terms[c])
    return dict(B=B, seed=seed, chain0=chain0, step=step, fine=fine, coarse=coarse, theta0=theta0, phic0=phic0, want=want, terms=terms,
                acc=acc)


TWOLEVEL = [(24, 0), (24, 1), (32, 1)]


@pytest.mark.parametrize("Mt,level", TWOLEVEL)
def test_twolevel_inputs_give_both_outcomes_and_the_reference_agrees(orc, Mt, level):
    """CPU: the oracle accepts some chains of each case and rejects others (a condition of the GPU test, not a measurement),
    and the long-double restatement gives the same action differences, decisions and states."""
    k = _twolevel_case(Mt, level)
    assert set(k["acc"].tolist()) == {0, 1}, k["acc"]
    fine, B = k["fine"], k["B"]
    pairs, fineonly = fine.tables()
    normals = np.stack([ref.oracle_random(orc, k["seed"], k["chain0"] + c, k["step"], ref.P_FILLIN, 0, fine.N)[:, 2] for c in range(B)])
    prime, terms = ref.twolevel_step(k["theta0"], k["phic0"], fine.nb(), pairs, fineonly, fine.mu2, normals, _ref_energy(fine),
                                     _ref_energy(k["coarse"]))
    u = np.array([ref.oracle_random(orc, k["seed"], k["chain0"] + c, k["step"], ref.P_ACCEPT2, 0, 1)[0, 0] for c in range(B)])
    assert np.array_equal(ref.accepts(terms, u), k["acc"] == 1)
    for c in range(B):
        assert np.max(np.abs(terms[c] - k["terms"][c])) < 1e-10 * max(1.0, np.abs(k["terms"][c]).max())
        assert np.max(np.abs((prime[c] if k["acc"][c] else k["theta0"][c]) - k["want"][c])) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,level", TWOLEVEL)
def test_twolevel_step_beyond_one_block(gpu_ops, orc, Mt, level):
    """mlmcpi_gff_twolevel_draw with more than 256 fine vertices: gff_twolevel_accept_kernel runs two or three blocks per
    chain, of which only the first writes the flag while all of them copy.  Accepted chains hold the whole trial state
    (bit for bit the one in the workspace, vertices >= 256 included), rejected ones their input, bit for bit."""
    import torch
    from mlmcpathintegral_amd import abi
    k = _twolevel_case(Mt, level)
    fine, coarse, B, acc_o = k["fine"], k["coarse"], k["B"], k["acc"]
    assert set(acc_o.tolist()) == {0, 1} and fine.N > 256
    nbytes = C.c_size_t()
    abi.call("mlmcpi_gff_twolevel_workspace_bytes", fine.h, B, C.byref(nbytes))
    phic = torch.tensor(k["phic0"], device="cuda")

    def run(with_outputs):
        theta = torch.tensor(k["theta0"], device="cuda")
        work = torch.zeros(nbytes.value, dtype=torch.uint8, device="cuda")
        acc = torch.full((B,), -5, dtype=torch.int32, device="cuda")
        terms = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
        abi.call("mlmcpi_gff_twolevel_draw", fine.h, coarse.h, _ptr(phic), _ptr(theta), B, k["seed"], k["chain0"], k["step"], _ptr(work),
                 _ptr(acc) if with_outputs else None, _ptr(terms) if with_outputs else None, None)
        prime = work[:B * fine.N * 8].view(torch.float64).reshape(B, fine.N)   # workspace: theta' [B N_f] first
        return theta.cpu().numpy(), prime.cpu().numpy(), acc.cpu().numpy(), terms.cpu().numpy()

    got, prime, acc, terms = run(True)
    pairs, fineonly = fine.tables()
    normals = np.stack([ref.oracle_random(orc, k["seed"], k["chain0"] + c, k["step"], ref.P_FILLIN, 0, fine.N)[:, 2] for c in range(B)])
    rprime, rterms = ref.twolevel_step(k["theta0"], k["phic0"], fine.nb(), pairs, fineonly, fine.mu2, normals, _ref_energy(fine),
                                       _ref_energy(coarse))
    for c in range(B):
        scale = max(1.0, float(np.abs(k["terms"][c]).max()))
        print(f"two-level {Mt} level {level} chain {c}: terms {terms[c]}, device - reference {np.max(np.abs(terms[c] - rterms[c])):.2e}, accept {acc[c]}")
        assert np.max(np.abs(terms[c] - rterms[c])) < 1e-10 * scale and np.max(np.abs(terms[c] - k["terms"][c])) < 1e-10 * scale
        assert acc[c] == acc_o[c]
        assert np.max(np.abs(prime[c] - rprime[c])) < 1e-11 * max(1.0, float(np.abs(rprime[c]).max()))
        if acc_o[c]:
            assert np.array_equal(got[c], prime[c]) and np.array_equal(got[c, 256:], prime[c, 256:])
            assert np.max(np.abs(got[c] - k["want"][c])) < 1e-11 * max(1.0, np.abs(k["want"][c]).max())
        else:
            assert np.array_equal(got[c], k["theta0"][c])
    # d_accept = NULL and d_terms = NULL: the same step, nothing reported
    got2, _, acc2, terms2 = run(False)
    assert np.array_equal(got2, got) and np.all(acc2 == -5) and np.all(terms2 == 0.0)
