"""CPU: the long-double restatement of the GFF multilevel glue and of the spectral sampler (tests/gff_level_reference.py)
against the oracle's orc_gff_level_* functions and orc_dev_gff_exact_draw at the sizes the suite has had all along
(Mt = 8, 16), so that the two independent statements agree before tests/test_gff_levels.py and tests/test_gpu_parity.py
hold the device to either; and the error of the double-precision ifft2 form at the large lattices of the GPU tests."""
import os
import re

import numpy as np
import pytest

import gff_level_reference as ref
from test_gff_levels import BOTH, ROTATE, Level, OLevel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SEED = 0x1234567812345678


def test_purposes_are_the_ones_of_the_sources():
    src = ""
    for name in ("device_common.hpp", "gff_levels.hip"):
        with open(os.path.join(ROOT, "mlmcpathintegral_amd", "csrc", name)) as f:
            src += f.read()
    for name in ("P_FILLIN", "P_ACCEPT2", "P_EXACT", "P_GFF_GIBBS", "P_GFF_EXACT"):
        m = re.search(r"\b%s = (\d+)\b" % name, src)
        assert m and int(m.group(1)) == getattr(ref, name), name


def test_pair_normals_take_both_branches_and_drop_the_odd_tail():
    rows = np.arange(20.0).reshape(5, 4)
    assert np.array_equal(ref.pair_normals(rows, 10), [2, 3, 6, 7, 10, 11, 14, 15, 18, 19])
    assert np.array_equal(ref.pair_normals(rows, 9), [2, 3, 6, 7, 10, 11, 14, 15, 18])
    with pytest.raises(AssertionError):
        ref.pair_normals(rows, 11)


def _energy(lv):
    if lv.n_gibbs == 0:
        nb = lv.nb()
        return lambda phi: ref.stencil_energy(phi, nb, lv.mu2)
    Q = lv.matrix(0)
    return lambda phi: ref.dense_energy(phi, Q)


@pytest.mark.parametrize("Mt,ctype,level,n_gibbs,omega", [(8, ROTATE, 0, 0, 1.0), (8, ROTATE, 1, 2, 1.0), (16, ROTATE, 1, 2, 1.3),
                                                          (16, ROTATE, 0, 1, 1.0), (8, ROTATE, 1, 0, 1.0), (3, BOTH, 0, 1, 1.3)])
def test_level_energy_and_draw_equal_oracle(orc, Mt, ctype, level, n_gibbs, omega):
    mass, B, chain0, step = 10.0, 3, 4, 6
    a, b = Level(Mt, ctype, level, mass, n_gibbs, omega), OLevel(orc, Mt, ctype, level, mass, n_gibbs, omega)
    mu2 = ref.mu2_of(Mt, a.rotated, mass)
    # (the fp64 values come from four rounded operations: 1 / Mt, its square, mass^2, their product)
    assert abs(mu2 - a.mu2) <= 4 * 2.0 ** -52 * a.mu2 and abs(mu2 - b.L.orc_gff_level_mu2(b.h)) <= 4 * 2.0 ** -52 * a.mu2
    nb, n = a.nb(), a.N
    phi = 0.3 * np.random.default_rng(n).normal(size=(B, n))
    S = _energy(a)(phi)
    assert S.dtype == LD
    for c in range(B):
        want = b.L.orc_gff_level_evaluate(b.h, phi[c])
        assert abs(S[c] - want) < 1e-12 * max(1.0, abs(want))
    psi = np.stack([ref.pair_normals(ref.oracle_random(orc, SEED, chain0 + c, step, ref.P_GFF_EXACT, 0, (n + 1) // 2), n) for c in range(B)])
    gibbs = np.stack([[ref.pair_normals(ref.oracle_random(orc, SEED, chain0 + c, step, ref.P_GFF_GIBBS, k, (n + 1) // 2), n)
                       for c in range(B)] for k in range(n_gibbs)]) if n_gibbs else np.zeros((0, B, n))
    got = ref.level_draw(psi, a.matrix(1), nb, mu2, omega, gibbs)
    for c in range(B):
        want = np.zeros(n)
        b.L.orc_gff_level_dev_draw(b.h, want, SEED, chain0 + c, step)
        assert np.max(np.abs(got[c] - want)) < 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("Mt,level", [(8, 0), (8, 1), (16, 0), (16, 1)])
def test_fill_in_copies_and_two_level_step_equal_oracle(orc, Mt, level):
    mass, B, chain0, step = 10.0, 6, 2, 9
    ng = 0 if level == 0 else 2
    fine, ofine = Level(Mt, ROTATE, level, mass, ng), OLevel(orc, Mt, ROTATE, level, mass, ng)
    coarse, ocoarse = Level(fine.Mt_c, ROTATE, level + 1, mass, 2), OLevel(orc, fine.Mt_c, ROTATE, level + 1, mass, 2)
    nb, (pairs, fineonly) = fine.nb(), fine.tables()
    rng = np.random.default_rng(5)
    theta = 0.3 * rng.normal(size=(B, fine.N))
    phic = 0.3 * rng.normal(size=(B, coarse.N))
    # copies: bit for bit
    tc = ref.copy_from_fine(theta, pairs, coarse.N)
    back = ref.copy_from_coarse(phic, pairs, theta)
    for c in range(B):
        want = np.zeros(coarse.N)
        ofine.L.orc_gff_copy(ofine.h, theta[c].copy(), want, 1)
        assert np.array_equal(tc[c], want)
        want = theta[c].copy()
        ofine.L.orc_gff_copy(ofine.h, want, phic[c].copy(), 0)
        assert np.array_equal(back[c], want)
    normals = np.stack([ref.oracle_random(orc, SEED, chain0 + c, step, ref.P_FILLIN, 0, fine.N)[:, 2] for c in range(B)])
    filled, S = ref.cfa_fill(theta, nb, fineonly, fine.mu2, normals)
    for c in range(B):
        want = theta[c].copy()
        Sw = ofine.L.orc_gff_cfa_dev_fill(ofine.h, want, SEED, chain0 + c, step)
        assert np.max(np.abs(filled[c] - want)) < 1e-13 and abs(S[c] - Sw) < 1e-12 * max(1.0, Sw)
        assert abs(ref.cfa_action(theta[c], nb, fineonly, fine.mu2) - ofine.L.orc_gff_cfa_evaluate(ofine.h, theta[c])) < 1e-12 * max(1.0, Sw)
    prime, terms = ref.twolevel_step(theta, phic, nb, pairs, fineonly, fine.mu2, normals, _energy(fine), _energy(coarse))
    u = np.array([ref.oracle_random(orc, SEED, chain0 + c, step, ref.P_ACCEPT2, 0, 1)[0, 0] for c in range(B)])
    acc = ref.accepts(terms, u)
    for c in range(B):
        want, t = theta[c].copy(), np.zeros(3)
        a = ofine.L.orc_gff_dev_twolevel_draw(ofine.h, ocoarse.h, np.ascontiguousarray(phic[c]), want, SEED, chain0 + c, step, t)
        assert np.max(np.abs(terms[c] - t)) < 1e-10 * max(1.0, np.abs(t).max()), (terms[c], t)
        assert bool(a) == bool(acc[c])
        assert np.max(np.abs((prime[c] if a else theta[c]) - want)) < 1e-13


@pytest.mark.parametrize("Mt,mass", [(4, 2.0), (8, 10.0), (16, 1.0), (5, 3.0)])
def test_spectral_draw_equals_oracle_in_both_forms(orc, Mt, mass):
    A = orc.Action(orc.GFF, Mt=Mt, Mx=Mt, mass=mass)
    n, mu2 = Mt * Mt, ref.mu2_of(Mt, False, mass)
    assert abs(mu2 - orc.lib().orc_action_gff_mu2(A.h)) <= 4 * 2.0 ** -52 * mu2
    for chain, step in ((2, 0), (3, 1)):
        rows = ref.oracle_random(orc, SEED, chain, step, ref.P_EXACT, 0, n)
        want = np.zeros(n)
        orc.lib().orc_dev_gff_exact_draw(A.h, want, SEED, chain, step)
        scale = np.abs(want).max()
        direct = ref.spectral_direct(rows, Mt, Mt, mu2)
        assert direct.dtype == LD
        assert np.max(np.abs(direct - want)) < 1e-13 * scale
        assert np.max(np.abs(ref.spectral_fft(rows, Mt, Mt, mu2) - direct)) < 1e-13 * scale
        some = np.array([0, n - 1, n // 2 + 1])
        assert np.array_equal(ref.spectral_direct(rows, Mt, Mt, mu2, sites=some), direct[some])


@pytest.mark.parametrize("Mt", [576, 1024])
def test_double_precision_ifft2_is_far_inside_the_exact_samplers_tolerance(Mt):
    """The GPU tests hold the device to ifft2 in double precision at 576 x 576 and 1024 x 1024, at the exact sampler's
    tolerance 1e-12 max|phi|.  Distance of that ifft2 from the direct long-double sum on 64 sites spread over the lattice
    (seeded normals stand in for the Philox ones: the distance does not depend on their source), measured: 576:
    2.1e-16 max|phi|, 1024: 1.8e-16 max|phi| (with the spectrum computed in long double; 5e-14 with a double-precision
    spectrum, whose smallest eigenvalues cancel).  8 x the larger is 1.7e-15 max|phi|: the reference's own error is under
    0.2 % of the tolerance, which stays as it is; asserted here at 1/8 of it."""
    n, mass = Mt * Mt, 10.0
    rows = np.zeros((n, 4))
    rows[:, 2:] = np.random.default_rng(Mt).normal(size=(n, 2))
    mu2 = ref.mu2_of(Mt, False, mass)
    fft = ref.spectral_fft(rows, Mt, Mt, mu2)
    sites = np.concatenate([[0, 1, Mt - 1, Mt, n - Mt, n - 1], np.random.default_rng(1).integers(0, n, 58)])
    d = float(np.max(np.abs(fft[sites] - ref.spectral_direct(rows, Mt, Mt, mu2, sites=sites))) / np.abs(fft).max())
    print(f"ifft2 (double) against the direct long-double sum, {Mt} x {Mt}, 64 sites: {d:.2e} max|phi|")
    assert d < 1e-12 / 8
