"""CPU: pins tests/sigma_correlator_reference.py (the long-double reference of mlmcpi_sigma_level_correlator) to the
definitions, the host arithmetic of include/mlmcpi/correlator.hh to its closed forms, and the driver's --correlator refusals."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigma_correlator_reference as ref
import sigma_level_model as lm
import sigma_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "driver")
SMALL = [(2, 2), (4, 2), (2, 6), (6, 4)]
LEVELS = [(Mt, Mx, rot) for Mt, Mx in SMALL for rot in (0, 1)]


def _random_state(Mt, Mx, rot, B, seed):
    return lm.initialise(lm.Level(Mt, Mx, rot), B, seed)


@pytest.mark.parametrize("Mt,Mx,rot", LEVELS + [(8, 12, 0), (8, 12, 1)])
def test_coordinate_map_is_the_level_model_s(Mt, Mx, rot):
    L = lm.Level(Mt, Mx, rot)
    i, j = ref.coords(Mt, Mx, rot)
    assert [(int(a), int(b)) for a, b in zip(i, j)] == [tuple(c) for c in L.coords]
    assert i.size == L.n == ref.nvert(Mt, Mx, rot)


@pytest.mark.parametrize("Mt,Mx,rot", LEVELS)
def test_correlator_is_the_double_sum_over_vertex_pairs(Mt, Mx, rot):
    phi = _random_state(Mt, Mx, rot, 5, 11)
    C, brute = ref.correlator(Mt, Mx, rot, phi), ref.brute_force(Mt, Mx, rot, phi)
    assert C.shape == (5, ref.n_out(Mt, Mx)) and C.dtype == np.longdouble
    assert float(np.max(np.abs(C - brute))) <= 1e-15 * Mt * Mx
    # a slice of a rotated level holds half the vertices of a row / column, and all slices exist
    St, Sx = ref.slice_sums(Mt, Mx, rot, phi)
    assert St.shape == (5, Mt, 3) and Sx.shape == (5, Mx, 3)
    assert np.all(np.abs(St).sum(axis=(0, 2)) > 0) and np.all(np.abs(Sx).sum(axis=(0, 2)) > 0)


@pytest.mark.parametrize("Mt,Mx,rot", LEVELS + [(10, 16, 0), (10, 16, 1)])
def test_sum_identities_and_structure_factor(Mt, Mx, rot):
    phi = _random_state(Mt, Mx, rot, 6, 3)
    Ct, Cx = ref.split(ref.correlator(Mt, Mx, rot, phi), Mt, Mx)
    chi = lm.magnetic_susceptibility(lm.Level(Mt, Mx, rot), phi)
    if not rot:
        assert np.allclose(chi, sm.magnetic_susceptibility(phi, Mt, Mx), rtol=1e-14, atol=0)
    bound = 1e-14 * Mt * Mx
    assert float(np.max(np.abs(ref.susceptibility(Ct, Mt) - chi))) <= bound
    assert float(np.max(np.abs(ref.susceptibility(Cx, Mx) - chi))) <= bound
    St, Sx = ref.slice_sums(Mt, Mx, rot, phi)
    N = ref.nvert(Mt, Mx, rot)
    for C, S, M in ((Ct, St, Mt), (Cx, Sx, Mx)):
        ph = np.exp(2j * np.pi * np.arange(M) / M)
        F = (np.abs(np.einsum("bic,i->bc", S.astype(np.float64), ph)) ** 2).sum(axis=-1) / N
        assert float(np.max(np.abs(ref.structure_factor(C, M) - F))) <= bound


@pytest.mark.parametrize("M", [8, 64])
@pytest.mark.parametrize("m", [0.1, 1.0])
def test_xi_second_moment_of_a_single_cosh(M, m):
    xi = float(ref.xi_second_moment(ref.single_cosh(M, m), M))
    assert abs(xi - 1.0 / (2.0 * np.sinh(0.5 * m))) <= 1e-12 * xi, (xi, 1.0 / (2.0 * np.sinh(0.5 * m)))


def test_host_xi_second_moment_of_a_single_cosh(tmp_path):
    """the C++ functions of include/mlmcpi/correlator.hh themselves, in a program of a dozen lines"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "xi.cc"
    src.write_text('#include <cstdio>\n#include "mlmcpi/correlator.hh"\nint main() {\n  const unsigned Ms[2] = {8, 64};\n'
                   '  const double ms[2] = {0.1, 1.0};\n  for (unsigned M : Ms) for (double m : ms) {\n    std::vector<double> C;\n'
                   '    for (unsigned t = 0; t <= M / 2; ++t) C.push_back((std::exp(-m * t) + std::exp(-m * (M - t))) / (1.0 - std::exp(-m * M)));\n'
                   '    std::printf("%u %.17g %.17g %.17g %.17g\\n", M, m, mlmcpi::xi_second_moment(C, M), mlmcpi::structure_factor(C, M),\n'
                   '                mlmcpi::correlator_susceptibility(C, M));\n  }\n  return 0;\n}\n')
    exe = tmp_path / "xi"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:4]
    assert len(lines) == 4
    for line in lines:
        M, m, xi, F, chi = line.split()
        M, m, xi, F, chi = int(M), float(m), float(xi), float(F), float(chi)
        C = ref.single_cosh(M, m)
        assert abs(xi - 1.0 / (2.0 * np.sinh(0.5 * m))) <= 1e-12 * xi
        assert abs(F - ref.structure_factor(C, M)) <= 1e-13 * F and abs(chi - ref.susceptibility(C, M)) <= 1e-13 * chi


def test_exact_two_by_two_values_and_a_heat_bath_chain():
    """C_t(0) = 1 + c1, C_t(1) = c1 + c2 on the 2 x 2 lattice (a ring of four spins with coupling 2 beta), against 512 chains of
    the model's heat bath at beta = 1: 20 sweeps of burn-in, then 60 draws of 2 sweeps; error = spread of the chain means.
    z-values at this seed: C_t(0) +0.65, C_t(1) -0.18, C_x(0) -0.70, C_x(1) +0.50 (gate 4.5)."""
    beta, B, seed = 1.0, 512, 20261
    c1, c2 = ref.ring_c1_c2(beta)
    S_exact, chi_exact = sm.ring_exact(beta)
    assert abs(chi_exact - (1.0 + 2.0 * c1 + c2)) < 1e-14 and abs(S_exact + 8.0 * beta * c1) < 1e-13
    phi = sm.sweep_draw(sm.initialise(B, 2, 2, seed), 2, 2, beta, 0, 20, seed, 0, 0)
    acc = np.zeros((B, 4))
    n = 60
    for k in range(n):
        phi = sm.sweep_draw(phi, 2, 2, beta, 0, 2, seed, 0, 20 + 2 * k)
        acc += ref.correlator(2, 2, 0, phi).astype(np.float64)
    means = acc / n
    mean, err = means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(B)
    z = (mean - np.array([1.0 + c1, c1 + c2, 1.0 + c1, c1 + c2])) / err
    print("z-values (C_t(0), C_t(1), C_x(0), C_x(1)):", z)
    assert np.all(np.abs(z) < 4.5), z


REFUSALS = [
    (["--action", "schwinger", "--sampler", "heatbath"], "--correlator 1 is not supported for chosen action"),
    (["--action", "gff", "--sampler", "heatbath"], "--correlator 1 is not supported for chosen action"),
    (["--action", "rotor", "--sampler", "heatbath"], "--correlator 1 is not supported for chosen action"),
    (["--action", "nonlinearsigma", "--sampler", "heatbath", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--method", "twolevel"],
     "--correlator 1 runs --method singlelevel only, not twolevel"),
    (["--action", "nonlinearsigma", "--sampler", "heatbath", "--method", "throughput"],
     "--correlator 1 runs --method singlelevel only, not throughput"),
    (["--action", "nonlinearsigma", "--sampler", "hierarchical", "--coarsening", "rotate", "--coarsesampler", "heatbath"],
     "--correlator 1 takes --sampler heatbath, wolff or swendsenwang, not hierarchical"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_driver_refuses_the_correlator_where_it_is_not_built(args, message):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    r = subprocess.run([EXE, *args, "--Mt_lat", "16", "--correlator", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-2000:]
