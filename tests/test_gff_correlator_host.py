"""CPU: the host arithmetic on the GFF slice correlators (include/mlmcpi/correlator.hh, GffCorrelator of include/mlmcpi/qoi.hh)
through the stand-alone host/test_gff_correlator: the mode sum and the dispersion relation against the long-double values of
tests/gff_correlator_reference.py, the effective mass of the exact law, and the jackknife of E_q on a constructed input."""
import os
import subprocess

import numpy as np

import gff_correlator_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_gff_correlator")


def _run():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def test_host_arithmetic():
    lines = _run()
    assert lines[-1] == "0 failure(s)"
    checks = [line for line in lines[:-1] if not line.startswith(("exact ", "dispersion ", "jackknife "))]
    assert len(checks) == 20 and all(line.startswith("ok  ") for line in checks)
    assert sum("the mode sum is the closed cosh form" in line for line in checks) == 8
    assert sum("the effective mass of the exact law is E_q" in line for line in checks) == 4
    # gff_dispersion_exact and gff_correlator_exact against long double: E to 1e-13 relative over its condition 1 / (E sinh E) of the
    # acosh, the mode sum to 1e-13 of C(0; q) (a sum of terms of that size)
    disp = [line.split() for line in lines if line.startswith("dispersion ")]
    assert len(disp) == 2 * 2 * 4
    for _, Mt, Mx, mass, q, value in disp:
        want = ref.dispersion_exact(int(Mt), int(Mx), float(mass), int(q))
        assert abs(float(value) - want) <= 1e-15 * float(np.cosh(want) / np.sinh(want)) * 4, (Mt, Mx, mass, q, value, want)
    exact = [line.split() for line in lines if line.startswith("exact ")]
    assert len(exact) == 2 * 4 * 9 + 2 * 4 * 33
    seen = set()
    for _, Mt, Mx, mass, q, tau, value in exact:
        Mt, Mx, mass, q, tau = int(Mt), int(Mx), float(mass), int(q), int(tau)
        seen.add((Mt, Mx, mass))
        want, scale = ref.correlator_exact(Mt, Mx, mass, q, tau), ref.correlator_exact(Mt, Mx, mass, q, 0)
        assert abs(float(value) - want) <= 1e-13 * scale, (Mt, Mx, mass, q, tau, value, want)
    assert seen == {(16, 16, 1.0), (16, 16, 8.0), (64, 32, 1.0), (64, 32, 8.0)}
    # the jackknife of E = acosh((C0 + C2) / (2 C1)) over four chains
    value, error, has = [line.split()[1:] for line in lines if line.startswith("jackknife ")][0]
    E = 0.7
    m = np.array([[(b + 1.0) * np.cosh(E * (2.0 - tau)) for tau in range(3)] for b in range(4)])
    m[:, 1] *= 1.0 - 0.05 * np.arange(4)
    mass_of = lambda c: np.arccosh((c[0] + c[2]) / (2 * c[1]))
    leave = np.array([mass_of((m.sum(axis=0) - m[b]) / 3) for b in range(4)])
    assert has == "1" and abs(float(value) - mass_of(m.mean(axis=0))) <= 1e-14
    assert abs(float(error) - np.sqrt(3 / 4 * np.sum((leave - leave.mean()) ** 2))) <= 1e-14
