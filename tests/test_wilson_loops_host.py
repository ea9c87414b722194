"""CPU: the host arithmetic on Wilson loops (include/mlmcpi/correlator.hh, WilsonLoops of include/mlmcpi/qoi.hh) through the
stand-alone host/test_wilson_loops: the exact series against the long-double series of tests/wilson_loops_reference.py, the Creutz
ratio of a pure area law, and the jackknife on a constructed input."""
import os
import subprocess

import numpy as np

import wilson_loops_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_wilson_loops")


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
    checks = [line for line in lines[:-1] if not line.startswith(("exact ", "jackknife "))]
    assert len(checks) == 18 and all(line.startswith("ok  ") for line in checks)
    assert sum("Creutz ratio of a pure area law" in line for line in checks) == 3
    assert sum("the loop around the whole lattice is 1" in line for line in checks) == 6
    # wilson_loop_exact against the Python series: 1e-13 relative at beta = 0.5, 2, 10 on 4 x 4 and 64 x 64, r, s <= 4
    exact = [line.split() for line in lines if line.startswith("exact ")]
    assert len(exact) == 3 * 2 * 16
    seen = set()
    for _, beta, Mt, Mx, r, s, value in exact:
        beta, Mt, Mx, r, s = float(beta), int(Mt), int(Mx), int(r), int(s)
        seen.add((beta, Mt))
        want = ref.wilson_loop_exact(beta, Mt, Mx, r, s)
        assert abs(float(value) / want - 1) <= 1e-13, (beta, Mt, Mx, r, s, value, want)
    assert seen == {(b, m) for b in (0.5, 2.0, 10.0) for m in (4, 64)}
    # the jackknife of chi(1, 1) = -log(mean) over chains with means 0.5 .. 0.8
    value, error, has = [line.split()[1:] for line in lines if line.startswith("jackknife ")][0]
    w = np.array([0.5, 0.6, 0.7, 0.8])
    leave = -np.log((w.sum() - w) / 3)
    assert has == "1" and abs(float(value) + np.log(w.mean())) <= 1e-15
    assert abs(float(error) - np.sqrt(3 / 4 * np.sum((leave - leave.mean()) ** 2))) <= 1e-15
