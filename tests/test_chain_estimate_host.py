"""CPU: the host arithmetic the measurements beside the QoI share (include/mlmcpi/chain_estimate.hh) through the stand-alone
host/test_chain_estimate: the chain-spread and naive errors, the jackknife over chains with the xi_2, effective-mass, Creutz-ratio
and offset-slice functions of the four classes of include/mlmcpi/qoi.hh against numpy, and the static entry points of WilsonLoops and
GffCorrelator against tests/golden/chain_estimate_statics.txt, character for character."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_chain_estimate")
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_estimate_statics.txt")

# the input of the jackknife runs of host/test_chain_estimate.cc
M = np.array([[1.00, 0.60, 0.45, 1.10, 0.62, 0.50],
              [1.05, 0.58, 0.40, 1.00, 0.66, 0.48],
              [0.95, 0.64, 0.50, 1.20, 0.70, 0.52],
              [1.10, 0.55, 0.42, 0.90, 0.58, 0.44]])


def _run(*args):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def xi_second_moment(C, M_):
    """correlator.hh: sqrt(chi / F - 1) / (2 sin(pi / M)) with the folded weights 1, 2, .., 2, 1"""
    tau = np.arange(M_ // 2 + 1)
    w = np.where((tau == 0) | (2 * tau == M_), 1.0, 2.0)
    return np.sqrt(np.sum(w * C) / np.sum(w * C * np.cos(2 * np.pi * tau / M_)) - 1) / (2 * np.sin(np.pi / M_))


def effective_mass(C, tau):
    return np.arccosh((C[tau - 1] + C[tau + 1]) / (2 * C[tau]))


def creutz_22(W):
    """chi(2, 2) of W [2][3]"""
    return -np.log(W[4] * W[0] / (W[1] * W[3]))


def jackknife(m, f):
    B = len(m)
    leave = np.array([f((m.sum(axis=0) - m[b]) / (B - 1)) for b in range(B)])
    return f(m.mean(axis=0)), np.sqrt((B - 1) / B * np.sum((leave - leave.mean()) ** 2))


FUNCTIONS = {
    "xi": lambda C: xi_second_moment(C[3:], 4),
    "mass": lambda C: effective_mass(C, 2),
    "creutz": creutz_22,
    "energy": lambda C: effective_mass(C[3:], 1),
}


def test_host_arithmetic():
    lines = _run().strip().split("\n")
    assert lines[-1] == "0 failure(s)"
    checks = [line for line in lines[:-1] if not line.startswith(("estimate ", "jackknife "))]
    assert len(checks) == 11 and all(line.startswith("ok  ") for line in checks)
    # mean and chain-spread error of two entries over four chains
    m0, e0, m1, e1, spread = [line.split()[1:] for line in lines if line.startswith("estimate ")][0]
    for got_mean, got_error, chain in ((m0, e0, 0.5 + 0.1 * np.arange(4)), (m1, e1, 10.0 * np.arange(1, 5) + 1.0)):
        assert abs(float(got_mean) / chain.mean() - 1) <= 1e-15
        assert abs(float(got_error) / np.sqrt(np.sum((chain - chain.mean()) ** 2) / 12) - 1) <= 1e-15
    assert spread == "1"
    # the jackknife with each of the four functions, 1e-15 relative
    seen = {}
    for _, name, value, error, has in [line.split() for line in lines if line.startswith("jackknife ")]:
        want_value, want_error = jackknife(M, FUNCTIONS[name])
        print(name, float(value) / want_value - 1, float(error) / want_error - 1)
        assert has == "1" and abs(float(value) / want_value - 1) <= 1e-15, (name, value, want_value)
        assert abs(float(error) / want_error - 1) <= 1e-15, (name, error, want_error)
        seen[name] = float(value)
    assert set(seen) == set(FUNCTIONS) and len(set(seen.values())) == 4


def test_static_entry_points_keep_their_bits():
    with open(GOLDEN) as f:
        assert _run("statics") == f.read()
