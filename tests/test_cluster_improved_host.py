"""CPU: ClusterImprovedSums (include/mlmcpi/cluster_improved.hh) alone, through the stand-alone host/test_cluster_improved: its
output against tests/golden/cluster_improved_sums.txt character for character (the class as it was inside sampler.hh), the chain
spread and the xi jackknife against numpy, one chain without an error, and the texts of its fatal messages."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_cluster_improved")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_improved_sums.txt")

# the level and the draws of host/test_cluster_improved.cc
MT, MX, N_OUT, N_UPDATES, N_DRAWS = 8, 6, 9, 2, 3
C_BASE = [1.0, 0.6, 0.4, 0.3, 0.28, 1.0, 0.55, 0.35, 0.3]
F_BASE = [1.1, 0.9]


def _run(*args):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), EXE])
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def output():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _lines(output, kind, B, config):
    """the numbers after `kind B config` of every such line, hexadecimal floats read exactly"""
    rows = [line.split()[3:] for line in output.splitlines() if line.split()[:3] == [kind, str(B), config]]
    return [[float.fromhex(v) if v.startswith(("0x", "-0x")) else int(v) for v in row] for row in rows]


def chain_sums(B):
    """per-chain sums over the draws of imp [B], F [B][2], C [B][n_out]: the generator and the order of the program"""
    state = 2481317
    imp, F, C = np.zeros(B), np.zeros((B, 2)), np.zeros((B, N_OUT))

    def nxt(base):
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        return N_UPDATES * base * (0.9 + 0.2 * ((state >> 11) * 2.0 ** -53))

    for _ in range(N_DRAWS):
        for b in range(B):
            imp[b] += nxt(3.9)
            for d in range(2):
                F[b, d] += nxt(F_BASE[d])
            for k in range(N_OUT):
                C[b, k] += nxt(C_BASE[k])
    return imp, F, C


def spread(per_chain):
    """mean over the chains of the per-chain means and their spread over sqrt(B)"""
    B = len(per_chain)
    return per_chain.mean(axis=0), np.sqrt(np.sum((per_chain - per_chain.mean(axis=0)) ** 2, axis=0) / (B * (B - 1)))


def xi_2(chi, F, M):
    return np.sqrt(chi / F - 1) / (2 * np.sin(np.pi / M))


def test_output_keeps_its_bits(output):
    with open(GOLDEN) as f:
        assert output == f.read()


@pytest.mark.parametrize("B", [2, 5])
def test_chain_spread_against_numpy(output, B):
    _, F, C = chain_sums(B)
    n = N_DRAWS * N_UPDATES
    worst = 0.0
    want_mean, want_error = spread(F / n)
    for d, value, error, has_error in _lines(output, "structure", B, "structure"):
        worst = max(worst, abs(value / want_mean[d] - 1), abs(error / want_error[d] - 1))
        assert has_error == 1
    want_mean, want_error = spread(C / n)
    rows = _lines(output, "correlator", B, "correlator")
    assert len(rows) == N_OUT
    for k, value, error, chain_spread in rows:
        worst = max(worst, abs(value / want_mean[k] - 1), abs(error / want_error[k] - 1))
        assert chain_spread == 1
    print("chain spread, B =", B, ": worst relative deviation from numpy", worst)
    assert worst <= 1e-15


@pytest.mark.parametrize("B", [2, 5])
def test_xi_jackknife_against_numpy(output, B):
    chi, F, _ = chain_sums(B)
    worst = 0.0
    rows = _lines(output, "xi", B, "structure")
    assert len(rows) == 2
    for d, value, error, has_error in rows:
        M = (MT, MX)[d]
        leave = np.array([xi_2((chi.sum() - chi[b]) / (B - 1), (F[:, d].sum() - F[b, d]) / (B - 1), M) for b in range(B)])
        want_value = xi_2(chi.sum() / B, F[:, d].sum() / B, M)
        want_error = np.sqrt((B - 1) / B * np.sum((leave - leave.mean()) ** 2))
        worst = max(worst, abs(value / want_value - 1), abs(error / want_error - 1))
        assert has_error == 1 and np.isfinite(value) and error > 0
    print("xi jackknife, B =", B, ": worst relative deviation from numpy", worst)
    assert worst <= 1e-15


def test_one_chain_has_no_error(output):
    for config in ("structure", "both", "both_given_F"):
        rows = _lines(output, "structure", 1, config) + _lines(output, "xi", 1, config)
        assert len(rows) == 4
        for d, value, error, has_error in rows:
            assert has_error == 0 and error == 0.0 and np.isfinite(value)
    for config in ("correlator", "both", "both_given_F"):
        rows = _lines(output, "correlator", 1, config)
        assert len(rows) == N_OUT
        for k, value, error, chain_spread in rows:
            assert chain_spread == 0 and error == 0.0


def test_F_formed_from_C_is_the_structure_factor_of_C(output):
    """with both options and no F handed in, F_d of a draw is structure_factor() of the draw's C_d, which is linear in C: the
    chain-averaged F_d is that function of the chain-averaged correlator"""
    for B in (1, 2, 5):
        C = np.array([row[1] for row in _lines(output, "correlator", B, "both")])
        for d, value, error, has_error in _lines(output, "structure", B, "both"):
            M, c = ((MT, C[:MT // 2 + 1]), (MX, C[MT // 2 + 1:]))[d]
            tau = np.arange(M // 2 + 1)
            w = np.where((tau == 0) | (2 * tau == M), 1.0, 2.0)
            assert abs(value / np.sum(w * c * np.cos(2 * np.pi * tau / M)) - 1) <= 1e-14


@pytest.mark.parametrize("what,why,text", [
    ("correlator", "without", "ERROR: TestSampler::improved_correlator: constructed without ClusterParameters::correlator."),
    ("correlator", "nodraws", "ERROR: TestSampler::improved_correlator: no draws since reset_improved()."),
    ("structure_factor", "without", "ERROR: TestSampler::improved_structure_factor: constructed without ClusterParameters::structure."),
    ("structure_factor", "nodraws", "ERROR: TestSampler::improved_structure_factor: no draws since reset_improved()."),
    ("xi", "without", "ERROR: TestSampler::improved_xi: constructed without ClusterParameters::structure."),
    ("xi", "nodraws", "ERROR: TestSampler::improved_xi: no draws since reset_improved()."),
])
def test_fatal_messages_keep_their_text(what, why, text):
    r = _run("fatal", what, why)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == text + "\n"
