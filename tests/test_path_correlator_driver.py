"""GPU: host/driver --path_correlator on the harmonic oscillator with the exact sampler: the printed C(tau) against the printed
exact column, the effective mass against the exact lattice gap, and the output without the option."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "host", "driver")
ARGS = ["--action", "harmonicoscillator", "--M_lat", "16", "--T_final", "4", "--sampler", "exact", "--batch", "256", "--n_samples", "200"]
NUM = r"(-?[0-9.]+(?:e[-+]?[0-9]+)?|-?nan)"


def _run(extra):
    if not os.path.exists(DRIVER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    r = subprocess.run([DRIVER, *ARGS, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_block_against_the_exact_columns(gpu_ops):
    out = _run(["--path_correlator", "9"])
    print(out)
    block = out.split("=== Path correlator ===")
    assert len(block) == 2 and "=== Single level MC ===" in block[0]
    assert "samples = 200, chains = 256, errors: spread of the per-chain means" in block[1]
    C = re.findall(r" C\(tau = (\d+)\) = %s \+/- %s exact = %s" % (NUM, NUM, NUM), block[1])
    assert [int(c[0]) for c in C] == list(range(9))
    for tau, mean, err, exact in C:
        z = (float(mean) - float(exact)) / float(err)
        print(f"C({tau}): z = {z:+.2f}")
        assert float(err) > 0 and abs(z) < 4.5, (tau, mean, err, exact)
    m = re.findall(r" m_eff\(tau = (\d+)\) = %s \+/- %s \(jackknife over chains\), Delta E = m_eff / a = %s" % (NUM, NUM, NUM), block[1])
    assert [int(x[0]) for x in m] == list(range(1, 8))
    w, gap = map(float, re.search(r" exact lattice gap: omega~ = %s, omega~ / a = %s" % (NUM, NUM), block[1]).groups())
    assert abs(w - 0.249353) < 1e-5 and abs(gap - 4 * w) < 1e-6      # acosh(1 + 1/32), a = 1/4
    value, err, de = (float(v) for v in m[3][1:])
    assert int(m[3][0]) == 4 and err > 0 and abs(value - w) < 4.5 * err, (value, err, w)
    assert abs(de - 4 * value) < 1e-6


def test_without_the_option_the_output_is_todays(gpu_ops):
    plain, zero = _run([]), _run(["--path_correlator", "0"])
    for out in (plain, zero):
        assert "Path correlator" not in out and "m_eff" not in out
        lines = out.strip().split("\n")
        assert lines[0].startswith("Action: M_lat = 16, T_final = 4") and "=== Single level MC ===" in lines
        assert lines[-2].startswith(" analytic result = ") and lines[-1].startswith(" |analytic - numerical| / error = ")
    assert plain == zero
