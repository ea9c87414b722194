"""GPU: host/driver --sampler swendsenwang --correlator 1 prints the cluster-improved time-slice correlators of the
Swendsen-Wang sampler (SwendsenWangSampler with ClusterParameters::correlator) per lag after the improved xi_2,
they agree with the plain block of the same run within errors, and they are absent without --correlator 1."""
import re

import pytest

from conftest import zcheck
from test_sigma_level_sw_gpu import _driver

pytestmark = pytest.mark.gpu
NUM = r"([0-9.eE+-]+)"


def test_driver_prints_the_improved_correlators_after_the_improved_xi_and_they_agree_with_the_plain_block():
    r = _driver("--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.5", "--sampler", "swendsenwang", "--n_updates", "1", "--batch", "64",
                "--n_samples", "500", "--correlator", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert (out.index("=== Time-slice correlator ===") < out.index(" C(tau = 0):") < out.index(" improved F (t) = ")
            < out.index(" improved xi_2 (x) = ") < out.index(" improved C(tau = 0):"))
    for tau in range(9):
        plain = re.search(rf"^ C\(tau = {tau}\): C_t = {NUM} \+/- {NUM} C_x = {NUM} \+/- {NUM} avg = {NUM} \+/- {NUM}$", out, re.M)
        imp = re.search(rf"^ improved C\(tau = {tau}\): improved C_t = {NUM} \+/- {NUM} improved C_x = {NUM} \+/- {NUM}$", out, re.M)
        assert plain and imp, out[-4000:]
        for name, k in (("t", 1), ("x", 3)):
            v_i, e_i, v_p, e_p = float(imp.group(k)), float(imp.group(k + 1)), float(plain.group(k)), float(plain.group(k + 1))
            assert v_i > 0 and e_i > 0
            # the plain block measures the states AFTER each draw, the improved one the field BEFORE each update: the same law
            zcheck(f"host/driver 16x16 beta=1.5 swendsenwang: improved C_{name}({tau}) vs plain", v_i, e_i, v_p, e_p, gate=4.5)
    assert " improved C(tau = 9):" not in out


def test_driver_without_the_correlator_prints_no_improved_correlator_lines():
    r = _driver("--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.5", "--sampler", "swendsenwang", "--n_updates", "1", "--n_samples", "50")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "improved chi_m" in r.stdout and "improved C" not in r.stdout
