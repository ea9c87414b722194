"""GPU: host/driver --sampler swendsenwang --correlator 1 reports the cluster-improved structure factor and xi_2 of the
Swendsen-Wang sampler (SwendsenWangSampler with ClusterParameters::structure) after the time-slice correlator
block, and the improved xi_2 agrees with the plain one of the same run."""
import re

import pytest

from conftest import zcheck
from test_sigma_level_sw_gpu import _driver

pytestmark = pytest.mark.gpu
NUM = r"([0-9.eE+-]+|nan|-nan)"


def test_driver_prints_the_improved_structure_factor_and_xi_and_they_agree_with_the_plain_ones():
    r = _driver("--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.5", "--sampler", "swendsenwang", "--n_updates", "1", "--batch", "64",
                "--n_samples", "500", "--correlator", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert out.index("=== Time-slice correlator ===") < out.index(" improved F (t) = ") < out.index(" improved xi_2 (t) = ")
    for d, M in (("t", 16), ("x", 16)):
        F = re.search(rf"^ improved F \({d}\) = {NUM} \+/- {NUM}$", out, re.M)
        imp = re.search(rf"^ improved xi_2 \({d}\) = {NUM} \+/- {NUM}, xi_2 / M = {NUM}$", out, re.M)
        plain = re.search(rf"^ xi_2 \({d}\) = {NUM} \+/- {NUM} \(jackknife over chains\), xi_2 / M = {NUM}$", out, re.M)
        assert F and imp and plain, out[-3000:]
        assert float(F.group(1)) > 0 and float(F.group(2)) > 0
        xi_i, e_i, xi_p, e_p = float(imp.group(1)), float(imp.group(2)), float(plain.group(1)), float(plain.group(2))
        assert e_i > 0 and abs(float(imp.group(3)) - xi_i / M) < 1e-5
        print(f"driver 16x16 beta=1.5: xi_2({d}) improved {xi_i} +- {e_i}, plain {xi_p} +- {e_p}")
        zcheck(f"host/driver 16x16 beta=1.5 swendsenwang: improved xi_2({d}) vs plain xi_2({d})", xi_i, e_i, xi_p, e_p)


def test_driver_without_the_correlator_prints_no_improved_structure_lines():
    r = _driver("--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.5", "--sampler", "swendsenwang", "--n_updates", "1", "--n_samples", "50")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "improved chi_m" in r.stdout and "improved F" not in r.stdout and "improved xi_2" not in r.stdout
