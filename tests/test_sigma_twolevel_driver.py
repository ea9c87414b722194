"""host/driver for the O(3) sigma model's two-level method and hierarchical sampler (--coarsening rotate): both run, the
hierarchical chain's chi_m agrees with the heat-bath sampler's, and what stays refused is refused by name."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "driver")
COMMON = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1"]
# the two-level step is exact for proposals independent of the current state; successive states of the coarse chain are not, and
# with one 10 + 1 draw between proposals chi_m sits 2.6 % high at this shape.  Forty overrelaxation and four
# heat-bath sweeps per coarse draw decorrelate the proposals, as the four 10 + 1 draws of tests/test_sigma_twolevel_gpu.py do.
COARSE = ["--coarsening", "rotate", "--coarsesampler", "heatbath"]
DECORRELATED = ["--n_sweep_overrelax", "40", "--n_sweep_heatbath", "4"]


def _driver(*args, timeout=600):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _avg(out):
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


@pytest.mark.gpu
def test_twolevel_method_runs_and_reports_both_levels():
    r = _driver(*COMMON, *COARSE, "--sampler", "heatbath", "--method", "twolevel", "--n_samples", "300", "--n_burnin", "50", "--n_meas", "20")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for what in ("QoI[fine]", "QoI[coarse]", "delta QoI", "Two level sampler statistics", "acceptance probability"):
        assert what in r.stdout, (what, r.stdout[-2000:])
    rate = float(re.findall(r"acceptance probability\s+p = ([0-9.]+)", r.stdout)[-1])
    print("two-level acceptance rate", rate)
    assert 0.0 < rate < 1.0


@pytest.mark.gpu
def test_hierarchical_sampler_agrees_with_the_heat_bath():
    h = _driver(*COMMON, *COARSE, *DECORRELATED, "--sampler", "hierarchical", "--n_level", "2", "--n_samples", "6000", "--n_burnin", "200",
                "--n_meas", "20")
    assert h.returncode == 0, h.stdout[-2000:] + h.stderr[-2000:]
    s = _driver(*COMMON, "--sampler", "heatbath", "--n_samples", "4000", "--n_burnin", "100")
    assert s.returncode == 0, s.stdout[-2000:] + s.stderr[-2000:]
    (ha, he), (sa, se) = _avg(h.stdout), _avg(s.stdout)
    print(f"chi_m hierarchical {ha} +- {he}, heat bath {sa} +- {se}, z = {(ha - sa) / (he * he + se * se) ** 0.5:+.2f}")
    assert abs(ha - sa) < 3 * (he * he + se * se) ** 0.5
    # three levels: 8 x 8, rotated 8 x 8, 4 x 4
    k = _driver(*COMMON, *COARSE, "--sampler", "hierarchical", "--n_level", "3", "--n_samples", "200", "--n_burnin", "20", "--n_meas", "10")
    assert k.returncode == 0, k.stdout[-2000:] + k.stderr[-2000:]
    assert "level 2" in k.stdout


@pytest.mark.parametrize("extra,why", [
    (["--method", "twolevel"], "coarsens by rotate only"),                                   # the default coarsening, both
    (["--method", "twolevel", "--coarsening", "temporal", "--coarsesampler", "heatbath"], "coarsens by rotate only"),
    (["--sampler", "hierarchical", "--coarsening", "alternate", "--coarsesampler", "heatbath"], "coarsens by rotate only"),
    (["--method", "multilevel", "--coarsening", "rotate", "--coarsesampler", "heatbath"], "--method multilevel is not supported"),
    (["--method", "multilevel"], "--method multilevel is not supported"),
    (["--method", "twolevel", "--coarsening", "rotate"], "--coarsesampler heatbath only"),    # the default coarse sampler, hmc
    (["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "wolff"], "--coarsesampler wolff is not supported"),
    (["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "swendsenwang"], "--coarsesampler swendsenwang is not supported"),
    (["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--sampler", "wolff"], "singlelevel only"),
    (["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--sampler", "swendsenwang"], "singlelevel only"),
    (["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--renormalisation", "exact"], "non-perturbative")])
def test_refusals_name_the_action_and_the_method(extra, why):
    args = list(COMMON)
    if "--sampler" not in extra:
        args += ["--sampler", "heatbath"]
    r = _driver(*args, *extra, timeout=120)
    out = r.stderr + r.stdout
    assert r.returncode != 0, out[-1500:]
    assert "nonlinearsigma" in out or "nonlinear sigma" in out, out[-1500:]
    assert why in out, out[-1500:]
