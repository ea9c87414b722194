"""GPU: host/driver --sampler wolff --correlator 1 appends the improved estimators of the single cluster (WolffClusterSampler
with ClusterParameters::improved, ::structure and ::correlator) in the format of the Swendsen-Wang block; the lines
before it keep the format they had; the improved chi_m agrees with the plain one; without --correlator 1 nothing is added."""
import re

import pytest

from conftest import zcheck
from test_sigma_cluster_gpu import _driver

pytestmark = pytest.mark.gpu
NUM = r"([0-9.eE+-]+|nan|-nan)"
ARGS = ["--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1.0", "--sampler", "wolff", "--n_updates", "10", "--n_samples", "500"]
# the lines of the correlator block of this command before the improved estimators existed, in order
BEFORE = ([r"=== Time-slice correlator ===", rf" samples = \d+, chains = 64, errors: spread of the per-chain means"]
          + [rf" C\(tau = {tau}\): C_t = {NUM} \+/- {NUM} C_x = {NUM} \+/- {NUM} avg = {NUM} \+/- {NUM}" for tau in range(9)]
          + [rf" chi from C_t = {NUM}, from C_x = {NUM}", rf" F_t = {NUM}, F_x = {NUM}"]
          + [rf" xi_2 \({d}\) = {NUM} \+/- {NUM} \(jackknife over chains\), xi_2 / M = {NUM}" for d in "tx"])
ADDED = ([rf" improved chi_m = {NUM} \+/- {NUM}"] + [rf" improved F \({d}\) = {NUM} \+/- {NUM}" for d in "tx"]
         + [rf" improved xi_2 \({d}\) = {NUM} \+/- {NUM}, xi_2 / M = {NUM}" for d in "tx"]
         + [rf" improved C\(tau = {tau}\): improved C_t = {NUM} \+/- {NUM} improved C_x = {NUM} \+/- {NUM}" for tau in range(9)])


def test_driver_appends_the_improved_block_and_keeps_the_lines_before_it():
    r = _driver(*ARGS, "--batch", "64", "--correlator", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    start = lines.index("=== Time-slice correlator ===")
    block = lines[start:start + len(BEFORE) + len(ADDED)]
    for line, want in zip(block, BEFORE + ADDED):
        assert re.fullmatch(want, line), (line, want)
    # what comes before the block: the sampler's statistics as they were, no new line among them
    assert lines[start - 1] == "" and re.fullmatch(r"  mean cluster size        = [0-9.]+ sites", lines[start - 2]), lines[start - 3:start]
    assert lines[start - 3] == "  cluster updates per draw = 10"
    assert not any("improved" in l for l in lines[:start])
    plain = _driver(*ARGS, "--correlator", "0")                      # one chain: a single-level run without the correlator samples one
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert "improved" not in plain.stdout and "Time-slice" not in plain.stdout

    out = r.stdout
    avg = re.search(rf"Avg \+/- Err = {NUM} \+/- {NUM}", out)
    imp = re.search(rf"^ improved chi_m = {NUM} \+/- {NUM}$", out, re.M)
    assert avg and imp, out[-4000:]
    zcheck("host/driver 16x16 beta=1 wolff: improved chi_m vs plain chi_m", float(imp.group(1)), float(imp.group(2)), float(avg.group(1)),
           float(avg.group(2)), gate=5.0)
    for tau in range(9):
        p = re.search(rf"^ C\(tau = {tau}\): C_t = {NUM} \+/- {NUM} ", out, re.M)
        i = re.search(rf"^ improved C\(tau = {tau}\): improved C_t = {NUM} \+/- {NUM} ", out, re.M)
        zcheck(f"host/driver 16x16 beta=1 wolff: improved C_t({tau}) vs plain", float(i.group(1)), float(i.group(2)), float(p.group(1)),
               float(p.group(2)), gate=5.0)
