"""host/driver --action nonlinearsigma: the C++ layer's NonlinearSigmaAction and QoI2DMagneticSusceptibility through the
reference's single-level loop and through the throughput loop, and the methods / samplers it refuses."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "driver")
COMMON = ["--action", "nonlinearsigma", "--Mt_lat", "16", "--beta", "1", "--sampler", "heatbath"]


def _driver(*args, timeout=600):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("extra,what", [(["--sampler", "hmc"], "sin theta"), (["--method", "twolevel"], "twolevel"),
                                        (["--method", "multilevel"], "multilevel")])
def test_driver_refuses_what_the_sigma_model_does_not_support(extra, what):
    r = _driver(*COMMON, *extra, timeout=120)
    assert r.returncode != 0
    assert "nonlinearsigma" in r.stderr + r.stdout and what in r.stderr + r.stdout


@pytest.mark.gpu
def test_driver_singlelevel_and_throughput_agree():
    r = _driver(*COMMON, "--n_samples", "4000", "--n_burnin", "100")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    avg, err = float(m.group(1)), float(m.group(2))
    print("singlelevel chi_m =", avg, "+-", err)
    t = _driver(*COMMON, "--method", "throughput", "--batch", "64", "--n_samples", "200", "--warmup", "50")
    assert t.returncode == 0, t.stdout[-2000:] + t.stderr[-2000:]
    line = json.loads([l for l in t.stdout.splitlines() if l.startswith("{")][-1])
    print(line)
    assert line["batch"] == 64 and line["samples"] == 200
    # N vertex updates per sweep, 11 sweeps per sample
    assert line["updates_per_s"] > 0
    assert abs(line["qoi_mean"] - avg) < 3 * err, (line["qoi_mean"], avg, err)
