"""CPU: the host arithmetic on a path correlator (include/mlmcpi/correlator.hh) through the stand-alone host/test_path_correlator,
and the driver's --path_correlator refusals, which come before any device call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_path_correlator")
DRIVER = os.path.join(ROOT, "host", "driver")


def _build():
    if not (os.path.exists(EXE) and os.path.exists(DRIVER)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])


def test_host_arithmetic():
    """effective_mass on the exact HO form returns omega~ to 1e-12 at every interior lag for (M, a^2 mu2) = (16, 1/16) and
    (128, 1e-3), NaN on a non-convex triple; path_correlator_ho_exact at lag 0 is the action's analytic <x^2>"""
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "0 failure(s)" and len(lines) == 9 and all(line.startswith("ok  ") for line in lines[:-1])
    assert sum("effective mass of the exact correlator" in line for line in lines) == 2
    assert sum("analytic <x^2>" in line for line in lines) == 2 and sum("NaN on a triple" in line for line in lines) == 1


QM = ["--action", "harmonicoscillator", "--M_lat", "16", "--T_final", "4", "--sampler", "exact"]
REFUSALS = [
    (["--action", "schwinger", "--sampler", "heatbath", "--path_correlator", "4"], "--path_correlator 4 is not supported for chosen action"),
    (["--action", "gff", "--sampler", "heatbath", "--path_correlator", "4"], "--path_correlator 4 is not supported for chosen action"),
    (["--action", "nonlinearsigma", "--sampler", "heatbath", "--path_correlator", "4"], "--path_correlator 4 is not supported for chosen action"),
    (QM + ["--method", "twolevel", "--path_correlator", "4"], "--path_correlator runs --method singlelevel only, not twolevel"),
    (QM + ["--method", "multilevel", "--path_correlator", "4"], "--path_correlator runs --method singlelevel only, not multilevel"),
    (QM + ["--method", "throughput", "--path_correlator", "4"], "--path_correlator runs --method singlelevel only, not throughput"),
    (QM + ["--path_correlator", "10"], "--path_correlator 10 is more than M_lat / 2 + 1 = 9 lags"),
    (QM + ["--path_correlator", "-1"], "--path_correlator takes a non-negative integer"),
    (QM + ["--path_correlator", "2.5"], "--path_correlator takes a non-negative integer"),
    (QM + ["--path_correlator", "nine"], "--path_correlator takes a non-negative integer"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_driver_refuses_by_name(args, message):
    _build()
    r = subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-2000:]
    assert "=== " not in r.stdout


def test_driver_refuses_several_ranks():
    _build()
    env = dict(os.environ, RANK="0", WORLD_SIZE="2", LOCAL_RANK="0")
    r = subprocess.run([DRIVER, *QM, "--path_correlator", "4"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "--path_correlator runs on one rank" in r.stderr, r.stderr[-2000:]
