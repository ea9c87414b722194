"""host/driver --qoi magnetic|topological: the refusals by name and the unchanged first line without the flag (CPU: they come before
any device call), and on the GPU the topological susceptibility of a heat-bath run of the 8 x 8 lattice at beta = 1.2 against the
ops-level estimate, and the two-level method on it."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "host", "driver")
SIGMA = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1.2", "--sampler", "heatbath"]
NAMED = "QoI: topological susceptibility chi_t = Q^2 / n of the geometric (Berg-Luescher) charge"
REFUSALS = [
    (["--action", "schwinger", "--sampler", "heatbath", "--qoi", "topological"], "--qoi topological is not supported for chosen action"),
    (["--action", "gff", "--sampler", "heatbath", "--qoi", "topological"], "built for nonlinearsigma only, not gff"),
    (["--action", "rotor", "--qoi", "topological"], "built for nonlinearsigma only, not rotor"),
    (["--qoi", "topological"], "built for nonlinearsigma only, not harmonicoscillator"),
    (["--action", "quarticoscillator", "--qoi", "topological"], "built for nonlinearsigma only, not quarticoscillator"),
    (SIGMA + ["--qoi", "electric"], "--qoi takes magnetic or topological, not electric"),
    (["--action", "schwinger", "--sampler", "heatbath", "--qoi", "plaquette"], "--qoi takes magnetic or topological, not plaquette"),
    (SIGMA + ["--qoi", ""], "--qoi takes magnetic or topological, not "),
]


def _build():
    if not os.path.exists(DRIVER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])


def _driver(*args, timeout=300):
    _build()
    return subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("args,message", REFUSALS)
def test_driver_refuses_by_name(args, message):
    r = _driver(*args, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-2000:]
    assert r.stdout == ""                       # before the action is built, let alone a device call


def test_without_the_flag_the_first_line_is_unchanged():
    """the line the parent printed first for this command, and nothing about the QoI unless it is asked for (with a device the run
    goes on, without one it ends at the first allocation; either way the text up to there is the same)"""
    short = ["--n_samples", "10", "--n_burnin", "2"]
    plain, named, asked = (_driver(*SIGMA, *short, *extra) for extra in ([], ["--qoi", "magnetic"], ["--qoi", "topological"]))
    first = "Action: Mt_lat = 8, Mx_lat = 8, beta = 1.200000\n"
    assert plain.stdout.startswith(first) and "QoI:" not in plain.stdout
    assert named.stdout == plain.stdout and named.returncode == plain.returncode
    assert asked.stdout.startswith(first + NAMED + "\n")


def _avg(out):
    m = re.search(r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


@pytest.mark.gpu
def test_single_level_run_names_the_qoi_and_agrees_with_ops(gpu_ops):
    import torch
    from mlmcpathintegral_amd import abi
    r = _driver(*SIGMA, "--batch", "64", "--n_samples", "200", "--qoi", "topological")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert NAMED in r.stdout and "=== Single level MC ===" in r.stdout
    avg, err = _avg(r.stdout)
    # the ops-level estimate: 1024 independent chains, 30 draws of 10 + 1 sweeps from a hot start, then 4 measured draws each;
    # the error is the spread of the per-chain means
    lv = abi.sigma_level(8, 8, 0, 1.2)
    x = gpu_ops.sigma_level_initialise(lv, 1024, 99)
    scratch, chi = torch.empty_like(x), []
    for k in range(34):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 99, 0, 11 * k)
        if k >= 30:
            chi.append(gpu_ops.sigma_level_topological_charge(lv, x)[1])
    m = torch.stack(chi).mean(dim=0).cpu().numpy()
    want, want_err = float(m.mean()), float(m.std(ddof=1) / np.sqrt(m.size))
    z = (avg - want) / np.hypot(err, want_err)
    print(f"driver chi_t = {avg} +- {err}, ops {want} +- {want_err}, z = {z:+.2f}")
    assert err > 0 and abs(z) < 5


@pytest.mark.gpu
def test_two_level_run_prints_fine_coarse_and_difference(gpu_ops):
    r = _driver(*SIGMA, "--batch", "64", "--n_samples", "200", "--qoi", "topological", "--method", "twolevel", "--coarsening", "rotate",
                "--coarsesampler", "heatbath")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for what in (NAMED, "QoI[fine]", "QoI[coarse]", "delta QoI", "=== Two level MC ==="):
        assert what in r.stdout, (what, r.stdout[-2000:])
