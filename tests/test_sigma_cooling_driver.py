"""host/driver --n_cool k and --cooling_profile d0,d1,.. with --qoi topological: the refusals by name (CPU: they come before any
device call) and, on the GPU, --n_cool 0 against plain --qoi topological byte for byte, the cooled chi_t of single-level, two-level
and hierarchical runs, and the rows of the cooling profile against the --n_cool runs of the same seeds and against ops."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "host", "driver")
SIGMA = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1.2", "--sampler", "heatbath"]
TOPO = SIGMA + ["--qoi", "topological"]
RUN = ["--batch", "64", "--n_samples", "200"]
TWOLEVEL = ["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "heatbath"]
HIERARCHICAL = SIGMA[:-1] + ["hierarchical", "--qoi", "topological", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--n_level", "2"]
# the two-level step is exact for proposals independent of the current state; forty overrelaxation and four heat-bath sweeps per
# coarse draw decorrelate them, as in tests/test_sigma_twolevel_driver.py
DECORRELATED = ["--n_sweep_overrelax", "40", "--n_sweep_heatbath", "4"]
REFUSALS = [
    (["--action", "schwinger", "--sampler", "heatbath", "--n_cool", "3"], "--n_cool 3 is not supported for chosen action: cooling is built for nonlinearsigma only, not schwinger"),
    (["--n_cool", "0"], "cooling is built for nonlinearsigma only, not harmonicoscillator"),
    (["--action", "gff", "--sampler", "heatbath", "--cooling_profile", "0,1"], "--cooling_profile 0,1 is not supported for chosen action"),
    (SIGMA + ["--n_cool", "3"], "--n_cool needs --qoi topological"),
    (SIGMA + ["--qoi", "magnetic", "--cooling_profile", "0,1"], "--cooling_profile needs --qoi topological"),
    (TOPO + ["--n_cool", "x"], "--n_cool takes a non-negative integer"),
    (TOPO + ["--n_cool", "4097"], "--n_cool 4097 is more than 4096 cooling sweeps"),
    (TOPO + TWOLEVEL + ["--cooling_profile", "0,1"], "--cooling_profile runs --method singlelevel only, not twolevel"),
    (TOPO + ["--method", "throughput", "--cooling_profile", "0,1"], "--cooling_profile runs --method singlelevel only, not throughput"),
    (TOPO + ["--cooling_profile", "0,1", "--correlator", "1"], "--cooling_profile and --correlator 1 do not run together"),
    (TOPO + ["--cooling_profile", "1,1"], "--cooling_profile takes strictly ascending depths"),
    (TOPO + ["--cooling_profile", "3,1"], "--cooling_profile takes strictly ascending depths"),
    (TOPO + ["--cooling_profile", "0,,1"], "--cooling_profile takes a comma-separated list of depths"),
    (TOPO + ["--cooling_profile", "a"], "--cooling_profile takes a comma-separated list of depths"),
    (TOPO + ["--cooling_profile", ""], "--cooling_profile takes a comma-separated list of depths"),
    (TOPO + ["--cooling_profile", "0,4097"], "--cooling_profile takes depths up to 4096, not 4097"),
    (TOPO + ["--cooling_profile", ",".join(str(d) for d in range(33))], "--cooling_profile takes at most 32 depths, not 33"),
]


def _build():
    if not os.path.exists(DRIVER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])


def _driver(*args, timeout=300):
    _build()
    return subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=timeout)


def _ok(*args):
    r = _driver(*args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("args,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_driver_refuses_by_name(args, message):
    r = _driver(*args, timeout=120)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-2000:]
    assert r.stdout == ""                       # before the action is built, let alone a device call


def _avg(out, label=None):
    m = re.search((re.escape(label) + r".*?" if label else "") + r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out, re.S)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


def _rows(out):
    rows = re.findall(r" depth (\d+): chi_t = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+) \(jackknife over chains\), <E> / 4 pi = ([0-9.eE+-]+) "
                      r"\+/- ([0-9.eE+-]+) \(jackknife over chains\)", out)
    return {int(r[0]): tuple(float(v) for v in r[1:]) for r in rows}


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], TWOLEVEL], ids=["singlelevel", "twolevel"])
def test_n_cool_zero_prints_what_the_uncooled_qoi_prints(gpu_ops, extra):
    """the cooled QoI at depth 0 returns the uncooled QoI's bits: every printed digit agrees (timings aside)"""
    strip = lambda s: re.sub(r"(?i)[^\n]*(time|elapsed|seconds)[^\n]*\n", "", s)   # noqa: E731
    plain, zero = _ok(*TOPO, *RUN, *extra), _ok(*TOPO, *RUN, *extra, "--n_cool", "0")
    assert strip(zero) == strip(plain)
    assert "Cooling:" not in zero


def _ops_chi(gpu_ops, depths, rot=0):
    """the ops-level estimate of test_sigma_topology_driver.py on the plain (rot = 1: the rotated) 8 x 8 level, at the depths:
    (mean, error) of chi_t and of E / 4 pi per depth"""
    import torch
    from mlmcpathintegral_amd import abi
    lv = abi.sigma_level(8, 8, rot, 1.2)
    x = gpu_ops.sigma_level_initialise(lv, 1024, 99 + rot)
    scratch, chi, en = torch.empty_like(x), [], []
    for k in range(34):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 99 + rot, 0, 11 * k)
        if k >= 30:
            _, c, e = gpu_ops.sigma_level_cooled_charge(lv, x, depths, energy=True)
            chi.append(c)
            en.append(e / (4 * np.pi))
    est = lambda t: (float(t.mean()), float(t.std(ddof=1) / np.sqrt(t.size)))   # noqa: E731
    return ([est(torch.stack(chi).mean(dim=0)[:, j].cpu().numpy()) for j in range(len(depths))],
            [est(torch.stack(en).mean(dim=0)[:, j].cpu().numpy()) for j in range(len(depths))])


@pytest.mark.gpu
def test_single_level_n_cool_equals_ops_on_the_same_seeds(gpu_ops):
    """the single-level heat-bath run replayed through ops, draw by draw: the Philox streams are functions of (seed, chain, sweep),
    the sampler burns in --n_burnin draws, the loop another --n_burnin, then every draw is a sample whose Q is the mean of chi_3 over
    the chains.  The driver prints the mean over the samples to six decimals; the replay gives that number."""
    import torch
    from mlmcpathintegral_amd import abi
    seed, batch, n_burnin, n_samples = 2481317, 64, 10, 50
    out = _ok(*TOPO, "--batch", str(batch), "--n_samples", str(n_samples), "--n_burnin", str(n_burnin), "--seed", str(seed), "--n_cool", "3")
    avg, _ = _avg(out)
    lv = abi.sigma_level(8, 8, 0, 1.2)
    x = gpu_ops.sigma_level_initialise(lv, batch, seed)
    scratch, q = torch.empty_like(x), []
    for k in range(2 * n_burnin + n_samples):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, seed, 0, 11 * k)
        if k >= 2 * n_burnin:
            q.append(float(gpu_ops.sigma_level_cooled_charge(lv, x, [3])[1][:, 0].mean()))
    print(f"driver Avg = {avg}, replay through ops = {np.mean(q):.9f}")
    assert abs(avg - np.mean(q)) <= 0.5e-6 + 1e-12


@pytest.mark.gpu
def test_profile_rows_against_the_n_cool_runs_and_ops(gpu_ops):
    """--cooling_profile 0,1,3 measures the states the QoI is read from: its depth-3 row is the Avg of the --n_cool 3 run of the same
    seeds and its depth-0 row that of the uncooled run, to the digits printed; every row agrees with ops within errors"""
    out = _ok(*TOPO, *RUN, "--cooling_profile", "0,1,3")
    assert "=== Cooling profile ===" in out and "samples = 200, chains = 64" in out
    rows = _rows(out)
    assert sorted(rows) == [0, 1, 3], out[-2000:]
    cooled = _ok(*TOPO, *RUN, "--n_cool", "3")
    assert "Cooling: chi_t is read after 3 cooling sweeps" in cooled
    for depth, run in ((0, out), (3, cooled)):
        avg, _ = _avg(run)
        assert abs(rows[depth][0] - avg) <= 0.5e-6 + 1e-12, (depth, rows[depth], avg)   # Avg is printed to six decimals
    chi, en = _ops_chi(gpu_ops, [0, 1, 3])
    for j, d in enumerate([0, 1, 3]):
        for what, got, err, (want, want_err) in (("chi_t", rows[d][0], rows[d][1], chi[j]), ("E / 4 pi", rows[d][2], rows[d][3], en[j])):
            z = (got - want) / np.hypot(err, want_err)
            print(f"depth {d} {what}: driver {got} +- {err}, ops {want} +- {want_err}, z = {z:+.2f}")
            assert err > 0 and abs(z) < 5
    assert rows[0][0] > rows[1][0] > rows[3][0] and rows[0][2] > rows[1][2] > rows[3][2]


@pytest.mark.gpu
def test_two_level_and_hierarchical_runs_cool_every_level(gpu_ops):
    """--n_cool 3 in --method twolevel (fine plain, coarse rotated) and --sampler hierarchical (plain over rotated).  These
    two samplers are not replayed draw by draw: in place of the equality on the same seeds that the single-level test makes, the
    fine chi_3 and the coarse chi_3 of the two-level run are held to independent ops estimates of chi_3 on the plain and on the
    ROTATED 8 x 8 level at the same beta (--renormalisation none), and the hierarchical run's chi_3 to the plain one, each within
    |z| < 5 of the combined error.  Both runs take decorrelated proposals (DECORRELATED): with one 10 + 1 draw per proposal the
    two-level chain itself sits low (uncooled fine chi_t 0.0063 against 0.0073), cooling or not.  At this shape chi_0 = 0.0073,
    chi_1 = 0.0018, chi_3 = 0.0006 on the plain level and chi_3 = 0.00004 on the rotated one, so a wrong depth or a wrong
    rotated flag in a level's QoI misses the two-level gates by ten sigma and more, the one-chain hierarchical gate by about five."""
    two = _ok(*TOPO, *RUN, *TWOLEVEL, *DECORRELATED, "--n_cool", "3")
    for what in ("Cooling: chi_t is read after 3 cooling sweeps", "QoI[fine]", "QoI[coarse]", "delta QoI", "=== Two level MC ==="):
        assert what in two, (what, two[-2000:])
    (_, _, plain3), _ = _ops_chi(gpu_ops, [0, 1, 3])
    (_, _, rot3), _ = _ops_chi(gpu_ops, [0, 1, 3], rot=1)
    print(f"ops chi_3: plain {plain3}, rotated {rot3}")
    long_run = ["--n_samples", "6000", "--n_burnin", "200", "--n_meas", "20"]   # the hierarchical sampler runs one chain
    hier = _ok(*HIERARCHICAL, *DECORRELATED, *long_run, "--n_cool", "3")
    assert "Cooling: chi_t is read after 3 cooling sweeps" in hier and "=== Single level MC ===" in hier
    for name, (got, err), (want, want_err) in (("two-level fine", _avg(two, "QoI[fine]"), plain3),
                                               ("two-level coarse (rotated)", _avg(two, "QoI[coarse]"), rot3),
                                               ("hierarchical", _avg(hier), plain3)):
        z = (got - want) / np.hypot(err, want_err)
        print(f"{name} chi_t after 3 sweeps: {got} +- {err}, ops {want} +- {want_err}, z = {z:+.2f}")
        assert err > 0 and abs(z) < 5, name
