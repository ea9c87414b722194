"""host/driver --flow_time t [--flow_eps e], --flow_profile t0,t1,.. and --flow_scale c with --qoi topological: the refusals by
name and host/test_flow_scale (CPU: they come before any device call) and, on the GPU, --flow_time 0 against plain --qoi
topological byte for byte, the single-level run replayed through ops on the same seeds, the flowed chi_t of two-level and
hierarchical runs against independent ops estimates, and the rows and the scale of the flow profile against ops and a numpy
restatement of flow_scale."""
import os
import re
import subprocess

import numpy as np
import pytest

import sigma_flow_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "host", "driver")
FLOW_SCALE = os.path.join(ROOT, "host", "test_flow_scale")
SIGMA = ["--action", "nonlinearsigma", "--Mt_lat", "8", "--beta", "1.2", "--sampler", "heatbath"]
TOPO = SIGMA + ["--qoi", "topological"]
RUN = ["--batch", "64", "--n_samples", "200"]
TWOLEVEL = ["--method", "twolevel", "--coarsening", "rotate", "--coarsesampler", "heatbath"]
HIERARCHICAL = SIGMA[:-1] + ["hierarchical", "--qoi", "topological", "--coarsening", "rotate", "--coarsesampler", "heatbath", "--n_level", "2"]
# decorrelated proposals for the two-level step, as in tests/test_sigma_cooling_driver.py
DECORRELATED = ["--n_sweep_overrelax", "40", "--n_sweep_heatbath", "4"]
EPS, T, STEPS = 0.05, "0.25", 5
REFUSALS = [
    (["--action", "schwinger", "--sampler", "heatbath", "--flow_time", "0.5"], "--flow_time 0.5 is not supported for chosen action: the gradient flow is built for nonlinearsigma only, not schwinger"),
    (["--flow_time", "0"], "the gradient flow is built for nonlinearsigma only, not harmonicoscillator"),
    (["--action", "gff", "--sampler", "heatbath", "--flow_profile", "0,1"], "--flow_profile 0,1 is not supported for chosen action"),
    (["--action", "rotor", "--flow_eps", "0.1"], "--flow_eps 0.1 is not supported for chosen action"),
    (["--action", "rotor", "--flow_scale", "0.1"], "--flow_scale 0.1 is not supported for chosen action"),
    (SIGMA + ["--flow_time", "0.5"], "--flow_time needs --qoi topological"),
    (SIGMA + ["--qoi", "magnetic", "--flow_profile", "0,1"], "--flow_profile needs --qoi topological"),
    (TOPO + ["--flow_time", "0.5", "--n_cool", "3"], "--flow_time and --n_cool do not run together"),
    (TOPO + ["--flow_eps", "0.1"], "--flow_eps needs --flow_time t or --flow_profile"),
    (TOPO + ["--flow_scale", "0.03"], "--flow_scale needs --flow_profile"),
    (TOPO + ["--flow_time", "x"], "--flow_time takes flow times t >= 0, not x"),
    (TOPO + ["--flow_time", "-0.5"], "--flow_time takes flow times t >= 0"),
    (TOPO + ["--flow_time", "0.52"], "--flow_time 0.52 is not a whole number of steps of --flow_eps 0.05"),
    (TOPO + ["--flow_time", "0.5", "--flow_eps", "0.3"], "--flow_eps takes a step size 0 < eps <= 0.25, not 0.3"),
    (TOPO + ["--flow_time", "0.5", "--flow_eps", "0"], "--flow_eps takes a step size 0 < eps <= 0.25"),
    (TOPO + ["--flow_time", "0.5", "--flow_eps", "nan"], "--flow_eps takes a step size 0 < eps <= 0.25"),
    (TOPO + ["--flow_time", "205"], "--flow_time 205 is more than 4096 steps of --flow_eps 0.05"),
    (TOPO + TWOLEVEL + ["--flow_profile", "0,1"], "--flow_profile runs --method singlelevel only, not twolevel"),
    (TOPO + ["--method", "throughput", "--flow_profile", "0,1"], "--flow_profile runs --method singlelevel only, not throughput"),
    (TOPO + ["--flow_profile", "0,1", "--correlator", "1"], "--flow_profile and --correlator 1 do not run together"),
    (TOPO + ["--flow_profile", "0,1", "--cooling_profile", "0,1"], "--flow_profile and --cooling_profile do not run together"),
    (TOPO + ["--flow_profile", "1,1"], "--flow_profile takes strictly ascending flow times"),
    (TOPO + ["--flow_profile", "1,0.5"], "--flow_profile takes strictly ascending flow times"),
    (TOPO + ["--flow_profile", "0,,1"], "--flow_profile takes a comma-separated list of flow times"),
    (TOPO + ["--flow_profile", "a"], "--flow_profile takes a comma-separated list of flow times"),
    (TOPO + ["--flow_profile", ""], "--flow_profile takes a comma-separated list of flow times"),
    (TOPO + ["--flow_profile", "0,0.33"], "--flow_profile 0.33 is not a whole number of steps"),
    (TOPO + ["--flow_profile", ",".join("%g" % (0.05 * d) for d in range(33))], "--flow_profile takes at most 32 flow times, not 33"),
    (TOPO + ["--flow_profile", "0,1", "--flow_scale", "c"], "--flow_scale takes the value c"),
]


def _build():
    if not os.path.exists(DRIVER) or not os.path.exists(FLOW_SCALE):
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


def test_flow_scale_host_program():
    """host/test_flow_scale: the interpolation, its NaN cases, and the jackknife over three chains redone here in numpy"""
    _build()
    r = subprocess.run([FLOW_SCALE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all ok" in r.stdout and "FAIL" not in r.stdout, r.stdout
    value, error, has = re.search(r"jackknife flow_scale (\S+) (\S+) (\d)", r.stdout).groups()
    t, y = [0.0, 0.5, 1.0, 2.0], np.array([0.0, 0.02, 0.05, 0.07])
    chains = np.stack([f * y for f in (0.9, 1.0, 1.1)])
    leave = np.array([ref.flow_scale(t, np.delete(chains, b, axis=0).mean(axis=0), 0.035) for b in range(3)])
    want = np.sqrt(2.0 / 3.0 * np.sum((leave - leave.mean()) ** 2))
    assert has == "1" and float(value) == pytest.approx(ref.flow_scale(t, chains.mean(axis=0), 0.035), abs=1e-15)
    assert float(error) == pytest.approx(want, rel=1e-12)


def _avg(out, label=None):
    m = re.search((re.escape(label) + r".*?" if label else "") + r"Avg \+/- Err = ([0-9.eE+-]+) \+/- ([0-9.eE+-]+)", out, re.S)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2))


_NUM = r"([0-9.eE+-]+|nan)"
_JK = r" \+/- " + _NUM + r" \(jackknife over chains\)"


def _rows(out):
    rows = re.findall(r" t " + _NUM + r" \(step (\d+)\): chi_t = " + _NUM + _JK + r", <E> / 4 pi = " + _NUM + _JK + r", t <E> / n = " + _NUM + _JK, out)
    return {int(r[1]): tuple(float(v) for v in (r[0],) + r[2:]) for r in rows}


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], TWOLEVEL], ids=["singlelevel", "twolevel"])
def test_flow_time_zero_prints_what_the_uncooled_qoi_prints(gpu_ops, extra):
    """the flowed QoI at step 0 returns the uncooled QoI's bits: every printed digit agrees (timings aside)"""
    strip = lambda s: re.sub(r"(?i)[^\n]*(time|elapsed|seconds)[^\n]*\n", "", s)   # noqa: E731
    plain, zero = _ok(*TOPO, *RUN, *extra), _ok(*TOPO, *RUN, *extra, "--flow_time", "0")
    assert strip(zero) == strip(plain)
    assert "Gradient flow:" not in zero


def _ops_flow(gpu_ops, steps, rot=0):
    """an independent ops-level estimate on the plain (rot = 1: the rotated) 8 x 8 level at beta = 1.2: (mean, error) of chi_t
    and of E / 4 pi per step count, and the per-chain means of E / 4 pi"""
    import torch
    from mlmcpathintegral_amd import abi
    lv = abi.sigma_level(8, 8, rot, 1.2)
    x = gpu_ops.sigma_level_initialise(lv, 1024, 99 + rot)
    scratch, chi, en = torch.empty_like(x), [], []
    for k in range(34):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, 99 + rot, 0, 11 * k)
        if k >= 30:
            _, c, e = gpu_ops.sigma_level_flowed_charge(lv, x, EPS, steps, energy=True)
            chi.append(c)
            en.append(e / (4 * np.pi))
    est = lambda t: (float(t.mean()), float(t.std(ddof=1) / np.sqrt(t.size)))   # noqa: E731
    en_chain = torch.stack(en).mean(dim=0).cpu().numpy()
    return ([est(torch.stack(chi).mean(dim=0)[:, j].cpu().numpy()) for j in range(len(steps))],
            [est(en_chain[:, j]) for j in range(len(steps))], en_chain)


@pytest.mark.gpu
def test_single_level_flow_time_equals_ops_on_the_same_seeds(gpu_ops):
    """the single-level heat-bath run replayed through ops, draw by draw, as tests/test_sigma_cooling_driver.py replays --n_cool: the
    driver prints the mean over the samples to six decimals; the replay gives that number"""
    import torch
    from mlmcpathintegral_amd import abi
    seed, batch, n_burnin, n_samples = 2481317, 64, 10, 50
    out = _ok(*TOPO, "--batch", str(batch), "--n_samples", str(n_samples), "--n_burnin", str(n_burnin), "--seed", str(seed),
              "--flow_time", T, "--flow_eps", str(EPS))
    assert "Gradient flow: chi_t is read at flow time 0.25 (5 steps of 0.05)" in out
    avg, _ = _avg(out)
    lv = abi.sigma_level(8, 8, 0, 1.2)
    x = gpu_ops.sigma_level_initialise(lv, batch, seed)
    scratch, q = torch.empty_like(x), []
    for k in range(2 * n_burnin + n_samples):
        gpu_ops.sigma_level_sweep_draw(lv, x, scratch, 10, 1, seed, 0, 11 * k)
        if k >= 2 * n_burnin:
            q.append(float(gpu_ops.sigma_level_flowed_charge(lv, x, EPS, [STEPS])[1][:, 0].mean()))
    print(f"driver Avg = {avg}, replay through ops = {np.mean(q):.9f}")
    assert abs(avg - np.mean(q)) <= 0.5e-6 + 1e-12


@pytest.mark.gpu
def test_profile_rows_and_scale_against_ops(gpu_ops):
    """--flow_profile 0,0.25,1: its t = 0.25 row is the Avg of the --flow_time 0.25 run of the same seeds and its t = 0 row that of
    the unflowed run, to the digits printed; every row agrees with ops within errors; t <E> / n is t 4 pi (<E> / 4 pi) / n of the
    printed row; the scale is the numpy flow_scale of the printed rows and agrees with that of the ops estimate within errors"""
    steps, n = [0, 5, 20], 64
    ops_chi, ops_en, en_chain = _ops_flow(gpu_ops, steps)
    tE_ops = np.array([s * EPS for s in steps]) * 4 * np.pi * np.array([e[0] for e in ops_en]) / n
    c = 0.5 * (tE_ops[1] + tE_ops[2])           # a value the listed times bracket, from the independent estimate
    out = _ok(*TOPO, *RUN, "--flow_profile", "0,0.25,1", "--flow_scale", "%.6f" % c)
    assert "=== Flow profile ===" in out and "samples = 200, chains = 64" in out
    rows = _rows(out)
    assert sorted(rows) == steps, out[-2000:]
    flowed = _ok(*TOPO, *RUN, "--flow_time", T)
    for s, run in ((0, out), (STEPS, flowed)):
        avg, _ = _avg(run)
        assert abs(rows[s][1] - avg) <= 0.5e-6 + 1e-12, (s, rows[s], avg)   # Avg is printed to six decimals
    for j, s in enumerate(steps):
        t, chi, chi_err, en, en_err, te, te_err = rows[s]
        assert t == pytest.approx(s * EPS) and te == pytest.approx(t * 4 * np.pi * en / n, rel=1e-7, abs=1e-12)
        assert te_err == pytest.approx(t * 4 * np.pi * en_err / n, rel=1e-6, abs=1e-12)
        for what, got, err, (want, want_err) in (("chi_t", chi, chi_err, ops_chi[j]), ("E / 4 pi", en, en_err, ops_en[j])):
            z = (got - want) / np.hypot(err, want_err)
            print(f"t {t} {what}: driver {got} +- {err}, ops {want} +- {want_err}, z = {z:+.2f}")
            assert err > 0 and abs(z) < 5
    assert rows[0][1] > rows[5][1] > rows[20][1] and rows[0][3] > rows[5][3] > rows[20][3]
    m = re.search(r" flow scale: t <E> / n = " + _NUM + r" at t = " + _NUM + _JK, out)
    assert m, out[-1500:]
    got_c, scale, scale_err = (float(v) for v in m.groups())
    times = [rows[s][0] for s in steps]
    assert got_c == pytest.approx(c, abs=1e-6)
    assert scale == pytest.approx(ref.flow_scale(times, [rows[s][5] for s in steps], got_c), rel=1e-6)
    # the same scale from the independent ops chains, jackknifed here
    B = en_chain.shape[0]
    tE_chain = np.array(times)[None, :] * 4 * np.pi * en_chain / n
    full = ref.flow_scale(times, tE_chain.mean(axis=0), got_c)
    leave = np.array([ref.flow_scale(times, (tE_chain.sum(axis=0) - tE_chain[b]) / (B - 1), got_c) for b in range(B)])
    ops_err = np.sqrt((B - 1) / B * np.sum((leave - leave.mean()) ** 2))
    z = (scale - full) / np.hypot(scale_err, ops_err)
    print(f"flow scale at c = {got_c}: driver {scale} +- {scale_err}, ops {full} +- {ops_err}, z = {z:+.2f}")
    assert scale_err > 0 and abs(z) < 5
    nan = _ok(*TOPO, "--batch", "64", "--n_samples", "20", "--flow_profile", "0,0.25", "--flow_scale", "10")
    assert "at t = nan (the listed flow times do not bracket it)" in nan


@pytest.mark.gpu
def test_two_level_and_hierarchical_runs_flow_every_level(gpu_ops):
    """--flow_time 0.25 in --method twolevel (fine plain, coarse rotated) and --sampler hierarchical (plain over rotated): the fine
    and the coarse chi_t of the two-level run against independent ops estimates at the same flow time on the plain and on the
    ROTATED 8 x 8 level, the hierarchical run's against the plain one, each within |z| < 5 of the combined error; proposals
    decorrelated as in tests/test_sigma_cooling_driver.py"""
    two = _ok(*TOPO, *RUN, *TWOLEVEL, *DECORRELATED, "--flow_time", T)
    for what in ("Gradient flow: chi_t is read at flow time 0.25", "QoI[fine]", "QoI[coarse]", "delta QoI", "=== Two level MC ==="):
        assert what in two, (what, two[-2000:])
    plain = _ops_flow(gpu_ops, [STEPS])[0][0]
    rot = _ops_flow(gpu_ops, [STEPS], rot=1)[0][0]
    print(f"ops chi_t at t = {T}: plain {plain}, rotated {rot}")
    long_run = ["--n_samples", "6000", "--n_burnin", "200", "--n_meas", "20"]   # the hierarchical sampler runs one chain
    hier = _ok(*HIERARCHICAL, *DECORRELATED, *long_run, "--flow_time", T)
    assert "Gradient flow: chi_t is read at flow time 0.25" in hier and "=== Single level MC ===" in hier
    for name, (got, err), (want, want_err) in (("two-level fine", _avg(two, "QoI[fine]"), plain),
                                               ("two-level coarse (rotated)", _avg(two, "QoI[coarse]"), rot),
                                               ("hierarchical", _avg(hier), plain)):
        z = (got - want) / np.hypot(err, want_err)
        print(f"{name} chi_t at t = {T}: {got} +- {err}, ops {want} +- {want_err}, z = {z:+.2f}")
        assert err > 0 and abs(z) < 5, name
