"""GPU: device results do not depend on the stream or on the host thread that issues the calls.

Every entry point of include/mlmcpi_hip.h takes a stream, PathMLMC.pass_ runs every level on a stream of its own, and
runtime.hip keeps one scratch buffer per (host thread, device, stream).  The jobs of tests/stream_cases.py are short call
sequences through every `scratch(...)` call site, every asynchronous memset / copy inside a draw and every process-wide cache
of the library.  Each test runs them on side streams (alone, against a copy of themselves, against another job, under a long
kernel, around a growing scratch buffer, from two host threads, as the first calls of a fresh process) and requires every
output tensor to equal, bit for bit (torch.equal: the arithmetic and the launch plan are the same on any stream, so there is
no tolerance), what the same calls give one after another on the default stream.

Two side streams, never more.  Tests 2 to 4 print whether the two streams' intervals (an event before a job's first call and one
behind its last, against one base event) intersected: evidence that the comparison was made under concurrency, not a gate -- the hardware promises no overlap.
"""
import os
import subprocess
import sys
import threading

import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n, _ in sc.JOBS]
SHIFT = 1000   # chain0 of the second copy of a job

_serial = {}     # (job name, shift) -> outputs on the default stream: computed once, never changed
_side = []       # the two side streams, shared by all tests


def serial(ops, name, shift=0, **kw):
    key = (name, shift, tuple(sorted(kw.items())))
    if key not in _serial:
        fn = sc.filler if name == "filler" else sc.scratch_growth if name == "scratch_growth" else sc.JOB[name]
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        _serial[key] = sc.run_serial(fn(ops, shift, **kw))
        torch.cuda.synchronize()
    return _serial[key]


def side_streams():
    if not _side:
        _side.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _side


def bits_equal(a, b):
    """torch.equal on the bytes: NaN equals NaN of the same bits, and -0.0 differs from 0.0"""
    return torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def assert_same(got, want, what):
    assert got is not None and sorted(got) == sorted(want), (what, sorted(got or ()), sorted(want))
    for k in sorted(want):
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if not bits_equal(a, b):
            bad = (a != b)
            raise AssertionError(f"{what}: output '{k}' differs from the default-stream result in {int(bad.sum())} of {bad.numel()} "
                                 f"entries, the first at {bad.nonzero()[0].tolist()}")


def report(what, backend):
    (a0, a1), (b0, b1) = backend.intervals()
    yes = sc.intervals_overlap((a0, a1), (b0, b1))
    print(f"[overlap] {what}: stream 1 [{a0:.3f}, {a1:.3f}] ms, stream 2 [{b0:.3f}, {b1:.3f}] ms, overlap: {'yes' if yes else 'no'}")
    return yes


# ---- 1. a side stream alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_side_stream_alone(gpu_ops, name):
    """catches a launch or an asynchronous copy that ignores `stream`: nothing orders the default stream behind the side one"""
    want = serial(gpu_ops, name)
    s1 = side_streams()[0]
    got, = sc.run_interleaved([sc.JOB[name](gpu_ops, 0)], [s1])
    torch.cuda.synchronize()
    assert_same(got, want, f"{name} on a side stream")


# ---- 2. the same job twice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_same_job_twice_interleaved(gpu_ops, name):
    """the same kernels and the same scratch size on both streams: the worst case for a work buffer shared behind the API"""
    want = [serial(gpu_ops, name), serial(gpu_ops, name, SHIFT)]
    backend = sc.TorchStreams()
    got = sc.run_interleaved([sc.JOB[name](gpu_ops, 0), sc.JOB[name](gpu_ops, SHIFT)], side_streams(), backend=backend)
    report(f"{name} x 2", backend)
    for g, w, c0 in zip(got, want, (0, SHIFT)):
        assert_same(g, w, f"{name} (chain0 + {c0}) beside its copy")


# ---- 3. a job against its neighbour -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_job_against_its_neighbour(gpu_ops, i):
    a, b = NAMES[i], NAMES[(i + 1) % len(NAMES)]
    want = [serial(gpu_ops, a), serial(gpu_ops, b)]
    backend = sc.TorchStreams()
    got = sc.run_interleaved([sc.JOB[a](gpu_ops, 0), sc.JOB[b](gpu_ops, 0)], side_streams(), backend=backend)
    report(f"{a} | {b}", backend)
    assert_same(got[0], want[0], f"{a} beside {b}")
    assert_same(got[1], want[1], f"{b} beside {a}")


# ---- 4. a job under the filler ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_job_under_the_filler(gpu_ops, name):
    """the filler (one path_hmc_run launch, stream_cases.FILLER_DRAWS draws) goes to stream 2 first, then the job to stream 1.
    The line printed gives both intervals; FILLER_DRAWS was grown until the filler's interval held the partner's for the
    jobs whose calls do not wait for the device."""
    want = [serial(gpu_ops, "filler"), serial(gpu_ops, name)]
    s1, s2 = side_streams()
    backend = sc.TorchStreams()
    got = sc.run_interleaved([sc.filler(gpu_ops, 0), sc.JOB[name](gpu_ops, 0)], [s2, s1], backend=backend)
    (f0, f1), (j0, j1) = backend.intervals()
    print(f"[overlap] filler | {name}: filler [{f0:.3f}, {f1:.3f}] ms, job [{j0:.3f}, {j1:.3f}] ms, overlap: "
          f"{'yes' if sc.intervals_overlap((f0, f1), (j0, j1)) else 'no'}, job inside the filler: {'yes' if f0 <= j0 and j1 <= f1 else 'no'}")
    assert_same(got[0], want[0], f"the filler beside {name}")
    assert_same(got[1], want[1], f"{name} under the filler")


# ---- 5. scratch growth under load -------------------------------------------------------------------------------------------
def test_scratch_growth_under_load(gpu_ops):
    """stream 1: a request the slot's first 1 MiB serves, one beyond it, the small one again (stream_cases.scratch_growth: the
    large one is mlmcpi_lattice_random_sweep_order on Schwinger 64 x 64, B = 64, which asks for 16 bytes per link and chain,
    8 MiB, plus its workspace: random_sweep.hip, `scratch(16 * total + work + cub, ...)`; the 1 MiB floor is runtime.hip's
    `want`).  The stream is a fresh one, so that its slot starts empty whatever ran before.  Stream 2 runs the Schwinger
    closed-form job meanwhile."""
    assert sc.scratch_growth_bytes() > (1 << 20)
    want = [serial(gpu_ops, "scratch_growth"), serial(gpu_ops, "schwinger_closed_form")]
    fresh, other = torch.cuda.Stream(), side_streams()[1]
    backend = sc.TorchStreams()
    got = sc.run_interleaved([sc.scratch_growth(gpu_ops, 0), sc.JOB["schwinger_closed_form"](gpu_ops, 0)], [fresh, other], backend=backend)
    report("scratch growth | schwinger_closed_form", backend)
    assert_same(got[0], want[0], "scratch growth")
    assert_same(got[1], want[1], "schwinger_closed_form beside a growing scratch buffer")


# ---- 6. two host threads ----------------------------------------------------------------------------------------------------
def test_two_host_threads(gpu_ops):
    """each thread has its own stream and its own scratch pool (thread_local) and runs half of the job list; the library is a
    ctypes.CDLL, so its calls release the GIL"""
    want = {n: serial(gpu_ops, n) for n in NAMES}
    halves = [NAMES[0::2], NAMES[1::2]]
    barrier = threading.Barrier(2)
    got, errors = {}, []

    def work(names):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            barrier.wait(timeout=60)
            with torch.cuda.stream(st):
                for n in names:
                    got[n] = sc.run_serial(sc.JOB[n](gpu_ops, 0))
            st.synchronize()
        except BaseException as e:   # reaches the test below
            errors.append((names, e))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(h,)) for h in halves]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    assert sorted(got) == sorted(NAMES)
    for n in NAMES:
        assert_same(got[n], want[n], f"{n} from a second host thread")


# ---- 7. first use from two threads, in a fresh process -------------------------------------------------------------------------
digests = sc.digests


_CHILD = r"""
import sys, threading
sys.path[:0] = [%r, %r]
import torch
import stream_cases as sc
from mlmcpathintegral_amd import abi, ops
digests = sc.digests
abi.load()
torch.cuda.set_device(0)
torch.cuda.init()
barrier, out, errors = threading.Barrier(2), {}, []
def work(k):
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            barrier.wait(timeout=60)      # the library's first calls: both threads at once
            for name in ("schwinger_closed_form", "sigma_sw"):
                out[k, name] = sc.run_serial(sc.JOB[name](ops, 0))
        st.synchronize()
    except BaseException as e:
        errors.append(e)
        barrier.abort()
threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
for t in threads: t.start()
for t in threads: t.join()
if errors: raise errors[0]
torch.cuda.synchronize()
for (k, name), o in sorted(out.items()):
    for key, d in sorted(digests(o).items()):
        print("DIGEST", k, name, key, d)
"""


def test_first_use_from_two_threads_in_a_fresh_process(gpu_ops):
    """the LDS-attribute flags, the step tables and the tuning options are set on first use, behind mutexes; this process is
    past that point, so ONE child process makes its first library calls from two threads released together: both run the
    Schwinger closed-form job (the same beta: the same step table) and then the Swendsen-Wang job"""
    want = {name: digests(serial(gpu_ops, name)) for name in ("schwinger_closed_form", "sigma_sw")}
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    seen = set()
    for line in r.stdout.splitlines():
        if line.startswith("DIGEST "):
            _, k, name, key, d = line.split()
            assert d == want[name][key], f"thread {k}: {name} output '{key}' differs from the default-stream result of this process"
            seen.add((int(k), name, key))
    assert seen == {(k, name, key) for k in range(2) for name in want for key in want[name]}, r.stdout[-2000:]


# ---- 8. the estimator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hierarchical", [False, True], ids=["plain", "hierarchical"])
def test_estimator_does_not_depend_on_concurrent_levels(gpu_ops, hierarchical):
    """PathMLMC with every level on its own stream (the default) against the levels one after another on the caller's
    stream: quartic M0 = 128, 3 levels, B = 64; thermalise, pass_(8), and two more passes, which reuse the cached streams"""
    from mlmcpathintegral_amd import abi, mlmc

    def build(concurrent):
        m = mlmc.PathMLMC(abi.QUARTIC, 128, 16.0, 3, 64, nt=6, dt0=0.1, seed=11, params=dict(lam=1.0, x0=1.0),
                          hierarchical=hierarchical, dt_coarse=0.2)
        m.concurrent_levels = concurrent
        m.thermalise(8)
        return m

    both = [build(True), build(False)]
    assert both[0].concurrent_levels and not both[1].concurrent_levels and len(both[0].levels) == 3
    for n_pass, n_samples in enumerate((8, 3, 3)):
        for m in both:
            m.pass_(n_samples)
        torch.cuda.synchronize()
        assert len(both[0]._streams) == 3 and not both[1]._streams
        a, b = both
        for l in sorted(a.levels):
            la, lb = a.levels[l], b.levels[l]
            what = f"level {l} after pass {n_pass}"
            assert bits_equal(la.acc, lb.acc), f"{what}: acc"
            assert bits_equal(la.step_accepted, lb.step_accepted), f"{what}: step_accepted"
            assert la.site_steps == lb.site_steps and la.n_draws == lb.n_draws, what
            assert bits_equal(la.hmc.n_accepted, lb.hmc.n_accepted), f"{what}: hmc.n_accepted"
            if hierarchical:
                assert la.n_sub_sum == lb.n_sub_sum, f"{what}: n_sub_sum {la.n_sub_sum} != {lb.n_sub_sum}"
                assert bits_equal(la.wstats, lb.wstats), f"{what}: windowed statistics"
        assert bits_equal(a.table(), b.table()), f"table after pass {n_pass}"
