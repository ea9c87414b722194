"""CPU: the drivers of tests/stream_cases.py with fake jobs and a fake stream context (no torch, no device).  What
tests/test_streams_gpu.py relies on: run_interleaved issues the jobs' calls strictly round-robin, each under its own stream,
a job that ends leaves the rotation, and every job's return value reaches the caller."""
import contextlib
import subprocess
import sys

import stream_cases as sc


def _fake_job(name, n_calls, log, current):
    """a job of n_calls calls: logs (name, call, the stream that is current) per call"""
    for k in range(n_calls):
        log.append((name, k, current[0]))
        yield
    return {"name": name, "calls": n_calls}


def _fake_context(current, entered):
    @contextlib.contextmanager
    def ctx(stream):
        assert current[0] is None, "stream contexts must not nest"
        current[0] = stream
        entered.append(stream)
        try:
            yield
        finally:
            current[0] = None
    return ctx


def test_run_serial_returns_the_jobs_dict():
    log, current = [], ["default"]
    assert sc.run_serial(_fake_job("a", 4, log, current)) == {"name": "a", "calls": 4}
    assert log == [("a", k, "default") for k in range(4)]
    assert sc.run_serial(_fake_job("none", 0, log, current)) == {"name": "none", "calls": 0}


def test_interleaved_is_strictly_round_robin_under_each_jobs_stream():
    log, current, entered = [], [None], []
    jobs = [_fake_job("a", 3, log, current), _fake_job("b", 3, log, current)]
    res = sc.run_interleaved(jobs, ["s1", "s2"], stream_context=_fake_context(current, entered))
    assert log == [("a", 0, "s1"), ("b", 0, "s2"), ("a", 1, "s1"), ("b", 1, "s2"), ("a", 2, "s1"), ("b", 2, "s2")]
    assert res == [{"name": "a", "calls": 3}, {"name": "b", "calls": 3}]
    # one more turn each, in which the generators end: every advance happens under the job's own stream
    assert entered == ["s1", "s2"] * 4
    assert current[0] is None


def test_a_job_that_ends_early_leaves_the_rotation():
    log, current, entered = [], [None], []
    jobs = [_fake_job("long", 5, log, current), _fake_job("short", 1, log, current), _fake_job("mid", 3, log, current)]
    res = sc.run_interleaved(jobs, ["s1", "s2", "s3"], stream_context=_fake_context(current, entered))
    assert [(n, k) for n, k, _ in log] == [("long", 0), ("short", 0), ("mid", 0), ("long", 1), ("mid", 1), ("long", 2), ("mid", 2),
                                           ("long", 3), ("long", 4)]
    assert all(s == {"long": "s1", "short": "s2", "mid": "s3"}[n] for n, _, s in log)
    assert [r["name"] for r in res] == ["long", "short", "mid"] and [r["calls"] for r in res] == [5, 1, 3]
    # "short" is advanced twice (its call, then its end) and never again
    assert entered.count("s2") == 2 and entered.count("s3") == 4 and entered.count("s1") == 6


def test_fork_and_join_bracket_the_calls():
    events, log, current = [], [], [None]

    class Backend(sc.PlainStreams):
        def fork(self, streams):
            events.append(("fork", tuple(streams), len(log)))

        def join(self, streams):
            events.append(("join", tuple(streams), len(log)))

    jobs = [_fake_job("a", 2, log, current), _fake_job("b", 1, log, current)]
    res = sc.run_interleaved(jobs, ["s1", "s2"], backend=Backend(_fake_context(current, [])))
    assert events == [("fork", ("s1", "s2"), 0), ("join", ("s1", "s2"), 3)]
    assert res == [{"name": "a", "calls": 2}, {"name": "b", "calls": 1}]


def test_an_exception_in_a_job_reaches_the_caller():
    def bad():
        yield
        raise ValueError("from the job")

    try:
        sc.run_interleaved([bad()], ["s"], stream_context=lambda s: contextlib.nullcontext())
    except ValueError as e:
        assert "from the job" in str(e)
    else:
        raise AssertionError("the job's exception was swallowed")


def test_intervals_overlap():
    assert sc.intervals_overlap((0.0, 2.0), (1.0, 3.0)) and sc.intervals_overlap((1.0, 3.0), (0.0, 2.0))
    assert sc.intervals_overlap((0.0, 5.0), (1.0, 2.0))
    assert not sc.intervals_overlap((0.0, 1.0), (1.0, 2.0)) and not sc.intervals_overlap((3.0, 4.0), (0.0, 1.0))


def test_job_list_and_import_without_torch():
    names = [n for n, _ in sc.JOBS]
    assert len(names) == len(set(names)) == 17
    assert sc.scratch_growth_bytes() == 8 << 20 and sc.scratch_growth_bytes() > 1 << 20   # beyond the slot's 1 MiB floor
    code = "import sys; sys.path.insert(0, %r); import stream_cases; assert 'torch' not in sys.modules" % sc.__file__.rsplit("/", 1)[0]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
