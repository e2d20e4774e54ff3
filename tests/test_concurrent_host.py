"""Scheduling of ``concurrent.map_on_streams`` with stand-in streams (no GPU), and the thread safety of the host
operator cache that concurrent simulations share."""
from __future__ import annotations

import threading
import time

import numpy as np
import pytest

from quantum_computations_amd.concurrent import map_on_streams
from quantum_computations_amd.cv_simulator import gates as CV


class FakeStream:
    """Records which jobs ran inside it and whether it was released; at most one job may be inside at a time."""

    def __init__(self, slot: int, log: "Log"):
        self.slot, self.log = slot, log
        self.inside = 0
        self.released = False

    def __enter__(self):
        with self.log.lock:
            self.inside += 1
            if self.inside > 1:
                self.log.shared.append(self.slot)
            self.log.in_flight += 1
            self.log.peak = max(self.log.peak, self.log.in_flight)
            self.log.current.stream = self
        return self

    def __exit__(self, *exc):
        with self.log.lock:
            self.inside -= 1
            self.log.in_flight -= 1
        return False

    def release(self):
        self.released = True


class Log:
    def __init__(self):
        self.lock = threading.Lock()
        self.in_flight = self.peak = 0
        self.shared: list[int] = []
        self.streams: list[FakeStream] = []
        self.started: list[int] = []
        self.current = threading.local()

    def factory(self, slot: int) -> FakeStream:
        stream = FakeStream(slot, self)
        self.streams.append(stream)
        return stream


def test_results_come_back_in_input_order():
    log = Log()

    def job(x):
        time.sleep(0.001 * ((7 * x) % 5))      # finish out of order
        return x * x

    assert map_on_streams(job, range(40), max_concurrent=6, stream_factory=log.factory) == [x * x for x in range(40)]
    assert map_on_streams(job, [], stream_factory=log.factory) == []


def test_in_flight_jobs_are_bounded_and_never_share_a_stream():
    log = Log()
    seen: dict[int, set] = {}

    def job(x):
        time.sleep(0.002)
        stream = log.current.stream
        with log.lock:
            seen.setdefault(stream.slot, set()).add(x)
        return stream.slot

    slots = map_on_streams(job, range(50), max_concurrent=4, stream_factory=log.factory)
    assert 1 < log.peak <= 4
    assert log.shared == []
    assert len(log.streams) == 4 and set(slots) <= {0, 1, 2, 3}
    assert sorted(x for xs in seen.values() for x in xs) == list(range(50))
    assert all(s.released for s in log.streams)
    # fewer items than workers: one stream per item, no more
    log2 = Log()
    map_on_streams(lambda x: x, range(3), max_concurrent=8, stream_factory=log2.factory)
    assert len(log2.streams) == 3


def test_first_failure_in_input_order_is_raised_after_the_others_stop():
    log = Log()
    gate = threading.Barrier(3)
    finished: list[int] = []

    def job(x):
        with log.lock:
            log.started.append(x)
        if x < 3:
            gate.wait(timeout=10)          # jobs 0..2 are in flight together
        if x == 2:
            raise KeyError("late failure")
        if x == 1:
            time.sleep(0.05)               # fails after job 2, but comes first in input order
            raise ValueError("first in input order")
        time.sleep(0.1)
        with log.lock:
            finished.append(x)
        return x

    with pytest.raises(ValueError, match="first in input order"):
        map_on_streams(job, range(30), max_concurrent=3, stream_factory=log.factory)
    assert 0 in finished                    # the job still running when the failures came was let finish
    assert all(s.released for s in log.streams)
    assert log.in_flight == 0


def test_no_job_starts_after_a_failure():
    log = Log()
    failed = threading.Event()
    late: list[int] = []

    def job(x):
        if failed.is_set():
            late.append(x)
        if x == 0:
            failed.set()
            raise RuntimeError("boom")
        time.sleep(0.01)
        return x

    with pytest.raises(RuntimeError, match="boom"):
        map_on_streams(job, range(200), max_concurrent=2, stream_factory=log.factory)
    # job 1 (or the one the other worker had already taken) may have been in flight; nothing is started afterwards
    assert len(late) <= 1


def test_a_batch_after_a_failure_runs():
    log = Log()

    def bad(x):
        if x == 5:
            raise OSError("disk")
        return x

    with pytest.raises(OSError):
        map_on_streams(bad, range(10), max_concurrent=3, stream_factory=log.factory)
    assert map_on_streams(lambda x: x + 1, range(10), max_concurrent=3, stream_factory=log.factory) == list(range(1, 11))
    assert all(s.released for s in log.streams)


def test_max_concurrent_must_be_positive():
    with pytest.raises(ValueError):
        map_on_streams(lambda x: x, [1], max_concurrent=0, stream_factory=Log().factory)


def test_operator_cache_under_threads():
    """16 threads request more distinct operators than the LRU keeps: no KeyError, and equal gates share one array."""
    domain = np.linspace(-4.0, 4.0, 16)
    errors: list[BaseException] = []
    results: dict[tuple, set] = {}
    lock = threading.Lock()
    start = threading.Barrier(16)

    def worker(t: int):
        try:
            start.wait(timeout=10)
            for round_ in range(200):
                s = 0.1 * ((t + round_) % (3 * CV._OPERATORS_KEPT))
                gate = CV.X(0, s)
                op = CV._cached(gate, "op", domain, lambda: gate.operator(domain))
                assert op.shape == (16, 16)
                with lock:
                    results.setdefault(s, set()).add(float(np.abs(op).sum()))
        except BaseException as exc:       # noqa: BLE001 -- reported below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    assert len(results) == 3 * CV._OPERATORS_KEPT
    assert all(len(v) == 1 for v in results.values())        # every thread saw the same operator for a key
    assert len(CV._OPERATORS) <= CV._OPERATORS_KEPT
