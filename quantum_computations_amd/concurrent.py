"""Independent simulations side by side on one GPU, one HIP stream each.

The matrix-product (MPS) and GKP simulations spend their GPU time in kernels of one or a few workgroups -- the small
Jacobi SVD, the panel factorisations of the splits -- and in host round trips between them, so one run leaves most of
the chip idle.  The reference fans its sweeps out over a process pool (``average_clifford_fidelity.py:212``,
``grover.py:119``); here the runs of a sweep share one process and one device, each on a worker thread that owns a
stream of its own: libqsv.so keeps a context per (device, stream) and holds no lock across a launch or a wait
(include/qsv.h, "Threading"), and every register waits on its own stream only.

    results = map_on_streams(run_one, experiments, max_concurrent=8)

``cv_simulator.Simulator.run_batch`` and ``gkp_simulator.Simulator.run_batch`` are this for lists of simulators.
Runs are not batched into shared launches: GKP runs diverge (classically controlled corrections, bond dimensions), so
each keeps its own sequence of calls and its own generator, and a seeded run draws exactly what it draws alone.
"""
from __future__ import annotations

import contextlib
import threading
from typing import Callable, Iterable, Sequence, TypeVar

T = TypeVar("T")
R = TypeVar("R")

# Jobs in flight by default: what profiles/r05_gkp_concurrent_scaling.json supports for the GKP Grover sweep.
DEFAULT_MAX_CONCURRENT = 8

# Streams of the batches.  ``torch.cuda.Stream()`` hands out streams from a small pool in round-robin order, so two
# workers -- or a worker and unrelated code -- could get the same HIP stream, and with it the same library context.
# The batches use streams of their own instead: created with hipStreamCreateWithFlags, checked out by one worker at a
# time, and kept for later batches (never destroyed: a tensor a job used on one may outlive the batch).
_IDLE_STREAMS: dict[int, list] = {}
_IDLE_LOCK = threading.Lock()


def _new_stream(torch, device: int):
    import ctypes as C

    hip = C.CDLL("libamdhip64.so.7")       # the HIP runtime libqsv.so and torch already share (_lib.load)
    handle = C.c_void_p()
    with torch.cuda.device(device):
        status = hip.hipStreamCreateWithFlags(C.byref(handle), C.c_uint(1))      # hipStreamNonBlocking
    if status != 0 or not handle.value:
        raise RuntimeError(f"hipStreamCreateWithFlags failed ({status})")
    return torch.cuda.ExternalStream(handle.value, device=torch.device("cuda", device))


def _checkout_stream(torch, device: int):
    with _IDLE_LOCK:
        idle = _IDLE_STREAMS.setdefault(device, [])
        if idle:
            return idle.pop()
    return _new_stream(torch, device)


def _return_stream(device: int, stream) -> None:
    with _IDLE_LOCK:
        _IDLE_STREAMS.setdefault(device, []).append(stream)


class _TorchStreams:
    """The default stream source: a dedicated HIP stream per worker (see ``_IDLE_STREAMS``); each job runs with it as
    torch's current stream, and its library context is released when the batch ends."""

    def __init__(self, device: int, workspace_bytes: int):
        import torch

        from . import _lib

        self._torch, self._lib = torch, _lib
        self.device = int(device)
        self.workspace_bytes = int(workspace_bytes)
        _lib.load()          # once, on the calling thread

    def make(self, slot: int):
        import ctypes as C

        stream = _checkout_stream(self._torch, self.device)
        if self.workspace_bytes > 0:
            try:
                self._lib.call("qsv_tensor_reserve_workspace", self.device, C.c_void_p(stream.cuda_stream),
                               self.workspace_bytes)
            except BaseException:
                self.release(stream)
                raise
        return stream

    def enter(self, stream):
        return self._torch.cuda.stream(stream)

    def release(self, stream) -> None:
        import ctypes as C

        try:
            self._lib.call("qsv_tensor_release_stream_workspace", self.device, C.c_void_p(stream.cuda_stream))
        finally:
            _return_stream(self.device, stream)


class _FactoryStreams:
    """Streams from a caller's factory (tests without a GPU): ``stream_factory(slot)`` returns any object; if it is a
    context manager a job runs inside it, and its ``release()`` (if any) is called when the batch ends."""

    def __init__(self, factory: Callable[[int], object]):
        self._factory = factory

    def make(self, slot: int):
        return self._factory(slot)

    @staticmethod
    def enter(stream):
        return stream if hasattr(stream, "__enter__") else contextlib.nullcontext()

    @staticmethod
    def release(stream) -> None:
        release = getattr(stream, "release", None)
        if release is not None:
            release()


def map_on_streams(fn: Callable[[T], R], items: Iterable[T], *, max_concurrent: int = DEFAULT_MAX_CONCURRENT,
                   device: int = 0, stream_factory: Callable[[int], object] | None = None,
                   workspace_bytes: int = 0) -> list[R]:
    """``[fn(item) for item in items]``, with up to ``max_concurrent`` calls in flight on worker threads.

    Each worker owns one stream for its whole life -- a dedicated HIP stream that no other worker and no other code
    holds meanwhile -- and runs its jobs one after another with that stream as torch's current stream, so no two jobs
    in flight share a stream.  Results come back in input order.  When a job raises,
    the jobs already running finish, no new job starts, every stream's library context is released, and the first
    failure in input order is re-raised.  A register that a job closes must own its stream (``SiteRegister(...,
    stream=)`` or ``adopt_stream``): without one, ``close`` releases the library contexts of the whole device, which
    other jobs are using.

    ``workspace_bytes`` > 0 pre-sizes each stream's scratch pool (``qsv_tensor_reserve_workspace``) so that no split
    grows it mid-batch.  ``stream_factory(slot)`` replaces the torch streams (see ``_FactoryStreams``): it exists so
    that the scheduling can be tested without a GPU.
    """
    items = list(items)
    if max_concurrent < 1:
        raise ValueError("max_concurrent must be at least 1")
    if not items:
        return []
    streams = _FactoryStreams(stream_factory) if stream_factory is not None else _TorchStreams(device, workspace_bytes)
    workers = min(int(max_concurrent), len(items))
    results: list = [None] * len(items)
    failures: dict[int, BaseException] = {}
    lock = threading.Lock()
    next_index = [0]
    made: list = []
    try:
        for slot in range(workers):
            made.append(streams.make(slot))
    except BaseException:
        for stream in made:
            streams.release(stream)
        raise

    def take() -> int | None:
        with lock:
            if failures or next_index[0] >= len(items):
                return None
            index = next_index[0]
            next_index[0] += 1
            return index

    def worker(slot: int) -> None:
        stream = made[slot]
        while (index := take()) is not None:
            try:
                with streams.enter(stream):
                    results[index] = fn(items[index])
            except BaseException as exc:
                with lock:
                    failures[index] = exc

    threads = [threading.Thread(target=worker, args=(slot,), name=f"qsv-stream-{slot}", daemon=True)
               for slot in range(workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    release_error = None
    for stream in made:
        try:
            streams.release(stream)
        except BaseException as exc:       # a job's failure takes precedence over one of the clean-up
            release_error = release_error or exc
    if failures:
        raise failures[min(failures)]
    if release_error is not None:
        raise release_error
    return results


def run_simulators(simulators: Sequence, initial_states: Sequence, **kw) -> list:
    """``[s.run(x) for s, x in zip(simulators, initial_states)]`` through :func:`map_on_streams`; every register is
    adopted onto the stream of the job that runs it (``SiteRegister.adopt_stream``) and handed back to the stream it
    came from when the job ends, so that it is used after the batch as it was before."""
    simulators, initial_states = list(simulators), list(initial_states)
    if len(simulators) != len(initial_states):
        raise ValueError(f"{len(simulators)} simulators for {len(initial_states)} initial states")
    if len({id(s) for s in simulators}) != len(simulators):
        raise ValueError("a simulator object can run only one job of a batch")
    gpu = kw.get("stream_factory") is None
    if gpu:
        import torch

        producer = torch.cuda.current_stream(kw.get("device", 0))     # where the initial states were built

    def job(pair):
        simulator, state = pair
        reg = getattr(state, "reg", None)
        if not (gpu and getattr(reg, "layout", None) == "sites"):
            return simulator.run(state)
        home = reg.stream                           # None: torch's current stream at each call, as before the batch
        back_to = home if home is not None else producer
        worker_stream = torch.cuda.current_stream(reg.device)
        reg.adopt_stream(worker_stream, source=back_to)
        try:
            return simulator.run(state)
        finally:
            # hand the register back: the caller's stream waits for the job's work, and the worker's stream -- which a
            # later batch may check out -- is no longer the register's
            reg.adopt_stream(back_to, source=worker_stream)
            reg.stream = home

    return map_on_streams(job, list(zip(simulators, initial_states)), **kw)
