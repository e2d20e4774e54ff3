"""Basis-state sampling (``qsv_sample``, ``DeviceState.sample``) at the edges of its inverse CDF, against the exact
rational reference of tests/basis_sample_reference.py: sparse registers, draws on and next to CDF edges, registers that
end inside a chunk of 4096 amplitudes, and registers of 2^14 amplitudes.  Two statements per (state, draw list), neither
of which uses anything the device computed:

* POSSIBLE: every returned index has |amplitude|^2 > 0 in the uploaded data;
* RIGHT: a draw further than ``TIE_BAND`` from every CDF edge returns the exact answer, a draw inside the band returns
  one of the two support indices on either side of that edge.

The last section puts the three entry points that choose a two-outcome measurement through the same kind of edge.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_sample_reference as R
from quantum_computations_amd import _lib
from quantum_computations_amd.device import DeviceState, QuditState
from quantum_computations_amd.dv_simulator import gates as G
from quantum_computations_amd.dv_simulator import program
from quantum_computations_amd.ensemble import TrajectoryEnsemble

CHUNK, PER_THREAD = 4096, 16            # k_chunk_sums / k_sample_in_chunk: amplitudes per workgroup and per thread
RANDOM_DRAWS = 2000
BELOW_ONE = float(np.nextafter(1.0, 0.0))
SENTINEL = np.uint64(0xdeadbeefdeadbeef)

# How far from a CDF edge, as a fraction of the total T, the device may still decide either way.  Every term is >= 0,
# so each rounding is an error of at most eps = 2^-53 relative to a partial sum that is itself at most T:
#   a weight x*x + y*y                                                     3 roundings (2 where it is contracted)
#   a chunk sum: 16 sequential adds, 6 butterfly steps, 4 waves           26 deep, 29 with the weight
#   cum[c] and the total: one add per chunk, at most 4 chunks here        33
#   target = u * total                                                    1 more, and u times the total's 33:  34
#   residual = target - cum[c]                                            1 more, and cum[c]'s 33:             +34
#   the walk's running sum: up to 255 thread sums and 15 slots, each
#   weight through at most 16 + 255 adds, and the compare's own add       3 + 271 + 1 = 275
# 34 + 34 + 275 = 343 eps; the band is the next power of two, 512 eps = 2^-44 = 5.7e-14.
TIE_BAND = 2.0 ** -44

REGISTERS = {                           # name -> (kind, shape): qubits, or (n_modes, d)
    "q12": ("qubits", 12),              # exactly one chunk
    "q13": ("qubits", 13),              # two chunks
    "q14": ("qubits", 14),              # four chunks; the streaming-side register size
    "m3d5": ("modes", (3, 5)),          # 125 amplitudes: less than one chunk
    "m8d3": ("modes", (8, 3)),          # 6561: one full chunk and a partial one
    "q1": ("qubits", 1),                # 2 amplitudes
    "m1d3": ("modes", (1, 3)),          # 3 amplitudes
}


def size_of(register: str) -> int:
    kind, shape = REGISTERS[register]
    return 1 << shape if kind == "qubits" else shape[1] ** shape[0]


def chunk_ranges(size: int):
    return [(first, min(first + CHUNK, size)) for first in range(0, size, CHUNK)]


# ---- states: random complex amplitudes on the support, exact zeros elsewhere -------------------------------------------------
def gaussian(rng, count):
    return rng.normal(size=count) + 1j * rng.normal(size=count)


def on_support(size, indices, rng):
    amps = np.zeros(size, dtype=np.complex128)
    indices = np.asarray(sorted(set(int(i) for i in indices)), dtype=np.int64)
    amps[indices] = gaussian(rng, len(indices))
    return amps


def first_100(size, rng):               # of every chunk: each chunk's upper edge is followed by zeros only
    return on_support(size, [i for first, stop in chunk_ranges(size) for i in range(first, min(first + 100, stop))], rng)


def one_thread(size, rng):              # the sixteen slots of one thread, in every chunk
    thread = 37 if size >= CHUNK else 3
    return on_support(size, [first + thread * PER_THREAD + k for first, stop in chunk_ranges(size) for k in range(PER_THREAD)
                             if first + thread * PER_THREAD + k < stop], rng)


def chunk_seam(size, rng):              # the last amplitude of chunk 0 and the first of chunk 1
    return on_support(size, [CHUNK - 1, CHUNK], rng)


def random_points(size, rng, chunks=None):   # 300 per chunk (a third of a chunk shorter than 900)
    picked = []
    for c, (first, stop) in enumerate(chunk_ranges(size)):
        if chunks is None or c in chunks:
            picked += [first + int(i) for i in rng.choice(stop - first, size=min(300, max(1, (stop - first) // 3)), replace=False)]
    return on_support(size, picked, rng)


def dense(size, rng):
    return gaussian(rng, size)


def underflow(size, rng):
    """Order-one amplitudes on 300 points per chunk, and EVERY other amplitude about 1e-163: the largest decade near 1e-160
    whose squares (|re|, |im| < 4e-163, so below 2^-1075) all round to a weight of exactly 0.  1e-160 itself squares to
    the denormal 1e-320, a weight that is small but possible."""
    amps = random_points(size, rng)
    tiny = np.clip(rng.normal(size=size), -3.9, 3.9) + 1j * np.clip(rng.normal(size=size), -3.9, 3.9)
    return np.where(amps != 0, amps, 1e-163 * tiny)


FAMILIES = {
    "first_100": first_100,
    "one_thread": one_thread,
    "chunk_seam": chunk_seam,
    "random_300": random_points,
    "empty_chunks_odd": lambda size, rng: random_points(size, rng, chunks=(1, 3)),       # leading and inner empty chunks
    "empty_chunks_even": lambda size, rng: random_points(size, rng, chunks=(0, 2)),      # inner and trailing
    "empty_chunks_but_1": lambda size, rng: random_points(size, rng, chunks=(1,)),       # leading and trailing
    "dense": dense,
    "first_100_times_1e-8": lambda size, rng: 1e-8 * first_100(size, rng),
    "first_100_times_1e+8": lambda size, rng: 1e+8 * first_100(size, rng),
    "underflow": underflow,
    "only_first": lambda size, rng: on_support(size, [0], rng),
    "only_last": lambda size, rng: on_support(size, [size - 1], rng),
}
SPARSE_ONE_CHUNK = ["first_100", "one_thread", "random_300", "dense", "first_100_times_1e-8", "first_100_times_1e+8", "underflow"]
TINY = ["dense", "only_first", "only_last"]
CASES = ([("q12", f) for f in SPARSE_ONE_CHUNK]
         + [("q13", f) for f in ["first_100", "one_thread", "chunk_seam", "random_300", "empty_chunks_odd", "empty_chunks_even",
                                 "dense", "underflow"]]
         + [("q14", f) for f in ["first_100", "one_thread", "chunk_seam", "random_300", "empty_chunks_odd", "empty_chunks_even",
                                 "empty_chunks_but_1", "dense", "underflow"]]
         + [("m3d5", f) for f in ["first_100", "one_thread", "random_300", "dense", "only_last"]]
         + [("m8d3", f) for f in ["first_100", "one_thread", "chunk_seam", "random_300", "empty_chunks_odd", "empty_chunks_even",
                                  "dense", "first_100_times_1e-8", "underflow"]]
         + [("q1", f) for f in TINY] + [("m1d3", f) for f in TINY])
CASE_IDS = [f"{register}-{family}" for register, family in CASES]


class Case:
    """A state, its draw list and what the exact reference says about every draw.  Built once, never changed."""

    def __init__(self, register, family):
        self.register, self.family, self.size = register, family, size_of(register)
        rng = np.random.default_rng([CASES.index((register, family)), 20240917])
        self.amps = FAMILIES[family](self.size, rng)
        self.amps.setflags(write=False)
        self.possible = R.float_weights(self.amps) > 0.0
        self.cdf = R.ExactCdf(self.amps)
        draws = [float(x) for x in rng.random(RANDOM_DRAWS)] + [0.0, BELOW_ONE]
        for first, stop in chunk_ranges(self.size):                       # every chunk's upper CDF edge
            draws += self.cdf.draws_at_edge(self.cdf.edge_of_index(stop))
        interior = np.arange(1, len(self.cdf.support))                    # 32 interior support edges, spread evenly
        for edge in interior[np.unique(np.linspace(0, len(interior) - 1, min(32, len(interior))).astype(int))] if len(interior) else []:
            draws += self.cdf.draws_at_edge(int(edge))
        self.u = np.array(draws)
        self.u.setflags(write=False)
        self.answer, self.bracket, self.distance = R.exact_inverse_cdf(self.cdf, self.u)
        self.in_band = self.distance <= TIE_BAND

    def right(self, got):
        got = np.asarray(got).astype(np.int64)
        return np.where(self.in_band, (got == self.bracket[:, 0]) | (got == self.bracket[:, 1]), got == self.answer)


@functools.lru_cache(maxsize=None)
def case_of(register, family) -> Case:
    return Case(register, family)


# ---- the device ----------------------------------------------------------------------------------------------------------------
def make_register(register, amps):
    kind, shape = REGISTERS[register]
    if kind == "qubits":
        return DeviceState.from_numpy(amps)
    return QuditState.from_numpy(amps.reshape((shape[1],) * shape[0]))


def view_of(register, dev):
    """A second handle over the same device memory."""
    kind, shape = REGISTERS[register]
    ptr = C.c_void_p()
    _lib.call("qsv_device_ptr", dev._h, C.byref(ptr))
    if kind == "qubits":
        return DeviceState.view(shape, ptr.value, size_of(register), device=dev.device)
    h = C.c_void_p()
    _lib.call("qsv_create_qudit_view", shape[0], shape[1], dev.device, ptr, size_of(register), C.c_void_p(0), C.byref(h))
    return QuditState(h, dev.device)


def sample(dev, u):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.full(u.shape[0], SENTINEL, dtype=np.uint64)
    _lib.call("qsv_sample", dev._h, int(u.shape[0]), u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


@functools.lru_cache(maxsize=None)
def sampled(register, family):
    """(first call, second call, through a view, register afterwards) for the case's draws: one upload per case."""
    case = case_of(register, family)
    dev = make_register(register, case.amps)
    first, second = sample(dev, case.u), sample(dev, case.u)
    view = view_of(register, dev)
    through_view = sample(view, case.u)
    view.close()
    after = dev.to_numpy().reshape(-1)
    dev.close()
    return first, second, through_view, after


# ---- the reference alone: the committed seeds give draw lists the two statements can be made about -------------------------
@pytest.mark.parametrize("register,family", CASES, ids=CASE_IDS)
def test_draw_lists_by_the_reference_alone(register, family):
    case = case_of(register, family)
    assert np.count_nonzero(case.in_band[:RANDOM_DRAWS]) <= 1, "at most one random draw inside the tie band"
    assert case.u[RANDOM_DRAWS] == 0.0 and case.u[RANDOM_DRAWS + 1] == BELOW_ONE
    assert np.count_nonzero(case.in_band[RANDOM_DRAWS:]) >= 4, "the edge draws are inside it"
    # a draw inside the band of one edge stays outside the band of the next (a device off by a band sees it within two
    # bands of the first): "one of the two indices at that edge" then says all there is
    assert min(case.cdf.weights) / case.cdf.total > 2 * TIE_BAND
    assert np.all(case.possible[case.answer]) and np.all(case.possible[case.bracket])
    if family == "underflow":                   # every amplitude is nonzero, most weights are zero
        assert np.count_nonzero(case.amps) == case.size and np.count_nonzero(case.possible) == len(case.cdf.support) < case.size // 4


# ---- the two statements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("register,family", CASES, ids=CASE_IDS)
def test_possible_outcome(register, family):
    case, (got, _, _, _) = case_of(register, family), sampled(register, family)
    assert got.dtype == np.uint64 and int(got.max()) < case.size
    impossible = ~case.possible[got.astype(np.int64)]
    print(f"{register} {family}: {np.count_nonzero(impossible)} of {len(got)} draws returned an index of weight zero"
          f" ({np.count_nonzero(impossible[:RANDOM_DRAWS])} of the random ones)")
    assert not impossible.any(), [(float(u).hex(), int(i)) for u, i in zip(case.u[impossible][:8], got[impossible][:8])]


@pytest.mark.parametrize("register,family", CASES, ids=CASE_IDS)
def test_right_outcome(register, family):
    case, (got, _, _, _) = case_of(register, family), sampled(register, family)
    wrong = ~case.right(got)
    print(f"{register} {family}: {np.count_nonzero(case.in_band)} draws inside the band ({np.count_nonzero(case.in_band[:RANDOM_DRAWS])}"
          f" random); wrong: {np.count_nonzero(wrong & case.in_band)} inside, {np.count_nonzero(wrong & ~case.in_band)} outside")
    assert not wrong.any(), [(float(u).hex(), int(i), int(a), b.tolist(), float(d)) for u, i, a, b, d in
                             zip(case.u[wrong][:6], got[wrong][:6], case.answer[wrong][:6], case.bracket[wrong][:6], case.distance[wrong][:6])]


@pytest.mark.parametrize("register,family", CASES, ids=CASE_IDS)
def test_same_draws_same_indices_and_an_untouched_register(register, family):
    case, (first, second, through_view, after) = case_of(register, family), sampled(register, family)
    assert np.array_equal(first, second), "two calls"
    assert np.array_equal(first, through_view), "a view over the same memory"
    assert np.array_equal(after.view(np.uint64), np.ascontiguousarray(case.amps).view(np.uint64)), "sampling reads only"


# ---- shot counts, refusals -----------------------------------------------------------------------------------------------------
def test_one_shot_and_more_shots_than_65535_workgroups():
    case = case_of("q13", "random_300")
    dev = make_register("q13", case.amps)
    for u in (0.0, 0.37, BELOW_ONE):
        got = sample(dev, [u])
        answer, _, _ = R.exact_inverse_cdf(case.cdf, [u])
        assert got.shape == (1,) and int(got[0]) == int(answer[0]), u
    rng = np.random.default_rng(70000)
    edges = np.array(case.cdf.draws_at_edge(case.cdf.edge_of_index(CHUNK)) + [0.0, BELOW_ONE])
    u = np.concatenate([rng.random(70000 - len(edges)), edges])          # the edge draws go to the workgroups past 65535
    got = sample(dev, u)
    answer, bracket, distance = R.exact_inverse_cdf(case.cdf, u)
    in_band = distance <= TIE_BAND
    right = np.where(in_band, (got.astype(np.int64) == bracket[:, 0]) | (got.astype(np.int64) == bracket[:, 1]), got.astype(np.int64) == answer)
    print(f"70000 shots: {np.count_nonzero(in_band)} inside the band, {np.count_nonzero(~right)} wrong,"
          f" {np.count_nonzero(~case.possible[got.astype(np.int64)])} of weight zero")
    assert np.all(case.possible[got.astype(np.int64)]) and np.all(right)
    assert np.all(in_band[-len(edges):])
    dev.close()


@pytest.mark.parametrize("register", ["q13", "m8d3", "q1"])
def test_no_shots_and_draws_outside_the_unit_interval(register):
    case = case_of(register, "dense")
    dev = make_register(register, case.amps)
    u = np.array([0.5, 0.25])
    out = np.full(2, SENTINEL, dtype=np.uint64)
    _lib.call("qsv_sample", dev._h, 0, u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.all(out == SENTINEL), "shots = 0 leaves `out` alone"
    _lib.call("qsv_sample", dev._h, 0, None, None)
    for bad in ([0.5, 1.0], [-1e-300, 0.5], [0.5, float("nan")], [float(np.nextafter(1.0, 2.0))], [-0.5]):
        with pytest.raises(ValueError, match=r"uniform draws must lie in \[0, 1\)"):
            sample(dev, bad)
        assert np.array_equal(dev.to_numpy().reshape(-1).view(np.uint64), np.ascontiguousarray(case.amps).view(np.uint64)), bad
    assert np.array_equal(sample(dev, case.u[:50]), sampled(register, "dense")[0][:50]), "and the register still samples as before"
    dev.close()


def test_a_register_of_zero_norm_is_refused():
    dev = DeviceState.from_numpy(np.zeros(1 << 13, dtype=np.complex128))
    with pytest.raises(ValueError, match="zero norm"):
        sample(dev, [0.5])
    dev.upload(np.full(1 << 13, 1e-170))         # every weight underflows: the same refusal, not an index of weight zero
    with pytest.raises(ValueError, match="zero norm"):
        sample(dev, [0.0, BELOW_ONE])
    dev.close()


# ---- two-outcome measurement at the same edges -----------------------------------------------------------------------------------
# qsv_measure decides u (p0 + p1) < p0, the MEASURE op of qsv_run_programs u < p0 / (p0 + p1), qsv_ensemble_measure walks
# the two weights.  Qubit q of n is bit n - 1 - q of the index; one measured bit below 6 (inside a wave) and the top bit.
MEASURE_SHAPES = [(3, 0), (3, 2), (7, 2), (7, 6), (14, 3), (14, 13)]
Z0, Z1 = np.array([1.0, 0.0], dtype=np.complex128), np.array([0.0, 1.0], dtype=np.complex128)


def half_state(n, bit, value, seed):
    """Random amplitudes where index bit ``bit`` is ``value``, exact zeros elsewhere: the other outcome has probability 0."""
    rng = np.random.default_rng(seed)
    ket = gaussian(rng, 1 << n)
    ket[((np.arange(1 << n) >> bit) & 1) != value] = 0.0
    return ket / np.linalg.norm(ket)


def quarter_state(n, bit):
    """p0 = 1/4 and p1 = 3/4 exactly, in any summation order: every weight is a multiple of 1/16."""
    ket = np.zeros(1 << n, dtype=np.complex128)
    zeros = [i for i in range(1 << n) if not (i >> bit) & 1]
    ones = [i for i in range(1 << n) if (i >> bit) & 1]
    spread = np.linspace(0, len(zeros) - 1, 4).astype(int)
    ket[[zeros[j] for j in spread]] = [0.25, -0.25, 0.25j, 0.25]                 # 4 / 16
    ket[[ones[j] for j in spread]] = [0.25 + 0.25j, 0.5, -0.5j, 0.25 - 0.25j]    # 2/16 + 4/16 + 4/16 + 2/16
    return ket


def measure_register(n, bit, ket, u):
    dev = DeviceState.from_numpy(ket)
    outcome, p0, p1 = dev.measure(n - 1 - bit, Z0, Z1, u01=u)
    after = dev.to_numpy()
    dev.close()
    return outcome, (p0, p1), after


def measure_program(n, bit, ket, u, monkeypatch):
    prog = program.compile_circuit([G.MZ(n - 1 - bit)], n)
    assert len(prog.uniform_slots) == 1
    monkeypatch.setattr(np.random, "random_sample", lambda *a: u)
    (after, results, probs), = program.run_programs([prog], [ket])
    return results[0], tuple(probs[0]), after


def measure_ensemble(n, bit, ket, draws):
    """One member per draw; the measured qubit stays.  Returns the members' outcomes and kets."""
    ens = TrajectoryEnsemble.from_ket(ket, len(draws))
    ens.measure(n - 1 - bit, u=np.array(draws), bit=0)
    outcomes = [int(w) & 1 for w in ens.bits()]
    after = ens.state.to_numpy().reshape(len(draws), -1)
    ens.close()
    return outcomes, after


def program_shape(n, bit):
    """The executor holds at most ``program.MAX_QUBITS`` = 13 qubits: 14 runs there as 13, its top bit as bit 12."""
    return (n, bit) if n <= program.MAX_QUBITS else (program.MAX_QUBITS, min(bit, program.MAX_QUBITS - 1))


@pytest.mark.parametrize("n,bit", MEASURE_SHAPES)
def test_measurement_never_chooses_an_outcome_of_probability_zero(n, bit, monkeypatch):
    e0, e1 = G.MZ(0).eigenvectors()
    assert np.array_equal(e0, Z0) and np.array_equal(e1, Z1)
    pn, pbit = program_shape(n, bit)
    for value in (0, 1):
        ket, pket = half_state(n, bit, value, 10 * n + bit), half_state(pn, pbit, value, 10 * n + bit)
        for u in (0.0, BELOW_ONE):
            outcome, probs, after = measure_register(n, bit, ket, u)
            assert outcome == value and probs[1 - value] == 0.0 and np.all(np.isfinite(after.view(np.float64))), ("qsv_measure", value, u)
            assert abs(np.linalg.norm(after) - 1.0) < 1e-12
            outcome, probs, after = measure_program(pn, pbit, pket, u, monkeypatch)
            assert outcome == value and probs[1 - value] == 0.0 and np.all(np.isfinite(after.view(np.float64))), ("MEASURE op", value, u)
            assert abs(np.linalg.norm(after) - 1.0) < 1e-12
        outcomes, after = measure_ensemble(n, bit, ket, [0.0, BELOW_ONE])
        assert outcomes == [value, value] and np.all(np.isfinite(after.view(np.float64))), ("qsv_ensemble_measure", value)
        assert np.max(np.abs(np.linalg.norm(after, axis=1) - 1.0)) < 1e-12


@pytest.mark.parametrize("n,bit", MEASURE_SHAPES)
def test_measurement_at_a_dyadic_edge(n, bit, monkeypatch):
    """p0 = 0.25 exactly: a draw of 0.25 is outcome 1, the float below it outcome 0, on all three entry points."""
    below = float(np.nextafter(0.25, 0.0))
    pn, pbit = program_shape(n, bit)
    ket, pket = quarter_state(n, bit), quarter_state(pn, pbit)
    for u, want in ((0.25, 1), (below, 0)):
        outcome, probs, after = measure_register(n, bit, ket, u)
        assert probs == (0.25, 0.75) and outcome == want, ("qsv_measure", u)
        assert np.all(np.isfinite(after.view(np.float64)))
        outcome, probs, after = measure_program(pn, pbit, pket, u, monkeypatch)
        assert probs == (0.25, 0.75) and outcome == want, ("MEASURE op", u)
        assert np.all(np.isfinite(after.view(np.float64)))
    outcomes, after = measure_ensemble(n, bit, ket, [0.25, below])
    assert outcomes == [1, 0] and np.all(np.isfinite(after.view(np.float64))), "qsv_ensemble_measure"
