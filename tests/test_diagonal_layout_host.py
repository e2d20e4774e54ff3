"""The host-side planning of the diagonal-operator calls (quantum_computations_amd/csrc/qsv_diagonal_layout.h), on the
host only.

tests/layout/diagonal_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan, as
tests/test_krylov_layout_host.py compiles its driver; requests go in as text and answers come back as text.  Checked
against models written here: letters to masks in the big-endian qubit order and every refusal of the term packer (with
the output left untouched), the value the build kernel's loop gives for an index, the grids with and without
QSV_OPT_GRID_CAP, the scratch slices of every reducing kernel (no overlap, inside the requested bytes), and the host-side
combination of the partials, ties of the extrema included.
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as R
import hostcheck

BLOCK, REDUCE_BLOCKS, MAX_BLOCKS = 256, 1024, (1 << 24) - 1
PACK_OK, PACK_NULL, PACK_OFFSETS, PACK_LENGTH, PACK_RANGE, PACK_REPEAT, PACK_LETTER = range(7)
SLOTS = {"expect": 4, "transition": 2, "phase_adjoint": 2, "extrema": 4}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "diagonal_layout_driver.cpp", tmp_path_factory.mktemp("diagonal_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=600)
        return [[part.split() for part in line.split("|")] for line in lines]
    return run


def spell(terms):
    return " ".join(f"{letters or '-'}:{','.join(map(str, qubits))}:{float(c)!r}" for c, letters, qubits in terms)


def pack(n, terms, coeffs=True):
    return f"pack {n} {int(coeffs)} {len(terms)} {spell(terms)}"


def mask_of(n, letters, qubits):
    return sum(1 << (n - 1 - q) for letter, q in zip(letters, qubits) if letter in "Zz")


def test_letters_become_masks_in_the_register_order(ask):
    cases = [(3, [(1.5, "Z", [0]), (-2.0, "Z", [2]), (0.25, "ZIZ", [0, 1, 2]), (4.0, "", []), (1.0, "zi", [1, 0])]),
             (1, [(1.0, "Z", [0])]), (0, [(2.0, "", [])]), (0, []), (40, [(1.0, "ZZ", [0, 39])]),
             (64, [(0.5, "Z" * 64, list(range(64)))]), (64, [(0.5, "I" * 63 + "Z", list(range(63, -1, -1)))])]
    cases += [(n, R.random_z_terms(n, count, seed=count)) for n in (6, 13) for count in (1, 2, 63, 64, 65, 200)]
    for (n, terms), answer in zip(cases, ask([pack(n, t) for n, t in cases])):
        assert int(answer[0][0]) == PACK_OK and len(answer) == 1 + len(terms)
        for (c, letters, qubits), (mask, coeff) in zip(terms, answer[1:]):
            assert int(mask) == mask_of(n, letters, qubits) and float.fromhex(coeff) == c
    # no coefficients: all 1
    (answer,) = ask([pack(3, [(7.0, "Z", [1]), (9.0, "", [])], coeffs=False)])
    assert [float.fromhex(part[1]) for part in answer[1:]] == [1.0, 1.0] and int(answer[1][0]) == 2


def test_refusals_leave_the_output_alone(ask):
    good = (1.0, "Z", [0])
    cases = [([good, (1.0, "X", [1])], PACK_LETTER), ([good, (1.0, "ZY", [1, 2])], PACK_LETTER), ([(1.0, "Q", [0])], PACK_LETTER),
             ([good, (1.0, "Z", [4])], PACK_RANGE), ([(1.0, "Z", [-1])], PACK_RANGE), ([good, (1.0, "ZZ", [2, 2])], PACK_REPEAT),
             ([(1.0, "IZI", [1, 3, 1])], PACK_REPEAT), ([good, (1.0, "I" * 65, list(range(65)))], PACK_LENGTH)]
    for (terms, want), answer in zip(cases, ask([pack(4, t) for t, _ in cases])):
        assert answer == [[str(want)]], (terms, answer)
    (answer,) = ask([pack(64, [(1.0, "Z" * 65, list(range(65)))])])
    assert answer == [[str(PACK_LENGTH)]]


def test_table_value_adds_in_the_callers_order(ask):
    n = 7
    terms = R.random_z_terms(n, 65, seed=3)
    want = R.diagonal_from_terms(n, terms)
    start = R.diagonal_from_terms(n, terms[:3])
    indices = [0, 1, 2, 63, 64, 65, 126, 127]
    requests = [f"value {n} 0 {i} {len(terms)} {spell(terms)}" for i in indices]
    requests += [f"value {n} {float(start[i])!r} {i} {len(terms) - 3} {spell(terms[3:])}" for i in indices]
    answers = ask(requests)
    for k, i in enumerate(indices):
        assert float.fromhex(answers[k][0][0]) == want[i]                       # equal, not close
        assert float.fromhex(answers[len(indices) + k][0][0]) == want[i]


def blocks_model(items, cap):
    blocks = max(1, -(-items // BLOCK))
    if cap > 0:
        blocks = min(blocks, cap)
    return min(blocks, MAX_BLOCKS)


def reduce_grid(items, grid_cap):
    return blocks_model(items, min(grid_cap, REDUCE_BLOCKS) if grid_cap > 0 else REDUCE_BLOCKS)


def stream_grid(items, grid_cap):
    return blocks_model(items, grid_cap if grid_cap > 0 else 0)


SIZES = [1, 2, 255, 256, 257, 1 << 13, 1 << 14, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, 1 << 19, 1 << 28, 1 << 32, 1 << 33, 1 << 40]
CAPS = [0, 1, 2, 1000, 1024, 5000]


def test_grids(ask):
    cases = [(items, cap) for items in SIZES for cap in CAPS]
    for (items, cap), ((reduce, stream),) in zip(cases, ask([f"grids {a} {c}" for a, c in cases])):
        assert int(reduce) == reduce_grid(items, cap) and int(stream) == stream_grid(items, cap), (items, cap)
        assert 1 <= int(reduce) <= REDUCE_BLOCKS and 1 <= int(stream) <= MAX_BLOCKS
        if cap:
            assert int(reduce) <= cap and int(stream) <= cap
    # uncapped streaming grid: one item per thread up to the dispatch limit; the reducing grid loops from 2^18 items on,
    # so 2^19 is the smallest power of two at which every thread of the capped grid makes more than one trip
    assert stream_grid(1 << 28, 0) * BLOCK == 1 << 28 and stream_grid(1 << 33, 0) == MAX_BLOCKS
    assert reduce_grid(1 << 18, 0) * BLOCK == 1 << 18 and reduce_grid(1 << 19, 0) * BLOCK * 2 == 1 << 19
    assert stream_grid(1 << 13, 2) * BLOCK * 16 == 1 << 13


@pytest.mark.parametrize("kernel", sorted(SLOTS))
def test_scratch_slices(ask, kernel):
    slots = SLOTS[kernel]
    cases = [(items, cap) for items in (1, 256, 257, 1 << 13, 1 << 18, 1 << 19, 1 << 28) for cap in (0, 2, 1024, 5000)]
    for (items, cap), ((grid, words, nbytes), indices) in zip(cases, ask([f"slices {a} {c} {slots}" for a, c in cases])):
        grid, words, nbytes = int(grid), int(words), int(nbytes)
        indices = [int(v) for v in indices]
        assert grid == reduce_grid(items, cap) and words == grid * slots and nbytes == 8 * words
        assert len(indices) == words and len(set(indices)) == words                 # one word each: no overlap
        assert min(indices) == 0 and max(indices) == words - 1                      # inside the requested bytes
        assert indices == sorted(indices)                                           # [block][slot]


def test_host_sums_run_in_index_order(ask):
    rng = np.random.default_rng(4)
    for items, cap, slots in [(1 << 13, 0, 4), (1 << 13, 2, 2), (1000, 0, 4), (1 << 19, 0, 2)]:
        grid = reduce_grid(items, cap)
        host = rng.standard_normal(grid * slots) * 10.0 ** rng.integers(-8, 8, grid * slots)
        ((got,),) = ask([f"sums {items} {cap} {slots} " + " ".join(repr(float(v)) for v in host)])
        for s in range(slots):
            want = 0.0
            for b in range(grid):
                want += host[b * slots + s]
            assert float.fromhex(got[s]) == want


def test_extrema_combine_with_ties_to_the_lowest_index(ask):
    blocks = [(3.0, 700, 9.0, 600), (-1.0, 40, 9.0, 90), (-1.0, 12, 2.0, 300), (5.0, 2, 9.0, 91)]
    spelled = " ".join(f"{mn!r} {amn} {mx!r} {amx}" for mn, amn, mx, amx in blocks)
    ((got,),) = ask([f"extrema 1024 0 {spelled}"])
    assert (float.fromhex(got[0]), int(got[1]), float.fromhex(got[2]), int(got[3])) == (-1.0, 12, 9.0, 90)
    ((got,),) = ask(["extrema 5 0 -0.5 3 -0.5 3"])
    assert (float.fromhex(got[0]), int(got[1]), float.fromhex(got[2]), int(got[3])) == (-0.5, 3, -0.5, 3)
