"""The pass planner of qsv_apply_pauli_rotations (quantum_computations_amd/csrc/qsv_pauli_rotation_plan.h), on the host.

tests/pauli_plan/rotation_plan_driver.cpp is compiled against the header with AddressSanitizer + UBSan exactly as
tests/test_pauli_plan_host.py compiles its driver; term lists go in as text and plans come back as text.  Every plan is
compared with the Python model of the greedy rule (tests/pauli_rotation_reference.py) and checked for the properties the
kernel relies on: the caller's order, one flipped mask per pass, the cap, maximality and the pivot on the highest bit.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck
import pauli_rotation_reference as R

MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "pauli_plan" / "rotation_plan_driver.cpp", tmp_path_factory.mktemp("pauli_rotation_plan"))

    def run(term_lists):
        """term_lists: [[(xmask, zmask), ...]] -> [(cap, [pass dict, ...])], one per list."""
        requests = [" ".join([str(len(terms))] + [f"{x:x} {z:x}" for x, z in terms]) for terms in term_lists]
        lines = hostcheck.ask(exe, requests, timeout=600)
        plans = []
        for line in lines:
            head, *parts = [part.split() for part in line.split("|")]
            cap, count = int(head[0]), int(head[1])
            assert count == len(parts)
            passes = []
            for tokens in parts:
                assert len(tokens) >= 6 and (len(tokens) - 2) % 4 == 0, "a pass never comes back empty"
                body = tokens[2:]
                passes.append({"xmask": int(tokens[0], 16), "pivot": int(tokens[1]), "index": [int(t) for t in body[0::4]],
                               "term_xmask": [int(t, 16) for t in body[1::4]], "zmask": [int(t, 16) for t in body[2::4]],
                               "n_y": [int(t) for t in body[3::4]]})
            plans.append((cap, passes))
        return plans
    return run


def check(terms, cap, passes):
    assert cap == R.ROTATIONS_PER_PASS == 8
    assert passes == R.plan(terms, cap)                                       # the model, field by field
    assert [i for p in passes for i in p["index"]] == list(range(len(terms))), "0..T-1, in the caller's order"
    for p in passes:
        assert 1 <= len(p["index"]) <= cap
        flips = {x for x in p["term_xmask"] if x}
        assert len(flips) <= 1 and flips == ({p["xmask"]} if p["xmask"] else set())
        assert p["pivot"] == p["xmask"].bit_length() - 1                       # the highest set bit; -1 for a diagonal pass
        for t, x, z, n_y in zip(p["index"], p["term_xmask"], p["zmask"], p["n_y"]):
            assert (x, z) == tuple(terms[t]) and n_y == bin(x & z).count("1")
    for p, nxt in zip(passes, passes[1:]):                                     # maximality: the next term could not have joined
        x = nxt["term_xmask"][0]
        assert len(p["index"]) == cap or not (x == 0 or p["xmask"] == 0 or x == p["xmask"])


def run_and_check(ask, lists):
    plans = ask(lists)
    for terms, (cap, passes) in zip(lists, plans):
        check(terms, cap, passes)
    return [passes for _, passes in plans]


def test_empty_single_and_diagonal_runs(ask):
    lists = [[], [(0b110, 0b010)], [(0, 0)]] + [[(0, z + 1) for z in range(count)] for count in (8, 9, 17)]
    plans = run_and_check(ask, lists)
    assert [len(p) for p in plans] == [0, 1, 1, 1, 2, 3]
    assert plans[1][0]["pivot"] == 2 and plans[2][0]["pivot"] == -1
    assert [len(p["index"]) for p in plans[5]] == [8, 8, 1]


def test_alternating_masks_never_share(ask):
    a, b = 0b0110, 0b1001
    lists = [[(a if t % 2 else b, t) for t in range(7)], [(a, 0), (a, a), (b, 0), (b, b), (a, 1)]]
    plans = run_and_check(ask, lists)
    assert len(plans[0]) == 7
    assert [p["index"] for p in plans[1]] == [[0, 1], [2, 3], [4]]


def test_diagonal_terms_before_between_and_after_a_flipping_run(ask):
    x = 0b101000
    lists = [[(0, 1), (0, 2), (x, 0), (x, x), (0, 4)],                         # before and after
             [(x, 0), (0, 7), (x, 8), (0, 1), (0, 2), (x, x)],                 # between
             [(0, 1)] * 3 + [(x, 0)] * 3 + [(0, 2)] * 3,                       # nine terms: the cap cuts, not the masks
             [(0, 1), (x, 0), (0, 2), (x >> 1, 0), (0, 3)]]                    # a diagonal term after a closed pass opens the next
    plans = run_and_check(ask, lists)
    assert [len(p) for p in plans] == [1, 1, 2, 2]
    assert plans[0][0]["xmask"] == x and plans[0][0]["pivot"] == 5
    assert [p["index"] for p in plans[2]] == [list(range(8)), [8]] and plans[2][1]["xmask"] == 0
    assert [p["index"] for p in plans[3]] == [[0, 1, 2], [3, 4]]


def test_heisenberg_chain_is_one_pass_per_bond(ask):
    n = 12
    chain = []
    for q in range(n - 1):
        pair = (1 << (n - 1 - q)) | (1 << (n - 2 - q))
        chain += [(pair, 0), (pair, pair), (0, pair)]
    (passes,) = run_and_check(ask, [chain])
    assert len(passes) == 11 and [p["pivot"] for p in passes] == list(range(11, 0, -1))
    assert all(p["n_y"] == [0, 2, 0] for p in passes)


def test_bit_63(ask):
    top = 1 << 63
    lists = [[(top, 0), (top, top), (0, MASK64), (top, MASK64)], [(top | 1, top), (0, top), (MASK64, MASK64), (MASK64, 1), (1, 0)]]
    plans = run_and_check(ask, lists)
    assert len(plans[0]) == 1 and plans[0][0]["pivot"] == 63 and plans[0][0]["n_y"] == [0, 1, 0, 1]
    assert [p["pivot"] for p in plans[1]] == [63, 63, 0] and plans[1][1]["n_y"] == [64, 1]


def test_random_lists(ask):
    rng = np.random.default_rng(23)
    lists = []
    for n in (1, 2, 3, 7, 14, 28, 40, 62):
        for count in (1, 2, 9, 40):
            pool = [0, 0] + [int(rng.integers(0, 1 << n)) for _ in range(2)]
            lists.append([(pool[int(rng.integers(4))], int(rng.integers(0, 1 << n))) for _ in range(count)])
    run_and_check(ask, lists)
