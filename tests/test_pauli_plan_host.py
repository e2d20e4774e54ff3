"""The pass planner of qsv_expect_pauli_sum (quantum_computations_amd/csrc/qsv_pauli_plan.h), on the host only.

tests/pauli_plan/plan_driver.cpp is compiled against the header with AddressSanitizer + UBSan; term lists go in as text
and plans come back as text.  Every plan is compared with a NumPy model of the grouping written here (groups by xmask
in order of first appearance, the caller's order inside a group, chunks of PAULI_TERMS_PER_PASS), and the factor the
planner puts in front of a term's accumulator is checked against the dense Pauli operators of ``npq.PAULIS``: the model
of one pass (each pair visited once through the index whose pivot bit is clear) must give <psi|P|psi>.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck
from quantum_computations_amd.dv_simulator import numpy_quantum as npq

MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "pauli_plan" / "plan_driver.cpp", tmp_path_factory.mktemp("pauli_plan"))

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
                passes.append({"xmask": int(tokens[0], 16), "pivot": int(tokens[1]),
                               "zmask": [int(t, 16) for t in body[0::4]], "n_y": [int(t) for t in body[1::4]],
                               "index": [int(t) for t in body[2::4]], "scale": [int(t) for t in body[3::4]]})
            plans.append((cap, passes))
        return plans
    return run


def model(terms, cap):
    """The grouping the header documents: dict order = first appearance, list order = the caller's."""
    groups: dict[int, list[int]] = {}
    for t, (x, _) in enumerate(terms):
        groups.setdefault(x, []).append(t)
    passes = []
    for x, members in groups.items():
        for first in range(0, len(members), cap):
            chunk = members[first:first + cap]
            passes.append({"xmask": x, "pivot": (x & -x).bit_length() - 1 if x else -1,
                           "zmask": [terms[t][1] for t in chunk],
                           "n_y": [bin(x & terms[t][1]).count("1") for t in chunk], "index": chunk})
    return passes


def check(terms, cap, passes):
    want = model(terms, cap)
    assert len(passes) == len(want)
    for got, ref in zip(passes, want):
        for key in ("xmask", "pivot", "zmask", "n_y", "index"):
            assert got[key] == ref[key], key
        assert 1 <= len(got["index"]) <= cap
    assert sorted(i for p in passes for i in p["index"]) == list(range(len(terms))), "every term exactly once"


def test_cap_is_at_least_eight(ask):
    (cap, passes), = ask([[]])
    assert cap >= 8 and passes == []          # an empty list is a valid plan of zero passes


def test_groups_pivots_and_ny(ask):
    rng = np.random.default_rng(5)
    lists = []
    for n in (1, 2, 3, 7, 14, 28, 40, 64):
        for count in (1, 2, 5, 23):
            xs = [int(rng.integers(0, 1 << min(n, 62))) & int(rng.integers(0, 1 << min(n, 62))) for _ in range(4)]
            lists.append([(xs[int(rng.integers(4))], int(rng.integers(0, 1 << min(n, 62)))) for _ in range(count)])
    # every pivot position of a 14-bit register, with and without further flips above it
    lists.append([(1 << b, 0) for b in range(14)] + [((1 << b) | (0x3fff & ~((2 << b) - 1)), 0x2aaa) for b in range(14)])
    # Heisenberg chain on 12 qubits: XX and YY of a pair share a group, every ZZ is diagonal
    chain = []
    for q in range(11):
        pair = (1 << (11 - q)) | (1 << (10 - q))
        chain += [(pair, 0), (pair, pair), (0, pair)]
    lists.append(chain)
    plans = ask(lists)
    for terms, (cap, passes) in zip(lists, plans):
        check(terms, cap, passes)
    cap, passes = plans[-1]
    assert len(passes) == 11 + -(-11 // cap)
    assert [p["n_y"] for p in passes if p["xmask"]] == [[0, 2]] * 11


def test_chunk_boundary(ask):
    (cap, _), = ask([[]])
    x = 0b1010
    counts = [1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 5 * cap]
    lists = [[(x, z) for z in range(count)] for count in counts]
    lists.append([(0, z) for z in range(cap + 1)])                       # the diagonal group is cut the same way
    # two groups interleaved, one a term over the cap: the chunks keep each group's own order
    lists.append([(x if t % 2 else 0b100, t) for t in range(2 * cap + 1)])
    for terms, (_, passes) in zip(lists, ask(lists)):
        check(terms, cap, passes)
        sizes: dict[int, list[int]] = {}
        for p in passes:
            sizes.setdefault(p["xmask"], []).append(len(p["index"]))
        for xmask, got in sizes.items():
            members = sum(1 for t in terms if t[0] == xmask)
            assert got == [cap] * (members // cap) + ([members % cap] if members % cap else [])
    assert len(ask([[(x, z) for z in range(cap)]])[0][1]) == 1 and len(ask([[(x, z) for z in range(cap + 1)]])[0][1]) == 2


def test_empty_and_identity_only(ask):
    (cap, _), = ask([[]])
    lists = [[], [(0, 0)], [(0, 0)] * 3, [(0, 0), (0, 5), (0, 0)], [(0, 0)] * (cap + 1)]
    plans = ask(lists)
    for terms, (_, passes) in zip(lists, plans):
        check(terms, cap, passes)
        for p in passes:
            assert p["xmask"] == 0 and p["pivot"] == -1 and p["n_y"] == [0] * len(p["index"]) and p["scale"] == [1] * len(p["index"])
    assert [len(p) for _, p in plans] == [0, 1, 1, 1, 2]


def test_bit_63(ask):
    top = 1 << 63
    lists = [[(top, 0), (top, top), (top | 1, top), (MASK64, MASK64), (MASK64, top | 1), (0, top), (0, MASK64), (top, MASK64)]]
    (cap, passes), = ask(lists)
    check(lists[0], cap, passes)
    by_x = {p["xmask"]: p for p in passes}
    assert by_x[top]["pivot"] == 63 and by_x[top]["n_y"] == [0, 1, 1]
    assert by_x[top | 1]["pivot"] == 0 and by_x[MASK64]["pivot"] == 0 and by_x[MASK64]["n_y"] == [64, 2]
    assert by_x[0]["pivot"] == -1


def test_duplicates_each_keep_their_slot(ask):
    terms = [(6, 2), (0, 1), (6, 2), (6, 2), (0, 1), (6, 4)]
    (cap, passes), = ask([terms])
    check(terms, cap, passes)
    assert [p["index"] for p in passes] == [[0, 2, 3, 5], [1, 4]]
    assert passes[0]["zmask"] == [2, 2, 2, 4]


def test_scale_against_the_dense_operators(ask):
    """One pass as the kernel walks it -- pairs through the index with a clear pivot bit, Re c for even nY, Im c for
    odd nY, times the planner's factor -- gives <psi|P|psi> of the dense Kronecker product, for every nY mod 4."""
    n = 5
    rng = np.random.default_rng(9)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    ket /= np.linalg.norm(ket)
    strings = ["IIIII", "ZIZIZ", "XIIII", "IIYII", "YYIII", "XYZIY", "YYYIX", "YYYYI", "YYYYY", "ZXZXZ", "IIIIX", "IZIIY"]
    terms = []
    for letters in strings:
        x = sum(1 << (n - 1 - q) for q, c in enumerate(letters) if c in "XY")
        z = sum(1 << (n - 1 - q) for q, c in enumerate(letters) if c in "ZY")
        terms.append((x, z))
    (cap, passes), = ask([terms])
    check(terms, cap, passes)
    seen = set()
    idx = np.arange(1 << n)
    for p in passes:
        visit = idx if p["pivot"] < 0 else idx[(idx >> max(p["pivot"], 0)) & 1 == 0]
        c = np.conj(ket[visit ^ p["xmask"]]) * ket[visit]
        for z, n_y, t, scale in zip(p["zmask"], p["n_y"], p["index"], p["scale"]):
            sign = 1.0 - 2.0 * np.array([bin(int(i) & z).count("1") & 1 for i in visit])
            got = scale * np.sum(sign * (c.imag if n_y & 1 else c.real))
            dense = npq.tensor(*[npq.IDTY if ch == "I" else npq.PAULIS["XYZ".index(ch)] for ch in strings[t]])
            want = np.vdot(ket, dense @ ket)
            assert abs(got - want) < 1e-14 * 10, (strings[t], got, want)
            seen.add(n_y & 3 if p["pivot"] >= 0 else -1)
    assert seen == {-1, 0, 1, 2, 3}
