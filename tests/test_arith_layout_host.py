"""The host side of ``qsv_apply_arith`` (``csrc/qsv_arith_layout.h``) on the CPU, under AddressSanitizer + UBSan.

``tests/layout/arith_layout_driver.cpp`` is a stand-alone program (text in, text out; nothing is loaded into Python).
Checked here against rules restated in Python: operand segments, the form per lowest operand bit, launch shapes for 3 to 34
qubits, the division-free reduction against Python integers, modular inverses, table inversion, every refusal of
``qsv_arith_create`` -- and the kernel's whole index computation (``arith_source`` walked as ``k_arith`` walks it) against
the statement of ``tests/arith_reference.py`` for every GPU case of up to 14 qubits.
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import pytest

import arith_reference as R
import hostcheck

HERE = Path(__file__).resolve().parent
KIND = {name: k for k, name in enumerate(R.KINDS)}
SMALL, LINE, ELEMENT = 0, 1, 2
SHIFT, MULT, XOR, TABLE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return hostcheck.compile_driver(HERE / "layout" / "arith_layout_driver.cpp", tmp_path_factory.mktemp("arith_layout"))


def create_args(spec: dict) -> str:
    table = spec["table"] or []
    modulus = spec["M"] if spec["kind"] in R.MODULAR else 0
    return (f"{KIND[spec['kind']]} {spec['m']} {spec['mx']} {spec['a']} {spec['c']} {modulus} {int(spec['table'] is not None)} "
            f"{len(table)} " + " ".join(map(str, table))).strip()


def raw_create(kind, m, mx, a=0, c=0, modulus=0, table=None, length=None) -> str:
    table_len = len(table) if length is None and table is not None else (length or 0)
    return f"create {kind} {m} {mx} {a} {c} {modulus} {int(table is not None)} {table_len} " + " ".join(map(str, (table or [])[:table_len]))


def test_segments_of_contiguous_reversed_and_scattered_operands(driver):
    operands = {"contiguous": [9, 8, 7, 6, 5], "reversed": [5, 6, 7, 8, 9], "scattered": [11, 3, 7, 0], "one": [4], "two runs": [13, 12, 3, 2, 1],
                "wide": list(range(31, -1, -1)), "wide scattered": list(range(0, 64, 2))[::-1]}
    answers = hostcheck.ask(driver, [f"seg {len(bits)} " + " ".join(map(str, bits)) for bits in operands.values()])
    for (name, bits), line in zip(operands.items(), answers):
        numbers = hostcheck.nums(line.split())
        segs = [tuple(numbers[1 + 3 * k:4 + 3 * k]) for k in range(numbers[0])]
        m = len(bits)
        # every value bit j is covered once, at the index bit the operand lists for it
        covered = {j + d: pos + d for pos, j, length in segs for d in range(length)}
        assert covered == {j: bits[m - 1 - j] for j in range(m)}, name
        assert sum(length for _, _, length in segs) == m
        # merged as far as possible: neighbouring segments do not continue each other
        for (p0, j0, l0), (p1, j1, _) in zip(segs, segs[1:]):
            assert j1 == j0 + l0 and p1 != p0 + l0
    counts = {name: int(line.split()[0]) for name, line in zip(operands, answers)}
    assert counts == {"contiguous": 1, "reversed": 5, "scattered": 4, "one": 1, "two runs": 2, "wide": 1, "wide scattered": 32}


def test_form_for_each_lowest_operand_bit(driver):
    # the lowest bit among target, source and controls: a low source or control bit splits a destination line as a low target bit does
    requests = [(n, t0) for n in (3, 13, 14, 28, 34) for t0 in range(6) if t0 < n]
    answers = hostcheck.ask(driver, [f"form {n} {t0}" for n, t0 in requests])
    for (n, t0), line in zip(requests, answers):
        assert int(line) == (SMALL if n < 14 else LINE if t0 >= 3 else ELEMENT), (n, t0)


def test_launch_shapes_from_3_to_34_qubits(driver):
    rng = np.random.default_rng(261)
    requests = []
    for n in range(3, 35):
        for _ in range(4):
            m = int(rng.integers(1, min(n, 32) + 1))
            bits = [int(b) for b in rng.permutation(n)]
            tmask = sum(1 << b for b in bits[:m])
            used = tmask | sum(1 << b for b in bits[m:m + int(rng.integers(0, n - m + 1))])
            requests.append((n, tmask, used, int(rng.integers(0, 3))))
        requests.append((n, 1 << (n - 1), 1 << (n - 1), 2))            # one high target bit: the most spectators
        requests.append((n, (1 << n) - 1 if n <= 32 else (1 << 32) - 1, (1 << n) - 1, 2))       # no spectator at all
    answers = hostcheck.ask(driver, [f"shape {n} {used} {items}" for n, tmask, used, items in requests])
    for (n, tmask, used, max_items), line in zip(requests, answers):
        form, items, bit0, bit1, W, grid, block = hostcheck.nums(line.split())
        d0 = (used & -used).bit_length() - 1
        assert tmask & used == tmask and form == (SMALL if n < 14 else LINE if d0 >= 3 else ELEMENT)
        spectators = [b for b in range(6, n) if not (used >> b) & 1] if n >= 14 else []
        assert items == min(max_items, 2, len(spectators)) and [bit0, bit1][:items] == spectators[:items]
        assert W == (1 << n) >> items and block == 256
        assert 1 <= grid <= 1 << 20 and grid * block < 1 << 32 and grid == min(-(-W // block), 1 << 20)
        assert grid * block >= min(W, 1 << 28)       # one sweep covers the register up to 2^28 work items; beyond, threads stride


def test_reduction_against_python_integers(driver):
    rng = np.random.default_rng(262)
    triples = []
    for M in (2, 3, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32):
        triples += [(M, M - 1, M - 1), (M, 0, 0), (M, 1, M - 1), (M, M - 1, 1), (M, 2 ** 64 - 1, 1), (M, 2 ** 63, 1), (M, M, 1), (M, 2 * M - 1, 1)]
        triples += [(M, int(rng.integers(0, M)), int(rng.integers(0, M))) for _ in range(4000)]
    while len(triples) < 100_000 + 40:
        M = int(rng.integers(2, 2 ** 32 + 1)) if rng.random() < 0.7 else int(2 ** rng.integers(1, 33)) - int(rng.integers(0, 2))
        M = max(M, 2)
        triples.append((M, int(rng.integers(0, M)), int(rng.integers(0, M))))
    (line,) = hostcheck.ask(driver, [f"triples {len(triples)} " + " ".join(f"{M} {a} {y}" for M, a, y in triples)])
    numbers = hostcheck.nums(line.split())
    for k, (M, a, y) in enumerate(triples):
        assert numbers[2 * k] == 2 ** 64 // M, M
        assert numbers[2 * k + 1] == (a * y) % M, (M, a, y)


def test_modular_inverses(driver):
    rng = np.random.default_rng(263)
    pairs = [(1, 2), (1, 3), (2, 3), (7, 15), (2 ** 32 - 1, 2 ** 32), (2 ** 31 - 2, 2 ** 31 - 1), (3, 2 ** 32), (6, 15), (4, 2 ** 32), (5, 10)]
    while len(pairs) < 2000:
        M = int(rng.integers(2, 2 ** 32 + 1))
        pairs.append((int(rng.integers(1, M)), M))
    answers = hostcheck.ask(driver, [f"inv {a} {M}" for a, M in pairs])
    for (a, M), line in zip(pairs, answers):
        assert int(line) == (pow(a, -1, M) if math.gcd(a, M) == 1 else 0), (a, M)


def test_table_inversion(driver):
    rng = np.random.default_rng(264)
    tables = [[0], [1, 0], [int(v) for v in rng.permutation(64)], [int(v) for v in rng.permutation(1 << 12)], [0, 0], [0, 2], [1, 2, 3, 1]]
    answers = hostcheck.ask(driver, [f"tinv {len(t)} " + " ".join(map(str, t)) for t in tables])
    for table, line in zip(tables, answers):
        numbers = hostcheck.nums(line.split())
        if sorted(table) == list(range(len(table))):
            assert numbers[0] == 1 and [numbers[1 + table[y]] for y in range(len(table))] == list(range(len(table)))
        else:
            assert numbers == [0]


def test_every_refusal_of_create(driver):
    ADD, MUL, ADD_REG, MUL_POW, XOR_LOOKUP, PERMUTE = range(6)
    perm = [2, 0, 3, 1]
    refused = {
        "unknown kind": [raw_create(6, 2, 0), raw_create(-1, 2, 0)],
        "m out of range": [raw_create(ADD, 0, 0, c=0), raw_create(ADD, 33, 0, c=1), raw_create(PERMUTE, 25, 0, table=[0], length=1), raw_create(MUL, -1, 0, a=1)],
        "mx out of range": [raw_create(ADD_REG, 4, 0, a=1), raw_create(ADD_REG, 4, 33, a=1), raw_create(MUL_POW, 4, 25, a=3), raw_create(XOR_LOOKUP, 2, 0, table=[1]),
                            raw_create(XOR_LOOKUP, 2, 25, table=[1]), raw_create(ADD, 4, 1, c=1), raw_create(MUL, 4, 2, a=3), raw_create(PERMUTE, 2, 1, table=perm)],
        "modulus": [raw_create(ADD, 4, 0, c=0, modulus=1), raw_create(ADD, 4, 0, c=1, modulus=17), raw_create(MUL, 32, 0, a=1, modulus=2 ** 32 + 1),
                    raw_create(XOR_LOOKUP, 1, 1, table=[0, 1], modulus=2), raw_create(PERMUTE, 2, 0, table=perm, modulus=4)],
        "a out of range": [raw_create(MUL, 4, 0, a=16), raw_create(MUL, 4, 0, a=15, modulus=15), raw_create(ADD_REG, 4, 2, a=13, modulus=13), raw_create(MUL_POW, 4, 2, a=16),
                           raw_create(ADD, 4, 0, a=1, c=1), raw_create(XOR_LOOKUP, 1, 1, a=1, table=[0, 1]), raw_create(PERMUTE, 2, 0, a=1, table=perm)],
        "c out of range": [raw_create(ADD, 4, 0, c=16), raw_create(ADD, 4, 0, c=13, modulus=13), raw_create(ADD_REG, 4, 2, a=1, c=2 ** 40), raw_create(MUL, 4, 0, a=3, c=1),
                           raw_create(MUL_POW, 4, 2, a=3, c=1), raw_create(XOR_LOOKUP, 1, 1, c=1, table=[0, 1])],
        "not coprime": [raw_create(MUL, 4, 0, a=0), raw_create(MUL, 4, 0, a=6), raw_create(MUL, 4, 0, a=5, modulus=15), raw_create(MUL_POW, 4, 3, a=3, modulus=15),
                        raw_create(MUL_POW, 4, 3, a=0)],
        "table": [raw_create(XOR_LOOKUP, 2, 1, table=[1, 4]), raw_create(PERMUTE, 2, 0, table=[0, 1, 2, 4]), raw_create(PERMUTE, 2, 0, table=[0, 1, 1, 2]),
                  raw_create(XOR_LOOKUP, 2, 2, table=[1, 2, 3]), raw_create(PERMUTE, 2, 0, table=perm + [0]), raw_create(PERMUTE, 2, 0, table=perm[:3]),
                  raw_create(XOR_LOOKUP, 2, 1), raw_create(PERMUTE, 2, 0), raw_create(ADD, 2, 0, c=1, table=[1], length=1)],
    }
    flat = [(group, request) for group, requests in refused.items() for request in requests]
    answers = hostcheck.ask(driver, [request for _, request in flat])
    for (group, request), line in zip(flat, answers):
        assert line.startswith("refused: ") and len(line) > len("refused: ") + 8, (group, request, line)
    accepted = [raw_create(ADD, 32, 0, c=2 ** 32 - 1), raw_create(MUL, 32, 0, a=2 ** 32 - 1), raw_create(MUL, 1, 0, a=1), raw_create(ADD, 4, 0, c=0, modulus=2),
                raw_create(ADD_REG, 32, 32, a=2 ** 32 - 2, c=5, modulus=2 ** 32 - 1), raw_create(MUL_POW, 5, 3, a=2, modulus=21), raw_create(PERMUTE, 2, 0, table=perm),
                raw_create(XOR_LOOKUP, 2, 1, table=[3, 0])]
    for line in hostcheck.ask(driver, accepted):
        assert line.startswith("ok ")


def parse_created(line: str):
    numbers = hostcheck.nums(line.split()[1:])
    M, pow2, recip = numbers[:3]
    sets, at = [], 3
    for _ in range(2):
        body, a, c, identity, length = numbers[at:at + 5]
        sets.append({"body": body, "a": a, "c": c, "identity": bool(identity), "table": numbers[at + 5:at + 5 + length]})
        at += 5 + length
    assert at == len(numbers)
    return M, bool(pow2), recip, sets


def test_both_parameter_sets_of_every_kind(driver):
    specs = [c["spec"] for c in R.cases() if c["spec"]["m"] + c["spec"]["mx"] <= 10]
    answers = hostcheck.ask(driver, ["create " + create_args(spec) for spec in specs])
    for spec, line in zip(specs, answers):
        M, pow2, recip, (own, inverse) = parse_created(line)
        m, mx, kind = spec["m"], spec["mx"], spec["kind"]
        assert M == spec["M"] and pow2 == (M == 1 << m) and recip == 2 ** 64 // M
        assert own["identity"] == inverse["identity"] == R.is_identity(spec)
        if kind in ("add", "add_register"):
            assert own["body"] == inverse["body"] == SHIFT and (own["a"], own["c"]) == (spec["a"], spec["c"])
            assert (inverse["a"], inverse["c"]) == ((M - spec["a"]) % M, (M - spec["c"]) % M)
        elif kind == "multiply":
            assert own["body"] == inverse["body"] == MULT and own["a"] == spec["a"] and inverse["a"] * spec["a"] % M == 1 % M and not own["table"]
        elif kind == "modexp":
            assert own["table"] == [pow(spec["a"], x, M) for x in range(1 << mx)]
            assert [f * g % M for f, g in zip(own["table"], inverse["table"])] == [1 % M] * (1 << mx)
        elif kind == "xor_lookup":
            assert own["body"] == XOR and own["table"] == inverse["table"] == spec["table"]
        else:
            assert own["body"] == TABLE and own["table"] == spec["table"] and [own["table"][v] for v in inverse["table"]] == list(range(1 << m))


@pytest.mark.parametrize("max_items", [0, 1, 2])
def test_the_kernels_index_walk_reproduces_the_statement(driver, max_items):
    cases = [c for c in R.cases() if c["n"] <= 14]
    if max_items < 2:
        cases = [c for c in cases if c["n"] == 14][::2]
    requests, wanted = [], []
    for c in cases:
        for inverse in (0, 1):
            words = ["gather", create_args(c["spec"]), inverse, c["n"], max_items, *c["tbits"], *c["sbits"], len(c["cbits"]), *c["cbits"]]
            requests.append(" ".join(map(str, words)))
            j = R.destination(c["n"], c["spec"], c["target"], c["source"], c["controls"])      # forward: out[j[i]] = ket[i]
            if inverse:
                wanted.append(j)                        # out[i] = ket[j[i]]
            else:
                back = np.empty_like(j)
                back[j] = np.arange(j.size)
                wanted.append(back)                     # out[i] = ket[j^-1[i]]
    answers = hostcheck.ask(driver, requests)
    for c, line, want in zip([c for c in cases for _ in range(2)], answers, wanted):
        assert np.array_equal(np.array(line.split(), dtype=np.int64), want), c["id"]
