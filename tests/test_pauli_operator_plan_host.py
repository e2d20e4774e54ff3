"""The argument builders of qsv_apply_pauli_sum and qsv_pauli_rotations_adjoint (``pauli_sum_apply_passes`` and
``pauli_adjoint_passes`` in quantum_computations_amd/csrc/qsv_readout_layout.h), on the host.

tests/pauli_plan/operator_plan_driver.cpp is a stand-alone program compiled against the headers with AddressSanitizer +
UBSan exactly as tests/test_pauli_rotation_plan_host.py compiles its driver; term lists go in as text and the kernel
arguments of every launch come back as text (doubles as hex floats: compared exactly).  Every launch is compared with
the Python model in tests/pauli_operator_reference.py: the pivot on the highest flipped bit, ``items``,
``d_t = c_t i^{nY}``, the odd-``nY`` bits, ``FIRST`` on exactly the first pass of a call that overwrites, the reversed
order and negated sines of the backward walk, and 64-bit item counts at 33 / 34 qubits.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck
import pauli_operator_reference as P

CAP = 8


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "pauli_plan" / "operator_plan_driver.cpp", tmp_path_factory.mktemp("pauli_operator_plan"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=600)
        answers = []
        for line in lines:
            head, *parts = [part.split() for part in line.split("|")]
            assert int(head[0]) == len(parts)
            answers.append(parts)
        return answers
    return run


def ask_sum(ask, cases):
    """cases: [(amps, accumulate, [(xmask, zmask)], [complex])] -> the launches of each, parsed."""
    requests = []
    for amps, accumulate, terms, coeffs in cases:
        body = [f"{x:x} {z:x} {complex(c).real.hex()} {complex(c).imag.hex()}" for (x, z), c in zip(terms, coeffs)]
        requests.append(" ".join([f"S {amps:x} {int(accumulate)} {len(terms)}"] + body))
    out = []
    for parts in ask(requests):
        launches = []
        for tokens in parts:
            assert len(tokens) == 7 + 3 * CAP
            slots = [tokens[7 + 3 * t:10 + 3 * t] for t in range(CAP)]
            launches.append({"ok": int(tokens[0]), "xmask": int(tokens[1], 16), "pivot": int(tokens[2]), "items": int(tokens[3], 16),
                             "odd": int(tokens[4], 16), "width": int(tokens[5]), "first": bool(int(tokens[6])),
                             "zmask": [int(s[0], 16) for s in slots],
                             "d": [complex(float.fromhex(s[1]), float.fromhex(s[2])) for s in slots]})
        out.append(launches)
    return out


def check_sum(case, launches):
    amps, accumulate, terms, coeffs = case
    want = P.apply_launches(terms, coeffs, amps, accumulate)
    assert len(launches) == len(want)
    for got, model in zip(launches, want):
        count = len(model["d"])
        assert got["ok"] == 1
        for key in ("xmask", "pivot", "items", "odd", "width", "first"):
            assert got[key] == model[key], (key, got, model)
        assert got["zmask"] == model["zmask"] + [0] * (CAP - count)
        assert got["d"] == model["d"] + [0j] * (CAP - count)                   # exactly: i^{nY} is a swap and signs
        assert 1 <= count <= got["width"] <= CAP
        if got["xmask"]:
            assert got["pivot"] == got["xmask"].bit_length() - 1 and got["items"] * 2 == amps     # the HIGHEST flipped bit
    assert [l["first"] for l in launches] == [not accumulate and k == 0 for k in range(len(launches))]


def ask_adjoint(ask, cases):
    """cases: [(amps, [(xmask, zmask)], cs, sn)]."""
    requests = []
    for amps, terms, cs, sn in cases:
        body = [f"{x:x} {z:x} {float(c).hex()} {float(s).hex()}" for (x, z), c, s in zip(terms, cs, sn)]
        requests.append(" ".join([f"A {amps:x} {len(terms)}"] + body))
    out = []
    for parts in ask(requests):
        launches = []
        for tokens in parts:
            assert len(tokens) == 7 + 5 * CAP
            slots = [tokens[7 + 5 * t:12 + 5 * t] for t in range(CAP)]
            launches.append({"ok": int(tokens[0]), "xmask": int(tokens[1], 16), "pivot": int(tokens[2]), "items": int(tokens[3], 16),
                             "diag": int(tokens[4], 16), "rot": int(tokens[5], 16), "width": int(tokens[6]),
                             "index": [int(s[0]) for s in slots], "n_y": [int(s[1]) for s in slots],
                             "zmask": [int(s[2], 16) for s in slots], "cs": [float.fromhex(s[3]) for s in slots],
                             "sn": [float.fromhex(s[4]) for s in slots]})
        out.append(launches)
    return out


def check_adjoint(case, launches):
    amps, terms, cs, sn = case
    want = P.adjoint_launches(terms, cs, sn, amps)
    assert len(launches) == len(want) == len(P.R.plan(terms))                  # the forward count
    for got, model in zip(launches, want):
        count = len(model["index"])
        pad = CAP - count
        assert got["ok"] == 1
        for key in ("xmask", "pivot", "items", "width"):
            assert got[key] == model[key], (key, got, model)
        assert got["index"] == model["index"] + [-1] * pad
        assert got["n_y"] == model["n_y"] + [0] * pad
        assert got["zmask"] == model["zmask"] + [0] * pad
        assert got["cs"] == model["cs"] + [1.0] * pad and got["sn"] == model["sn"] + [0.0] * pad       # -theta; padding: theta = 0
        assert got["diag"] == sum(1 << t for t in range(CAP) if t >= count or model["diag"][t])
        assert got["rot"] == sum((model["n_y"][t] & 3) << (2 * t) for t in range(count) if not model["diag"][t])
    visited = [t for l in launches for t in l["index"] if t >= 0]
    assert visited == list(range(len(terms)))[::-1]                            # every term once, the last first


def random_case(rng, n, count, pool_size=3):
    pool = [0] + [int(rng.integers(1, 1 << n)) for _ in range(pool_size)]
    terms = [(pool[int(rng.integers(len(pool)))], int(rng.integers(0, 1 << n))) for _ in range(count)]
    coeffs = [complex(rng.standard_normal(), rng.standard_normal()) for _ in range(count)]
    return terms, coeffs


def test_sum_launches_follow_the_model(ask):
    rng = np.random.default_rng(5)
    cases = [(8, False, [], []), (8, True, [], []), (2, False, [(1, 1)], [2.0 - 1j]), (2, True, [(0, 0)], [1j])]
    for n in (1, 2, 3, 7, 14, 28, 33, 34, 40):
        for count in (1, 2, 5, 9, 40):
            for accumulate in (False, True):
                terms, coeffs = random_case(rng, n, count)
                cases.append((1 << n, accumulate, terms, coeffs))
    for count in (1, 2, 3, 4, 5, 8, 9, 17):                                    # one xmask, and diagonal: padding and the second pass
        cases.append((1 << 7, False, [(0b1011010, int(rng.integers(0, 128))) for _ in range(count)], [1.0 + t for t in range(count)]))
        cases.append((1 << 7, False, [(0, t) for t in range(count)], [1j * (t + 1) for t in range(count)]))
    answers = ask_sum(ask, cases)
    for case, launches in zip(cases, answers):
        check_sum(case, launches)
    assert answers[0] == [] and answers[1] == []
    assert answers[2][0]["d"][0] == 1j * (2.0 - 1j) and answers[2][0]["odd"] == 1 and answers[2][0]["first"]
    assert not answers[3][0]["first"]


def test_every_power_of_i_and_the_odd_bits(ask):
    x = 0b11110
    terms = [(x, 0b00000), (x, 0b00010), (x, 0b00110), (x, 0b01110), (x, 0b11110), (x, 0b11111)]
    coeffs = [1 + 2j] * 6
    (launches,) = ask_sum(ask, [(32, False, terms, coeffs)])
    assert len(launches) == 1 and launches[0]["pivot"] == 4 and launches[0]["odd"] == 0b001010
    assert launches[0]["d"][:6] == [1 + 2j, -2 + 1j, -1 - 2j, 2 - 1j, 1 + 2j, 1 + 2j]
    check_sum((32, False, terms, coeffs), launches)


def test_item_counts_at_33_and_34_qubits(ask):
    top33, top34 = 1 << 32, 1 << 33
    cases = [(1 << 33, False, [(top33 | 1, 0), (0, top33)], [1.0, 1.0]), (1 << 34, True, [(top34, top34), (0, 1)], [1.0, 1.0])]
    answers = ask_sum(ask, cases)
    assert [l["items"] for l in answers[0]] == [1 << 32, 1 << 33] and answers[0][0]["pivot"] == 32
    assert [l["items"] for l in answers[1]] == [1 << 33, 1 << 34] and answers[1][0]["pivot"] == 33
    walk = ask_adjoint(ask, [(1 << 34, [(top34 | 2, 0), (1, 1), (0, top34)], [0.5, 0.6, 0.7], [0.1, 0.2, 0.3])])[0]
    assert [l["items"] for l in walk] == [1 << 33, 1 << 33] and [l["pivot"] for l in walk] == [0, 33]
    for case, launches in zip(cases, answers):
        check_sum(case, launches)


def test_a_mask_outside_the_register_is_refused(ask):
    (launches,) = ask_sum(ask, [(8, False, [(0b1000, 0)], [1.0])])
    assert [l["ok"] for l in launches] == [0]
    (walk,) = ask_adjoint(ask, [(8, [(0b1000, 0)], [1.0], [0.0])])
    assert [l["ok"] for l in walk] == [0]


def test_adjoint_launches_are_the_forward_plan_backwards(ask):
    rng = np.random.default_rng(6)
    cases = [(8, [], [], [])]
    for n in (1, 2, 3, 7, 14, 28, 34):
        for count in (1, 2, 9, 40, 100):
            terms, _ = random_case(rng, n, count, pool_size=2)
            thetas = rng.uniform(-3, 3, size=count)
            cases.append((1 << n, terms, np.cos(thetas / 2).tolist(), np.sin(thetas / 2).tolist()))
    x = 0b101000
    cases.append((64, [(0, 1)] * 9 + [(x, 0), (x, x), (0, x), (x, 1)], [0.1 * t for t in range(13)], [0.05 * t for t in range(13)]))
    answers = ask_adjoint(ask, cases)
    for case, launches in zip(cases, answers):
        check_adjoint(case, launches)
    assert answers[0] == []
    last = answers[-1]
    assert [l["index"][:5] for l in last] == [[12, 11, 10, 9, 8], [7, 6, 5, 4, 3]]
    assert last[0]["n_y"][:5] == [0, 0, 2, 0, 0] and last[0]["pivot"] == 5 and last[1]["xmask"] == 0
