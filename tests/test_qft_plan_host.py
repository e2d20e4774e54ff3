"""The pass planner of ``qsv_apply_qft`` (``csrc/qsv_qft_plan.h``) on the CPU, under AddressSanitizer + UBSan.

``tests/layout/qft_plan_driver.cpp`` is a stand-alone program (text in, text out; nothing is loaded into Python).  For seeded
random registers of up to 40 qubits and the shapes of the GPU parity table the printed records are checked against the rules
restated here, ``qft_turns`` against Python integers, and -- at up to 14 qubits -- the records are executed in NumPy and
compared with the ``numpy.fft`` statement.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import hostcheck
import qft_reference as R

HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return hostcheck.compile_driver(HERE / "layout" / "qft_plan_driver.cpp", tmp_path_factory.mktemp("qft_plan"))


def cases() -> list[tuple[int, list[int], int]]:
    rng = np.random.default_rng(20)
    out = []
    for n in list(range(1, 41)) + [40, 40, 33, 27, 64]:
        m = int(rng.integers(1, n + 1))
        bits = [int(b) for b in rng.permutation(n)[:m]]
        out.append((n, bits, int(rng.integers(8))))
    for n in (12, 13, 20, 28, 40):
        out += [(n, list(range(n))[::-1], flags) for flags in (0, R.INVERSE)]      # full registers, qubit 0 on top
    for n, qubits in R.SHAPES:
        out += [(n, [n - 1 - q for q in qubits], flags) for flags in R.ALL_FLAGS]
    return out


def turns_of(index: int, bits: list[int], r: int) -> int:
    m = len(bits)
    return sum(((index >> bits[s]) & 1) << (m - 1 - s) for s in range(r + 1, m)) % (1 << (m - r))


def test_plans_follow_the_rules_and_turns_match_python_integers(driver):
    rng = np.random.default_rng(21)
    all_cases = cases()
    queries = [[int(rng.integers(1 << 62)) % (1 << n) for _ in range(6)] + [(1 << n) - 1, 0] for n, _, _ in all_cases]
    answers = hostcheck.ask(driver, [R.request(n, bits, flags, idx) for (n, bits, flags), idx in zip(all_cases, queries)])
    for (n, bits, flags), indices, line in zip(all_cases, queries, answers):
        m, passes = len(bits), R.parse_plan(line, len(indices))
        ranks = [s["rank"] for p in passes for s in p["stages"]]
        assert ranks == (list(range(m))[::-1] if flags & R.INVERSE else list(range(m)))
        assert [p["n_stages"] for p in passes] == R.greedy_counts(n, bits, flags)
        for p in passes:
            pos = p["pos"]
            assert p["tile_bits"] == min(n, 12) and len(set(pos)) == len(pos) and pos == sorted(pos) and max(pos) < n
            if n >= 12:
                assert pos[:6] == list(range(6))
            assert p["twiddle_first"] == bool(flags & R.INVERSE)
            assert p["conj_twiddle"] == (bool(flags & R.INVERSE) != bool(flags & R.CONJUGATE))
            assert p["scale"] == pytest.approx(2.0 ** (-p["n_stages"] / 2), rel=2 * R.EPS)
            if p["n_stages"] % 2 == 0:
                assert p["scale"] == 2.0 ** (-p["n_stages"] // 2)          # a power of two: exact
            for number, s in enumerate(p["stages"]):
                assert pos[s["tile_index"]] == bits[s["rank"]] and s["L"] == m - s["rank"]
                run = p["runs"][s["run"]]
                assert run["first"] <= number < run["first"] + run["count"] and run["q"][s["reg"]] == s["tile_index"]
                later = {(pos[where] if in_tile else where): shift for in_tile, where, shift in s["later"]}
                assert later == {bits[t]: m - 1 - t for t in range(s["rank"] + 1, m)}
                assert all((b in pos) == bool(in_tile) for in_tile, where, _ in s["later"] for b in [pos[where] if in_tile else where])
            covered = [i for run in p["runs"] for i in range(run["first"], run["first"] + run["count"])]
            assert covered == list(range(p["n_stages"]))
            for run in p["runs"]:
                assert 1 <= run["count"] <= 4 and run["q"] == sorted(set(run["q"])) and max(run["q"]) < p["tile_bits"]
            for index, row in zip(indices, p["turns"]):
                assert row == [turns_of(index, bits, s["rank"]) for s in p["stages"]]


def test_full_register_pass_counts(driver):
    sizes = {28: 4, 20: 3, 13: 2, 12: 1}
    answers = hostcheck.ask(driver, [R.request(n, list(range(n))[::-1], flags) for n in sizes for flags in (0, R.INVERSE)])
    counts = [len(R.parse_plan(line)) for line in answers]
    assert counts == [c for c in sizes.values() for _ in range(2)]


def test_turns_at_forty_qubits_include_the_widest_stage(driver):
    n = 40
    bits = [int(b) for b in np.random.default_rng(22).permutation(n)]
    index = (1 << n) - 1
    (line,) = hostcheck.ask(driver, [R.request(n, bits, 0, [index])])
    passes = R.parse_plan(line, 1)
    first = passes[0]["stages"][0]
    assert first["L"] == 40 and passes[0]["turns"][0][0] == (1 << 39) - 1 == turns_of(index, bits, 0)


def executed_cases():
    rng = np.random.default_rng(23)
    out = [(n, qubits) for n, qubits in R.SHAPES if n <= 14]
    for n in (3, 6, 9, 12, 13, 14, 14):
        out.append((n, [int(q) for q in rng.permutation(n)[:int(rng.integers(1, n + 1))]]))
    return out


def test_executed_records_reproduce_the_statement(driver):
    todo = [(n, qubits, flags) for n, qubits in executed_cases() for flags in R.ALL_FLAGS]
    answers = hostcheck.ask(driver, [R.request(n, [n - 1 - q for q in qubits], flags) for n, qubits, flags in todo])
    kets = {}
    for (n, qubits, flags), line in zip(todo, answers):
        ket = kets.setdefault(n, R.random_ket(n, 100 + n))
        got = R.run_plan_with_swaps(ket, qubits, flags, R.parse_plan(line))
        want = R.qft_statement(ket, qubits, flags)
        err, bound = np.linalg.norm(got - want), 8 * len(qubits) * R.EPS
        print(f"n={n} m={len(qubits)} flags={flags}: l2 error {err:.2e} / bound {bound:.2e}")
        assert err <= bound
