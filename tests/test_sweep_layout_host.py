"""The launch rules of the per-member parameter kernels (quantum_computations_amd/csrc/qsv_sweep_layout.h), on the host only.

tests/layout/sweep_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan into a program of its own,
as the other layout tests compile theirs; nothing is loaded into Python.  For members of n = 1 .. 26 qubits, 2^b members with
b = 0 .. 12 and n + b <= 30, every pivot and the diagonal form, grid caps 0, 1 and 2: every amplitude of every member is owned
by exactly one (member, part, item); both amplitudes of a pair lie in the owner's member; the table offset of
(member, pass, t) stays inside the table; the grid is within its limits; the parts per member do not depend on b; and where
the header says a wave or a unit lies in one member, it does.
"""
from __future__ import annotations

import pytest

import hostcheck

BLOCK_BITS, MAX_BLOCKS, READ_ITEM_BITS, MAX_PART_BITS = 8, (1 << 24) - 1, 5, 7


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "sweep_layout_driver.cpp", tmp_path_factory.mktemp("sweep_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=900)
        return [[[int(x) for x in part.split()] for part in line.split("|")] for line in lines]
    return run


def cases():
    return [(n, b, pivot, cap) for n in range(1, 27) for b in range(0, 13) if n + b <= 30 for pivot in range(-1, n) for cap in (0, 1, 2)]


def test_every_amplitude_has_one_owner_inside_its_member(ask):
    todo = cases()
    answers = ask([f"case {n} {b} {pivot} {cap}" for n, b, pivot, cap in todo])
    parts_of = {}
    waves, units_uniform = set(), set()
    for (n, b, pivot, cap), (shape, found) in zip(todo, answers):
        item_bits, pbits, sbits, units, grid, wave, unit = shape
        members = 1 << b
        assert item_bits == (n if pivot < 0 else n - 1)
        cap_bits = (cap.bit_length() - 1) if cap else 99
        share = max(BLOCK_BITS - item_bits, 0)
        assert pbits == min(max(item_bits - BLOCK_BITS, 0), cap_bits) and sbits == share
        assert units == max(members >> share, 1) << pbits
        assert 1 <= grid <= min(units, MAX_BLOCKS) and (cap == 0 or grid <= cap)
        assert wave == (1 if item_bits >= 6 else 0) and unit == (1 if item_bits >= BLOCK_BITS else 0)
        # how a member is cut depends on n, the form and the cap alone
        assert parts_of.setdefault((n, pivot < 0, cap), pbits) == pbits
        checked, cover_min, cover_max, bad_owner, bad_member, bad_table, bad_uniform = found
        assert checked > 0 and (cover_min, cover_max) == (1, 1), (n, b, pivot, cap, found)
        assert (bad_owner, bad_member, bad_table, bad_uniform) == (0, 0, 0, 0), (n, b, pivot, cap, found)
        if (members << n) <= 1 << 12:
            assert checked == members << n                               # walked whole
        waves.add(wave)
        units_uniform.add(unit)
    assert waves == {0, 1} and units_uniform == {0, 1}                    # all three kinds of unit were met


def test_the_read_pass_of_the_moments(ask):
    todo = [(n, b, cap) for n in range(0, 27) for b in range(0, 13) if n + b <= 30 for cap in (0, 1, 2)]
    answers = ask([f"expect {n} {b} {cap}" for n, b, cap in todo])
    parts_of = {}
    for (n, b, cap), ((item_bits, pbits, sbits, units, grid, values, doubles),) in zip(todo, answers):
        members = 1 << b
        cap_bits = (cap.bit_length() - 1) if cap else 99
        assert item_bits == n and sbits == max(BLOCK_BITS - n, 0)
        assert pbits == min(max(n - BLOCK_BITS - READ_ITEM_BITS, 0), MAX_PART_BITS, cap_bits)
        assert parts_of.setdefault((n, cap), pbits) == pbits              # never on the number of members
        assert units == max(members >> sbits, 1) << pbits and 1 <= grid <= min(units, MAX_BLOCKS)
        assert values == 4 * members and doubles == values + 4 * (members << pbits)


def test_table_sizes(ask):
    assert ask(["table 19 4096", "table 1 1", "table 0 8"]) == [[[2 * 19 * 4096 + 16]], [[2 + 16]], [[0]]]      # 16 doubles of padding
