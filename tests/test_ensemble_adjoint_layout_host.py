"""The launch rules of the per-member adjoint walk (the adjoint part of quantum_computations_amd/csrc/qsv_sweep_layout.h), on the
host only.

tests/layout/ensemble_adjoint_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan into a program of
its own, as the other layout tests compile theirs; nothing is loaded into Python.  For members of n = 1 .. 26 qubits, 2^b
members with b = 0 .. 12 and n + b <= 30, every pivot and the diagonal form, grid caps 0, 1 and 2: every amplitude of both
registers is owned by exactly one (member, part, item); both amplitudes of a pair lie in the owner's member; every table offset
a thread reads -- the threads of a member beyond the last included, which fetch the last member's row -- is inside the table;
every partial slot is inside the workspace's ``[members][P_max][16]``; and the parts per member do not depend on b.
"""
from __future__ import annotations

import pytest

import hostcheck

BLOCK_BITS, MAX_BLOCKS, READ_ITEM_BITS, MAX_PART_BITS = 8, (1 << 24) - 1, 5, 7


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "ensemble_adjoint_layout_driver.cpp", tmp_path_factory.mktemp("ensemble_adjoint_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=900)
        return [[part.split() for part in line.split("|")] for line in lines]
    return run


def part_bits(item_bits, cap):
    cap_bits = (cap.bit_length() - 1) if cap else 99
    return min(max(item_bits - BLOCK_BITS - READ_ITEM_BITS, 0), MAX_PART_BITS, cap_bits)


def test_every_amplitude_has_one_owner_and_every_fetch_and_partial_is_in_bounds(ask):
    todo = [(n, b, pivot, cap) for n in range(1, 27) for b in range(0, 13) if n + b <= 30 for pivot in range(-1, n) for cap in (0, 1, 2)]
    answers = ask([f"case {n} {b} {pivot} {cap}" for n, b, pivot, cap in todo])
    parts_of, waves = {}, set()
    for (n, b, pivot, cap), (shape, found) in zip(todo, answers):
        item_bits, pbits, sbits, units, grid, wave = (int(x) for x in shape)
        members = 1 << b
        assert item_bits == (n if pivot < 0 else n - 1)
        share = max(BLOCK_BITS - item_bits, 0)
        assert pbits == part_bits(item_bits, cap) and sbits == share           # the cut of a read pass
        assert pbits <= part_bits(n, 0)                                        # at most the workspace's P_max(n)
        assert units == max(members >> share, 1) << pbits
        assert 1 <= grid <= min(units, MAX_BLOCKS) and (cap == 0 or grid <= cap)
        assert wave == (1 if item_bits >= 6 else 0)
        # how a member is cut depends on n, the form and the cap alone
        assert parts_of.setdefault((n, pivot < 0, cap), pbits) == pbits
        checked, cover_min, cover_max, bad_owner, bad_member, bad_table, bad_partial, bad_fit = (int(x) for x in found)
        assert checked > 0 and (cover_min, cover_max) == (1, 1), (n, b, pivot, cap, found)
        assert (bad_owner, bad_member, bad_table, bad_partial, bad_fit) == (0, 0, 0, 0, 0), (n, b, pivot, cap, found)
        if (members << n) <= 1 << 12:
            assert checked == members << n                                     # walked whole, each register once
        waves.add(wave)
    assert waves == {0, 1}


def test_the_read_passes_of_the_inner_product_and_the_cost_phase_walk(ask):
    todo = [(n, b, cap) for n in range(0, 27) for b in range(0, 13) if n + b <= 30 for cap in (0, 1, 2)]
    answers = ask([f"pair {n} {b} {cap}" for n, b, cap in todo])
    parts_of = {}
    for (n, b, cap), (shape, found) in zip(todo, answers):
        item_bits, pbits, sbits, units, grid = (int(x) for x in shape)
        members = 1 << b
        assert item_bits == n and sbits == max(BLOCK_BITS - n, 0) and pbits == part_bits(n, cap)
        assert parts_of.setdefault((n, cap), pbits) == pbits                   # never on the number of members
        assert units == max(members >> sbits, 1) << pbits and 1 <= grid <= min(units, MAX_BLOCKS)
        assert [int(x) for x in found] == [0, 0], (n, b, cap, found)


def test_some_gpu_size_has_two_parts_and_a_looping_grid_in_each_form(ask):
    (sizes,), = ask(["gpusizes"])
    print("GPU sizes with parts >= 2 and grid < units:", " ".join(sizes))
    assert any(s.endswith(":diag") for s in sizes) and any(s.endswith(":flip") for s in sizes)
    assert all(int(s.split(":")[0]) <= 16 for s in sizes)
