"""The predicate rule of the ensemble's conditional gate (quantum_computations_amd/csrc/qsv_ensemble_control_layout.h), on the host only.

tests/layout/ensemble_control_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan into a program of
its own, as the other layout tests compile theirs.  For members of n = 1 .. 26 qubits, 2^b members with b = 0 .. 12 and
n + b <= 30, every target bit and every ordered pair of target bits, grid caps 0, 1 and 2, the lane and the round-1 forms:
every amplitude of a member that takes the gate is owned by exactly one (unit, thread, item) and no amplitude of any other
member by anyone; every ``shfl_xor`` partner of a lane tests the word of the lane's own member, so it has the same predicate;
a unit that lies in one member has a member index that is a function of the unit alone, and the chunked walk in which a
workgroup fetches the words of up to 64 consecutive units at once visits every unit exactly once.
"""
from __future__ import annotations

import pytest

import hostcheck

BLOCK_BITS, LANE_BITS, MAX_BLOCKS, MAX_CHUNK_BITS, MIN_GRID_BITS = 8, 6, (1 << 24) - 1, 6, 11


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "ensemble_control_layout_driver.cpp", tmp_path_factory.mktemp("ensemble_control_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=900)
        return [[[int(x) for x in part.split()] for part in line.split("|")] for line in lines]
    return run


def cases():
    out = []
    for n in range(1, 27):
        placements = [(b0,) for b0 in range(n)] + [(b0, b1) for b0 in range(n) for b1 in range(n) if b0 != b1]
        for b in range(0, 13):
            if n + b > 30:
                continue
            for bits in placements:
                for cap in (0, 1, 2):
                    out.append((n, b, bits, 1, cap))
            if b in (0, 3):                                            # the round-1 forms: no lane bits at any size
                out += [(n, b, bits, 0, 0) for bits in placements]
    return out


def test_takers_are_covered_once_non_takers_never_and_partners_share_the_predicate(ask):
    todo = cases()
    answers = ask([f"case {n} {b} {len(bits)} {bits[0]} {bits[1] if len(bits) > 1 else -1} {lanes} {cap}" for n, b, bits, lanes, cap in todo])
    forms = set()
    for (n, b, bits, lanes, cap), a in zip(todo, answers):
        head, shape, found = a
        kh, kl, item_bits = head
        members, k = 1 << b, len(bits)
        want_kl = sum(1 for bit in bits if bit < LANE_BITS) if (lanes and n >= LANE_BITS) else 0
        assert (kh, kl) == (k - want_kl, want_kl), (n, bits, lanes)
        assert item_bits == n - kh
        pbits, sbits, units, grid, uniform, lanes_safe, chunk_bits = shape
        cap_bits = (cap.bit_length() - 1) if cap else 99
        share = max(BLOCK_BITS - item_bits, 0)
        assert pbits == min(max(item_bits - BLOCK_BITS, 0), cap_bits) and sbits == share
        assert units == max(members >> share, 1) << pbits
        # chunks of consecutive units where a unit lies in one member: none up to 2^11 units, then as many as keep 2^11
        # workgroups, at most the 64 lanes of a wave
        want_chunk = min(max(units.bit_length() - 1 - MIN_GRID_BITS, 0), MAX_CHUNK_BITS) if item_bits >= BLOCK_BITS else 0
        assert chunk_bits == want_chunk
        assert grid == min(units >> chunk_bits, MAX_BLOCKS, cap or MAX_BLOCKS)
        if cap:
            assert grid <= cap
        # one word per unit exactly where a unit lies in one member; a per-thread predicate everywhere else
        assert uniform == (1 if item_bits >= BLOCK_BITS else 0)
        assert uniform == 0 or share == 0
        # the lane form only where a wave lies in one member
        assert lanes_safe == 1
        if kl:
            assert item_bits >= 6
        checked, takers, cover_min, cover_max, touched, bad_owner, bad_partner, bad_unit, bad_batch = found
        assert (bad_owner, bad_partner, bad_unit, touched, bad_batch) == (0, 0, 0, 0, 0), (n, b, bits, lanes, cap)
        assert 1 <= takers and (members == 1 or takers < members)      # both kinds of member wherever there are two
        amps = members << n
        if amps <= 1 << 12:
            assert (cover_min, cover_max) == (1, 1), (n, b, bits, lanes, cap)
            assert checked == takers << n                              # the takers' amplitudes and nothing else
        else:
            assert checked == 16
        forms.add((k, kl, min(item_bits, 9), uniform))
    # many members per workgroup, one and two waves per member with shuffles, whole workgroups, every lane form
    assert {(1, 0, 0, 0), (1, 0, 5, 0), (1, 1, 6, 0), (1, 1, 7, 0), (1, 1, 8, 1), (1, 1, 9, 1), (2, 2, 9, 1), (2, 1, 9, 1), (2, 0, 9, 1),
            (2, 2, 6, 0), (2, 2, 7, 0), (2, 1, 6, 0), (1, 0, 9, 1), (2, 0, 8, 1), (2, 1, 8, 1), (2, 2, 8, 1)} <= forms
