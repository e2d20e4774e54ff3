"""The launch shapes of the trajectory-ensemble kernels (quantum_computations_amd/csrc/qsv_ensemble_layout.h), on the host only.

tests/layout/ensemble_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan, as the other layout
tests compile theirs.  For members of n = 1 .. 26 qubits, 2^b members with b = 0 .. 12 and n + b <= 30, every target bit and
every ordered pair of target bits, grid caps 0, 1 and 2: every amplitude owned by exactly one (member, part, item), no
workgroup sum that mixes members, the parts per member independent of b, every grid within its limits, and the regions of
the workspace disjoint and large enough.
"""
from __future__ import annotations

import pytest

import hostcheck

BLOCK_BITS, READ_ITEM_BITS, MAX_PART_BITS, MAX_BLOCKS, LANE_BITS, LOG_SLOTS, LOG_BUDGET = 8, 5, 7, (1 << 24) - 1, 6, 256, 1 << 22


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "ensemble_layout_driver.cpp", tmp_path_factory.mktemp("ensemble_layout"))

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


def floor_log2(v):
    return v.bit_length() - 1


def test_every_shape_covers_every_member_once_and_no_sum_mixes_members(ask):
    todo = cases()
    answers = ask([f"case {n} {b} {len(bits)} {bits[0]} {bits[1] if len(bits) > 1 else -1} {lanes} {cap}" for n, b, bits, lanes, cap in todo])
    parts_of = {}
    forms = set()
    for (n, b, bits, lanes, cap), a in zip(todo, answers):
        head, read, update, walk_read, walk_update, ws = a
        kh, kl, item_bits, W = head
        members, k = 1 << b, len(bits)
        # the lane rule: n >= 6 and the streaming forms allowed; then a member's items are a multiple of 64
        want_kl = sum(1 for bit in bits if bit < LANE_BITS) if (lanes and n >= LANE_BITS) else 0
        assert (kh, kl) == (k - want_kl, want_kl), (n, bits, lanes)
        assert item_bits == n - kh and W == 1 << item_bits
        if kl:
            assert item_bits >= 6
        cap_bits = floor_log2(cap) if cap else 99
        want_read = min(max(item_bits - BLOCK_BITS - READ_ITEM_BITS, 0), MAX_PART_BITS, cap_bits)
        want_update = min(max(item_bits - BLOCK_BITS, 0), cap_bits)
        share = max(BLOCK_BITS - item_bits, 0)
        for (pbits, sbits, units, grid), want in ((read, want_read), (update, want_update)):
            assert pbits == want and sbits == share
            assert units == max(members >> share, 1) << pbits
            assert 1 <= grid <= min(units, MAX_BLOCKS)
            if cap:
                assert grid <= cap
            assert share == 0 or pbits == 0                            # members that share a workgroup have one part
        # P depends on the member size, the target bits and the cap -- never on the number of members
        key = (n, bits, lanes, cap)
        assert parts_of.setdefault(key, (read[0], update[0])) == (read[0], update[0]), key
        amps = members << n
        for checked, cover_min, cover_max, bad_owner, bad_mix, bad_wave in (walk_read, walk_update):
            assert (cover_min, cover_max, bad_owner, bad_mix, bad_wave) == (1, 1, 0, 0, 0), (n, b, bits, lanes, cap)
            assert checked == (amps if amps <= 1 << 12 else 16)
        # the workspace: partials for the most parts any pass over such a member has, one matrix, one draw pair and `slots`
        # log rows per member; regions in order, none overlapping
        slots, partials, matrix, draws, log, doubles = ws
        assert slots == min(LOG_SLOTS, max(LOG_BUDGET // members, 1))
        most_parts = 1 << min(max(n - BLOCK_BITS - READ_ITEM_BITS, 0), MAX_PART_BITS)
        assert (1 << read[0]) <= most_parts
        assert partials == 0 and matrix - partials >= members * most_parts * 16
        assert draws - matrix >= members * 32 and log - draws >= members * 2 and doubles - log >= slots * members * 2
        forms.add((k, kl, min(item_bits, 9)))
    # many members per workgroup (with and without a butterfly), one wave and two waves per member, whole workgroups, every lane form
    assert {(1, 0, 0), (1, 0, 5), (1, 1, 6), (1, 1, 7), (1, 1, 8), (1, 1, 9), (2, 2, 9), (2, 1, 9), (2, 0, 9), (2, 2, 6), (1, 0, 9)} <= forms
