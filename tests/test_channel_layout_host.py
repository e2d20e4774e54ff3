"""The launch shapes of the Kraus-channel kernels (quantum_computations_amd/csrc/qsv_channel_layout.h), on the host only.

tests/layout/channel_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan, as the other layout
tests compile theirs; requests go in as text and answers come back as text.  For n = 1 .. 30 qubits, every target bit and
every ordered pair of target bits, with and without the streaming forms: which bits are lane bits and which are loaded by
the thread, the offsets and lane masks against a model written here, every amplitude owned exactly once with the group
index of its own target bits, every shfl_xor partner inside the wave's 64-amplitude segment, and the grids within their
caps.  Also the slots of the reduced density matrix and the branch rule against tests/noise_reference.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck
import noise_reference as R

BLOCK, REDUCE_BLOCKS, MAX_BLOCKS, LANE_BITS, MIN_STREAM = 256, 1024, (1 << 24) - 1, 6, 14


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "channel_layout_driver.cpp", tmp_path_factory.mktemp("channel_layout"))

    def run(requests, number=int):
        lines = hostcheck.ask(exe, requests, timeout=600)
        return [[[number(x) for x in part.split()] for part in line.split("|")] for line in lines]
    return run


def blocks_for(items, cap):
    blocks = max((items + BLOCK - 1) // BLOCK, 1)
    if cap > 0:
        blocks = min(blocks, cap)
    return min(blocks, MAX_BLOCKS)


def model(n, bits, streaming):
    """(kh, kl, pos, lbit, weights of the high / low combination bits) as the header's comment defines them."""
    k = len(bits)
    lanes = streaming and n >= MIN_STREAM
    legs = sorted(range(k), key=lambda j: bits[j])
    pos, lbit, hw, lw = [], [], [], []
    for leg in legs:
        weight = 1 << (k - 1 - leg)
        if lanes and bits[leg] < LANE_BITS:
            lbit.append(bits[leg])
            lw.append(weight)
        else:
            pos.append(bits[leg])
            hw.append(weight)
    return len(pos), len(lbit), pos, lbit, hw, lw


def combos(values):
    return [sum(v for i, v in enumerate(values) if (c >> i) & 1) for c in range(4)]


def cases():
    out = []
    for n in range(1, 31):
        for streaming in (0, 1):
            for cap in (0, 2):
                if cap and n not in (1, 13, 14, 19, 30):
                    continue
                for b in range(n):
                    out.append((n, (b,), streaming, cap))
                for b0 in range(n):
                    for b1 in range(n):
                        if b0 != b1:
                            out.append((n, (b0, b1), streaming, cap))
    return out


def test_every_shape_covers_the_register_once_and_stays_within_the_caps(ask):
    todo = cases()
    answers = ask([f"plan {n} {len(bits)} {bits[0]} {bits[1] if len(bits) > 1 else -1} {streaming} {cap}" for n, bits, streaming, cap in todo])
    placements = set()
    for (n, bits, streaming, cap), a in zip(todo, answers):
        head, pos, hoff, lbit, lxor, ghi, glo, grids, check = a
        kh, kl, want_pos, want_lbit, hw, lw = model(n, bits, streaming)
        amps = 1 << n
        assert head == [amps >> kh, kh, kl], (n, bits, streaming)
        assert pos == want_pos and lbit == want_lbit
        assert hoff == combos([1 << p for p in want_pos]) and lxor == combos([1 << b for b in want_lbit])
        assert ghi == combos(hw) and glo == combos(lw)
        assert all(b >= LANE_BITS or not kl or b in lbit for b in bits)
        if not (streaming and n >= MIN_STREAM):
            assert kl == 0                                         # small registers and the plain forms: strided loads only
        W = amps >> kh
        if kl:
            assert W % 64 == 0                                     # a wave is in the loop as a whole
        assert grids == [blocks_for(W, min(cap, REDUCE_BLOCKS) if cap else REDUCE_BLOCKS), blocks_for(W, cap)]
        assert 1 <= grids[0] <= REDUCE_BLOCKS and 1 <= grids[1] <= MAX_BLOCKS
        if cap:
            assert max(grids) <= cap
        checked, cover_min, cover_max, bad_group, bad_partner, bad_range = check
        assert (cover_min, cover_max, bad_group, bad_partner, bad_range) == (1, 1, 0, 0, 0), (n, bits, streaming, check)
        assert checked == (amps if n <= 16 else (4096 + 7) << kh)
        placements.add((len(bits), kh, kl))
    assert placements == {(1, 1, 0), (1, 0, 1), (2, 2, 0), (2, 1, 1), (2, 0, 2)}


def test_reduced_density_slots_are_distinct_and_dense(ask):
    for D, (entries, slots) in zip((2, 4), ask(["slots 2", "slots 4"])):
        assert entries == [D * D]
        assert slots == list(range(D, D * D, 2))                  # (re, im) pairs right after the D diagonal entries


def test_branch_rule_matches_the_reference(ask):
    rng = np.random.default_rng(7)
    requests, want = [], []
    for trial in range(300):
        count = int(rng.integers(1, 17))
        w = rng.random(count)
        w[rng.random(count) < 0.3] = 0.0
        if trial % 10 == 0:
            w[:] = 0.0
        u = [0.0, float(np.nextafter(1.0, 0.0)), float(rng.random())][trial % 3]
        requests.append("pick " + repr(u) + " " + " ".join(repr(float(x)) for x in w))
        total = 0.0
        for x in w:
            total += float(x)
        want.append((R.pick_branch(list(w), u), total))
    for (j, total), ((gj, gtotal),) in zip(want, ask(requests, number=str)):
        assert int(gj) == j and float(gtotal) == total
