"""The launch plans of the subsystem read-out (quantum_computations_amd/csrc/qsv_subsystem_layout.h), on the host only.

tests/layout/subsystem_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan, as the other layout
tests compile theirs; requests go in as text and answers come back as text.  For n = 1 .. 34 qubits and k = 1 .. 12 kept
qubits on the lowest bits, the highest bits (reversed), all from bit 6 up and a random unsorted choice: the position
tables, the block / slice split and the workspace against a model written here; every (row, group) of a walked tile
staged exactly once, at the address the model gives and in an LDS slot of its own; every entry of the caller's matrix
written exactly once, mirror included; grids within 2^32 work-items; the workspace within 256 MiB; both forms on the
domain the design states.  The marginal plan (k up to 26) gets the same ownership check.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck

BLOCK, LANE_BITS, MIN_TILED, MAX_K, MARG_MAX_K = 256, 6, 14, 12, 26
ROWS, TILE_GROUPS, PART_BYTES = 64, 64, 8 * 2 * 64 * 64
TARGET_ITEMS, MAX_ITEMS, WORKSPACE_LIMIT = 1024, 4096, 256 << 20
MARG_WAVES, MARG_PARTIALS = 4096, 1 << 22


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "subsystem_layout_driver.cpp", tmp_path_factory.mktemp("subsystem_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=900)
        return [[[int(x) for x in part.split()] for part in line.split("|")] for line in lines]
    return run


def placements(n, k, rng):
    """Physical bits of the caller's qubits: lowest k, top k reversed, all from bit 6 up (where they fit), random unsorted."""
    out = {tuple(range(k)), tuple(range(n - k, n)), tuple(int(b) for b in rng.permutation(n)[:k])}
    if n - LANE_BITS >= k:
        out.add(tuple(range(LANE_BITS, LANE_BITS + k)))
    return sorted(out)


def pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


def rdm_model(n, k, bits, cap):
    """What the header's comment and DESIGN.md section 22 say the plan is."""
    kk = max(k, 6)
    tiled = n >= MIN_TILED and n - kk >= 6
    if not tiled:
        kk = k
    kept = set(bits)
    extra = [b for b in range(n) if b not in kept][:kk - k]
    kpos = sorted(kept | set(extra))
    tpos = [b for b in range(n) if b not in kpos]
    m = dict(tiled=tiled, kk=kk, extra=kk - k, l=sum(b < 6 for b in kpos), h=sum(b >= 6 for b in kpos),
             lmask=sum(1 << b for b in kpos if b < 6), kpos=kpos, tpos=tpos, rbit=[kpos.index(b) for b in bits],
             xbit=[kpos.index(b) for b in extra], W=1 << (n - kk), finish_grid=max((4 ** k + BLOCK - 1) // BLOCK, 1))
    if tiled:
        nb = 1 << (kk - 6)
        pairs = nb * (nb + 1) // 2
        tiles = (1 << (n - kk)) // TILE_GROUPS
        slices = pow2_at_least((TARGET_ITEMS + pairs - 1) // pairs)
        while slices > 1 and pairs * slices > MAX_ITEMS:
            slices //= 2
        slices = min(slices, tiles)
        m.update(nb=nb, slices=slices, tiles_per_slice=tiles // slices, items=pairs * slices,
                 grid=min(pairs * slices, cap) if cap else pairs * slices, workspace=pairs * slices * PART_BYTES)
    else:
        m.update(nb=0, slices=0, tiles_per_slice=0, items=0, grid=m["finish_grid"], workspace=0)
    return m


def rdm_cases():
    rng = np.random.default_rng(22)
    out = []
    for n in range(1, 35):
        for k in range(1, min(n, MAX_K) + 1):
            for bits in placements(n, k, rng):
                out.append((n, k, bits, 0))
    out += [(16, 7, tuple(range(7)), 2), (16, 7, tuple(range(9, 16)), 2), (28, 10, tuple(range(10)), 2)]
    return out


def test_reduced_state_plans_own_every_row_and_group_once(ask):
    todo = rdm_cases()
    answers = ask([f"rdm {n} {k} {cap} " + " ".join(map(str, bits)) for n, k, bits, cap in todo])
    forms = set()
    for (n, k, bits, cap), a in zip(todo, answers):
        head, kpos, tpos, rbit, xbit, cover, finish = a
        m = rdm_model(n, k, bits, cap)
        tiled, kk, extra, l, h, lmask, nb, slices, tiles_per_slice, items, grid, finish_grid, workspace, W = head
        where = (n, k, bits, cap)
        assert (bool(tiled), kk, extra, l, h, lmask, W) == (m["tiled"], m["kk"], m["extra"], m["l"], m["h"], m["lmask"], m["W"]), where
        assert (kpos, tpos, rbit, xbit) == (m["kpos"], m["tpos"], m["rbit"], m["xbit"]), where
        assert (nb, slices, tiles_per_slice, items, grid, finish_grid, workspace) == \
            (m["nb"], m["slices"], m["tiles_per_slice"], m["items"], m["grid"], m["finish_grid"], m["workspace"]), where
        # the domain of the two forms: the matrix cores from 14 qubits up and with at least one tile of 64 groups
        assert bool(tiled) == (n >= MIN_TILED and n - max(k, 6) >= 6), where
        assert workspace <= WORKSPACE_LIMIT, where
        assert grid * BLOCK < 1 << 32 and finish_grid * BLOCK < 1 << 32 and grid >= 1, where
        if tiled:
            assert slices * tiles_per_slice * TILE_GROUPS == W and 1 <= items <= MAX_ITEMS, where    # the slices cut the groups exactly
            assert cap == 0 or grid <= cap
        checked, cover_min, cover_max, bad_addr, bad_slot, bad_range = cover
        assert (cover_min, cover_max, bad_addr, bad_slot, bad_range) == (1, 1, 0, 0, 0), (where, cover)
        if n <= 16:     # walked whole: every block pair reads its rows for every group
            pairs = nb * (nb + 1) // 2
            want = (sum(2 if I != J else 1 for I in range(nb) for J in range(I, nb)) * ROWS * W) if tiled else (1 << n)
            assert checked == want, (where, checked, pairs)
        else:
            assert checked > 0
        entries, write_min, write_max, bad_entry = finish
        assert (write_min, write_max, bad_entry) == (1, 1, 0), (where, finish)
        if k <= 9:
            assert entries == (1 << k) * ((1 << k) + 1) // 2
        forms.add((bool(tiled), extra > 0, l))
    assert {(True, False, l) for l in range(7)} <= forms and (True, True, 6) in forms and (False, False, 0) in forms


def test_block_pair_index_and_partial_slots(ask):
    answers = ask(["slots"] + [f"pairs {nb}" for nb in (1, 2, 4, 8, 16, 32, 64)])
    slots = np.array(answers[0][0]).reshape(64, 64)
    # v_mfma_f64_16x16x4 leaves D[row][col] in lane (row % 4) * 16 + col, register row / 4; the
    # partial is [row tile of I][row tile of J][re, im][register][lane]
    ip, jp = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    want = (((ip // 16) * 4 + jp // 16) * 2) * 256 + ((ip % 16) // 4) * 64 + ((ip % 16) % 4) * 16 + jp % 16
    assert np.array_equal(slots, want)
    assert len(set(slots.reshape(-1))) == 4096 and np.all((slots // 256) % 2 == 0)     # distinct real slots; imaginary 256 on
    for nb, (flat,) in zip((1, 2, 4, 8, 16, 32, 64), answers[1:]):
        got = list(zip(flat[0::2], flat[1::2]))
        assert got == [(I, J) for I in range(nb) for J in range(I, nb)]


def marg_model(n, k, bits):
    kpos = sorted(bits)
    tpos = [b for b in range(n) if b not in kpos]
    l, h = sum(b < 6 for b in kpos), sum(b >= 6 for b in kpos)
    w_bits = n - 6 - h
    streaming = n >= MIN_TILED and k <= MAX_K and w_bits >= 6
    m = dict(streaming=streaming, l=l, h=h, lmask=sum(1 << b for b in kpos if b < 6), kpos=kpos, tpos=tpos,
             rbit=[kpos.index(b) for b in bits], W=1 << (n - k))
    if streaming:
        waves = min(1 << w_bits, MARG_WAVES, MARG_PARTIALS >> k)
        m.update(waves=waves, run=(1 << w_bits) // waves, grid=waves // 4, workspace=8 * (waves + 1) * (1 << k))
    else:
        m.update(waves=0, run=0, grid=((1 << k) + BLOCK - 1) // BLOCK, workspace=8 << k)
    return m


def test_marginal_plans_read_every_amplitude_once(ask):
    rng = np.random.default_rng(23)
    todo = [(n, k, bits) for n in range(1, 35) for k in range(1, min(n, MARG_MAX_K) + 1) for bits in placements(n, k, rng)]
    answers = ask([f"marg {n} {k} " + " ".join(map(str, bits)) for n, k, bits in todo])
    forms = set()
    for (n, k, bits), a in zip(todo, answers):
        head, kpos, tpos, rbit, cover = a
        m = marg_model(n, k, bits)
        streaming, l, h, lmask, waves, run, grid, workspace, W = head
        assert (bool(streaming), l, h, lmask, waves, run, grid, workspace, W) == \
            (m["streaming"], m["l"], m["h"], m["lmask"], m["waves"], m["run"], m["grid"], m["workspace"], m["W"]), (n, k, bits)
        assert (kpos, tpos, rbit) == (m["kpos"], m["tpos"], m["rbit"])
        assert 1 <= grid and grid * BLOCK < 1 << 32
        assert workspace <= (32 << 20) + (8 << MAX_K) if streaming else workspace == 8 << k
        if streaming:
            assert waves % 4 == 0 and waves * run == 1 << (n - 6 - h)       # whole workgroups; the runs cut the loads exactly
        checked, cover_min, cover_max, bad_addr, bad_entry, bad_range = cover
        assert (cover_min, cover_max, bad_addr, bad_entry, bad_range) == (1, 1, 0, 0, 0), (n, k, bits, cover)
        if n <= 18:
            assert checked == 1 << n                                        # one read pass
        forms.add((bool(streaming), l))
    assert {(True, l) for l in range(7)} <= forms and (False, 0) in forms
    # the shapes the GPU tests name
    assert marg_model(19, 3, (0, 1, 2))["waves"] == MARG_WAVES and marg_model(19, 3, (0, 1, 2))["run"] == 2


def test_refused_shapes_have_no_plan(ask):
    assert ask(["rdm 16 13 0 " + " ".join(map(str, range(13))), "rdm 4 5 0 0 1 2 3 4", "rdm 41 2 0 0 1",
                "marg 30 27 " + " ".join(map(str, range(27))), "marg 3 4 0 1 2 3"]) == [[[-1]]] * 5
