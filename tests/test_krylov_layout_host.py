"""The launch shapes of qsv_lincomb and qsv_inner_many (quantum_computations_amd/csrc/qsv_krylov_layout.h), on the host
only.

tests/layout/krylov_layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan, as
tests/test_readout_layout_host.py compiles its driver; requests go in as text and answers come back as text.  Checked
against models written here: the grids, the split of 0, 1, 8, 9 and 17 operands into passes of at most eight, which pass
carries beta and which the norm, the kernel arguments of every pass (only the pass's own slots are filled), the slices
of the scratch buffer per pass and slot, and the host sums.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck

BLOCK, REDUCE_BLOCKS, MAX_BLOCKS, PER_PASS = 256, 1024, (1 << 24) - 1, 8


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "krylov_layout_driver.cpp", tmp_path_factory.mktemp("krylov_layout"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=600)
        return [[part.split() for part in line.split("|")] for line in lines]
    return run


def blocks_model(amps, cap):
    blocks = max(1, -(-amps // BLOCK))
    if cap > 0:
        blocks = min(blocks, cap)
    return min(blocks, MAX_BLOCKS)


def reduce_grid(amps, grid_cap):
    return blocks_model(amps, min(grid_cap, REDUCE_BLOCKS) if grid_cap > 0 else REDUCE_BLOCKS)


def stream_grid(amps, grid_cap):
    return blocks_model(amps, grid_cap if grid_cap > 0 else 0)


SIZES = [1, 2, 255, 256, 257, 1 << 13, 1 << 14, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, 1 << 19, 1 << 28, 1 << 32, 1 << 33]
CAPS = [0, 1, 2, 1000, 1024, 5000]


def test_grids(ask):
    cases = [(amps, cap) for amps in SIZES for cap in CAPS]
    for (amps, cap), ((reduce, stream),) in zip(cases, ask([f"grids {a} {c}" for a, c in cases])):
        assert int(reduce) == reduce_grid(amps, cap) and int(stream) == stream_grid(amps, cap), (amps, cap)
        assert 1 <= int(reduce) <= REDUCE_BLOCKS and 1 <= int(stream) <= MAX_BLOCKS
    # the threads of a reducing pass loop from 2^18 amplitudes on; those of a streaming pass beyond 2^32 only
    assert reduce_grid(1 << 18, 0) * BLOCK == 1 << 18 and reduce_grid(1 << 19, 0) * BLOCK < 1 << 19
    assert stream_grid(1 << 32, 0) * BLOCK < 1 << 32 and stream_grid(1 << 31, 0) * BLOCK == 1 << 31


@pytest.mark.parametrize("n_src", [0, 1, 2, 7, 8, 9, 16, 17])
def test_lincomb_passes(ask, n_src):
    cases = [(beta, norm, amps, cap) for beta in ((0.0, 0.0), (1.0, 0.0), (0.0, -0.5), (-0.0, 0.0)) for norm in (0, 1)
             for amps, cap in ((1 << 10, 0), (1 << 19, 0), (1 << 19, 7), (1 << 19, 4000))]
    answers = ask([f"lincomb {n_src} {b[0]!r} {b[1]!r} {norm} {amps} {cap}" for b, norm, amps, cap in cases])
    for (beta, norm, amps, cap), answer in zip(cases, answers):
        passes = max(1, -(-n_src // PER_PASS))
        assert len(answer) == passes
        for p, tokens in enumerate(answer):
            assert "BAD" not in tokens and len(tokens) == 8 + 3 * PER_PASS
            first, count = int(tokens[0]), int(tokens[1])
            beta_re, beta_im = float.fromhex(tokens[2]), float.fromhex(tokens[3])
            reads, has_norm, grid, offset = (int(t) for t in tokens[4:8])
            assert first == PER_PASS * p and count == max(0, min(PER_PASS, n_src - first))
            assert (beta_re, beta_im) == (beta if p == 0 else (1.0, 0.0)), "the first pass carries beta, the others 1"
            assert reads == int(p > 0 or beta[0] != 0.0 or beta[1] != 0.0), "beta == 0 (either sign): dst is not read"
            assert has_norm == int(bool(norm) and p == passes - 1), "the last pass carries the norm"
            assert grid == (reduce_grid(amps, cap) if has_norm else stream_grid(amps, cap)) and offset == 0
            c_re = [float.fromhex(t) for t in tokens[8:16]]
            c_im = [float.fromhex(t) for t in tokens[16:24]]
            src = [int(t) for t in tokens[24:32]]
            for k in range(PER_PASS):
                used = k < count
                assert c_re[k] == (first + k + 1 if used else 0.0) and c_im[k] == (-(first + k + 1) if used else 0.0)
                assert src[k] == (4096 * (first + k + 1) if used else 0), "slots beyond the pass's sources stay null"
        assert sum(int(tokens[1]) for tokens in answer) == n_src


@pytest.mark.parametrize("n_x", [0, 1, 8, 9, 17])
def test_inner_passes_and_sums(ask, n_x):
    rng = np.random.default_rng(n_x)
    for amps, cap in ((1, 0), (1 << 10, 0), (1 << 14, 0), (1 << 19, 0), (1 << 19, 3)):
        (head, *passes), = ask([f"inner {n_x} {amps} {cap}"])
        grid = reduce_grid(amps, cap)
        assert len(passes) == -(-n_x // PER_PASS)
        offset = 0
        for p, tokens in enumerate(passes):
            assert "BAD" not in tokens
            first, count, g, off, *x = (int(t) for t in tokens)
            assert first == PER_PASS * p and count == min(PER_PASS, n_x - first) and 1 <= count <= PER_PASS
            assert g == grid and off == offset
            assert x == [4096 * (first + k + 1) if k < count else 0 for k in range(PER_PASS)]
            offset += grid * count * 2              # one complex partial per workgroup and slot; slices do not meet
        assert int(head[0]) == offset == 2 * grid * n_x
        if n_x == 0 or grid > 64:
            continue
        # the host sums: partial (block, slot) of pass p at offset_p + (block * count + slot) * 2, added in block order
        host = rng.normal(size=offset)
        (values,), = ask([f"innersum {n_x} {amps} {cap} " + " ".join(repr(float(v)) for v in host)])
        values = np.array([float.fromhex(t) for t in values])
        assert values.size == 2 * n_x
        for k in range(n_x):
            p, slot = divmod(k, PER_PASS)
            count = min(PER_PASS, n_x - PER_PASS * p)
            base_offset = 2 * grid * PER_PASS * p
            for part in (0, 1):
                want = 0.0
                for block in range(grid):
                    want += host[base_offset + (block * count + slot) * 2 + part]
                assert values[2 * k + part] == want
