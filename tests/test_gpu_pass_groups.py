"""The grouped pass kernel (k_pass_tile: the gates of a pass applied in registers, one LDS round trip per group of gates
whose targets fit four tile bits) against the per-gate path, at the smallest sizes where each of its parts can break.

Every gate keeps the arithmetic of its per-gate kernel, so every comparison is np.array_equal between a register with
QSV_OPT_DEFER = 2 and one with QSV_OPT_DEFER = 0 filled from the same seed.  Qubit q of an n-qubit register is index bit
n - 1 - q; the gates below are placed by BIT.  At n = 12 the tile is the whole register (tile index = bit); at n = 13 and
14 one or two bits lie outside the tile, and a group's register bits are its targets completed with the highest tile
indices, so a control can be a register bit, a thread bit or a bit outside the tile.
"""
from __future__ import annotations

import numpy as np
import pytest

from quantum_computations_amd import _lib
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DeviceState

pytestmark = pytest.mark.gpu


def run_both(n, seed, ops):
    """Apply ops to a deferring register and to one on the per-gate path; the amplitudes must agree bit for bit."""
    a = DeviceState.random(n, seed)
    b = DeviceState.random(n, seed)
    a.set_option(_lib.OPT_DEFER, 2)
    b.set_option(_lib.OPT_DEFER, 0)
    for gate in W.to_gates(ops):
        gate.apply(a)
        gate.apply(b)
    got, want = a.to_numpy(), b.to_numpy()
    queued, launches = a.defer_stats()
    assert np.array_equal(got, want), (np.max(np.abs(got - want)), int(np.count_nonzero(got != want)))
    assert queued > 0 and launches < queued, (queued, launches)      # a pass really ran
    assert b.defer_stats() == (0, 0)
    return queued, launches


class Bits:
    """Ops on index bits of an n-qubit register."""

    def __init__(self, n, seed):
        self.n, self.rng, self.ops = n, np.random.default_rng(seed), []

    def q(self, bit):
        return self.n - 1 - bit

    def u1(self, bit):
        self.ops.append(W.op("U", self.q(bit), matrix=W.haar_unitary(2, self.rng)))

    def u2(self, b0, b1):
        self.ops.append(W.op("U", self.q(b0), self.q(b1), matrix=W.haar_unitary(4, self.rng)))

    def cu(self, ctrl, target):
        m = np.identity(4, dtype=complex)
        m[2:, 2:] = W.haar_unitary(2, self.rng)
        self.ops.append(W.op("U", self.q(ctrl), self.q(target), matrix=m))

    def d1(self, bit):
        self.ops.append(W.op("U", self.q(bit), matrix=np.diag(np.exp(1j * self.rng.uniform(0, 6.3, 2)))))

    def d2(self, b0, b1):
        self.ops.append(W.op("U", self.q(b0), self.q(b1), matrix=np.diag(np.exp(1j * self.rng.uniform(0, 6.3, 4)))))

    def named(self, name, *bits):
        self.ops.append(W.op(name, *[self.q(b) for b in bits]))


@pytest.mark.parametrize("a", range(12))
def test_two_qubit_gates_on_every_ordered_pair_of_tile_bits(a):
    """n = 12: a Haar 4x4 on legs (a, b) for every b, a Haar 2x2 before and after it in the same group.  Covers the three
    summation orders (both legs below bit 6, both above, one of each), both leg orders, every register position."""
    c = Bits(12, 40 + a)
    for b in range(12):
        if b != a:
            c.u1(a)
            c.u2(a, b)
            c.u1(b)
    run_both(12, a, c.ops)


def test_one_qubit_gates_on_every_tile_bit():
    c = Bits(12, 7)
    for b in range(12):
        c.u1(b)
    for b in reversed(range(12)):
        c.u1(b)
    run_both(12, 7, c.ops)


@pytest.mark.parametrize("n", [13, 14])
@pytest.mark.parametrize("kind", ["cu", "CX", "CZ"])
def test_controls_on_register_thread_and_outside_bits(n, kind):
    """Every ordered (control, target) pair of bits, each between dense gates of its group.  With targets t and t + 1
    (mod n) in the group, the control is a register bit (t + 1, or one of the highest tile indices that complete the
    group), a thread bit (the other tile bits) or outside the tile (one or two of bits 6 .. n - 1), in turn."""
    c = Bits(n, 3 * n + len(kind))
    for t in range(n):
        for ctrl in range(n):
            if ctrl == t:
                continue
            c.u1(t)
            if kind == "cu":
                c.cu(ctrl, t)
            else:
                c.named(kind, ctrl, t)
            c.u1((t + 1) % n)
    run_both(n, n, c.ops)


def test_pass_in_which_some_gates_act_on_half_the_tiles():
    """n = 14, tile = bits 0..11: the CX and the controlled-U have their controls on bits 12 and 13, outside the tile, so
    they act on half the tiles each and the Haar gates between them on all; the last two on a quarter of the tiles only."""
    c = Bits(14, 21)
    c.u1(0)
    c.named("CX", 13, 1)
    c.u1(2)
    c.cu(12, 3)
    c.u2(7, 1)
    c.named("CZ", 13, 12)
    c.named("CX", 12, 9)
    c.d1(4)
    run_both(14, 21, c.ops)
    c = Bits(14, 22)
    c.named("CX", 13, 1)          # every gate of the pass is controlled from outside: a quarter of the tiles is never loaded
    c.cu(13, 2)
    c.named("CX", 13, 8)
    c.cu(12, 3)
    run_both(14, 22, c.ops)


@pytest.mark.parametrize("n", [13, 14])
def test_diagonal_gates_and_phases_between_dense_gates_of_one_group(n):
    """Dense gates on bits 0 and 7 keep one group open (register bits 0, 7 and the two highest tile indices); the diagonal
    gates between them select their factors by register bits, thread bits, one of each, or bits outside the tile."""
    c = Bits(n, 5 * n)
    for z0 in range(n):
        c.u2(0, 7)
        c.d1(z0)
        c.named(["P", "T", "Z", "Tdg"][z0 % 4], z0)
        for z1 in range(n):
            if z1 != z0:
                c.u1(7 if z1 % 2 else 0)
                c.d2(z0, z1)
    run_both(n, n + 1, c.ops)


@pytest.mark.parametrize("n", [13, 14])
def test_swap_and_cx_as_exchanges_on_low_high_and_mixed_legs(n):
    c = Bits(n, 9 * n)
    for a in range(n):
        for b in range(n):
            if a != b:
                c.u1(a)
                c.named("SWAP" if (a + b) % 2 else "CX", a, b)
                c.u1(b)
    run_both(n, n + 2, c.ops)


def test_sixty_four_gates_in_one_pass():
    """n = 14: more than 64 gates that all fit one tile, so the first pass holds MAX_PASS_GATES = 64 of them."""
    c = Bits(14, 64)
    for i in range(70):
        if i % 3 == 2:
            c.u2(i % 12, (i + 5) % 12)
        else:
            c.u1((5 * i) % 12)
    queued, launches = run_both(14, 64, c.ops)
    assert (queued, launches) == (70, 2)


def test_targets_alternating_between_two_disjoint_sets_of_four_bits():
    """Two consecutive gates never have more than four target bits, so no cut has fewer than two gates per group: here
    every second gate opens a new group ((0, 1) (4, 9) | (2, 3) (6, 11) | ...), the most a list of gates can ask for."""
    c = Bits(14, 31)
    for i in range(12):
        c.u2(0, 1)
        c.u2(4, 9)
        c.u2(3, 2)
        c.u2(11, 6)
    c.u1(5)
    run_both(14, 31, c.ops)


def test_run_inside_one_set_of_four_bits_is_one_group():
    c = Bits(14, 32)
    four = [1, 4, 7, 10]
    for i in range(40):
        if i % 2:
            c.u2(four[i % 4], four[(i + 1 + (i // 4) % 3) % 4])
        else:
            c.u1(four[(i // 2) % 4])
    run_both(14, 32, c.ops)


def mixed_circuit(n, depth, seed):
    """cfg2's generator plus the other gate shapes the queue classifies: diagonals, phases, controlled-U, CX / SWAP on
    low bits, X and Z, and placements with every qubit among the lowest or the highest bits."""
    rng = np.random.default_rng(seed)
    ops = W.random_circuit(n, depth, seed)
    extra = []
    for i in range(depth // 2):
        kind = int(rng.integers(8))
        lo = bool(rng.integers(2))
        pool = list(range(n - 6, n)) if lo else list(range(6))      # qubit n-1 = bit 0
        q0, q1 = (int(v) for v in rng.choice(pool if i % 3 == 0 else n, size=2, replace=False))
        if kind == 0:
            extra.append(W.op("U", q0, matrix=np.diag(np.exp(1j * rng.uniform(0, 6.3, 2)))))
        elif kind == 1:
            extra.append(W.op("U", q0, q1, matrix=np.diag(np.exp(1j * rng.uniform(0, 6.3, 4)))))
        elif kind == 2:
            extra.append(W.op(["T", "Z", "P", "X"][i % 4], q0))
        elif kind == 3:
            u = W.haar_unitary(2, rng)
            m = np.identity(4, dtype=complex)
            m[2:, 2:] = u
            extra.append(W.op("U", q0, q1, matrix=m))                   # controlled-U, control on leg 0
        elif kind == 4:
            extra.append(W.op("CX", q0, q1))
        elif kind == 5:
            extra.append(W.op("SWAP", q0, q1))
        elif kind == 6:
            extra.append(W.op("CZ", q0, q1))
        else:
            extra.append(W.op("U", q0, q1, matrix=W.haar_unitary(4, rng)))
    out = []
    for i, o in enumerate(ops):
        out.append(o)
        if i % 2 == 1 and extra:
            out.append(extra.pop())
    return out + extra


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_circuits_at_18_qubits(seed):
    """The tile's high bits vary between the passes."""
    run_both(18, seed, mixed_circuit(18, 120, seed))
