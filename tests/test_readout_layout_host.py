"""The host-side layouts of the read-out and Pauli launchers (quantum_computations_amd/csrc/qsv_readout_layout.h), on the
host only.

tests/layout/layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan exactly as
tests/test_layout_host.py compiles it; requests go in as text and answers come back as text.  Every check compares the
header with a NumPy model written here: the tile and byte tables of the qubit permutation (end to end against the oracle),
the plan of a reduced density matrix (form, tile sizes, offset tables, argument structs, grid) and the unpacking of the
matrix cores' result layout, the chunk choice of the sampler and its walk inside the chunk, and the argument structs of
the Pauli passes.
"""
from __future__ import annotations

import bisect
import itertools

import numpy as np
import pytest

import hostcheck
import pauli_operator_reference as P
import pauli_rotation_reference as R
from hostcheck import floats, nums, text
from oracle import dv_oracle as O

RO_MIN_QUBITS = 14
RDM_LOADS = 4


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "layout_driver.cpp", tmp_path_factory.mktemp("readout_layout"))

    def run(requests):
        """requests: [str] -> one answer line per request, as a list of '|'-separated token lists."""
        return [[part.split() for part in line.split("|")] for line in hostcheck.ask(exe, requests, timeout=600)]
    return run


def deposit_bits(value, positions):
    """Bit i of value -> bit positions[i]."""
    return sum(((value >> i) & 1) << p for i, p in enumerate(positions))


# ---- permutation -----------------------------------------------------------------------------------------------------------
def permute_orders(n):
    """src_bit_of_dst_bit lists: bit j of the destination index comes from bit order[j] of the source index."""
    rng = np.random.default_rng(100 + n)
    yield list(range(n))
    yield list(range(n))[::-1]
    yield list(range(3, n)) + [0, 1, 2]
    yield [2, 0, 1] + list(range(3, n))               # moves bits 0..2 only
    for _ in range(20):
        yield [int(b) for b in rng.permutation(n)]


@pytest.mark.parametrize("n", [14, 15])
def test_permute_tile_and_lut(ask, n):
    orders = list(permute_orders(n))
    answers = ask([f"permute {n} " + " ".join(map(str, order)) for order in orders])
    j = np.arange(1 << n, dtype=np.uint64)
    ket = np.arange(1 << n).astype(complex)           # ket[i] = i: the permuted ket spells out every source index
    for order, (head, dst, src, lut) in zip(orders, answers):
        tiles, nbytes = nums(head)
        dst, src, lut = nums(dst), nums(src), np.array([int(t) for t in lut], dtype=np.uint64)
        assert tiles == (1 << n) >> 6 and nbytes == (n + 7) // 8 and len(lut) == 256 * nbytes
        assert len(set(dst)) == 6 and dst == sorted(dst) and all(0 <= d < n for d in dst)
        assert {0, 1, 2} <= set(dst), "destination bits inside a 128-byte line"
        assert {order.index(b) for b in (0, 1, 2)} <= set(dst), "and the destinations of the source bits inside one"
        assert src == [order[d] for d in dst]
        source = np.zeros(1 << n, dtype=np.uint64)
        for b in range(nbytes):
            source |= lut[256 * b + ((j >> np.uint64(8 * b)) & np.uint64(255)).astype(np.int64)]
        # qsv_permute: the qubit at position q moves to new_ordering[q]; destination bit n-1-new_ordering[q] <- bit n-1-q
        new_ordering = [0] * n
        for d, s in enumerate(order):
            new_ordering[n - 1 - s] = n - 1 - d
        assert np.array_equal(ket[source.astype(np.int64)], O.permute_qubits(ket, new_ordering))


# ---- reduced density matrices: the plan ----------------------------------------------------------------------------------
def kept_sets(n, k):
    rng = np.random.default_rng(1000 * n + k)
    yield list(range(k))                                # the lowest bits
    yield list(range(n - 1, n - 1 - k, -1))             # the highest bits, reversed
    yield list(range(6, 6 + k))                         # all from bit 6
    yield ([0, 7, 3, n - 1, 5, 9])[:k]                  # mixed
    for _ in range(5):
        yield [int(b) for b in rng.permutation(n)[:k]]


def rdm_cases():
    """(n, amps, k, variant, remap, cus, bits).  Registers are 2^n amplitudes, for which the divisibility tests of both
    matrix-core forms always hold from 14 qubits on: W = 2^(n - k) >= 2^8, and the largest divisor is 64 S = 512 = 2^9 at
    k = 1, where W >= 2^13.  So that those tests return false too, some cases pass an `amps` of their own that leaves W an
    odd multiple of 8, or 0: the function takes n and amps separately."""
    for n, k, variant in itertools.product((13, 14, 15, 16), range(1, 7), (0, 2)):
        for s, bits in enumerate(kept_sets(n, k)):
            remap = (-1, -1, 0, 4, 3)[s % 5]
            for cus in (256, 1):
                yield n, 1 << n, k, variant, remap, cus, bits
    for n, k, variant in itertools.product((14, 16), range(1, 7), (0, 2)):
        yield n, (1 << n) + (8 << k), k, variant, -1, 256, list(range(k))
        yield n, 1 << (k - 1), k, variant, -1, 256, list(range(k))        # W = 0: no whole tile (the tile form's W >= 64 S)


def plan_model(n, amps, k, variant, remap, cus, bits):
    D, srt = 1 << k, sorted(bits)
    T = 1 if D <= 16 else 2 if D <= 32 else 4
    S = 16 // D if D < 16 else 1
    W = amps >> k
    old = variant == 2
    if old:
        big = n >= RO_MIN_QUBITS and W % (4 * S * 4 * (RDM_LOADS // T)) == 0
    else:
        big = n >= RO_MIN_QUBITS and W % (64 * S) == 0 and W >= 64 * S
    m = {"big": big, "old": old, "T": T, "P": T * (T + 1) // 2, "S": S, "sorted": srt,
         "off": [deposit_bits(r, srt) if r < D else 0 for r in range(16 * T)],
         "g": [W, k, D] + srt + [0] * (8 - k), "gt": [0] * 16, "hoff": [0] * 64, "blocks": 0}
    if big and not old:
        low, high = [b for b in srt if b < 6], [b for b in srt if b >= 6]
        tiles = W // (64 * S)
        want = remap if remap >= 0 else (8 if srt[-1] >= 20 or k == 6 else 0)
        regions = want if want > 1 and tiles % want == 0 else 0
        m["gt"] = [tiles, len(high), k, len(low), len(high), sum(1 << b for b in low), S.bit_length() - 1, regions] + high + [0] * (8 - len(high))
        m["hoff"] = [deposit_bits(c, high) if c < (1 << len(high)) else 0 for c in range(64)]
        m["blocks"] = min(tiles, (2 if T == 4 else 4 if T == 2 else 8) * cus)
    elif big:
        most = min((4 if T <= 2 else 2) * cus, max(1, W // (4 * S) // (4 * (RDM_LOADS // T))))
        m["blocks"] = 1 << (most.bit_length() - 1)
    m["entries"] = m["P"] * 2 * 256 if big else 2 * D * D
    return m


@pytest.fixture(scope="module")
def rdm_plans(ask):
    cases = list(rdm_cases())
    answers = ask(["rdm {} {} {} {} {} {} ".format(*c[:6]) + " ".join(map(str, c[6])) for c in cases])
    return cases, answers


def test_rdm_plan(rdm_plans):
    cases, answers = rdm_plans
    seen = set()
    for case, (head, srt, off, g, gt, hoff) in zip(cases, answers):
        n, amps, k, variant, remap, cus, bits = case
        m = plan_model(*case)
        big, old, T, P, S, blocks, entries = nums(head)
        assert (big, old, T, P, S) == (int(m["big"]), int(m["old"]), m["T"], m["P"], m["S"]), case
        assert nums(srt) == m["sorted"] and nums(off) == m["off"], case
        assert nums(g) == m["g"], case
        assert nums(gt) == m["gt"] and nums(hoff) == m["hoff"], case
        assert blocks == m["blocks"] and entries == m["entries"], case
        tiles, regions = nums(gt)[0], nums(gt)[7]
        assert regions == 0 or tiles % regions == 0
        if big and old:
            assert blocks & (blocks - 1) == 0 and blocks >= 1
        seen.add((variant, amps == 1 << n, n >= RO_MIN_QUBITS, bool(big)))
    # false below 14 qubits for both forms; true from 14 on for every register; false there through each form's own test
    for variant in (0, 2):
        assert (variant, True, False, False) in seen and (variant, True, False, True) not in seen
        assert (variant, True, True, True) in seen and (variant, True, True, False) not in seen
        assert (variant, False, True, False) in seen


# ---- reduced density matrices: the unpacking -----------------------------------------------------------------------------
def user_index(k, bits, srt):
    """Caller's matrix index of kernel index c: kernel bit i <-> srt[i], caller's bit k-1-j <-> bits[j]."""
    return [sum(((c >> i) & 1) << (k - 1 - bits.index(srt[i])) for i in range(k)) for c in range(1 << k)]


def pack_raw(rng, m, variant):
    """A random matrix in kernel order and the `raw` the kernels would leave for it."""
    D, T, S = m["g"][2], m["T"], m["S"]
    if not m["big"]:                                     # k_rdm_small: 2 (r D + c), any complex matrix
        M = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
        return M, np.stack([M.real, M.imag], axis=-1).reshape(-1)
    raw = rng.normal(size=m["entries"])                  # garbage wherever nothing is written below
    if D < 16:                                           # S summands on the diagonal blocks of the one shared tile
        parts = rng.normal(size=(S, D, D)) + 1j * rng.normal(size=(S, D, D))
        M = np.zeros((D, D), dtype=complex)
        for s in range(S):                               # summed in block order, as rdm_unpack does
            M = M + parts[s]
    else:
        M = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    M = np.triu(M) + np.conj(np.triu(M, 1)).T            # Hermitian, exactly
    M[np.diag_indices(D)] = M.diagonal().real

    def put(pidx, row, col, value):
        reg, lane = row // 4, (row % 4) * 16 + col
        raw[((pidx * 2 + 0) * 4 + reg) * 64 + lane] = value.real
        raw[((pidx * 2 + 1) * 4 + reg) * 64 + lane] = value.imag
    pairs = [(ti, tj) for ti in range(T) for tj in range(ti, T)]
    for pidx, (ti, tj) in enumerate(pairs):
        for row in range(16):
            for col in range(16):
                if D < 16:
                    s = row // D
                    if col // D != s or row > col:
                        continue                         # off-diagonal blocks and lower triangles stay garbage
                    put(pidx, row, col, parts[s][row % D, col % D])
                elif variant == 0 and T == 4 and (ti, tj) == (0, 3):
                    put(pidx, row, col, M[48 + row, col])   # held as the block of (3, 0)
                elif ti != tj or row < col:
                    put(pidx, row, col, M[16 * ti + row, 16 * tj + col])
                elif row == col:                         # the diagonal's imaginary part is garbage: rounding only
                    raw[((pidx * 2 + 0) * 4 + row // 4) * 64 + (row % 4) * 16 + col] = M[16 * ti + row, 16 * tj + col].real
    return M, raw


def test_rdm_unpack(ask, rdm_plans):
    cases, answers = rdm_plans
    rng = np.random.default_rng(7)
    chosen, requests, wanted = [], [], []
    for case, answer in zip(cases, answers):
        n, amps, k, variant, remap, cus, bits = case
        if cus != 256:
            continue                                     # the same plan but for the grid: every kept set stays
        m = plan_model(*case)
        M, raw = pack_raw(rng, m, variant)
        ui = user_index(k, bits, m["sorted"])
        want = np.zeros_like(M)
        want[np.ix_(ui, ui)] = M
        chosen.append(case)
        wanted.append(want)
        requests.append("rdmunpack {} {} {} {} {} {} ".format(*case[:6]) + " ".join(map(str, bits)) + " " + text(raw))
    forms = {(bool(plan_model(*c)["big"]), c[3], plan_model(*c)["T"], plan_model(*c)["S"]) for c in chosen}
    assert {(True, 0, 4, 1), (True, 2, 4, 1), (True, 0, 1, 8), (True, 0, 2, 1), (False, 0, 1, 8), (False, 2, 4, 1)} <= forms
    for case, want, (rho,) in zip(chosen, wanted, ask(requests)):
        got = floats(rho).reshape(want.shape + (2,))
        got = got[..., 0] + 1j * got[..., 1]
        assert np.array_equal(got, want), case
        if plan_model(*case)["big"]:
            assert np.array_equal(got, np.conj(got).T) and not got.diagonal().imag.any(), case


# ---- sampling --------------------------------------------------------------------------------------------------------------
def sample_model(sums, draws):
    cum = [0.0]
    for s in sums:
        cum.append(cum[-1] + s)
    total, chunks = cum[-1], len(sums)
    if not total > 0.0:
        return 1, total, [], []
    chunk, resid = [], []
    for u in draws:
        if not 0.0 <= u < 1.0:
            return 2, total, [], []
        target = u * total
        c = bisect.bisect_right(cum, target)             # first cum > target
        c = 0 if c == 0 else c - 1
        while c + 1 < chunks and sums[c] == 0.0:         # never land in an empty chunk
            c += 1
        c = min(c, chunks - 1)
        chunk.append(c)
        resid.append(target - cum[c])
    return 0, total, chunk, resid


def test_sample_chunks(ask):
    rng = np.random.default_rng(11)
    below_one = float(np.nextafter(1.0, 0.0))
    lists = [[0.75], [0.25, 0.5], [0.0, 1.5], [2.0, 0.0],
             [0.0, 0.25, 0.0, 0.5, 0.25, 0.0, 0.0],      # leading, inner and trailing empty chunks; dyadic: exact boundaries
             [0.0, 0.0, 0.125, 0.0, 0.0, 0.375, 0.0],
             [float(x) for x in rng.random(7)], [float(x) for x in rng.random(2)]]
    cases = []
    for sums in lists:
        total = sum(sums)
        edges = [float(c) / total for c in np.cumsum(sums)[:-1] if c < total]
        cases.append((sums, [0.0, below_one] + edges + [float(x) for x in rng.random(200)]))
    cases += [([0.0], [0.5]), ([0.0, 0.0, 0.0], [0.5]),                  # zero norm
              ([0.5, 0.5], [0.25, 1.0]), ([0.5, 0.5], [-1e-300, 0.5])]   # a draw outside [0, 1)
    answers = ask([f"sample {len(s)} {len(u)} {text(s)} {text(u)}" for s, u in cases])
    statuses = []
    for (sums, draws), (head, *rest) in zip(cases, answers):
        status, total, chunk, resid = sample_model(sums, draws)
        assert int(head[0]) == status and float.fromhex(head[1]) == total
        statuses.append(status)
        if status == 0:
            assert nums(rest[0]) == chunk and np.array_equal(floats(rest[1]), np.array(resid))
            assert all(sums[c] > 0.0 for c in chunk) and all(r >= 0.0 for r in resid)
    assert statuses[:len(lists)] == [0] * len(lists) and statuses[len(lists):] == [1, 1, 2, 2]


def walk_model(p, threads, slots, residual):
    """sample_walk: the first crossing of the running sum, thread sums first and the owner's slots next; where rounding
    leaves none, the last thread of positive sum and its last slot of positive weight."""
    sums = []
    for t in range(threads):
        s = 0.0
        for k in range(slots):
            s += p[t * slots + k]
        sums.append(s)
    run, owner, last = 0.0, -1, -1
    for t, s in enumerate(sums):
        if s > 0.0:
            last = t
        if run + s > residual:
            owner = t
            break
        run += s
    crossed = owner >= 0
    if not crossed:
        owner = max(last, 0)
    slot, last = -1, -1
    for k in range(slots):
        m = p[owner * slots + k]
        if m > 0.0:
            last = k
        if crossed and run + m > residual:
            slot = k
            break
        run += m
    if slot < 0:
        slot = max(last, 0)
    return owner * slots + slot


def walk_sums(p, threads, slots):
    """What the walk can compare a residual with: the running sum over the thread sums, as the first level forms it, and
    for every thread the running sum over its slots on top of the sum in front of it, as the second level does."""
    firsts, seconds, run = [], [], 0.0
    for t in range(threads):
        s, inner = 0.0, run
        for k in range(slots):
            s += p[t * slots + k]
            inner += p[t * slots + k]
            seconds.append(inner)
        run += s
        firsts.append(run)
    return firsts, seconds


def test_sample_walk(ask):
    rng = np.random.default_rng(13)

    def weights(threads, slots, support):
        p = np.zeros(threads * slots)
        p[support] = rng.normal(size=len(support)) ** 2 + rng.normal(size=len(support)) ** 2
        return [float(x) for x in p]
    shapes = [(256, 16), (4, 4), (1, 16), (8, 1)]
    cases = []
    for threads, slots in shapes:
        size = threads * slots
        lists = [weights(threads, slots, np.arange(size)),                                              # dense
                 weights(threads, slots, np.arange(max(1, size // 40))),                                # trailing zeros
                 weights(threads, slots, np.arange(size // 2, size // 2 + max(1, slots // 2))),         # leading and trailing
                 weights(threads, slots, rng.choice(size, size=max(1, size // 14), replace=False)),     # scattered
                 weights(threads, slots, [size // 3]), weights(threads, slots, [0]), weights(threads, slots, [size - 1]),
                 [0.0] * size]                                                                          # all zero: offset 0
        for p in lists:
            firsts, seconds = walk_sums(p, threads, slots)
            marks = {0.0, firsts[-1], seconds[-1], sum(p), float(np.sum(p))}                            # the sequential sums
            if size <= 64:                                                                              # and inner ones
                marks |= set(firsts) | set(seconds[::3])
            residuals = set()
            for mark in marks:                                                                          # equal, one ulp above and below
                residuals |= {mark, float(np.nextafter(mark, np.inf)), float(np.nextafter(mark, -np.inf)), 0.5 * mark}
            residuals.add(2.0 * firsts[-1] + 1.0)                                                       # far past the end
            cases += [(threads, slots, r, p) for r in sorted(residuals) if r >= 0.0]
    answers = ask([f"samplewalk {threads} {slots} {r!r} {text(p)}" for threads, slots, r, p in cases])
    fell_through = 0
    for (threads, slots, r, p), (tokens,) in zip(cases, answers):
        got, = nums(tokens)
        assert got == walk_model(p, threads, slots, r), (threads, slots, r)
        if any(p):
            assert p[got] > 0.0, "never an amplitude of weight zero"
            last = max(i for i, x in enumerate(p) if x > 0.0)
            firsts, seconds = walk_sums(p, threads, slots)
            if r >= max(firsts[-1], max(seconds)):
                assert got == last, "past every running sum: the last possible amplitude"
                fell_through += 1
            if r == 0.0:
                assert got == min(i for i, x in enumerate(p) if x > 0.0), "a residual of 0: the first possible amplitude"
            # away from rounding the answer is the plain inverse CDF over the flat list
            exact = np.cumsum(np.array(p, dtype=np.longdouble))
            slack = 1e-12 * float(exact[-1])
            if r < float(exact[-1]) - slack:
                want = int(np.searchsorted(exact, np.longdouble(r), side="right"))
                if abs(float(exact[want]) - r) > slack and (want == 0 or abs(float(exact[want - 1]) - r) > slack):
                    assert got == want, (threads, slots, r)
        else:
            assert got == 0
    assert fell_through >= 8 * len(shapes)


# ---- Pauli passes ----------------------------------------------------------------------------------------------------------
def width_of(count):
    return 1 if count <= 1 else 2 if count <= 2 else 4 if count <= 4 else 8


def pauli_lists(n=10):
    """(xmask, zmask) lists on 10 qubits: passes of 1, 2, 3, 5 and 8 terms, diagonal-only ones and terms carrying Y."""
    rng = np.random.default_rng(21)
    masks = [0, 0b1000000001, 0b0000110000, 0b0000000100, 0b1111111111]   # diagonal, two bits apart, inside a line, bit 2, all
    for count in (1, 2, 3, 5, 8):
        for x in masks:
            yield [(x, int(z)) for z in rng.integers(0, 1 << n, size=count)]      # one shared xmask: z & x carries the Ys
    yield [(int(x), int(z)) for x, z in zip(rng.choice(masks, size=40), rng.integers(0, 1 << n, size=40))]


def test_pauli_pass_args(ask):
    n, lists = 10, list(pauli_lists())
    answers = ask([f"paulisum {n} {len(terms)} " + " ".join(f"{x} {z}" for x, z in terms) for terms in lists])
    widths = set()
    for terms, answer in zip(lists, answers):
        passes = P.sum_plan(terms, 8)
        assert len(answer) == len(passes) + 1 and answer[-1] == []
        for p, tokens in zip(passes, answer):
            ok, width, items, xmask, pivot, odd, *zmask = nums(tokens)
            count = len(p["zmask"])
            low = (p["xmask"] & -p["xmask"]).bit_length() - 1      # the lowest flipped bit; -1: a diagonal pass
            assert ok == 1 and width == width_of(count) and width >= count
            assert items == ((1 << n) if low < 0 else (1 << n) // 2)
            assert xmask == p["xmask"] and pivot == max(low, 0)
            assert zmask == p["zmask"] + [0] * (8 - count)
            assert odd == sum((y & 1) << t for t, y in enumerate(p["n_y"]))
            widths.add((width, low < 0))
    assert widths == {(w, d) for w in (1, 2, 4, 8) for d in (False, True)}
    raw = [f"passraw {n} 3 0 {c} " + " ".join("5 1" for _ in range(c)) for c in (0, 1, 8, 9)]
    assert [nums(a[0])[0] for a in ask(raw)] == [0, 1, 1, 0], "1 .. 8 terms"


def test_pauli_rotate_args(ask):
    n, lists = 10, list(pauli_lists())
    rng = np.random.default_rng(23)
    angles = [rng.uniform(-3, 3, size=len(terms)) for terms in lists]
    requests = [f"paulirot {n} {len(terms)} " + " ".join(f"{x} {z} {float(np.cos(a / 2))!r} {float(np.sin(a / 2))!r}" for (x, z), a in zip(terms, th))
                for terms, th in zip(lists, angles)]
    widths = set()
    for terms, th, answer in zip(lists, angles, ask(requests)):
        passes = R.plan(terms)
        assert len(answer) == len(passes) + 1 and answer[-1] == []
        for p, tokens in zip(passes, answer):
            ok, width, items, xmask, pivot, diag, rot = nums(tokens[:7])
            zmask, cs, sn = nums(tokens[7:15]), floats(tokens[15:23]), floats(tokens[23:31])
            count = len(p["index"])
            assert ok == 1 and width == width_of(count) and len(tokens) == 31
            assert items == ((1 << n) if p["pivot"] < 0 else (1 << n) // 2)
            assert xmask == p["xmask"] and pivot == max(p["pivot"], 0)
            assert zmask == p["zmask"] + [0] * (8 - count)
            assert np.array_equal(cs, [np.cos(th[i] / 2) for i in p["index"]] + [1.0] * (8 - count)), "padded with the identity"
            assert np.array_equal(sn, [np.sin(th[i] / 2) for i in p["index"]] + [0.0] * (8 - count))
            flips = [t for t in range(count) if p["term_xmask"][t]]
            assert diag == sum(1 << t for t in range(8) if t not in flips), "diagonal terms and the padding"
            assert rot == sum((p["n_y"][t] & 3) << (2 * t) for t in flips)
            widths.add(width)
    assert widths == {1, 2, 4, 8}

    def raw(xmask, pivot, count, n_bits=n):
        return f"rotraw {n_bits} {xmask} {pivot} {count} " + " ".join(f"{xmask} 5 1" for _ in range(count))
    requests = [raw(0b110, 2, 1), raw(0b110, 2, 8), raw(0, -1, 3), raw(1 << 9, 9, 2),          # well-formed
                raw(0b110, 2, 0), raw(0b110, 2, 9),                                            # 1 .. 8 terms
                raw(1 << 9, 10, 2), raw(1 << 9, 63, 2), raw(1 << 9, 64, 2),                    # a pivot outside the register
                raw(0b110, -1, 2), raw(0, 2, 2),                                               # pivot and xmask disagree
                raw(1 << 10, 9, 2)]                                                            # xmask outside the register
    assert [nums(a[0])[0] for a in ask(requests)] == [1, 1, 1, 1] + [0] * 8
