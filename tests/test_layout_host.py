"""The host-side layouts of the dense-gate launchers (quantum_computations_amd/csrc/qsv_layout.h), on the host only.

tests/layout/layout_driver.cpp is compiled against the header with AddressSanitizer + UBSan; requests go in as text and
answers come back as text.  Every check compares the header with a NumPy model written here: target split and stand-in
bits, offset tables and the five matrix layouts end to end (gather, multiply, scatter on a 10-qubit state against the
oracle), the low-bit fields of the line-granular forms, SeqGate records, the pass cutter of k_seq_tile, the dispatch
ranges of split launches, the gate records of a k_pass_tile pass (executed by the model of test_defer_groups_host.py, bit
for bit against the gates applied one by one), the choice of kernel form, and the launch rules of the 1- and 2-qubit
register forms (items per thread, stride bit, tile order, grid) against a model of the launchers they were lifted from and
against the figures tests/test_gpu_options.py holds last_kernel() to.
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import defer_plan_model as base
import hostcheck
from defer_plan_model import interleaved, op_line, random_pass_list
from hostcheck import floats, nums, text
from oracle import dv_oracle as O
from quantum_computations_amd import workloads as W

GATE_TOL = 1e-13      # one gate, as tests/test_gpu_parity.py
MAT_COMPLEX, MAT_REAL, MAT_3M_ROWS, MAT_3M_ENTRIES, MAT_COLUMNS, MAT_COLUMNS_REAL = range(6)
FORM_GATHER, FORM_MFMA, FORM_MTILE5, FORM_TILE, FORM_LDS, FORM_BIG = range(6)
PASS_D2, PASS_D2X, PASS_D4, PASS_D4X, PASS_D4HL, PASS_PAIR, PASS_DIAG_T, PASS_DIAG_R1, PASS_DIAG_R2, PASS_DIAG_M = range(10)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "layout_driver.cpp", tmp_path_factory.mktemp("layout"))

    def run(requests):
        """requests: [str] -> one answer line per request, as a list of '|'-separated token lists."""
        lines = hostcheck.ask(exe, requests, timeout=600)
        return [[part.split() for part in line.split("|")] for line in lines]
    return run


# ---- split and stand-ins ------------------------------------------------------------------------------------------------
def split_cases():
    rng = np.random.default_rng(1)
    for k in range(3, 7):
        for n in (k + 5, k + 6):
            for size in range(k + 1):
                for low in itertools.combinations(range(6), size):
                    if k - size > n - 6:
                        continue            # k high targets do not fit k - 1 high bits
                    high = [int(b) for b in rng.choice(np.arange(6, n), size=k - size, replace=False)]
                    bits = list(low) + high
                    rng.shuffle(bits)
                    yield n, k, [int(b) for b in bits]


def test_split_and_standins(ask):
    cases = list(split_cases())
    assert len(cases) > 300
    answers = ask([f"split {n} {k} " + " ".join(map(str, bits)) for n, k, bits in cases])
    for (n, k, bits), (head, high, low, standin) in zip(cases, answers):
        enough, KB = nums(head)
        want_low = sorted(b for b in bits if b < 6)
        free = [b for b in range(6, n) if b not in bits]
        assert nums(high) == [b for b in bits if b >= 6] and nums(low) == want_low
        assert nums(standin) == free[:len(want_low)], "the lowest free bits >= 6"
        assert not set(nums(standin)) & set(bits)
        assert enough == int(len(free) >= len(want_low)) and KB == sum(b < 3 for b in bits)
        if want_low:
            assert enough == int(n == k + 6), "n = k + 5 has no room for stand-ins, n = k + 6 exactly enough"


# ---- offsets and matrix writers, end to end -------------------------------------------------------------------------------
def deposit(w, pos, or_mask):
    for p in sorted(pos):
        w = ((w >> p) << (p + 1)) | (w & ((1 << p) - 1))
    return w | or_mask


def read_matrix(layout, D, rows, data):
    """The written matrix read back through its layout, as the kernels index it."""
    def at(r, c):
        return ((r // rows) * D + c) * rows + r % rows if rows else r * D + c
    m = np.zeros((D, D), dtype=complex)
    for r in range(D):
        for c in range(D):
            if layout == MAT_COMPLEX:
                m[r, c] = complex(data[2 * at(r, c)], data[2 * at(r, c) + 1])
            elif layout == MAT_REAL:
                m[r, c] = data[at(r, c)]
            elif layout == MAT_3M_ROWS:
                re, im, both = data[3 * D * r + c], data[3 * D * r + D + c], data[3 * D * r + 2 * D + c]
                assert both == re + im, "plane three is plane one plus plane two, exactly"
                m[r, c] = complex(re, im)
            elif layout == MAT_3M_ENTRIES:
                re, im, both = data[3 * at(r, c):3 * at(r, c) + 3]
                assert both == re + im
                m[r, c] = complex(re, im)
            elif layout == MAT_COLUMNS:
                m[r, c] = complex(data[c * D + r], data[D * D + c * D + r])
            else:
                m[r, c] = data[c * D + r]
    return m


def gate_cases():
    """(form, k, bits, controls, kernel bit order, layout, rows, real matrix): the forms without a lane exchange."""
    n, rng = 10, np.random.default_rng(3)

    def legs(k, lowest):
        return [int(b) for b in rng.permutation(np.arange(lowest, n))[:k]]
    for k in range(1, 7):
        for trial in range(4):
            real = trial % 2 == 1
            if 3 <= k <= 5:         # k_dense_big<K, 0>: no transpose, kernel bit i <-> leg i
                bits = legs(k, 0)
                yield "big", k, bits, [], bits, MAT_3M_ROWS if k == 5 and trial == 2 else MAT_COMPLEX, 0, real
                bits = legs(k, 3)   # k_dense_tile: every target on bit 3 or higher, rows of a wave regrouped
                layout = MAT_REAL if real else MAT_3M_ENTRIES if k == 5 and trial == 2 else MAT_COMPLEX
                yield "tile", k, bits, [], bits, layout, {3: 2, 4: 4, 5: 8}[k], real
            if k <= 2:              # k_dense_tile12 / _ctrl: kernel bit i <-> leg i; k_dense with KL = 0: high targets in leg order
                bits = legs(k, 3 if k == 1 else 6)
                yield "tile12", k, bits, [], bits, MAT_COMPLEX, 0, real
                if k == 1:
                    ctrl = [int(b) for b in rng.permutation([b for b in range(3, n) if b not in bits])[:1 + trial % 2]]
                    yield "tile12", k, bits, ctrl, bits, MAT_COMPLEX, 0, real
                bits = legs(k, 6)
                yield "dense", k, bits, [], bits, MAT_COMPLEX, 0, real
            if k >= 5:              # k_dense_mfma: kernel bit i <-> the i-th lowest target
                bits = legs(k, 0)
                yield "mfma", k, bits, [], sorted(bits), MAT_COLUMNS_REAL if real else MAT_COLUMNS, 0, real


def test_offsets_and_matrix_layouts_end_to_end(ask):
    n = 10
    psi = W.random_ket(n, 5)
    cases = list(gate_cases())
    assert {c[0] for c in cases} == {"big", "tile", "tile12", "dense", "mfma"} and {c[5] for c in cases} == set(range(6))
    rng = np.random.default_rng(4)
    requests, mats = [], []
    for form, k, bits, ctrl, kb, layout, rows, real in cases:
        D = 1 << k
        u = np.linalg.qr(rng.standard_normal((D, D)))[0].astype(complex) if real else W.haar_unitary(D, rng)
        mats.append(u)
        # the test's own map from kernel index to the caller's matrix index: kernel bit i stands for target kb[i], which is
        # leg bits.index(kb[i]) of the matrix, leg 0 most significant
        ui = [sum(((c >> i) & 1) << (k - 1 - bits.index(kb[i])) for i in range(k)) for c in range(D)]
        requests.append(f"ui {k} " + " ".join(map(str, bits + kb)))
        requests.append(f"offsets {k} " + " ".join(map(str, kb)))
        requests.append(f"matrix {layout} {D} {rows} " + " ".join(map(str, ui)) + " " + text(interleaved(u)))
        requests.append(f"enum {(1 << n) >> (k + len(ctrl))} {sum(1 << b for b in ctrl)} {k + len(ctrl)} " + " ".join(map(str, bits + ctrl)))
        requests.append(f"order {n} {k} 0 0 " + " ".join(map(str, bits)))
    answers = iter(ask(requests))
    for (form, k, bits, ctrl, kb, layout, rows, real), u in zip(cases, mats):
        D = 1 << k
        ui = [sum(((c >> i) & 1) << (k - 1 - bits.index(kb[i])) for i in range(k)) for c in range(D)]
        (got_ui,), (off,), (written,), (enum,), order = (next(answers) for _ in range(5))
        assert nums(got_ui) == ui
        off = np.array(nums(off))
        assert list(off) == [sum(((c >> i) & 1) << kb[i] for i in range(k)) for c in range(D)]
        assert int(written[0]) == int(real)
        m = read_matrix(layout, D, rows, floats(written[1:]))
        Wn, or_mask, nins, *pos = nums(enum)
        assert pos == sorted(bits + ctrl) and nins == len(pos) and or_mask == sum(1 << b for b in ctrl)
        if form in ("big", "tile", "tile12"):      # without a transpose every target is its own kernel, address and inserted bit
            assert nums(order[0]) == bits and nums(order[1]) == bits and nums(order[2]) == sorted(bits)
        base_index = np.array([deposit(w, pos, or_mask) for w in range(Wn)])
        index = base_index[:, None] + off[None, :]            # x[c] = a[deposit(w) + off[c]]
        assert len(set(index.reshape(-1).tolist())) == index.size, "every amplitude at most once"
        got = psi.copy()
        got[index] = psi[index] @ m.T
        want = O.apply_gate(psi, u, [n - 1 - b for b in bits])
        if ctrl:
            on = np.array([all((i >> b) & 1 for b in ctrl) for i in range(1 << n)])
            want = np.where(on, want, psi)
        assert np.max(np.abs(got - want)) < GATE_TOL, (form, k, bits, ctrl, layout)


# ---- low-bit fields --------------------------------------------------------------------------------------------------------
def test_low_bit_fields_of_the_line_granular_forms(ask):
    cases = [(n, k, bits) for n, k, bits in split_cases() if n == k + 6]
    answers = ask([f"low {n} {k} " + " ".join(map(str, bits)) for n, k, bits in cases])
    for (n, k, bits), (head, abit, aE, bdep) in zip(cases, answers):
        amask, bmask, na = nums(head)
        low = sorted(b for b in bits if b < 6)
        standin = [b for b in range(6, n) if b not in bits][:len(low)]
        A, B = [b for b in low if b >= 3], [b for b in low if b < 3]
        assert amask == sum(1 << b for b in A) and bmask == sum(1 << b for b in B)
        assert na == len(A) and na + len(B) == len(low)
        assert list(zip(nums(abit), nums(aE))) == [(b, standin[low.index(b)]) for b in A], "each A target with its stand-in"
        want = [sum(((v >> j) & 1) << B[j] for j in range(len(B))) if v < (1 << len(B)) else 0 for v in range(8)]
        assert nums(bdep) == want


# ---- SeqGate records -------------------------------------------------------------------------------------------------------
def apply_seq_record(x, code, m, width):
    """seq_apply1 / seq_apply2 on the 2^width amplitudes of a thread."""
    x = x.copy()
    idx = np.arange(1 << width)
    if code < 5:
        m2 = (m[0:8:2] + 1j * m[1:8:2]).reshape(2, 2)
        lo0 = idx[(idx >> code) & 1 == 0]
        a0, a1 = x[lo0], x[lo0 | 1 << code]
        x[lo0], x[lo0 | 1 << code] = m2[0, 0] * a0 + m2[0, 1] * a1, m2[1, 0] * a0 + m2[1, 1] * a1
        return x
    pairs = [(hi, lo) for hi in range(1, 5) for lo in range(hi)]      # the numbering documented on SeqGate: 5 + p
    hi, lo = pairs[code - 5]
    m4 = (m[0::2] + 1j * m[1::2]).reshape(4, 4)
    zero = idx[((idx >> hi) & 1 == 0) & ((idx >> lo) & 1 == 0)]
    ins = [x[zero | (r >> 1) << hi | (r & 1) << lo] for r in range(4)]
    for r in range(4):
        x[zero | (r >> 1) << hi | (r & 1) << lo] = sum(m4[r, c] * ins[c] for c in range(4))
    return x


def test_seq_records_on_every_pair_of_register_bits(ask):
    rng = np.random.default_rng(6)
    x = W.random_ket(5, 9)
    cases = [(2, j0, j1, W.haar_unitary(4, rng)) for j0 in range(5) for j1 in range(5) if j0 != j1]
    cases += [(1, j, 0, W.haar_unitary(2, rng)) for j in range(5)]
    assert len({(max(a, b), min(a, b)) for _, a, b, _ in cases[:20]}) == 10
    answers = ask([f"seq {arity} {j0} {j1} " + text(interleaved(u)) for arity, j0, j1, u in cases])
    codes = set()
    for (arity, j0, j1, u), (ans,) in zip(cases, answers):
        code, m = int(ans[0]), floats(ans[1:])
        codes.add(code)
        if arity == 1:
            assert code == j0
            want = O.apply_gate(x, u, [4 - j0])
        else:
            hi, lo = max(j0, j1), min(j0, j1)
            assert code == 5 + [(h, l) for h in range(1, 5) for l in range(h)].index((hi, lo))
            want = O.apply_gate(x, u, [4 - j0, 4 - j1])
        assert np.max(np.abs(apply_seq_record(x, code, m, 5) - want)) < GATE_TOL, (arity, j0, j1)
    assert codes == set(range(15))


# ---- pass cutter of k_seq_tile ---------------------------------------------------------------------------------------------
def model_tile_cut(n, k, bits, gates):
    tile_bits = sorted(bits + [b for b in range(n) if b not in bits][:12 - k])
    passes = []
    for g, (arity, l0, l1) in enumerate(gates):
        where = [tile_bits.index(bits[l0])] + ([tile_bits.index(bits[l1])] if arity == 2 else [])
        merged = list(passes[-1][0]) if passes else []
        merged += [t for t in where if t not in merged]
        if not passes or len(merged) > 4:
            passes.append(([], []))
            merged = where
        passes[-1] = (merged, passes[-1][1] + [g])
    done = []
    for q, members in passes:
        q = sorted(q + [t for t in range(12) if t not in q][:4 - len(q)])      # completed with the lowest unused tile indices
        done.append((q, members))
    return tile_bits, done


def test_tile_pass_cutter(ask):
    rng = np.random.default_rng(8)
    (limits,), = ask(["limits"])
    max_passes = int(limits[2])
    cases = []
    for trial in range(120):
        n, k = (12, 17)[trial % 2], 1 + trial % 6
        bits = [int(b) for b in rng.choice(n, size=k, replace=False)]
        gates = []
        for _ in range(int(rng.integers(1, 49))):
            if k == 1 or rng.random() < 0.4:
                gates.append((1, int(rng.integers(k)), 0))
            else:
                l0, l1 = (int(v) for v in rng.choice(k, size=2, replace=False))
                gates.append((2, l0, l1))
        cases.append((n, k, bits, gates))
    # 52 gates that need 26 passes: two 2-qubit gates fit four bits, the third pair does not
    cases.append((12, 6, [0, 1, 2, 3, 4, 5], [(2, 2 * (g % 3), 2 * (g % 3) + 1) for g in range(52)]))
    requests = []
    for n, k, bits, gates in cases:
        body = " ".join(f"{a} {l0} {l1} " + text(np.arange(8 if a == 1 else 32) + 100 * g) for g, (a, l0, l1) in enumerate(gates))
        requests.append(f"tilecut {n} {k} {len(gates)} " + " ".join(map(str, bits)) + " " + body)
    answers = ask(requests)
    assert nums(answers[-1][0]) == [1], "more passes than the kernel's table holds: unhandled"
    assert len(model_tile_cut(*cases[-1])[1]) == 26 > max_passes
    for (n, k, bits, gates), ans in zip(cases[:-1], answers[:-1]):
        assert nums(ans[0]) == [0]
        tile_bits, passes = model_tile_cut(n, k, bits, gates)
        assert len(passes) <= max_passes and nums(ans[1]) == tile_bits
        got = nums(ans[2])
        assert got[0] == len(passes)
        rec = ans[3]
        assert len(rec) == 33 * len(gates), "every gate exactly once"
        at = 0
        for p, (q, members) in enumerate(passes):
            first, count, *gq = got[1 + 6 * p:7 + 6 * p]
            assert (first, count) == (at, len(members)) and members == list(range(at, at + count)), "in order"
            assert gq == q and len(set(gq)) == 4 and gq == sorted(gq)
            for g in members:
                arity, l0, l1 = gates[g]
                code, m = int(rec[33 * g]), floats(rec[33 * g + 1:33 * g + 33])
                t0 = tile_bits.index(bits[l0])
                if arity == 1:
                    assert gq[code] == t0 and list(m[:8]) == list(np.arange(8) + 100.0 * g)
                else:
                    hi, lo = [(h, l) for h in range(1, 4) for l in range(h)][code - 5]
                    assert {gq[hi], gq[lo]} == {t0, tile_bits.index(bits[l1])}
                    assert sorted(m) == sorted(np.arange(32) + 100.0 * g)
            at += count
        assert at == len(gates)


# ---- dispatch ranges -------------------------------------------------------------------------------------------------------
def test_dispatch_ranges(ask):
    (limits,), = ask(["limits"])
    tiles, items = int(limits[0]), int(limits[1])
    assert tiles == 1 << 23 and items == 0x00ffffff * 256
    cases = [(W_, limit) for limit in (tiles * 64, tiles, items) for W_ in (limit - 64, limit, limit + 64, 3 * limit)]
    for (W_, limit), (ans,) in zip(cases, ask([f"ranges {a} {b}" for a, b in cases])):
        v = nums(ans)
        chunks = list(zip(v[0::2], v[1::2]))
        at = 0
        for w0, count in chunks:
            assert w0 == at and 0 < count <= limit
            at += count
        assert at == W_, "contiguous, covering [0, W)"
        if limit != items:
            assert all(count == limit and w0 % limit == 0 for w0, count in chunks[:-1]) and chunks[-1][0] % limit == 0


# ---- gate records of one pass ----------------------------------------------------------------------------------------------
def tile12_takes(n, k, bits, ctrl):
    if ctrl and k != 1 or any(c < 3 for c in ctrl):
        return False
    Wn = (1 << n) >> (k + len(ctrl))
    return not (min(bits) < (3 if k == 1 else 6) or Wn < 64 or Wn % 64)


def record_as_rec(n, r, form, code, rc, tc, tz0, tz1, m, q, tindex):
    """One PassGate record as a gate on TILE indices (what the kernel does with it), re-expressed in the caller's leg order
    so that the model sums products in the order of the gate applied on its own."""
    cmask = tc | sum(1 << q[j] for j in range(4) if (rc >> j) & 1)
    d = m[0:8:2] + 1j * m[1:8:2]
    if form in (PASS_D2, PASS_D2X):
        want = PASS_D2 if tile12_takes(n, 1, r.targets, r.ctrl) or r.targets[0] >= 6 else PASS_D2X
        assert form == want and q[code] == tindex(r.targets[0])
        return base.Rec("dense", [q[code]], [], d.reshape(2, 2)), cmask
    if form in (PASS_D4, PASS_D4X, PASS_D4HL):
        low = sum(b < 6 for b in r.targets)
        want = PASS_D4 if tile12_takes(n, 2, r.targets, r.ctrl) or low == 0 else PASS_D4X if low == 2 else PASS_D4HL
        assert form == want
        t0, t1 = q[code // 4], q[code % 4]                  # tile indices of kernel bits 0 and 1
        m4 = (m[0::2] + 1j * m[1::2]).reshape(4, 4)
        L0, L1 = (tindex(b) for b in r.targets)
        assert {t0, t1} == {L0, L1}
        if L0 == t0:                                        # the caller's leg 0 is kernel bit 0: swap the index bits back
            swap = [0, 2, 1, 3]
            m4 = m4[np.ix_(swap, swap)]
        if form == PASS_D4HL:
            assert t0 < 6 <= t1, "kernel bit 0 is the low target"
        return base.Rec("dense", [L0, L1], [], m4), cmask
    if form == PASS_PAIR:
        lo, hi = code // 4, code % 4
        assert lo < hi and {q[lo], q[hi]} == {tindex(b) for b in r.targets}
        return base.Rec("pair", [q[lo], q[hi]], [], base.X), cmask
    regs = set(q)
    if form == PASS_DIAG_T:
        assert not {tz0, tz1} & regs or r.kind == "phase"
        return base.Rec("diag", [tz0, tz1], [], d), cmask
    if form == PASS_DIAG_R1:
        return base.Rec("diag", [q[code]], [], d[:2]), cmask
    if form == PASS_DIAG_R2:
        assert code // 4 < code % 4
        return base.Rec("diag", [q[code // 4], q[code % 4]], [], d), cmask
    assert form == PASS_DIAG_M and tz0 not in regs
    return base.Rec("diag", [q[code], tz0], [], d), cmask


def test_pass_records_reproduce_the_gates_applied_one_by_one(ask):
    rng = np.random.default_rng(12)
    cases = []
    for trial in range(24):
        n = 12 + trial % 2
        tile = sum(1 << b for b in (range(6, 12) if n == 12 else [b for b in range(6, 13) if b != 6 + trial % 7]))
        cases.append((n, tile, random_pass_list(rng, n, tile), W.random_ket(n, 200 + trial)))
    answers = ask([f"pass {n} {tile} {len(recs)} " + " ".join(op_line(r) for r in recs) for n, tile, recs, _ in cases])
    seen, outside = set(), 0
    for (n, tile, recs, psi), ans in zip(cases, answers):
        assert nums(ans[0]) == [0]
        tbits = list(range(6)) + [b for b in range(6, n) if (tile >> b) & 1]
        assert nums(ans[1]) == tbits
        g = nums(ans[2])
        groups = [g[1 + 7 * p:8 + 7 * p] for p in range(g[0])]
        rec = ans[3]
        assert len(rec) == 39 * len(recs)
        want = psi.copy()
        for r in recs:
            base.apply_rec(want, r, lambda b: b, r.ctrl_mask)
        others = [b for b in range(n) if b not in tbits]
        local = np.arange(1 << 12)
        offset = sum(((local >> i) & 1) << b for i, b in enumerate(tbits))
        got = psi.copy()
        for w in range(1 << len(others)):
            origin = sum(((w >> i) & 1) << b for i, b in enumerate(others))
            omask = [int(rec[39 * i + 6]) for i in range(len(recs))]
            active = [origin & o == o for o in omask]
            if not any(active):
                continue
            v = got[origin | offset]
            at = 0
            for first, count, q0, q1, q2, q3, members in groups:
                assert first == at and members == sum(1 << i for i in range(first, first + count))
                at += count
                if not any(active[first:first + count]):
                    continue
                for i in range(first, first + count):
                    if not active[i]:
                        continue
                    form, code, rc, tc, tz0, tz1 = nums(rec[39 * i:39 * i + 6])
                    seen.add(form)
                    outside += omask[i] != 0
                    assert omask[i] == sum(1 << b for b in recs[i].ctrl if b not in tbits)
                    as_rec, cmask = record_as_rec(n, recs[i], form, code, rc, tc, tz0, tz1, floats(rec[39 * i + 7:39 * i + 39]),
                                                  [q0, q1, q2, q3], lambda b: base.tile_index(b, tile))
                    assert cmask == sum(1 << base.tile_index(b, tile) for b in recs[i].ctrl if b in tbits)
                    base.apply_rec(v, as_rec, lambda t: t, cmask)
            assert at == len(recs)
            got[origin | offset] = v
        assert np.array_equal(got, want)
    assert seen == set(range(10)), seen
    assert outside > 0, "n = 13: controls outside the tile decide per tile"


# ---- form selection --------------------------------------------------------------------------------------------------------
def expected_form(n, k, variant, real, all_from_bit3, has_low):
    """The form qsvk_generic takes (QSV_OPT_COMPLEX_PRODUCT = 0, QSV_MTILE unset), as the comments of choose_form say."""
    fits = n - k >= 6                      # whole waves of columns: n = k + 8 yes, n = k + 5 no
    if k <= 2:
        return FORM_GATHER, False, False, False
    if (k == 6 and variant == 0) or (k == 5 and variant == 5):
        return FORM_MFMA, False, real, not real             # 16 groups fill a wave at both sizes; complex: three MFMAs
    if k == 6:                                              # only the line-granular kernel is built for 64 x 64 matrices
        return (FORM_LDS, has_low and variant != 2, real, False) if fits else (FORM_GATHER, False, False, False)
    tile_ok = all_from_bit3 and fits
    table = {
        0: FORM_TILE if tile_ok and (k <= 4 or real) else FORM_LDS if fits and k == 5 and (has_low or real) else FORM_BIG,
        1: FORM_BIG,                                        # wave shuffles
        2: FORM_BIG,                                        # no transpose
        3: FORM_LDS if fits else FORM_BIG,                  # line-granular
        4: FORM_TILE if tile_ok else FORM_BIG,              # workgroup tile
        5: FORM_BIG,                                        # k = 3, 4: no override applies
        6: FORM_MTILE5 if tile_ok and k == 5 and not real else FORM_BIG,
    }
    form = table[variant]
    transposed = has_low and fits and variant != 2 and form in (FORM_LDS, FORM_BIG)    # stand-ins exist at n = k + 8 only
    return form, transposed, real and form in (FORM_TILE, FORM_LDS), False


def test_form_selection(ask):
    cases = []
    for k in range(1, 7):
        for n in (k + 5, k + 8):
            placements = [(False, True, list(range(3))[:min(k, 2)] + list(range(6, 6 + max(k - 2, 0)))),     # a target below bit 3
                          (True, True, [3, 4][:min(k, 2)] + list(range(6, 6 + max(k - 2, 0))))]              # low targets on 3..5
            if n == k + 8:
                placements.append((True, False, list(range(7, 7 + k))))                                       # all high
            for all3, has_low, bits in placements:
                for variant in range(7):
                    for real in (False, True):
                        cases.append((n, k, variant, real, all3, has_low, bits[::-1]))
    answers = ask([f"form {n} {k} {int(real)} {variant} 0 0 " + " ".join(map(str, bits)) for n, k, variant, real, _, _, bits in cases])
    seen = set()
    for (n, k, variant, real, all3, has_low, bits), (ans,) in zip(cases, answers):
        assert max(bits) < n and (min(bits) >= 3) == all3 and (min(bits) < 6) == has_low
        want = expected_form(n, k, variant, real, all3, has_low)
        got = nums(ans)
        assert (got[0], bool(got[1]), bool(got[2]), bool(got[3])) == want, (n, k, variant, real, bits, got, want)
        seen.add(got[0])
    assert seen == set(range(6))


# ---- launch rules of the 1- and 2-qubit register forms ----------------------------------------------------------------------
# The model is the parent commit's launch_dense / default_unroll / launch_diag (then inline in the gate-kernel file), kept
# in their shape: the far-stride scan once in default_unroll and once more in launch_dense, the single-stride special case,
# the halving loop, the tile-order table, the stride-bit clamp, grid_for.
BLOCK = 256


def parent_grid_for(items, per_block, cap):
    blocks = max((items + per_block - 1) // per_block, 1)
    if cap > 0:
        blocks = min(blocks, cap)
    return min(blocks, 0x00FFFFFF)


def parent_default_unroll(KH, KL, hbit):
    if KH == 0:
        return 2 if KL == 2 else 1
    far = False
    for b in hbit[:KH]:
        far = far or 20 <= b <= 25
    if KH == 1 and KL == 1:
        return 1
    if KH == 1 and KL == 0 and far:
        return 4 if hbit[0] == 20 else 1
    return 4 if far else 1


def parent_launch_dense(KH, KL, hbit, sub, W, unroll, remap, ubit, cap):
    U = unroll if unroll > 0 else parent_default_unroll(KH, KL, hbit)
    while U > 1 and W < BLOCK * U:
        U >>= 1
    if remap >= 0:
        regions = remap
    else:
        top = 0
        for b in hbit[:KH]:
            top = max(top, b)
        if sub:
            regions = 0
        elif KH == 0:
            regions = 0 if KL == 2 else 32
        elif KH == 1 and KL == 0:
            regions = 0 if top == 20 else 2 if top == 24 else 8
        elif KH == 1:
            regions = 32 if top in (20, 24) else 8
        else:
            regions = 8 if top < 20 else 0
    while ubit > 8 and (W >> ubit) < U:
        ubit -= 1
    return U, ubit, regions, parent_grid_for(W, BLOCK * U, cap)


def parent_launch_diag(sub, W, unroll, remap, ubit, cap):
    regions = remap if remap >= 0 else (8 if sub else 32)
    U = unroll if unroll > 0 else (4 if sub else 1)
    while U > 1 and W < BLOCK * U:
        U >>= 1
    return U, ubit, regions, parent_grid_for(W, BLOCK * U, cap)      # k_diag has no stride bit: passed through


def launch12_line(KH, KL, hbit, sub, W, unroll, remap, ubit, cap):
    return f"launch12 {KH} {KL} {int(sub)} {W} {unroll} {remap} {ubit} {cap} {hbit[0]} {hbit[1]}"


def launch12_cases():
    """(KH, KL, hbit, sub, W, unroll, remap, ubit, cap); KH = -1 is the diagonal launch."""
    unset = (0, -1, 8, 0)
    one_at_a_time = [unset] + [(u, -1, 8, 0) for u in (1, 2, 4, 8)] + [(0, r, 8, 0) for r in (0, 2, 8, 32)] \
        + [(0, -1, b, 0) for b in (8, 10, 12)] + [(0, -1, 8, c) for c in (0, 3, 7)]
    product = list(itertools.product((0, 1, 2, 4, 8), (-1, 0, 2, 8, 32), (8, 10, 12), (0, 3, 7)))
    placements = []
    for b in range(6, 28):                                     # every high-target position, alone and as one of a pair
        placements += [(1, 0, (b, 0)), (1, 1, (b, 0))]
        placements += [(2, 0, pair) for other in (6, 20, 23, 27) if other != b for pair in ((b, other), (other, b))]
    placements += [(0, 1, (0, 0)), (0, 2, (0, 0)), (-1, 0, (0, 0))]
    for KH, KL, hbit in placements:
        # the full product of the options on a sample of placements (a near, a 16 MiB and a 256 MiB stride), one option
        # at a time on the others
        combined = KH <= 0 or (KH == 1 and hbit[0] in (6, 20, 24)) or hbit in ((7, 6), (20, 23), (6, 24))
        for options in (product if combined else one_at_a_time):
            for sub in (False, True):
                for logw in range(7, 28):
                    yield (KH, KL, hbit, sub, 1 << logw, *options)


def test_launch_rules_of_the_register_forms(ask):
    cases = list(launch12_cases())
    answers = ask([launch12_line(*c) for c in cases])
    tops, halved, clamped = set(), set(), set()
    for case, (ans,) in zip(cases, answers):
        KH, KL, hbit, sub, W, unroll, remap, ubit, cap = case
        want = parent_launch_diag(sub, W, unroll, remap, ubit, cap) if KH < 0 else parent_launch_dense(*case)
        assert tuple(nums(ans)) == want, (case, nums(ans), want)
        if KH > 0 and remap < 0 and not unroll:
            top = max(hbit[:KH])
            tops.add("<20" if top < 20 else "21..23" if 21 <= top <= 23 else ">25" if top > 25 else str(top))
        start = unroll or ((4 if sub else 1) if KH < 0 else parent_default_unroll(KH, KL, hbit))     # U before the halving
        if start > 1:
            halved.add(want[0] < start)
        if KH >= 0 and ubit > 8:
            clamped.add(want[1] < ubit)
    assert {(c[0], c[1]) for c in cases} == {(1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (-1, 0)}
    assert tops == {"<20", "20", "21..23", "24", "25", ">25"}, tops
    assert halved == {False, True} and clamped == {False, True}, "the U halving and the stride-bit clamp both fire and both do not"


def gpu_option_settings():
    """SETTINGS of tests/test_gpu_options.py, read from its source (importing the module would load the GPU library)."""
    import ast
    tree = ast.parse((hostcheck.HERE / "test_gpu_options.py").read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and [getattr(t, "id", None) for t in node.targets] == ["SETTINGS"]:
            return ast.literal_eval(node.value)
    raise AssertionError("SETTINGS not found in tests/test_gpu_options.py")


def test_launch_rules_give_what_the_gpu_option_settings_record(ask):
    """Rows A..N of SETTINGS: the (U, stride bit, tiles) that test_gpu_options.py holds last_kernel() to, asked of the header."""
    rows = [s for s in gpu_option_settings() if s[7] is not None]
    assert [s[0] for s in rows] == list("ABCDEFGHIJMN")
    requests, wants = [], []
    for name, n, nt, unroll, regions, ubit, cap, high, low in rows:
        for kind, W, want in (((1, 0), 1 << (n - 1), high), ((0, 1), 1 << n, low), ((-1, 0), 1 << n, low)):
            requests.append(launch12_line(kind[0], kind[1], (n - 1, 0), False, W, unroll, regions, ubit, cap))
            wants.append((name, kind, W, cap, want))
    for (name, kind, W, cap, want), (ans,) in zip(wants, ask(requests)):
        U, stride_bit, remap, grid = nums(ans)
        tiles = -(-W // (BLOCK * U))
        assert grid == (min(tiles, cap) if cap else tiles), (name, kind)
        trips = -(-tiles // grid)
        if kind[0] < 0:                                        # k_diag has no stride bit
            assert (U, tiles, trips) == (want[0], want[2], want[4]), (name, kind)
        else:
            assert (U, stride_bit, tiles, trips) == (want[0], want[1], want[2], want[4]), (name, kind)
