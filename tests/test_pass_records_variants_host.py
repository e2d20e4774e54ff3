"""What pass_records (quantum_computations_amd/csrc/qsv_layout.h) hands the pass kernel for its body variants, on the host.

tests/layout/pass_variants_driver.cpp is compiled against the header with AddressSanitizer + UBSan and run on its own.
For random gate lists the control class of every gate, the packed array of outside-control masks and the every-tile flag
are compared with a model written here; for gate lists without controls the records must be, field for field and double
for double, the ones recorded before those fields existed (tests/golden/pass_records_uncontrolled.json), and every byte
of a record outside its named fields must be zero.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import defer_plan_model as base
import hostcheck
from defer_plan_model import op_line, random_pass_list
from hostcheck import nums
from quantum_computations_amd import workloads as W

CTL_NONE, CTL_REG, CTL_THREAD = range(3)
GOLDEN = hostcheck.HERE / "golden" / "pass_records_uncontrolled.json"


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = hostcheck.compile_driver(hostcheck.HERE / "layout" / "pass_variants_driver.cpp", tmp_path_factory.mktemp("pass_variants"))

    def run(requests):
        lines = hostcheck.ask(exe, requests, timeout=600)
        return [[part.split() for part in line.split("|")] for line in lines]
    return run


def test_record_layout(ask):
    """The fields of before in their order, the control class in front of omask, no padding beyond its alignment."""
    (v,), = ask(["layout"])
    size, form, code, rc, tc, tz0, tz1, ctl, omask, m = nums(v)
    assert (form, code, rc, tc, tz0, tz1, ctl) == (0, 4, 8, 12, 16, 20, 24)
    assert omask == 32 and m == 40 and size == 40 + 32 * 8


def cases():
    rng = np.random.default_rng(31)
    out = []
    for trial in range(30):
        n = 12 + trial % 3
        high = sorted(int(b) for b in rng.choice(np.arange(6, n), size=6, replace=False))
        tile = sum(1 << b for b in high)
        recs = random_pass_list(rng, n, tile)
        if trial % 5 == 4:               # every gate controlled from outside the tile, where the register has such bits
            outside = [b for b in range(6, n) if b not in high]
            recs = [r for r in recs if set(r.ctrl) & set(outside)]
        if recs:
            out.append((n, tile, recs))
    return out


def test_control_class_packed_omasks_and_every_tile_flag(ask):
    todo = cases()
    answers = ask([f"pass {n} {tile} {len(recs)} " + " ".join(op_line(r) for r in recs) for n, tile, recs in todo])
    classes, flags = set(), set()
    for (n, tile, recs), ans in zip(todo, answers):
        assert nums(ans[0]) == [0]
        tbits = list(range(6)) + [b for b in range(6, n) if (tile >> b) & 1]
        g = nums(ans[1])
        groups = [g[1 + 7 * p:8 + 7 * p] for p in range(g[0])]
        rec, ctl, packed = ans[2], nums(ans[3]), nums(ans[4])
        assert len(rec) == 39 * len(recs) and len(ctl) == len(recs) and len(packed) == len(recs)
        group_of = {}
        for first, count, q0, q1, q2, q3, members in groups:
            for i in range(first, first + count):
                group_of[i] = [q0, q1, q2, q3]
        assert sorted(group_of) == list(range(len(recs)))
        for i, r in enumerate(recs):
            q = group_of[i]
            inside = [tbits.index(b) for b in r.ctrl if b in tbits]           # controls as tile indices
            want_rc = sum(1 << q.index(t) for t in inside if t in q)
            want_tc = sum(1 << t for t in inside if t not in q)
            want_omask = sum(1 << b for b in r.ctrl if b not in tbits)
            form, code, got_rc, got_tc, tz0, tz1, got_omask = nums(rec[39 * i:39 * i + 7])
            assert (got_rc, got_tc, got_omask) == (want_rc, want_tc, want_omask), (n, tile, i)
            want_ctl = CTL_THREAD if want_tc else CTL_REG if want_rc else CTL_NONE
            assert ctl[i] == want_ctl, (n, tile, i, r.kind, r.ctrl, q)
            assert packed[i] == want_omask
            classes.add(want_ctl)
        every = int(any(all(b in tbits for b in r.ctrl) for r in recs))
        assert nums(ans[5]) == [every]
        flags.add(every)
        assert nums(ans[6]) == [1] * len(recs), "no byte set outside the named fields"
    assert classes == {CTL_NONE, CTL_REG, CTL_THREAD} and flags == {0, 1}


def test_records_of_gate_lists_without_controls_are_the_recorded_ones(ask):
    golden = json.loads(GOLDEN.read_text())
    answers = ask(golden["requests"])
    assert len(answers) == 4
    for ans, line in zip(answers, golden["answers"]):
        status, tile_bits, groups, records = [part.split() for part in line.split("|")]
        assert ans[0] == status == ["0"]
        assert ans[1] == groups
        assert ans[2] == records, "form, code, rc, tc, tz0, tz1, omask and the 32 doubles of every record"
        count = len(records) // 39
        assert nums(ans[3]) == [CTL_NONE] * count and nums(ans[4]) == [0] * count and nums(ans[5]) == [1]
        assert nums(ans[6]) == [1] * count


@pytest.mark.parametrize("kind", ["cu", "CX"])
def test_control_classes_of_the_gpu_test_gate_lists(ask, kind):
    """The gate lists of tests/test_gpu_pass_variants.py::test_control_classes_back_to_back_on_every_register_position,
    for the targets on tile bits, as the queue classifies them (a controlled 2 x 2 with its control on bit 3 or higher is
    a dense 1-qubit gate with one control), on the tile of bits 0..11 of a 14-qubit register: after the Haar 4x4 the
    classes are none, register, thread, none, thread, register, none (bit 13 is outside the tile), thread, none, none."""
    n, tile = 14, sum(1 << b for b in range(6, 12))
    rng = np.random.default_rng(5)
    requests, wants = [], []
    for t in range(12):
        r = (t + 1) % 12
        s = next(b for b in (3, 4, 5) if b not in (t, r))
        recs = [base.Rec("dense", [t, r], [], W.haar_unitary(4, rng))]
        ctrls = (None, r, s, None, s, r, 13, s, 12, None)
        for ctrl in ctrls:
            u = base.X if kind == "CX" else W.haar_unitary(2, rng)
            recs.append(base.Rec("dense", [t], [] if ctrl is None else [ctrl], u))
        recs.append(base.Rec("dense", [r], [], W.haar_unitary(2, rng)))
        requests.append(f"pass {n} {tile} {len(recs)} " + " ".join(op_line(x) for x in recs))
        wants.append((t, r, s))
    for (t, r, s), ans in zip(wants, ask(requests)):
        assert nums(ans[0]) == [0]
        g = nums(ans[1])
        assert g[0] == 1, "one group: targets t and r only"
        q = g[3:7]
        assert t in q and r in q and s not in q, (t, r, s, q)
        ctl, packed = nums(ans[3]), nums(ans[4])
        assert ctl == [CTL_NONE, CTL_NONE, CTL_REG, CTL_THREAD, CTL_NONE, CTL_THREAD, CTL_REG, CTL_NONE, CTL_THREAD,
                       CTL_NONE, CTL_NONE, CTL_NONE], (t, ctl)
        assert packed == [0, 0, 0, 0, 0, 0, 0, 1 << 13, 0, 1 << 12, 0, 0]
        assert all(a != b for a, b in zip(ctl[1:4], ctl[2:5])) and ctl[4:7] == [CTL_NONE, CTL_THREAD, CTL_REG]
