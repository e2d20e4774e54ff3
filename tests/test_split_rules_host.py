"""The host-side rules of the MPS splits (quantum_computations_amd/csrc/qsv_split_rules.h) and the pair schedule of the
Jacobi kernels (qsv_jacobi.h), on the host only.

tests/layout/split_rules_driver.cpp is compiled against the two headers with AddressSanitizer + UBSan, as the other layout
tests compile theirs; requests go in as text and answers come back as text.  The models below are written from the
reference's rule (mps.py:83-86) and from the comments of the split code; where a model transcribes an expression it keeps
the order of the floating-point operations, so that equality is exact.
"""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

import hostcheck

EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return hostcheck.compile_driver(hostcheck.HERE / "layout" / "split_rules_driver.cpp", tmp_path_factory.mktemp("split_rules"))


@pytest.fixture(scope="module")
def ask(exe):
    return lambda requests: hostcheck.ask(exe, requests, timeout=900)


def num(value):
    return repr(float(value))


def vec(values):
    return f"{len(values)} " + hostcheck.text(values)


def total_of(s):
    return float(np.cumsum(s)[-1]) if len(s) else 0.0      # added in index order, as the header adds


def tails_of(s):
    return np.cumsum(np.asarray(s, dtype=float)[::-1])[::-1]    # tails[i] = s[i] + ... + s[-1], added from the end


def model_allowed(s, abs_err, rel_err):
    return max(abs_err, total_of(s) * rel_err, 0.0)


def model_rank_for(s, cap, allowed):
    r = int(np.count_nonzero(tails_of(s) > allowed))
    if cap >= 0:
        r = min(r, cap)
    return min(r, len(s))


def model_rank(s, cap, abs_err, rel_err):
    """allowed = max(abs_err, rel_err * sum(s), 0); every index whose tail sum exceeds it is kept; then the cap."""
    return model_rank_for(s, cap, model_allowed(s, abs_err, rel_err))


# ---- the pair schedule -----------------------------------------------------------------------------------------------
def test_tournament_pairs_every_two_columns_once(ask):
    sizes = list(range(2, 67, 2)) + [128, 256, 2048]
    for lp, line in zip(sizes, ask([f"schedule {lp}" for lp in sizes])):
        pairs = np.array(line.split(), dtype=np.int64).reshape(lp - 1, lp // 2, 2)
        p, q = pairs[..., 0], pairs[..., 1]
        assert np.all(p < q) and p.min() >= 0 and q.max() == lp - 1, lp
        assert np.array_equal(np.sort(pairs.reshape(lp - 1, lp), axis=1), np.tile(np.arange(lp), (lp - 1, 1))), lp   # disjoint
        assert len(np.unique(p * lp + q)) == lp * (lp - 1) // 2, lp                 # every unordered pair exactly once
        assert np.all(np.count_nonzero(q >= lp - 1, axis=1) == 1), lp               # odd l = lp - 1: one pair sits out


# ---- the truncation rule ---------------------------------------------------------------------------------------------
def spectra():
    rng = np.random.default_rng(31)
    for n in range(1, 301):
        yield np.exp(-rng.uniform(0.03, 0.7) * np.arange(n)) * rng.uniform(0.1, 10.0)                        # geometric
        yield np.sort(rng.uniform(0.05, 1.0, n) * 10.0 ** rng.uniform(-3, 3))[::-1]                          # random, sorted


def test_truncation_rule_against_the_model(ask):
    rng = np.random.default_rng(32)
    requests, want = [], []
    for s in spectra():
        n, tails = len(s), np.append(tails_of(s), 0.0)
        for j in {-1, n - 1, int(rng.integers(0, n)), int(rng.integers(0, n))}:
            # a threshold between tails[j] and tails[j + 1] (geometric mean: rounding of the sums cannot flip a case);
            # j = -1: above every tail sum, j = n - 1: below the last one
            threshold = 2.0 * tails[0] if j < 0 else (0.5 * tails[j] if j == n - 1 else math.sqrt(tails[j] * tails[j + 1]))
            assert j < 0 or tails[j] > threshold * (1 + 1e-9) > tails[j + 1] * (1 + 1e-9) ** 2
            for cap in (-1, 0, n + 3, int(rng.integers(0, n + 1))):
                for abs_err, rel_err in ((threshold, 0.0), (0.0, threshold / total_of(s)), (threshold, 1e-3 * threshold / total_of(s))):
                    requests.append(f"rank {cap} {num(abs_err)} {num(rel_err)} " + vec(s))
                    keep = j + 1
                    want.append(min(keep, cap) if cap >= 0 else keep)
                    assert model_rank(s, cap, abs_err, rel_err) == want[-1]
    got = [int(line.split()[0]) for line in ask(requests)]
    assert got == want


def test_truncation_rule_edge_cases(ask):
    s = [4.0, 2.0, 1.0, 0.5]
    cases = [((-1, 0.0, 0.0), []), ((5, 1.0, 1e-3), []),                       # the empty spectrum
             ((-1, 0.0, 0.0), [0.0, 0.0, 0.0]), ((-1, 0.0, 1e-12), [0.0] * 5),  # all zeros: no tail exceeds 0
             ((-1, 0.0, 0.0), s), ((-1, 0.0, 0.0), s + [0.0, 0.0]),             # nothing allowed: everything above zero stays
             ((0, 0.0, 0.0), s), ((-1, -1.0, 0.0), s), ((-7, 0.0, 0.0), s),     # cap 0; a negative allowance is 0; no cap
             ((9, 0.0, 0.0), s), ((2, 0.0, 0.0), s), ((-1, 100.0, 0.0), s), ((-1, 0.0, 1.0), s)]
    want = [0, 0, 0, 0, 4, 4, 0, 4, 4, 4, 2, 0, 0]
    lines = ask([f"rank {cap} {num(a)} {num(r)} " + vec(v) for (cap, a, r), v in cases])
    assert [int(line.split()[0]) for line in lines] == want
    assert [model_rank(v, cap, a, r) for (cap, a, r), v in cases] == want
    assert [float.fromhex(line.split()[1]) for line in lines] == [model_allowed(v, a, r) for (cap, a, r), v in cases]
    fixed = ask([f"rankfor {cap} {num(allowed)} " + vec(s) for cap in (-1, 2) for allowed in (0.0, 0.75, 3.5, 7.5)])
    assert [int(x) for x in fixed] == [4, 3, 1, 0, 2, 2, 1, 0]


def test_truncation_rule_gives_the_bonds_of_the_reference(ask, golden):
    """Every ``tensor_svd`` case of the golden file on the exact branch: the rule on LAPACK's spectrum of the golden input
    gives the bond the reference kept.  No case sits within 1e-9 (relative) of its threshold, so none is left out."""
    g = golden["cv_mps"]
    cases = [c for c in json.loads(str(g["cases"])) if c.get("kind") == "tensor_svd"]
    requests, want = [], []
    for c in cases:
        t = g[f"svd_in_{c['index']}"]
        rows = int(np.prod([t.shape[i] for i in c["left"]]))
        matrix = np.moveaxis(t, c["left"] + c["right"], range(t.ndim)).reshape(rows, -1)
        cap = c["options"].get("max_bond_dim", -1)
        if 0 <= cap and cap * 10 < min(matrix.shape):
            continue                                   # the randomized branch
        abs_err, rel_err = c["options"].get("abs_err", 0.0), c["options"].get("rel_err", 1e-12)
        s = np.linalg.svd(matrix, compute_uv=False)
        allowed = model_allowed(s, abs_err, rel_err)
        assert allowed == 0.0 or np.min(np.abs(tails_of(s) - allowed)) > 1e-9 * allowed, c
        requests.append(f"rank {cap} {num(abs_err)} {num(rel_err)} " + vec(s))
        want.append(c["rank"])
    assert len(requests) == len(cases) == 4
    assert [int(line.split()[0]) for line in ask(requests)] == want


# ---- the verified low-rank route -------------------------------------------------------------------------------------
def test_low_rank_settled_agrees_with_the_rule_on_the_full_spectrum(ask):
    """``computed`` plays the l = 64 values of the projection; a true spectrum of length ``full`` is built from it with
    non-negative d_i, sum d_i = rho^2: sigma_i^2 = computed_i^2 + d_i (i < l), sigma_i^2 = d_i beyond.  Settled with rank
    r means the rule gives r on that spectrum; a wider bound on rho may unsettle a rank but never change it."""
    rng = np.random.default_rng(33)
    l, keep, n_cases = 64, 54, 360
    requests, truth, params = [], [], []
    for _ in range(n_cases):
        full = int(rng.integers(256, 2049))
        computed = np.exp(-rng.uniform(0.15, 1.2) * np.arange(l)) * 10.0 ** rng.uniform(-2, 2)
        rho = computed[0] * 10.0 ** rng.uniform(-13, -2)
        weights = rng.random(full) * (rng.random(full) < rng.uniform(0.02, 1.0))
        weights[int(rng.integers(0, full))] += 1.0                      # never all zero
        if rng.random() < 0.3:
            weights[:l] = 0.0                                          # all of the missed mass beyond the captured block
        d = rho * rho * weights / weights.sum()
        true = np.sqrt(np.concatenate([computed ** 2, np.zeros(full - l)]) + d)
        true = np.sort(true)[::-1]
        rho2 = float(np.sum(d)) * (1 + 1e-12)                          # the bound handed in is never below the mass
        rel_err = float(rng.choice([1e-2, 1e-4, 1e-6, 1e-9, 1e-12]))
        abs_err = float(rng.choice([0.0, 0.0, 1e-5 * computed[0]]))
        cap = int(rng.choice([-1, -1, 4, 25]))
        for widen in (1.0, 9.0, 400.0):
            requests.append(f"settled {num(rho2 * widen)} {full} {cap} {keep} {num(abs_err)} {num(rel_err)} " + vec(computed))
        truth.append(f"rank {cap} {num(abs_err)} {num(rel_err)} " + vec(true))
        params.append((computed, math.sqrt(rho2), full, cap, abs_err, rel_err))
    answers = [line.split() for line in ask(requests)]
    true_ranks = [int(line.split()[0]) for line in ask(truth)]
    settled = 0
    for i, (computed, rho, full, cap, abs_err, rel_err) in enumerate(params):
        narrow, wide, wider = answers[3 * i: 3 * i + 3]
        if narrow[0] == "1":
            settled += 1
            r = int(narrow[1])
            assert r == true_ranks[i], (i, r, true_ranks[i])
            assert r <= keep and (r == 0 or computed[r - 1] > 100.0 * rho)
        # the intermediate numbers the trace lines print: rho, margin, allowed
        assert [float.fromhex(x) for x in narrow[3:6]] == [rho, math.sqrt(float(full)) * rho, model_allowed(computed, abs_err, rel_err)]
        for a, b in ((narrow, wide), (wide, wider)):
            assert b[0] == "0" or (a[0] == "1" and a[1] == b[1]), (i, a, b)     # wider: the same rank, or undecided
    assert settled >= n_cases // 5 and n_cases - settled >= n_cases // 5, settled


# ---- the exact split: zgesdd guard, route, dust --------------------------------------------------------------------------
def gram_model(s, cap, abs_err, rel_err):
    if len(s) == 0:
        return False
    floor_value = 2e-8 * s[0]
    margin = floor_value * float(len(s))
    allowed = model_allowed(s, abs_err, rel_err)
    if not allowed > 100.0 * margin:
        return False
    r_lo, r_hi = model_rank_for(s, cap, allowed + margin), model_rank_for(s, cap, allowed - margin)
    return r_lo == r_hi and (r_lo == 0 or s[r_lo - 1] > 1e3 * floor_value)


def test_gram_values_decide_against_its_transcription(ask):
    rng = np.random.default_rng(34)
    todo = []
    for n in (0, 1, 2, 40, 300, 2048, 2049):
        for decay in (0.05, 0.5, 3.0):
            s = np.exp(-decay * np.arange(n)) + 1e-9 * rng.random(n)
            s = np.sort(s)[::-1]
            for rel_err in (1e-2, 1e-3, 1e-5, 1e-6, 1e-7, 1e-12, 0.0):
                for abs_err in (0.0, 5e-3, 1e-9):
                    for cap in (-1, 3, 40):
                        todo.append((s, cap, abs_err, rel_err))
    got = [x == "1" for x in ask([f"gram {cap} {num(a)} {num(r)} " + vec(s) for s, cap, a, r in todo])]
    want = [gram_model(*t) for t in todo]
    assert got == want
    assert 0.1 * len(todo) < sum(want) < 0.9 * len(todo)            # both outcomes


def test_exact_route_against_its_transcription(ask):
    shapes = [(1, 50), (50, 1), (2, 50), (50, 2), (2048, 2048), (2048, 32768), (2048, 32769), (32769, 2048), (2049, 3000),
              (3000, 2049), (8192, 8192), (8193, 8192), (700, 520)]
    todo = [(rows, cols, a, r, f2, svd) for rows, cols in shapes for a in (0.0, 1e-3, 1e-9) for r in (1e-7, 9.99e-7, 1e-6, 1e-5, 0.0)
            for f2 in (-1.0, 0.0, 1.0, 1e6, 1e-6) for svd in ("-", "exact", "library", "jacobi")]
    got = [tuple(int(x) for x in line.split()) for line in ask([f"route {rows} {cols} {num(a)} {num(r)} {num(f2)} {svd}" for rows, cols, a, r, f2, svd in todo])]
    want = []
    for rows, cols, a, r, f2, svd in todo:
        hopeless = False
        if f2 > 0.0:
            norm = math.sqrt(f2)
            hopeless = max(a, r * norm) < 1e-5 * norm
        loose = not hopeless and (r >= 1e-6 or a > 0.0)
        fits = svd not in ("exact", "library") and 2 <= min(rows, cols) <= 2048 and rows * cols <= 1 << 26
        want.append((int(hopeless), int(loose), int(fits)))
    assert got == want
    assert {(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1)} == set(want)     # every reachable combination


def test_dust_floor_and_relabelling_against_their_transcription(ask):
    rng = np.random.default_rng(35)
    sizes = [(L, f2) for L in (1, 7, 4096, 1 << 20) for f2 in (0.0, 1.0, 3.7e5, 2.2e-9)]
    floors = [float.fromhex(x) for x in ask([f"dust {L} {num(f2)}" for L, f2 in sizes])]
    assert floors == [16.0 * float(L) * 4.930380657631324e-32 * f2 for L, f2 in sizes]
    assert floors[6] == pytest.approx((4.0 * math.sqrt(4096.0) * EPS) ** 2 * 3.7e5, rel=1e-12)     # 4 sqrt(L) eps ||X||_F, squared
    todo = []
    for n in (1, 2, 9, 200):
        for dusty in (0, 1, n // 2, n):
            norm2 = np.sort(rng.random(n) + 0.1)[::-1]
            floor2 = 1e-24 * norm2[0]
            if dusty:
                norm2[n - dusty:] = floor2 * np.sort(rng.random(dusty) * 10.0 ** rng.uniform(-6, 0, dusty))[::-1]
            todo.append((floor2, norm2))
        todo.append((0.5, np.full(n, 0.5)))                           # exactly at the floor: not above it, so dust
    for (floor2, norm2), line in zip(todo, ask([f"relabel {num(f)} " + vec(v) for f, v in todo])):
        flag, values, after = line.split("|")
        sv, n2 = np.sqrt(norm2), norm2.copy()
        for c in range(len(sv)):
            if not n2[c] > floor2:
                sv[c] = min(sv[c], EPS * sv[0])
                n2[c] = sv[c] * sv[c]
        assert flag.strip() == str(int(np.any(~(norm2 > floor2))))
        assert np.array_equal(hostcheck.floats(values.split()), sv) and np.array_equal(hostcheck.floats(after.split()), n2)
        assert np.all(sv[~(norm2 > floor2)] <= EPS * math.sqrt(norm2[0])) and np.array_equal(sv[norm2 > floor2], np.sqrt(norm2[norm2 > floor2]))


# ---- the share plan of the skinny products ---------------------------------------------------------------------------
def share_model(out_rows, depth, l, share_amps):
    row_blocks = (out_rows + 63) // 64
    split, shares = (2 if row_blocks < 512 and depth >= 4 * 32 else 1), False
    if split > 1 and share_amps and row_blocks < 256:
        want = min((512 + row_blocks - 1) // row_blocks, 16, depth // (4 * 32))
        while want > 2 and want * out_rows * l > share_amps:
            want -= 1
        if want > 2 and want * out_rows * l <= share_amps:
            split, shares = want, True
    return split, shares


def test_skinny_share_plan_against_its_transcription(ask):
    rows = [1, 64, 100, 4000, 255 * 64, 255 * 64 + 1, 256 * 64, 256 * 64 + 1, 511 * 64, 511 * 64 + 1, 512 * 64 + 1, 100000]
    todo = []
    for out_rows in rows:
        for depth in (1, 127, 128, 129, 383, 384, 1000, 5000, 10 ** 6):
            for l in (1, 16, 33, 64):
                for share_amps in (0, 10, 3 * out_rows * l - 1, 3 * out_rows * l, 7 * out_rows * l + 5, 16 * out_rows * 64):
                    todo.append((out_rows, depth, l, share_amps))
    got = [(int(a), b == "1") for a, b in (line.split() for line in ask([f"shares {o} {d} {l} {s}" for o, d, l, s in todo]))]
    assert got == [share_model(*t) for t in todo]
    for (out_rows, depth, l, share_amps), (split, shares) in zip(todo, got):
        assert 1 <= split <= 16
        if shares:
            assert split > 2 and depth // split >= 4 * 32 and split * out_rows * l <= share_amps       # four slabs of 32 each
        else:
            assert split == (2 if (out_rows + 63) // 64 < 512 and depth >= 128 else 1)
    assert {s for s, _ in got} >= {1, 2, 3, 7, 16} and any(sh for _, sh in got)


# ---- the environment switches ----------------------------------------------------------------------------------------
def test_split_options_parse_every_documented_value(ask, exe, monkeypatch):
    default = (1, 1, 1, 256, 2, 0)
    table = [("- - - - -", default),
             ("exact - - - -", (0, 0, 1, 256, 2, 0)), ("library - - - -", (1, 0, 1, 256, 2, 0)), ("fast - - - -", default),
             ("- rocsolver - - -", (1, 1, 0, 256, 2, 0)), ("- fused - - -", default),
             ("- - 512 - -", (1, 1, 1, 512, 2, 0)), ("- - 1024 - -", (1, 1, 1, 1024, 2, 0)), ("- - 256 - -", default),
             ("- - 300 - -", default), ("- - many - -", default),
             ("- - - 3 -", (1, 1, 1, 256, 3, 0)), ("- - - 2 -", default), ("- - - 5 -", default), ("- - - x -", default),
             ("- - - - 1", (1, 1, 1, 256, 2, 1)), ("- - - - 0", (1, 1, 1, 256, 2, 1)),             # set at all: on
             ("library rocsolver 1024 3 yes", (1, 0, 0, 1024, 3, 1))]
    assert [tuple(int(x) for x in line.split()) for line in ask(["options " + t for t, _ in table])] == [w for _, w in table]
    # split_options() itself: read from the environment of the process, once
    names = ("QSV_SVD", "QSV_RSVD", "QSV_SVD_THREADS", "QSV_PANEL_ROUNDS", "QSV_TRACE_SPLIT")
    for name in names:
        monkeypatch.delenv(name, raising=False)
    assert hostcheck.ask(exe, ["env", "env"]) == ["1 1 1 256 2 0"] * 2
    for name, value in zip(names, ("exact", "rocsolver", "512", "3", "")):
        monkeypatch.setenv(name, value)
    assert hostcheck.ask(exe, ["env"]) == ["0 0 0 512 3 1"]
