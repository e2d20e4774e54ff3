"""The pass planner of ``qsv_apply_layer`` (``csrc/qsv_layer_plan.h``) on the CPU, under AddressSanitizer + UBSan.

``tests/layout/layer_plan_driver.cpp`` is a stand-alone program (text in, text out; nothing is loaded into Python).  For
members of 1 to 30 bits, as 2^0 to 2^12 members with at most 30 bits in all, and the layer sets all bits / bits 0..5 / the top
bit / every single bit / 50 seeded random subsets, listed in a shuffled order, the printed records are checked against the
rules restated here.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import hostcheck
import layer_reference as L

HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return hostcheck.compile_driver(HERE / "layout" / "layer_plan_driver.cpp", tmp_path_factory.mktemp("layer_plan"))


def layer_sets(n: int) -> list[list[int]]:
    rng = np.random.default_rng(1000 + n)
    sets = [list(range(n)), list(range(min(n, 6))), [n - 1]] + [[b] for b in range(n)]
    for _ in range(50):
        sets.append([int(b) for b in rng.permutation(n)[:int(rng.integers(1, n + 1))]])
    return [[int(b) for b in rng.permutation(s)] for s in sets]           # the listing order must not matter


def parse(line: str, k: int) -> dict:
    t = [int(x) for x in line.split()]
    out = {"passes": t[0], "formula": t[1], "table_doubles": t[2], "order": t[3:3 + k], "plan": []}
    i = 3 + k
    for _ in range(out["passes"]):
        tile_bits, n_stages, first = t[i:i + 3]
        i += 3
        p = {"tile_bits": tile_bits, "n_stages": n_stages, "first": first, "pos": t[i:i + tile_bits], "stages": [], "runs": []}
        i += tile_bits
        for _ in range(n_stages):
            p["stages"].append(dict(zip(("bit", "tile_index", "run", "reg", "offset_first", "offset_last"), t[i:i + 6])))
            i += 6
        n_runs = t[i]
        i += 1
        width = min(4, tile_bits)
        for _ in range(n_runs):
            p["runs"].append({"first": t[i], "count": t[i + 1], "q": t[i + 2:i + 2 + width]})
            i += 2 + width
        p["pairs_ok"] = t[i]
        i += 1
        out["plan"].append(p)
    assert i == len(t)
    return out


def formula(n: int, bits: list[int]) -> int:
    if not bits:
        return 0
    return 1 if n <= 12 else max(1, -(-sum(1 for b in bits if b >= 6) // 6))


def check(n: int, b: int, bits: list[int], answer: dict) -> None:
    k = len(bits)
    assert answer["passes"] == answer["formula"] == formula(n, bits) == L.pass_count(n, [n - 1 - x for x in bits])
    assert answer["table_doubles"] == (8 * k) << b
    assert sorted(answer["order"]) == list(range(k))
    walked = []
    for p in answer["plan"]:
        pos = p["pos"]
        assert p["tile_bits"] == min(n, 12) == len(pos) == len(set(pos)) and pos == sorted(pos) and max(pos) < n
        assert pos[:min(n, 6)] == list(range(min(n, 6)))
        assert p["first"] == len(walked) and p["pairs_ok"] == 1
        stage_bits = [s["bit"] for s in p["stages"]]
        if n > 12:
            assert sum(1 for x in stage_bits if x >= 6) <= 6
        covered = [i for run in p["runs"] for i in range(run["first"], run["first"] + run["count"])]
        assert covered == list(range(p["n_stages"]))                      # every stage in exactly one run
        for run in p["runs"]:
            assert 1 <= run["count"] <= 4 and run["q"] == sorted(set(run["q"])) and max(run["q"]) < p["tile_bits"]
        for number, s in enumerate(p["stages"]):
            assert pos[s["tile_index"]] == s["bit"]                       # the stage bit lies in the tile
            run = p["runs"][s["run"]]
            assert run["first"] <= number < run["first"] + run["count"] and run["q"][s["reg"]] == s["tile_index"]
            place = len(walked) + number
            assert s["offset_first"] == 8 * place and s["offset_last"] == 8 * ((((1 << b) - 1) * k) + place)
            assert s["offset_last"] + 8 <= answer["table_doubles"]        # inside the table
        walked += stage_bits
    assert walked == sorted(bits)                                         # every stage once, ascending over the whole plan
    assert [bits[j] for j in answer["order"]] == walked


def test_plans_follow_the_rules(driver):
    cases = [(n, b, bits) for n in range(1, 31) for bits in layer_sets(n) for b in range(0, 13) if n + b <= 30]
    answers = hostcheck.ask(driver, [f"{n} {b} {len(bits)} " + " ".join(map(str, bits)) for n, b, bits in cases])
    alone = {}
    for (n, b, bits), line in zip(cases, answers):
        answer = parse(line, len(bits))
        check(n, b, bits, answer)
        key = (n, tuple(bits))
        if b == 0:
            alone[key] = answer
        else:                                                             # the plan does not depend on the number of members
            strip = lambda a: [{**p, "stages": [{**s, "offset_last": 0} for s in p["stages"]]} for p in a["plan"]]
            assert strip(answer) == strip(alone[key]) and answer["order"] == alone[key]["order"]


def test_pass_counts_of_the_documented_shapes(driver):
    sizes = {28: 4, 13: 2, 18: 2, 19: 3, 16: 2, 20: 3, 12: 1, 7: 1}
    answers = hostcheck.ask(driver, [f"{n} 0 {n} " + " ".join(map(str, range(n))) for n in sizes] + ["9 3 0"])
    assert [int(line.split()[0]) for line in answers] == list(sizes.values()) + [0]
    # 13 bits: the second pass holds the one stage left, its run completed with the highest tile bits
    second = parse(answers[1], 13)["plan"][1]
    assert [s["bit"] for s in second["stages"]] == [12] and second["runs"] == [{"first": 0, "count": 1, "q": [8, 9, 10, 11]}]
