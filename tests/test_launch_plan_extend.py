"""The launch plan of an extension (rt_render_extend, Job::first_sample != 0; csrc/rt_launch_plan.h) on a CPU: it is the plan of
the same job at the target sample count with two passes forced, less pass A and the ordering -- pass B's every field, the pools,
the waves and the list are those of `passes = 2`; pass A's grid, the pairs and the sort workspace are 0 -- and a job with
first_sample = 0 is planned word for word as tests/golden/launch_plans.json records it.  tests/c/extend_plan_table.cpp is the
planner behind launch_plan_table.cpp's text interface with the one input added."""
import json
import os
import subprocess

import pytest

from test_launch_plan import IN_ORDER, LDS_BYTES

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME, FOOTPRINTS = 0, 3
PASS_KEYS = ("mode", "grid", "lds_bytes", "chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "lds_node_thr", "yield", "leaf_wait",
             "refill", "k", "total_waves")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_extend") / "extend_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "extend_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER + ("first_sample",)) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "launch_plans.json")) as f:
        return json.load(f)["rows"]


def _jobs(table):
    """The table's frame jobs a buffer of 12 samples can be extended to (spp >= 12, no tune probe), and each of them again as a
    footprint list of as many pixels."""
    frames = [dict(r["in"]) for r in table if r["in"]["kind"] == FRAME and r["in"]["spp"] >= 12 and not r["in"].get("log")]
    lists = [dict(i, kind=FOOTPRINTS, n=i["n_rows"] * (2 * i["max_w"] + 1), n_rows=0, max_w=0) for i in frames]
    return frames + [i for i in lists if i["n"] <= 2**31 - 1]


def test_first_sample_zero_reproduces_every_recorded_decision(planner, table):
    got = planner([dict(r["in"], first_sample=0) for r in table])
    wrong = [(r["name"], {k: (r["out"].get(k), g.get(k)) for k in set(r["out"]) | set(g) if r["out"].get(k) != g.get(k)})
             for r, g in zip(table, got) if r["out"] != g]
    assert not wrong, wrong[:5]


def test_an_extension_is_the_two_pass_plan_less_pass_a_and_the_ordering(planner, table):
    jobs = _jobs(table)
    assert len(jobs) > 200 and {j["kind"] for j in jobs} == {FRAME, FOOTPRINTS}
    for done in (12, 13):
        todo = [j for j in jobs if j["spp"] > done]  # (target == done returns before planning)
        ext = planner([dict(j, first_sample=done) for j in todo])
        two = planner([dict(j, s_passes=2) for j in todo])
        seen = {"lds": set(), "b_chunk": set(), "misfit": 0, "empty": 0}
        for j, e, t in zip(todo, ext, two):
            pixels = j["n"] if j["kind"] == FOOTPRINTS else j["n_rows"] * (2 * j["max_w"] + 1)
            for k in ("q_lds", "q_count", "q_block", "q_mode", "q_tex", "q_lds_bytes", "pool", "waves"):
                assert e[k] == t[k], (j, k)
            if pixels == 0:  # an empty shard: nothing is launched either way (the entry points return before planning)
                assert e["two_pass"] == 0 and e["F_grid"] == 0 and e["error"] == 0, j
                seen["empty"] += 1
                continue
            assert t["two_pass"] == 1 and e["two_pass"] == 1, j
            assert e["pairs"] == 0 and e["sort"] == 0 and e["list"] == t["list"] == (pixels * 4 + 15) // 16 * 16, j
            if t["error"]:  # the LDS misfit path stays: it is pass B's misfit too, or the extension fits where pass A did not
                seen["misfit"] += 1
                continue
            assert e["error"] == 0, j
            for k in PASS_KEYS:
                assert e[f"B_{k}"] == t[f"B_{k}"], (j, k)
                assert e[f"A_{k}"] == 0, (j, k)  # no pass A: every word the library reports for it is 0
            assert e["B_mode"] == (8 if j["kind"] == FOOTPRINTS else 2) and e["B_grid"] > 0 and e["B_lds_bytes"] <= LDS_BYTES
            seen["lds"].add(e["q_lds"]); seen["b_chunk"].add(e["B_chunk"])
        assert seen["lds"] == {0, 1} and len(seen["b_chunk"]) >= 3, seen


def test_an_extension_never_widens_units_for_few_samples(planner):
    """A frame of 16 samples per pixel is planned with 64-pixel units (fused); its extension 12 -> 16 is pass B with pass B's."""
    job = dict(kind=FRAME, lds_total=135808, lds32_total=89296, n_nodes=969, n_obj=487, n_rows=1601, max_w=1200, spp=16, cu_count=256, per_cu=1)
    fresh, ext, two = planner([job, dict(job, first_sample=12), dict(job, s_passes=2)])
    assert fresh["two_pass"] == 0 and fresh["F_chunk"] == 64
    assert ext["two_pass"] == 1 and ext["q_lds_bytes"] == two["q_lds_bytes"] and ext["B_chunk"] == two["B_chunk"] and ext["A_grid"] == 0
    for passes in (1, 2):  # `passes` is accepted and ignored
        assert planner([dict(job, first_sample=12, s_passes=passes)])[0] == ext

