"""The launch plan of an extension by map (rt_render_extend_map, Job::map; csrc/rt_launch_plan.h) on a CPU: it is the extension
12 -> cap with pass B's per-pixel variant -- mode 9 (frame) or 10 (footprints) and that variant's larger per-wave scratch -- so two
passes, no pass A, pass B within the LDS with at least one pixel per unit; and with the flag off every job is planned word for word
as tests/golden/launch_plans.json records it.  tests/c/extend_map_plan_table.cpp is the planner behind launch_plan_table.cpp's text
interface with the two inputs added."""
import json
import os
import subprocess

import pytest

from test_launch_plan import IN_ORDER, LDS_BYTES

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME, FOOTPRINTS = 0, 3
MIN_DONE = 12
PASS_KEYS = ("mode", "grid", "lds_bytes", "chunk", "park", "park_l", "park_l_lds", "lds_node_bytes", "lds_node_thr", "yield", "leaf_wait",
             "refill", "k", "total_waves")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_extend_map") / "extend_map_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "extend_map_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER + ("first_sample", "map")) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "launch_plans.json")) as f:
        return json.load(f)["rows"]


def _jobs(table):
    """Every frame job of the recorded table whose spp can be a map's cap (>= 12; no tune probe), and each again as a footprint list."""
    frames = [dict(r["in"]) for r in table if r["in"]["kind"] == FRAME and r["in"]["spp"] >= MIN_DONE and not r["in"].get("log")]
    lists = [dict(i, kind=FOOTPRINTS, n=i["n_rows"] * (2 * i["max_w"] + 1), n_rows=0, max_w=0) for i in frames]
    return frames + [i for i in lists if i["n"] <= 2**31 - 1]


def test_the_flag_off_reproduces_every_recorded_decision(planner, table):
    got = planner([dict(r["in"], first_sample=0, map=0) for r in table])
    wrong = [(r["name"], {k: (r["out"].get(k), g.get(k)) for k in set(r["out"]) | set(g) if r["out"].get(k) != g.get(k)})
             for r, g in zip(table, got) if r["out"] != g]
    assert not wrong, wrong[:5]


def test_a_map_is_the_extension_from_12_with_its_own_pass_b(planner, table):
    jobs = _jobs(table)
    assert len(jobs) > 200 and {j["kind"] for j in jobs} == {FRAME, FOOTPRINTS}
    maps = planner([dict(j, first_sample=MIN_DONE, map=1) for j in jobs])
    exts = planner([dict(j, first_sample=MIN_DONE, map=0) for j in jobs])
    seen = {"lds": set(), "b_chunk": set(), "narrowed": 0, "empty": 0, "cap12": 0}
    for j, m, e in zip(jobs, maps, exts):
        pixels = j["n"] if j["kind"] == FOOTPRINTS else j["n_rows"] * (2 * j["max_w"] + 1)
        for k in ("q_lds", "q_count", "q_block", "q_mode", "q_tex", "q_lds_bytes", "pool", "waves"):
            assert m[k] == e[k], (j, k)
        if pixels == 0:  # an empty shard: nothing is launched (the entry points return before planning)
            assert m["two_pass"] == 0 and m["F_grid"] == 0 and m["error"] == 0, j
            seen["empty"] += 1
            continue
        # two passes, no pass A, nothing sorted -- also when the cap is 12 and no pixel can be continued (the classes are still checked)
        assert m["two_pass"] == 1 and m["error"] == 0 and m["pairs"] == 0 and m["sort"] == 0 and m["list"] == (pixels * 4 + 15) // 16 * 16, j
        seen["cap12"] += j["spp"] == MIN_DONE
        for k in PASS_KEYS:
            assert m[f"A_{k}"] == 0, (j, k)
        waves = m["q_block"] // 64
        assert m["B_mode"] == (10 if j["kind"] == FOOTPRINTS else 9) and m["B_grid"] > 0
        assert 1 <= m["B_chunk"] <= 64 and m["B_lds_bytes"] <= LDS_BYTES
        # the variant's scratch is what was placed: 22 words a pixel, a wave, beside the resident scene
        scene = (j["lds_total"] if j.get("count") else j["lds32_total"]) if m["q_lds"] else 0
        assert m["B_lds_bytes"] >= scene + waves * 22 * m["B_chunk"] * 4, j
        if j["spp"] > MIN_DONE:  # the extension's own pass B: the same but for what follows from the scratch
            assert e["two_pass"] == 1 and e["error"] == 0
            assert m["B_chunk"] <= e["B_chunk"] and (m["B_chunk"] == e["B_chunk"] or scene + waves * 22 * e["B_chunk"] * 4 > LDS_BYTES), j
            seen["narrowed"] += m["B_chunk"] < e["B_chunk"]
            for k in ("grid", "park", "yield", "leaf_wait", "refill", "k", "total_waves"):
                assert m[f"B_{k}"] == e[f"B_{k}"], (j, k)
        seen["lds"].add(m["q_lds"]); seen["b_chunk"].add(m["B_chunk"])
    assert seen["lds"] == {0, 1} and len(seen["b_chunk"]) >= 3, seen
    print(seen)


def test_the_plan_halves_pass_b_units_until_the_map_scratch_fits(planner):
    """A resident scene beside which pass B's 18 words a pixel fit at 64-pixel units and the map's 22 do not: the map runs at 32."""
    scene = LDS_BYTES - 16 * 20 * 64 * 4  # room for 20 words a pixel at 1024 threads and 64 pixels
    job = dict(kind=FRAME, lds_total=scene, lds32_total=scene, n_nodes=100, n_obj=50, n_rows=101, max_w=50, spp=40, cu_count=256, per_cu=1, s_chunk=64)
    ext, m = planner([dict(job, first_sample=MIN_DONE, map=0), dict(job, first_sample=MIN_DONE, map=1)])
    assert ext["q_lds"] == 1 and ext["error"] == 0 and ext["B_chunk"] == 64 and ext["B_mode"] == 2
    assert m["q_lds"] == 1 and m["error"] == 0 and m["B_chunk"] == 32 and m["B_mode"] == 9 and m["B_lds_bytes"] <= LDS_BYTES
    for passes in (1, 2):  # `passes` is accepted and ignored
        assert planner([dict(job, first_sample=MIN_DONE, map=1, s_passes=passes)])[0] == m
    # a cap of 12 continues no pixel, and is still planned: the list builder classifies every pixel, rgb is written
    low = planner([dict(job, spp=MIN_DONE, first_sample=MIN_DONE, map=1)])[0]
    assert low["two_pass"] == 1 and low["error"] == 0 and low["B_mode"] == 9 and low["B_grid"] > 0
