"""The launch plan (csrc/rt_launch_plan.h) on a CPU.  Frames are bit-identical whatever the block, the unit size or the number of
passes, so no render test can see a shifted threshold; this one can.  tests/c/launch_plan_table.cpp is the planner behind a text
interface, built here with g++; tests/golden/launch_plans.json holds the decisions the library took on the device BEFORE the
planner existed (its header names the commit; NOTES.md says how it was recorded), and every row is compared on every field.
Besides the table: the invariants the kernels rely on, on synthetic inputs."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_BYTES = 163840
IN_ORDER = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill",
            "s_passes", "s_park", "count", "log", "n_rows", "max_w", "spp", "n", "cu_count", "per_cu")
FRAME, TRACE, HIT = 0, 1, 2


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "launch_plan_table.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in run(lines)]

    plans.check = lambda settings: run(["check " + " ".join(str(v) for v in s) for s in settings])
    return plans


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "launch_plans.json")) as f:
        return json.load(f)["rows"]


def test_every_recorded_decision_is_reproduced(planner, table):
    got = planner([r["in"] for r in table])
    wrong = [(r["name"], {k: (r["out"].get(k), g.get(k)) for k in set(r["out"]) | set(g) if r["out"].get(k) != g.get(k)})
             for r, g in zip(table, got) if r["out"] != g]
    assert not wrong, wrong[:5]


def test_the_table_reaches_every_branch(table):
    """The rows the plan's branches need (named in NOTES.md): a missing one would let a threshold move unseen."""
    rows = {r["name"]: r for r in table}
    out = lambda n: rows[n]["out"]  # noqa: E731
    assert [out(n)["F_chunk"] for n in ("c3_301_spp16", "c3_1201_spp16", "c3_2401_spp16", "c3_2401_spp4")] == [16, 32, 64, 64]
    assert out("c3_1201_spp16_chunk8")["F_chunk"] == 8 and out("c3_tune_probe")["F_mode"] == 3 and out("c3_tune_probe")["F_chunk"] == 4
    assert out("c3_whole_spp500")["two_pass"] == 1 and out("c3_2401_spp100")["two_pass"] == 1 and out("c3_1201_spp100")["two_pass"] == 0
    assert out("c3_2401_spp75")["two_pass"] == 1 and out("c3_2401_spp74")["two_pass"] == 0  # n2 >= 64 at 2 Mpx
    assert out("c3_1201_spp139")["two_pass"] == 1 and out("c3_1201_spp138")["two_pass"] == 0  # n2 >= 128
    assert out("c4_whole_spp1000")["two_pass"] == 0 and out("c3_whole_spp500_passes1")["two_pass"] == 0
    assert out("c3_301_spp40_passes2")["two_pass"] == 1 and out("c3_301_spp11_passes2")["two_pass"] == 0  # no second phase
    assert [(out(f"c3_shard_1_of_{w}_spp500")["A_chunk"], out(f"c3_shard_1_of_{w}_spp500")["B_chunk"]) for w in (8, 4, 2)] == [(16, 8), (32, 16), (32, 32)]
    assert out("c3_empty_stats")["F_grid"] == 0 and out("c3_empty_nostats")["F_grid"] == 0
    # the Lambert pool: 64 entries in LDS, fewer, left in global memory; pass A narrowed so that it fits
    assert (out("c3_1201_spp16_chunk8")["F_park_l"], out("c3_1201_spp16_chunk8")["F_park_l_lds"]) == (64, 1)
    assert (out("c3_1201_spp16")["F_park_l"], out("c3_1201_spp16")["F_park_l_lds"]) == (42, 1)
    assert (out("ms535_spp14_passes1")["F_park_l"], out("ms535_spp14_passes1")["F_park_l_lds"]) == (64, 0)
    assert out("ms580_spp14_passes2")["A_park_l"] == 32 and out("ms600_spp14_passes2")["A_chunk"] == 16
    assert out("c3_2401_spp100_park_off")["A_park"] == 0 and out("c3_2401_spp100_park_off")["A_park_l"] == 0
    # residency: resident, hybrid, counting variant without hybrid, 16384 objects and more
    assert out("c3_1201_spp16")["q_lds"] == 1 and out("ms1000_spp20")["F_lds_node_bytes"] > 0 and out("ms6400_spp20")["F_lds_node_bytes"] > 0
    assert out("ms1000_spp20_counted")["q_lds"] == 0 and out("ms1000_spp20_counted")["F_lds_node_bytes"] == 0
    assert rows["ms16500_spp20"]["in"]["n_obj"] >= 16384 and out("ms16500_spp20")["q_lds"] == 0
    assert {out(f"c3_1201_spp40_block{b}")["q_block"] for b in (256, 512, 768, 1024)} == {256, 512, 768, 1024}
    assert rows["ms1000_spp20_block256_counted_bpc1"]["in"]["per_cu"] > 1  # blocks_per_cu below the occupancy
    assert out("c5_1201_spp40")["q_tex"] == 1 and out("c3_1201_spp16")["q_tex"] == 0
    # ray lists
    for n in (1, 64, 65, 1000000):
        assert out(f"c3_hit_{n}")["F_mode"] == 5 and out(f"c5_trace_{n}")["F_mode"] == 4 and out(f"c5_trace_{n}")["q_tex"] == 1
    assert out("c5_hit_64")["q_tex"] == 0 and out("c3_hit_64")["F_grid"] == 1 and out("c3_hit_65")["waves"] == 16
    assert out("c3_hit_5000_block256")["q_block"] == 256 and out("c3_hit_5000_block512")["q_block"] == 1024


def _frame(**kw):
    i = dict(kind=FRAME, lds_total=136000, lds32_total=89000, n_nodes=969, n_obj=488, has_tex=0, n_rows=801, max_w=600, spp=100, cu_count=256, per_cu=1)
    i.update(kw)
    return i


def _jobs(**kw):
    """Every job kind over the same scene and settings: whole frames short and long, a forced two-pass frame, the tune probe, ray lists."""
    return [_frame(spp=16, **kw), _frame(spp=500, n_rows=1601, max_w=1200, **kw), _frame(spp=40, s_passes=2, **kw), _frame(spp=48, s_chunk=4, s_passes=1, log=1, **kw),
            _frame(kind=TRACE, n=5000, **kw), _frame(kind=HIT, n=5000, **kw)]


def _passes(plan):
    return [p for p in "FAB" if f"{p}_grid" in plan]


def test_leaf_wait_lies_between_the_yield_point_and_the_wave(planner):
    """yield <= leaf_wait <= 64 for every settable yield_lanes and every job kind: a hand-over point beyond the 64 lanes of a wave is
    one the node loop never reaches."""
    inputs = [j for y in range(0, 65) for j in _jobs(s_yield=y)]
    for i, plan in zip(inputs, planner(inputs)):
        assert _passes(plan)
        for p in _passes(plan):
            y = plan[f"{p}_yield"]
            assert y == (i["s_yield"] or 50) and y <= plan[f"{p}_leaf_wait"] <= 64 and plan[f"{p}_leaf_wait"] == min(64, y + 5), (i, plan)


def _check_invariants(i, plan):
    assert plan["error"] == 0 and plan["q_lds_bytes"] <= LDS_BYTES, (i, plan)
    per_cu = min(i["per_cu"], i.get("s_bpc") or i["per_cu"])
    for p in _passes(plan):
        assert plan[f"{p}_lds_bytes"] <= LDS_BYTES, (i, plan)
        assert plan[f"{p}_lds_node_bytes"] % 64 == 0 and plan[f"{p}_lds_node_bytes"] <= 64 * i["n_nodes"], (i, plan)
        cap, in_lds = plan[f"{p}_park_l"], plan[f"{p}_park_l_lds"]
        assert cap % 2 == 0 and (cap == 0 or 32 <= cap <= 64) and (in_lds == 0 or cap >= 32), (i, plan)
        assert (cap == 0) == (plan[f"{p}_park"] == 0) and (in_lds or cap in (0, 64)), (i, plan)
        assert plan[f"{p}_grid"] <= i["cu_count"] * per_cu, (i, plan)
        assert plan[f"{p}_chunk"] >= 1 and plan[f"{p}_chunk"] <= 64, (i, plan)


def test_invariants_hold_for_every_recorded_row(planner, table):
    for r, plan in zip(table, planner([r["in"] for r in table])):
        _check_invariants(r["in"], plan)


def test_invariants_hold_around_the_residency_edge(planner):
    """Scene sizes swept across the point where the image stops fitting the LDS, for every block, with and without parking, counted and
    timed: no pass asks for more than the 160 KiB, the hybrid bytes are whole records, the Lambert pool is even and 0 or 32..64."""
    inputs = []
    for lds32 in list(range(60000, 170000, 1872)) + [163840 - 18432, 163840 - 18432 + 16, 163840, 163856]:
        for block in (0, 256, 512, 768, 1024):
            for park in (0, -1, 7):
                for count in (0, 1):
                    sc = dict(lds32_total=lds32, lds_total=lds32 * 3 // 2, n_nodes=lds32 // 92, n_obj=lds32 // 184, s_block=block, s_park=park, count=count)
                    inputs += _jobs(**sc) + [_frame(spp=14, n_rows=961, max_w=853, s_passes=2, per_cu=2, s_bpc=1, **sc)]
    plans = planner(inputs)
    for i, plan in zip(inputs, plans):
        _check_invariants(i, plan)
    assert {p["q_lds"] for p in plans} == {0, 1} and any(p.get("F_lds_node_bytes") for p in plans) and any(p["two_pass"] for p in plans)


def test_check_settings_guards_each_range_with_its_message(planner):
    ok = [(0, 0, 0, 0, 0, 0, 0), (256, 0, 0, 0, 0, 0, 0), (512, 64, 8, 64, 64, 2, 256), (768, 0, 0, 0, 0, 0, -1), (1024, 1, 1, 1, 1, 1, 1)]
    assert planner.check(ok) == ["ok"] * len(ok)
    bad = {
        "block_threads must be 0, 256, 512, 768 or 1024": [(128, 0, 0, 0, 0, 0, 0), (1025, 0, 0, 0, 0, 0, 0), (-256, 0, 0, 0, 0, 0, 0)],
        "chunk_pixels must be in [0, 64]": [(0, -1, 0, 0, 0, 0, 0), (0, 65, 0, 0, 0, 0, 0)],
        "blocks_per_cu must be in [0, 8]": [(0, 0, -1, 0, 0, 0, 0), (0, 0, 9, 0, 0, 0, 0)],
        "thresholds must be in [0, 64]": [(0, 0, 0, -1, 0, 0, 0), (0, 0, 0, 65, 0, 0, 0), (0, 0, 0, 0, -1, 0, 0), (0, 0, 0, 0, 65, 0, 0)],
        "passes must be 0 (auto), 1 (fused) or 2 (two-pass)": [(0, 0, 0, 0, 0, -1, 0), (0, 0, 0, 0, 0, 3, 0)],
        "park_lanes must be in [-1, 256]": [(0, 0, 0, 0, 0, 0, -2), (0, 0, 0, 0, 0, 0, 257)],
    }
    for message, settings in bad.items():
        assert planner.check(settings) == [message] * len(settings)
