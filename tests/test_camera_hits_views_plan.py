"""Camera hits over a batch of views (rt_camera_hits_views) on a CPU: the work units (tests/c/camera_hits_views_units_table.cpp over
csrc/rt_views_plan.h -- a stand-alone program, built plainly and once with -fsanitize=address,undefined) and the launch plan of the new
job kind (tests/c/camera_hits_views_plan_table.cpp over csrc/rt_launch_plan.h) for the scene sizes of the recorded table: the unit
count, the grid, the LDS bytes, the default chunk with its halving, one view planned exactly as the camera-hit job of the same list, and
every recorded row of the other kinds reproduced word for word."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_BYTES = 163840
IN_ORDER = ("kind", "lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex", "s_block", "s_chunk", "s_bpc", "s_yield", "s_refill",
            "s_passes", "s_park", "count", "log", "n_rows", "max_w", "spp", "n", "cu_count", "per_cu", "first_sample", "n_views")
CAMERA_HITS, CAMERA_HITS_VIEWS = 5, 7
SCENE_KEYS = ("lds_total", "lds32_total", "n_nodes", "n_obj", "has_tex")


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan-ubsan"])
def test_units_cover_every_view_entry_once_and_slots_partition_the_outputs(tmp_path, flags):
    exe = str(tmp_path / "camera_hits_views_units_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", *flags, "-o", exe, os.path.join(HERE, "c", "camera_hits_views_units_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "camera hits views units: ok (224 cases)" in out.stdout and not out.stderr  # 6 * 4 * 4 * 2 tables and 4 * 4 * 2 bounds


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_camera_hits_views") / "camera_hits_views_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "camera_hits_views_plan_table.cpp")])

    def plans(inputs):
        lines = ["plan " + " ".join(str(int(i.get(k, 0))) for k in IN_ORDER) for i in inputs]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return plans


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "launch_plans.json")) as f:
        return json.load(f)["rows"]


def test_the_other_kinds_are_planned_as_recorded(planner, table):
    """With the new kind unused the probe reproduces tests/golden/launch_plans.json word for word (as launch_plan_table.cpp does)."""
    got = planner([dict(r["in"], first_sample=0, n_views=0) for r in table])
    assert len(table) > 100 and all(r["out"] == g for r, g in zip(table, got))


def _scene_sizes(table):
    """The different scenes of the recorded table (plain ones: nothing is shaded, so a textured scene plans the same)."""
    seen = {}
    for r in table:
        seen.setdefault(tuple(r["in"][k] for k in SCENE_KEYS), None)
    return [dict(zip(SCENE_KEYS, s)) for s in seen]


def _ceil(a, b):
    return -(-a // b)


def test_camera_hits_views_plan(planner, table):
    scenes_ = _scene_sizes(table)
    assert len(scenes_) >= 5
    inputs, singles = [], []
    for sc in scenes_:
        for count in (0, 1):
            for per in (1, 7, 12, 500):
                for block in (0, 256, 512, 768, 1024):
                    for chunk in (0, 1, 10, 64):
                        for n, k in ((9, 70), (5, 70), (63, 5), (2911, 64), (1, 1), (65, 1), (1201 * 801, 1), (9, 4097), (1001, 3)):
                            if k * n * per > 2**31 - 1:
                                continue
                            base = dict(sc, count=count, s_block=block, s_chunk=chunk, cu_count=256, per_cu=2, n=n, spp=per, first_sample=3)
                            inputs.append(dict(base, kind=CAMERA_HITS_VIEWS, n_views=k))
                            singles.append(dict(base, kind=CAMERA_HITS))
    plans, ones = planner(inputs), planner(singles)
    seen = {"lds": set(), "chunk": set(), "grid": set(), "halved": 0}
    for i, p, one in zip(inputs, plans, ones):
        n, k, per, chunk = i["n"], i["n_views"], i["spp"], i["s_chunk"]
        assert p["two_pass"] == 0 and p["error"] == 0 and p["q_mode"] == p["F_mode"] == 14 and p["q_tex"] == 0 and p["views"] == 1, i
        assert p["q_block"] == (256 if i["s_block"] == 256 else 1024) and p["q_count"] == i["count"], i
        assert p["units"] == k * _ceil(n, p["F_chunk"]), i                                        # n_views * ceil(n / chunk): none spans two views
        full = i["cu_count"] * i["per_cu"]
        waves = p["q_block"] // 64
        assert 1 <= p["F_grid"] <= full and p["F_grid"] == min(full, _ceil(_ceil(k * n * per, 64), waves)), i  # the camera-hit rule over n_views * n * n_samples rays
        assert p["waves"] == p["F_grid"] * waves, i
        assert p["F_lds_bytes"] <= LDS_BYTES and p["q_lds_bytes"] == p["F_lds_bytes"], i
        image = 0 if not p["q_lds"] else (i["lds_total"] if i["count"] else i["lds32_total"])
        assert p["F_lds_bytes"] == image + waves * 6 * p["F_chunk"] * 4 + p["F_lds_node_bytes"], i
        assert p["F_park"] == p["F_park_l"] == p["F_park_l_lds"] == p["pool"] == 0, i
        # the chunk: the caller's, or ceil(64 / n_samples), halved while an LDS-resident scene leaves the waves' scratch no room
        if chunk:
            assert p["F_chunk"] == chunk, i
        else:
            want = 1 if per >= 64 else _ceil(64, per)
            while p["q_lds"] and want > 1 and image + waves * 6 * want * 4 > LDS_BYTES:
                want //= 2
                seen["halved"] += 1
            assert p["F_chunk"] == want, i
        # residency, the thresholds, the chunk and the LDS: the camera-hit job's of the same list -- the view count moves the grid alone
        for key in p:
            if key not in ("units", "views", "F_grid", "waves"):
                assert p[key] == one[key], (key, i)
        if k == 1:  # one view IS the kind-5 plan, in every word but the kind
            assert {key: v for key, v in p.items() if key not in ("units", "views")} == one, i
        seen["lds"].add(p["q_lds"]); seen["chunk"].add(p["F_chunk"]); seen["grid"].add(p["F_grid"])
    assert seen["lds"] == {0, 1} and len(seen["chunk"]) >= 6 and len(seen["grid"]) >= 6 and seen["halved"] > 0
    # 64 views of 71 x 41 at one sample: 186,304 rays are 2,911 waves' worth, 728 blocks of 256 threads -- the full grid of 512 takes them
    p = planner([dict(scenes_[0], kind=CAMERA_HITS_VIEWS, n=2911, n_views=64, spp=1, s_block=256, cu_count=256, per_cu=2)])[0]
    assert p["F_grid"] == 512 and p["units"] == 64 * 46 and p["F_chunk"] == 64
