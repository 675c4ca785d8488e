"""The table of render_kernel's modes (csrc/rt_modes.h) on a CPU, against the expressions it replaced.  Until the table existed a mode's
meaning was arithmetic on its number in three files; those expressions are written out here as they stood -- the kernel's MAP / PX /
CAM / FP / PM lines and its four-way scratch ternary (rt_render_kernel.h), the factors 18 / 13 / 22 / 6 / 0 of rt_launch_consts.h, the
planner's fp + 1 and fp ? 10 : 9 (rt_launch_plan.h), kernel_if_built's condition (rtfs_amd.hip) -- and are the oracle: nothing below
reads the new header but the program tests/c/modes_table.cpp, which prints it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME, FOOTPRINTS, LIST, NONE = range(4)                 # rtmode::Pixels
FUSED, PASS_A, PASS_B, RAY_LIST, CAMERA_HITS = range(5)  # rtmode::Pass
BLOCKS = (256, 512, 768, 1024)


def old(MODE):
    """What the parent's device and host code derived from the number."""
    MAP = MODE == 9 or MODE == 10
    PX = MODE >= 11 and MODE <= 13
    CAM = MODE == 14
    FP = MODE >= 6 and MODE != 9 and not PX and not CAM
    PM = 2 if MAP else MODE - 11 if PX else MODE - 6 if FP else MODE
    RAYS = MODE == 4 or MODE == 5

    def words(P):
        return 0 if RAYS else 6 * P if CAM else 13 * P if PM == 1 else 22 * P if MAP else 18 * P

    def built(BLOCK, TEX):
        return not ((MODE >= 4 and MODE != 9 and BLOCK != 256 and BLOCK != 1024) or ((MODE == 5 or MODE == 14) and TEX))

    return dict(
        mode=MODE,
        pixels=NONE if RAYS else FOOTPRINTS if FP else LIST if PX or CAM else FRAME,
        **{"pass": RAY_LIST if RAYS else CAMERA_HITS if CAM else {0: FUSED, 1: PASS_A, 2: PASS_B, 3: FUSED}[PM]},
        map=int(MAP), log=int(not RAYS and not CAM and PM == 3), hits=int(MODE == 5 or CAM),  # (run_rays<.., MODE == 5>; camera hits answer as mode 5)
        words1=words(1), words16=words(16), words64=words(64),
        built="".join(str(int(built(b, t))) for b in BLOCKS for t in (False, True)))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modes") / "modes_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "modes_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    head = dict(kv.split("=") for kv in out[0].split())
    rows = [{k: (v if k == "built" else int(v)) for k, v in (kv.split("=") for kv in line.split())} for line in out[1:]]
    return head, rows


def test_the_table_is_what_the_numbers_meant(table):
    head, rows = table
    assert head["count"] == "15" and len(rows) == 15
    for m, row in enumerate(rows):
        want = old(m)
        assert {k: row[k] for k in want} == want, m
        # the two rules "is built" is made of, each against the parent's condition
        assert row["every_block"] == int(not (m >= 4 and m != 9)) and row["textured"] == int(not (m == 5 or m == 14)), m
    assert sum(r["built"].count("1") for r in rows) * 4 == 304  # x (lds, count): the render_kernel symbols of the library's listing


def test_the_round_trip_and_the_planner_s_arithmetic(table):
    head, rows = table
    assert [r["inverse"] for r in rows] == list(range(15))  # no two modes share a description
    assert head["outside"] == "-1,-1"                        # ... and a number outside the table is none
    number = {(r["pixels"], r["pass"], r["map"], r["log"], r["hits"]): r["mode"] for r in rows}
    assert len(number) == 15
    # rt_launch_plan.h built the number from the other direction: fp = 0 / 6 / 11 for a frame / a footprint list / a pixel list
    for pixels, fp in ((FRAME, 0), (FOOTPRINTS, 6), (LIST, 11)):
        assert number[(pixels, FUSED, 0, 0, 0)] == fp       # q.mode = 0, or 6, or 11
        assert number[(pixels, PASS_A, 0, 0, 0)] == fp + 1  # pl.a.mode = fp + 1
        assert number[(pixels, PASS_B, 0, 0, 0)] == fp + 2  # pl.b.mode = fp + 2
    assert number[(FRAME, FUSED, 0, 1, 0)] == 3              # job.ray_log ? 3 : 0
    assert number[(FRAME, PASS_B, 1, 0, 0)] == 9 and number[(FOOTPRINTS, PASS_B, 1, 0, 0)] == 10  # job.map ? (fp ? 10 : 9)
    # (no entry point extends a pixel list by map and the table has no such mode; the planner still answers 10 for it, as `fp ? 10 : 9` did)
    assert (LIST, PASS_B, 1, 0, 0) not in number
    assert number[(NONE, RAY_LIST, 0, 0, 0)] == 4 and number[(NONE, RAY_LIST, 0, 0, 1)] == 5 and number[(LIST, CAMERA_HITS, 0, 0, 1)] == 14
