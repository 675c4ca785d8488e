"""csrc/rt_scene_plan.h alone (tests/c/scene_plan_table.cpp): the check of a hittable and its order, Sphere.make's box, outward rounding at
zero, the subnormals and the ends of the float range (and against nextafterf), the section offsets, the node / node32 / geo / meta / mat
records and the box_implied predicate at its bounds -- hand-checked values.  Built plainly, and once as a stand-alone program under
-fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scene_plan_table(tmp_path, sanitize):
    exe = str(tmp_path / "scene_plan_table")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "scene_plan_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["checks ok", "boxes ok", "rounding ok", "offsets ok", "nodes ok", "objects ok", "implied ok"]
