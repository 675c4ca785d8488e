"""csrc/rt_walk_plan.h alone (tests/c/walk_plan_table.cpp): the order-preserving key with its canonical zero and its inverse, the bin index at
its edges, the pre-order positions against a plain recursion, the level bound, the costs' association, half_area's clamp and the binned
choice's first minimum.  Built plainly, and once as a stand-alone program under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_walk_plan_table(tmp_path, sanitize):
    exe = str(tmp_path / "walk_plan_table")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "walk_plan_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["keys ok", "bins ok", "positions ok", "costs ok"]
