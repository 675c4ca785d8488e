"""csrc/rt_tree_plan.h alone (tests/c/tree_plan_table.cpp): the shape of BoundingBoxTree.make's tree as a function of n -- segments, node
indices, skip links, depth -- against the plain recursion for every n in 1..4100 and for 1e5, 1e6 and 4,500,000; the order-preserving key;
the two merge rules; the first-minimum rule.  Built plainly, and once as a stand-alone program under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tree_plan_against_the_recursion(tmp_path, sanitize):
    exe = str(tmp_path / "tree_plan_table")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "tree_plan_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["shape 1..4100 ok", "shape large ok", "keys ok"]
