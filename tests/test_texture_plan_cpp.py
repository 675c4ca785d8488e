"""tests/c/texture_plan_table.cpp over csrc/rt_texture_plan.h (and the host texture half of csrc/rt_scene.h): a stand-alone program, built
plainly and with -fsanitize=address,undefined, and once per deliberate fault of the rules, each of which must make it fail.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "c", "texture_plan_table.cpp")


def build(tmp_path, name, flags):
    """(rt_scene.h reads the HIP headers, so the host compiler is hipcc's, host only.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", *flags, "-o", exe, SOURCE])
    return exe


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan-ubsan"])
def test_layout_source_index_and_the_lane_loop(tmp_path, flags):
    """texel_layout against the old loop (0, 1, 254 records), source_index and its stepped form over every destination byte of 1x1, 1x5, 5x1,
    17x9 and 64x33 with both flag values, find_image at every boundary, and place_unit over whole blobs, byte-equal to the host's blob."""
    out = subprocess.run([build(tmp_path, "texture_plan_table", flags)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:4] == ["layout ok", "source_index ok", "find_image ok", "blob ok"] and out.stderr == ""


@pytest.mark.parametrize("mutant, stage", [("RTX_MUTANT_NO_FLIP", "source_index"), ("RTX_MUTANT_PADDING", "blob"), ("RTX_MUTANT_FIND", "find_image")])
def test_each_mutant_of_the_rules_is_caught(tmp_path, mutant, stage):
    """The flip dropped, padding not stored as 0, find_image off by one at an image's first byte: each fails the stage that is about it."""
    out = subprocess.run([build(tmp_path, mutant.lower(), ("-D" + mutant,))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "CHECK(" in out.stderr, out.stdout + out.stderr
    assert f"{stage} ok" not in out.stdout
