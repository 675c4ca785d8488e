"""tests/c/texprog_table.cpp over csrc/rt_texprog.h: a stand-alone program, built plainly and with -fsanitize=address,undefined, and once per
deliberate fault of the header, each of which must make it fail.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "c", "texprog_table.cpp")
STAGES = ["check ok", "eval ok", "enumerate ok", "bytes ok"]


def build(tmp_path, name, flags):
    """(hipcc's host compiler on plain C++: in the host pass of a HIP translation unit rt_trig.h's sine tables are stubs, since nothing on
    the host side of the product evaluates a sine; rt_texprog.h as plain C++17 has the real ones)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-command-line-argument", "-O1", *flags, "-o", exe, SOURCE])
    return exe


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "asan-ubsan"])
def test_check_eval_every_short_program_and_the_byte_rule(tmp_path, flags):
    """check over every reason (each program a heap block of exactly its size), eval on programs whose values are known by hand, every
    program of at most three instructions checked or refused without a fault, the byte rule at 0, 255, 255.999, 256, -1, -0.0, +-2^31,
    +-1e300, +-inf and NaN."""
    out = subprocess.run([build(tmp_path, "texprog_table", flags)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:4] == STAGES and out.stderr == ""


@pytest.mark.parametrize("mutant, stage", [("RTXP_MUTANT_NO_DEPTH_CHECK", "check"), ("RTXP_MUTANT_SELECT_ORDER", "eval"), ("RTXP_MUTANT_NO_CLAMP", "eval")])
def test_each_fault_of_the_header_is_caught(tmp_path, mutant, stage):
    """The depth check dropped, SELECT's operands the other way round, the clamp in front of the int conversion dropped."""
    out = subprocess.run([build(tmp_path, mutant.lower(), ("-D" + mutant,))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "CHECK(" in out.stderr, out.stdout + out.stderr
    assert f"{stage} ok" not in out.stdout
