"""The numpy model of texture programs (tests/texprog_model.py) against the compiled C++ eval of csrc/rt_texprog.h on the CPU
(tests/c/texprog_table.cpp in its `eval` mode), over the family the GPU tests use; and three mutants of the model, each caught.  No GPU."""
import struct
import subprocess

import numpy as np
import pytest

import texprog_model as M
import texture_cases as tc
from test_texprog_cpp import build


@pytest.fixture(scope="module")
def evaluated(tmp_path_factory):
    """name -> (program, u, v, points, colours from the C++ eval), computed once."""
    exe = build(tmp_path_factory.mktemp("texprog"), "texprog_table", ())
    rng = np.random.default_rng(11)
    centre = (0.3, -0.2, 0.1)
    points = M.seam_points(rng, 1.5, centre, 400)
    uv = M.uv_of(1.5, centre, points)
    out = {}
    for name, prog in M.family().items():
        lines = "".join(prog.hex() + " " + " ".join(struct.pack("<d", x)[::-1].hex() for x in (u, v, *p)) + "\n" for (u, v), p in zip(uv, points))
        res = subprocess.run([exe, "eval"], input=lines, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "refused" not in res.stdout, (name, res.stdout[-200:], res.stderr[-400:])
        out[name] = (prog, uv[:, 0], uv[:, 1], points, np.array([[int(t) for t in ln.split()] for ln in res.stdout.split("\n") if ln], np.uint8))
    return out


def test_the_family_covers_what_it_says():
    fam = M.family()
    ops = {name for prog in fam.values() for name, _ in M.T.decode(prog)[0]}
    assert ops == set(M.T.OPCODES)
    assert len(M.T.decode(fam["len64"])[0]) == 64 and M.depth_of(fam["depth8"]) == 8 and max(M.depth_of(p) for p in fam.values()) == 8
    for prog in fam.values():
        M.T.check_program(prog)


def test_the_model_is_the_compiled_eval(evaluated):
    for name, (prog, u, v, pts, cpp) in evaluated.items():
        got = M.run(prog, u, v, pts)
        assert got.shape == cpp.shape and np.array_equal(got, cpp), (name, int((got != cpp).any(axis=1).sum()))


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_each_mutant_of_the_model_is_caught(evaluated, mutant):
    """MIN made commutative in its NaN, the byte by rounding, FLT without the band: each differs from the compiled eval somewhere."""
    assert any(not np.array_equal(M.run(prog, u, v, pts, mutant), cpp) for prog, u, v, pts, cpp in evaluated.values())


def test_the_byte_rule_of_the_model():
    v = np.array([0.0, 255.0, 255.999, 256.0, -1.0, -0.0, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 1, 1e300, -1e300, np.inf, -np.inf, np.nan, 257.5, -257.0])
    assert M.to_byte(v).tolist() == [0, 255, 255, 0, 255, 0, 255, 0, 255, 255, 0, 255, 0, 0, 1, 255]
    x = np.arange(256) / 255.0
    assert np.array_equal(M.to_byte(x * 255.0), (x * 255.0).astype(np.int32).astype(np.uint8))  # ramp_byte
