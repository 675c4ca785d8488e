"""tests/golden/texprog_cases.npz against its generator: tests/fsharp_literal.py, with the closure each program denotes, renders the
frames again on the CPU (mpmath) and they equal the recorded ones.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def test_the_recorded_frames_are_what_the_literal_renders():
    pytest.importorskip("mpmath")
    import make_texprog_cases as G
    recorded = np.load(G.PATH)
    fresh = G.generate()
    assert sorted(recorded.files) == sorted(fresh) and len(fresh) == 6
    for name, frame in fresh.items():
        assert frame.shape == (2 * G.MAX_H + 1, 2 * G.MAX_W + 1, 4) and frame.dtype == np.int32
        assert np.array_equal(recorded[name], frame), name
    # the frames are about the programs: every case differs from every other
    names = sorted(fresh)
    assert all((fresh[a] != fresh[b]).any() for i, a in enumerate(names) for b in names[i + 1:])


def test_the_closure_is_the_model_on_single_points():
    """The generator's scalar closure (Python floats, the literal's sine) and the numpy model agree on the whole family: two restatements
    of the rules, written apart."""
    pytest.importorskip("mpmath")
    import fsharp_literal as L
    import make_texprog_cases as G
    import texprog_model as M
    rng = np.random.default_rng(2)
    pts = M.seam_points(rng, 1.0, (0.0, 0.0, 0.0), 60)
    uv = M.uv_of(1.0, (0.0, 0.0, 0.0), pts)
    for name, prog in G.programs().items():
        want = M.run(prog, uv[:, 0], uv[:, 1], pts)
        f = G.closure_of(prog, L)
        got = np.array([f(float(u), float(v))[1](tuple(float(x) for x in p)) for (u, v), p in zip(uv, pts)], np.uint8)
        assert np.array_equal(got, want), name
