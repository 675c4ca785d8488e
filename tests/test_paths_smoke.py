"""tests/c/paths_smoke.c, the C99 consumer of rt_camera_paths / rt_trace_paths: its argument checks hold without a GPU (with one,
tests/test_gpu_paths.py compares what its two launches print with the composer of tests/path_cases.py)."""
import dataclasses
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_paths_smoke(tmp_path):
    exe = str(tmp_path / "paths_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "paths_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def smoke_case(rt, orc):
    """paths_smoke.c's two launches, composed: (camera paths of its six list entries, ray paths of its five rays)."""
    import path_cases as pc
    from test_gpu_ray_queries import _smoke_scene
    max_w, max_h, cols, rows = 12, 7, 25, 15
    cam = rt.Camera.makeBasic(24, 1.0, 25.0 / 15.0, rt.Point.make(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=10)
    o = orc.OracleScene(_smoke_scene(rt))
    px = np.array([7 * cols + 12, 0, 9 * cols + 20, 8 * cols + 5, rows * cols - 1, 7 * cols + 12])
    rays = np.array([[0.0, 0.5, -2.0, 0.0, 0.0, 1.0], [0.0, 0.5, -2.0, 0.7, -0.2, 2.0], [0.0, 0.5, -2.0, 0.0, 0.0, 0.0],
                     [0.0, 0.5, -2.0, 0.0, -1.0, 0.3], [5.0, 5.0, 5.0, -1.0, -1.0, -1.0]])
    return (pc.camera_paths(orc, o, cam.to_abi(), max_w, max_h, 5, px, 4, 3), pc.ray_paths(orc, o, rays, 10, rng=None, seed=9, stream_base=100, sample=2))


def test_c_program_checks_the_path_arguments(rt, tmp_path):
    out = subprocess.run([build_paths_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "paths: argument checks ok" in out.stdout
