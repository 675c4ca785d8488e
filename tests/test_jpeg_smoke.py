"""tests/c/jpeg_smoke.c, the C99 consumer of rt_jpeg_get_info / rt_decode_jpeg / rt_decode_jpeg_device: the host decoder and the refusals
hold without a GPU (with one, tests/test_gpu_jpeg.py runs it again and it decodes on the device)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_jpeg_smoke(tmp_path):
    exe = str(tmp_path / "jpeg_smoke")
    libdir = os.path.join(ROOT, "ray-tracing-fsharp_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "jpeg_smoke.c"),
                           "-L", libdir, "-lrtfs_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


def run_jpeg_smoke(tmp_path):
    """The program over the cut-source case and its damaged twin -> (stdout, the fixture's bitmap)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    (tmp_path / "good.jpg").write_bytes(z["jpeg/cut-source-40x56-420-q75"].tobytes())
    (tmp_path / "damaged.jpg").write_bytes(z["bad/flipped"].tobytes())
    out = subprocess.run([build_jpeg_smoke(tmp_path), str(tmp_path / "good.jpg"), str(tmp_path / "damaged.jpg")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout, z["rgb/cut-source-40x56-420-q75"]


def test_c_program_decodes_on_the_host_and_checks_the_refusals(rt, tmp_path):
    text, want = run_jpeg_smoke(tmp_path)
    assert "jpeg: refusals ok" in text
    assert f"host 56x40 sum {int(want.astype(np.int64).sum())}" in text  # libjpeg's bitmap
    assert ("jpeg: decoded on the GPU" in text) == (rt.device_count() > 0)
