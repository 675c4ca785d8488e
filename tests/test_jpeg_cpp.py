"""LoadImage in the C++ host mirror (RayTracing.hpp LoadImage::fromFile, SampleImages::earth(path)) and `rtfs_render earth --earthmap
PATH`: the scene the driver builds from tests/golden/earthmap.jpg is the Python mirror's from the decoded fixture, a missing or refused
file is a loud error, and -- on the GPU -- the driver renders the bytes of the Python mirror.  (`--list` keeps printing the catalogue of
scenes that take no data: `earth` needs its file, as `gradient` needs none of the renderer.)"""
import dataclasses
import os

import numpy as np
import pytest

from test_host_cpp import exe, fnv1a, run  # noqa: F401  (exe: the module-scoped fixture that builds the driver)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, "tests", "golden", "earthmap.jpg")


def _bitmap():
    return np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb.npz"))["rgb"]


def test_cpp_earth_scene_flattens_like_the_python_mirror(rt, exe):  # noqa: F811
    out = run(exe, "earth", "--info", "--earthmap", JPEG)
    assert out.returncode == 0, out.stderr
    fields = dict(kv.split("=") for kv in out.stdout.split())
    objs, cam, w, h = rt.sample_images.earth(_bitmap())
    s = rt.Scene.make(objs)
    info = s.info()
    assert (int(fields["bounded"]), int(fields["unbounded"]), int(fields["nodes"])) == (info["n_bounded"], info["n_unbounded"], info["n_nodes"]) == (1, 1, 1)
    assert (int(fields["maxW"]), int(fields["maxH"]), int(fields["spp"]), int(fields["bounce"])) == (w, h, cam.SamplesPerPixel, cam.BounceDepth)
    assert int(fields["tree"]) == fnv1a(*s.tree())


def test_cpp_earth_refusals(exe, tmp_path):  # noqa: F811
    r = run(exe, "earth", str(tmp_path / "x.ppm"))
    assert r.returncode == 1 and "earth needs --earthmap PATH" in r.stderr
    r = run(exe, "earth", str(tmp_path / "x.ppm"), "--earthmap", str(tmp_path / "missing.jpg"))
    assert r.returncode == 1 and "cannot open" in r.stderr
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    for name, text in (("progressive", "progressive JPEG (SOF2)"), ("flipped", "coefficient index past 63")):
        (tmp_path / "bad.jpg").write_bytes(z["bad/" + name].tobytes())
        r = run(exe, "earth", str(tmp_path / "x.ppm"), "--info", "--earthmap", str(tmp_path / "bad.jpg"))
        assert r.returncode == 1 and text in r.stderr, r.stderr
    assert not (tmp_path / "x.ppm").exists()


@pytest.mark.gpu
def test_cpp_driver_renders_earth_from_the_jpeg(rt, exe, tmp_path):  # noqa: F811
    out = tmp_path / "o.ppm"
    r = run(exe, "earth", str(out), "--earthmap", JPEG, "--scale", "20", "--spp", "20", "--seed", "8")
    assert r.returncode == 0, r.stderr
    objs, cam, w, h = rt.sample_images.earth(_bitmap())
    cam = dataclasses.replace(cam, SamplesPerPixel=20)
    total, image = rt.Scene.render(lambda _: None, lambda _: None, max(1, w // 20), max(1, h // 20), cam, rt.Scene.make(objs), seed=8)
    assert out.read_bytes() == rt.ImageOutput.formatPpm(True, rt.Image.render(image))
