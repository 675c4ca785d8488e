"""Image textures from device memory, the part that needs no GPU: the symbols, every refusal that comes before a device call (status and
text), RT_ERR_NO_DEVICE after them, the Python errors of ofImageDevice / ofJpeg, TextureTable's compatibility, and the host texture half
after its move to rtt::texel_layout (the blob's size for every scene of tests/texture_cases.py against the rule restated here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("rt_scene_create_textures", "rt_scene_create_device_textures", "rt_of_image_device", "rt_scene_set_texels_device", "rt_dev_scene_texels",
       "rt_dev_last_texture_plan")


@pytest.fixture(scope="module")
def jpegs():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    good = {k[5:]: (z[k].tobytes(), z["rgb/" + k[5:]]) for k in z.files if k.startswith("jpeg/")}
    bad = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("bad/")}
    return good, bad


def err(rt):
    return (rt.lib.rt_last_error() or b"").decode()


def test_the_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib
    A = rt._abi
    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared and hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols and one struct only
    assert rt.lib.rt_abi_sizeof(A.ABI_STRUCT_TEXELS_SOURCE) == C.sizeof(A.rt_texels_source) == 32
    assert (A.RT_TEXELS_RECORD, A.RT_TEXELS_DEVICE, A.RT_TEXELS_JPEG, A.RT_TEXELS_TOP_FIRST) == (0, 1, 2, 1)
    for name in ("ofImageDevice", "ofJpeg"):
        assert callable(getattr(rt.ParameterisedTexture, name))
    assert callable(rt.Scene.set_image) and callable(rt.Scene.texture_index) and callable(rt.sample_images.earth_device)
    assert callable(rt.hooks.scene_texels) and callable(rt.hooks.texture_plan)


def table(rt, *records):
    return (rt._abi.rt_texture * len(records))(*records)


def sources(rt, *entries):
    return (rt._abi.rt_texels_source * len(entries))(*entries)


def create(rt, which, tex, ntex, src, out=True, opt=None, d_h=0x1000, n=1):
    """rt_scene_create_textures (which = "host") / rt_scene_create_device_textures ("device") -> (status, text, *out)."""
    A = rt._abi
    o = C.c_void_p(0x1234)
    if which == "host":
        hs = (A.rt_hittable * 1)(tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0, 0, 0), 1.0, -1))
        code = rt.lib.rt_scene_create_textures(hs, n, tex, ntex, src, opt, 0, None, C.byref(o) if out else None)
    else:
        code = rt.lib.rt_scene_create_device_textures(0, d_h, n, tex, ntex, src, opt, None, C.byref(o) if out else None)
    return code, err(rt), o.value


@pytest.mark.parametrize("which", ["host", "device"])
def test_argument_refusals_come_before_any_device_call(rt, which):
    """(so they are the same with and without a GPU; no pointer is read)"""
    A = rt._abi
    S = A.rt_texels_source
    keep = []
    img = tc.rec_image(tc.synthetic_image(3, 5), keep)  # 45 bytes
    col = tc.rec_colour((1, 2, 3))
    ok = S(A.RT_TEXELS_DEVICE, A.RT_TEXELS_TOP_FIRST, 0x2000, 45)
    bad_size = S(A.RT_TEXELS_DEVICE, 0, 0x2000, 45)
    bad_size.struct_size = 24
    cases = [
        ((table(rt, img), 1, sources(rt, ok), False), "out is NULL"),
        ((None, 1, sources(rt, ok)), "textures is NULL"),
        ((table(rt, img), 1, sources(rt, ok), True, C.byref(A.rt_scene_options(A.RT_WALK_TREE_TUNED))), "walk_tree must be"),
        ((table(rt, img), 1, sources(rt, bad_size)), "source 0: struct_size is not sizeof(rt_texels_source)"),
        ((table(rt, col, img), 2, sources(rt, S(), S(3, 0, 0x2000, 45))), "source 1: unknown kind"),
        ((table(rt, img), 1, sources(rt, S(A.RT_TEXELS_DEVICE, 2, 0x2000, 45))), "source 0: unknown flag bit"),
        ((table(rt, img), 1, sources(rt, S(A.RT_TEXELS_RECORD, 0x80000000))), "source 0: unknown flag bit"),
        ((table(rt, img, col), 2, sources(rt, ok, S(A.RT_TEXELS_DEVICE, 0, 0x2000, 45))), "source 1: texels for a texture that is not an image"),
        ((table(rt, img, col), 2, sources(rt, ok, S(A.RT_TEXELS_JPEG, 0, 0x2000, 45))), "source 1: texels for a texture that is not an image"),
        ((table(rt, img), 1, sources(rt, S(A.RT_TEXELS_DEVICE, 0, None, 45))), "source 0: data is NULL"),
        ((table(rt, img), 1, sources(rt, S(A.RT_TEXELS_JPEG, 0, None, 45))), "source 0: data is NULL"),
        ((table(rt, img), 1, sources(rt, S(A.RT_TEXELS_DEVICE, 0, 0x2000, 44))), "source 0: bytes is below width * height * 3"),
    ]
    for args, text in cases:
        code, msg, out = create(rt, which, *args)
        assert code == A.RT_ERR_INVALID_ARGUMENT and (msg == text or (text.endswith("must be") and text in msg)), (text, code, msg)
        assert out == 0x1234  # *out is written on success only
    if which == "device":
        for d_h, n, text in ((None, 3, "d_hittables is NULL"), (0x1004, 3, "d_hittables is not 8-byte aligned")):
            code, msg, out = create(rt, which, table(rt, img), 1, sources(rt, ok), d_h=d_h, n=n)
            assert code == A.RT_ERR_INVALID_ARGUMENT and msg == text and out == 0x1234


def test_of_image_and_set_texels_refusals_come_before_any_device_call(rt):
    A = rt._abi
    lib = rt.lib
    for args, text in (((0, None, 5, 3, 0x3000, 45, None), "NULL argument"), ((0, 0x2000, 5, 3, None, 45, None), "NULL argument"),
                       ((0, 0x2000, 0, 3, 0x3000, 45, None), "width and height must be positive"),
                       ((0, 0x2000, 5, -1, 0x3000, 45, None), "width and height must be positive"),
                       ((0, 0x2000, 5, 3, 0x3000, 44, None), "capacity is below width * height * 3"),
                       ((0, 0x2000, 5, 3, 0x2000, 45, None), "d_texels overlaps d_bitmap: the reversal is not done in place"),
                       ((0, 0x2000, 5, 3, 0x2000 + 44, 45, None), "d_texels overlaps d_bitmap: the reversal is not done in place"),
                       ((0, 0x2000 + 44, 5, 3, 0x2000, 45, None), "d_texels overlaps d_bitmap: the reversal is not done in place")):
        assert lib.rt_of_image_device(*args) == A.RT_ERR_INVALID_ARGUMENT and err(rt) == text, args
    # a scene made on the host: records 0 (an image, 3 x 5), 1 (a colour)
    keep = []
    tex = table(rt, tc.rec_image(tc.synthetic_image(3, 5), keep), tc.rec_colour((1, 2, 3)))
    hs = (A.rt_hittable * 1)(tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0, 0, 0), 1.0, 0))
    out = C.c_void_p()
    assert lib.rt_scene_create(hs, 1, tex, 2, C.byref(out)) == 0
    scene = rt.Scene(out.value, keep)
    for args, text in (((None, 0, 0, 0x2000, 45, 1, None), "NULL argument"), ((scene.handle, 0, 0, None, 45, 1, None), "NULL argument"),
                       ((scene.handle, 0, 0, 0x2000, 45, 2, None), "unknown flag bit"),
                       ((scene.handle, 2, 0, 0x2000, 45, 1, None), "texture index out of range"),
                       ((scene.handle, -1, 0, 0x2000, 45, 1, None), "texture index out of range"),
                       ((scene.handle, 1, 0, 0x2000, 45, 1, None), "texture 1 is not an image"),
                       ((scene.handle, 0, 0, 0x2000, 44, 0, None), "bytes is below width * height * 3")):
        assert lib.rt_scene_set_texels_device(*args) == A.RT_ERR_INVALID_ARGUMENT and err(rt) == text, args
    assert rt.hooks.scene_has_host_mirror(scene) and scene.info()["texel_bytes"] == 48  # unchanged
    assert lib.rt_dev_last_texture_plan(None) == A.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_dev_scene_texels(None, 0, None, 0, None, None) == A.RT_ERR_INVALID_ARGUMENT


def test_no_gpu_means_no_device_after_the_checks(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    S = A.rt_texels_source
    keep = []
    img = tc.rec_image(tc.synthetic_image(3, 5), keep)
    ok = S(A.RT_TEXELS_DEVICE, A.RT_TEXELS_TOP_FIRST, 0x2000, 45)
    for which in ("host", "device"):
        code, msg, out = create(rt, which, table(rt, img), 1, sources(rt, ok))
        assert code == A.RT_ERR_NO_DEVICE and "no CPU fallback" in msg and out == 0x1234
        # sources == NULL is the existing call, which without a GPU answers the same
        code, msg, out = create(rt, which, table(rt, img), 1, None)
        assert code == A.RT_ERR_NO_DEVICE and out == 0x1234
    hs = (A.rt_hittable * 1)(tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0, 0, 0), 1.0, 0))
    o = C.c_void_p(0x1234)
    assert rt.lib.rt_scene_create_gpu_trees(hs, 1, table(rt, img), 1, None, 0, C.byref(o)) == A.RT_ERR_NO_DEVICE and o.value == 0x1234
    assert rt.lib.rt_of_image_device(0, 0x2000, 5, 3, 0x3000, 45, None) == A.RT_ERR_NO_DEVICE
    out = C.c_void_p()
    assert rt.lib.rt_scene_create(hs, 1, table(rt, img), 1, C.byref(out)) == 0
    scene = rt.Scene(out.value, keep)
    assert rt.lib.rt_scene_set_texels_device(scene.handle, 0, 0, 0x2000, 45, 1, None) == A.RT_ERR_NO_DEVICE
    assert rt.hooks.scene_has_host_mirror(scene)
    with pytest.raises(rt.RtError) as e:
        rt.hooks.scene_texels(scene)
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert rt.hooks.texture_plan() == dict.fromkeys(rt.hooks.TEXTURE_PLAN, 0)


def test_of_image_device_refuses_in_the_style_of_the_other_wrappers(rt):
    import torch
    PT = rt.ParameterisedTexture
    with pytest.raises(TypeError, match="bitmap must be a torch tensor on a GPU, not ndarray"):
        PT.ofImageDevice(np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(TypeError, match="bitmap must have dtype torch.uint8, not torch.float32"):
        PT.ofImageDevice(torch.zeros((2, 2, 3)))
    for shape in ((2, 2), (2, 2, 4), (0, 2, 3), (2, 0, 3), (1, 2, 2, 3)):
        with pytest.raises(ValueError, match=r"bitmap must have shape \[height, width, 3\], not "):
            PT.ofImageDevice(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="bitmap must be on a GPU"):
        PT.ofImageDevice(torch.zeros((2, 2, 3), dtype=torch.uint8))


def test_texture_table_keeps_its_three_positional_fields(rt):
    t = rt.TextureTable((rt._abi.rt_texture * 1)(), 0, [])
    assert t.sources is None and t.index is None and len(t) == 5 and t[:3] == (t.records, t.count, t.keep)
    objs = __import__("scenes").all_materials()[0]
    rec, tex = rt.hittable_records(objs, textures=True)
    assert tex.sources is None  # host texels alone: the existing calls
    assert len(rt.raytracing.flatten_hittables(objs)) == 5


def test_of_jpeg_reads_the_header_and_refuses_as_the_decoder_does(rt, jpegs):
    good, bad = jpegs
    A = rt._abi
    data, rgb = good["noise-17x33-420-q95-r2"]
    t = rt.ParameterisedTexture.ofJpeg(data)
    assert t.kind == A.RT_TEXTURE_IMAGE and t.size == rgb.shape[:2] and t.jpeg == data and t.image is None and t.bitmap is None
    sphere = rt.Hittable.Sphere(rt.Sphere.make(rt.SphereStyle.LightSource(rt.ParameterisedTexture.toTexture((1.0, rt.Point.make(0, 0, 0)), t)),
                                               rt.Point.make(0, 0, 0), 1.0))
    rec, table_ = rt.hittable_records([sphere], textures=True)
    assert table_.count == 1 and (table_.records[0].height, table_.records[0].width) == rgb.shape[:2] and not table_.records[0].texels
    q = table_.sources[0]
    assert (q.struct_size, q.kind, q.flags, q.bytes) == (32, A.RT_TEXELS_JPEG, A.RT_TEXELS_TOP_FIRST, len(data))
    assert C.string_at(q.data, 4) == data[:4] and table_.index[id(t)][0] == 0
    refused = 0
    for name, blob in bad.items():
        buf = np.zeros(1 << 16, np.uint8)
        i = A.rt_jpeg_info()
        if rt.lib.rt_jpeg_get_info(blob, len(blob), C.byref(i)) == 0:
            continue  # (a damaged stream behind a good header: found when the scene is made, on the device)
        rc = rt.lib.rt_decode_jpeg(blob, len(blob), buf.ctypes.data, buf.size)
        want = err(rt)
        with pytest.raises(rt.RtError) as e:
            rt.ParameterisedTexture.ofJpeg(blob)
        assert e.value.code == rc != 0 and str(want) in str(e.value), name
        refused += 1
    assert refused >= 2  # progressive, cmyk


def layout(records, ntex, image_kind):
    """The rule, restated: images in index order, width * height * 3 bytes each, zero-padded to a multiple of 16."""
    at, offs = 0, []
    for i in range(ntex):
        r = records[i]
        if r.kind != image_kind:
            offs.append(None)
            continue
        offs.append(at)
        at += (r.width * r.height * 3 + 15) // 16 * 16
    return at, offs


def test_the_texture_half_lays_the_blob_out_as_before(rt):
    seen = 0
    for case in (c for family in sorted(tc.FAMILIES) for c in tc.FAMILIES[family]()):
        out = C.c_void_p()
        assert rt.lib.rt_scene_create(case.hs, case.n, case.tex, case.ntex, C.byref(out)) == 0, case.name
        scene = rt.Scene(out.value, case.keep)
        total, offs = layout(case.tex, case.ntex, rt._abi.RT_TEXTURE_IMAGE)
        assert scene.info()["texel_bytes"] == total and scene.info()["n_textures"] == case.ntex, case.name
        seen += sum(o is not None for o in offs)
    assert seen >= 8
