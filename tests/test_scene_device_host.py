"""Scene.make on the device, the part that needs no GPU: the symbols and their signatures, the refusals that come before any device call,
HITTABLE_DTYPE against the ABI, and the host code -- which now computes every record through csrc/rt_scene_plan.h -- held to the scenes
the code before it made (tests/golden/scene_images_parent.json, written by tests/golden/make_scene_images_parent.py on the parent commit)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import scene_device_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = json.load(open(os.path.join(HERE, "golden", "scene_images_parent.json")))


def test_the_symbols_exist_with_the_documented_signatures(rt):
    from ray_tracing_fsharp_amd import _lib
    A = rt._abi
    P = C.POINTER
    want = {
        "rt_scene_create_device": (C.c_int, [C.c_int32, C.c_void_p, C.c_size_t, P(A.rt_texture), C.c_size_t, P(A.rt_scene_options), C.c_void_p, P(C.c_void_p)]),
        "rt_dev_scene_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, P(C.c_size_t), P(C.c_uint32)]),
        "rt_dev_encode_image": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_size_t)]),
        "rt_dev_encode_image_radix": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, P(C.c_size_t)]),
        "rt_dev_scene_has_host_mirror": (C.c_int, [C.c_void_p]),
    }
    header = open(os.path.join(os.path.dirname(HERE), "include", "rtfs_amd.h")).read()
    for name, (res, args) in want.items():
        assert hasattr(rt.lib, name) and name + "(" in header
        assert _lib.SIGNATURES[name][0] is res and _lib.SIGNATURES[name][1] == args, name
    assert rt.lib.rt_abi_version() == 7  # added symbols only
    assert callable(rt.Scene.make_device) and callable(rt.hittable_records)


def test_hittable_dtype_is_rt_hittable(rt):
    A = rt._abi
    dt = rt.HITTABLE_DTYPE
    assert dt.itemsize == C.sizeof(A.rt_hittable) == rt.lib.rt_abi_sizeof(0)
    assert list(dt.names) == [f[0] for f in A.rt_hittable._fields_]
    for k, name in enumerate(dt.names):
        assert dt.fields[name][1] == getattr(A.rt_hittable, name).offset == rt.lib.rt_abi_offsetof(0, k), name
    assert dt == sc.DT  # the cases' own spelling of it
    objs = __import__("scenes").all_materials()[0]
    rec, tex = rt.hittable_records(objs, textures=True)
    hs, n, t, ntex, _ = rt.raytracing.flatten_hittables(objs)
    assert rec.dtype == dt and rec.shape == (n,) and rec.tobytes() == bytes(hs)[: n * dt.itemsize]
    assert tex.count == ntex and np.array_equal(rt.hittable_records(objs), rec)


def _call(rt, ptr, n, tex=None, ntex=0, opt=None, out=True, device=0):
    o = C.c_void_p(0x1234)
    code = rt.lib.rt_scene_create_device(device, ptr, n, tex, ntex, opt, None, C.byref(o) if out else None)
    return code, (rt.lib.rt_last_error() or b"").decode(), o.value


def test_argument_refusals_come_before_any_device_call(rt):
    """(so they are the same with and without a GPU; the pointer is never read)"""
    A = rt._abi
    t = (A.rt_texture * 1)()
    for args, text in (((None, 3), "d_hittables is NULL"),
                       ((0x1000, 3, None, 2), "textures is NULL"),
                       ((0x1004, 3), "d_hittables is not 8-byte aligned"),
                       ((0x1000, 3, t, 1, None, False), "out is NULL"),
                       ((0x1000, 3, t, 1, C.byref(A.rt_scene_options(A.RT_WALK_TREE_TUNED))), "walk_tree must be")):
        code, msg, out = _call(rt, *args)
        assert code == A.RT_ERR_INVALID_ARGUMENT and text in msg, (args, msg)
        assert out == 0x1234  # *out is written on success only


def test_no_gpu_means_no_device_not_a_fallback(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    code, msg, out = _call(rt, 0x1000, 3)
    assert code == A.RT_ERR_NO_DEVICE and "no CPU fallback" in msg and out == 0x1234
    code, msg, _ = _call(rt, None, 0)  # the empty scene too
    assert code == A.RT_ERR_NO_DEVICE
    s = sc.create("rt_scene_create_ex", *sc.CASES["spheres-3"]())[1]
    assert rt.hooks.scene_has_host_mirror(s)  # a scene made on the host always has its arrays
    with pytest.raises(rt.RtError) as e:
        rt.hooks.scene_image(s)
    assert e.value.code == A.RT_ERR_NO_DEVICE
    with pytest.raises(rt.RtError) as e:
        rt.hooks.encode_image(s)
    assert e.value.code == A.RT_ERR_NO_DEVICE


def test_make_device_refuses_in_the_style_of_the_other_wrappers(rt):
    rec = sc.CASES["spheres-3"]()[0]
    with pytest.raises(TypeError, match="records must be a numpy array or a torch tensor on a GPU, not list"):
        rt.Scene.make_device([1, 2])
    with pytest.raises(TypeError, match="records must have dtype HITTABLE_DTYPE, not uint8"):
        rt.Scene.make_device(rec.view(np.uint8))
    with pytest.raises(ValueError, match=r"records must have shape \[n\], not \[3, 1\]"):
        rt.Scene.make_device(rec.reshape(3, 1))
    with pytest.raises(TypeError, match="textures must be a TextureTable"):
        rt.Scene.make_device(rec, textures=[1])
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(rec.view(np.uint8).reshape(3, -1).copy())
    with pytest.raises(ValueError, match="records must be on a GPU"):
        rt.Scene.make_device(t)
    with pytest.raises(TypeError, match="records must have dtype torch.uint8, not torch.int32"):
        rt.Scene.make_device(t.to(torch.int32))
    with pytest.raises(ValueError, match=r"records must have shape \[n, 104\], not \[104, 3\]"):
        rt.Scene.make_device(t.T)


def test_the_peel_case_is_as_deep_as_its_name_says(rt):
    """(the case is there for the depth scan and the order by depth on a deep, unbalanced tree: it must not lose that unnoticed)"""
    scene = sc.create("rt_scene_create_ex", *sc.CASES["peel-64"](), "sah")[1]
    assert scene.info()["walk_tree_depth"] == sc.PEEL_DEPTH == PARENT["peel-64/sah"]["info"]["walk_tree_depth"]
    assert max(v["info"]["walk_tree_depth"] for v in PARENT.values()) == sc.PEEL_DEPTH


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_host_scene_is_the_parents(rt, name):
    records, textures = sc.CASES[name]()
    for walk in ("sah", "reference"):
        code, scene, text = sc.create("rt_scene_create_ex", records, textures, walk)
        assert code == 0, text
        assert sc.scene_record(scene) == PARENT[f"{name}/{walk}"], walk


@pytest.mark.parametrize("name", sorted(sc.REFUSALS))
def test_the_refusals_name_the_smallest_index_and_its_first_failing_check(rt, name):
    """What the device route has to reproduce: the host's own status and text for these record sets (the smaller index wins, and on one
    hittable the first check in the order kind, style, texture range, Pixel style)."""
    A = rt._abi
    records, textures = sc.REFUSALS[name]()
    code, scene, text = sc.create("rt_scene_create_ex", records, textures)
    want = {"bad-kind-at-5": (A.RT_ERR_INVALID_ARGUMENT, "hittable 5: bad kind"),
            "two-bad-smaller-wins": (A.RT_ERR_INVALID_ARGUMENT, "hittable 2: bad kind"),
            "bad-style": (A.RT_ERR_INVALID_ARGUMENT, "hittable 3: bad style"),
            "bad-plane-style": (A.RT_ERR_INVALID_ARGUMENT, "hittable 3: bad style"),
            "texture-out-of-range": (A.RT_ERR_INVALID_ARGUMENT, "hittable 4: texture index out of range"),
            "kind-and-texture-on-one": (A.RT_ERR_INVALID_ARGUMENT, "hittable 1: bad kind"),
            "textures-255": (A.RT_ERR_UNSUPPORTED, "at most 254 textures")}.get(name)
    if name == "texture-on-pixel-style":
        assert code == A.RT_ERR_INVALID_ARGUMENT and text.endswith(": this style carries a Pixel, not a Texture")
    else:
        assert (code, text) == want
    assert scene is None
