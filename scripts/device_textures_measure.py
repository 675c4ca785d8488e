"""From a JPEG file's bytes in host memory to a scene ready to render: three routes, wall clock, medians of 7 with the routes alternating.

  parent  the route before image textures were device data, on a PARENT build of the library (--parent-lib): rt_decode_jpeg_device ->
          download -> numpy row reversal -> rt_scene_create_device with host texels
  jpeg    rt_scene_create_device_textures with a RT_TEXELS_JPEG source (ParameterisedTexture.ofJpeg)
  device  rt_decode_jpeg_device (not waited for) -> a RT_TEXELS_DEVICE source (ParameterisedTexture.ofImageDevice)

The scene is sample_images.earth's (two objects, resident as records on the device).  Files: tests/golden/earthmap.jpg, and an 8192x4096
enlargement of it encoded 4:4:4 when PIL is importable (otherwise recorded as not measured).  Also of_image_kernel alone (through
rt_scene_set_texels_device) against a device-to-device copy of the same byte count, from HIP events.  Needs a GPU.
usage: python scripts/device_textures_measure.py --parent-lib build_ab/librtfs_parent.so [--out profiles/r27/device_textures_measure.json]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "device_textures_measure.json"))
    args = ap.parse_args()
    import torch

    import ray_tracing_fsharp_amd as rt
    A, lib = rt._abi, rt.lib
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert parent.rt_abi_version() == A.RT_ABI_VERSION and not hasattr(parent, "rt_scene_create_device_textures")
        for name in ("rt_scene_destroy", "rt_scene_create_device", "rt_decode_jpeg_device"):
            getattr(parent, name).argtypes = getattr(lib, name).argtypes
    where = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(where).cuda_stream
    opt = A.rt_scene_options(A.RT_WALK_TREE_SAH)
    res = {"device_name": torch.cuda.get_device_name(0), "unit": "ms", "reps": REPS, "files": {}}

    files = {"earthmap.jpg": open(os.path.join(ROOT, "tests", "golden", "earthmap.jpg"), "rb").read()}
    try:
        from PIL import Image
        big = Image.open(io.BytesIO(files["earthmap.jpg"])).resize((8192, 4096), Image.BICUBIC)
        buf = io.BytesIO()
        big.save(buf, "JPEG", quality=90, subsampling=0)
        files["8192x4096-444-q90"] = buf.getvalue()
    except ImportError:
        res["files"]["8192x4096-444-q90"] = "not measured: PIL is not importable here"

    for name, data in files.items():
        info = rt.LoadImage.info(data)
        w, h = info["width"], info["height"]
        objs = rt.sample_images.earth(np.zeros((h, w, 3), np.uint8))[0]
        rec, table = rt.hittable_records(objs, textures=True)
        t = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), -1).copy()).to(where)
        tex = table.records
        d_rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=where)
        src = (A.rt_texels_source * 1)()

        def route_parent(which):
            stats = A.rt_jpeg_stats()
            assert which.rt_decode_jpeg_device(0, data, len(data), d_rgb.data_ptr(), d_rgb.numel(), stream, C.byref(stats)) == 0
            rows = np.ascontiguousarray(d_rgb.cpu().numpy()[::-1])
            tex[0].texels = rows.ctypes.data
            out = C.c_void_p()
            assert which.rt_scene_create_device(0, t.data_ptr(), len(rec), tex, 1, C.byref(opt), stream, C.byref(out)) == 0
            return out

        def route_jpeg():
            tex[0].texels = None
            src[0] = A.rt_texels_source(A.RT_TEXELS_JPEG, A.RT_TEXELS_TOP_FIRST, C.cast(C.c_char_p(data), C.c_void_p), len(data))
            out = C.c_void_p()
            assert lib.rt_scene_create_device_textures(0, t.data_ptr(), len(rec), tex, 1, src, C.byref(opt), stream, C.byref(out)) == 0, lib.rt_last_error()
            return out

        def route_device():
            tex[0].texels = None
            assert lib.rt_decode_jpeg_device(0, data, len(data), d_rgb.data_ptr(), d_rgb.numel(), stream, None) == 0
            src[0] = A.rt_texels_source(A.RT_TEXELS_DEVICE, A.RT_TEXELS_TOP_FIRST, d_rgb.data_ptr(), d_rgb.numel())
            out = C.c_void_p()
            assert lib.rt_scene_create_device_textures(0, t.data_ptr(), len(rec), tex, 1, src, C.byref(opt), stream, C.byref(out)) == 0, lib.rt_last_error()
            return out

        def timed(fn, destroy):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ms = 1e3 * (time.perf_counter() - t0)
            destroy(out)
            return round(ms, 4)

        routes = {"jpeg": (route_jpeg, lib.rt_scene_destroy), "device": (route_device, lib.rt_scene_destroy),
                  "old_route_this_build": (lambda: route_parent(lib), lib.rt_scene_destroy)}
        if parent is not None:
            routes["parent"] = (lambda: route_parent(parent), parent.rt_scene_destroy)
        # the same texels on every route first
        blobs = {}
        for key, (fn, destroy) in routes.items():
            if key == "parent":
                destroy(fn())
                continue
            s = rt.Scene(fn().value, [])
            blobs[key] = rt.hooks.scene_texels(s)[0]
            del s
        assert all(np.array_equal(b, blobs["jpeg"]) for b in blobs.values())
        row = {key: [] for key in routes}
        for _ in range(REPS):  # alternating
            for key, (fn, destroy) in routes.items():
                row[key].append(timed(fn, destroy))
        row["median"] = {key: round(float(np.median(v)), 4) for key, v in row.items()}
        row.update(width=w, height=h, file_bytes=len(data), texel_bytes=int(blobs["jpeg"].size))
        # of_image_kernel alone against a device-to-device copy of the same bytes
        s = rt.Scene(route_device().value, [])
        other = torch.empty_like(d_rgb)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        kernel, copy = [], []
        for _ in range(REPS):
            ev[0].record()
            assert lib.rt_scene_set_texels_device(s.handle, 0, 0, d_rgb.data_ptr(), d_rgb.numel(), A.RT_TEXELS_TOP_FIRST, stream) == 0
            ev[1].record()
            ev[1].synchronize()
            kernel.append(round(ev[0].elapsed_time(ev[1]), 4))
            ev[0].record()
            other.copy_(d_rgb)
            ev[1].record()
            ev[1].synchronize()
            copy.append(round(ev[0].elapsed_time(ev[1]), 4))
        row["of_image_kernel_ms"], row["device_to_device_copy_ms"] = kernel, copy
        row["median"]["of_image_kernel_ms"], row["median"]["device_to_device_copy_ms"] = float(np.median(kernel)), float(np.median(copy))
        del s
        res["files"][name] = row
        print(name, row["median"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
