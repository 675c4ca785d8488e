"""Texture programs (RT_TEXTURE_PROGRAM, csrc/rt_texprog.h) on the device.  Two witnesses:

  * the numpy model (tests/texprog_model.py, held to the compiled C++ eval on the CPU by tests/test_texprog_model.py) for single points,
    through rt_dev_texture_colour_at and rt_dev_reflection;
  * equivalence: a scene whose UvRamp, Colour and two-colour Checkered records are replaced by the programs that denote them must give,
    bit for bit, the frame the oracle renders for the original scene, and on every other route what the original scene gives there.

The scene is texture_cases.mostly_textured_scene at 14 px: every primary hit evaluates a texture, so the texture park pool fills, and the
64 lanes of a wave sit on nine different programs, on images and on plain colours.  Every test fails on a library where kind 5 is refused.
"""
import dataclasses

import numpy as np
import pytest

import texprog_model as M
import texture_cases as tc
from ray_tracing_fsharp_amd import _abi as A
from ray_tracing_fsharp_amd import texprog as T
from test_gpu_textures import _first_difference, _plain_field

pytestmark = pytest.mark.gpu


# ---- programs that denote the existing kinds -------------------------------------------------------------------------------------------------
def twin(rt, p, root=True):
    """The ParameterisedTexture with every UvRamp, every two-colour Checkered and a root Colour replaced by the program that denotes it."""
    PT = rt.ParameterisedTexture
    if p.kind == A.RT_TEXTURE_UV_RAMP:
        return PT.Program(*[(float(p.pixel[k]), T.U * 255.0, T.V * 255.0)[p.ramp[k]] for k in range(3)])
    if p.kind == A.RT_TEXTURE_COLOUR and root:
        return PT.Program(*[float(c) for c in p.pixel])
    if p.kind == A.RT_TEXTURE_CHECKERED:
        if p.even.kind == A.RT_TEXTURE_COLOUR and p.odd.kind == A.RT_TEXTURE_COLOUR:  # Texture.fs:56-62 stated exactly
            less = T.flt(T.sin(p.grid * T.U) * T.sin(p.grid * T.V), 0.0)
            return PT.Program(*[T.select(less, float(p.even.pixel[k]), float(p.odd.pixel[k])) for k in range(3)])
        return PT.Checkered(twin(rt, p.even, False), twin(rt, p.odd, False), p.grid)
    return p


def twin_objects(rt, objs):
    out = []
    for o in objs:
        body = o.plane if o.kind == A.RT_HITTABLE_INFINITE_PLANE else o.sphere
        t = body.Style.texture
        if t is not None and t.param is not None:
            body = dataclasses.replace(body, Style=dataclasses.replace(body.Style, texture=dataclasses.replace(t, param=twin(rt, t.param))))
            o = dataclasses.replace(o, **({"plane": body} if o.kind == A.RT_HITTABLE_INFINITE_PLANE else {"sphere": body}))
        out.append(o)
    return out


@pytest.fixture(scope="module")
def frame(rt, orc):
    """The mostly-textured scene, its program twin, and the oracle's frame of the ORIGINAL (computed once, shared, never written)."""
    objs, cam, w, h = tc.mostly_textured_scene()
    progs = twin_objects(rt, objs)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=9, threads=8)
    for a in (acc, rgb):
        a.setflags(write=False)
    plain, scene = rt.Scene.make(objs), rt.Scene.make(progs)
    _, _, tex, ntex, _ = tc.flatten_hittables(progs)
    kinds = [tex[i].kind for i in range(ntex)]
    programs = {bytes(np.ctypeslib.as_array((A.C.c_uint8 * tex[i].width).from_address(tex[i].texels))) for i in range(ntex) if kinds[i] == A.RT_TEXTURE_PROGRAM}
    assert len(programs) >= 8 and A.RT_TEXTURE_IMAGE in kinds and A.RT_TEXTURE_CHECKERED in kinds
    return dict(objs=objs, progs=progs, cam=cam, w=w, h=h, acc=acc, rgb=rgb, st=st, plain=plain, scene=scene)


def _same(res, f, what):
    assert np.array_equal(res.accum.reshape(f["acc"].shape), f["acc"]) and np.array_equal(res.rgb.reshape(f["rgb"].shape), f["rgb"]), what


# ---- points: the model -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family_scene(rt):
    fam = M.family()
    names = sorted(fam)
    PT, H, S = rt.ParameterisedTexture, rt.Hittable, rt.SphereStyle
    objs = []
    for i, name in enumerate(names):
        param = dataclasses.replace(PT.Program(1.0, 2.0, 3.0), program=fam[name])  # (some are written by hand, not by the compiler)
        c = tc.centre_of(i)
        objs.append(H.Sphere(rt.Sphere.make(S.LightSource(PT.toTexture((1.5, tc.P(*(c + np.array([0.3, -0.2, 0.1])))), param)), tc.P(*c), 1.0)))
    objs.append(tc.sky())
    hs, _, _, _, _ = tc.flatten_hittables(objs)
    return names, fam, rt.Scene.make(objs), [hs[i].texture for i in range(len(names))]


def test_points_equal_the_model_through_the_hook_and_reflection(rt, orc, family_scene):
    """About 1,000 points per program -- uniform, the seam, the poles, the axis points with both signs of zero: (u, v) bit for bit the
    oracle's, the colour the model's; and Hittable.reflection of a LightSource wearer under white light hands that colour on."""
    names, fam, scene, ids = family_scene
    rng = np.random.default_rng(5)
    for i, name in enumerate(names):
        centre = tc.centre_of(i) + np.array([0.3, -0.2, 0.1])
        pts = M.seam_points(rng, 1.5, centre, 1000)
        uv, want = M.colour_at(fam[name], 1.5, centre, pts)
        uv1, got = rt.hooks.texture_colour_at(scene, ids[i], pts)
        assert np.array_equal(uv1.view(np.uint64), uv.view(np.uint64)), name
        assert np.array_equal(got, want), f"{name}: {_first_difference(got, want)}"
        n = len(pts)
        rays = np.concatenate([pts + (pts - tc.centre_of(i)), tc.centre_of(i) - pts], axis=1)
        st = rng.integers(1, 2 ** 31 - 1, size=(n, 4), dtype=np.uint32)
        absorbed, col, _, _ = rt.hooks.reflection(scene, np.full(n, i), rays, np.full((n, 3), 255, np.uint8), pts, st)
        assert absorbed.all() and np.array_equal(col, want), f"{name} (reflection): {_first_difference(col, want)}"


def test_the_ramps_with_every_source_and_three_constants(rt, orc):
    """(U*255, V*255, const) for all 27 ramp_src combinations against RT_TEXTURE_UV_RAMP, and three constants against Colour: the hook on both."""
    case = next(tc.family_ramps())
    progs = twin_objects(rt, case.objs)
    a, b = rt.Scene.make(case.objs), rt.Scene.make(progs)
    for q in case.queries:
        uv1, c1 = rt.hooks.texture_colour_at(a, q.texture, q.points)
        uv2, c2 = rt.hooks.texture_colour_at(b, q.texture, q.points)
        assert np.array_equal(uv1.view(np.uint64), uv2.view(np.uint64)) and np.array_equal(c1, c2), q.texture
    grids = next(tc.family_grids())  # select(flt(sin(g U) sin(g V), 0), even, odd) against Checkered, next to the lines where the band decides
    twins = twin_objects(rt, grids.objs)
    b, o = rt.Scene.make(twins), orc.OracleScene(grids.objs)
    ids = tc.flatten_hittables(twins)[0]  # (a twin is one record where the original is three: the wearers' ids differ)
    for q in grids.queries:
        _, c1 = rt.hooks.texture_colour_at(b, ids[q.hittable].texture, q.points)
        _, c2 = o.texture_colour_at(q.texture, q.points)
        assert np.array_equal(c1, c2), f"grid {tc.GRIDS[q.hittable]}: {_first_difference(c1, c2)}"


# ---- frames: the oracle behind whole frames, on every route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("passes", [1, 2])
def test_frames_equal_the_oracle_at_every_block_and_pass_count(rt, frame, block, passes):
    """rt_render_frame on one device, fused and in two passes, counting and timed: the oracle's frame of the original scene.  The plan
    reports the program variant (tex word 2) and runs a request for 512 threads at 1024."""
    f = frame
    for counters in (True, False):
        res = f["scene"].render_frame(f["w"], f["h"], f["cam"], seed=9, devices=(0,), counters=counters, options=A.rt_render_options(passes=passes, block_threads=block))
        _same(res, f, (block, passes, counters))
        plan = rt.hooks.last_launch_plan()
        assert plan["in"]["has_tex"] == 2 and plan["out"]["q_tex"] == 2 and plan["out"]["q_block"] == (256 if block == 256 else 1024)
        assert plan["out"]["two_pass"] == (passes == 2)
        if counters:
            assert all(res.stats[0][k] == f["st"][k] for k in ("rays", "prim_tests", "reflections", "samples", "pixels_early"))


def test_a_scene_without_programs_plans_and_runs_what_it_did(rt, frame):
    """The original scene: tex word 1, a request for 512 threads runs at 512, and its frame is still the oracle's."""
    f = frame
    res = f["plain"].render_frame(f["w"], f["h"], f["cam"], seed=9, devices=(0,), options=A.rt_render_options(block_threads=512))
    _same(res, f, "plain")
    plan = rt.hooks.last_launch_plan()
    assert plan["in"]["has_tex"] == 1 and plan["out"]["q_tex"] == 1 and plan["out"]["q_block"] == 512
    # ... and a textured scene whose plans were recorded from the device before any of this: every word, fused and in two passes
    import json
    import os
    import scenes
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")) as fh:
        rows = {r["name"]: r for r in json.load(fh)["rows"]}
    objs, cam, w, h = scenes.all_materials(pixels=60)
    assert (w, h) == (106, 60)
    scene = rt.Scene.make(objs)
    for name, passes in (("allmat_spp24", 0), ("allmat_spp24_passes2", 2)):
        scene.render_frame(w, h, cam, seed=1, devices=(0,), options=A.rt_render_options(passes=passes))
        plan = rt.hooks.last_launch_plan()
        want = rows[name]
        assert {k: plan["in"][k] for k in want["in"] if k != "want_stats"} == {k: v for k, v in want["in"].items() if k != "want_stats"}, name
        assert {k: plan["out"].get(k) for k in want["out"]} == want["out"], (name, plan["out"])


def test_render_rows_after_tune_and_with_the_park_pool_off(rt, frame):
    f = frame
    scene = rt.Scene.make(f["progs"])
    assert scene.tune(f["w"], f["h"], f["cam"], seed=9, device=0)["tuned"] in (0, 1)
    _same(scene.render_rows(f["w"], f["h"], f["cam"], seed=9), f, "tuned")
    for park in (-1, 1, 256):
        _same(f["scene"].render_frame(f["w"], f["h"], f["cam"], seed=9, devices=(0,), options=A.rt_render_options(park_lanes=park)), f, park)


def test_pixel_lists_footprints_and_extensions(rt, frame):
    f = frame
    rows, cols = f["acc"].shape[:2]
    rng = np.random.default_rng(3)
    px = rng.permutation(rows * cols).astype(np.int32)[:700]
    res = f["scene"].renderPixels(f["w"], f["h"], f["cam"], px, seed=9)
    assert np.array_equal(res.accum, f["acc"].reshape(-1, 4)[px]) and np.array_equal(res.rgb, f["rgb"].reshape(-1, 3)[px])
    # an extension: 12 samples continued to the frame's 16 is the frame at 16
    short = dataclasses.replace(f["cam"], SamplesPerPixel=12)
    first = f["scene"].render_rows(f["w"], f["h"], short, seed=9)
    _same(f["scene"].extend_rows(f["w"], f["h"], f["cam"], first.accum, 12, seed=9), f, "extend")
    # footprints have no frame to compare with: the original scene on the same route
    fp = np.zeros((300, 12))
    fp[:, 0:3] = [24.0, 9.0, -2.0]
    fp[:, 3:6] = np.array([0.0, -4.0, 1.0]) + rng.normal(size=(300, 3)) * 0.5
    fp[:, 6] = 0.01
    fp[:, 10] = 0.01
    a = f["plain"].renderFootprints(fp, 16, 6, seed=4)
    b = f["scene"].renderFootprints(fp, 16, 6, seed=4)
    assert np.array_equal(a.accum, b.accum) and np.array_equal(a.rgb, b.rgb) and int((a.accum[:, 0] > 0).sum()) == 300


@pytest.mark.parametrize("padding", [900, 17000])
def test_frames_lists_and_jobs_of_a_scene_beyond_the_lds(rt, frame, padding):
    """The divergence scene padded out of the LDS (hybrid and global placements; 16-bit and full-width queue entries): frames fused and in
    two passes at both block sizes, counting and timed, a pixel list, an extension and a budgeted job then finished -- against the padded
    ORIGINAL scene's frame (the field is far from the camera's view, but its spheres are in the tree every ray walks)."""
    f = frame
    field = _plain_field(padding, seed=padding)
    a, b = rt.Scene.make(f["objs"] + field), rt.Scene.make(f["progs"] + field)
    assert b.info()["lds_resident"] == 0
    want = a.render_rows(f["w"], f["h"], f["cam"], seed=9)
    for passes in (1, 2):
        for block in (256, 1024):
            for counters in (False, True):
                res = b.render_frame(f["w"], f["h"], f["cam"], seed=9, devices=(0,), counters=counters, options=A.rt_render_options(passes=passes, block_threads=block))
                assert np.array_equal(res.accum, want.accum) and np.array_equal(res.rgb, want.rgb), (padding, passes, block, counters)
                out = rt.hooks.last_launch_plan()["out"]
                assert out["q_tex"] == 2 and out["q_lds"] == 0 and out["q_block"] == block
    px = np.random.default_rng(4).permutation(want.accum.shape[0] * want.accum.shape[1]).astype(np.int32)[:500]
    res = b.renderPixels(f["w"], f["h"], f["cam"], px, seed=9)
    assert np.array_equal(res.accum, want.accum.reshape(-1, 4)[px])
    first = b.render_rows(f["w"], f["h"], dataclasses.replace(f["cam"], SamplesPerPixel=12), seed=9)
    assert np.array_equal(b.extend_rows(f["w"], f["h"], f["cam"], first.accum, 12, seed=9).accum, want.accum)
    for passes, limits, block in ((1, (3, -1), 256), (2, (2, 40), 1024)):
        rt._lib.check(rt.lib.rt_dev_set_job_limits(*limits))
        try:
            with b.render_job(f["w"], f["h"], f["cam"], seed=9, options=A.rt_render_options(passes=passes, block_threads=block)) as job:
                assert not job.wait()["complete"]
                rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))
                job.finish()
                assert np.array_equal(job.accum, want.accum) and np.array_equal(job.rgb, want.rgb), (padding, passes)
        finally:
            rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))


@pytest.mark.parametrize("padding", [0, 900, 17000])
def test_traced_rays_and_path_records_at_every_residency(rt, frame, padding):
    """rt_trace_rays (timed and counting) and rt_camera_paths' colours: the program scene against the original, LDS-resident and padded to
    the hybrid and global placements (16-bit and full-width queue entries)."""
    f = frame
    field = _plain_field(padding, seed=padding) if padding else []
    a, b = (f["plain"], f["scene"]) if not padding else (rt.Scene.make(f["objs"] + field), rt.Scene.make(f["progs"] + field))
    assert b.info()["lds_resident"] == (1 if not padding else 0)
    rng = np.random.default_rng(8)
    rays = np.zeros((3000, 6))
    rays[:, 0:3] = [24.0, 9.0, -2.0]
    rays[:, 3:6] = np.array([0.0, -4.0, 1.0]) + rng.normal(size=(3000, 3)) * 0.7
    st = rng.integers(1, 2 ** 31 - 1, size=(3000, 4), dtype=np.uint32)
    want, g = a.traceRays(rays, 6, rng=st)
    try:
        for counters in (False, True):
            for block in (256, 512):  # (512: runs at 1024)
                rt.set_launch_config(block_threads=block)
                got, g1 = b.traceRays(rays, 6, rng=st, counters=counters)
                assert np.array_equal(got, want) and np.array_equal(g1, g), (padding, counters, block, _first_difference(got, want))
                assert rt.hooks.last_launch_plan()["out"]["q_block"] == (256 if block == 256 else 1024) and rt.hooks.last_launch_plan()["out"]["q_tex"] == 2
    finally:
        rt.set_launch_config()
    pa = a.cameraPaths(f["w"], f["h"], f["cam"], n=400, n_samples=3, seed=9, records=False, first_ray=False)
    try:
        for counters in (False, True):
            for block in (256, 512, 0):
                rt.set_launch_config(block_threads=block)
                pb = b.cameraPaths(f["w"], f["h"], f["cam"], n=400, n_samples=3, seed=9, records=False, first_ray=False, counters=counters)
                assert np.array_equal(pa.colour, pb.colour) and np.array_equal(pa.n_vertices, pb.n_vertices), (padding, counters, block)
                assert rt.hooks.last_paths_plan()["textured"] == 2 and rt.hooks.last_paths_plan()["block"] == (256 if block == 256 else 1024)
    finally:
        rt.set_launch_config()


def test_a_job_stopped_by_its_budget_and_then_finished(rt, frame):
    """A render job of the program scene with a budget in mid-frame (fused and two passes), then finished: the oracle's frame."""
    f = frame
    for passes, limits, block in ((1, (3, -1), 0), (2, (2, 40), 0), (1, (3, -1), 256), (2, (2, 40), 512)):
        rt._lib.check(rt.lib.rt_dev_set_job_limits(*limits))
        try:
            with f["scene"].render_job(f["w"], f["h"], f["cam"], seed=9, options=A.rt_render_options(passes=passes, block_threads=block)) as job:
                res = job.wait()
                assert not res["complete"] and 0 < res["n_present"] < res["pixels_total"]
                present = job.present.astype(bool)
                assert np.array_equal(job.accum[present], f["acc"][present])
                rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))
                job.finish()
                assert np.array_equal(job.accum, f["acc"]) and np.array_equal(job.rgb, f["rgb"]), passes
        finally:
            rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))


def test_scenes_made_on_the_device_routes(rt, frame):
    """Scene.make_device (rt_scene_create_device: records resident, the host's texture half) and a scene with an image placed from device
    memory beside the programs (rt_scene_create_textures, sources RECORD for the programs): the same frame."""
    import torch
    f = frame
    recs, table = rt.hittable_records(f["progs"], textures=True)
    scene = rt.Scene.make_device(recs, table, device=0)
    _same(scene.render_rows(f["w"], f["h"], f["cam"], seed=9), f, "make_device")
    # the wearers' images from device memory: texture_cases' images are img.[y] rows; ofImageDevice takes the bitmap, top first
    def on_device(p):
        PT = rt.ParameterisedTexture
        if p.kind == A.RT_TEXTURE_IMAGE:
            return PT.ofImageDevice(torch.from_numpy(np.ascontiguousarray(p.image[::-1])).cuda())
        if p.kind == A.RT_TEXTURE_CHECKERED:
            return PT.Checkered(on_device(p.even), on_device(p.odd), p.grid)
        return p
    objs = []
    for o in f["progs"]:
        t = o.sphere.Style.texture
        if t is not None and t.param is not None:
            o = dataclasses.replace(o, sphere=dataclasses.replace(o.sphere, Style=dataclasses.replace(o.sphere.Style, texture=dataclasses.replace(t, param=on_device(t.param)))))
        objs.append(o)
    scene = rt.Scene.make(objs)
    assert rt.hooks.texture_plan()["device_sourced"] > 0
    _same(scene.render_rows(f["w"], f["h"], f["cam"], seed=9), f, "device textures")
    # set_texels_device on a program record of a scene that is on the device: refused, the scene untouched
    idx = next(i for i in range(table.count) if table.records[i].kind == A.RT_TEXTURE_PROGRAM)
    bitmap = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    assert rt.lib.rt_scene_set_texels_device(f["scene"].handle, idx, 0, bitmap.data_ptr(), 48, 1, None) == A.RT_ERR_INVALID_ARGUMENT
    _same(f["scene"].render_rows(f["w"], f["h"], f["cam"], seed=9), f, "after the refusal")
    # a DEVICE or JPEG source on a program record, with real device memory behind it: refused, *out untouched, the bitmap unread and unchanged
    import ctypes as C
    S = A.rt_texels_source
    hs = tc.flatten_hittables(f["progs"])[0]
    d_hs = torch.from_numpy(recs.view(np.uint8).reshape(len(recs), -1).copy()).cuda()
    bitmap.fill_(7)
    for kind in (A.RT_TEXELS_DEVICE, A.RT_TEXELS_JPEG):
        src = (S * table.count)(*[S(kind, 0, bitmap.data_ptr(), 48) if i == idx else S() for i in range(table.count)])
        for which in ("textures", "device_textures"):
            out = C.c_void_p(0x1234)
            if which == "textures":
                code = rt.lib.rt_scene_create_textures(hs, len(recs), table.records, table.count, src, None, 0, None, C.byref(out))
            else:
                code = rt.lib.rt_scene_create_device_textures(0, d_hs.data_ptr(), len(recs), table.records, table.count, src, None, None, C.byref(out))
            assert code == A.RT_ERR_INVALID_ARGUMENT and out.value == 0x1234, (kind, which)
            assert (rt.lib.rt_last_error() or b"").decode() == f"source {idx}: a program's bytes come from the record (RT_TEXELS_RECORD)"
    assert bool((bitmap == 7).all())
    _same(f["scene"].render_rows(f["w"], f["h"], f["cam"], seed=9), f, "after the refusals")


# ---- frames of programs that no existing kind expresses: tests/fsharp_literal.py's, recorded (tests/golden/make_texprog_cases.py) -------------
@pytest.fixture(scope="module")
def literal_cases(rt):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_texprog_cases as G  # (the scenes; the literal and mpmath are only needed to generate)
    recorded = np.load(G.PATH)
    return G, {name: (objs, cam, recorded[name]) for name, (objs, cam) in G.cases().items()}


@pytest.mark.parametrize("name", [f"row{k}" for k in range(6)])
def test_recorded_literal_frames_on_every_route(rt, literal_cases, name):
    """9 x 7 px, 12 samples, depth 6; strike-point inputs, DIV, SQRT, FLOOR, MIN / MAX, LT / LE, wrapping bytes, the 64-instruction and the
    depth-8 program, below a Checkered and as roots, on every style: rt_render fused and in two passes at blocks 256, 512 (runs at 1024)
    and 1024, counting and timed; after rt_scene_tune; a scene from rt_scene_create_device; rt_render_pixels; rt_camera_paths' colours
    summed per pixel; a budgeted job then finished.  (An extension needs 12 samples done and these frames have 12: the equivalence
    scene covers rt_render_extend.)"""
    G, cases = literal_cases
    objs, cam, want = cases[name]
    w, h = G.MAX_W, G.MAX_H
    scene = rt.Scene.make(objs)
    for passes in (1, 2):
        for block in (256, 512, 1024):
            for counters in (False, True):
                res = scene.render_frame(w, h, cam, seed=G.SEED, devices=(0,), counters=counters, options=A.rt_render_options(passes=passes, block_threads=block))
                assert np.array_equal(res.accum, want), (name, passes, block, counters, int((res.accum != want).any(-1).sum()))
                assert rt.hooks.last_launch_plan()["out"]["q_tex"] == 2
    tuned = rt.Scene.make(objs)
    tuned.tune(w, h, cam, seed=G.SEED, device=0)
    assert np.array_equal(tuned.render_rows(w, h, cam, seed=G.SEED).accum, want), (name, "tuned")
    recs, table = rt.hittable_records(objs, textures=True)
    assert np.array_equal(rt.Scene.make_device(recs, table, device=0).render_rows(w, h, cam, seed=G.SEED).accum, want), (name, "make_device")
    px = np.arange(want.shape[0] * want.shape[1], dtype=np.int32)[::-1].copy()
    assert np.array_equal(scene.renderPixels(w, h, cam, px, seed=G.SEED).accum, want.reshape(-1, 4)[px]), (name, "pixels")
    # the path behind every sample: a pixel's sums are the colours of its first Count samples
    paths = scene.cameraPaths(w, h, cam, n=len(px), n_samples=G.SPP, seed=G.SEED, records=False, first_ray=False)
    col = np.asarray(paths.colour).reshape(len(px), G.SPP, 3).astype(np.int64)
    flat = want.reshape(-1, 4)
    sums = np.array([col[i, : flat[i, 0]].sum(axis=0) for i in range(len(px))])
    assert np.array_equal(sums, flat[:, 1:]), (name, "paths")
    rt._lib.check(rt.lib.rt_dev_set_job_limits(2, -1))
    try:
        with scene.render_job(w, h, cam, seed=G.SEED, options=A.rt_render_options(passes=1, chunk_pixels=8)) as job:
            res = job.wait()
            assert not res["complete"] and 0 < res["n_present"] < res["pixels_total"]
            present = job.present.astype(bool)
            assert np.array_equal(job.accum[present], want[present])
            rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))
            job.finish()
            assert np.array_equal(job.accum, want), (name, "job")
    finally:
        rt._lib.check(rt.lib.rt_dev_set_job_limits(-1, -1))
