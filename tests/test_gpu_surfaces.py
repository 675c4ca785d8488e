"""Scene.surfaces / Scene.cameraSurfaces -- rt_surfaces, rt_camera_surfaces, their device variants, surface_kernel -- against the answer
composed from the oracle's pieces (tests/surface_cases.py; itself held to the literal restatement and to its seeded mutants by
tests/test_surface_cases.py), bit for bit, NaNs by position; never against the library's own shading.  Witness vertices at the edges of
Hittable.Reflection's decisions, slot counts around a wave and a tile with the textured slots placed where the per-tile list can go
wrong, every output alone, no-surface slots, duplicates, malformed lists, the device entry on streams, scenes made on the device and
tuned, texture programs, camera frames, and the C consumer.  One cross-check against the library itself, labelled as such."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import camera_hit_cases as chc
import reflection_cases as rc
import scenes
import surface_cases as sc
import texture_cases
from test_surface_cases import CLASSES, SEED, build_surfaces_smoke, frame, frame_surfaces, raw_roots, witness

pytestmark = pytest.mark.gpu

FIELDS = ("normal", "inside", "colour", "tint", "uv")
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def _np(a):
    return None if a is None else (a if isinstance(a, np.ndarray) else a.cpu().numpy())


def _assert_surfaces(got, want, what=(), rows=None):
    """Every output `got` holds against the composer's (rows: the composer's slots the call was made of)."""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    for f in FIELDS:
        g = _np(getattr(got, f))
        if g is None:
            continue
        w = pick(getattr(want, f)).reshape(g.shape)
        if f in ("normal", "uv"):
            assert sc.same_f64(g, w), (what, f, np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))).reshape(len(w.reshape(-1, g.shape[-1])), -1).all(axis=1))[:8])
        else:
            assert np.array_equal(g, w), (what, f, np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[:8])


_CACHE = {}


def _vertices(orc, kind, cluster=False):
    """The witness, its product scene and the composer's answer over the five vertex classes, computed once and never written."""
    key = (kind, cluster)
    if key not in _CACHE:
        objs, osc, table = witness(orc, kind, cluster)
        v = rc.concat([rc.vertices(orc, cls).spread(2000) for cls in CLASSES])
        want = sc.compose(orc, osc, table, v.idx, v.strike, v.rays)
        _CACHE[key] = (rc.rt.Scene.make(objs), v, want)
    return _CACHE[key]


# ---- 1: witness vertices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cluster", [("tex", False), ("planes", False), ("planes", True)])
def test_surfaces_on_witness_vertices(rt, orc, kind, cluster):
    scene, v, want = _vertices(orc, kind, cluster)
    assert len(v) >= 5000
    if cluster:  # the 1000 bounded spheres reorder the object table: orig_to_obj is not the identity
        assert scene.info()["n_bounded"] >= 1000
    got = scene.surfaces(v.idx, v.strike, v.rays, uv=True)
    _assert_surfaces(got, want, (kind, cluster))
    st, plan = got.stats, rt.hooks.last_surface_plan()
    assert st["samples"] == len(v) and st["rays"] == st["pixels"] == st["reflections"] == 0 and st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
    assert plan["slots"] == len(v) and plan["tile"] == 1024 and plan["block"] == 256 and plan["grid"] == -(-len(v) // 1024) and plan["program"] == 0
    assert plan["texture_phase"] == int(kind == "tex") and plan["textured"] == int(want.textured.sum())
    assert (want.textured.sum() > 200) == (kind == "tex")
    again = scene.surfaces(v.idx, v.strike, v.rays, uv=True, counters=True)  # RT_RENDER_COUNTERS is accepted and changes nothing
    _assert_surfaces(again, want, (kind, cluster, "counters"))
    assert again.stats["rays"] == 0 and again.stats["samples"] == len(v)


# ---- 2: slot counts around a wave and a tile ---------------------------------------------------------------------------------------------
def test_slot_counts_around_a_wave_and_a_tile(rt, orc):
    scene, v, want = _vertices(orc, "tex")
    tex, plain = np.flatnonzero(want.textured), np.flatnonzero(~want.textured)
    assert len(tex) >= 500 and len(plain) >= 2049  # (the pools are drawn from with repetition)
    rng = np.random.default_rng(8)
    for n in COUNTS:
        last = (n - 1) // 1024 * 1024  # where the last (partial) tile begins
        patterns = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "one": np.zeros(n, bool), "last_tile": np.arange(n) >= last}
        patterns["one"][int(rng.integers(0, min(n, 1024)))] = True
        for name, textured in patterns.items():
            rows = np.where(textured, tex[rng.integers(0, len(tex), n)], plain[rng.integers(0, len(plain), n)])
            got = scene.surfaces(v.idx[rows], v.strike[rows], v.rays[rows], uv=True)
            _assert_surfaces(got, want, (n, name), rows)
            plan = rt.hooks.last_surface_plan()
            assert plan["slots"] == n and plan["grid"] == -(-n // 1024) and plan["textured"] == int(textured.sum()), (n, name)


# ---- 3: outputs -----------------------------------------------------------------------------------------------------------------------
def test_every_output_alone_and_null_outputs_stay_untouched(rt, orc):
    import torch
    scene, v, want = _vertices(orc, "tex")
    rows = np.arange(0, len(v), 3)
    n = len(rows)
    A = rt._abi
    dev = torch.device("cuda", 0)
    hit, strike, rays = (torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev) for a in (v.idx, v.strike, v.rays))
    shapes = {"normal": ((n, 3), torch.float64), "inside": ((n,), torch.uint8), "colour": ((n, 3), torch.uint8), "tint": ((n, 3), torch.uint8),
              "uv": ((n, 2), torch.float64)}
    for asked in [(f,) for f in FIELDS] + [("normal", "inside"), FIELDS]:
        bufs = {f: torch.full(shape, 77, dtype=dt, device=dev) for f, (shape, dt) in shapes.items()}
        out = A.rt_surface_outputs(**{f: bufs[f].data_ptr() for f in asked})
        st = A.rt_stats()
        rc_ = rt.lib.rt_surfaces_device(scene.handle, 0, n, hit.data_ptr(), strike.data_ptr(), rays.data_ptr(), 0, C.byref(out),
                                        torch.cuda.current_stream(dev).cuda_stream, None, C.byref(st))
        assert rc_ == A.RT_OK, rt.lib.rt_last_error()
        got = rt.Surfaces(**{f: (bufs[f] if f in asked else None) for f in FIELDS}, stats=None)
        _assert_surfaces(got, want, asked, rows)
        for f in FIELDS:
            if f not in asked:
                assert bool((bufs[f] == 77).all()), (asked, f)  # a NULL output's buffer is not written
        plan = rt.hooks.last_surface_plan()
        wants_tex = bool(set(asked) & {"colour", "tint", "uv"})
        assert plan["texture_phase"] == int(wants_tex), asked  # normal / inside alone never evaluate a texture
        assert plan["textured"] == (int(want.textured[rows].sum()) if wants_tex else 0), asked
    # ... and through the wrapper: fields not asked for are None
    got = scene.surfaces(v.idx[rows], v.strike[rows], v.rays[rows], colour=False, tint=False)
    assert got.colour is None and got.tint is None and got.uv is None
    _assert_surfaces(got, want, "wrapper", rows)
    assert rt.hooks.last_surface_plan()["texture_phase"] == 0


# ---- 4: slot contents -------------------------------------------------------------------------------------------------------------------
def test_no_surface_slots_and_duplicates(rt, orc):
    scene, v, want = _vertices(orc, "tex")
    objs, osc, table = witness(orc, "tex")
    rng = np.random.default_rng(12)
    rows = rng.integers(0, len(v), 700)
    rows[100:140] = rows[95]  # duplicates: every store is indexed by slot
    hit, strike, rays = v.idx[rows].copy(), v.strike[rows].copy(), v.rays[rows].copy()
    hit[0:20] = -1
    hit[20:40] = -2
    strike[40:50, 0] = np.nan
    strike[50:60, 2] = np.inf
    rays[60:70, 1] = -np.inf
    rays[70:80, 0] = np.nan
    rays[80:90, 4] = np.nan  # (a direction is never read)
    expect = sc.compose(orc, osc, table, hit, strike, rays)
    assert np.isnan(expect.normal[:80]).all() and not expect.colour[:80].any() and not np.isnan(expect.normal[80:90]).any()
    got = scene.surfaces(hit, strike, rays, uv=True)
    _assert_surfaces(got, expect, "no-surface")
    for f in FIELDS:
        assert np.array_equal(getattr(got, f)[100:140], np.broadcast_to(getattr(got, f)[95], getattr(got, f)[100:140].shape), equal_nan=f in ("normal", "uv"))
    # the scene made by hand: COLOUR roots (the record's Pixel, no uv) and emitters whose albedo is not 1 (never darkened)
    arrays, rosc, rtable, rhit, rstrike, rrays = raw_roots(orc)
    rscene, _ = scenes.raw_scene_pair(None, *arrays)
    _assert_surfaces(rscene.surfaces(rhit, rstrike, rrays, uv=True), sc.compose(orc, rosc, rtable, rhit, rstrike, rrays), "raw roots")


# ---- 5: malformed lists -----------------------------------------------------------------------------------------------------------------
def test_a_malformed_list_writes_nothing(rt, orc):
    import torch
    scene, v, want = _vertices(orc, "planes")
    n_obj = len(witness(orc, "planes")[0])
    rows = np.arange(1500)
    dev = torch.device("cuda", 0)
    for entry in (n_obj, -3):
        hit = v.idx[rows].copy()
        hit[1200] = entry
        with pytest.raises(rt.RtError) as e:  # the host variant refuses it on the host
            scene.surfaces(hit, v.strike[rows], v.rays[rows])
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT
        t_hit, t_strike, t_rays = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (hit, v.strike[rows], v.rays[rows]))
        A = rt._abi
        for with_stats in (True, False):
            bufs = {"normal": torch.full((1500, 3), 7.5, dtype=torch.float64, device=dev), "inside": torch.full((1500,), 77, dtype=torch.uint8, device=dev),
                    "colour": torch.full((1500, 3), 77, dtype=torch.uint8, device=dev), "tint": torch.full((1500, 3), 77, dtype=torch.uint8, device=dev)}
            out = A.rt_surface_outputs(**{f: b.data_ptr() for f, b in bufs.items()})
            st = A.rt_stats()
            got = rt.lib.rt_surfaces_device(scene.handle, 0, 1500, t_hit.data_ptr(), t_strike.data_ptr(), t_rays.data_ptr(), 0, C.byref(out),
                                            torch.cuda.current_stream(dev).cuda_stream, None, C.byref(st) if with_stats else None)
            assert got == (A.RT_ERR_INVALID_ARGUMENT if with_stats else A.RT_OK), (entry, with_stats)
            torch.cuda.synchronize(dev)
            assert bool((bufs["normal"] == 7.5).all()) and all(bool((bufs[f] == 77).all()) for f in ("inside", "colour", "tint")), (entry, with_stats)
    # the same list, mended, is answered
    _assert_surfaces(scene.surfaces(v.idx[rows], v.strike[rows], v.rays[rows]), want, "mended", rows)


# ---- 6: the device entry ------------------------------------------------------------------------------------------------------------------
def test_tensors_streams_and_no_stats(rt, orc):
    import torch
    scene, v, want = _vertices(orc, "tex")
    dev = torch.device("cuda", 0)
    rows = np.arange(0, len(v), 2)
    t = [torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev) for a in (v.idx, v.strike, v.rays)]
    got = scene.surfaces(*t, uv=True)
    assert all(getattr(got, f).is_cuda for f in FIELDS) and got.stats["samples"] == len(rows)
    _assert_surfaces(got, want, "tensors", rows)
    got = scene.surfaces(*t, uv=True, stats=False)  # returns after the launch
    assert got.stats is None and scene.last_stats is None and rt.hooks.last_surface_plan()["textured"] == -1
    torch.cuda.synchronize(dev)
    _assert_surfaces(got, want, "no stats", rows)
    # two streams in flight, each with its own slots
    halves = [rows[: len(rows) // 2], rows[len(rows) // 2:]]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    results = []
    for s, part in zip(streams, halves):
        with torch.cuda.stream(s):
            tt = [torch.from_numpy(np.ascontiguousarray(a[part])).to(dev, non_blocking=False) for a in (v.idx, v.strike, v.rays)]
            results.append((tt, [scene.surfaces(*tt, uv=True, stats=False) for _ in range(3)]))
    for s in streams:
        s.synchronize()
    for (_, outs), part in zip(results, halves):
        for o in outs:
            _assert_surfaces(o, want, "streams", part)
    assert torch.cuda.current_device() == 0


# ---- 7: scene routes --------------------------------------------------------------------------------------------------------------------
def test_a_scene_made_on_the_device_and_a_tuned_scene(rt, orc):
    objs, osc, table = witness(orc, "planes", True)
    _, v, want = _vertices(orc, "planes", True)
    rows = np.arange(0, len(v), 2)
    made = rt.Scene.make_device(rt.hittable_records(objs))
    _assert_surfaces(made.surfaces(v.idx[rows], v.strike[rows], v.rays[rows]), want, "make_device", rows)
    # after tune: the image is rebuilt, the object table stays -- the same answers as before it
    fobjs, cam, w, h, fosc, ftable, hits = frame(orc, "all_materials")
    big = rc.witness("tex", True)
    scene = rt.Scene.make(big)
    _, tv, twant = _vertices(orc, "tex")
    trows = np.arange(0, len(tv), 2)
    before = scene.surfaces(tv.idx[trows], tv.strike[trows], tv.rays[trows], uv=True)
    _assert_surfaces(before, twant, "before tune", trows)
    eye = rt.Point.make(9045.0, 9045.0, 8900.0)
    tcam = rt.Camera.makeBasic(20, 1.0, 1.5, eye, rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    info = scene.tune(12, 8, tcam, seed=1, device=0)
    after = scene.surfaces(tv.idx[trows], tv.strike[trows], tv.rays[trows], uv=True)
    _assert_surfaces(after, twant, ("after tune", info["tuned"]), trows)


# ---- 8: texture programs -------------------------------------------------------------------------------------------------------------------
def test_a_program_scene_equals_the_original(rt, orc):
    from test_gpu_texprog import twin_objects
    objs, cam, w, h, osc, table, hits = frame(orc, "mostly_textured")
    want = frame_surfaces(orc, "mostly_textured")
    scene = rt.Scene.make(twin_objects(rt, objs))
    got_hits, got = scene.cameraSurfaces(w, h, cam, seed=SEED, uv=True)
    assert np.array_equal(got_hits.hit_index, hits.hit) and chc.same_f64(got_hits.strike, hits.strike)
    _assert_surfaces(got, want, "programs")
    plan = rt.hooks.last_surface_plan()
    assert plan["program"] == 1 and plan["texture_phase"] == 1 and plan["textured"] == 1653
    flat = scene.surfaces(hits.hit.reshape(-1), hits.strike.reshape(-1, 3), hits.rays.reshape(-1, 6), uv=True)
    _assert_surfaces(flat, want, "programs, list")
    assert rt.hooks.last_surface_plan()["program"] == 1


# ---- 9: camera surfaces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_materials", "mostly_textured", "earth_thumb", "lights"])
def test_camera_surfaces_on_a_frame(rt, orc, name):
    objs, cam, w, h, osc, table, hits = frame(orc, name)
    want = frame_surfaces(orc, name)
    scene = rt.Scene.make(objs)
    n = (2 * w + 1) * (2 * h + 1)
    for counters in (False, True):  # both camera-hit kernel variants
        got_hits, got = scene.cameraSurfaces(w, h, cam, seed=SEED, uv=True, counters=counters)
        assert np.array_equal(got_hits.hit_index, hits.hit) and chc.same_f64(got_hits.strike, hits.strike) and got_hits.rays is None, (name, counters)
        _assert_surfaces(got, want, (name, counters))
        st = got.stats
        assert st["pixels"] == n and st["samples"] == n and st["reflections"] == 0 and st["rays"] == (n if counters else 0)
        assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
        plan = rt.hooks.last_surface_plan()
        assert plan["slots"] == n and plan["textured"] == int(want.textured.sum())
        assert rt.hooks.last_launch_plan()["out"]["q_mode"] == 14 and rt.hooks.last_launch_plan()["out"]["q_count"] == int(counters)
    # hit_index / strike not asked for: the records do not change
    got_hits, got = scene.cameraSurfaces(w, h, cam, seed=SEED, uv=True, hit_index=False, strike=False)
    assert got_hits.hit_index is None and got_hits.strike is None
    _assert_surfaces(got, want, (name, "no hits"))
    got_hits, got = scene.cameraSurfaces(w, h, cam, seed=SEED, strike=False, normal=False, inside=False)
    assert np.array_equal(got_hits.hit_index, hits.hit)
    _assert_surfaces(got, want, (name, "no strike"))


def test_camera_surfaces_sample_ranges_lists_and_tensors(rt, orc):
    import torch
    objs, cam, w, h, osc, table, _ = frame(orc, "all_materials")
    scene = rt.Scene.make(objs)
    cols, n = 2 * w + 1, (2 * w + 1) * (2 * h + 1)
    rng = np.random.default_rng(4)
    px = rng.permutation(np.arange(0, n, 13)).astype(np.int32)
    px = np.concatenate([px, px[:9]])  # in any order, with duplicates
    hits = chc.compose(orc, osc, cam.to_abi(), w, h, SEED, px, 0, 3)
    want = sc.compose(orc, osc, table, hits.hit.reshape(-1), hits.strike.reshape(-1, 3), hits.rays.reshape(-1, 6))
    assert want.textured.sum() > 0 and want.inside.sum() > 0
    got_hits, got = scene.cameraSurfaces(w, h, cam, px, sample_first=0, n_samples=3, seed=SEED, uv=True)
    assert got.normal.shape == (len(px), 3, 3) and got.inside.shape == (len(px), 3)
    assert np.array_equal(got_hits.hit_index, hits.hit) and chc.same_f64(got_hits.strike, hits.strike)
    _assert_surfaces(got, want, "list")
    t_hits, t_got = scene.cameraSurfaces(w, h, cam, torch.from_numpy(px).to("cuda:0"), sample_first=0, n_samples=3, seed=SEED, uv=True)
    assert t_got.normal.is_cuda and np.array_equal(_np(t_hits.hit_index), hits.hit)
    _assert_surfaces(t_got, want, "tensor list")
    t_hits, t_got = scene.cameraSurfaces(w, h, cam, torch.from_numpy(px).to("cuda:0"), sample_first=0, n_samples=3, seed=SEED, uv=True, stats=False, hit_index=False)
    torch.cuda.synchronize()
    assert t_got.stats is None and t_hits.hit_index is None
    _assert_surfaces(t_got, want, "tensor list, no stats")
    # a device list with an entry outside the frame: nothing is written, and the statistics say so
    bad = px.copy()
    bad[5] = n
    with pytest.raises(rt.RtError) as e:
        scene.cameraSurfaces(w, h, cam, torch.from_numpy(bad).to("cuda:0"), n_samples=3, seed=SEED)
    assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT


def test_the_c_consumer_renders_a_frames_normals_and_colours(rt, orc, tmp_path):
    out = subprocess.run([build_surfaces_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "surfaces: 117 slots answered on the GPU" in out.stdout
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("slot ")]
    assert len(lines) == 117
    P, S, PS, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.InfinitePlaneStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    objs = [H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0)),
            H.Sphere(rt.Sphere.make(S.Glass(1.0, Tex(Px(255, 255, 255)), 1.5), P(1.5, 0.0, 4.0), 0.7)),
            H.InfinitePlane(rt.InfinitePlane.make(PS.FuzzedReflection(0.9, Px(180, 200, 220), 0.2), P(0.0, -1.0, 0.0), rt.Vector.unitise(rt.Vector.make(0.0, 1.0, 0.0)))),
            H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(230, 230, 255))), P(0.0, 0.0, 0.0), 100.0))]
    cam = rt.Camera.makeBasic(24, 1.0, 13.0 / 9.0, P(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    osc = orc.OracleScene(objs)
    hits = chc.compose(orc, osc, cam.to_abi(), 6, 4, 5, np.arange(117), 0, 1)
    want = sc.compose(orc, osc, sc.SceneTable(objs), hits.hit.reshape(-1), hits.strike.reshape(-1, 3), hits.rays.reshape(-1, 6))
    f64 = lambda words: np.array([int(x, 16) for x in words], np.uint64).view(np.float64)  # noqa: E731
    for i, ln in enumerate(lines):
        assert int(ln[1]) == i and int(ln[2]) == hits.hit[i, 0]
        assert chc.same_f64(f64(ln[3:6]), hits.strike[i, 0]) and sc.same_f64(f64(ln[6:9]), want.normal[i])
        nums = [int(x) for x in ln[9:16]]
        assert nums[0] == want.inside[i] and nums[1:4] == want.colour[i].tolist() and nums[4:7] == want.tint[i].tolist(), i
    assert len({int(ln[2]) for ln in lines}) >= 3


# ---- 10: one cross-check against the library itself (NOT the witness) ----------------------------------------------------------------------
def test_cross_check_tint_is_the_first_vertex_of_the_librarys_own_paths(rt, orc):
    objs, cam, w, h, _, _, hits = frame(orc, "all_materials")
    scene = rt.Scene.make(objs)
    _, got = scene.cameraSurfaces(w, h, cam, seed=SEED)
    paths = scene.cameraPaths(w, h, cam, seed=SEED, max_vertices=1, first_ray=False)
    assert np.array_equal(paths.hit_index[..., 0], hits.hit)
    assert np.array_equal(got.tint, paths.colour_after[..., 0, :])
