"""Scene.renderFootprints -- Scene.renderPixel for caller-defined cameras, the render kernel's footprint modes -- against the
composition of footprint_cases.compose (stream state, GetTwo, the footprint's vector, Ray.make', the oracle's traceRay, renderPixel's
rule in integers), bit for bit: every sample count around the adaptive rule's edges, LDS-resident, global-memory and textured
scenes, both kernel variants, every launch setting, list sizes around a unit, slices, a degenerate footprint, the statistics and
the device entry on streams."""
import ctypes as C
import functools

import numpy as np
import pytest

import footprint_cases as fc
import scenes

pytestmark = pytest.mark.gpu

DEPTH = 12
SEED = 5
SPPS = (1, 2, 3, 9, 10, 11, 12, 40)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(objects, footprints): about 130-143 pixels, two full 64-pixel units and a ragged one."""
    if name == "all_materials":
        return scenes.all_materials()[0], fc.equirect(13, 10, (0.0, 0.3, -1.0))
    if name == "many_spheres":  # not LDS-resident
        return scenes.many_spheres(n=2600)[0], fc.equirect(13, 10, (0.0, 1.0, 0.0))
    objs, cam, _, _ = scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])  # textured; its own camera (a panorama from its
    return objs, fc.pinhole(cam, 6, 5)                                          # eye stops early at every pixel)


@functools.lru_cache(maxsize=None)
def _scene(rt, name, walk_tree=None):
    return rt.Scene.make(_case(name)[0], walk_tree=walk_tree)


@functools.lru_cache(maxsize=None)
def _oracle(orc, name):
    return orc.OracleScene(_case(name)[0])


@functools.lru_cache(maxsize=None)
def _expected(orc, name, spp):
    return fc.compose(orc, _oracle(orc, name), _case(name)[1], spp, DEPTH, SEED)


@pytest.mark.parametrize("name", ["all_materials", "many_spheres", "earth"])
def test_equals_the_composition(rt, orc, name):
    fp = _case(name)[1]
    s = _scene(rt, name)
    assert 130 <= len(fp) <= 143
    assert s.info()["lds_resident"] == (0 if name == "many_spheres" else 1)
    for spp in SPPS:
        want = _expected(orc, name, spp)
        if spp == 40:  # both branches of the decision are exercised (a condition on the EXPECTED values)
            early, full = int(want.early.sum()), int((want.accum[:, 0] == 40).sum())
            print(f"{name}: {early} pixels stop early, {full} run all samples, of {len(fp)}")
            assert early >= 0.05 * len(fp) and full >= 0.05 * len(fp)
        for counters in (False, True):
            got = s.renderFootprints(fp, spp, DEPTH, seed=SEED, counters=counters)
            assert np.array_equal(got.accum, want.accum), (name, spp, counters)
            assert np.array_equal(got.rgb, want.rgb), (name, spp, counters)


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_launch_settings_do_not_change_results(rt, name):
    torch = pytest.importorskip("torch")
    A = rt._abi
    s = _scene(rt, name)
    fp = torch.from_numpy(fc.equirect(64, 32, _case(name)[1][0, :3])).cuda()  # 2048 pixels: two-pass has a list to order
    base = s.renderFootprints(fp, 40, DEPTH, seed=SEED)
    plan = rt.hooks.last_launch_plan()
    assert plan["in"]["kind"] == 3 and plan["in"]["n"] == 2048 and plan["in"]["spp"] == 40
    assert 0 < int((base.accum[:, 0] == 40).sum().item()) < 2048
    for opt in (dict(passes=1), dict(passes=2), dict(block_threads=256), dict(block_threads=1024), dict(chunk_pixels=1),
                dict(chunk_pixels=16), dict(chunk_pixels=64), dict(park_lanes=-1), dict(passes=2, block_threads=256, chunk_pixels=64)):
        for counters in (False, True):
            got = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters, options=A.rt_render_options(**opt))
            assert torch.equal(got.accum, base.accum) and torch.equal(got.rgb, base.rgb), (name, opt, counters)
            plan = rt.hooks.last_launch_plan()
            assert plan["in"]["kind"] == 3
            if "passes" in opt:
                assert plan["out"]["two_pass"] == (1 if opt["passes"] == 2 else 0)
                assert plan["out"]["q_mode"] == 6 and (opt["passes"] == 1 or (plan["out"]["A_mode"], plan["out"]["B_mode"]) == (7, 8))
            assert got.stats["pixels"] == 2048 and got.stats["samples"] == int(base.accum[:, 0].sum().item())


def test_sizes_and_a_large_list(rt, orc):
    s, o = _scene(rt, "all_materials"), _oracle(orc, "all_materials")
    fp = _case("all_materials")[1]
    for n in (1, 63, 64, 65):
        want = fc.compose(orc, o, fp[:n], 12, DEPTH, SEED)
        for counters in (False, True):
            got = s.renderFootprints(fp[:n], 12, DEPTH, seed=SEED, counters=counters)
            assert np.array_equal(got.accum, want.accum) and np.array_equal(got.rgb, want.rgb), (n, counters)
    objs = scenes.small_final()[0]
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    fp = fc.equirect(800, 375, (13.0, 2.0, 3.0))
    n = len(fp)
    assert n == 300000
    got = s.renderFootprints(fp, 3, 50, seed=9)
    assert got.stats["pixels"] == n and got.stats["samples"] == 3 * n
    sub = np.arange(0, n, 601)
    want = fc.compose(orc, o, fp[sub], 3, 50, 9, index=sub)
    assert len(sub) == 500 and np.array_equal(got.accum[sub], want.accum) and np.array_equal(got.rgb[sub], want.rgb)
    assert len(np.unique(want.rgb, axis=0)) > 20


def test_slices_with_stream_base_concatenate_to_the_whole(rt):
    for name in ("all_materials", "many_spheres"):
        s, fp = _scene(rt, name), _case(name)[1]
        whole = s.renderFootprints(fp, 40, DEPTH, seed=SEED, stream_base=1000)
        parts = [s.renderFootprints(fp[a:b], 40, DEPTH, seed=SEED, stream_base=1000 + a) for a, b in ((0, 7), (7, 71), (71, len(fp)))]
        assert np.array_equal(np.concatenate([p.accum for p in parts]), whole.accum)
        assert np.array_equal(np.concatenate([p.rgb for p in parts]), whole.rgb)
        assert sum(p.stats["pixels_early"] for p in parts) == whole.stats["pixels_early"]


def test_a_degenerate_footprint_is_black_and_stops_early(rt, orc):
    s, fp = _scene(rt, "all_materials"), _case("all_materials")[1].copy()
    plain = _expected(orc, "all_materials", 40)
    fp[[0, 70, 129], 3:] = 0.0  # base = du = dv = 0: Ray.make' gives ValueNone at every sample
    fp[33, 3:] = 1e-5           # below the tolerance (|v|^2 < 1e-8) as well
    want = plain.accum.copy()
    want[[0, 33, 70, 129]] = [11, 0, 0, 0]  # 2 * firstTrial + 1 samples, all Black: the two means agree
    for counters in (False, True):
        got = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters)
        assert np.array_equal(got.accum, want)
        assert (got.rgb[[0, 33, 70, 129]] == 0).all()
        assert got.stats["pixels_early"] == int(plain.early.sum()) + int((~plain.early[[0, 33, 70, 129]]).sum())
    # rgb may be NULL
    accum = np.full((len(fp), 4), -1, np.int32)
    rc = rt.lib.rt_render_footprints(s.handle, 0, len(fp), fp.ctypes.data_as(C.POINTER(C.c_double)), 40, DEPTH, SEED, 0, 0,
                                     accum.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    assert rc == rt._abi.RT_OK and np.array_equal(accum, want)


def test_statistics(rt, orc):
    for name in ("all_materials", "many_spheres", "earth"):
        fp = _case(name)[1]
        want = _expected(orc, name, 40)
        s = _scene(rt, name, "reference")
        for counters in (False, True):
            got = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters)
            st = got.stats
            assert st is s.last_stats
            assert st["samples"] == int(want.accum[:, 0].sum()) == int(got.accum[:, 0].sum())
            assert st["pixels"] == len(fp) and st["pixels_early"] == int(want.early.sum())
            assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
        # the counting variant's totals are those of the same rays and advanced generators through rt_trace_rays (whose counting
        # path test_gpu_ray_queries.py holds to the oracle)
        s.traceRays(want.rays, DEPTH, rng=want.states, counters=True)
        for key in ("rays", "aabb_tests", "prim_tests", "reflections"):
            assert st[key] == s.last_stats[key] > 0, (name, key)


def test_device_path_on_streams(rt):
    torch = pytest.importorskip("torch")
    s = _scene(rt, "all_materials")
    eye = _case("all_materials")[1][0, :3]
    lists = [fc.equirect(96, 48, eye), fc.equirect(64, 40, eye)]
    want = [s.renderFootprints(f, 40, DEPTH, seed=3, stream_base=7) for f in lists]
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for f, st in zip(lists, streams):
        with torch.cuda.stream(st):
            t = torch.from_numpy(f).to("cuda", non_blocking=False)
            got.append(s.renderFootprints(t, 40, DEPTH, seed=3, stream_base=7, stats=False))  # both launches in flight
            assert s.last_stats is None and got[-1].stats is None
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for g, w in zip(got, want):
        assert g.accum.dtype == torch.int32 and g.rgb.dtype == torch.uint8 and g.accum.is_cuda
        assert np.array_equal(g.accum.cpu().numpy(), w.accum) and np.array_equal(g.rgb.cpu().numpy(), w.rgb)
    with torch.cuda.stream(streams[1]):
        g = s.renderFootprints(torch.from_numpy(lists[0]).cuda(), 40, DEPTH, seed=3, stream_base=7)
    assert g.stats["kernel_ms"] > 0.0 and g.stats["pixels"] == len(lists[0]) and g.stats["samples"] == int(want[0].accum[:, 0].sum())
    assert np.array_equal(g.accum.cpu().numpy(), want[0].accum)


def test_c_program_renders_eight_footprints(rt, orc, tmp_path):
    import subprocess

    from test_footprints_host import build_footprint_smoke
    from test_gpu_ray_queries import _smoke_scene
    out = subprocess.run([build_footprint_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "footprints: rendered 8 pixels on the GPU" in out.stdout
    rows = np.array([[int(x) for x in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith("pixel ")])
    fp = np.zeros((8, 12))
    for i in range(8):  # footprint_smoke.c's list
        fp[i] = [0.0, 0.5, -2.0, -0.8 + 0.2 * i, -0.3, 1.0, 0.2, 0.0, 0.0, 0.0, 0.6, 0.0]
    fp[7, 3:] = 0.0
    want = fc.compose(orc, orc.OracleScene(_smoke_scene(rt)), fp, 20, 10, 5, stream_base=100)
    assert np.array_equal(rows[:, :4], want.accum) and np.array_equal(rows[:, 4:], want.rgb)
    assert list(want.accum[7]) == [11, 0, 0, 0]
