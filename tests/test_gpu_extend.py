"""Extending a rendered buffer (rt_render_extend, rt_render_footprints_extend and their device variants): render at a, extend
a -> b, and hold every PixelStats word and every rgb byte to the ORACLE rendered directly at b (OracleScene.render_rows; for
footprints footprint_cases.compose) -- never to the library's own render.  LDS-resident, global-memory and textured scenes, both
kernel variants on either side, steps of one sample and of many, chains, interleaved shards, every launch setting with the plan
the library reports, list sizes around a wave, lists with nothing and with everything to continue, the statistics, buffers that
are not what the arguments say, two extensions in flight on two streams, and the C consumer."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import footprint_cases as fc
import scenes
from test_gpu_footprints import DEPTH, _case
from test_gpu_footprints import _expected as _fp_expected
from test_gpu_footprints import _oracle as _fp_oracle
from test_gpu_footprints import _scene as _fp_scene

pytestmark = pytest.mark.gpu

SEED = 5
EARLY = 11  # Count of a pixel that stopped early, at every spp >= 10
STEPS = ((12, 13), (12, 40), (13, 40), (39, 40))
CLASSES = {"all_materials": (739, 2172), "many_spheres": (442, 293), "earth_thumb": (2243, 162)}  # final / continued, from the oracle


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(objects, camera, max_w, max_h) at the scene's default size"""
    if name == "earth_thumb":
        return scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    return getattr(scenes, name)()


def _cam(name, spp):
    return dataclasses.replace(_frame(name)[1], SamplesPerPixel=spp)


@functools.lru_cache(maxsize=None)
def _scene(rt, name, walk_tree=None):
    return rt.Scene.make(_frame(name)[0], walk_tree=walk_tree)


@functools.lru_cache(maxsize=None)
def _oracle(orc, name, spp):
    """The oracle's whole frame at spp: (accum, rgb, stats), computed once and never written to."""
    _, _, w, h = _frame(name)
    acc, rgb, st = orc.OracleScene(_frame(name)[0]).render_rows(w, h, _cam(name, spp).to_abi(), seed=SEED, threads=16)
    acc.setflags(write=False); rgb.setflags(write=False)
    return acc, rgb, st


@functools.lru_cache(maxsize=None)
def _base(rt, name, spp, counters=False, walk_tree=None):
    _, _, w, h = _frame(name)
    res = _scene(rt, name, walk_tree).render_rows(w, h, _cam(name, spp), seed=SEED, counters=counters)
    res.accum.setflags(write=False)
    return res


def _extend(rt, name, accum, done, to, **kw):
    _, _, w, h = _frame(name)
    return _scene(rt, name, kw.pop("walk_tree", None)).extend_rows(w, h, _cam(name, to), accum, done, seed=SEED, **kw)


@pytest.mark.parametrize("name", ["all_materials", "many_spheres", "earth_thumb"])
def test_extension_equals_the_oracle_at_the_target(rt, orc, name):
    _, _, w, h = _frame(name)
    assert _scene(rt, name).info()["lds_resident"] == (0 if name == "many_spheres" else 1)
    for b in (13, 40):  # both classes of the list builder are exercised: a condition on the EXPECTED frame
        want = _oracle(orc, name, b)[0]
        n, final, cont = want.shape[0] * want.shape[1], int((want[..., 0] == EARLY).sum()), int((want[..., 0] == b).sum())
        print(f"{name} at {b}: {final} final, {cont} continued, of {n}")
        assert (final, cont) == CLASSES[name] and final + cont == n == (2 * w + 1) * (2 * h + 1)
        assert final >= 0.05 * n and cont >= 0.05 * n
    for base_counters in (False, True):
        for ext_counters in (False, True):
            for a, b in STEPS:
                got = _extend(rt, name, _base(rt, name, a, base_counters).accum, a, b, counters=ext_counters)
                want_acc, want_rgb, _ = _oracle(orc, name, b)
                assert np.array_equal(got.accum, want_acc), (name, a, b, base_counters, ext_counters)
                assert np.array_equal(got.rgb, want_rgb), (name, a, b, base_counters, ext_counters)
            mid = _extend(rt, name, _base(rt, name, 12, base_counters).accum, 12, 13, counters=ext_counters)  # the chain 12 -> 13 -> 40
            assert np.array_equal(mid.accum, _oracle(orc, name, 13)[0]) and np.array_equal(mid.rgb, _oracle(orc, name, 13)[1])
            end = _extend(rt, name, mid.accum, 13, 40, counters=not ext_counters)
            assert np.array_equal(end.accum, _oracle(orc, name, 40)[0]) and np.array_equal(end.rgb, _oracle(orc, name, 40)[1])


def test_interleaved_shards_reassemble_to_the_oracles_frame(rt, orc):
    name = "all_materials"
    s, (_, _, w, h) = _scene(rt, name), _frame(name)
    want_acc, want_rgb, _ = _oracle(orc, name, 40)
    acc, rgb = np.zeros_like(want_acc), np.zeros_like(want_rgb)
    for r in range(3):
        part = s.render_rows(w, h, _cam(name, 12), seed=SEED, row_first=r, row_stride=3)
        got = s.extend_rows(w, h, _cam(name, 40), part.accum, 12, seed=SEED, row_first=r, row_stride=3)
        assert got.stats["pixels"] == part.accum.shape[0] * part.accum.shape[1]
        acc[r::3], rgb[r::3] = got.accum, got.rgb
    assert np.array_equal(acc, want_acc) and np.array_equal(rgb, want_rgb)
    row = 2 * h - 6  # one shard of a single row
    part = s.render_rows(w, h, _cam(name, 12), seed=SEED, row_first=row, n_rows=1)
    got = s.extend_rows(w, h, _cam(name, 40), part.accum, 12, seed=SEED, row_first=row)
    assert got.accum.shape[0] == 1 and 0 < int((want_acc[row, :, 0] == 40).sum())
    assert np.array_equal(got.accum[0], want_acc[row]) and np.array_equal(got.rgb[0], want_rgb[row])


SETTINGS = ([dict(block_threads=b) for b in (256, 512, 768, 1024)] + [dict(chunk_pixels=c) for c in (1, 4, 64)] +
            [dict(park_lanes=-1), dict(yield_lanes=20), dict(passes=1), dict(passes=2), dict(passes=1, block_threads=256, chunk_pixels=64)])


def _check_plan(rt, kind, done, to, opt):
    plan = rt.hooks.last_launch_plan()
    i, o = plan["in"], plan["out"]
    assert i["kind"] == kind and i["spp"] == to and i["first_sample"] == done
    if "passes" in opt:  # accepted, reported as given, and ignored: the plan below is the same
        assert i["s_passes"] == opt["passes"]
    assert o["two_pass"] == 1 and o["error"] == 0 and o["pairs"] == 0 and o["sort"] == 0 and o["list"] > 0
    assert o["B_mode"] == (8 if kind == 3 else 2) and o["B_grid"] > 0 and o["B_k"] == 5
    assert all(v == 0 for k, v in o.items() if k.startswith("A_")) and "A_grid" in o  # no pass A
    if "chunk_pixels" in opt:
        assert o["B_chunk"] == opt["chunk_pixels"]
    if "block_threads" in opt:
        assert o["q_block"] == (opt["block_threads"] if kind == 0 or opt["block_threads"] == 256 else 1024)
    if opt.get("park_lanes") == -1:
        assert o["B_park"] == 0 and o["B_park_l"] == 0
    if "yield_lanes" in opt:
        assert o["B_yield"] == opt["yield_lanes"]


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_launch_settings_do_not_change_results(rt, orc, name):
    torch = pytest.importorskip("torch")
    A = rt._abi
    want_acc, want_rgb, _ = _oracle(orc, name, 40)
    base = torch.from_numpy(np.array(_base(rt, name, 12).accum)).cuda()
    for opt in SETTINGS:
        for counters in (False, True):
            got = _extend(rt, name, base.clone(), 12, 40, counters=counters, options=A.rt_render_options(**opt))
            assert np.array_equal(got.accum.cpu().numpy(), want_acc) and np.array_equal(got.rgb.cpu().numpy(), want_rgb), (name, opt, counters)
            _check_plan(rt, 0, 12, 40, opt)
    # the same settings over a footprint list
    s, fp = _fp_scene(rt, name), torch.from_numpy(_case(name)[1]).cuda()
    want = _fp_expected(orc, name, 40)
    base = s.renderFootprints(fp, 12, DEPTH, seed=SEED).accum
    for opt in SETTINGS:
        for counters in (False, True):
            got = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters, options=A.rt_render_options(**opt), extend=(base.clone(), 12))
            assert np.array_equal(got.accum.cpu().numpy(), want.accum) and np.array_equal(got.rgb.cpu().numpy(), want.rgb), (name, opt, counters)
            _check_plan(rt, 3, 12, 40, opt)
    # a fresh render still reports first_sample 0
    s.renderFootprints(fp, 40, DEPTH, seed=SEED)
    assert rt.hooks.last_launch_plan()["in"]["first_sample"] == 0


def test_list_sizes_around_a_wave_and_lists_of_one_class(rt, orc):
    s, o, fp = _fp_scene(rt, "all_materials"), _fp_oracle(orc, "all_materials"), _case("all_materials")[1]
    for n in (1, 63, 64, 65):
        want = fc.compose(orc, o, fp[:n], 13, DEPTH, SEED)
        for counters in (False, True):
            base = s.renderFootprints(fp[:n], 12, DEPTH, seed=SEED, counters=counters)
            got = s.renderFootprints(fp[:n], 13, DEPTH, seed=SEED, counters=not counters, extend=(base.accum, 12))
            assert np.array_equal(got.accum, want.accum) and np.array_equal(got.rgb, want.rgb), (n, counters)
            assert got.stats["pixels"] == n and got.stats["pixels_early"] == int(want.early.sum())
    # no pixel continues: degenerate footprints (Ray.make' fails at every sample) are Black and final; the result equals the base
    dead = fp[:65].copy()
    dead[:, 3:] = 0.0
    base = s.renderFootprints(dead, 12, DEPTH, seed=SEED)
    assert (base.accum == [EARLY, 0, 0, 0]).all()
    got = s.renderFootprints(dead, 40, DEPTH, seed=SEED, extend=(base.accum, 12))
    assert np.array_equal(got.accum, base.accum) and (got.rgb == 0).all()
    assert got.stats["samples"] == 0 and got.stats["pixels_early"] == 65 and got.stats["pixels"] == 65
    # every pixel continues: the longest run of the many_spheres list that the EXPECTED values continue, as a slice with its stream_base
    s, fp, want = _fp_scene(rt, "many_spheres"), _case("many_spheres")[1], _fp_expected(orc, "many_spheres", 40)
    cont = np.concatenate([[False], want.accum[:, 0] == 40, [False]])
    edges = np.flatnonzero(cont[1:] != cont[:-1]).reshape(-1, 2)
    a, b = (int(x) for x in max(edges, key=lambda e: e[1] - e[0]))
    assert b - a > 64  # more than a wave
    base = s.renderFootprints(fp[a:b], 12, DEPTH, seed=SEED, stream_base=a)
    assert (base.accum[:, 0] == 12).all()
    got = s.renderFootprints(fp[a:b], 40, DEPTH, seed=SEED, stream_base=a, extend=(base.accum, 12))
    assert np.array_equal(got.accum, want.accum[a:b]) and np.array_equal(got.rgb, want.rgb[a:b])
    assert got.stats["samples"] == 28 * (b - a) and got.stats["pixels_early"] == 0


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_footprints_equal_the_composition_at_the_target(rt, orc, name):
    s, fp = _fp_scene(rt, name), _case(name)[1]
    assert 130 <= len(fp) <= 143
    want40, want13 = _fp_expected(orc, name, 40), fc.compose(orc, _fp_oracle(orc, name), fp, 13, DEPTH, SEED)
    early, full = int(want40.early.sum()), int((want40.accum[:, 0] == 40).sum())
    assert early >= 0.05 * len(fp) and full >= 0.05 * len(fp)
    for counters in (False, True):
        base = s.renderFootprints(fp, 12, DEPTH, seed=SEED, counters=counters)
        got = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters, extend=(base.accum, 12))
        assert np.array_equal(got.accum, want40.accum) and np.array_equal(got.rgb, want40.rgb), (name, counters)
        mid = s.renderFootprints(fp, 13, DEPTH, seed=SEED, counters=not counters, extend=(base.accum, 12))
        assert np.array_equal(mid.accum, want13.accum) and np.array_equal(mid.rgb, want13.rgb), (name, counters)
        end = s.renderFootprints(fp, 40, DEPTH, seed=SEED, counters=counters, extend=(mid.accum, 13))
        assert np.array_equal(end.accum, want40.accum) and np.array_equal(end.rgb, want40.rgb), (name, counters)
    # a slice [a, b) extended with stream_base + a equals that slice of the whole (the whole composed with stream_base 1000 would cost a
    # second composition: the slice is taken of the list itself, stream_base = a)
    for a, b in ((0, 7), (7, 71), (71, len(fp))):
        base = s.renderFootprints(fp[a:b], 12, DEPTH, seed=SEED, stream_base=a)
        got = s.renderFootprints(fp[a:b], 40, DEPTH, seed=SEED, stream_base=a, extend=(base.accum, 12))
        assert np.array_equal(got.accum, want40.accum[a:b]) and np.array_equal(got.rgb, want40.rgb[a:b]), (name, a, b)


def test_statistics_describe_the_extension_alone(rt, orc):
    for name in ("all_materials", "many_spheres"):
        want_acc, _, want_st = _oracle(orc, name, 40)
        for counters in (False, True):
            base = _base(rt, name, 12, counters, "reference")
            got = _extend(rt, name, base.accum, 12, 40, counters=counters, walk_tree="reference")
            st = got.stats
            assert st is _scene(rt, name, "reference").last_stats
            assert st["samples"] == int(got.accum[..., 0].sum()) - int(base.accum[..., 0].sum()) == 28 * int((want_acc[..., 0] == 40).sum())
            assert st["pixels_early"] == int((want_acc[..., 0] == EARLY).sum()) == want_st["pixels_early"]
            assert st["pixels"] == want_acc.shape[0] * want_acc.shape[1]
            assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
            assert base.stats["samples"] + st["samples"] == want_st["samples"]
            for key in ("rays", "aabb_tests", "prim_tests", "reflections"):  # (aabb_tests: the scene walks the reference's tree)
                if counters:
                    assert base.stats[key] + st[key] == want_st[key] and st[key] > 0, (name, key)
                else:
                    assert st[key] == 0


def _raw_extend(rt, name, accum, rgb, done, to):
    _, _, w, h = _frame(name)
    cam = _cam(name, to).to_abi()
    return rt.lib.rt_render_extend(_scene(rt, name).handle, C.byref(cam), w, h, SEED, 0, 0, 1, accum.shape[0], 0, done,
                                   accum.ctypes.data_as(C.POINTER(C.c_int32)), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), None)


def test_a_malformed_buffer_is_refused_and_left_unchanged(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name = "all_materials"
    _, _, w, h = _frame(name)
    good = np.array(_base(rt, name, 12).accum)
    cont = np.argwhere(good[..., 0] == 12)
    final = np.argwhere(good[..., 0] == EARLY)
    for (r, c), count in ((cont[len(cont) // 2], 13), (cont[0], 0), (final[-1], 12 + 40), (cont[-1], -12)):
        bad = good.copy()
        bad[r, c, 0] = count
        accum, rgb = bad.copy(), np.full(good.shape[:2] + (3,), 0xA5, np.uint8)
        assert _raw_extend(rt, name, accum, rgb, 12, 40) == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error()
        assert np.array_equal(accum, bad) and (rgb == 0xA5).all()
        with pytest.raises(rt.RtError) as e:
            _extend(rt, name, bad, 12, 40)
        assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
        # the device variant: with stats it reports the buffer, without it cannot -- either way nothing is written
        for stats in (True, False):
            d_acc, d_rgb = torch.from_numpy(bad).cuda(), torch.full(good.shape[:2] + (3,), 0xA5, dtype=torch.uint8, device="cuda")
            cam, st = _cam(name, 40).to_abi(), A.rt_stats()
            rc = rt.lib.rt_render_extend_device(_scene(rt, name).handle, C.byref(cam), w, h, SEED, 0, 0, 1, bad.shape[0], 0, 12, d_acc.data_ptr(),
                                                d_rgb.data_ptr(), torch.cuda.current_stream().cuda_stream, None, C.byref(st) if stats else None)
            torch.cuda.synchronize()
            assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK)
            assert np.array_equal(d_acc.cpu().numpy(), bad) and bool((d_rgb == 0xA5).all())
    # the wrong samples_done for a good buffer is such a buffer too; the right one still works afterwards
    accum, rgb = good.copy(), np.full(good.shape[:2] + (3,), 0xA5, np.uint8)
    assert _raw_extend(rt, name, accum, rgb, 13, 40) == A.RT_ERR_INVALID_ARGUMENT
    assert np.array_equal(accum, good) and (rgb == 0xA5).all()
    assert _raw_extend(rt, name, accum, rgb, 12, 40) == A.RT_OK
    assert np.array_equal(accum, _oracle(orc, name, 40)[0]) and np.array_equal(rgb, _oracle(orc, name, 40)[1])
    # footprints
    s, fp = _fp_scene(rt, name), _case(name)[1]
    base = s.renderFootprints(fp, 12, DEPTH, seed=SEED).accum
    base[5, 0] = 14
    with pytest.raises(rt.RtError) as e:
        s.renderFootprints(fp, 40, DEPTH, seed=SEED, extend=(base, 12))
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT


def test_two_extensions_in_flight_on_two_streams(rt, orc):
    torch = pytest.importorskip("torch")
    name = "all_materials"
    s, (_, _, w, h) = _scene(rt, name), _frame(name)
    want_acc, want_rgb, _ = _oracle(orc, name, 40)
    parts = [s.render_rows(w, h, _cam(name, 12), seed=SEED, row_first=r, row_stride=2).accum for r in range(2)]
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for r, st in enumerate(streams):
        with torch.cuda.stream(st):
            t = torch.from_numpy(parts[r]).to("cuda", non_blocking=False)
            got.append(s.extend_rows(w, h, _cam(name, 40), t, 12, seed=SEED, row_first=r, row_stride=2, stats=False))  # both in flight
            assert s.last_stats is None and got[-1].stats is None and got[-1].accum is t
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for r, g in enumerate(got):
        assert np.array_equal(g.accum.cpu().numpy(), want_acc[r::2]) and np.array_equal(g.rgb.cpu().numpy(), want_rgb[r::2])


def test_a_rank_extends_its_own_shard(rt, orc):
    torch = pytest.importorskip("torch")
    from ray_tracing_fsharp_amd import distributed as dist
    name = "all_materials"
    s, (_, _, w, h) = _scene(rt, name), _frame(name)
    want_acc = _oracle(orc, name, 40)[0]
    first, stride, n = dist.shard_rows(2 * h + 1, 1, 4)
    local = torch.zeros((n, 2 * w + 1, 4), dtype=torch.int32, device="cuda:0")
    dist.render_shard_device(s, _cam(name, 12), w, h, SEED, 0, first, stride, n, local)
    st = dist.extend_shard_device(s, _cam(name, 40), w, h, SEED, 0, first, stride, n, local, 12, want_stats=True)
    assert np.array_equal(local.cpu().numpy(), want_acc[1::4]) and st["pixels"] == n * (2 * w + 1)


def _digest(accum, rgb):  # extend_smoke.c's: FNV-1a over the PixelStats words (little-endian bytes), then the rgb bytes
    h = 1469598103934665603
    for byte in np.ascontiguousarray(accum, "<i4").tobytes() + np.ascontiguousarray(rgb, np.uint8).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_program_extends_a_frame(rt, orc, tmp_path):
    from test_extend_host import build_extend_smoke
    from test_gpu_ray_queries import _smoke_scene
    out = subprocess.run([build_extend_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "extend: a malformed buffer is refused and left unchanged" in out.stdout
    line = [ln for ln in out.stdout.splitlines() if "12 -> 24 equals a render at 24" in ln]
    assert len(line) == 1
    max_w, max_h = 12, 7  # extend_smoke.c's frame and camera
    cam = rt.Camera.makeBasic(24, 1.0, 25.0 / 15.0, rt.Point.make(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=10)
    acc, rgb, _ = orc.OracleScene(_smoke_scene(rt)).render_rows(max_w, max_h, cam.to_abi(), seed=5, threads=4)
    assert int(line[0].split()[-1], 16) == _digest(acc, rgb)
    assert f"{int((acc[..., 0] == EARLY).sum())} final" in line[0]
