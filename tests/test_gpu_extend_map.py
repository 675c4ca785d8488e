"""Extending by map (rt_render_extend_map, rt_render_footprints_extend_map and their device variants): render at 12, continue
every pixel to a target of its own, and hold every PixelStats word and every rgb byte to the ORACLE -- pixel i of the oracle's
frame at spp = targets[i] where the pixel is continued, at spp = its Count where it is left or final (for footprints
footprint_cases.compose) -- never to the library's own render.

SHAPES: the three scenes at their tests/scenes.py sizes (about 2,900 pixels); base 12, cap 41, targets the cyclic pattern
(0, 12, 13, 14, 40, 11, 41, 16, -1) over the pixel index, so that one range of pass B holds pixels adding 1, 2, 28 and 29 samples
side by side and the final-rgb pass has "left" pixels (targets 0, 12, 11, -1) to write."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_gpu_extend import CLASSES, EARLY, SEED, SETTINGS, _base, _cam, _digest, _frame, _oracle, _scene
from test_gpu_footprints import DEPTH, _case
from test_gpu_footprints import _expected as _fp_expected
from test_gpu_footprints import _scene as _fp_scene

pytestmark = pytest.mark.gpu

BASE, CAP = 12, 41
PATTERN = (0, 12, 13, 14, 40, 11, 41, 16, -1)
PATTERN2 = (16, 41, 0, 13, 14, 40, -1, 12, 11)  # the second map of a chain: other targets for the same pixels, some below the first
NAMES = ["all_materials", "many_spheres", "earth_thumb"]


def _targets(n, pattern=PATTERN):
    return np.resize(np.array(pattern, np.int32), n)


def _expect(count, targets, at):
    """The per-pixel expectation: `count` [n] the pixels' Counts before the call, at(spp) -> (accum [n, 4], rgb [n, 3]) the oracle's
    values at spp.  Returns accum, rgb and the continued mask."""
    cont = (count >= BASE) & (targets > count)
    acc, rgb = (np.array(a) for a in at(BASE))
    assert set(np.unique(count)) <= {EARLY, BASE}
    for t in np.unique(targets[cont]):
        a, r = at(int(t))
        pick = cont & (targets == t)
        acc[pick], rgb[pick] = a[pick], r[pick]
    return acc, rgb, cont


def _frame_at(orc, name):
    def at(spp):
        a, r, _ = _oracle(orc, name, spp)
        return a.reshape(-1, 4), r.reshape(-1, 3)
    return at


def _frame_expect(orc, name, targets, count=None):
    want12 = _oracle(orc, name, BASE)[0]
    shape = want12.shape[:2]
    count = want12[..., 0].reshape(-1) if count is None else count
    acc, rgb, cont = _expect(count, targets.reshape(-1), _frame_at(orc, name))
    return acc.reshape(shape + (4,)), rgb.reshape(shape + (3,)), cont.reshape(shape)


def _map(rt, name, accum, targets, cap=CAP, **kw):
    _, _, w, h = _frame(name)
    return _scene(rt, name, kw.pop("walk_tree", None)).extend_rows_map(w, h, _cam(name, cap), accum, targets, seed=SEED, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_a_map_equals_the_oracle_pixel_by_pixel(rt, orc, name):
    _, _, w, h = _frame(name)
    shape = (2 * h + 1, 2 * w + 1)
    n = shape[0] * shape[1]
    targets = _targets(n).reshape(shape)
    want_acc, want_rgb, cont = _frame_expect(orc, name, targets)
    # conditions on the EXPECTED frame: at least 5 % of the pixels are final and at least 5 % are not -- test_gpu_extend's CLASSES, the
    # oracle's own counts -- and every target above 12 is in use.  (Of the pixels that are not final the pattern continues five in
    # nine -- earth_thumb: 90 of 162, 3.7 % of the frame -- and leaves the others.)
    final, live = int((want_acc[..., 0] == EARLY).sum()), int((want_acc[..., 0] != EARLY).sum())
    print(f"{name}: {final} final, {live} not final of which {int(cont.sum())} continued by the pattern, of {n}")
    assert (final, live) == CLASSES[name] and final >= 0.05 * n and live >= 0.05 * n and 0.5 * live <= cont.sum() < live
    assert set(np.unique(targets[cont])) == {t for t in PATTERN if t > BASE} == {13, 14, 16, 40, 41}
    assert int(((want_acc[..., 0] == BASE) & ~cont).sum()) > 0  # "left" pixels
    for counters in (False, True):
        base = _base(rt, name, BASE, counters).accum
        got = _map(rt, name, base, targets, counters=not counters)
        assert np.array_equal(got.accum, want_acc) and np.array_equal(got.rgb, want_rgb), (name, counters)
        assert got.stats["samples"] == int((want_acc[..., 0] - base[..., 0]).sum()) == int((targets - BASE)[cont].sum())
        assert got.stats["pixels"] == n and got.stats["pixels_early"] == final
        # a chain of two different maps: the end state is the oracle at the per-pixel maximum
        t2 = _targets(n, PATTERN2).reshape(shape)
        end = _map(rt, name, got.accum, t2, counters=counters)
        both = np.maximum(targets, t2)
        end_acc, end_rgb, _ = _frame_expect(orc, name, both)
        assert np.array_equal(end.accum, end_acc) and np.array_equal(end.rgb, end_rgb), (name, counters)
        assert end.stats["samples"] == int((end_acc[..., 0] - want_acc[..., 0]).sum()) > 0
        # a uniform map is rt_render_extend's result: the oracle at 40; on top of the first map it takes only what is below 40 there
        uni = _map(rt, name, base, np.full(shape, 40, np.int32), counters=counters)
        assert np.array_equal(uni.accum, _oracle(orc, name, 40)[0]) and np.array_equal(uni.rgb, _oracle(orc, name, 40)[1])
        top = _map(rt, name, got.accum, np.full(shape, 40, np.int32), counters=counters)
        top_acc, top_rgb, _ = _frame_expect(orc, name, np.maximum(targets, 40))
        assert np.array_equal(top.accum, top_acc) and np.array_equal(top.rgb, top_rgb)
        # all zeros: the buffer as it is, rgb for every pixel
        zero = _map(rt, name, got.accum, np.zeros(shape, np.int32), counters=counters)
        assert np.array_equal(zero.accum, want_acc) and np.array_equal(zero.rgb, want_rgb) and zero.stats["samples"] == 0
        assert zero.stats["pixels_early"] == final and zero.stats["pixels"] == n
    low = _map(rt, name, _base(rt, name, BASE).accum, np.full(shape, 12, np.int32), cap=12)  # the least cap: nothing to continue
    assert np.array_equal(low.accum, _oracle(orc, name, BASE)[0]) and np.array_equal(low.rgb, _oracle(orc, name, BASE)[1])


def _check_plan(rt, kind, cap, opt):
    plan = rt.hooks.last_launch_plan()
    i, o = plan["in"], plan["out"]
    assert i["kind"] == kind and i["spp"] == cap and i["first_sample"] == BASE and i["map"] == 1  # words 77 and 78
    if "passes" in opt:  # accepted, reported as given, and ignored
        assert i["s_passes"] == opt["passes"]
    assert o["two_pass"] == 1 and o["error"] == 0 and o["pairs"] == 0 and o["sort"] == 0 and o["list"] > 0
    assert o["B_mode"] == (10 if kind == 3 else 9) and o["B_grid"] > 0 and o["B_k"] == 5 and o["B_lds_bytes"] <= 160 * 1024
    assert all(v == 0 for k, v in o.items() if k.startswith("A_")) and "A_grid" in o  # no pass A
    if "chunk_pixels" in opt:  # (halved only where the map's scratch does not fit the LDS: not at these scenes)
        assert o["B_chunk"] == opt["chunk_pixels"]
    assert o["B_chunk"] >= 1
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
    _, _, w, h = _frame(name)
    shape = (2 * h + 1, 2 * w + 1)
    targets = _targets(shape[0] * shape[1]).reshape(shape)
    want_acc, want_rgb, _ = _frame_expect(orc, name, targets)
    base, d_t = torch.from_numpy(np.array(_base(rt, name, BASE).accum)).cuda(), torch.from_numpy(targets).cuda()
    for opt in SETTINGS:
        for counters in (False, True):
            got = _map(rt, name, base.clone(), d_t, counters=counters, options=A.rt_render_options(**opt))
            assert np.array_equal(got.accum.cpu().numpy(), want_acc) and np.array_equal(got.rgb.cpu().numpy(), want_rgb), (name, opt, counters)
            _check_plan(rt, 0, CAP, opt)
    # the same settings over a footprint list
    s, fp = _fp_scene(rt, name), torch.from_numpy(_case(name)[1]).cuda()
    tg = _targets(len(fp))
    want_acc, want_rgb, _ = _fp_expect(orc, name, tg)
    base, d_t = s.renderFootprints(fp, BASE, DEPTH, seed=SEED).accum, torch.from_numpy(tg).cuda()
    for opt in SETTINGS:
        for counters in (False, True):
            got = s.renderFootprints(fp, CAP, DEPTH, seed=SEED, counters=counters, options=A.rt_render_options(**opt), extend_map=(base.clone(), d_t))
            assert np.array_equal(got.accum.cpu().numpy(), want_acc) and np.array_equal(got.rgb.cpu().numpy(), want_rgb), (name, opt, counters)
            _check_plan(rt, 3, CAP, opt)
    # an extension to one target and a fresh render still report word 78 as 0
    s.renderFootprints(fp, 40, DEPTH, seed=SEED, extend=(base.clone(), BASE))
    assert rt.hooks.last_launch_plan()["in"]["map"] == 0 and rt.hooks.last_launch_plan()["in"]["first_sample"] == BASE
    s.renderFootprints(fp, 40, DEPTH, seed=SEED)
    assert rt.hooks.last_launch_plan()["in"]["map"] == 0 and rt.hooks.last_launch_plan()["in"]["first_sample"] == 0


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_the_reference_tree_and_a_tuned_tree_give_the_same_pixels(rt, orc, name):
    _, _, w, h = _frame(name)
    shape = (2 * h + 1, 2 * w + 1)
    targets = _targets(shape[0] * shape[1]).reshape(shape)
    want_acc, want_rgb, _ = _frame_expect(orc, name, targets)
    base = _base(rt, name, BASE).accum
    got = _map(rt, name, base, targets, walk_tree="reference")
    assert np.array_equal(got.accum, want_acc) and np.array_equal(got.rgb, want_rgb)
    tuned = rt.Scene.make(_frame(name)[0])
    assert tuned.tune(w, h, _cam(name, CAP), seed=SEED)["tuned"] == 1
    for counters in (False, True):
        got = tuned.extend_rows_map(w, h, _cam(name, CAP), base, targets, seed=SEED, counters=counters)
        assert np.array_equal(got.accum, want_acc) and np.array_equal(got.rgb, want_rgb), counters


def _fp_expect(orc, name, targets, count=None):
    count = _fp_expected(orc, name, BASE).accum[:, 0] if count is None else count

    def at(spp):
        e = _fp_expected(orc, name, spp)
        return e.accum, e.rgb
    return _expect(count, targets, at)


@pytest.mark.parametrize("name", ["all_materials", "many_spheres"])
def test_footprints_equal_the_composition_at_the_per_pixel_targets(rt, orc, name):
    s, fp = _fp_scene(rt, name), _case(name)[1]
    tg = _targets(len(fp))
    want_acc, want_rgb, cont = _fp_expect(orc, name, tg)
    final = int((want_acc[:, 0] == EARLY).sum())
    live = int((want_acc[:, 0] != EARLY).sum())
    assert final >= 0.05 * len(fp) and live >= 0.05 * len(fp) and 0 < cont.sum() < live and set(np.unique(tg[cont])) == {13, 14, 16, 40, 41}
    for counters in (False, True):
        base = s.renderFootprints(fp, BASE, DEPTH, seed=SEED, counters=counters)
        got = s.renderFootprints(fp, CAP, DEPTH, seed=SEED, counters=not counters, extend_map=(base.accum, tg))
        assert np.array_equal(got.accum, want_acc) and np.array_equal(got.rgb, want_rgb), (name, counters)
        assert got.stats["samples"] == int((tg - BASE)[cont].sum()) and got.stats["pixels"] == len(fp) and got.stats["pixels_early"] == final
        t2 = _targets(len(fp), PATTERN2)
        end = s.renderFootprints(fp, CAP, DEPTH, seed=SEED, counters=counters, extend_map=(got.accum, t2))
        end_acc, end_rgb, _ = _fp_expect(orc, name, np.maximum(tg, t2))
        assert np.array_equal(end.accum, end_acc) and np.array_equal(end.rgb, end_rgb), (name, counters)
    # a slice [a, b) with stream_base = a equals that slice of the whole
    for a, b in ((0, 7), (7, 71), (71, len(fp))):
        base = s.renderFootprints(fp[a:b], BASE, DEPTH, seed=SEED, stream_base=a)
        got = s.renderFootprints(fp[a:b], CAP, DEPTH, seed=SEED, stream_base=a, extend_map=(base.accum, np.ascontiguousarray(tg[a:b])))
        assert np.array_equal(got.accum, want_acc[a:b]) and np.array_equal(got.rgb, want_rgb[a:b]), (name, a, b)


def test_lists_of_63_64_and_65_continued_pixels(rt, orc):
    """Every pixel of the list is continued (one range of a wave: one pixel short, full, one over), each by another amount: the longest
    run of the many_spheres list that the EXPECTED values continue, as slices with their stream_base."""
    torch = pytest.importorskip("torch")
    s, fp = _fp_scene(rt, "many_spheres"), _case("many_spheres")[1]
    cont = np.concatenate([[False], _fp_expected(orc, "many_spheres", 40).accum[:, 0] == 40, [False]])
    edges = np.flatnonzero(cont[1:] != cont[:-1]).reshape(-1, 2)
    a, b = (int(x) for x in max(edges, key=lambda e: e[1] - e[0]))
    assert b - a >= 65
    for n in (63, 64, 65):
        tg = _targets(len(fp), (13, 41, 14, 40, 16))
        want_acc, want_rgb, c = _fp_expect(orc, "many_spheres", tg)
        assert c[a:a + n].all()
        for counters in (False, True):
            for chunk in (0, 64):  # the plan's units, and one range holding the whole list
                base = s.renderFootprints(torch.from_numpy(fp[a:a + n]).cuda(), BASE, DEPTH, seed=SEED, stream_base=a, counters=counters)
                assert bool((base.accum[:, 0] == BASE).all())
                got = s.renderFootprints(torch.from_numpy(fp[a:a + n]).cuda(), CAP, DEPTH, seed=SEED, stream_base=a, counters=counters,
                                         options=rt._abi.rt_render_options(chunk_pixels=chunk), extend_map=(base.accum, torch.from_numpy(tg[a:a + n].copy()).cuda()))
                assert np.array_equal(got.accum.cpu().numpy(), want_acc[a:a + n]) and np.array_equal(got.rgb.cpu().numpy(), want_rgb[a:a + n]), (n, counters, chunk)
                assert got.stats["samples"] == int((tg[a:a + n] - BASE).sum()) and got.stats["pixels_early"] == 0 and got.stats["pixels"] == n


def test_interleaved_shards_and_a_one_row_shard(rt, orc):
    name = "all_materials"
    s, (_, _, w, h) = _scene(rt, name), _frame(name)
    shape = (2 * h + 1, 2 * w + 1)
    targets = _targets(shape[0] * shape[1]).reshape(shape)
    want_acc, want_rgb, cont = _frame_expect(orc, name, targets)
    acc, rgb = np.zeros_like(want_acc), np.zeros_like(want_rgb)
    for r in range(3):
        part = s.render_rows(w, h, _cam(name, BASE), seed=SEED, row_first=r, row_stride=3)
        got = s.extend_rows_map(w, h, _cam(name, CAP), part.accum, np.ascontiguousarray(targets[r::3]), seed=SEED, row_first=r, row_stride=3)
        assert got.stats["pixels"] == part.accum.shape[0] * part.accum.shape[1]
        acc[r::3], rgb[r::3] = got.accum, got.rgb
    assert np.array_equal(acc, want_acc) and np.array_equal(rgb, want_rgb)
    row = 2 * h - 6  # one shard of a single row
    part = s.render_rows(w, h, _cam(name, BASE), seed=SEED, row_first=row, n_rows=1)
    got = s.extend_rows_map(w, h, _cam(name, CAP), part.accum, np.ascontiguousarray(targets[row:row + 1]), seed=SEED, row_first=row)
    assert got.accum.shape[0] == 1 and 0 < int(cont[row].sum())
    assert np.array_equal(got.accum[0], want_acc[row]) and np.array_equal(got.rgb[0], want_rgb[row])


def test_statistics_describe_the_map_alone(rt, orc):
    for name in ("all_materials", "many_spheres"):
        _, _, w, h = _frame(name)
        shape = (2 * h + 1, 2 * w + 1)
        targets = _targets(shape[0] * shape[1]).reshape(shape)
        want_acc, _, cont = _frame_expect(orc, name, targets)
        want41 = _oracle(orc, name, CAP)
        for counters in (False, True):
            base = _base(rt, name, BASE, counters, "reference")
            got = _map(rt, name, base.accum, targets, counters=counters, walk_tree="reference")
            st = got.stats
            assert st is _scene(rt, name, "reference").last_stats
            assert st["samples"] == int(got.accum[..., 0].sum()) - int(base.accum[..., 0].sum()) == int((targets - BASE)[cont].sum())
            assert st["pixels_early"] == int((want_acc[..., 0] == EARLY).sum()) and st["pixels"] == shape[0] * shape[1]
            assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
            # the oracle exposes counters per frame: render(12), the map, and a second map that takes every pixel to 41 together
            # trace exactly the samples of the oracle's frame at 41
            rest = _map(rt, name, got.accum, np.full(shape, CAP, np.int32), counters=counters, walk_tree="reference")
            assert np.array_equal(rest.accum, want41[0])
            assert base.stats["samples"] + st["samples"] + rest.stats["samples"] == want41[2]["samples"]
            for key in ("rays", "aabb_tests", "prim_tests", "reflections"):  # (aabb_tests: the scene walks the reference's tree)
                if counters:
                    assert base.stats[key] + st[key] + rest.stats[key] == want41[2][key] and st[key] > 0 and rest.stats[key] > 0, (name, key)
                else:
                    assert st[key] == 0


def test_a_malformed_buffer_or_map_is_refused_and_everything_left_unchanged(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    name = "all_materials"
    _, _, w, h = _frame(name)
    good = np.array(_base(rt, name, BASE).accum)
    shape = good.shape[:2]
    targets = _targets(shape[0] * shape[1]).reshape(shape)
    cont = np.argwhere((good[..., 0] == BASE) & (targets > BASE))
    left = np.argwhere((good[..., 0] == BASE) & (targets <= BASE))
    cam = _cam(name, CAP).to_abi()
    S = _scene(rt, name).handle
    cases = []
    for r, c in (cont[len(cont) // 2], left[0]):  # one pixel with Count 7 -- whatever its target
        bad = good.copy(); bad[r, c, 0] = 7
        cases.append((bad, targets))
    for r, c in (cont[0], left[-1]):              # one target above the cap
        t = targets.copy(); t[r, c] = CAP + 1
        cases.append((good, t))
    for acc0, t in cases:
        accum, rgb = acc0.copy(), np.full(shape + (3,), 0xA5, np.uint8)
        rc = rt.lib.rt_render_extend_map(S, C.byref(cam), w, h, SEED, 0, 0, 1, shape[0], 0, t.ctypes.data_as(C.POINTER(C.c_int32)),
                                         accum.ctypes.data_as(C.POINTER(C.c_int32)), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), None)
        assert rc == A.RT_ERR_INVALID_ARGUMENT and rt.lib.rt_last_error()
        assert np.array_equal(accum, acc0) and (rgb == 0xA5).all()
        with pytest.raises(rt.RtError) as e:
            _map(rt, name, acc0, t)
        assert e.value.code == A.RT_ERR_INVALID_ARGUMENT
        # the device variant: with stats it reports, without it cannot -- the unchanged Counts are the only evidence
        for stats in (True, False):
            d_acc, d_t = torch.from_numpy(acc0).cuda(), torch.from_numpy(t).cuda()
            d_rgb = torch.full(shape + (3,), 0xA5, dtype=torch.uint8, device="cuda")
            st = A.rt_stats()
            rc = rt.lib.rt_render_extend_map_device(S, C.byref(cam), w, h, SEED, 0, 0, 1, shape[0], 0, d_t.data_ptr(), d_acc.data_ptr(), d_rgb.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream, None, C.byref(st) if stats else None)
            torch.cuda.synchronize()
            assert rc == (A.RT_ERR_INVALID_ARGUMENT if stats else A.RT_OK)
            assert np.array_equal(d_acc.cpu().numpy(), acc0) and bool((d_rgb == 0xA5).all())
    # a final pixel is untouched whatever its target is -- above the cap too; the good buffer still works afterwards
    final = np.argwhere(good[..., 0] == EARLY)
    t = targets.copy(); t[tuple(final[0])] = CAP + 5
    got = _map(rt, name, good, t)
    want_acc, want_rgb, _ = _frame_expect(orc, name, targets)
    assert np.array_equal(got.accum, want_acc) and np.array_equal(got.rgb, want_rgb)
    # footprints
    s, fp = _fp_scene(rt, name), _case(name)[1]
    tg = _targets(len(fp))
    base = s.renderFootprints(fp, BASE, DEPTH, seed=SEED).accum
    bad = base.copy(); bad[5, 0] = 7
    high = tg.copy(); high[int(np.flatnonzero(base[:, 0] == BASE)[0])] = CAP + 1
    for acc0, t in ((bad, tg), (base, high)):
        with pytest.raises(rt.RtError) as e:
            s.renderFootprints(fp, CAP, DEPTH, seed=SEED, extend_map=(acc0, t))
        assert e.value.code == A.RT_ERR_INVALID_ARGUMENT


def test_two_maps_in_flight_on_two_streams(rt, orc):
    torch = pytest.importorskip("torch")
    name = "all_materials"
    s, (_, _, w, h) = _scene(rt, name), _frame(name)
    shape = (2 * h + 1, 2 * w + 1)
    targets = _targets(shape[0] * shape[1]).reshape(shape)
    want_acc, want_rgb, _ = _frame_expect(orc, name, targets)
    parts = [s.render_rows(w, h, _cam(name, BASE), seed=SEED, row_first=r, row_stride=2).accum for r in range(2)]
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for r, st in enumerate(streams):
        with torch.cuda.stream(st):
            t = torch.from_numpy(parts[r]).to("cuda", non_blocking=False)
            m = torch.from_numpy(np.ascontiguousarray(targets[r::2])).to("cuda", non_blocking=False)
            got.append((s.extend_rows_map(w, h, _cam(name, CAP), t, m, seed=SEED, row_first=r, row_stride=2, stats=False), m))  # both in flight
            assert s.last_stats is None and got[-1][0].stats is None and got[-1][0].accum is t
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for r, (g, _m) in enumerate(got):
        assert np.array_equal(g.accum.cpu().numpy(), want_acc[r::2]) and np.array_equal(g.rgb.cpu().numpy(), want_rgb[r::2])


def test_c_program_continues_a_frame_by_map(rt, orc, tmp_path):
    import dataclasses

    from test_extend_map_host import build_extend_map_smoke
    from test_gpu_ray_queries import _smoke_scene
    out = subprocess.run([build_extend_map_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "extend_map: a target above the cap is refused and the buffer left unchanged" in out.stdout
    line = [ln for ln in out.stdout.splitlines() if "continued 12 -> 24" in ln]
    assert len(line) == 1
    max_w, max_h = 12, 7  # extend_map_smoke.c's frame, camera and map: even pixels to 24, odd ones left
    cam = rt.Camera.makeBasic(24, 1.0, 25.0 / 15.0, rt.Point.make(0.0, 0.5, -2.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
    cam = dataclasses.replace(cam, BounceDepth=10)
    o = orc.OracleScene(_smoke_scene(rt))
    acc12, rgb12, _ = o.render_rows(max_w, max_h, dataclasses.replace(cam, SamplesPerPixel=12).to_abi(), seed=5, threads=4)
    acc24, rgb24, _ = o.render_rows(max_w, max_h, cam.to_abi(), seed=5, threads=4)
    even = (np.arange(acc12.shape[0] * acc12.shape[1]) % 2 == 0).reshape(acc12.shape[:2])
    cont = even & (acc12[..., 0] == 12)
    acc, rgb = np.where(cont[..., None], acc24, acc12), np.where(cont[..., None], rgb24, rgb12)
    assert int(line[0].split()[-1], 16) == _digest(acc, rgb)
    assert f"{int((acc12[..., 0] == EARLY).sum())} final, {int(cont.sum())} continued" in line[0]


def test_host_variants_without_rgb_equal_the_oracle(rt, orc):
    """The host variants lay their buffers out in one device allocation, and an optional buffer that is absent takes no room in it: so
    every host variant that takes `rgb`, called with rgb == NULL and with one (the wrapper always passes one), against the oracle's
    frame at 12, at 40 and at the per-pixel targets, and footprint_cases.compose for a list of 65 footprints (one wave and one)."""
    name = "all_materials"
    _, _, w, h = _frame(name)
    L, S = rt.lib, _scene(rt, name).handle
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    cam = lambda spp: C.byref(_cam(name, spp).to_abi())     # noqa: E731
    rows, cols = 2 * h + 1, 2 * w + 1
    targets = _targets(rows * cols).reshape(rows, cols)
    want12, want40, want_map = _oracle(orc, name, 12), _oracle(orc, name, 40), _frame_expect(orc, name, targets)
    n = 65
    px = np.ascontiguousarray(np.arange(rows * cols, dtype=np.int32)[::-1][3::rows * cols // n][:n])  # back to front, duplicates none
    fs, fp = _fp_scene(rt, name).handle, np.ascontiguousarray(_case(name)[1][:n])
    tg = np.ascontiguousarray(_targets(len(_case(name)[1]))[:n])
    fp12, fp40 = _fp_expected(orc, name, 12), _fp_expected(orc, name, 40)
    fp_map = _fp_expect(orc, name, _targets(len(_case(name)[1])))
    assert len(px) == n == len(fp)
    for with_rgb in (False, True):
        def run(call, shape, accum, want_acc, want_rgb, what):
            rgb = np.full(shape + (3,), 0xA5, np.uint8) if with_rgb else None
            assert call(i32(accum), rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if with_rgb else None) == rt._abi.RT_OK, (what, rt.lib.rt_last_error())
            assert np.array_equal(accum, want_acc.reshape(accum.shape)), (what, with_rgb)
            assert rgb is None or np.array_equal(rgb, want_rgb.reshape(rgb.shape)), what
            return accum

        frame = (rows, cols)
        base = run(lambda a, r: L.rt_render(S, cam(12), w, h, SEED, 0, 0, 1, rows, 0, a, r, None), frame, np.zeros(frame + (4,), np.int32), *want12[:2], "rt_render")
        run(lambda a, r: L.rt_render_extend(S, cam(40), w, h, SEED, 0, 0, 1, rows, 0, 12, a, r, None), frame, base.copy(), *want40[:2], "rt_render_extend")
        run(lambda a, r: L.rt_render_extend_map(S, cam(CAP), w, h, SEED, 0, 0, 1, rows, 0, i32(targets), a, r, None), frame, base.copy(), *want_map[:2],
            "rt_render_extend_map")
        flat12, flat40 = [x.reshape(rows * cols, -1)[px] for x in want12[:2]], [x.reshape(rows * cols, -1)[px] for x in want40[:2]]
        lst = run(lambda a, r: L.rt_render_pixels(S, cam(12), w, h, SEED, 0, n, i32(px), 0, a, r, None), (n,), np.zeros((n, 4), np.int32), *flat12, "rt_render_pixels")
        run(lambda a, r: L.rt_render_pixels_extend(S, cam(40), w, h, SEED, 0, n, i32(px), 0, 12, a, r, None), (n,), lst.copy(), *flat40, "rt_render_pixels_extend")
        f64 = fp.ctypes.data_as(C.POINTER(C.c_double))
        fb = run(lambda a, r: L.rt_render_footprints(fs, 0, n, f64, 12, DEPTH, SEED, 0, 0, a, r, None), (n,), np.zeros((n, 4), np.int32), fp12.accum[:n], fp12.rgb[:n],
                 "rt_render_footprints")
        run(lambda a, r: L.rt_render_footprints_extend(fs, 0, n, f64, 40, DEPTH, SEED, 0, 0, 12, a, r, None), (n,), fb.copy(), fp40.accum[:n], fp40.rgb[:n],
            "rt_render_footprints_extend")
        run(lambda a, r: L.rt_render_footprints_extend_map(fs, 0, n, f64, CAP, DEPTH, SEED, 0, 0, i32(tg), a, r, None), (n,), fb.copy(), fp_map[0][:n], fp_map[1][:n],
            "rt_render_footprints_extend_map")
