"""Scene.extendViews and Scene.extendViewsMap -- rt_render_views_extend(_device), rt_render_views_extend_map(_device): the batch's list builders,
its ordering and pass B of the views kernels from first_b on or over per-pixel ranges -- against the ORACLE's frame of each view's camera
and seed at the pixel's final Count (OracleScene.render_rows), bit for bit in every PixelStats word and every rgb byte, never against
the library's own render: mixed views with an empty view last and in the middle, both kernel variants, blocks and unit sizes; tiny views;
maps with a budget per pixel, an empty view in the middle, a second map on the first one's result; malformed buffers and maps, which
leave every byte of every view alone; buffers interchanged with the frame calls; the global-memory and the textured route, streams, the
array route; and what the statistics say."""
import ctypes as C
import types

import numpy as np
import pytest

import views_edge_cases as E
from test_gpu_views import COUNTERS, EARLY, _assert_views, _cam, _cameras, _np, _oracle, _render, _scene, _tensor_accum

pytestmark = pytest.mark.gpu

VIEWS_KIND = 6
NAME = "small_final"
SEED_OF = {0: 5, 1: 5, 2: 9}  # test_gpu_views.py's seeds of small_final's three views: the oracle frames are shared with it


def _extend(rt, name, views, spp, seeds, accum, done, size=None, **kw):
    cams, w, h = _cameras(name)
    if size is not None:
        w, h = size
    return _scene(rt, name).extendViews(w, h, [_cam(cams[v], spp) for v in views], accum, done, seeds=list(seeds), **kw)


def _extend_map(rt, name, views, cap, seeds, accum, targets, size=None, **kw):
    cams, w, h = _cameras(name)
    if size is not None:
        w, h = size
    return _scene(rt, name).extendViewsMap(w, h, [_cam(cams[v], cap) for v in views], accum, targets, seeds=list(seeds), **kw)


def _frames(orc, name, views, seeds, counts):
    """{count: (accum [K, rows, cols, 4], rgb [K, rows, cols, 3])} of the oracle, per view its own camera and seed"""
    return {c: (np.array([_oracle(orc, name, v, c, s)[0] for v, s in zip(views, seeds)]), np.array([_oracle(orc, name, v, c, s)[1] for v, s in zip(views, seeds)]))
            for c in counts}


def _mapped(frames, base, targets):
    """What a map makes of the buffer whose Counts are base[..., 0] (each a key of `frames`, or 11): every pixel the oracle's at its
    resulting Count -> (accum, rgb, the resulting Counts)."""
    count = base[..., 0]
    final = np.where(count == EARLY, EARLY, np.maximum(count, targets))
    acc, rgb = np.zeros_like(base), np.zeros(base.shape[:3] + (3,), np.uint8)
    for c in np.unique(final).tolist():
        src = frames[min(frames) if c == EARLY else c]  # (a pixel that stopped early is the same in every frame)
        sel = final == c
        acc[sel], rgb[sel] = src[0][sel], src[1][sel]
    assert np.array_equal(acc[..., 0], final)
    return acc, rgb, final


def _assert_same(got, want_acc, want_rgb, what=()):
    E.assert_batch(got, want_acc, want_rgb, what)


def _plan(rt, k, block, first_sample, mapped, chunk=None):
    p = rt.hooks.last_launch_plan()
    assert p["in"]["kind"] == VIEWS_KIND and p["in"]["n"] == k and p["in"]["first_sample"] == first_sample and p["in"]["map"] == int(mapped)
    o = p["out"]
    assert o["two_pass"] == 1 and o["error"] == 0 and o["q_block"] == block and o["B_mode"] == (9 if mapped else 2)
    assert o["A_grid"] == 0 and o["A_chunk"] == 0 and o["pairs"] > 0 and o["sort"] > 0
    if chunk:
        assert o["B_chunk"] == chunk
    return p


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(12, 13), (12, 40), (13, 40)])
@pytest.mark.parametrize("views", [(0, 1, 2), (0, 2, 1)], ids=["sky-last", "sky-in-the-middle"])
def test_mixed_views(rt, orc, views, a, b):
    """small_final at 49 x 33 with the scene's own camera, the off-centre one and the sky, which continues no pixel: an empty view last, and
    one in the middle of the list."""
    torch = pytest.importorskip("torch")
    A = rt._abi
    seeds = [SEED_OF[v] for v in views]
    _, w, h = _cameras(NAME)
    assert (2 * w + 1, 2 * h + 1) == (49, 33)
    want_a = [_oracle(orc, NAME, v, a, s) for v, s in zip(views, seeds)]
    want_b = [_oracle(orc, NAME, v, b, s) for v, s in zip(views, seeds)]
    sky = views.index(2)
    assert (want_a[sky][0][..., 0] == EARLY).all() and all((x[0][..., 0] == a).any() for i, x in enumerate(want_a) if i != sky)
    added = sum(int(y[0][..., 0].sum()) - int(x[0][..., 0].sum()) for x, y in zip(want_a, want_b))
    final = sum(int((x[0][..., 0] == EARLY).sum()) for x in want_a)
    for counters in (False, True):
        for block in (256, 1024):
            for chunk in (0, 1, 7):
                what = (views, a, b, counters, block, chunk)
                base = _render(rt, NAME, views, a, seeds, counters=counters, accum=_tensor_accum(torch, 3, w, h))
                _assert_views(base, orc, NAME, views, a, seeds, what=what)
                got = _extend(rt, NAME, views, b, seeds, base.accum, a, counters=counters, options=A.rt_render_options(block_threads=block, chunk_pixels=chunk))
                assert got.accum is base.accum
                _assert_views(got, orc, NAME, views, b, seeds, what=what)
                _plan(rt, 3, block, a, False, chunk)
                st = got.stats
                assert st["pixels"] == 3 * 1617 and st["samples"] == added and st["pixels_early"] == final and st["kernel_ms"] > 0.0, what
                for key in COUNTERS:
                    if not counters:
                        assert st[key] == 0
                    elif key != "aabb_tests":  # render(a) + extend(a -> b) is the oracle's render(b)
                        assert base.stats[key] + st[key] == sum(x[2][key] for x in want_b), (key,) + what


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,k,chunk", [(E.TINY, 70, 1), ((2, 1), 9, 0), (E.TINY, 25, 0)], ids=["3x3-70", "5x3-9", "3x3-25"])
@pytest.mark.parametrize("b", (13, 24))
def test_tiny_views(rt, orc, size, k, chunk, b):
    """More views than a wave has lanes with one-pixel units; 5 x 3 frames; 25 views, which go up in two launches of views_init_kernel."""
    torch = pytest.importorskip("torch")
    w, h, _, _ = E.dims(size)
    cams, seeds = E.batch(k)
    three_a, three_b = E.cameras(12), E.cameras(b)
    want_a, want_b = E.expected(orc, size, 12, cams, seeds), E.expected(orc, size, b, cams, seeds)
    for counters in (False, True):
        opts = rt._abi.rt_render_options(chunk_pixels=chunk)
        base = _scene(rt, NAME).renderViews(w, h, [three_a[c] for c in cams.tolist()], seeds=seeds.tolist(), counters=counters, accum=_tensor_accum(torch, k, w, h))
        E.assert_batch(base, want_a[0], want_a[1], ("base", k))
        got = _scene(rt, NAME).extendViews(w, h, [three_b[c] for c in cams.tolist()], base.accum, 12, seeds=seeds.tolist(), counters=counters, options=opts)
        E.assert_batch(got, want_b[0], want_b[1], (k, b, counters))
        _plan(rt, k, 1024, 12, False, chunk)
        assert got.stats["samples"] == want_b[2]["samples"] - want_a[2]["samples"] and got.stats["pixels_early"] == want_a[2]["pixels_early"]
        if counters:
            for key in E.COUNTERS:
                assert base.stats[key] + got.stats[key] == want_b[2][key], key
    # by map, every view to b but the views v % 5 == 3, which stay where they are
    targets = np.full(want_a[0].shape[:3], b, np.int32)
    targets[3::5] = 0
    frames = {12: want_a[:2], b: want_b[:2]}
    acc, rgb, _ = _mapped(frames, want_a[0], targets)
    base = _scene(rt, NAME).renderViews(w, h, [three_a[c] for c in cams.tolist()], seeds=seeds.tolist(), accum=_tensor_accum(torch, k, w, h))
    got = _scene(rt, NAME).extendViewsMap(w, h, [three_b[c] for c in cams.tolist()], base.accum, torch.from_numpy(targets).cuda(), seeds=seeds.tolist(),
                                          options=rt._abi.rt_render_options(chunk_pixels=chunk))
    E.assert_batch(got, acc, rgb, (k, b, "map"))
    _plan(rt, k, 1024, 12, True, chunk)


def test_more_views_than_the_ordering_has_cost_buckets_for(rt, orc):
    """4097 views of 3 x 3, 12 -> 13: the list is ordered by view alone (one key a view); expected values from views_edge_cases.table."""
    torch = pytest.importorskip("torch")
    k = 4097
    w, h, _, _ = E.dims(E.TINY)
    cams, seeds = E.batch(k)
    three_a, three_b = E.cameras(12), E.cameras(13)
    want_a, want_b = E.expected(orc, E.TINY, 12, cams, seeds), E.expected(orc, E.TINY, 13, cams, seeds)
    base = _scene(rt, NAME).renderViews(w, h, [three_a[c] for c in cams.tolist()], seeds=seeds.tolist(), accum=_tensor_accum(torch, k, w, h))
    E.assert_batch(base, want_a[0], want_a[1], ("base", k))
    got = _scene(rt, NAME).extendViews(w, h, [three_b[c] for c in cams.tolist()], base.accum, 12, seeds=seeds.tolist())
    E.assert_batch(got, want_b[0], want_b[1], (k,))
    p = _plan(rt, k, 1024, 12, False)
    assert p["out"]["sort"] == (k * 2 * 4 + 15) // 16 * 16
    assert got.stats["samples"] == want_b[2]["samples"] - want_a[2]["samples"] and got.stats["pixels"] == k * 9


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
def test_a_map_with_a_budget_per_pixel(rt, orc):
    """Views (own, off-centre, own), seed 5 each; targets drawn per pixel from {0, 11, 12, 13, 24, 40, the pixel's Count}, cap 40; the middle
    view's targets are all at or below its Counts, so it has no entry in the middle of the list.  Then a second map, up to 40, on the
    first one's result."""
    torch = pytest.importorskip("torch")
    views, seeds, cap = (0, 1, 0), (5, 5, 5), 40
    _, w, h = _cameras(NAME)
    frames = _frames(orc, NAME, views, seeds, (12, 13, 24, 40))
    base_acc = frames[12][0]
    count = base_acc[..., 0]
    rng = np.random.default_rng(20240534)
    targets = rng.choice(np.array([0, 11, 12, 13, 24, 40, -1], np.int32), size=count.shape).astype(np.int32)
    targets = np.where(targets == -1, count, targets).astype(np.int32)
    targets[1] = np.minimum(targets[1], count[1])
    assert not ((targets[1] > count[1]) & (count[1] != EARLY)).any() and ((targets[0] > count[0]) & (count[0] == 12)).any()
    acc1, rgb1, final1 = _mapped(frames, base_acc, targets)
    assert set(np.unique(final1).tolist()) == {11, 12, 13, 24, 40} and np.array_equal(acc1[1], base_acc[1])
    targets2 = rng.choice(np.array([0, 13, 24, 40, -1], np.int32), size=count.shape).astype(np.int32)
    targets2 = np.where(targets2 == -1, final1, targets2).astype(np.int32)
    acc2, rgb2, final2 = _mapped(frames, acc1, targets2)
    assert (final2 >= final1).all() and (final2 > final1).any() and (final2[1] > final1[1]).any()
    for counters in (False, True):
        for block, chunk in ((1024, 0), (256, 7), (1024, 1)):
            opts = rt._abi.rt_render_options(block_threads=block, chunk_pixels=chunk)
            base = _render(rt, NAME, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
            got = _extend_map(rt, NAME, views, cap, seeds, base.accum, torch.from_numpy(targets).cuda(), counters=counters, options=opts)
            assert got.accum is base.accum
            _assert_same(got, acc1, rgb1, ("first map", counters, block, chunk))
            _plan(rt, 3, block, 12, True, chunk)
            st = got.stats
            assert st["pixels"] == 3 * 1617 and st["samples"] == int((final1 - count).sum()) and st["pixels_early"] == int((count == EARLY).sum())
            got = _extend_map(rt, NAME, views, cap, seeds, got.accum, torch.from_numpy(targets2).cuda(), counters=counters, options=opts)
            _assert_same(got, acc2, rgb2, ("second map", counters, block, chunk))
            assert got.stats["samples"] == int((final2 - final1).sum()) and got.stats["pixels_early"] == int((count == EARLY).sum())


@pytest.mark.parametrize("n1", (53, 54, 55))
def test_a_map_of_few_entries_around_a_unit(rt, orc, n1):
    """Exactly 10 pixels of view 0 and 53, 54 or 55 of view 1 are continued: 63, 64 or 65 list entries at chunk_pixels = 64, the end of view 0
    at entry 10.  (Pass B sizes a reservation by the entries left over twice the waves of the grid, so a list this short is handed out entry by
    entry whatever the unit size; reservations that span view ends are test_reservations_that_cross_view_ends' below.)"""
    torch = pytest.importorskip("torch")
    views, seeds, cap = (0, 1), (5, 5), 40
    _, w, h = _cameras(NAME)
    frames = _frames(orc, NAME, views, seeds, (12, 13, 24, 40))
    base_acc = frames[12][0]
    count = base_acc[..., 0]
    targets = np.zeros(count.shape, np.int32)
    for v, n in ((0, 10), (1, n1)):
        live = np.argwhere(count[v] == 12)
        assert len(live) > 3 * n
        for i, (r, c) in enumerate(live[::3][:n]):  # every third live pixel, budgets in turn
            targets[v, r, c] = (13, 24, 40)[i % 3]
    acc, rgb, final = _mapped(frames, base_acc, targets)
    assert int((final > count).sum()) == 10 + n1 and int((final[0] > count[0]).sum()) == 10
    for counters in (False, True):
        for block in (256, 1024):  # (at 1024 threads the plan halves a map's units until the waves' scratch fits the LDS beside the scene)
            base = _render(rt, NAME, views, 12, seeds, accum=_tensor_accum(torch, 2, w, h))
            got = _extend_map(rt, NAME, views, cap, seeds, base.accum, torch.from_numpy(targets).cuda(), counters=counters,
                              options=rt._abi.rt_render_options(chunk_pixels=64, block_threads=block))
            _assert_same(got, acc, rgb, (n1, counters, block))
            p = _plan(rt, 2, block, 12, True, 64 if block == 256 else None)
            assert p["in"]["s_chunk"] == 64 and p["out"]["B_chunk"] in (32, 64)
            assert got.stats["samples"] == int((final - count).sum())


def test_reservations_that_cross_view_ends(rt, orc):
    """views_edge_cases' batch of 16,384 views of 3 x 3 at blocks of 256 threads, one a CU, ranges of up to 64 entries: pass B's reservations
    provably span view ends (views_edge_cases.crossing_numbers, from the oracle's frames and the plan's total_waves alone), so restN and
    restFirst carry remainders into ranges of other views -- 12 -> 13 uniformly, and by a map whose views have budgets of their own."""
    torch = pytest.importorskip("torch")
    k = E.CROSS_K
    w, h, _, _ = E.dims(E.TINY)
    cams, seeds = E.batch(k)
    three_a, three_13, three_24 = E.cameras(12), E.cameras(13), E.cameras(24)
    want = {c: E.expected(orc, E.TINY, c, cams, seeds) for c in (12, 13, 24)}
    opts = rt._abi.rt_render_options(chunk_pixels=64, blocks_per_cu=1, block_threads=256)
    scene = _scene(rt, NAME)
    base = scene.renderViews(w, h, [three_a[c] for c in cams.tolist()], seeds=seeds.tolist(), accum=_tensor_accum(torch, k, w, h))
    E.assert_batch(base, want[12][0], want[12][1], ("base",))
    keep = base.accum.clone()
    got = scene.extendViews(w, h, [three_13[c] for c in cams.tolist()], base.accum, 12, seeds=seeds.tolist(), options=opts)
    E.assert_batch(got, want[13][0], want[13][1], ("uniform",))
    p = _plan(rt, k, 256, 12, False, 64)
    numbers = E.crossing_numbers(orc, E.TINY, 12, k, p["out"]["B_total_waves"], 64)  # (the live list of the extension is the list of a render at 12)
    assert numbers["holds"], numbers
    # by map: views in turn to 13, to 24, left alone
    targets = np.zeros(want[12][0].shape[:3], np.int32)
    targets[0::3], targets[1::3] = 13, 24
    acc, rgb, _ = _mapped({c: want[c][:2] for c in want}, want[12][0], targets)
    got = scene.extendViewsMap(w, h, [three_24[c] for c in cams.tolist()], keep, torch.from_numpy(targets).cuda(), seeds=seeds.tolist(), options=opts)
    E.assert_batch(got, acc, rgb, ("map",))
    _plan(rt, k, 256, 12, True, 64)


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def test_a_malformed_buffer_or_map_leaves_every_view_alone(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    views, seeds, b = (0, 1, 2), (5, 5, 9), 40
    cams, w, h = _cameras(NAME)
    scene = _scene(rt, NAME)
    base = _render(rt, NAME, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
    _assert_views(base, orc, NAME, views, 12, seeds)
    good = base.accum.clone()
    abi = (A.rt_camera * 3)(*[_cam(cams[v], b).to_abi() for v in views])
    keys = (C.c_uint64 * 3)(*seeds)
    stream = torch.cuda.current_stream().cuda_stream
    targets = torch.full((3, 33, 49), b, dtype=torch.int32, device="cuda")
    live = np.argwhere(_np(good)[1, ..., 0] == 12)[5]

    def uniform(acc, rgb, st):
        return rt.lib.rt_render_views_extend_device(scene.handle, abi, 3, w, h, keys, 0, 0, 0, 12, acc.data_ptr(), rgb.data_ptr(), stream, None, st)

    def mapped(acc, rgb, st, tg=targets):
        return rt.lib.rt_render_views_extend_map_device(scene.handle, abi, 3, w, h, keys, 0, 0, 0, tg.data_ptr(), acc.data_ptr(), rgb.data_ptr(), stream, None, st)

    bad_acc = good.clone()
    bad_acc[1, int(live[0]), int(live[1]), 0] = 7  # one pixel of the middle view
    bad_tg = targets.clone()
    bad_tg[1, int(live[0]), int(live[1])] = b + 1  # one target above the cap
    cases = [("Count 7, uniform", uniform, bad_acc, "accum is not a buffer of samples_done samples per pixel"),
             ("Count 7, by map", mapped, bad_acc, "accum or targets are not what the arguments say"),
             ("target above the cap", lambda acc, rgb, st: mapped(acc, rgb, st, bad_tg), good, "accum or targets are not what the arguments say")]
    for what, call, src, message in cases:
        for with_stats in (True, False):
            acc = src.clone()
            rgb = torch.full((3, 33, 49, 3), 0xA5, dtype=torch.uint8, device="cuda")
            st = A.rt_stats()
            rc = call(acc, rgb, C.byref(st) if with_stats else None)
            torch.cuda.synchronize()
            if with_stats:
                assert rc == A.RT_ERR_INVALID_ARGUMENT and message in rt.lib.rt_last_error().decode(), what
            else:
                assert rc == A.RT_OK, what  # (nothing waits for the device: the untouched buffers are the evidence)
            assert torch.equal(acc, src) and bool((rgb == 0xA5).all()), what
    # through the wrapper: RtError, and the tensor as it was
    acc = bad_acc.clone()
    with pytest.raises(rt.RtError) as e:
        _extend(rt, NAME, views, b, seeds, acc, 12)
    assert e.value.code == A.RT_ERR_INVALID_ARGUMENT and torch.equal(acc, bad_acc)
    # and the same buffers, put right, are continued
    rgb = torch.full((3, 33, 49, 3), 0xA5, dtype=torch.uint8, device="cuda")
    st = A.rt_stats()
    assert mapped(good, rgb, C.byref(st)) == A.RT_OK
    _assert_views(types.SimpleNamespace(accum=good, rgb=rgb), orc, NAME, views, b, seeds)


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_buffers_are_interchangeable_with_the_frame_calls(rt, orc):
    torch = pytest.importorskip("torch")
    views, seeds = (0, 1, 2), (5, 5, 9)
    cams, w, h = _cameras(NAME)
    scene = _scene(rt, NAME)
    # a slice the batch call continued (12 -> 13) is continued further by extend_rows with cameras[v] (13 -> 40)
    base = _render(rt, NAME, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
    mid = _extend(rt, NAME, views, 13, seeds, base.accum, 12)
    _assert_views(mid, orc, NAME, views, 13, seeds)
    ext = scene.extend_rows(w, h, _cam(cams[1], 40), mid.accum[1], 13, seed=5)
    want_acc, want_rgb, _ = _oracle(orc, NAME, 1, 40, 5)
    assert np.array_equal(_np(ext.accum), want_acc) and np.array_equal(_np(ext.rgb), want_rgb)
    for i in (0, 2):  # the neighbours stay at 13
        assert np.array_equal(_np(mid.accum[i]), _oracle(orc, NAME, views[i], 13, seeds[i])[0])
    # K frames of render_rows, stacked, are a batch's buffer
    stacked = np.stack([scene.render_rows(w, h, _cam(cams[v], 12), seed=s).accum for v, s in zip(views, seeds)])
    got = _extend(rt, NAME, views, 40, seeds, torch.from_numpy(stacked).cuda(), 12)
    _assert_views(got, orc, NAME, views, 40, seeds, what=("stacked frames",))
    got = _extend(rt, NAME, views, 40, seeds, stacked, 12)  # (and as an array: a copy is continued)
    _assert_views(got, orc, NAME, views, 40, seeds, what=("stacked frames, arrays",))
    assert got.accum is not stacked and np.array_equal(stacked[0], _oracle(orc, NAME, 0, 12, 5)[0])


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,resident,tex", [("many_spheres", 0, 0), ("earth_thumb", 1, 1)])
def test_every_scene_route(rt, orc, name, resident, tex):
    """The global-memory scene and the textured one, two cameras each: one uniform extension and one map."""
    torch = pytest.importorskip("torch")
    _, w, h = _cameras(name)
    info = _scene(rt, name).info()
    assert info["lds_resident"] == resident and (info["n_textures"] > 0) == bool(tex)
    views, seeds = (0, 1, 0), (5, 6, 7)
    rows, cols = 2 * h + 1, 2 * w + 1
    for counters in (False, True):
        base = _render(rt, name, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
        got = _extend(rt, name, views, 40, seeds, base.accum, 12, counters=counters)
        _assert_views(got, orc, name, views, 40, seeds, what=(counters,))
        assert rt.hooks.last_launch_plan()["out"]["q_tex"] == tex
    frames = _frames(orc, name, views, seeds, (12, 40))
    targets = np.random.default_rng(34).choice(np.array([0, 12, 40], np.int32), size=(3, rows, cols)).astype(np.int32)
    acc, rgb, final = _mapped(frames, frames[12][0], targets)
    assert (final == 40).any() and (final == 12).any()
    for counters in (False, True):
        base = _render(rt, name, views, 12, seeds, accum=_tensor_accum(torch, 3, w, h))
        got = _extend_map(rt, name, views, 40, seeds, base.accum, torch.from_numpy(targets).cuda(), counters=counters)
        _assert_same(got, acc, rgb, (name, "map", counters))
        assert rt.hooks.last_launch_plan()["out"]["B_mode"] == 9


def test_streams_and_arrays(rt, orc):
    torch = pytest.importorskip("torch")
    A = rt._abi
    cams, w, h = _cameras(NAME)
    scene = _scene(rt, NAME)
    prev = torch.cuda.current_device()
    # two batch extensions in flight on two streams, nothing waited for
    batches = [((0, 1, 2), (5, 5, 9)), ((2, 1, 0), (9, 5, 5))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for (vs, sd), st in zip(batches, streams):
        with torch.cuda.stream(st):
            base = _render(rt, NAME, vs, 12, sd, accum=_tensor_accum(torch, len(vs), w, h), stats=False)
            got.append(_extend(rt, NAME, vs, 40, sd, base.accum, 12, stats=False))
            assert got[-1].accum is base.accum and got[-1].stats is None and scene.last_stats is None
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for (vs, sd), g in zip(batches, got):
        assert g.rgb.is_cuda and g.rgb.dtype == torch.uint8 and tuple(g.rgb.shape) == (len(vs), 33, 49, 3)
        _assert_views(g, orc, NAME, vs, 40, sd)
    # the array route, with rgb (the wrapper) ...
    views, seeds = (0, 1, 2), (5, 5, 9)
    arr = _render(rt, NAME, views, 12, seeds)
    got = _extend(rt, NAME, views, 40, seeds, arr.accum, 12, counters=True)
    assert isinstance(got.accum, np.ndarray) and got.accum is not arr.accum
    _assert_views(got, orc, NAME, views, 40, seeds, what=("arrays",))
    _assert_views(arr, orc, NAME, views, 12, seeds, what=("the caller's array is left as it was",))
    # ... and without (the C ABI itself), uniform and by map
    abi = (A.rt_camera * 3)(*[_cam(cams[v], 40).to_abi() for v in views])
    keys = (C.c_uint64 * 3)(*seeds)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    acc = arr.accum.copy()
    assert rt.lib.rt_render_views_extend(scene.handle, abi, 3, w, h, keys, 0, 0, 0, 12, i32(acc), None, None) == A.RT_OK
    assert np.array_equal(acc, got.accum)
    acc = arr.accum.copy()
    targets = np.full((3, 33, 49), 40, np.int32)
    st = A.rt_stats()
    assert rt.lib.rt_render_views_extend_map(scene.handle, abi, 3, w, h, keys, 0, 0, 0, i32(targets), i32(acc), None, C.byref(st)) == A.RT_OK
    assert np.array_equal(acc, got.accum) and st.samples == got.stats["samples"] and st.pixels == 3 * 1617


# ---- 7 -----------------------------------------------------------------------------------------------------------------------
def test_the_statistics_describe_the_extension_alone(rt, orc):
    views, seeds, a, b = (0, 1, 2), (5, 5, 9), 13, 40
    want_a = [_oracle(orc, NAME, v, a, s) for v, s in zip(views, seeds)]
    want_b = [_oracle(orc, NAME, v, b, s) for v, s in zip(views, seeds)]
    arr = _render(rt, NAME, views, a, seeds, counters=True)
    got = _extend(rt, NAME, views, b, seeds, arr.accum, a, counters=True)
    st = got.stats
    n_live = sum(int((x[0][..., 0] == a).sum()) for x in want_a)
    assert st["pixels"] == 3 * 33 * 49
    assert st["samples"] == n_live * (b - a) == sum(x[2]["samples"] for x in want_b) - sum(x[2]["samples"] for x in want_a)
    assert st["pixels_early"] == 3 * 33 * 49 - n_live == sum(x[2]["pixels_early"] for x in want_b)
    for key in ("rays", "prim_tests", "reflections"):
        assert 0 < st[key] == sum(x[2][key] for x in want_b) - arr.stats[key], key
    assert st["kernel_ms"] > 0.0 and st["total_ms"] >= st["kernel_ms"]
