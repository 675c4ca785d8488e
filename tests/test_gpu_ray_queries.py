"""Scene.hitObject and Scene.traceRays -- the render kernel's ray-list modes -- against the CPU oracle, bit for bit.  The oracle is
given orc.ray_make(origin, vector) of the same inputs; the product the raw inputs, with vectors scaled by random factors from 1e-3
to 1e3, so that Ray.make' on the device is checked too."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import scenes
from test_ray_queries_host import build_ray_query_smoke

pytestmark = pytest.mark.gpu


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _scaled(rays, seed):
    """The caller's form of `rays` (unit directions): vectors scaled by 10^U(-3, 3)."""
    rng = np.random.default_rng(seed)
    out = np.array(rays, np.float64)
    out[:, 3:] *= (10.0 ** rng.uniform(-3.0, 3.0, len(out)))[:, None]
    return out


def _made(orc, raw):
    """Ray.make' of every raw ray on the host (the oracle): (made rays [m, 6], mask of the rays it accepts)."""
    ok = np.zeros(len(raw), bool)
    made = np.zeros_like(raw)
    for i, r in enumerate(raw):
        m = orc.ray_make(r[:3], r[3:])
        if m is not None:
            ok[i] = True
            made[i] = m
    return made[ok], ok


def _oracle_hits(orc, o, raw):
    made, ok = _made(orc, raw)
    hit = np.full(len(raw), -2, np.int32)
    strike = np.full((len(raw), 3), np.nan)
    h, s, c = o.hit_object(made)
    hit[ok], strike[ok] = h, s
    return hit, strike, c


def _oracle_trace(orc, o, raw, depth, rng):
    made, ok = _made(orc, raw)
    col = np.zeros((len(raw), 3), np.uint8)
    g = np.array(rng, np.uint32)
    c, r = o.trace_ray(depth, made, g[ok])
    col[ok], g[ok] = c, r
    return col, g


def _generator_rays(scene, n, seed):
    """test_gpu_parity.py::test_hit_object_through_the_hand_written_node_loop's rays: axis-aligned, in coordinate planes, from box
    corners, on box planes, 1e6 away -- plus vectors that are zero or below the Float tolerance (Ray.make' fails: -2)."""
    rng = np.random.default_rng(seed)
    _, _, boxes = scene.walk_tree()
    rays = scenes.random_rays(n, seed, origin_scale=5.0)
    k = n // 6
    rays[:k, 3:] = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], size=(k, 1))
    two = np.eye(3)[rng.integers(0, 3, k)] + np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], size=(k, 1))
    two[np.linalg.norm(two, axis=1) < 0.5] = [1.0, 1.0, 0.0]
    rays[k:2 * k, 3:] = two / np.linalg.norm(two, axis=1, keepdims=True)
    if len(boxes):
        b = boxes[rng.integers(0, len(boxes), 3 * k)]
        corner = np.stack([b[:, 0 + rng.integers(0, 2)], b[:, 2 + rng.integers(0, 2)], b[:, 4 + rng.integers(0, 2)]], axis=1)
        rays[:k, :3] = corner[:k]
        rays[2 * k:3 * k, :3] = corner[k:2 * k]
        rays[3 * k:4 * k, 1] = b[2 * k:, 2]
    rays[4 * k:5 * k, :3] *= 1e6
    raw = _scaled(rays, seed + 1)
    z = rng.choice(len(raw), 40, replace=False)
    raw[z[:20], 3:] = 0.0
    raw[z[20:], 3:] = rng.normal(size=(20, 3)) * 1e-5  # |v|^2 ~ 1e-10 < 1e-8
    return raw


def _hit_scenes():
    big = scenes.many_spheres(n=100000, seed=3)[0]
    return [("all_materials", scenes.all_materials()[0], 6000), ("small_final", scenes.small_final()[0], 6000),
            ("spheres_300", scenes.many_spheres(n=300, seed=5)[0], 6000), ("spheres_2600", scenes.many_spheres(n=2600)[0], 6000),
            ("spheres_100000", big, 3000)]


def test_hit_objects_equal_the_oracle(rt, orc):
    seen_placements = set()
    for name, objs, n in _hit_scenes():
        o = orc.OracleScene(objs)
        for tuned in (False, True):
            s = rt.Scene.make(objs)
            raw = _generator_rays(s, n, 17 + n)
            if tuned:
                s.tune_rays(_made(orc, raw[:4000])[0])
            seen_placements.add(s.info()["lds_resident"])
            h1, s1 = s.hitObject(raw)
            h0, s0 = s.hitObject(raw, counters=True)
            h2, s2, _ = _oracle_hits(orc, o, raw)
            assert np.array_equal(h1, h2) and _same_f64(s1, s2), (name, tuned)
            assert np.array_equal(h0, h2) and _same_f64(s0, s2), (name, tuned)
            assert (h2 == -2).sum() == 40 and 0.02 < np.mean(h2 >= 0), name
            if not tuned:  # the host variant without its optional output (the wrapper always passes one): 65 rays, one wave and one
                few, h3 = np.ascontiguousarray(raw[:65]), np.full(65, -9, np.int32)
                assert rt.lib.rt_hit_objects(s.handle, 0, 65, few.ctypes.data_as(C.POINTER(C.c_double)), 0, h3.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == 0
                assert np.array_equal(h3, h2[:65]), name
    assert seen_placements == {0, 1}


def test_hit_objects_count_what_the_reference_counts(rt, orc):
    for objs in (scenes.small_final()[0], scenes.many_spheres(n=2600)[0]):
        s, o = rt.Scene.make(objs, walk_tree="reference"), orc.OracleScene(objs)
        raw = _generator_rays(s, 5000, 5)
        h, _ = s.hitObject(raw, counters=True)
        st = s.last_stats
        h2, _, c = _oracle_hits(orc, o, raw)
        assert np.array_equal(h, h2)
        assert st["rays"] == (h2 != -2).sum()
        assert st["aabb_tests"] == int(c[:, 0].sum()) and st["prim_tests"] == int(c[:, 1].sum())
        assert st["samples"] == 0 and st["pixels"] == 0 and st["kernel_ms"] > 0.0


def _two_mirrors(rt):
    P, H, PS = rt.Point.make, rt.Hittable, rt.InfinitePlaneStyle
    up = rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0))
    return [H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(1.0, rt.Colour.White), P(0.0, 0.0, 5.0), up)),
            H.InfinitePlane(rt.InfinitePlane.make(PS.PureReflection(1.0, rt.Colour.White), P(0.0, 0.0, -5.0), up))]


def _camera_like_rays(n, seed, eye, spread=0.6, fwd=(0.0, 0.0, 1.0)):
    rng = np.random.default_rng(seed)
    d = np.asarray(fwd, np.float64) + rng.normal(size=(n, 3)) * spread
    return np.concatenate([np.tile(eye, (n, 1)), d], axis=1)


@pytest.mark.parametrize("depth", [0, 1, 7, 50])
def test_trace_rays_equal_the_oracle(rt, orc, depth):
    earth = scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])
    cases = [("all_materials", scenes.all_materials()[0], np.array([0.0, 0.3, -1.0]), (0.0, 0.0, 1.0)),
             ("earth", earth[0], np.array(earth[1].abi.view_origin[:]), tuple(earth[1].abi.view_dir[:])),
             ("mirrors", _two_mirrors(rt), np.array([0.0, 0.0, 0.0]), (0.0, 0.0, 1.0))]
    for name, objs, eye, fwd in cases:
        s, o = rt.Scene.make(objs), orc.OracleScene(objs)
        rays = np.concatenate([_camera_like_rays(3000, 7, eye, 0.3, fwd), scenes.random_rays(1000, 8, origin_scale=1.0)])
        if name == "mirrors":
            rays[:, 5] += np.sign(rays[:, 5]) * 0.2  # every ray meets a mirror
        raw = _scaled(rays, 9)
        raw[:10, 3:] = 0.0
        g = np.random.default_rng(10).integers(1, 2**32, size=(len(raw), 4), dtype=np.uint32)
        c1, r1 = s.traceRays(raw, depth, rng=g)
        c0, r0 = s.traceRays(raw, depth, rng=g, counters=True)
        c2, r2 = _oracle_trace(orc, o, raw, depth, g)
        assert np.array_equal(c1, c2) and np.array_equal(r1, r2), name
        assert np.array_equal(c0, c2) and np.array_equal(r0, r2), name
        assert (c2[:10] == 0).all() and np.array_equal(r2[:10], g[:10])
        if name == "mirrors":
            assert (c2[10:] == np.array(rt.Colour.HotPink, np.uint8)).all()
        elif depth >= 7:
            assert len(np.unique(c2, axis=0)) > 20


def test_trace_rays_streams_are_the_renders_keying(rt, orc):
    objs = scenes.all_materials()[0]
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    raw = _scaled(_camera_like_rays(4000, 3, np.array([0.0, 0.3, -1.0])), 4)
    seed, base, sample = 77, 1000, 5
    c1, r1 = s.traceRays(raw, 12, seed=seed, stream_base=base, sample=sample)
    assert r1 is None
    g = orc.stream_state(seed, np.arange(base, base + len(raw), dtype=np.uint64), np.full(len(raw), sample, np.uint32))
    c2, _ = _oracle_trace(orc, o, raw, 12, g)
    assert np.array_equal(c1, c2)


def test_sizes_and_a_large_batch(rt, orc):
    objs = scenes.small_final()[0]
    s, o = rt.Scene.make(objs), orc.OracleScene(objs)
    eye = np.array([13.0, 2.0, 3.0])
    for n in (1, 63, 64, 65, 127, 129):  # (64 rays per run of the queue by default: chunk - 1 and + 1 are 63 and 65)
        raw = _scaled(_camera_like_rays(n, n, eye, spread=0.3) * np.array([1, 1, 1, -1, -1, -1.0]), n)
        g = np.random.default_rng(n).integers(1, 2**32, size=(n, 4), dtype=np.uint32)
        c1, r1 = s.traceRays(raw, 50, rng=g)
        c2, r2 = _oracle_trace(orc, o, raw, 50, g)
        assert np.array_equal(c1, c2) and np.array_equal(r1, r2), n
        h1, s1 = s.hitObject(raw)
        h2, s2, _ = _oracle_hits(orc, o, raw)
        assert np.array_equal(h1, h2) and _same_f64(s1, s2), n
    n = 3_000_000
    rng = np.random.default_rng(1)
    raw = np.concatenate([np.tile(eye, (n, 1)), -eye + rng.normal(size=(n, 3)) * 3.0], axis=1)
    c1, _ = s.traceRays(raw, 50, seed=9)
    c0, _ = s.traceRays(raw, 50, seed=9, counters=True)
    assert np.array_equal(c0, c1)
    assert s.last_stats["rays"] > n
    sub = rng.choice(n, 200_000, replace=False)
    g = orc.stream_state(9, sub.astype(np.uint64), np.zeros(len(sub), np.uint32))
    c2, _ = _oracle_trace(orc, o, raw[sub], 50, g)
    assert np.array_equal(c1[sub], c2)
    h1, s1 = s.hitObject(raw)
    assert (h1 >= 0).mean() > 0.5
    h2, s2, _ = _oracle_hits(orc, o, raw[sub])
    assert np.array_equal(h1[sub], h2) and _same_f64(s1[sub], s2)


def test_launch_settings_do_not_change_results(rt):
    torch = pytest.importorskip("torch")
    A = rt._abi
    for objs in (scenes.all_materials()[0], scenes.many_spheres(n=2600)[0]):
        s = rt.Scene.make(objs)
        raw = _scaled(_camera_like_rays(20000, 2, np.array([0.0, 1.5, -6.0])), 3)
        r = torch.from_numpy(raw).cuda()
        g = torch.from_numpy(np.random.default_rng(4).integers(1, 2**31, size=(len(raw), 4), dtype=np.int64).astype(np.int32)).cuda()
        runs = []
        for opt in (None, A.rt_render_options(block_threads=256), A.rt_render_options(block_threads=1024),
                    A.rt_render_options(chunk_pixels=16), A.rt_render_options(park_lanes=-1)):
            c, gg = s.traceRays(r, 8, rng=g, options=opt)
            h, sk = s.hitObject(r, options=opt)
            runs.append([x.cpu().numpy() for x in (c, gg, h, sk)])
        for other in runs[1:]:
            assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(runs[0], other))


def test_device_path_on_streams(rt):
    torch = pytest.importorskip("torch")
    objs = scenes.small_final()[0]
    s = rt.Scene.make(objs)
    raw = [_scaled(_camera_like_rays(50000, k, np.array([13.0, 2.0, 3.0])) * np.array([1, 1, 1, -1, -1, -1.0]), k) for k in (1, 2)]
    want = [s.traceRays(r, 50, seed=3, stream_base=7) for r in raw]
    want_hit = s.hitObject(raw[0])
    prev = torch.cuda.current_device()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for r, st in zip(raw, streams):
        with torch.cuda.stream(st):
            t = torch.from_numpy(r).to("cuda", non_blocking=False)
            got.append(s.traceRays(t, 50, seed=3, stream_base=7, stats=False))  # both calls in flight
            assert s.last_stats is None
    with torch.cuda.stream(streams[0]):
        h, sk = s.hitObject(torch.from_numpy(raw[0]).cuda(), stats=False)
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == prev
    for (c, g), (wc, wg) in zip(got, want):
        assert g is None and wg is None
        assert np.array_equal(c.cpu().numpy(), wc)
    assert np.array_equal(h.cpu().numpy(), want_hit[0]) and _same_f64(sk.cpu().numpy(), want_hit[1])
    g0 = torch.from_numpy(np.random.default_rng(1).integers(1, 2**32, size=(50000, 4), dtype=np.uint32)).cuda()
    c, g1 = s.traceRays(torch.from_numpy(raw[0]).cuda(), 50, rng=g0)
    wc, wg = s.traceRays(raw[0], 50, rng=g0.cpu().numpy())
    assert np.array_equal(c.cpu().numpy(), wc) and np.array_equal(g1.cpu().numpy(), wg)
    assert s.last_stats["kernel_ms"] > 0.0


def _smoke_scene(rt):
    P, S, PS, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.InfinitePlaneStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return [H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0)),
            H.Sphere(rt.Sphere.make(S.Glass(1.0, Tex(rt.Colour.White), 1.5), P(1.5, 0.0, 4.0), 0.7)),
            H.InfinitePlane(rt.InfinitePlane.make(PS.FuzzedReflection(0.9, Px(180, 200, 220), 0.2), P(0.0, -1.0, 0.0), rt.Vector.make(0.0, 1.0, 0.0))),
            H.UnboundedSphere(rt.Sphere.make(S.LightSource(Tex(Px(230, 230, 255))), P(0.0, 0.0, 0.0), 100.0))]


def test_c_program_queries_equal_the_oracle(rt, orc, tmp_path):
    out = subprocess.run([build_ray_query_smoke(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ray queries: traced 8 rays on the GPU" in out.stdout
    lines = [ln.split() for ln in out.stdout.splitlines()]
    hit = np.array([int(ln[2]) for ln in lines if ln[0] == "hit"])
    strike = np.array([[float.fromhex(x) for x in ln[3:6]] for ln in lines if ln[0] == "hit"])
    trace = np.array([[int(x) for x in ln[2:]] for ln in lines if ln[0] == "trace"])
    stream = np.array([[int(x) for x in ln[2:]] for ln in lines if ln[0] == "stream"])
    raw = np.array([[0, 0, 0, 0, 0, 1], [0, 0, 0, 1.5, 0, 4], [0, 0, 0, 0, -2, 5], [0, 0, 0, 0, 1, 0], [0.3, 0.2, -1, 0, 0, 250],
                    [5, 0, 3, -1e-3, 0, 0], [1.5, 0, 4, 0, 0, 1], [0, 0, 0, 1e-5, 0, 0]], np.float64)
    o = orc.OracleScene(_smoke_scene(rt))
    h2, s2, _ = _oracle_hits(orc, o, raw)
    assert np.array_equal(hit, h2) and _same_f64(strike, s2)
    assert list(h2[[0, 1, 7]]) == [0, 1, -2]
    g = np.array([[11 + i, 7 * i + 3, 12345, 999] for i in range(8)], np.uint32)
    c2, r2 = _oracle_trace(orc, o, raw, 10, g)
    assert np.array_equal(trace[:, :3], c2) and np.array_equal(trace[:, 3:], r2)
    gs = orc.stream_state(5, np.arange(100, 108, dtype=np.uint64), np.full(8, 2, np.uint32))
    c3, _ = _oracle_trace(orc, o, raw, 10, gs)
    assert np.array_equal(stream, c3)
