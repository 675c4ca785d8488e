"""The composer of tests/path_cases.py -- what rt_camera_paths / rt_trace_paths are held to -- held itself to three independent witnesses,
none of them the library: the oracle's whole-frame render (PixelStats of every pixel), the oracle's own Scene.traceRay (colour and
advanced generator), and the literal restatement of the F# lines, instrumented from outside (every record).  Then the coverage the GPU
tests' fixtures must keep, and three deliberate mistakes that the first witness must catch.  No GPU."""
import numpy as np
import pytest

import path_cases as pc
import scenes

SEED = 5


def _pixel_sums(paths, acc, n_px, spp):
    """Sum of each pixel's path colours over its first Count samples, next to the render's PixelStats."""
    count = acc[:, 0].astype(np.int64)
    col = paths.colour.reshape(n_px, spp, 3).astype(np.int64)
    taken = np.arange(spp)[None, :] < count[:, None]
    return (col * taken[:, :, None]).sum(1)


@pytest.mark.parametrize("name", ["all_materials", "small_final", "many_spheres"])
def test_path_colours_sum_to_the_oracles_pixel_stats_for_every_pixel(rt, orc, name):
    f = pc.frame(name)
    acc, _, st = f.oracle.render_rows(f.w, f.h, f.cam_abi, seed=SEED, threads=orc.hardware_threads())
    acc = acc.reshape(-1, 4)
    n_px = (2 * f.w + 1) * (2 * f.h + 1)
    assert len(acc) == n_px and f.paths.colour.shape == (n_px * f.spp, 3)
    assert set(np.unique(acc[:, 0]).tolist()) <= {11, f.spp} and (acc[:, 0] == f.spp).any()
    assert np.array_equal(_pixel_sums(f.paths, acc, n_px, f.spp), acc[:, 1:].astype(np.int64))  # every pixel, no exceptions
    # the counters of the samples the render took are the composer's over the same slots
    taken = (np.arange(f.spp)[None, :] < acc[:, 0:1]).reshape(-1)
    assert int(f.paths.n_vertices[taken].sum()) == st["reflections"] and int(taken.sum()) == st["samples"]


@pytest.mark.parametrize("mutant", ["colour_before", "limit_ge", "miss_keeps_colour"])
def test_a_wrong_composer_is_caught_by_the_pixel_stats(rt, orc, mutant):
    """colour_after taken before Reflection (a STOPPED path's result is its last vertex's colour_after), the limit at
    bounces >= maxCount, MISS returning the ray's colour: each changes some pixel's sums."""
    if mutant == "miss_keeps_colour":
        objs, cam, w, h = pc.lights_scene()
    else:
        objs, cam, w, h = scenes.all_materials(spp=12, depth=2, pixels=6)
    o = orc.OracleScene(objs)
    n_px = (2 * w + 1) * (2 * h + 1)
    spp = cam.SamplesPerPixel
    acc = o.render_rows(w, h, cam.to_abi(), seed=SEED, threads=4)[0].reshape(-1, 4)
    good = pc.camera_paths(orc, o, cam.to_abi(), w, h, SEED, np.arange(n_px), 0, spp)
    bad = pc.camera_paths(orc, o, cam.to_abi(), w, h, SEED, np.arange(n_px), 0, spp, mutant=mutant)
    assert np.array_equal(_pixel_sums(good, acc, n_px, spp), acc[:, 1:].astype(np.int64))
    assert not np.array_equal(_pixel_sums(bad, acc, n_px, spp), acc[:, 1:].astype(np.int64))


def test_ray_paths_are_the_oracles_trace_ray(rt, orc):
    objs, cam, w, h = scenes.all_materials()
    o = orc.OracleScene(objs)
    rays = scenes.random_rays(2000, 17)
    rays[::97, 3:] = 0.0  # Ray.make' gives ValueNone
    states = np.random.default_rng(3).integers(1, 2**31 - 1, size=(len(rays), 4), dtype=np.int64).astype(np.uint32)
    for depth in (0, 1, 7):
        got = pc.ray_paths(orc, o, rays, depth, rng=states)
        made = ~np.isnan(got.first_ray[:, 0])
        assert (~made).sum() == len(rays[::97]) and (got.end[~made] == pc.NO_RAY).all()
        col, adv = o.trace_ray(depth, got.first_ray[made], states[made])
        assert np.array_equal(got.colour[made], col) and np.array_equal(got.rng[made], adv)
        assert np.array_equal(got.rng[~made], states[~made]) and (got.colour[~made] == 0).all() and (got.n_vertices[~made] == 0).all()
        assert got.n_vertices.max() == depth + 1 and (got.end[got.n_vertices == depth + 1] != pc.MISS).all()


def test_every_record_is_the_literal_restatements(rt, orc, monkeypatch):
    """tests/fsharp_literal.py's trace_ray, watched from outside: its hit_object and its two reflections are wrapped, nothing in it is
    changed.  Every record of every slot of a 5 x 3 frame."""
    import fsharp_literal as L
    from test_oracle_vs_literal import literal_camera, to_literal
    objs, cam, _, _ = scenes.all_materials(spp=6, depth=5, pixels=6)
    w, h, seed, per = 2, 1, 11, 6
    lits = to_literal(objs)
    for i, d in enumerate(lits):
        d["index"] = i
    scene, lcam, stream_for = L.scene_make(lits), literal_camera(cam), L.make_stream_for(seed)
    want = pc.camera_paths(orc, orc.OracleScene(objs), cam.to_abi(), w, h, seed, np.arange(15), 0, per)
    log = []
    real_hit, real_plane, real_sphere = L.hit_object, L.plane_reflection, L.sphere_reflection

    def hit(s, ray):
        things = real_hit(s, ray)
        if things is not None:
            log.append({"index": things[0]["index"], "strike": things[1]})
        return things

    def watched(real):
        def reflection(obj, light, strike, rand):
            stop = real(obj, light, strike, rand)
            log[-1]["colour"] = light["Colour"] if stop is None else stop
            log[-1]["ray"] = None if stop is not None else list(light["Ray"].Origin) + list(light["Ray"].Vector)
            return stop
        return reflection

    monkeypatch.setattr(L, "hit_object", hit)
    monkeypatch.setattr(L, "plane_reflection", watched(real_plane))
    monkeypatch.setattr(L, "sphere_reflection", watched(real_sphere))
    seen_ends = set()
    for g in range(15):
        r, c = divmod(g, 5)
        for s in range(per):
            slot = g * per + s
            rand = stream_for(g, s)
            r1, r2 = rand.GetTwo()
            landing = ((float(c - w) + r1) * lcam["vw"]) / float(w)
            on_x = L.walk_along(L.Ray(lcam["xo"], lcam["xd"]), landing)
            end = L.walk_along_ray(on_x, lcam["yd"], ((float(h - r - 1) + r2) * lcam["vh"]) / float(h))
            ray = L.ray_make_prime(lcam["eye"], L.v_diff(end, lcam["eye"]))
            assert ray is not None
            del log[:]
            colour = L.trace_ray(lcam["depth"], scene, {"Ray": ray, "Colour": (255, 255, 255)}, rand)
            assert tuple(want.colour[slot]) == tuple(colour) and want.n_vertices[slot] == len(log)
            for j, v in enumerate(log):
                assert want.hit_index[slot, j] == v["index"] and pc.same_f64(want.strike[slot, j], v["strike"])
                assert tuple(want.colour_after[slot, j]) == tuple(v["colour"])
                assert pc.same_f64(want.ray_after[slot, j], [np.nan] * 6 if v["ray"] is None else v["ray"])
            assert (want.hit_index[slot, len(log):] == -1).all()
            seen_ends.add(int(want.end[slot]))
    assert {pc.STOPPED, pc.BOUNCE_LIMIT} <= seen_ends or want.n_vertices.max() >= 3


def test_the_fixtures_of_the_gpu_tests_cover_every_case(rt, orc):
    am, sf, ms = pc.frame("all_materials"), pc.frame("small_final"), pc.frame("many_spheres")
    lights = pc.lights_paths()
    ends = set()
    for p in (am.paths, sf.paths, ms.paths, lights, pc.no_ray_camera_paths(), pc.ray_fixture()[2]):
        ends |= set(np.unique(p.end).tolist())
    assert ends == {pc.MISS, pc.STOPPED, pc.BOUNCE_LIMIT, pc.NO_RAY}
    for f in (am, sf, ms):
        assert (f.paths.n_vertices == f.depth + 1).any()                   # some slot runs into the bounce limit's length
        assert (f.paths.n_vertices >= 2).mean() >= 0.5
        assert (f.paths.end == pc.MISS).sum() == 0                         # (each has a dome)
    truncated = (am.paths.n_vertices > 4).mean()
    assert 0.02 <= truncated <= 0.50, truncated                             # K = 4 cuts some paths and leaves most whole
    assert (lights.end == pc.MISS).any() and (lights.end == pc.STOPPED).any()  # MISS: a scene without a dome
    nr = pc.no_ray_camera_paths()
    assert (nr.end == pc.NO_RAY).any() and (nr.end != pc.NO_RAY).any()     # NO_RAY: a viewport through the eye
    assert np.isnan(nr.first_ray[nr.end == pc.NO_RAY]).all() and (nr.n_vertices[nr.end == pc.NO_RAY] == 0).all()
    rays, _, rp = pc.ray_fixture()
    assert (rp.end == pc.NO_RAY).sum() == (np.abs(rays[:, 3:]).sum(1) == 0).sum() > 0  # ... and a zero vector


def test_the_summary_reducer_on_a_hand_made_case():
    nv = np.array([0, 3, 1, 2], np.int32)
    end = np.array([pc.NO_RAY, pc.BOUNCE_LIMIT, pc.STOPPED, pc.MISS], np.int32)
    colour = np.array([[0, 0, 0], [205, 105, 180], [10, 20, 30], [0, 0, 0]], np.uint8)
    c0 = np.array([[9, 9, 9], [100, 101, 102], [10, 20, 30], [1, 2, 3]], np.uint8)
    s = pc.summary(nv, end, colour, c0, 2, 2)
    assert s.tolist() == [[2, 3, 3, 0, 0, 1, 1, 1, 100, 101, 102, 0, 2, 205, 105, 180],
                          [2, 3, 2, 1, 1, 0, 0, 2, 11, 22, 33, 0, 2, 10, 20, 30]]
