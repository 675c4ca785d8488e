"""Scene.make on the device (rt_scene_create_device) against the routes that were there before it: the scene it returns is
rt_scene_create_gpu_trees' scene byte for byte (info, device image, both trees, the filter tree) and rt_scene_create_ex' with Branch boxes
equal as numbers; the encoder alone is encode_image byte for byte, also on a tuned n-ary tree; frames, counters and ray queries are the
host-made scene's; the host arrays stay on the device until something asks for them.  Every comparison is against the host route."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import scene_device_cases as sc
import scenes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def device_scene(rt, records, textures, walk_tree=None, tensor=True, stream=None):
    tex = rt.TextureTable(*textures) if textures else ()
    if not tensor:
        return rt.Scene.make_device(records, tex, walk_tree=walk_tree, device=0)
    t = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, rt.HITTABLE_DTYPE.itemsize).copy()).to("cuda:0")
    return rt.Scene.make_device(t, tex, walk_tree=walk_tree, stream=stream)


def same_arrays(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def host_made(rt):
    """name, walk -> (records, textures, rt_scene_create_gpu_trees' scene, rt_scene_create_ex' scene), each made once"""
    made = {}

    def get(name, walk="sah"):
        if (name, walk) not in made:
            records, textures = sc.CASES[name]()
            code, trees, text = sc.create("rt_scene_create_gpu_trees", records, textures, walk, device=0)
            assert code == 0, text
            code, ex, text = sc.create("rt_scene_create_ex", records, textures, walk)
            assert code == 0, text
            made[name, walk] = (records, textures, trees, ex)
        return made[name, walk]
    return get


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_scene_is_the_gpu_trees_scene_byte_for_byte(rt, host_made, name):
    for walk in ("sah", "reference"):
        records, textures, trees, ex = host_made(name, walk)
        want_image, want_off = rt.hooks.scene_image(trees)
        for tensor in (True, False):
            s = device_scene(rt, records, textures, walk, tensor)
            assert s.info() == trees.info() == ex.info(), (walk, tensor)
            image, off = rt.hooks.scene_image(s)
            assert np.array_equal(off, want_off), (walk, tensor, off, want_off)
            assert np.array_equal(image, want_image), (walk, tensor, np.flatnonzero(image != want_image)[:8])
            assert same_arrays(s.tree(), trees.tree()) and same_arrays(s.tree(), ex.tree()), (walk, tensor)
            assert same_arrays(s.walk_tree(), trees.walk_tree()), (walk, tensor)
            assert same_arrays(s.filter_tree(), trees.filter_tree()) and same_arrays(s.filter_tree(), ex.filter_tree()), (walk, tensor)
            # the host's surface-area builder: skip and prim the same, Branch boxes equal as numbers (its sign of a zero is std::nth_element's)
            (sk, pr, bx), (esk, epr, ebx) = s.walk_tree(), ex.walk_tree()
            assert np.array_equal(sk, esk) and np.array_equal(pr, epr) and np.array_equal(bx, ebx, equal_nan=True), (walk, tensor)


@pytest.mark.parametrize("name", ["final-485", "all-materials", "peel-64", "earth-thumb", "spheres-4097", "spheres-2", "objects-16384", "tiny-radii", "infinite-radius", "planes-only"])
def test_the_encoder_alone_is_encode_image(rt, host_made, name):
    ex = host_made(name)[3]
    want = rt.hooks.scene_image(ex)[0]
    assert np.array_equal(rt.hooks.encode_image(ex), want)


def test_the_encoder_is_encode_image_on_a_tuned_n_ary_tree(rt):
    objs, cam, w, h = scenes.small_final()
    records, textures = sc.from_objects(objs)
    ex = sc.create("rt_scene_create_ex", records, textures, "sah")[1]
    before = ex.info()["walk_tree_nodes"]
    info = ex.tune_rays(scenes.random_rays(4096, 3, 6.0))
    assert info["tuned"] == 1 and info["nodes_after"] < before  # thinned: nodes with more than two children
    want = rt.hooks.scene_image(ex)[0]
    assert np.array_equal(rt.hooks.encode_image(ex), want)


@pytest.mark.parametrize("bits", [1, 2, 3, 5])
def test_the_later_radix_passes_give_the_same_order_by_depth(rt, host_made, bits):
    """The product sorts the depth in passes of 8 bits, so only a tree of 256 levels takes a second one, and no builder makes such a tree.
    With narrower digits the 53 levels of the peel case take 6, 3, 2 and 2 passes: the later passes (a carried index, the two buffers in
    turn) against encode_image, byte for byte; and the tuned n-ary tree the same way."""
    for name in ("peel-64", "final-485"):
        ex = host_made(name)[3]
        assert np.array_equal(rt.hooks.encode_image(ex, digit_bits=bits), rt.hooks.scene_image(ex)[0]), name
    with pytest.raises(rt.RtError):
        rt.hooks.encode_image(host_made("peel-64")[3], digit_bits=9)


def test_every_scene_method_works_without_a_python_object_list(rt, host_made):
    """A Scene keeps no Python list of its objects on any route (only what its texture records point into), so a scene made from records
    has nothing to fetch or refuse: its getters, renders and queries are the host-made scene's."""
    records, textures, trees, ex = host_made("earth-thumb")
    s = device_scene(rt, records, textures, "sah")
    assert not hasattr(s, "_objects") and len(s._keep) == len(ex._keep) >= 1  # the texel array
    cam = scenes.all_materials()[1]
    assert s.info() == ex.info() and same_arrays(s.tree(), ex.tree()) and same_arrays(s.filter_tree(), ex.filter_tree())
    got, want = frame(rt, s, cam, True), frame(rt, ex, cam, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    rays = scenes.random_rays(33, 4, 2.0)
    assert same_arrays(s.hitObject(rays, device=0), ex.hitObject(rays, device=0))
    assert np.array_equal(s.traceRays(rays, 6, seed=3, device=0)[0], ex.traceRays(rays, 6, seed=3, device=0)[0])
    pix = np.array([0, 3 * 33 + 5, 10 * 33 + 16], np.int32)  # row * 33 + col
    a, b = s.renderPixels(16, 10, cam, pix, seed=2, device=0), ex.renderPixels(16, 10, cam, pix, seed=2, device=0)
    assert np.array_equal(a[0], b[0])
    assert s.tune_rays(rays)["nodes_after"] == ex.tune_rays(rays)["nodes_after"] and same_arrays(s.walk_tree(), ex.walk_tree())


def frame(rt, scene, cam, counters):
    cam = dataclasses.replace(cam, SamplesPerPixel=12, BounceDepth=8)
    r = scene.render_rows(16, 10, cam, seed=5, device=0, counters=counters)  # 33 x 21
    keys = ("rays", "aabb_tests", "prim_tests", "reflections", "samples", "pixels", "pixels_early")
    return r.accum, r.rgb, {k: r.stats[k] for k in keys}


@pytest.mark.parametrize("name", sc.RENDERED)
def test_frames_counters_and_ray_queries_are_the_host_made_scenes(rt, host_made, name):
    records, textures, trees, ex = host_made(name)
    s = device_scene(rt, records, textures, "sah")
    cam = scenes.all_materials()[1]
    for counters in (False, True):
        got, want = frame(rt, s, cam, counters), frame(rt, ex, cam, counters)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], counters
    rays = scenes.random_rays(65, 17, 6.0)
    (gi, gs), (wi, ws) = s.hitObject(rays, device=0), ex.hitObject(rays, device=0)
    assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint8), ws.view(np.uint8))
    assert not rt.hooks.scene_has_host_mirror(s)  # frames and ray queries need nothing of the host's arrays


def test_tuning_a_device_made_scene_gives_the_tuned_host_made_scene(rt, host_made):
    records, textures, trees, ex0 = host_made("final-485")
    objs, cam, w, h = scenes.small_final()
    s = device_scene(rt, records, textures, "sah")
    ex = sc.create("rt_scene_create_ex", records, textures, "sah")[1]
    assert not rt.hooks.scene_has_host_mirror(s)
    gi, wi = s.tune(w, h, cam, seed=1, device=0), ex.tune(w, h, cam, seed=1, device=0)
    drop = ("probe_ms", "build_ms")
    assert {k: v for k, v in gi.items() if k not in drop} == {k: v for k, v in wi.items() if k not in drop} and gi["tuned"] == 1
    assert rt.hooks.scene_has_host_mirror(s)
    assert s.info() == ex.info() and same_arrays(s.walk_tree(), ex.walk_tree()) and same_arrays(s.filter_tree(), ex.filter_tree())
    assert np.array_equal(rt.hooks.scene_image(s)[0], rt.hooks.scene_image(ex)[0])
    got, want = frame(rt, s, cam, True), frame(rt, ex, cam, True)
    assert np.array_equal(got[0], want[0]) and got[2] == want[2]


def test_the_host_arrays_stay_on_the_device_until_a_getter_asks(rt, host_made):
    records, textures, trees, ex = host_made("spheres-1026")
    s = device_scene(rt, records, textures, "sah")
    assert rt.hooks.scene_has_host_mirror(trees) and not rt.hooks.scene_has_host_mirror(s)
    assert s.info() == trees.info() and not rt.hooks.scene_has_host_mirror(s)  # rt_scene_get_info needs none of them
    frame(rt, s, scenes.all_materials()[1], False)
    rt.hooks.scene_image(s)
    assert not rt.hooks.scene_has_host_mirror(s)
    assert same_arrays(s.tree(), trees.tree()) and rt.hooks.scene_has_host_mirror(s)
    # and the hooks that translate hittable indices fetch them too
    s2 = device_scene(rt, records, textures, "sah")
    rays = scenes.random_rays(9, 2, 30.0)
    got, want = rt.hooks.hit_object(s2, rays), rt.hooks.hit_object(ex, rays)
    assert np.array_equal(got[0], want[0]) and rt.hooks.scene_has_host_mirror(s2)
    # nothing at all, or a NaN coordinate: the host's ground, the arrays are there from the start
    for name in ("empty", "nan-centre"):
        records, textures = sc.CASES[name]()
        assert rt.hooks.scene_has_host_mirror(device_scene(rt, records, textures))
    # fewer than 3 bounded spheres: the trivial tree is written on the device, nothing comes to the host
    for name in ("spheres-1", "spheres-2", "planes-only"):
        records, textures = sc.CASES[name]()
        assert not rt.hooks.scene_has_host_mirror(device_scene(rt, records, textures)), name


def test_two_builds_in_flight_on_two_streams_give_the_bytes_of_one(rt, host_made):
    a, b = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    ra, ta, trees_a, _ = host_made("spheres-4097")
    rb, tb, trees_b, _ = host_made("final-485")
    import threading
    out = {}

    def build(key, records, textures, stream):
        out[key] = device_scene(rt, records, textures, "sah", stream=stream.cuda_stream)
    torch.cuda.synchronize()
    threads = [threading.Thread(target=build, args=("a", ra, ta, a)), threading.Thread(target=build, args=("b", rb, tb, b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for key, trees in (("a", trees_a), ("b", trees_b)):
        assert np.array_equal(rt.hooks.scene_image(out[key])[0], rt.hooks.scene_image(trees)[0]), key
        assert same_arrays(out[key].walk_tree(), trees.walk_tree()) and same_arrays(out[key].tree(), trees.tree()), key


@pytest.mark.parametrize("name", sorted(sc.REFUSALS))
def test_refusals_are_rt_scene_create_exs(rt, name):
    records, textures = sc.REFUSALS[name]()
    code, scene, text = sc.create("rt_scene_create_ex", records, textures)
    assert code != 0 and scene is None
    for tensor in (True, False):
        with pytest.raises(rt.RtError) as e:
            device_scene(rt, records, textures, tensor=tensor)
        assert (e.value.code, e.value.message) == (code, text), tensor
