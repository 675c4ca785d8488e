"""Image textures from device memory on the GPU: rt_scene_create_textures / rt_scene_create_device_textures, of_image_kernel, the lazy host
copy of the texels, rt_scene_set_texels_device and rt_of_image_device -- every comparison against the scene the existing calls make from
the same texels on the host (ParameterisedTexture.ofImage's numpy rows), byte for byte and pixel for pixel.  Images are seeded noise, so
every row differs.  The rules themselves ran on a CPU under AddressSanitizer first (tests/test_texture_plan_cpp.py)."""
import ctypes as C
import dataclasses
import functools
import os

import numpy as np
import pytest

import scenes
import texture_cases as tc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(1, 1), (1, 5), (5, 1), (3, 2), (17, 9), (64, 33)]  # (width, height); 17 wide: 51-byte rows
TRIPLES = [(SIZES[0], SIZES[4], SIZES[1]), (SIZES[2], SIZES[3], SIZES[5]), (SIZES[5], SIZES[0], SIZES[4])]
PT = tc.PT


def noise(w, h, salt):
    return np.random.default_rng(1000 + salt).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gpu(a, odd=False):
    """The array as a uint8 tensor on cuda:0; odd: a slice of a larger tensor that starts at an odd address."""
    import torch
    a = np.array(a, dtype=np.uint8, order="C")  # (a copy: a reversed view of one row keeps its negative stride otherwise)
    if not odd:
        return torch.from_numpy(a).cuda()
    flat = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda:0")
    flat[1:] = torch.from_numpy(a.reshape(-1)).cuda()
    t = flat[1:].view(a.shape)
    assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    return t


def objects(images, wrap):
    """Six wearers: three images (wrap(bitmap top first, k) -> a ParameterisedTexture), a Checkered over the first two, a Colour, a UvRamp;
    and the sky.  -> (objects, the three image textures)"""
    tex = [wrap(img, k) for k, img in enumerate(images)]
    params = tex + [PT.Checkered(tex[0], tex[1], 7.0), PT.Colour(tc.colour_of(5)), PT.UvRamp("u", 9, "v")]
    return [tc.wear(i, p) for i, p in enumerate(params)] + [tc.sky()], tex


def host_wrap(img, k):
    return PT.ofImage(img)


def blob_and_image(rt, scene):
    texels, offs = rt.hooks.scene_texels(scene)
    return texels, offs, rt.hooks.scene_image(scene)[0]


def cam(rt):
    return dataclasses.replace(rt.Camera.makeBasic(12, 2.0, 2.0, scenes.P(20.0, 0.5, -30.0), scenes.unit(0.0, 0.0, 1.0), scenes.V(0.0, 1.0, 0.0)), BounceDepth=4)


def frame(rt, scene, counters=False, seed=3):
    r = scene.render_rows(24, 8, cam(rt), seed=seed, counters=counters)
    return r.accum, r.rgb


def same_frame(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. blob equality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", range(len(TRIPLES)))
@pytest.mark.parametrize("form", ["top_first", "reversed", "odd_pointer"])
def test_the_blob_is_the_host_made_scenes(rt, triple, form):
    images = [noise(w, h, 10 * triple + k) for k, (w, h) in enumerate(TRIPLES[triple])]
    want = blob_and_image(rt, rt.Scene.make(objects(images, host_wrap)[0]))
    if form == "reversed":  # rows already img.[y]: through the raw call, which alone can say so
        objs, tex = objects(images, lambda img, k: PT.ofImageDevice(gpu(img[::-1])))
        rec, table = rt.hittable_records(objs, textures=True)
        for q in table.sources:
            q.flags = 0
        scene = rt.Scene.make_device(rec, table)
    else:
        objs, tex = objects(images, lambda img, k: PT.ofImageDevice(gpu(img, odd=(form == "odd_pointer"))))
        scene = rt.Scene.make(objs)
    plan = rt.hooks.texture_plan()
    got = blob_and_image(rt, scene)
    t = TRIPLES[triple]
    blob = sum((w * h * 3 + 15) // 16 * 16 for w, h in t + t[:2])  # the first two images once more, as the Checkered's children
    assert scene.info()["texel_bytes"] == blob == got[0].size == want[0].size
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert plan == {"textures": 8, "images": 5, "device_sourced": 5, "jpeg_sourced": 0, "blob_bytes": blob, "launches": 1,
                    "bytes_host_to_device": 0, "bytes_device_to_host": 0}
    assert [scene.texture_index(t) for t in tex] == [0, 1, 2]


# ---- 2. mixed sources -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpegs():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    good = {k[5:]: (z[k].tobytes(), z["rgb/" + k[5:]]) for k in z.files if k.startswith("jpeg/")}
    bad = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("bad/")}
    return good, bad


JPEGS = ("noise-1x1-444-q95-r0", "noise-17x33-420-q95-r0", "noise-40x56-422-q95-r2")  # 1x1; odd-sized 4:2:0; restart markers


def test_record_device_and_jpeg_sources_in_one_table(rt, jpegs):
    good = jpegs[0]
    files = [good[n] for n in JPEGS]
    plain = [noise(5, 3, 1), noise(17, 9, 2)]
    params = [PT.ofImage(plain[0]), PT.ofImageDevice(gpu(plain[1], odd=True))] + [PT.ofJpeg(data) for data, _ in files] + [PT.Colour(tc.colour_of(1))]
    objs = [tc.wear(i, p) for i, p in enumerate(params)] + [tc.sky()]
    scene = rt.Scene.make(objs)
    plan = rt.hooks.texture_plan()
    texels, offs = rt.hooks.scene_texels(scene)
    bitmaps = plain + [rgb for _, rgb in files]  # PIL's recorded decode for the files
    at = 0
    for k, rgb in enumerate(bitmaps):
        n = rgb.size
        assert offs[k] == at and np.array_equal(texels[at:at + n], rgb[::-1].reshape(-1)), k
        pad = (n + 15) // 16 * 16
        assert not texels[at + n:at + pad].any()
        at += pad
    assert offs[5] == 0xFFFFFFFF and at == texels.size == scene.info()["texel_bytes"]
    assert (plan["images"], plan["device_sourced"], plan["jpeg_sourced"], plan["launches"]) == (5, 1, 3, 1)
    assert plan["bytes_host_to_device"] == plain[0].size and plan["bytes_device_to_host"] == 0
    want = rt.Scene.make([tc.wear(i, p) for i, p in enumerate([PT.ofImage(b) for b in bitmaps] + [params[-1]])] + [tc.sky()])
    assert np.array_equal(rt.hooks.scene_texels(want)[0], texels) and same_frame(frame(rt, scene), frame(rt, want))


# ---- 3. evaluation and renders ----------------------------------------------------------------------------------------------------
def test_texture_evaluation_equals_the_host_made_scene(rt):
    images = [noise(w, h, 40 + k) for k, (w, h) in enumerate(TRIPLES[1])]
    host = rt.Scene.make(objects(images, host_wrap)[0])
    dev = rt.Scene.make(objects(images, lambda img, k: PT.ofImageDevice(gpu(img)))[0])
    grid = np.array([0.0, 1e-9, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.999999, 1.0])
    u, v = (a.reshape(-1) for a in np.meshgrid(grid, grid, indexing="ij"))
    for texture, wearer in ((0, 0), (1, 1), (2, 2), (5, 3)):
        pts = tc.plane_map(1.0, tc.centre_of(wearer), u, v)
        a, b = rt.hooks.texture_colour_at(host, texture, pts), rt.hooks.texture_colour_at(dev, texture, pts)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), texture


@functools.lru_cache(maxsize=None)
def earth_host():
    return scenes.earth_thumb(scenes.golden("earthmap_rgb")["rgb"])


@functools.lru_cache(maxsize=None)
def earth_oracle():
    import oracle as orc
    objs, cam_, w, h = earth_host()
    acc, rgb, _ = orc.OracleScene(objs).render_rows(w, h, cam_.to_abi(), seed=3, threads=8)
    return acc, rgb


def earth_device_objects(rt, source):
    objs, _, _, _ = rt.sample_images.earth_device(source)
    return objs


@pytest.mark.parametrize("source", ["path", "tensor"])
def test_the_earth_scene_renders_as_the_host_made_one_and_the_oracle(rt, source):
    import torch
    objs, cam_, w, h = earth_host()
    path = os.path.join(GOLDEN, "earthmap.jpg")
    given = path if source == "path" else torch.from_numpy(scenes.golden("earthmap_rgb")["rgb"]).cuda()
    dev, host = rt.Scene.make(earth_device_objects(rt, given)), rt.Scene.make(objs)
    assert dev.info() == host.info()
    for counters in (True, False):  # the counting and the timed kernel
        a, b = dev.render_rows(w, h, cam_, seed=3, counters=counters), host.render_rows(w, h, cam_, seed=3, counters=counters)
        assert np.array_equal(a.accum, b.accum) and np.array_equal(a.rgb, b.rgb)
        assert np.array_equal(a.accum, earth_oracle()[0]) and np.array_equal(a.rgb, earth_oracle()[1])
    g = scenes.golden("oracle_earth_thumb_seed3")
    assert np.array_equal(a.accum, g["accum"]) and np.array_equal(a.rgb, g["rgb"])


def padded_earth(rt, objs):
    """earth's two objects and 900 small spheres behind the camera: more than the LDS holds"""
    objs = list(objs)
    rng = np.random.default_rng(4)
    S, H = rt.SphereStyle, rt.Hittable
    pad = [H.Sphere(rt.Sphere.make(S.LambertReflection(0.5, rt.Texture.Colour(tc.colour_of(i))),
                                   scenes.P(40.0 + rng.uniform(0, 30), rng.uniform(-10, 10), -20.0 + rng.uniform(0, 30)), 0.05)) for i in range(900)]
    return objs + pad


def test_make_device_with_a_scene_beyond_the_lds(rt, orc):
    objs, cam_, w, h = earth_host()
    host = rt.Scene.make(padded_earth(rt, objs))
    acc, rgb, _ = orc.OracleScene(padded_earth(rt, objs)).render_rows(w, h, cam_.to_abi(), seed=3, threads=8)
    assert host.info()["lds_resident"] == 0
    rec, table = rt.hittable_records(padded_earth(rt, earth_device_objects(rt, os.path.join(GOLDEN, "earthmap.jpg"))), textures=True)
    assert table.sources is not None and table.sources[0].kind == rt._abi.RT_TEXELS_JPEG
    import torch
    dev = rt.Scene.make_device(torch.from_numpy(rec.view(np.uint8).reshape(len(rec), -1)).cuda(), table)
    assert dev.info() == host.info() and np.array_equal(rt.hooks.scene_texels(dev)[0], rt.hooks.scene_texels(host)[0])
    for counters in (True, False):
        a, b = dev.render_rows(w, h, cam_, seed=3, counters=counters), host.render_rows(w, h, cam_, seed=3, counters=counters)
        assert np.array_equal(a.accum, b.accum) and np.array_equal(a.rgb, b.rgb)
        assert np.array_equal(a.accum, acc) and np.array_equal(a.rgb, rgb)


# ---- 4. the lazy mirror -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["make", "make_device"])
def test_the_texels_come_to_the_host_once_when_tuning_needs_the_mirror(rt, route):
    images = [noise(w, h, 70 + k) for k, (w, h) in enumerate(TRIPLES[2])]
    extra = [tc.wear(10 + i, PT.Colour(tc.colour_of(i))) for i in range(6)]  # (enough bounded spheres for the probe to log rays)
    host = rt.Scene.make(objects(images, host_wrap)[0] + extra)
    objs = objects(images, lambda img, k: PT.ofImageDevice(gpu(img)))[0] + extra
    if route == "make":
        dev = rt.Scene.make(objs)
    else:
        rec, table = rt.hittable_records(objs, textures=True)
        dev = rt.Scene.make_device(rec, table)
    blob = dev.info()["texel_bytes"]
    assert not rt.hooks.scene_has_host_mirror(dev) and rt.hooks.scene_has_host_mirror(host)
    assert same_frame(frame(rt, dev), frame(rt, host))
    assert not rt.hooks.scene_has_host_mirror(dev) and rt.hooks.texture_plan()["bytes_device_to_host"] == 0  # a render fetches nothing
    ti, th = dev.tune(24, 8, cam(rt), seed=3), host.tune(24, 8, cam(rt), seed=3)
    assert ti["tuned"] == th["tuned"] == 1 and ti["nodes_after"] == th["nodes_after"]
    assert rt.hooks.scene_has_host_mirror(dev)
    assert same_frame(frame(rt, dev, counters=True), frame(rt, host, counters=True)) and same_frame(frame(rt, dev), frame(rt, host))
    dev.tree(), dev.tune(24, 8, cam(rt), seed=4)
    plan = rt.hooks.texture_plan()
    assert plan["bytes_device_to_host"] == blob and plan["bytes_host_to_device"] == 0  # exactly one fetch, of the blob's size
    assert np.array_equal(rt.hooks.scene_texels(dev)[0], rt.hooks.scene_texels(host)[0])


# ---- 5. refusals that need a device ------------------------------------------------------------------------------------------------------
def raw_jpeg_scene(rt, data, width, height):
    A = rt._abi
    r = tc.rec_colour((0, 0, 0))
    r.kind, r.width, r.height = A.RT_TEXTURE_IMAGE, width, height
    tex = (A.rt_texture * 1)(r)
    src = (A.rt_texels_source * 1)(A.rt_texels_source(A.RT_TEXELS_JPEG, 0, C.cast(C.c_char_p(data), C.c_void_p), len(data)))
    hs = (A.rt_hittable * 1)(tc.raw_sphere(A.RT_SPHERE_LIGHT_SOURCE, (0, 0, 0), 1.0, 0))
    out = C.c_void_p(0x1234)
    rc = rt.lib.rt_scene_create_textures(hs, 1, tex, 1, src, None, 0, None, C.byref(out))
    return rc, (rt.lib.rt_last_error() or b"").decode(), out


def test_jpeg_refusals_and_a_good_create_after_them(rt, jpegs):
    good, bad = jpegs
    A = rt._abi
    data, rgb = good["noise-17x33-420-q95-r0"]
    h, w = rgb.shape[:2]
    rc, msg, out = raw_jpeg_scene(rt, data, w + 1, h)
    assert rc == A.RT_ERR_INVALID_ARGUMENT and msg == f"texture 0: the jpeg is {w} x {h}, the record {w + 1} x {h}" and out.value == 0x1234
    rc, msg, out = raw_jpeg_scene(rt, bad["progressive"], 8, 8)
    buf = np.zeros(1 << 16, np.uint8)
    assert rt.lib.rt_decode_jpeg(bad["progressive"], len(bad["progressive"]), buf.ctypes.data, buf.size) == rc == A.RT_ERR_UNSUPPORTED
    assert msg == "texture 0: " + rt.lib.rt_last_error().decode() and out.value == 0x1234
    # a damaged entropy-coded stream behind a good header: found by the decoder on the device; an ordinary error path
    flipped = bad["flipped"]
    info = rt.LoadImage.info(flipped)
    want_rc = rt.lib.rt_decode_jpeg(flipped, len(flipped), buf.ctypes.data, buf.size)
    want_msg = rt.lib.rt_last_error().decode()
    rc, msg, out = raw_jpeg_scene(rt, flipped, info["width"], info["height"])
    assert rc == want_rc == A.RT_ERR_INVALID_ARGUMENT and msg == want_msg and out.value == 0x1234
    rc, msg, out = raw_jpeg_scene(rt, data, w, h)
    assert rc == 0 and out.value != 0x1234
    scene = rt.Scene(out.value, [data])
    assert np.array_equal(rt.hooks.scene_texels(scene)[0][:rgb.size], rgb[::-1].reshape(-1))


def test_of_image_device_alone_and_in_place(rt):
    import torch
    for w, h in ((17, 9), (1, 1)):
        img = noise(w, h, 90)
        src = gpu(img, odd=True)
        dst = torch.full((img.size + 33,), 0xA5, dtype=torch.uint8, device="cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        assert rt.lib.rt_of_image_device(0, src.data_ptr(), w, h, dst.data_ptr() + 1, img.size, st) == 0
        got = dst.cpu().numpy()
        assert np.array_equal(got[1:1 + img.size], img[::-1].reshape(-1)) and (got[:1] == 0xA5).all() and (got[1 + img.size:] == 0xA5).all()
        before = src.cpu().numpy().copy()
        assert rt.lib.rt_of_image_device(0, src.data_ptr(), w, h, src.data_ptr(), img.size, st) == rt._abi.RT_ERR_INVALID_ARGUMENT
        assert b"in place" in rt.lib.rt_last_error() and np.array_equal(src.cpu().numpy(), before)


# ---- 6. set_image -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_first", [True, False])
@pytest.mark.parametrize("made", ["host", "device"])
def test_set_image_replaces_one_image_of_three(rt, top_first, made):
    images = [noise(w, h, 50 + k) for k, (w, h) in enumerate(TRIPLES[0])]
    wrap = host_wrap if made == "host" else (lambda img, k: PT.ofImageDevice(gpu(img)))
    scene = rt.Scene.make(objects(images, wrap)[0])
    before, offs = rt.hooks.scene_texels(scene)
    new = noise(*TRIPLES[0][1], 99)
    fresh = rt.Scene.make(objects([images[0], new, images[2]], host_wrap)[0])
    # record 1 is the second image; record 4 is the same image again as the Checkered's child -- replaced too, as the fresh scene has it
    for index in (1, 4):
        scene.set_image(index, gpu(new if top_first else new[::-1], odd=True), top_first=top_first)
    after = rt.hooks.scene_texels(scene)[0]
    assert np.array_equal(after, rt.hooks.scene_texels(fresh)[0]) and not np.array_equal(after, before)
    changed = np.flatnonzero(after != before)
    n = new.size
    assert all(any(offs[i] <= c < offs[i] + n for i in (1, 4)) for c in (changed.min(), changed.max()))  # the other images' ranges are untouched
    assert same_frame(frame(rt, scene), frame(rt, fresh))
    assert not rt.hooks.scene_has_host_mirror(scene)  # the host's texels are out of date: dropped
    # refusals leave the blob as it is
    import torch
    t = gpu(new)
    for index, bitmap, code in ((8, t, "range"), (-1, t, "range"), (5, t, "not an image")):
        with pytest.raises(rt.RtError) as e:
            scene.set_image(index, bitmap)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARGUMENT and code in str(e.value)
    assert rt.lib.rt_scene_set_texels_device(scene.handle, 1, 0, t.data_ptr(), n - 1, 1, None) == rt._abi.RT_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert np.array_equal(rt.hooks.scene_texels(scene)[0], after)
    # tune needs the host mirror: the swapped texels are what comes back, and what a second device copy would get
    extra_cam = cam(rt)
    a, b = scene.tune(24, 8, extra_cam, seed=3), fresh.tune(24, 8, extra_cam, seed=3)
    assert a["tuned"] == b["tuned"] and same_frame(frame(rt, scene), frame(rt, fresh)) and rt.hooks.scene_has_host_mirror(scene)
    assert np.array_equal(rt.hooks.scene_texels(scene)[0], after)


def test_two_swaps_on_one_stream_without_host_synchronisation(rt):
    import torch
    images = [noise(w, h, 60 + k) for k, (w, h) in enumerate(TRIPLES[0])]
    first, second = noise(*TRIPLES[0][0], 97), noise(*TRIPLES[0][0], 98)
    scene = rt.Scene.make(objects(images, lambda img, k: PT.ofImageDevice(gpu(img)))[0])
    want = [frame(rt, rt.Scene.make(objects([x, images[1], images[2]], host_wrap)[0])) for x in (first, second)]
    a, b = gpu(first), gpu(second)
    c = cam(rt)
    rows, cols = 17, 49
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = [torch.zeros((rows * cols, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
        for k, t in enumerate((a, b)):
            for index in (0, 3):
                scene.set_image(index, t)
            st = torch.cuda.current_stream().cuda_stream
            assert st == stream.cuda_stream
            rc = rt.lib.rt_render_device(scene.handle, C.byref(c.to_abi()), 24, 8, 3, 0, 0, 1, rows, 0, out[k].data_ptr(), None, st, None)
            assert rc == 0, rt.lib.rt_last_error()
    stream.synchronize()
    for k in range(2):
        assert np.array_equal(out[k].cpu().numpy().reshape(rows, cols, 4), want[k][0]), k
