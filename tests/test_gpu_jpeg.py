"""LoadImage.fromResource on the device -- rt_decode_jpeg_device and its hooks (csrc/rt_jpeg_kernels.h): every case of
tests/golden/jpeg_cases.npz byte for byte PIL's decode, at the default subsequence size and at 4, 8 and 64 bytes; the earth map; the
plan (rounds, subsequences) showing that the synchronising loop really ran; refusals with the host decoder's status and an untouched
buffer; two decodes on two streams; a tensor through LoadImage; the earth scene rendered from the .jpg; the C consumer.  Every refusal
input here has been through tests/c/jpeg_table.cpp under AddressSanitizer on a CPU first (test_jpeg_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    good = {k[5:]: (z[k].tobytes(), z["rgb/" + k[5:]]) for k in z.files if k.startswith("jpeg/")}
    bad = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("bad/")}
    return good, bad


@pytest.fixture(scope="module")
def earth():
    return open(os.path.join(GOLDEN, "earthmap.jpg"), "rb").read(), np.load(os.path.join(GOLDEN, "earthmap_rgb.npz"))["rgb"]


def decode(rt, data, S, shape):
    """The hook into a tensor with 64 sentinel bytes behind the bitmap -> (status, bitmap as numpy, plan)."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    rc = rt.lib.rt_dev_decode_jpeg(0, data, len(data), S, buf.data_ptr(), n)
    got = buf.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), "bytes behind the bitmap were written"
    return rc, got[:n].reshape(shape), rt.hooks.last_jpeg_plan()


@pytest.mark.parametrize("S", [0, 4, 8, 64])
def test_every_case_equals_libjpeg(rt, cases, S):
    most = (0, None)
    for name, (data, want) in cases[0].items():
        rc, got, plan = decode(rt, data, S, want.shape)
        assert rc == 0, (name, rt.lib.rt_last_error())
        assert np.array_equal(got, want), name
        assert 1 <= plan["rounds"] <= plan["subsequences"] and plan["decodes"] >= plan["subsequences"], (name, plan)
        assert plan["subsequence_bytes"] == (S or 128) and plan["blocks"] > 0
        assert plan["boundaries"] == 0 or name.endswith("-r2"), (name, plan)
        most = max(most, (plan["rounds"], name))
    print(f"S={S or 128}: most rounds {most}")
    if S in (4, 8, 64):
        assert most[0] >= 3  # the loop is exercised


def test_noise_synchronises_slowly(rt, cases):
    """Noise at quality 95, 4:4:4, 40x56 in subsequences of 64 bytes: 20 rounds in the CPU run of the same rounds (tests/c/jpeg_table.cpp
    prints it); the device runs the same Jacobi rounds, so at least 2 in any case."""
    data, want = cases[0]["noise-40x56-444-q95-r0"]
    rc, got, plan = decode(rt, data, 64, want.shape)
    print(plan)
    assert rc == 0 and np.array_equal(got, want)
    assert 2 <= plan["rounds"] <= plan["subsequences"] == -(-plan_bytes(rt, data) // 64)


def plan_bytes(rt, data):
    """The clean stream's length: the entropy-coded bytes without the stuffed zeros and the restart markers."""
    n = rt.LoadImage.info(data)["entropy_bytes"]
    at = data.index(b"\xff\xda")
    ecs = data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):][:n]
    return n - ecs.count(b"\xff\x00") - 2 * sum(ecs.count(bytes([0xFF, 0xD0 + k])) for k in range(8))


@pytest.mark.parametrize("S", [0, 64, 128])
def test_the_earth_map(rt, earth, S):
    data, want = earth
    rc, got, plan = decode(rt, data, S, want.shape)
    print(plan)  # (recorded in NOTES.md, not asserted: the rounds at 128 bytes)
    assert rc == 0 and np.array_equal(got, want)
    assert plan["blocks"] == 24576 and plan["rounds"] <= plan["subsequences"] == -(-plan_bytes(rt, data) // (S or 128))


def test_refusals_have_the_host_status_and_leave_the_buffer(rt, cases):
    from test_jpeg_host import STREAM_REFUSALS, crafted
    made = crafted(cases)
    stream = {name: made[name] for name in STREAM_REFUSALS}  # a code not in its table, restart markers that do not fit the interval, ...
    for name, data in {**cases[1], **stream}.items():
        out = np.full(40 * 56 * 3, SENTINEL, np.uint8)
        host = rt.lib.rt_decode_jpeg(data, len(data), out.ctypes.data, out.size), rt.lib.rt_last_error()
        assert host[0] != 0 and (out == SENTINEL).all()
        for S in (0, 4, 64):
            rc, got, _ = decode(rt, data, S, (40, 56, 3))
            assert (rc, rt.lib.rt_last_error()) == host, (name, S)
            assert (got == SENTINEL).all(), (name, S)
        if name in STREAM_REFUSALS:
            assert STREAM_REFUSALS[name] in host[1].decode(), (name, host)
    # the product call: with stats the status, without them RT_OK and still nothing written
    import torch
    data = cases[1]["flipped"]
    buf = torch.full((40 * 56 * 3,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    st = rt._abi.rt_jpeg_stats()
    assert rt.lib.rt_decode_jpeg_device(0, data, len(data), buf.data_ptr(), buf.numel(), None, C.byref(st)) == rt._abi.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_decode_jpeg_device(0, data, len(data), buf.data_ptr(), buf.numel(), None, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_two_decodes_on_two_streams(rt, cases, earth):
    import torch
    (a, want_a), (b, want_b) = earth, cases[0]["noise-40x56-420-q95-r2"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out_a = torch.zeros(want_a.shape, dtype=torch.uint8, device="cuda:0")
    out_b = torch.zeros(want_b.shape, dtype=torch.uint8, device="cuda:0")
    for _ in range(2):
        assert rt.lib.rt_decode_jpeg_device(0, a, len(a), out_a.data_ptr(), out_a.numel(), s1.cuda_stream, None) == 0
        assert rt.lib.rt_decode_jpeg_device(0, b, len(b), out_b.data_ptr(), out_b.numel(), s2.cuda_stream, None) == 0
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(out_a.cpu().numpy(), want_a) and np.array_equal(out_b.cpu().numpy(), want_b)


def test_load_image_gives_a_tensor_or_an_array(rt, earth, tmp_path):
    import torch
    data, want = earth
    t = rt.LoadImage.fromFile(os.path.join(GOLDEN, "earthmap.jpg"), tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    a = rt.LoadImage.fromBytes(data)  # a GPU is visible: decoded there, returned as an array
    assert isinstance(a, np.ndarray) and np.array_equal(a, want)
    assert rt.hooks.last_jpeg_plan()["blocks"] == 24576
    assert np.array_equal(rt.LoadImage.fromBytes(data, device="host"), want)
    tex = rt.ParameterisedTexture.ofImage(t)  # comes back to the host: rt_texture.texels is a host pointer
    assert np.array_equal(tex.image, want[::-1])


def test_earth_scene_from_the_jpeg_renders_the_fixture(rt):
    g = scenes.golden("oracle_earth_thumb_seed3")
    objs, cam, w, h = scenes.earth_thumb(os.path.join(GOLDEN, "earthmap.jpg"))
    res = rt.Scene.make(objs).render_rows(w, h, cam, seed=int(g["seed"]))
    assert np.array_equal(res.accum, g["accum"]) and np.array_equal(res.rgb, g["rgb"])


def test_c_program_decodes_on_the_gpu(rt, tmp_path):
    from test_jpeg_smoke import run_jpeg_smoke
    text, _ = run_jpeg_smoke(tmp_path)
    assert "jpeg: decoded on the GPU" in text
