"""LoadImage.fromResource (RayTracing.App/LoadImage.fs:9-18) as far as it goes without a GPU: the host decoder rt_decode_jpeg and
rt_jpeg_get_info against PIL's decodes (tests/golden/jpeg_cases.npz, made by tests/golden/make_jpeg_cases.py: libjpeg-turbo is the
reference, never this project's decoder), every refusal with its status and text, the numpy model of the format and its mutants,
csrc/rt_jpeg.h driven alone -- the whole subsequence algorithm of the device route as a loop -- plainly and under the sanitizers, the
Python LoadImage and the refusals of the device calls."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import jpeg_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("rt_jpeg_get_info", "rt_decode_jpeg", "rt_decode_jpeg_device", "rt_dev_decode_jpeg", "rt_dev_last_jpeg_plan")
SENTINEL = 0xA5
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (31, 15), (40, 56), (3, 50)]


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    good = {k[5:]: (z[k].tobytes(), z["rgb/" + k[5:]]) for k in z.files if k.startswith("jpeg/")}
    bad = {k[4:]: z[k].tobytes() for k in z.files if k.startswith("bad/")}
    return good, bad


@pytest.fixture(scope="module")
def refusals():
    return json.load(open(os.path.join(GOLDEN, "jpeg_refusals.json")))


def host_decode(rt, data, shape=None, spare=64):
    """rt_decode_jpeg into a buffer of the bitmap's size and `spare` sentinel bytes -> (status, bitmap or None)."""
    if shape is None:
        i = rt._abi.rt_jpeg_info()
        rc = rt.lib.rt_jpeg_get_info(data, len(data), C.byref(i))
        if rc:
            shape = (40, 56, 3)
        else:
            shape = (i.height, i.width, 3)
    n = int(np.prod(shape))
    buf = np.full(n + spare, SENTINEL, np.uint8)
    rc = rt.lib.rt_decode_jpeg(data, len(data), buf.ctypes.data, n)
    assert (buf[n:] == SENTINEL).all(), "bytes behind the bitmap were written"
    if rc:
        assert (buf == SENTINEL).all(), "a refused file wrote into the bitmap"
        return rc, None
    return rc, buf[:n].reshape(shape)


def test_the_symbols_are_declared_exported_and_bound(rt):
    from ray_tracing_fsharp_amd import _lib

    header = open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    declared = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW:
        assert name in declared and hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    assert "#define RT_ABI_VERSION 7" in header and rt.lib.rt_abi_version() == 7  # symbols and two structs only
    assert rt.lib.rt_abi_sizeof(10) == C.sizeof(rt._abi.rt_jpeg_info) and rt.lib.rt_abi_sizeof(11) == C.sizeof(rt._abi.rt_jpeg_stats)


def test_the_grid_is_whole(cases):
    """Every sampling x restart x size combination, both contents, the extremes of quality, greyscale and optimised tables."""
    good, bad = cases
    for h, w in SIZES:
        for s in ("444", "422", "420"):
            for r in ("r0", "r2"):
                assert {f"noise-{h}x{w}-{s}-q95-{r}", f"noise-{h}x{w}-{s}-q30-{r}", f"earth-{h}x{w}-{s}-q75-{r}", f"earth-{h}x{w}-{s}-q95-{r}"} <= set(good)
    assert {"grey-9x20-q80", "grey-16x8-q80", "optimize-noise-40x56-420-q75", "optimize-earth-40x56-444-q90", "noise-40x56-420-q1-r0",
            "noise-40x56-420-q100-r0"} <= set(good)
    assert {"progressive", "cmyk", "flipped"} <= set(bad) and sum(k.startswith("cut-") for k in bad) >= 5


def test_host_decode_equals_libjpeg_for_every_case(rt, cases):
    for name, (data, want) in cases[0].items():
        rc, got = host_decode(rt, data, want.shape)
        assert rc == 0, (name, rt.lib.rt_last_error())
        assert np.array_equal(got, want), name


def test_host_decode_of_the_earth_map(rt):
    data = open(os.path.join(GOLDEN, "earthmap.jpg"), "rb").read()
    want = np.load(os.path.join(GOLDEN, "earthmap_rgb.npz"))["rgb"]
    rc, got = host_decode(rt, data, want.shape)
    assert rc == 0 and np.array_equal(got, want)
    assert rt.LoadImage.info(data) == {"width": 1024, "height": 512, "components": 3, "sampling": "4:4:4", "restart_interval": 0, "entropy_bytes": 160945}
    assert len(data) == 161345


def test_info_fields(rt, cases):
    A = rt._abi
    cls = {"444": A.RT_JPEG_444, "422": A.RT_JPEG_422, "420": A.RT_JPEG_420}
    for name, (data, want) in cases[0].items():
        i = A.rt_jpeg_info()
        assert rt.lib.rt_jpeg_get_info(data, len(data), C.byref(i)) == 0, name
        assert (i.height, i.width) == want.shape[:2], name
        sos = data.index(b"\xff\xda")
        assert i.entropy_bytes == len(data) - (sos + 2 + struct.unpack(">H", data[sos + 2:sos + 4])[0]) - 2, name  # up to the EOI
        if name.startswith("grey"):
            assert (i.components, i.sampling, i.restart_interval) == (1, A.RT_JPEG_GREY, 0)
            continue
        assert i.components == 3
        m = re.search(r"-(4\d\d)-q\d+(?:-(r\d))?$", name)
        assert i.sampling == cls[m.group(1)], name
        assert i.restart_interval == (2 if m.group(2) == "r2" else 0), name
    small = A.rt_jpeg_info()
    small.struct_size = 8
    data = cases[0]["grey-9x20-q80"][0]
    assert rt.lib.rt_jpeg_get_info(data, len(data), C.byref(small)) == A.RT_ERR_INVALID_ARGUMENT


def test_every_refusal_has_its_status_and_text(rt, cases, refusals):
    A = rt._abi
    seen = {}
    for name, data in cases[1].items():
        rc, _ = host_decode(rt, data)
        seen[name] = [rc, rt.lib.rt_last_error().decode()]
    assert seen["progressive"][0] == seen["cmyk"][0] == A.RT_ERR_UNSUPPORTED
    assert all(v[0] == A.RT_ERR_INVALID_ARGUMENT for k, v in seen.items() if k.startswith("cut-") or k == "flipped")
    assert seen == refusals["fixtures"]


def _patched(data, at, new):
    b = bytearray(data)
    b[at:at + len(new)] = new
    return bytes(b)


def crafted(cases):
    """Files made by editing one header field of a good one: name -> bytes."""
    good = cases[0]["noise-17x33-420-q95-r0"][0]
    sof, sos, dqt, dht = good.index(b"\xff\xc0"), good.index(b"\xff\xda"), good.index(b"\xff\xdb"), good.index(b"\xff\xc4")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    out = {
        "no-soi": b"\x00" + good[1:],
        "empty-after-soi": good[:2],
        "sof1": _patched(good, sof + 1, b"\xc1"),
        "sof9-arithmetic": _patched(good, sof + 1, b"\xc9"),
        "12-bit": _patched(good, sof + 4, b"\x0c"),
        "zero-height": _patched(good, sof + 5, b"\x00\x00"),
        "zero-width": _patched(good, sof + 7, b"\x00\x00"),
        "too-many-pixels": _patched(good, sof + 5, b"\xff\xff\xff\xff"),
        "two-components": _patched(good, sof + 9, b"\x02"),
        "sampling-4x1": _patched(good, sof + 11, b"\x41"),
        "sampling-chroma-2x1": _patched(good, sof + 14, b"\x21"),
        "16-bit-quantisers": _patched(good, dqt + 4, b"\x10"),
        "quantiser-undefined": _patched(good, sof + 12, b"\x03"),
        "huffman-undefined": _patched(good, sos + 6, b"\x33"),
        "component-undefined": _patched(good, sos + 5, b"\x09"),
        "scan-of-one-component": _patched(good, sos + 2, b"\x00\x08\x01\x01\x00\x00\x3f\x00") ,
        "spectral-selection": _patched(good, sos + 11, b"\x01"),
        "segment-past-the-end": _patched(good, dht + 2, b"\xff\xff"),
        "dht-overfull": _patched(good, dht + 5, b"\x03"),
        "adobe-rgb": good[:2] + adobe + b"\x00" + good[2:],
        "adobe-ycck": good[:2] + adobe + b"\x02" + good[2:],
        "second-scan": good[:-2] + good[sos:],
        "no-entropy-bytes": good[:sos + 14] + b"\xff\xd9",
        "restart-markers-without-dri": cases[0]["noise-17x33-420-q95-r2"][0].replace(b"\xff\xdd\x00\x04", b"\xff\xe5\x00\x04"),
        # 48 one bits in the entropy-coded data: no code is all ones
        "code-not-in-table": _patched(good, sos + 14 + 40, b"\xff\x00" * 6),
        # a restart interval of 2 MCUs declared in front of a scan without a marker, and one with its last marker taken out: the bitmap
        # would reset its DC sums where the file does not
        "dri-without-markers": good[:2] + b"\xff\xdd\x00\x04\x00\x02" + good[2:],
        "dri-too-few-markers": _without_last_marker(cases[0]["noise-17x33-420-q95-r2"][0]),
    }
    return out


def _without_last_marker(data):
    at = max(data.rfind(bytes([0xFF, 0xD0 + k])) for k in range(8))
    return data[:at] + data[at + 2:]


STREAM_REFUSALS = {  # crafted inputs whose fault is in the entropy-coded data -> what the text must say
    "code-not-in-table": "a code that is not in its Huffman table", "dri-without-markers": "the restart interval call for",
    "dri-too-few-markers": "the restart interval call for", "restart-markers-without-dri": "the restart interval call for",
    "no-entropy-bytes": "does not hold the blocks",
}


def test_crafted_refusals(rt, cases, refusals):
    A = rt._abi
    U, I = A.RT_ERR_UNSUPPORTED, A.RT_ERR_INVALID_ARGUMENT
    want = {"no-soi": I, "empty-after-soi": I, "sof1": U, "sof9-arithmetic": U, "12-bit": U, "zero-height": I, "zero-width": I, "too-many-pixels": I,
            "two-components": U, "sampling-4x1": U, "sampling-chroma-2x1": U, "16-bit-quantisers": U, "quantiser-undefined": I, "huffman-undefined": I,
            "component-undefined": I, "scan-of-one-component": U, "spectral-selection": U, "segment-past-the-end": I, "dht-overfull": I, "adobe-rgb": U,
            "adobe-ycck": U, "second-scan": U, "no-entropy-bytes": I, "restart-markers-without-dri": I, "code-not-in-table": I, "dri-without-markers": I,
            "dri-too-few-markers": I}
    seen = {}
    for name, data in crafted(cases).items():
        rc, _ = host_decode(rt, data)
        seen[name] = [rc, rt.lib.rt_last_error().decode()]
        assert rc == want[name], (name, seen[name])
    assert seen == refusals["crafted"]
    for name, text in STREAM_REFUSALS.items():  # each kind of stream error by its own words, whatever the JSON holds
        assert text in seen[name][1], (name, seen[name])
    assert "index past 63" in refusals["fixtures"]["flipped"][1]
    # an Adobe marker with the transform 1 is what a YCbCr file carries: the same bitmap
    good, rgb = cases[0]["noise-17x33-420-q95-r0"]
    rc, got = host_decode(rt, good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[2:], rgb.shape)
    assert rc == 0 and np.array_equal(got, rgb)
    # arguments
    out = np.full(16, SENTINEL, np.uint8)
    assert rt.lib.rt_decode_jpeg(None, 10, out.ctypes.data, 16) == I and rt.lib.rt_last_error() == b"data is NULL"
    assert rt.lib.rt_decode_jpeg(good, len(good), None, 16) == I and rt.lib.rt_last_error() == b"the output is NULL"
    assert rt.lib.rt_decode_jpeg(good, len(good), out.ctypes.data, 16) == I and rt.lib.rt_last_error() == b"jpeg: capacity 16 below the 1683 bytes of the bitmap"
    assert rt.lib.rt_decode_jpeg(good, 0, out.ctypes.data, 16) == I
    assert (out == SENTINEL).all()


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_equals_libjpeg_for_every_case(cases):
    for name, (data, want) in cases[0].items():
        assert np.array_equal(jm.to_rgb(data), want), name
    for name, data in cases[1].items():
        with pytest.raises(jm.Refused):
            jm.to_rgb(data)


@pytest.mark.parametrize("mutant", ["no-round", "duplicate", "plus8"])
def test_the_fixtures_catch_each_mutant(cases, mutant):
    caught = [name for name, (data, want) in cases[0].items() if not np.array_equal(jm.to_rgb(data, mutant), want)]
    print(mutant, "caught by", len(caught), "cases")
    assert caught
    if mutant != "no-round":  # the filters are not there at 4:4:4
        assert not any("-444-" in c or c.startswith("grey") for c in caught)
    if mutant == "plus8":
        assert all("-420-" in c for c in caught)


# ---- the header alone: tables, and the device route's algorithm as a loop ----------------------------------------------------------
def write_case_file(path, cases):
    good, bad = cases

    def blob(b):
        return struct.pack("<I", len(b)) + b

    out = [blob(n.encode()) + struct.pack("<I", 2 if n.startswith("cut-source") else 0) + blob(d) + blob(rgb.tobytes()) for n, (d, rgb) in good.items()]
    out += [blob(n.encode()) + struct.pack("<I", 1) + blob(d) + blob(b"") for n, d in bad.items()]
    out += [blob(n.encode()) + struct.pack("<I", 1) + blob(d) + blob(b"") for n, d in crafted(cases).items()]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(out))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "sanitizers"])
def test_subsequence_algorithm_alone(tmp_path, cases, refusals, flags):
    """tests/c/jpeg_table.cpp over csrc/rt_jpeg.h, a stand-alone program: the hand-computed tables, then every case, every refusal input
    and the cut file at EVERY prefix length through the synchronising rounds at 4, 8, 64 and the default bytes a subsequence -- equal
    bitmaps, equal statuses and texts, rounds <= subsequences, and no sanitizer report."""
    exe, case_file = str(tmp_path / "jpeg_table"), str(tmp_path / "cases.bin")
    write_case_file(case_file, cases)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "jpeg_table.cpp")])
    out = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "tables ok"
    n_good, n_bad = len(cases[0]), len(cases[1]) + len(crafted(cases))
    cut = len(cases[0]["cut-source-40x56-420-q75"][0])
    assert lines[-1] == f"cases ok {n_good} refusals ok {n_bad} prefixes ok {cut}"
    told = {m.group(1): [int(m.group(2)), m.group(3)] for m in (re.match(r"refused (\S+) (\d+) (.*)$", ln) for ln in lines) if m}
    assert told == {**refusals["fixtures"], **refusals["crafted"]}  # the texts of the library, through every subsequence size
    rounds = [ln for ln in lines if ln.startswith("rounds noise-40x56-444-q95-r0")]
    assert rounds and int(rounds[0].split()[2]) >= 3  # the loop is exercised: noise synchronises slowly
    print("\n".join(ln for ln in lines if ln.startswith(("rounds", "most"))))


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_load_image_on_the_host(rt, cases, tmp_path):
    data, want = cases[0]["earth-31x15-422-q95-r2"]
    assert np.array_equal(rt.LoadImage.fromBytes(data, device="host"), want)
    path = tmp_path / "x.jpg"
    path.write_bytes(data)
    got = rt.LoadImage.fromFile(str(path), device="host")
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    with pytest.raises(rt.RtError) as e:
        rt.LoadImage.fromBytes(cases[1]["progressive"], device="host")
    assert e.value.code == rt._abi.RT_ERR_UNSUPPORTED and "progressive" in e.value.message
    with pytest.raises(ValueError):
        rt.LoadImage.fromBytes(data, device="host", tensor=True)


def test_earth_scene_from_the_file_is_the_scene_from_the_bitmap(rt):
    """sample_images.earth / config5_mixed take a path: the same records and texels as from the decoded fixture."""
    bitmap = np.load(os.path.join(GOLDEN, "earthmap_rgb.npz"))["rgb"]
    path = os.path.join(GOLDEN, "earthmap.jpg")
    for make in (rt.sample_images.earth, lambda e: rt.sample_images.config5_mixed(e, spp=4, pixels=20)):
        a, b = make(path), make(bitmap)
        (ra, ta), (rb, tb) = rt.hittable_records(a[0], textures=True), rt.hittable_records(b[0], textures=True)
        assert np.array_equal(ra, rb) and a[1:] == b[1:] and ta.count == tb.count
        ka, kb = [k for k in ta.keep if isinstance(k, np.ndarray)], [k for k in tb.keep if isinstance(k, np.ndarray)]
        assert len(ka) == len(kb) >= 1 and all(np.array_equal(x, y) for x, y in zip(ka, kb))
        assert any(k.size == 1024 * 512 * 3 for k in ka)


# ---- the device calls without a device -------------------------------------------------------------------------------------------------
def test_device_calls_refuse_the_header_before_any_device(rt, cases):
    A = rt._abi
    out = np.full(40 * 56 * 3, SENTINEL, np.uint8)
    st = A.rt_jpeg_stats()
    for name in ("progressive", "cmyk", "cut-20"):
        data = cases[1][name]
        host = rt.lib.rt_decode_jpeg(data, len(data), out.ctypes.data, out.size), rt.lib.rt_last_error()
        assert (rt.lib.rt_decode_jpeg_device(99, data, len(data), out.ctypes.data, out.size, None, C.byref(st)), rt.lib.rt_last_error()) == host
        assert (rt.lib.rt_dev_decode_jpeg(99, data, len(data), 8, out.ctypes.data, out.size), rt.lib.rt_last_error()) == host
    good = cases[0]["noise-8x8-444-q95-r0"][0]
    assert rt.lib.rt_decode_jpeg_device(99, None, 5, out.ctypes.data, out.size, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_decode_jpeg_device(99, good, len(good), None, out.size, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_decode_jpeg_device(99, good, len(good), out.ctypes.data, 191, None, None) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_last_error() == b"jpeg: capacity 191 below the 192 bytes of the bitmap"
    assert rt.lib.rt_dev_decode_jpeg(99, good, len(good), 3, out.ctypes.data, out.size) == A.RT_ERR_INVALID_ARGUMENT
    assert rt.lib.rt_last_error() == b"subsequence_bytes must be at least 4"
    assert rt.lib.rt_dev_last_jpeg_plan(None) == A.RT_ERR_INVALID_ARGUMENT
    assert (out == SENTINEL).all()


def test_without_a_device_the_device_route_says_so(rt, cases):
    """After the header's checks: RT_ERR_NO_DEVICE, never the host decoder instead."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    A = rt._abi
    good = cases[0]["noise-8x8-444-q95-r0"][0]
    out = np.full(192, SENTINEL, np.uint8)
    assert rt.lib.rt_decode_jpeg_device(0, good, len(good), out.ctypes.data, out.size, None, None) == A.RT_ERR_NO_DEVICE
    assert "no CPU fallback" in rt.lib.rt_last_error().decode() and (out == SENTINEL).all()
    with pytest.raises(rt.RtError) as e:
        rt.LoadImage.fromBytes(good, device=0)
    assert e.value.code == A.RT_ERR_NO_DEVICE
    assert np.array_equal(rt.LoadImage.fromBytes(good), cases[0]["noise-8x8-444-q95-r0"][1])  # device=None: the host decoder when no GPU is visible
