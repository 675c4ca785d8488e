"""Makes tests/golden/jpeg_cases.npz: JPEG files encoded by PIL (libjpeg-turbo) and PIL's own decode of each, so that the independent
reference of every JPEG test is libjpeg-turbo and never this project's decoder.  Needs PIL; the tests need only the .npz.

    python tests/golden/make_jpeg_cases.py [path/to/earthmap.jpg]

Keys: "jpeg/<case>" the file's bytes, "rgb/<case>" PIL's [H, W, 3] decode, "bad/<case>" a file that must be refused.  With a path, the
file is also copied unchanged to tests/golden/earthmap.jpg after its decode is checked to equal tests/golden/earthmap_rgb.npz.

The grid: sizes 1x1 .. 40x56 (8x8 and 16x16 exactly one MCU of some sampling, the others not multiples of any), 4:4:4 / 4:2:2 / 4:2:0,
with and without restart markers every 2 MCUs, and per combination noise at quality 95 and 30 and a crop of the earth map at 75 and 95;
two greyscale files, two with optimised Huffman tables, and quality 1 and 100 at 4:2:0."""
import io
import os
import shutil
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_model  # noqa: E402  (only to choose which damaged file to keep)
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (31, 15), (40, 56), (3, 50)]
SAMPLING = {"444": 0, "422": 1, "420": 2}


def encode(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    rng = np.random.default_rng(26)
    earth = np.load(os.path.join(HERE, "earthmap_rgb.npz"))["rgb"]
    out = {}

    def add(name, data):
        out["jpeg/" + name] = np.frombuffer(data, np.uint8)
        out["rgb/" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    for h, w in SIZES:
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        crop = np.ascontiguousarray(earth[100:100 + h, 300:300 + w])
        for sname, sub in SAMPLING.items():
            for rname, extra in (("r0", {}), ("r2", {"restart_marker_blocks": 2})):
                for kind, a, qual in (("noise", noise, 95), ("noise", noise, 30), ("earth", crop, 75), ("earth", crop, 95)):
                    add(f"{kind}-{h}x{w}-{sname}-q{qual}-{rname}", encode(a, quality=qual, subsampling=sub, **extra))
    add("grey-9x20-q80", encode(rng.integers(0, 256, (9, 20), dtype=np.uint8), quality=80))
    add("grey-16x8-q80", encode(rng.integers(0, 256, (16, 8), dtype=np.uint8), quality=80))
    big = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    add("optimize-noise-40x56-420-q75", encode(big, quality=75, subsampling=2, optimize=True))
    add("optimize-earth-40x56-444-q90", encode(np.ascontiguousarray(earth[200:240, 500:556]), quality=90, subsampling=0, optimize=True))
    add("noise-40x56-420-q1-r0", encode(big, quality=1, subsampling=2))
    add("noise-40x56-420-q100-r0", encode(big, quality=100, subsampling=2))
    # what must be refused
    good = encode(big, quality=75, subsampling=2)
    out["bad/progressive"] = np.frombuffer(encode(big, quality=75, progressive=True), np.uint8)
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (16, 16, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    out["bad/cmyk"] = np.frombuffer(cmyk.getvalue(), np.uint8)
    sos = good.index(b"\xff\xda")
    for cut in (1, 2, 20, sos + 3, sos + 14 + 10, len(good) // 2, len(good) - 40):
        out[f"bad/cut-{cut}"] = np.frombuffer(good[:cut], np.uint8)
    add("cut-source-40x56-420-q75", good)  # (the test program cuts it at every length)
    for at in range(sos + 14 + 200, len(good) - 2):  # the first flip behind byte 200 of the scan that tests/jpeg_model.py cannot decode
        flipped = bytearray(good)
        flipped[at] ^= 0x5A
        try:
            jpeg_model.to_rgb(bytes(flipped))
        except jpeg_model.Refused:
            break
    out["bad/flipped"] = np.frombuffer(bytes(flipped), np.uint8)
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {sum(k.startswith('jpeg/') for k in out)} cases, {sum(k.startswith('bad/') for k in out)} refusal inputs, "
          f"{sum(v.size for k, v in out.items() if not k.startswith('rgb/'))} bytes of JPEG, file {os.path.getsize(path)} bytes")
    if len(sys.argv) > 1:
        data = open(sys.argv[1], "rb").read()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), earth), "not the file earthmap_rgb.npz was decoded from"
        shutil.copyfile(sys.argv[1], os.path.join(HERE, "earthmap.jpg"))
        print("earthmap.jpg copied;", len(data), "bytes")


if __name__ == "__main__":
    main()
