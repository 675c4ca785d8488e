"""Independent yardsticks and shared images of the PNG tests (test_png_host.py, test_gpu_png.py).

The decoder is written for the tests and shares nothing with the library: it walks the chunks, checks every chunk's CRC with zlib.crc32,
inflates with zlib.decompress (which also checks Adler-32) and undoes filter types 0..4 in numpy.  Where PIL imports, a second decode
with it, converted to RGBA, must give the same pixels with alpha 255.  The expected pixels come from oracle.gamma_correct."""
import functools
import io
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = b"\x89PNG\r\n\x1a\n"
GOLDEN_IMAGE = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[255, 255, 0], [255, 255, 255], [0, 0, 0]]], np.uint8)  # TestPpmOutput.fs:12-46


def chunks(data):
    """[(name, payload)] of a PNG; every length and CRC checked, nothing behind IEND."""
    assert data[:8] == SIGNATURE, "not a PNG signature"
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        assert n < 2**31 and at + 12 + n <= len(data), "a chunk runs past the file"
        name, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(name + payload), f"CRC of chunk {name!r}"
        out.append((name, payload))
        at += 12 + n
    assert out and out[-1] == (b"IEND", b"") and at == len(data)
    return out


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(raw, rows, cols, bpp=3):
    """The pixel bytes [rows, cols * bpp] of the filtered stream `raw`: filter types 0..4 (PNG 9.2)."""
    stride = cols * bpp
    assert len(raw) == rows * (1 + stride), "the inflated stream is not rows * (1 + 3 cols) bytes"
    lines = np.frombuffer(raw, np.uint8).reshape(rows, 1 + stride)
    out = np.zeros((rows, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for r in range(rows):
        ft, line = int(lines[r, 0]), lines[r, 1:].astype(np.int32)
        assert ft <= 4, f"filter type {ft}"
        cur = np.zeros(stride, np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:  # Sub: a running sum per byte lane
            cur = (np.cumsum(line.reshape(cols, bpp), axis=0) & 255).reshape(-1)
        else:
            for x in range(stride):
                a = cur[x - bpp] if x >= bpp else 0
                c = prev[x - bpp] if x >= bpp else 0
                pred = (a + prev[x]) // 2 if ft == 3 else int(_paeth(np.int32(a), np.int32(prev[x]), np.int32(c)))
                cur[x] = (line[x] + pred) & 255
        out[r] = cur
        prev = cur
    return out


def decode(data):
    """(pixels [rows, cols, 3] uint8, the IDAT payload) of a PNG of colour type 2, bit depth 8; both decoders must agree."""
    cs = chunks(data)
    assert cs[0][0] == b"IHDR" and len(cs[0][1]) == 13
    cols, rows, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", cs[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    idat = b"".join(p for n, p in cs if n == b"IDAT")
    px = unfilter(zlib.decompress(idat), rows, cols).reshape(rows, cols, 3)
    try:
        from PIL import Image
    except ImportError:
        return px, idat
    img = Image.open(io.BytesIO(data))
    img.load()
    rgba = np.asarray(img.convert("RGBA"))
    assert rgba.shape == (rows, cols, 4) and (rgba[:, :, 3] == 255).all() and np.array_equal(rgba[:, :, :3], px), "PIL decodes other pixels"
    return px, idat


def expected_pixels(orc, img, gamma):
    if not gamma:
        return np.ascontiguousarray(img, np.uint8)
    lut = np.array([orc.gamma_correct(b) for b in range(256)], np.uint8)
    return lut[img]


def tile_block_types(idat, filtered_len, tile_bytes):
    """BTYPE of every tile's block.  A tile is one block that ends on a byte boundary -- a stored block, or a Huffman block with the empty
    stored block 00 00 FF FF behind it -- and inflates to exactly its tile_bytes of the stream: a raw inflater is fed tile by tile, a Huffman
    tile byte by byte until its bytes are out (what is left of it is the end-of-block code, at most 15 bits, and the marker, so the first
    00 00 FF FF from there on is the marker)."""
    assert idat[:2] == b"\x78\x01"
    body, d, at, types = idat[2:-4], zlib.decompressobj(-15), 0, []
    for tile in range(-(-filtered_len // tile_bytes)):
        n = min(tile_bytes, filtered_len - tile * tile_bytes)
        assert body[at] & 1 == 0, "BFINAL inside the tiles"
        types.append((body[at] >> 1) & 3)
        if types[-1] == 0:
            assert body[at:at + 5] == b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF)
            end, got = at + 5 + n, 0
        else:
            got, end = 0, at
            while got < n:
                got += len(d.decompress(body[end:end + 1]))
                end += 1
            at, end = end, body.index(b"\x00\x00\xff\xff", end - 1) + 4
        got += len(d.decompress(body[at:end]))
        assert got == n, f"tile {tile} inflates to {got} bytes, not {n}"
        at = end
    assert body[at:] == b"\x01\x00\x00\xff\xff", "the final empty block"
    assert d.decompress(body[at:]) == b"" and d.eof
    return types


# ---- images -----------------------------------------------------------------------------------------------------------------------------
def image_of_filtered(stream):
    """The 1 x n image (gamma off) whose filtered stream is the byte 1 followed by `stream` (3 n bytes): the Sub filter undone."""
    s = np.asarray(stream, np.int64)
    assert s.size % 3 == 0 and s.size > 0
    return (np.cumsum(s.reshape(-1, 3), axis=0) & 255).astype(np.uint8).reshape(1, -1, 3)


def every_byte_image():
    v = np.arange(256, dtype=np.int64)
    return np.stack([v, (v * 7 + 3) % 256, 255 - v], axis=1).astype(np.uint8).reshape(16, 16, 3)  # test_gpu_output.py's


@functools.lru_cache(maxsize=None)
def golden_frames():
    out = []
    for name in ("oracle_config2_small_seed2", "oracle_all_materials_seed0", "oracle_final_thumb_seed7", "oracle_earth_thumb_seed3"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        rgb = np.ascontiguousarray(z["rgb"], np.uint8)
        rgb.setflags(write=False)
        out.append((name, rgb))
    return tuple(out)


def noise(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def _image_with_filtered_length(target, seed):
    """rows x cols noise with rows (1 + 3 cols) == target, the fewest rows that do it."""
    for rows in range(1, target // 4 + 1):
        if target % rows == 0 and (target // rows - 1) % 3 == 0 and target // rows >= 4:
            return noise(rows, (target // rows - 1) // 3, seed)
    raise AssertionError(f"no image has {target} filtered bytes")


def _image_split_at_boundary(T, part, seed):
    """Noise whose pixel at the first tile boundary has `part` (1 or 2) of its bytes in front of it: with stride S = 1 + 3 cols, row r starts
    at r S and byte T is its colour byte T - r S - 1."""
    for r in range(1, 7):
        cols = T // (r + 1) // 3 + 5
        S = 1 + 3 * cols
        if r * S + 1 < T < (r + 1) * S and (T - r * S - 1) % 3 == part:
            return noise(r + 1, cols, seed)
    raise AssertionError("no such image")


def shape_cases(T):
    """(name, image): every size at which a tile boundary falls somewhere else.  The filtered length of rows x cols is rows (1 + 3 cols)."""
    cases = [("1x1", noise(1, 1, 1)), ("1xN", noise(1, 77, 2)), ("Nx1", noise(77, 1, 3))]
    for k in (1, 2):  # filtered lengths k T, one byte either side, and one pixel a row either side of the image that is exactly k T
        exact = _image_with_filtered_length(k * T, seed=10 * k)
        cases.append((f"{k}T", exact))
        for name, target in (("-1B", k * T - 1), ("+1B", k * T + 1)):
            cases.append((f"{k}T{name}", _image_with_filtered_length(target, seed=10 * k + len(cases))))
        for name, d in (("-1px", -1), ("+1px", 1)):
            cases.append((f"{k}T{name}", noise(exact.shape[0], exact.shape[1] + d, 10 * k + len(cases))))
    first = next(s for s in range(4, T, 3) if T % s == 0)        # a row starts at T: its filter byte is a tile's FIRST byte
    cases.append(("filter-byte-first", noise(T // first + 2, (first - 1) // 3, 60)))
    last = next(s for s in range(4, T, 3) if (T - 1) % s == 0)   # a row starts at T - 1: its filter byte is a tile's LAST byte
    cases.append(("filter-byte-last", noise((T - 1) // last + 2, (last - 1) // 3, 61)))
    cases.append(("pixel-split-1+2", _image_split_at_boundary(T, 1, 62)))
    cases.append(("pixel-split-2+1", _image_split_at_boundary(T, 2, 63)))
    return cases


def run_cases(T):
    """(name, image) with runs of every length at which the token rule turns, built in the filtered domain (one row, gamma off)."""
    rng = np.random.default_rng(5)
    out = []
    stream = []
    last = 0
    for L in (1, 2, 3, 4, 258, 259, 260, 261, 262, 517):
        v = int(rng.integers(2, 256))
        v = v if v != last else (v % 254) + 2
        stream += [v] * L
        last = v
    while len(stream) % 3:
        last = (last % 254) + 2
        stream.append(last)
    out.append(("run-lengths", image_of_filtered(stream)))
    # a run crossing a tile boundary, and a run that ends with the image
    body = list(rng.integers(2, 256, T - 300)) + [7] * 700
    body += [9] * ((-len(body)) % 3 + 3 * 40)
    out.append(("run-across-tiles-and-to-the-end", image_of_filtered(body)))
    # a tile that is one run: tile 1 of three (the filter byte 1 is in tile 0)
    body = list(rng.integers(2, 256, T - 1 - 100)) + [5] * (100 + T + 50) + list(rng.integers(2, 256, 3 * 33 + 1))
    body += [11] * ((-len(body)) % 3)
    out.append(("tile-of-one-run", image_of_filtered(body)))
    out.append(("all-zero", np.zeros((64, 64, 3), np.uint8)))
    return out


def histogram_cases(T):
    """(name, image, BTYPE expected of tile 0 or None): one tile each, built in the filtered domain."""
    rng = np.random.default_rng(6)
    n = T - 1  # behind the filter byte
    out = []
    # a single literal value: the byte 1 everywhere (the filter byte is a 1 too) -- one literal, then matches
    out.append(("single-literal", image_of_filtered([1] * n), None))
    # all 256 values equally often, no two neighbours equal: stored must be chosen
    perm = np.concatenate([rng.permutation(256) for _ in range(T // 256)])[: n]
    perm[0] = perm[0] if perm[0] != 1 else 2
    for i in range(1, n):
        if perm[i] == perm[i - 1]:
            perm[i] = (perm[i] + 1) % 256
    out.append(("uniform", image_of_filtered(perm), 0))
    # Fibonacci counts: the end-of-block symbol 1, the value 1 once (the filter byte), then 2, 3, 5 ... 987 and 1598 (1597 + 1, so that the
    # bytes make whole pixels): 4180 literals.  Huffman's own tree is a chain 16 deep (unlimited_depth), one past the limit.
    fib = [2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1598]
    vals = _no_neighbours_equal(np.repeat(np.arange(len(fib)) * 3 + 2, fib))
    assert unlimited_depth([1, 1] + fib) > 15 and len(vals) % 3 == 0
    out.append(("fibonacci", image_of_filtered(vals), 2))
    # no match at all: HDIST = 1 with length 0
    two = np.tile(np.array([3, 200, 3, 17, 200, 17]), 500)[: 2997]
    out.append(("no-match", image_of_filtered(two), None))
    return out


def unlimited_depth(counts):
    """The longest code of Huffman's own (unlimited) tree for these counts."""
    import heapq

    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def _no_neighbours_equal(vals):
    """A permutation of vals without two equal neighbours: the commonest value is dealt out first, at every other place."""
    vals = np.asarray(vals)
    order = sorted(set(vals.tolist()), key=lambda v: -(vals == v).sum())
    seq = np.concatenate([np.full((vals == v).sum(), v) for v in order])
    n = len(seq)
    out = np.empty(n, seq.dtype)
    half = (n + 1) // 2
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    assert (out[1:] != out[:-1]).all()
    return out
