"""Pixel maps for the parse tests (test_pixel_map_device_host.py, test_gpu_pixel_map.py and tests/c/pixel_map_scan_table.cpp), built as
RECORDS -- never as random bytes -- so that the reference reader accepts every one of them except where a test says otherwise.

A record is `<row> <terminator> <column> <terminator> R G B` (ImageOutput.fs:46-161).  The writer emits 0 as no digits and uses ',' and
'\\n'; the reader takes any non-digit as a terminator, any number of leading zeros, and three colour bytes that are raw data."""
import random
import struct

import numpy as np

TERMINATORS = (b",", b"\n", b"A", b"\x00", b"\xff", b" ")
LEADING_ZEROS = (0, 1, 7, 300)
COLOURS = (b"123", b"7,8", b",\n0", b"\n\n\n", b"000", b"9,9", bytes([0, 255, 17]), bytes([200, 48, 44]), bytes([10, 57, 58]), bytes([47, 1, 254]))


def number(value, zeros=0, zero_digit=False):
    """writeAsciiInt's digits (none for 0) or "0" for 0, behind `zeros` leading zeros."""
    return b"0" * zeros + (str(value).encode() if value or zero_digit else b"")


def record(row, col, colour, zeros=(0, 0), zero_digit=(False, False), terms=(b",", b"\n")):
    assert len(colour) == 3
    return number(row, zeros[0], zero_digit[0]) + terms[0] + number(col, zeros[1], zero_digit[1]) + terms[1] + bytes(colour)


def random_records(rng, rows, cols, n, zeros=(0, 1, 7), distinct=True):
    """n records in range; distinct pixels unless told otherwise; every way of writing a number and every terminator turns up."""
    pixels = rng.sample(range(rows * cols), n) if distinct else [rng.randrange(rows * cols) for _ in range(n)]
    out = []
    for p in pixels:
        colour = rng.choice(COLOURS) if rng.random() < 0.7 else bytes(rng.randrange(256) for _ in range(3))
        out.append(record(p // cols, p % cols, colour, (rng.choice(zeros), rng.choice(zeros)), (rng.random() < 0.5, rng.random() < 0.5),
                          (rng.choice(TERMINATORS), rng.choice(TERMINATORS))))
    return out


def other_colour(rec):
    """The same record with other colour bytes (a duplicate must be told from the original)."""
    return rec[:-3] + bytes((b + 101) & 255 for b in rec[-3:])


def variants(rng, recs):
    """(name, records): whole, shuffled, every third dropped, and duplicated with DIFFERENT colours, earlier and later copies mixed in."""
    shuffled = list(recs)
    rng.shuffle(shuffled)
    dup = list(recs)
    for r in recs[::2]:
        dup.insert(rng.randrange(len(dup) + 1), other_colour(r))
    return [("whole", list(recs)), ("shuffled", shuffled), ("dropped", [r for i, r in enumerate(recs) if i % 3 != 2]), ("duplicated", dup)]


def small_files():
    """(name, rows, cols, data) of at most ~100 bytes each: the files whose EVERY truncation is tried."""
    rng = random.Random(2101)
    out = []
    for rows, cols, n in ((1, 1, 1), (1, 2, 2), (2, 1, 2), (3, 4, 5), (12, 103, 5), (101, 11, 5), (2, 1002, 4), (7, 5, 6)):
        recs = random_records(rng, rows, cols, n, zeros=(0, 0, 1, 7))
        for name, v in variants(rng, recs):
            out.append((f"{rows}x{cols}-{name}", rows, cols, b"".join(v)))
    return out


def long_files():
    """Files with 300-zero runs and a few hundred records: chunk and tile boundaries fall everywhere; no truncation sweep."""
    rng = random.Random(2102)
    out = []
    for rows, cols, n in ((5, 9, 12), (64, 1, 40), (1, 64, 64), (33, 49, 300)):
        recs = random_records(rng, rows, cols, n, zeros=LEADING_ZEROS if n < 100 else (0, 0, 0, 1, 7, 300))
        for name, v in variants(rng, recs):
            out.append((f"{rows}x{cols}-long-{name}", rows, cols, b"".join(v)))
    return out


def malformed_files():
    """A complete record outside the image in the first, a middle and the last position."""
    return _with_bad_record((record(6, 0, b"abc"), record(0, 7, b"abc"), record(2147483647, 1, b"abc")))


def overflow_files():
    """A digit run beyond int32 (11 nines): outside the host reader's contract (its int arithmetic overflows), malformed on the device."""
    return _with_bad_record((record(1, 99999999999, b"abc"), record(99999999999, 99999999999, b"999")))


def _with_bad_record(bads):
    rng = random.Random(2103)
    rows, cols = 6, 7
    good = random_records(rng, rows, cols, 9)
    out = []
    for k, bad in enumerate(bads):
        for at in (0, 4, len(good)):
            out.append((f"bad{k}-at{at}", rows, cols, b"".join(good[:at] + [bad] + good[at:]), good, bad, at))
    return out


def expected(orc, data, rows, cols):
    """The reference reader's answer: (count, rgb [rows, cols, 3], present [rows, cols] bool); count -1 for a malformed map."""
    return orc.parse_pixel_map(bytes(data), rows, cols)


def write_table_input(path, cases):
    """The cases for tests/c/pixel_map_scan_table.cpp: per case uint32 rows, cols, n_bytes, sweep (1: every truncation too), then the bytes."""
    with open(path, "wb") as f:
        for rows, cols, data, sweep in cases:
            f.write(struct.pack("<IIII", rows, cols, len(data), int(sweep)))
            f.write(data)


def map_of(orc, rgb, keep=None):
    """The writer's own records of an image, as a list (format_pixel_map's bytes cut at the record boundaries), optionally only pixels keep[i]."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    rows, cols = rgb.shape[0], rgb.shape[1]
    recs = [record(r, c, bytes(rgb[r, c])) for r in range(rows) for c in range(cols)]
    assert b"".join(recs) == orc.format_pixel_map(rgb)
    return recs if keep is None else [recs[i] for i in keep]
