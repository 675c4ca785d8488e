"""What tests/test_gpu_views_edges.py and tests/test_views_edge_cases.py share: large batches of views whose expected buffers come from a
small TABLE of oracle frames.  View v of a batch uses camera v % 3 of small_final's three (test_gpu_views._cameras: the scene's own, the
off-centre one, the sky) and seed 100 + v % 7 -- 21 distinct oracle frames per (frame size, spp); 3 and 7 are coprime, so neighbouring
views differ in both camera and seed and any slip of fewer than 21 views lands on another frame.  The expected [K, rows, cols, 4] and
[K, rows, cols, 3] arrays are the table indexed by (camera, seed); nothing here reads the library's output."""
import functools

import numpy as np

from test_gpu_views import _cam, _cameras, _np, _oracle

NAME = "small_final"
N_CAMERAS, N_SEEDS, SEED0 = 3, 7, 100
OWN, OFF_CENTRE, SKY = 0, 1, 2
TINY = (1, 1)    # max_w, max_h of a 3 x 3 frame, the smallest the library takes
FRAME = None     # the scene's own 49 x 33
EARLY = 11       # Count of a pixel that stopped early, at every spp >= 10
COUNTERS = ("rays", "prim_tests", "reflections")  # (the box-test count is the oracle's only when the reference's tree is walked)

# the batch whose pass-B reservations must cross view ends (test_gpu_views_edges.py, cases 4 and 5): 16,384 views of 3 x 3 = 147,456 pixels
CROSS_K = 16384


def batch(k):
    """(camera of view v, seed of view v) for v < k"""
    v = np.arange(k)
    return v % N_CAMERAS, SEED0 + v % N_SEEDS


def seeds_of(cams):
    return SEED0 + np.arange(len(cams)) % N_SEEDS


def dims(size):
    w, h = size if size is not None else _cameras(NAME)[1:]
    return w, h, 2 * h + 1, 2 * w + 1


@functools.lru_cache(maxsize=None)
def table(orc, size, spp):
    """The 21 oracle frames: (accum [3, 7, rows, cols, 4] int32, rgb [3, 7, rows, cols, 3] uint8, {statistic: [3, 7] int64}); read-only."""
    frames = [[_oracle(orc, NAME, c, spp, SEED0 + s, size) for s in range(N_SEEDS)] for c in range(N_CAMERAS)]
    acc = np.array([[f[0] for f in row] for row in frames])
    rgb = np.array([[f[1] for f in row] for row in frames])
    stats = {key: np.array([[int(f[2][key]) for f in row] for row in frames], np.int64) for key in ("samples", "pixels_early") + COUNTERS}
    assert acc.dtype == np.int32 and rgb.dtype == np.uint8
    assert np.array_equal(stats["samples"], acc[..., 0].sum(axis=(2, 3)))
    if spp > EARLY:
        assert np.array_equal(stats["pixels_early"], (acc[..., 0] == EARLY).sum(axis=(2, 3)))
    for a in (acc, rgb) + tuple(stats.values()):
        a.setflags(write=False)
    return acc, rgb, stats


def expected(orc, size, spp, cams, seeds):
    """The oracle's batch: (accum [K, rows, cols, 4], rgb [K, rows, cols, 3], {statistic: the sum over the views})"""
    cams, s = np.asarray(cams), np.asarray(seeds) - SEED0
    acc, rgb, stats = table(orc, size, spp)
    return acc[cams, s], rgb[cams, s], {key: int(t[cams, s].sum()) for key, t in stats.items()}


def assert_batch(got, want_acc, want_rgb, what=()):
    """Whole arrays, bit for bit; on a mismatch the first differing view and pixel."""
    acc, rgb = _np(got.accum), _np(got.rgb)
    assert acc.shape == want_acc.shape and rgb.shape == want_rgb.shape and acc.dtype == np.int32 and rgb.dtype == np.uint8, what
    if np.array_equal(acc, want_acc) and np.array_equal(rgb, want_rgb):
        return
    bad = (acc != want_acc).any(axis=-1) | (rgb != want_rgb).any(axis=-1)
    v, r, c = (int(x) for x in np.argwhere(bad)[0])
    raise AssertionError(f"{tuple(what)}: {int(bad.sum())} pixels of {int(bad.any(axis=(1, 2)).sum())} views differ from the oracle; the first is view {v} "
                         f"(camera {v % N_CAMERAS}, seed {SEED0 + v % N_SEEDS} under batch()) pixel ({r}, {c}): "
                         f"accum {acc[v, r, c].tolist()} rgb {rgb[v, r, c].tolist()}, the oracle {want_acc[v, r, c].tolist()} {want_rgb[v, r, c].tolist()}")


def assert_stats(st, want, k, size, counters):
    _, _, rows, cols = dims(size)
    assert st["pixels"] == k * rows * cols
    assert st["samples"] == want["samples"] and st["pixels_early"] == want["pixels_early"]
    for key in COUNTERS:
        assert st[key] == (want[key] if counters else 0), key
    if not counters:
        assert st["aabb_tests"] == 0


def cameras(spp):
    """small_final's three cameras at spp: the objects a batch repeats"""
    return tuple(_cam(c, spp) for c in _cameras(NAME)[0])


def live_per_view(orc, size, spp, k):
    """The oracle's live list of batch(k): entries per view (batch pixels whose Count is spp)"""
    cams, seeds = batch(k)
    return (table(orc, size, spp)[0][..., 0] == spp).sum(axis=(2, 3))[cams, seeds - SEED0]


def full_chunk_crossings(orc, size, spp, k, total_waves, chunk):
    """A second proof of crossings, for shapes whose w_half is too small for crossing_numbers': a reservation whose first entry is at most
    L = N - 2 W chunk was sized with seen <= first, so it asked for (N - seen) / (2 W) >= chunk entries and got exactly `chunk`; by
    induction those reservations start at the multiples of chunk.  A view end e in (0, L] that is no multiple of chunk therefore lies
    strictly inside one.  -> how many such ends the oracle's list has."""
    live = live_per_view(orc, size, spp, k)
    ends = np.cumsum(live)[live > 0]
    limit = int(live.sum()) - 2 * total_waves * chunk
    return int(((ends <= limit) & (ends % chunk != 0)).sum())


def crossing_numbers(orc, size, spp, k, total_waves, chunk):
    """The precondition under which pass B's reservations provably cross view ends, from the oracle's frames and the plan's total_waves
    alone: N live list entries (batch pixels whose oracle Count is spp), m entries per view that has one, and w_half, the least
    reservation while less than half the list is handed out -- want = clamp((N - seen) / (2 W), 1, chunk) with seen < N / 2.  Ranges of
    at least w_half entries tile that half without gaps, so it holds at most N / (2 w_half) of them, and about N / (2 m) view ends; with
    w_half >= 2 m at least half of those ends fall strictly inside a range."""
    live = live_per_view(orc, size, spp, k)
    n = int(live.sum())
    views_live = int((live > 0).sum())
    m = n / views_live
    w_half = min(chunk, n // (4 * total_waves))
    return {"N": n, "views_live": views_live, "m": m, "w_half": w_half, "W": total_waves, "most_in_a_view": int(live.max()), "holds": w_half >= 2 * m}
