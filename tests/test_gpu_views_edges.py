"""Scene.renderViews where pass B's ranges and the ordering of its list change path, each view held bit for bit to the ORACLE's frame for
its camera and seed (views_edge_cases.py: a table of 21 oracle frames indexed by view), never to the library's own output: batches that
end an upload launch exactly or with one camera; the ordering kernels at, below and beyond the keys the LDS holds; one cost bucket a
view above 4096 views; reservations of many list entries that cross view ends; and views -- whole batches -- with nothing in the list."""
import os

import numpy as np
import pytest

import views_edge_cases as E
from test_gpu_views import _scene, _tensor_accum

pytestmark = pytest.mark.gpu

VIEWS_KIND = 6
_SIZE_ID = {E.TINY: "3x3", E.FRAME: "49x33"}


def _launch(rt, size, spp, cams, seeds, *, arrays=False, counters=False, **options):
    """One renderViews of the batch (camera indices, seeds) -> (result, the launch plan as the library executed it)"""
    torch = pytest.importorskip("torch")
    w, h, _, _ = E.dims(size)
    three = E.cameras(spp)
    kw = {} if arrays else dict(accum=_tensor_accum(torch, len(cams), w, h), options=rt._abi.rt_render_options(**options))
    got = _scene(rt, E.NAME).renderViews(w, h, [three[c] for c in np.asarray(cams).tolist()], seeds=np.asarray(seeds).tolist(), counters=counters, **kw)
    return got, rt.hooks.last_launch_plan()


def _check(orc, got, plan, size, spp, cams, seeds, *, two_pass, counters=False, what=()):
    want_acc, want_rgb, want = E.expected(orc, size, spp, cams, seeds)
    _, _, rows, _ = E.dims(size)
    assert plan["in"]["kind"] == VIEWS_KIND and plan["in"]["n"] == len(cams) and plan["in"]["n_rows"] == rows and plan["in"]["count"] == int(counters), what
    assert plan["out"]["two_pass"] == int(two_pass) and plan["out"]["error"] == 0, what
    E.assert_batch(got, want_acc, want_rgb, what)
    E.assert_stats(got.stats, want, len(cams), size, counters)


def _run(rt, orc, size, spp, cams, seeds, passes, *, counters=False, what=(), **options):
    got, plan = _launch(rt, size, spp, cams, seeds, counters=counters, passes=passes, **options)
    _check(orc, got, plan, size, spp, cams, seeds, two_pass=passes == 2, counters=counters, what=tuple(what) + (len(cams), passes, counters))
    return plan


# ---- 1: upload chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (24, 25, 48, 49))
def test_batches_that_end_an_upload_launch(rt, orc, k):
    """The cameras go up 24 a launch: one full launch, one and a single camera, two full ones, two and a single camera."""
    cams, seeds = E.batch(k)
    for passes in (1, 2):
        _run(rt, orc, E.TINY, 40, cams, seeds, passes)
    if k == 25:
        _run(rt, orc, E.TINY, 40, cams, seeds, 2, counters=True)


# ---- 2: the LDS limit of the ordering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,k", [(E.TINY, 127), (E.TINY, 128), (E.TINY, 129), (E.FRAME, 128), (E.FRAME, 129)], ids=lambda x: _SIZE_ID.get(x, str(x)))
def test_the_ordering_at_the_keys_the_lds_holds(rt, orc, size, k):
    """128 views of 64 cost buckets are the 8192 keys the ordering counts in LDS (its scatter then asks for 64 KiB of it); 129 go to
    global memory item by item.  At 49 x 33 a view holds pixels of many cost buckets, so the order inside a view is exercised on both."""
    cams, seeds = E.batch(k)
    plan = _run(rt, orc, size, 40, cams, seeds, 2)
    assert plan["out"]["sort"] >= k * 65 * 4
    if size == E.TINY and k == 128:
        _run(rt, orc, size, 40, cams, seeds, 2, counters=True)


# ---- 3: one cost bucket a view -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4096, 4097))
def test_the_bucket_rule(rt, orc, k):
    """4096 views are ordered by view and cost (64 buckets each), 4097 by view alone.  spp 12: one sample a live pixel is left to pass B."""
    cams, seeds = E.batch(k)
    plan = _run(rt, orc, E.TINY, 12, cams, seeds, 2)
    assert plan["out"]["sort"] == (k * ((64 if k <= 4096 else 1) + 1) * 4 + 15) // 16 * 16
    if k == 4097:
        _run(rt, orc, E.TINY, 12, cams, seeds, 2, counters=True)
        # the host variant with its staging takes no options: two passes through the process's own setting
        rt.set_passes(2)
        try:
            got, plan = _launch(rt, E.TINY, 12, cams, seeds, arrays=True)
        finally:
            rt.set_passes(int(os.environ.get("RTFS_PASSES") or 0))
        assert isinstance(got.accum, np.ndarray)
        _check(orc, got, plan, E.TINY, 12, cams, seeds, two_pass=True, what=("arrays", k))


# ---- 4, 5: reservations that cross view ends -------------------------------------------------------------------------------------
def _crossing(rt, orc, spp, chunk, counters=False, **options):
    cams, seeds = E.batch(E.CROSS_K)
    got, plan = _launch(rt, E.TINY, spp, cams, seeds, counters=counters, chunk_pixels=chunk, blocks_per_cu=1, passes=2, **options)
    o = plan["out"]
    assert o["two_pass"] == 1 and o["error"] == 0 and o["q_block"] == options["block_threads"] and o["B_chunk"] == chunk
    numbers = E.crossing_numbers(orc, E.TINY, spp, E.CROSS_K, o["B_total_waves"], chunk)
    _check(orc, got, plan, E.TINY, spp, cams, seeds, two_pass=True, counters=counters, what=(spp, chunk, counters, sorted(numbers.items())))
    return numbers


@pytest.mark.parametrize("spp", (12, 40))
def test_reservations_that_cross_view_ends(rt, orc, spp):
    """16,384 views of 3 x 3 (147,456 batch pixels), blocks of 256 threads, one a CU, ranges of up to 64 entries.  From the oracle alone,
    at spp 12 and at spp 40 alike: N = 96,746 live entries in 10,923 views (the sky's 5,461 have none; 8 or 9 in every other), m = 8.857
    a view; with W = 1024 waves w_half = min(64, N // 4096) = 23 >= 2 m = 17.71, so at least half of the view ends in the list's first
    half fall strictly inside a reservation (views_edge_cases.crossing_numbers)."""
    numbers = _crossing(rt, orc, spp, 64, block_threads=256)
    assert numbers["W"] == 1024 and numbers["holds"], numbers
    if spp == 12:
        assert _crossing(rt, orc, spp, 64, counters=True, block_threads=256)["holds"]


@pytest.mark.parametrize("spp", (12, 40))
def test_short_ranges_that_cross_view_ends_at_1024_threads(rt, orc, spp):
    """The same batch with blocks of 1024 threads (the other instantiation of the views kernels), one a CU, and ranges of at most 7
    entries.  W = 4096 here, so w_half = min(7, N // 16384) = 5 < 2 m = 17.71: the counting argument of crossing_numbers does NOT prove
    crossings for this shape.  Another count from the oracle does (views_edge_cases.full_chunk_crossings): every reservation that starts
    at or below L = N - 2 * 4096 * 7 = 39,402 holds exactly 7 entries and starts at a multiple of 7, and 3,815 view ends up to L are no
    multiple of 7 -- each strictly inside a reservation."""
    numbers = _crossing(rt, orc, spp, 7, block_threads=1024)
    assert numbers["W"] == 4096, numbers
    assert E.full_chunk_crossings(orc, E.TINY, spp, E.CROSS_K, numbers["W"], 7) > 3000


# ---- 6: views with nothing in the list -------------------------------------------------------------------------------------------
O, F, S = E.OWN, E.OFF_CENTRE, E.SKY
EMPTY_BATCHES = {
    "sky_1": [S], "sky_5": [S] * 5, "sky_130": [S] * 130,
    "runs_of_sky": [S] * 5 + [O] + [S] * 70 + [F] + [S] * 3,
    "own_then_sky": [O] + [S] * 129,
}


@pytest.mark.parametrize("size,which", [(E.TINY, b) for b in EMPTY_BATCHES] + [(E.FRAME, "runs_of_sky")], ids=lambda x: _SIZE_ID.get(x, str(x)))
def test_views_with_nothing_in_the_list(rt, orc, size, which):
    """Batches of the sky camera alone, where every pixel stops early and pass B's list is empty, and runs of such views in front of,
    between and behind live ones: equal view ends in a row."""
    cams = np.array(EMPTY_BATCHES[which])
    seeds = E.seeds_of(cams)
    acc = E.table(orc, size, 40)[0]
    assert (acc[S, ..., 0] == E.EARLY).all() and all((acc[c, s, ..., 0] == 40).any() for c in (O, F) for s in range(E.N_SEEDS))
    for passes in (1, 2):
        _run(rt, orc, size, 40, cams, seeds, passes, what=(which,))
    if which in ("sky_5", "runs_of_sky"):
        _run(rt, orc, size, 40, cams, seeds, 2, counters=True, what=(which,))
