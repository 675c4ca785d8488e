"""The work units of a batch of views (csrc/rt_views_plan.h) on a CPU.  A unit of the fused kernel or of pass A, and a range of pass B,
must lie inside ONE view, because the camera and the seed key of a wave's current work are wave-uniform.  tests/c/views_plan_table.cpp is
the header behind a text interface, built here with g++; the properties are checked on its lines, and the same checks catch two
mutants of the mapping written here in Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PIXELS = (1, 15, 63, 64, 65, 1617, 2911)
CHUNKS = (1, 7, 32, 64)
VIEWS = (1, 2, 3, 70)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views") / "views_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "views_plan_table.cpp")])

    def run(lines):
        return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()

    return run


def _units(table, ppv, chunk, k):
    out = table([f"units {ppv} {chunk} {k}"])
    head = dict(kv.split("=") for kv in out[0].split())
    rows = [tuple(int(x) for x in line.split()) for line in out[1:]]
    assert len(rows) == int(head["units"]) and [r[0] for r in rows] == list(range(len(rows)))
    return int(head["per_view"]), [r[1:] for r in rows]  # (view, first, npx, batch_first)


def _violations(units, ppv, chunk, k):
    """What is wrong with a list of (view, first, npx, batch_first) as the units of k views of ppv pixels: [] for a sound mapping."""
    bad = []
    owner = [0] * (k * ppv)
    for view, first, npx, batch_first in units:
        if not 0 <= view < k or npx < 1 or npx > chunk:
            bad.append(("shape", view, first, npx))
            continue
        if first + npx > ppv:
            bad.append(("spans two views", view, first, npx))
        if batch_first != view * ppv + first:
            bad.append(("batch pixel", view, first, batch_first))
        for g in range(batch_first, min(batch_first + npx, k * ppv)):
            owner[g] += 1
    if any(c != 1 for c in owner):
        bad.append(("coverage", owner.count(0), sum(1 for c in owner if c > 1)))
    if sum(u[2] for u in units) != k * ppv:
        bad.append(("sizes", sum(u[2] for u in units)))
    return bad


def _model(ppv, chunk, k, mutant=None):
    """The mapping as the issue states it, in Python -- and its two mutants."""
    upv = -(-ppv // chunk)
    units = []
    n_units = k * upv
    if mutant == "runs past its view":  # units laid over the batch as over one frame: a unit may start in one view and end in the next
        n_units = -(-(k * ppv) // chunk)
    for u in range(n_units):
        if mutant == "runs past its view":
            g = u * chunk
            view, first = g // ppv, g % ppv
            npx = min(chunk, k * ppv - g)
        else:
            view, first = u // upv, (u % upv) * chunk
            npx = chunk if mutant == "last unit not clipped" else min(chunk, ppv - first)
        units.append((view, first, npx, view * ppv + first))
    return upv, units


def test_every_batch_pixel_lies_in_exactly_one_unit_and_no_unit_spans_two_views(table):
    for ppv in PIXELS:
        for chunk in CHUNKS:
            for k in VIEWS:
                upv, units = _units(table, ppv, chunk, k)
                assert upv == -(-ppv // chunk) and len(units) == k * upv
                assert _violations(units, ppv, chunk, k) == [], (ppv, chunk, k)
                assert (upv, units) == _model(ppv, chunk, k), (ppv, chunk, k)
                # the last unit of a view is short exactly when the chunk does not divide the view
                last = [u for u in units if u[1] + u[2] == ppv]
                assert len(last) == k and all(u[2] == (ppv % chunk or chunk) for u in last)


def test_the_checks_catch_a_unit_that_runs_past_its_view_and_an_unclipped_last_unit():
    caught = {"runs past its view": 0, "last unit not clipped": 0}
    for mutant in caught:
        for ppv in PIXELS:
            for chunk in CHUNKS:
                for k in VIEWS:
                    _, units = _model(ppv, chunk, k, mutant)
                    differs = units != _model(ppv, chunk, k)[1]
                    bad = _violations(units, ppv, chunk, k)
                    assert bool(bad) == differs, (mutant, ppv, chunk, k)  # every case where the mutant differs is caught, no other
                    caught[mutant] += bool(bad)
    assert all(n > 20 for n in caught.values()), caught
    # and the kind of fault found is the one planted
    assert any(v[0] == "spans two views" for v in _violations(_model(65, 64, 3, "runs past its view")[1], 65, 64, 3))
    assert any(v[0] == "spans two views" for v in _violations(_model(65, 64, 3, "last unit not clipped")[1], 65, 64, 3))


def test_a_pass_b_range_ends_with_its_view(table):
    cases = [(0, 4, 10, 4), (8, 4, 10, 2), (9, 1, 10, 1), (9, 64, 10, 1), (100, 32, 1000, 32), (2**31, 64, 2**31 + 3, 3)]
    out = table([f"range {f} {n} {e}" for f, n, e, _ in cases])
    assert [int(x) for x in out] == [w for _, _, _, w in cases]


def test_the_sort_key_orders_by_view_then_by_decreasing_cost(table):
    lines, want = [], []
    for k in (1, 3, 70, 4096):
        for view in sorted({0, k // 2, k - 1}):
            for bucket in (0, 1, 62, 63):
                lines.append(f"key {k} {view} {bucket}")
                want.append((64, view * 64 + 63 - bucket))
    for k in (4097, 100000):  # so many views that the table of keys would outgrow the list: by view alone
        for view in (0, k - 1):
            for bucket in (0, 63):
                lines.append(f"key {k} {view} {bucket}")
                want.append((1, view))
    got = [tuple(int(kv.split("=")[1]) for kv in line.split()) for line in table(lines)]
    assert got == want
