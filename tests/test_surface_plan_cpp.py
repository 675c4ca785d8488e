"""The plan of the surface-record kernel (csrc/rt_surface_plan.h) on a CPU, through tests/c/surface_plan_table.cpp: the tile and grid
arithmetic at the slot counts where it changes, and the kernel's predicates over every (kind, style, texture id sign, root kind)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 2**31 - 1  # the ray lists' bound (check_count)
TILE, BLOCK, PER_CU = 1024, 256, 8
SPHERE, UNBOUNDED_SPHERE, PLANE = 0, 1, 2  # the kind bits of a meta word (RT_HITTABLE_*)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_surface") / "surface_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "c", "surface_plan_table.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out]

    return run


def test_the_kind_bits_are_the_abis(rt):
    A = rt._abi
    assert (A.RT_HITTABLE_SPHERE, A.RT_HITTABLE_UNBOUNDED_SPHERE, A.RT_HITTABLE_INFINITE_PLANE) == (SPHERE, UNBOUNDED_SPHERE, PLANE)
    assert (A.RT_SPHERE_LIGHT_SOURCE, A.RT_SPHERE_LIGHT_SOURCE_CAP, A.RT_PLANE_LIGHT_SOURCE, A.RT_TEXTURE_COLOUR) == (0, 1, 0, 0)


def test_tiles_and_grid(table):
    cu = 256
    rows = [  # (slots, tiles, grid)
        (0, 0, 0), (1, 1, 1), (1023, 1, 1), (1024, 1, 1), (1025, 2, 2), (2**20, 1024, 1024), (2**20 + 1, 1025, 1025), (PER_CU * cu * TILE, 2048, 2048),
        (PER_CU * cu * TILE + 1, 2049, 2048), (BOUND, 2**21, 2048)]
    got = table([f"plan {s} {cu} 1 0 1" for s, _, _ in rows])
    for (s, tiles, grid), g in zip(rows, got):
        assert (g["slots"], g["tile"], g["block"], g["tiles"], g["grid"]) == (s, TILE, BLOCK, tiles, grid), s
    small = table([f"plan {BOUND} 1 0 0 0", f"plan {BOUND} 0 0 0 0", "plan 5000 304 0 0 0"])
    assert [g["grid"] for g in small] == [8, 8, 5]
    # the grid never exceeds the tiles, the tiles cover the slots, and the last tile is not empty
    for s, tiles, grid in rows:
        assert grid <= tiles and tiles * TILE >= s and (tiles == 0 or (tiles - 1) * TILE < s)


def test_the_variant_and_the_texture_phase(table):
    got = table([f"plan 5000 256 {t} {p} {w}" for t in (0, 1) for p in (0, 1) for w in (0, 1)])
    k = 0
    for t in (0, 1):
        for p in (0, 1):
            for w in (0, 1):
                assert got[k]["prog"] == (t and p) and got[k]["tex_phase"] == (t and w), (t, p, w)
                k += 1


def test_predicates_over_every_meta_word(table):
    cases = [(kind, style, tex, root, fl) for kind in (SPHERE, UNBOUNDED_SPHERE, PLANE) for style in range(7 if kind != PLANE else 4) for tex in (-1, 0, 252)
             for root in (0, 1, 2, 3, 5) for fl in (0, 1)]
    got = table([f"pred {k} {s} {t} {r} {f}" for k, s, t, r, f in cases])
    for (kind, style, tex, root, fl), g in zip(cases, got):
        carries = style == 0 if kind == PLANE else style != 1  # the styles that hold a Texture
        want_tex = tex if (tex >= 0 and carries) else -1
        assert g["texture_of"] == want_tex, (kind, style, tex)
        assert g["phase"] == g["uv"] == int(want_tex >= 0 and root != 0), (kind, style, tex, root)
        assert g["emitter"] == int(style == 0 if kind == PLANE else style <= 1), (kind, style)


def test_the_no_surface_predicate(table):
    rows = [(-3, 5, 1, 0, 1), (-2, 5, 1, 1, 1), (-1, 5, 1, 1, 1), (0, 5, 1, 1, 0), (4, 5, 1, 1, 0), (5, 5, 1, 0, 1), (0, 5, 0, 1, 1), (-1, 5, 0, 1, 1),
            (BOUND, BOUND, 1, 0, 1), (BOUND - 1, BOUND, 1, 1, 0), (-2**31, 5, 1, 0, 1), (0, 0, 1, 0, 1)]
    got = table([f"slot {h} {n} {f}" for h, n, f, _, _ in rows])
    for (h, n, f, ok, none), g in zip(rows, got):
        assert (g["ok"], g["none"]) == (ok, none), (h, n, f)
