"""A numpy model of what Scene.make computes around its two trees, in the form the device route computes it (csrc/rt_scene_kernels.h): the
stable partition, the ranks from the reference tree's depth-first leaf order, the depth of every walk-tree node from a difference array
over the pre-order ranges of the Branches, the stable order by depth, the outward rounding and the node32 record layout.  It is given
the two trees (rt_scene_get_tree, rt_scene_get_walk_tree) and returns what rt_scene_get_filter_tree and rt_scene_get_info expose.

mutant: None, or one deliberate fault a case must catch -- "unstable" (the order within a depth reversed), "nearest" (round to nearest
instead of outward), "input-rank" (rank taken in input order instead of leaf order)."""
import numpy as np

NODE, NODE32, MARK, WIDE = 112, 64, 0x4000, 0x80000000


def align16(v):
    return (v + 15) & ~15


def f32_outward(v, up, mutant=None):
    f = v.astype(np.float32)
    if mutant == "nearest":
        return f
    with np.errstate(invalid="ignore"):
        off = (f.astype(np.float64) < v) if up else (f.astype(np.float64) > v)
    return np.where(off, np.nextafter(f, np.float32(np.inf if up else -np.inf)), f)


def model(records, tree, walk, mutant=None):
    """tree, walk: (skip, prim, boxes) with prim as hittable indices.  -> dict(filter_boxes, filter_links, obj_to_orig, info)"""
    n = len(records)
    is_b = records["kind"] == 0
    bounded, unbounded = np.flatnonzero(is_b), np.flatnonzero(~is_b)  # order kept on both sides
    nb, nu = len(bounded), len(unbounded)
    tprim = tree[1]
    leaf_order = tprim[tprim >= 0] if mutant != "input-rank" else bounded
    obj_to_orig = np.concatenate([leaf_order, unbounded]).astype(np.int64)
    orig_to_obj = np.full(n, -1, np.int64)
    orig_to_obj[obj_to_orig] = np.arange(n)
    skip, wprim, boxes = (np.asarray(a) for a in walk)
    nn = len(skip)
    leaf = wprim >= 0
    # every Branch j covers the pre-order range (j, skip[j])
    diff = np.zeros(nn + 1, np.int64)
    np.add.at(diff, np.flatnonzero(~leaf) + 1, 1)
    np.add.at(diff, skip[~leaf], -1)
    depth = np.cumsum(diff)[:nn]
    order = np.argsort(depth, kind="stable") if mutant != "unstable" else np.lexsort((-np.arange(nn), depth))
    place = np.empty(nn + 1, np.int64)
    place[order] = np.arange(nn)
    place[nn] = nn
    fb = np.zeros((nn, 6), np.float32)
    fl = np.zeros((nn, 5), np.int32)
    if nn:
        lo, hi = f32_outward(boxes[:, 0::2], False, mutant), f32_outward(boxes[:, 1::2], True, mutant)
        at = place[:nn]
        fb[at, 0::2], fb[at, 1::2] = lo, hi
        rank = np.where(leaf, orig_to_obj[np.where(leaf, wprim, 0)], 0)
        entry = np.where(leaf, (MARK if n < 16384 else WIDE) | rank, 0)
        fl[at, 0] = np.where(leaf, place[skip], place[np.arange(nn) + 1])
        fl[at, 1] = place[skip]
        fl[at, 2] = entry.astype(np.uint32).view(np.int32)
        fl[at, 3] = np.where(leaf, 16, 0)
        fl[at, 4] = np.where(leaf, wprim, -1)
        with np.errstate(invalid="ignore"):
            mags = np.abs(np.concatenate([lo.ravel(), hi.ravel()]))
            bmax = np.float32(max(np.float32(1e-30), np.nanmax(np.where(np.isnan(mags), np.float32(0), mags))))
    else:
        bmax = np.float32(1e-30)
    radii = records["radius"][bounded]
    with np.errstate(invalid="ignore"):
        ok = bool(np.isfinite(bmax) and bmax <= np.float32(1000.0) and np.all((radii > 0.0) & (radii <= 100.0)))
        rmax = float(np.max(np.where(radii > 0.0, radii, 0.0), initial=0.0))
        implied = int(ok and rmax * float(bmax) <= 500.0)
    total = align16(align16(align16(align16(align16(nn * NODE) + n * 48) + n * 8) + nn * NODE32) + n * 32)
    info = {"n_bounded": nb, "n_unbounded": nu, "n_nodes": len(tree[0]), "walk_tree_nodes": nn, "leaf_box_implied": implied, "scene_bytes": total or 16}
    return {"filter_boxes": fb, "filter_links": fl, "obj_to_orig": obj_to_orig, "info": info}
