"""A numpy model of the surface-area build of the tree the device walks, written from the rules of csrc/rt_walk_plan.h (not from its code):
node layout, the full sweep up to 4096 boxes, 32 centroid bins above, halving from depth 48 on.  numpy does not fuse multiply-add, so the
arithmetic is the host's; minima and maxima of -0.0 and +0.0 may come out with either sign, so boxes compare with `==`, never by bits.

build(boxes) -> (skip, prim, node_boxes, info); info = {"depth": levels, "median_above": sizes of the nodes above 4096 boxes that were
halved, "binned": how many nodes were split on bins, "swept": how many by a full sweep}.  The keyword arguments are the mutants of
tests/test_walk_tree_host.py."""
import numpy as np

SWEEP, BINS, DEPTH = 4096, 32, 48


def _area(mn, mx, clamp):
    d = mx - mn
    if clamp:
        d = np.where(d > 0.0, d, 0.0)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 0] * d[..., 2]


def _first_min(c, last):
    """index of the first strict minimum as a sequential `<` scan finds it (a first NaN stays; later NaNs never win)"""
    if np.isnan(c[0]):
        return 0
    c = np.where(np.isnan(c), np.inf, c)
    if last:
        return len(c) - 1 - int(np.argmin(c[::-1]))
    return int(np.argmin(c))


def build(boxes, last_min=False, bins=BINS, weight_off=1, clamp=True):
    boxes = np.ascontiguousarray(boxes, np.float64)
    n = len(boxes)
    mn, mx = boxes[:, 0::2], boxes[:, 1::2]
    cen = mn + mx
    nn = max(2 * n - 1, 0)
    skip, prim, nb = np.zeros(nn, np.int32), np.full(nn, -1, np.int32), np.zeros((nn, 6))
    info = {"depth": 0, "median_above": [], "binned": 0, "swept": 0}
    if n == 0:
        return skip, prim, nb, info
    better = (lambda c, b: c <= b) if last_min else (lambda c, b: c < b)
    stack = [(np.arange(n), 0, 1)]
    while stack:
        ids, me, depth = stack.pop()
        m = len(ids)
        info["depth"] = max(info["depth"], depth)
        nb[me, 0::2], nb[me, 1::2] = mn[ids].min(0), mx[ids].max(0)
        skip[me] = me + 2 * m - 1
        if m == 1:
            prim[me] = ids[0]
            continue
        best_axis, best_cost, k, left, right, stuck = -1, 0.0, m // 2, None, None, False
        if depth < DEPTH:
            for axis in range(3):
                c = cen[ids, axis]
                if m <= SWEEP:
                    order = ids[np.lexsort((ids, c))]  # by (centroid, id); -0.0 == +0.0 ties go to the id
                    pmn, pmx = np.minimum.accumulate(mn[order], 0), np.maximum.accumulate(mx[order], 0)
                    smn, smx = np.minimum.accumulate(mn[order][::-1], 0)[::-1], np.maximum.accumulate(mx[order][::-1], 0)[::-1]
                    i = np.arange(1, m)
                    cost = (_area(pmn[:-1], pmx[:-1], clamp) * (2 * i - weight_off).astype(np.float64)
                            + _area(smn[1:], smx[1:], clamp) * (2 * (m - i) - weight_off).astype(np.float64))
                    j = _first_min(cost, last_min)
                    if best_axis < 0:
                        stuck = bool(np.isnan(cost[0]))  # a first candidate is accepted whatever it costs; nothing is < NaN
                    if best_axis < 0 or (not stuck and better(cost[j], best_cost)):
                        best_axis, best_cost, k = axis, cost[j], j + 1
                        left, right = order[:k], order[k:]
                else:
                    lo, hi = c.min(), c.max()
                    if not hi > lo:
                        continue
                    scale = np.float64(bins) / (hi - lo)
                    b = np.clip(((c - lo) * scale).astype(np.int64), 0, bins - 1)
                    cnt = np.bincount(b, minlength=bins)
                    bmn = np.array([mn[ids[b == q]].min(0) if cnt[q] else np.zeros(3) for q in range(bins)])
                    bmx = np.array([mx[ids[b == q]].max(0) if cnt[q] else np.zeros(3) for q in range(bins)])
                    for q in range(1, bins):
                        nl, nr = int(cnt[:q].sum()), int(cnt[q:].sum())
                        if nl == 0 or nr == 0:
                            continue
                        lu, ru = cnt[:q] > 0, cnt[q:] > 0
                        al = _area(bmn[:q][lu].min(0), bmx[:q][lu].max(0), clamp)
                        ar = _area(bmn[q:][ru].min(0), bmx[q:][ru].max(0), clamp)
                        cost = al * np.float64(2 * nl - weight_off) + ar * np.float64(2 * nr - weight_off)
                        if best_axis < 0:
                            stuck = bool(np.isnan(cost))
                        elif stuck or not better(cost, best_cost):
                            continue
                        best_axis, best_cost, k = axis, cost, nl
                        left, right = ids[b < q], ids[b >= q]
            if best_axis >= 0:
                info["binned" if m > SWEEP else "swept"] += 1
        if best_axis < 0:  # no winning axis, or depth >= 48: halve by (centroid on axis 0, id)
            order = ids[np.lexsort((ids, cen[ids, 0]))]
            k = m // 2
            left, right = order[:k], order[k:]
            if m > SWEEP:
                info["median_above"].append(m)
        stack.append((right, me + 2 * k, depth + 1))
        stack.append((left, me + 1, depth + 1))
    return skip, prim, nb, info
