"""A numpy model of the level-by-level build of BoundingBoxTree.make's tree, written from the rules of csrc/rt_tree_plan.h (the shape as a
function of n, the unique sort key, the two merge rules, the cost, the first minimum) -- not from any other implementation.  It is what
tests/test_tree_cases.py holds against rt_tree_make_host (bit for bit) and tests/fsharp_literal.tree_make (by value).

    build(boxes)                   -> skip, prim, node_boxes, order
    build(boxes, tie="index")      mutant: equal keys ordered by box index instead of by position in the segment's current order
    build(boxes, left="half")      mutant: the left child takes c/2 boxes instead of c/2 + 1
    build(boxes, axis="last")      mutant: the last minimum axis instead of the first
"""
import numpy as np


def left_count(c, left="reference"):
    c = np.asarray(c)
    return np.where(c == 2, 1, c // 2 + (1 if left == "reference" else 0))


def plan(n, left="reference"):
    """The levels of the tree over n boxes: per level the arrays (start, count, node) of its segments, in position order."""
    levels = []
    start, count, node = np.array([0]), np.array([n]), np.array([0])
    while len(start):
        levels.append((start, count, node))
        split = count >= 2
        s, c, d = start[split], count[split], node[split]
        nl = left_count(c, left)
        start = np.stack([s, s + nl], 1).ravel()
        count = np.stack([nl, c - nl], 1).ravel()
        node = np.stack([d + 1, d + 2 * nl], 1).ravel()
    return levels


def depth(n):
    d, c = (1 if n else 0), n
    while c > 1:
        c = 1 if c == 2 else c // 2 + 1
        d += 1
    return d


def _ordered_runs(cols, starts):
    """BoundingBox.merge over runs of boxes in order (cols: [m, 6] = minx, maxx, ...; a run starts at each of `starts`): the minimum keeps
    the LATER operand of a tie, the maximum the EARLIER one, which is visible only as the sign of a zero."""
    m = len(cols)
    pos = np.arange(m)
    out = np.empty((len(starts), 6))
    for k in range(6):
        v = cols[:, k]
        zero = v == 0.0
        if k % 2 == 0:
            r = np.minimum.reduceat(v, starts)
            pick = np.maximum.reduceat(np.where(zero, pos, -1), starts)  # the last zero of the run
        else:
            r = np.maximum.reduceat(v, starts)
            pick = np.minimum.reduceat(np.where(zero, pos, m), starts)  # the first zero of the run
        fix = r == 0.0
        r = r.copy()
        r[fix] = v[pick[fix]]
        out[:, k] = r
    return out


def _volume(b):
    return ((b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2])) * (b[:, 5] - b[:, 4])


def build(boxes, tie="position", left="reference", axis="first"):
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    n = len(boxes)
    nn = 2 * n - 1 if n else 0
    skip, prim, nb = np.zeros(nn, np.int32), np.full(nn, -1, np.int32), np.zeros((nn, 6))
    if n == 0:
        return skip, prim, nb, np.zeros(0, np.int32)
    ids = np.arange(n)
    nb[0] = _ordered_runs(boxes, np.array([0]))[0]
    skip[0] = nn
    if n == 1:
        prim[0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for start, count, node in plan(n, left):
            slot = np.repeat(np.arange(len(start)), count)
            # the positions of Leaves that ended above this level are in no segment of it any more
            covered = np.zeros(n + 1, np.int64)
            np.add.at(covered, start, 1)
            np.add.at(covered, start + count, -1)
            alive = np.cumsum(covered[:-1]) > 0
            where = np.flatnonzero(alive)  # positions, ascending; where[k] is in segment slot[k]
            big = count >= 3
            two = count == 2
            # Leaves of a two-box Branch: no sort
            for s, d in zip(start[two], node[two]):
                for k in (0, 1):
                    prim[d + 1 + k], skip[d + 1 + k], nb[d + 1 + k] = ids[s + k], d + 2 + k, boxes[ids[s + k]]
            if not big.any():
                continue
            nl = left_count(count, left)
            run_starts_pos = np.sort(np.concatenate([start, (start + nl)[big]]))  # in positions
            run_starts = np.searchsorted(where, run_starts_pos)  # in indices of `where`
            run_of = {int(p): k for k, p in enumerate(run_starts_pos)}
            cur = ids[where]
            costs, merged, orders = [], [], []
            for a in range(3):
                key = boxes[cur, 2 * a] + 0.0  # -0.0 + 0.0 = +0.0: both zeros tie
                last = cur if tie == "index" else where
                o = np.lexsort((last, key, slot))
                m = _ordered_runs(boxes[cur[o]], run_starts)
                lrun = np.array([run_of[int(s)] for s in start[big]])
                L, R = m[lrun], m[lrun + 1]
                costs.append(_volume(L) + _volume(R))
                merged.append((L, R))
                orders.append(o)
            best = np.zeros(big.sum(), np.int64)
            bc = costs[0].copy()
            for a in (1, 2):
                better = costs[a] <= bc if axis == "last" else costs[a] < bc
                best[better] = a
                bc[better] = costs[a][better]
            new = ids.copy()
            index_of = np.full(n, -1)
            index_of[where] = np.arange(len(where))
            for k, (s, c, d, l) in enumerate(zip(start[big], count[big], node[big], nl[big])):
                a = best[k]
                lo = index_of[s]
                seg = cur[orders[a][lo:lo + c]]
                new[s:s + c] = seg
                L, R = merged[a][0][k], merged[a][1][k]
                ln, rn, r = d + 1, d + 2 * l, c - l
                nb[ln], skip[ln], prim[ln] = L, ln + 2 * l - 1, seg[0] if l == 1 else -1
                nb[rn], skip[rn], prim[rn] = R, rn + 2 * r - 1, seg[l] if r == 1 else -1
            ids = new
    return skip, prim, nb, ids.astype(np.int32)
