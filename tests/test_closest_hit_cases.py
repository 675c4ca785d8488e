"""No GPU: the cases of tests/closest_hit_cases.py are what they claim to be.  The coverage conditions hold (no class drops more than a
tenth of its candidates, every class keeps at least 64 rays per pair, every unbounded pair occurs in every shape of the unbounded
list); the numpy model of Scene.hitObject gives each class the winner its table states and each mutant of the rule is caught by the
classes built to catch it; the oracle equals the model and the literal restatement (tests/fsharp_literal.py) on every crafted ray,
hit index and strike bits, and on every class of InfinitePlane.intersection; the mirror scene's bounce rays and the two frame
classes are decided as their classes say."""
import math

import numpy as np
import pytest

import closest_hit_cases as chc
import fsharp_literal as L
from test_oracle_vs_literal import to_literal

ALL = chc.RESIDENT + [("mirror",)]


def _class_of(b):
    """Each crafted ray's class: (leaf, leaf) and at_infinity count as classes of their own."""
    return np.where(b.pair == "leaf_leaf", "leaf_leaf", b.cls_of)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_coverage():
    """Conditions, not measurements: the lattice sizes are chosen so that the model alone meets them."""
    kept, cand = {}, {}
    for key in ALL:
        b = chc.scene(key)
        dropped = b.candidates - len(b)
        assert dropped * 10 <= b.candidates, (key, dropped, b.candidates)
        for c, p in zip(_class_of(b).tolist(), b.pair.tolist()):
            kept[(c, p)] = kept.get((c, p), 0) + 1
        cand[b.cls] = cand.get(b.cls, 0) + b.candidates
    for (c, p), n in sorted(kept.items()):
        print(f"{c:16s} {p:14s} kept {n}")
    print("candidates per class:", cand)
    for c in chc.CLASSES:
        for p in chc.PAIRS:
            assert kept[(c, p)] >= 64, (c, p, kept.get((c, p)))
    assert kept[("leaf_leaf", "leaf_leaf")] >= 64 and kept[("at_infinity", "infinite")] >= 64
    for key in chc.PADDED:  # the same rays, and the same kept ones
        assert np.array_equal(chc.scene(key).rays, chc.scene(key[:-1]).rays) and chc.scene(key).padded and len(chc.scene(key).objs) > 1300


def test_unbounded_list_shapes():
    """Every unbounded pair occurs in the first two positions of the unbounded list, in the last two, separated by other objects, in
    a list of at least 40, and with n_bounded = 0; (leaf, plane) with a list of ONE unbounded object."""
    seen = {p: set() for p in chc.PAIRS_UU}
    for key in chc.RESIDENT:
        b = chc.scene(key)
        if not len(b) or b.cls == "at_infinity":
            continue
        pe, pl, nu = b.unbounded_position(b.earlier), b.unbounded_position(b.later), b.n_unbounded
        for p in chc.PAIRS_UU:
            m = b.pair == p
            if not m.any():
                continue
            assert (pe[m] >= 0).all() and (pe[m] < pl[m]).all(), (key, p)
            seen[p] |= {"first_two"} if ((pe[m] == 0) & (pl[m] == 1)).any() else set()
            seen[p] |= {"last_two"} if ((pe[m] == nu - 2) & (pl[m] == nu - 1)).any() else set()
            seen[p] |= {"separated"} if (pl[m] - pe[m] >= 8).any() else set()
            seen[p] |= {"forty"} if nu >= 40 else set()
            seen[p] |= {"no_tree"} if b.n_bounded == 0 else set()
    print(seen)
    for p in chc.PAIRS_UU:
        assert seen[p] == {"first_two", "last_two", "separated", "forty", "no_tree"}, (p, seen[p])
    for c in chc.BAND[1:3]:
        b = chc.scene(("single", c))
        assert b.n_unbounded == 1 and len(b) >= 64 and (b.pair == "leaf_plane").all()


# what catches which mutant: the classes in which the mutant's winner differs from the reference's, exactly these
CAUGHT_BY = {
    "strict": {"inside_nearer", "tiny"},                                             # a nearer later hit inside the band is taken
    "nearest": {"inside_nearer", "tiny", "at_infinity"},                             # ... and so is a lone hit at t = 1e160
    "last_equal": {"tie", "inside_nearer", "inside_farther", "tiny", "far_tie"},     # an "Equal" later hit is taken
    "compare_in_leaves": {"leaf_leaf"},                                              # a nearer Leaf inside the band is NOT taken
    "accept_infinite": {"at_infinity"},
}


def test_class_winners_and_mutants():
    differs = {r: {} for r in chc.RULES[1:]}
    for key in ALL:
        b = chc.scene(key)
        ref = b.model("reference")
        assert np.array_equal(ref, b.want), key  # the table's winner
        if b.cls == "at_infinity":
            assert (ref == -1).all()
        cls = _class_of(b)
        for r in chc.RULES[1:]:
            d = b.model(r) != ref
            for c in set(cls.tolist()):
                differs[r][c] = differs[r].get(c, 0) + int(d[cls == c].sum())
    for r, by in differs.items():
        print(r, {c: n for c, n in sorted(by.items()) if n})
        assert {c for c, n in by.items() if n} == CAUGHT_BY[r], (r, by)
        assert all(by[c] >= 64 for c in CAUGHT_BY[r]), (r, by)
    # the contrast: in (leaf, leaf) the nearer sphere wins although it is inside the band, whichever of the two is visited first
    b = chc.scene(("leaf_leaf",))
    pos = np.argsort(b.order)
    assert (b.want == b.later).all() and (pos[b.later] > pos[b.earlier]).sum() >= 64 and (pos[b.later] < pos[b.earlier]).sum() >= 64
    # the pulled-back rays are the two classes just outside the band
    for c, want_later in (("inside_nearer", True), ("inside_farther", False)):
        for rot in range(5):
            b = chc.scene(("class", c, rot))
            assert chc.in_class("outside_nearer" if want_later else "outside_farther", b.objs, b.extra, b.earlier, b.later).all()
            assert np.array_equal(b.model(rays=b.extra), b.later if want_later else b.earlier), (c, rot)


def _literal_hits(objs, rays):
    lit = to_literal(objs)
    scene = L.scene_make(lit)
    index = {id(h): k for k, h in enumerate(lit)}
    hit, strike = np.full(len(rays), -1, np.int32), np.full((len(rays), 3), np.nan)
    for k, r in enumerate(rays.tolist()):
        got = L.hit_object(scene, L.Ray(tuple(r[:3]), tuple(r[3:])))
        if got is not None:
            hit[k], strike[k] = index[id(got[0])], got[1]
    return hit, strike


@pytest.mark.parametrize("key", ALL, ids=chc.label)
def test_oracle_equals_the_model_and_the_literal(orc, key):
    """OracleScene.hit_object = the model's winner = the literal's hit_object on every crafted ray (and on the pulled-back and
    oblique extra rays of the scene): hit index and strike bits."""
    b = chc.scene(key)
    extra = np.array([orc.ray_make(r[:3], r[3:]) for r in b.extra]).reshape(-1, 6)
    rays = np.concatenate([b.crafted(), extra])
    hit, strike, _ = orc.OracleScene(b.objs).hit_object(rays)
    n = len(b)
    assert np.array_equal(hit[len(rays) - len(extra) - n:len(rays) - len(extra)], b.want), key
    lhit, lstrike = _literal_hits(b.objs, rays)
    assert np.array_equal(hit, lhit), (key, np.flatnonzero(hit != lhit)[:8])
    some = hit >= 0
    assert np.array_equal(_bits(strike[some]), _bits(lstrike[some])), key
    if b.cls != "at_infinity":  # (its oblique extra rays: the model leaves Ray.make' and the box tests out)
        assert np.array_equal(b.model(rays=rays), hit), key
    else:
        assert (hit == -1).all()


@pytest.mark.parametrize("key", chc.PADDED, ids=chc.label)
def test_padding_changes_no_answer(orc, key):
    b, base = chc.scene(key), chc.scene(key[:-1])
    for _, rays, _ in chc.ray_lists(key):
        made = np.array([orc.ray_make(r[:3], r[3:]) for r in rays])
        got, want = orc.OracleScene(b.objs).hit_object(made), orc.OracleScene(base.objs).hit_object(made)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1][got[0] >= 0]), _bits(want[1][want[0] >= 0]))
    assert np.array_equal(orc.OracleScene(b.objs).hit_object(b.rays)[0], b.want)


def test_lists_hold_the_crafted_rays():
    for key in ALL + chc.PADDED:
        b, lists = chc.scene(key), chc.ray_lists(key)
        crafted = b.crafted()
        assert [len(r) for _, r, _ in lists][:3] == list(chc.SIZES)
        for _, rays, which in lists:
            m = which >= 0
            assert np.array_equal(rays[m], crafted[which[m]]) and m.sum() >= min(len(crafted), len(rays) // 2) and (~m).sum() >= 32
        assert set(lists[-1][2][lists[-1][2] >= 0].tolist()) == set(range(len(crafted))), key  # the longest list holds them all


def test_plane_classes(orc):
    """orc.plane_intersection = the literal's plane_intersection (NaN for None) = plane_t, and every class answers what it is built
    for: the guards `Float.equal denominator 0.0` and `Float.positive t` decide."""
    cls = chc.plane_classes()
    for name, (rays, planes) in cls.items():
        assert len(rays) >= 64, name
        want = orc.plane_intersection(rays, planes)
        lit = [L.plane_intersection({"point": tuple(p[:3]), "normal": tuple(p[3:])}, L.Ray(tuple(r[:3]), tuple(r[3:]))) for r, p in zip(rays.tolist(), planes.tolist())]
        lit = np.array([math.nan if t is None else t for t in lit])
        t, den, raw = chc.plane_t(rays, planes)
        for other in (lit, t):
            assert np.array_equal(np.isnan(want), np.isnan(other)) and np.array_equal(_bits(want[~np.isnan(want)]), _bits(other[~np.isnan(other)])), name
        print(f"{name:20s} {len(rays)} rays, {int((~np.isnan(want)).sum())} hits")
        if name == "den_zero":
            assert (den == 0.0).all() and not np.signbit(den).any() and np.isnan(want).all()
        elif name == "den_negative_zero":
            assert (den == 0.0).all() and np.signbit(den).all() and np.isnan(want).all()
        elif name.startswith("den_inside"):
            assert (np.abs(den) == 0.9e-8).all() and (np.sign(den) == (1 if name.endswith("pos") else -1)).all() and np.isnan(want).all()
            assert (np.abs(raw) > 10.0).all()  # but for the guard, half of them would be hits
        elif name.startswith("den_outside"):
            assert (np.abs(den) == 1.1e-8).all() and (np.sign(den) == (1 if name.endswith("pos") else -1)).all()
            assert np.array_equal(~np.isnan(want), raw > 0.0) and 20 <= (raw > 0.0).sum() <= len(raw) - 20  # a hit, or behind
        elif name == "t_inside":
            assert (np.abs(raw - 0.9e-8) < 1e-14).all() and np.isnan(want).all()
        elif name == "t_outside":
            assert (np.abs(raw - 1.1e-8) < 1e-14).all() and np.array_equal(_bits(want), _bits(raw))
        elif name == "t_zero":
            assert (raw == 0.0).all() and np.signbit(raw).any() and not np.signbit(raw).all() and np.isnan(want).all()
        elif name == "t_negative":
            assert (raw < 0.0).all() and raw.max() > -1e-11 and np.isnan(want).all()
        elif name == "t_huge":
            with np.errstate(over="ignore"):
                assert (raw >= 1e160).all() and np.isfinite(raw).all() and np.isposinf(raw * raw).all() and np.array_equal(_bits(want), _bits(raw))
        elif name == "t_overflow":
            assert np.isposinf(want).all() and np.isfinite(rays).all() and np.isfinite(planes).all()
        elif name == "non_finite":
            assert (~np.isfinite(np.concatenate([rays, planes], axis=1))).sum() == len(rays) and np.isnan(want).any() and np.isinf(want).any()
        else:
            assert name in ("non_unit", "coordinates_1e-3", "coordinates_1e6") and 10 <= (~np.isnan(want)).sum() <= len(want) - 10
    assert len(cls) >= 15


def test_mirror_bounce_rays_are_decided_as_their_class_says(orc):
    """Scene.traceRay at depth 1 by the literal: the first leg meets the mirror alone and comes back along the axis as the crafted
    band ray; the colour is the class' winner's (the mirror is White with albedo 1)."""
    b = chc.scene(("mirror",))
    hit, strike, _ = orc.OracleScene(b.objs).hit_object(b.first_leg)
    assert (hit == b.mirror).all() and np.array_equal(strike, b.rays[:, :3])
    scene = L.scene_make(to_literal(b.objs))
    col = np.array([L.trace_ray(1, scene, {"Ray": L.Ray(tuple(r[:3]), tuple(r[3:])), "Colour": (255, 255, 255)}, L.FloatProducer(1, 2, 3, 4)) for r in b.first_leg.tolist()])
    assert np.array_equal(col, np.array([chc.colour_of(k) for k in b.want]))
    g0 = np.tile(np.array([[1, 2, 3, 4]], np.uint32), (len(b), 1))
    assert np.array_equal(orc.OracleScene(b.objs).trace_ray(1, b.first_leg, g0)[0], col)
    for c in chc.BAND:
        m = b.cls_of == c
        assert m.sum() >= 64 and (b.want[m] == (b.later if chc.EXPECT[c] == "later" else b.earlier)[m]).all(), c
    # at depth 0 the ray ends on the mirror: HotPink (Scene.fs:113-114)
    assert (orc.OracleScene(b.objs).trace_ray(0, b.first_leg, g0)[0] == (205, 105, 180)).all()


@pytest.mark.parametrize("name", chc.FRAMES)
def test_frame_classes_give_one_colour(orc, name):
    objs, cam, w, h = chc.frame(name)
    acc, rgb, st = orc.OracleScene(objs).render_rows(w, h, cam.to_abi(), seed=5, threads=4)
    assert acc.shape == (17, 33, 4) and (acc[..., 0] >= 6).all()
    want = chc.colour_of(0) if name == "tiny" else (0, 0, 0)  # the first listed, farther plane; nothing at all
    assert np.array_equal(acc[..., 1:], acc[..., :1] * np.array(want, np.int32)), name
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) == 1
    assert st["rays"] == st["samples"] == int(acc[..., 0].sum())
