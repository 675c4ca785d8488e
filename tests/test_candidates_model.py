"""The timed kernel starts every camera ray of a pixel with the Leaves its pyramid can reach (pixel_candidates, csrc/rt_device.h)
instead of walking the tree.  That is legitimate only if the set CONTAINS every Leaf whose box some camera ray of the pixel hits
under the exact BoundingBox.hits (BoundingBox.fs:30-94).  Here: a bit-exact numpy model of the candidate walk
(tests/candidate_cases.py) against the oracle's exact box test, on cameras built by hand as an F# caller may build them -- off-grid
viewports, skewed and mirrored axes, flat pyramids, far and enclosed eyes -- and on Camera.makeBasic's.  The device is held to
the model in tests/test_gpu_candidates.py."""
import numpy as np
import pytest

import candidate_cases as cc
import ray_tracing_fsharp_amd as rt
import scenes


def _check_family(orc, family, legacy_gc=False):
    """-> (pixels, walked, lost): lost lists (case, row, col, leaves missed) for pixels whose candidates miss a reachable Leaf."""
    total = walked = 0
    lost = []
    for name, objs, cam, mw, mh, rc in family():
        s = rt.Scene.make(objs)
        cand, walk = cc.model(s, cam, mw, mh, rc, legacy_gc=legacy_gc)
        reach, ids = cc.reachable_leaves(orc, s, cam, mw, mh, rc, seed=len(name))
        for i in np.flatnonzero(~walk):
            need = set(int(x) for x in ids[reach[i]])
            have = set(int(x) for x in cand[i] if x >= 0)
            if not need <= have:
                lost.append((name, int(rc[i, 0]), int(rc[i, 1]), sorted(need - have)))
        total += len(rc)
        walked += int(walk.sum())
    return total, walked, lost


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
def test_candidates_contain_every_reachable_leaf(orc, family):
    total, walked, lost = _check_family(orc, cc.FAMILIES[family])
    assert not lost, f"{len(lost)} pixels lose a Leaf, first {lost[:3]}"
    assert walked < total, "every pixel walks: the family never reaches the candidate path"
    assert total - walked >= min(40, total // 4), (total, walked)


def test_the_eye_plane_without_its_guard_loses_a_hit(orc):
    """The kernel before the guard used the plane through the eye normal to the corners' sum for every pixel; family (a) reaches
    the cameras where that plane cuts the pyramid, and the old rule then drops a Leaf the exact test accepts."""
    _, _, lost = _check_family(orc, cc.family_off_centre, legacy_gc=True)
    assert lost
    assert any(name == "example" and row == 0 and col == 0 for name, row, col, _ in lost), lost[:5]


def test_the_guard_changes_nothing_for_the_bench_camera():
    """Config 3 (the bench frame, 2401 x 1601): for Camera.makeBasic every corner lies in front of the eye plane, so the guard
    keeps the plane on every pixel and the candidates are exactly those of the kernel before it (sampled rows, all columns)."""
    from ray_tracing_fsharp_amd import sample_images as si
    objs, cam, w, h = si.config3_final(seed=2024, spp=100, depth=50, pixels=800)
    s = rt.Scene.make(objs)
    rows = np.array([h - 1, h // 2, 7, 0, -1, -h // 3, -h + 5, -h - 1])
    rc = np.stack(np.broadcast_arrays(rows[:, None], np.arange(-w, w + 1)[None, :]), axis=-1).reshape(-1, 2).astype(np.int32)
    _, _, _, front = cc.pyramid(cam, w, h, rc)
    assert front.all()
    new, walk_new = cc.model(s, cam, w, h, rc)
    old, walk_old = cc.model(s, cam, w, h, rc, legacy_gc=True)
    assert np.array_equal(walk_new, walk_old) and np.array_equal(new, old)
    assert 0 < walk_new.sum() < len(rc) and (new[:, 0] >= 0).sum() > len(rc) // 4


def test_flat_pyramids_keep_their_pixels_on_the_candidate_path():
    """Family (c): the exact-zero degeneracy test does not send flat pyramids to the walk wholesale (rounding leaves their
    cross products non-zero), so the containment test above does exercise the candidate path on them."""
    n = 0
    for name, objs, cam, mw, mh, rc in cc.family_flat():
        _, walk = cc.model(rt.Scene.make(objs), cam, mw, mh, rc)
        n += int((~walk).sum())
    assert n > 0


def test_free_camera_refuses_a_viewport_at_the_eye():
    eye = (0.0, 0.0, 0.0)
    ok = scenes.free_camera(eye, (-0.25, -0.25, 0.05), (1, 0, 0), (0, 1, 0), 1.0, 1.0, 4, 2)
    assert scenes.require_clear_eye(ok, 1, 1) is ok
    assert abs(scenes.viewport_distance(ok, 1, 1) - 0.05) < 1e-15
    bad = scenes.free_camera(eye, (-0.25, -0.25, 5e-4), (1, 0, 0), (0, 1, 0), 1.0, 1.0, 4, 2)
    with pytest.raises(ValueError):
        scenes.require_clear_eye(bad, 1, 1)
    edge = scenes.free_camera((3.0, 0.5, 0.0), (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0), 1.0, 1.0, 4, 2)  # eye on the image's own plane
    assert abs(scenes.viewport_distance(edge, 1, 1) - 1.0) < 1e-15
    a = ok.to_abi()
    assert list(a.xaxis_dir) == [1.0, 0.0, 0.0] and list(a.yaxis_dir) == [0.0, 1.0, 0.0] and a.samples_per_pixel == 4
