"""No GPU: the cases of tests/sphere_arm_cases.py are what they claim to be.  Every class' arm of `Float.compare disc 0.0` is
confirmed by the numpy restatement of the discriminant, the oracle's Sphere.firstIntersection gives each class the result the arm
implies, and the coverage conditions hold: no class drops more than a tenth of its candidates, every class keeps at least 64, the
tangent hit decides the oracle's Scene.hitObject for enough rays that a wrong Equal arm cannot hide behind another object, and
every lane pattern puts the rare rays where it says."""
import numpy as np
import pytest

import sphere_arm_cases as sac

SCENES = ("base", "zoo")


def _objects(scene):
    return sac.base_objects() if scene == "base" else sac.zoo_objects()


@pytest.mark.parametrize("scene", SCENES)
def test_every_class_lands_in_its_arm(scene):
    """disc = b*b - (dd - r^2) restated in the device's operation order: eq0 is exactly zero, the two Equal classes lie inside the
    band on their own side, the two edge classes just outside it, the reversed rays are Equal with -b not positive."""
    cls, sph = sac.classes(scene), sac.spheres_of(_objects(scene))
    for name, c in cls.items():
        if name == "ordinary":
            continue
        dropped = c.candidates - len(c)
        print(scene, name, "candidates", c.candidates, "kept", len(c))
        assert dropped * 10 <= c.candidates, (scene, name, dropped, c.candidates)
        assert len(c) >= 64, (scene, name, len(c))
        disc, b = sac.disc_of(c.rays, sph[c.target])
        arm = sac.arm_of(disc)
        if name == "eq0":
            assert (disc == 0.0).all()
        elif name in ("equal_pos", "equal_neg"):
            assert (arm == "equal").all() and (np.sign(disc) == (1.0 if name == "equal_pos" else -1.0)).all()
            assert (np.abs(disc) > 0.7e-8).all()
        elif name == "greater_edge":
            assert (arm == "greater").all() and (disc < 1.3e-8).all()
        elif name == "less_edge":
            assert (arm == "less").all() and (disc > -1.3e-8).all()
        else:
            assert name == "equal_behind" and (arm == "equal").all() and (b > 0.0).all()
        assert (np.abs(b) == np.rint(np.abs(b))).all() and (np.abs(b) >= 1.0).all() and (np.abs(b) <= 39.0).all()  # b = -+k exactly


@pytest.mark.parametrize("scene", SCENES)
def test_the_oracle_gives_each_class_its_arms_result(orc, scene):
    """Sphere.firstIntersection as the oracle restates it: t = -b = k in the Equal classes, the nearer root within 2e-4 of k just
    above the band, none below it and behind the origin."""
    cls, sph = sac.classes(scene), sac.spheres_of(_objects(scene))
    for name in sac.TANGENT:
        c = cls[name]
        t = orc.sphere_first_intersection(c.rays, sph[c.target])
        _, b = sac.disc_of(c.rays, sph[c.target])
        if name in sac.EQUAL:
            assert np.array_equal(t, -b), name
        elif name == "greater_edge":
            assert np.isfinite(t).all() and (t < -b).all() and (t > -b - 2e-4).all(), name
        else:
            assert np.isnan(t).all(), name
    c = cls["equal_behind"]
    assert np.isnan(orc.sphere_first_intersection(c.rays, sph[c.target])).all()


def test_an_infinite_discriminant_is_a_hit_at_infinity_that_never_wins(orc):
    """radius 1e160: RadiusSquared and every discriminant are +inf, Sphere.firstIntersection answers +inf (sqrt inf - b), and
    Scene.hitObject never reports that object: the two +inf scenes' hits are those of (a), ray for ray."""
    cls = sac.classes("base")
    rays = np.concatenate([cls[k].rays[:100] for k in cls])
    made = np.array([orc.ray_make(r[:3], r[3:]) for r in rays])
    huge = np.array([[1.0, 2.0, 3.0, sac.HUGE_RADIUS]] * len(made))
    disc, _ = sac.disc_of(made, huge)
    assert np.isposinf(disc).all()
    assert np.isposinf(orc.sphere_first_intersection(made, huge)).all()
    want = orc.OracleScene(sac.base_objects()).hit_object(made)[:2]
    for bounded in (False, True):
        hit, strike, _ = orc.OracleScene(sac.inf_objects(bounded)).hit_object(made)
        assert np.array_equal(hit, want[0]) and (hit != len(sac.base_objects())).all()
        assert np.array_equal(np.isnan(strike), np.isnan(want[1])) and np.array_equal(strike[hit >= 0], want[1][hit >= 0])


@pytest.mark.parametrize("scene", SCENES)
def test_the_tangent_hit_decides_the_scenes_answer(orc, scene):
    """Coverage: for at least 64 rays of each Equal class the oracle's Scene.hitObject reports the tangent sphere itself, at the
    tangent point (so a device that skips the Equal arm, or takes its roots instead, answers differently); bounded and unbounded
    targets are both among them in (a) -- the leaf pass and the unbounded tests -- and both positions of its unbounded list."""
    objs = _objects(scene)
    cls, osc = sac.classes(scene), orc.OracleScene(objs)
    for name in sac.EQUAL:
        c = cls[name]
        hit, strike, _ = osc.hit_object(c.rays)
        own = hit == c.target
        print(scene, name, "tangent sphere is the hit for", int(own.sum()), "of", len(c))
        assert own.sum() >= 64, (scene, name, int(own.sum()))
        tangent_point = c.rays[:, :3] + c.rays[:, 3:] * np.abs(sac.disc_of(c.rays, sac.spheres_of(objs)[c.target])[1])[:, None]
        assert np.array_equal(strike[own], tangent_point[own]), (scene, name)
        if scene == "base":
            assert {0, 2} <= set(c.target[own].tolist()), (name, sorted(set(c.target[own].tolist())))
            # a bounded sphere is tested only if the ray meets its Leaf's box (Scene.fs:41), and a ray that passes outside the sphere
            # at a pole passes outside that box: equal_neg reaches the Equal arm through the unbounded list alone
            assert any(t >= 3 for t in c.target[own]) == (name != "equal_neg"), (name, sorted(set(c.target[own].tolist())))
    hit, _, _ = osc.hit_object(cls["equal_behind"].rays)
    assert (hit != cls["equal_behind"].target).all()


def test_lane_patterns_hold_what_they_say():
    cls = sac.classes("base")
    for n in sac.SIZES:
        waves = [(f, min(f + 64, n)) for f in range(0, n, 64)]
        for p in sac.PATTERNS:
            m = sac.rare_lanes(p, n)
            for f, l in waves:
                w = m[f:l]
                want = {"none": 0, "lane0": 1, "lane63": 1, "alternate": (l - f + 1) // 2, "all": l - f}[p]
                assert w.sum() == want, (n, p, f)
                if p == "lane0":
                    assert w[0]
                if p == "lane63":
                    assert w[-1]
    lists = sac.all_lists(cls)
    assert len(lists) == len(sac.RARE) * len(sac.PATTERNS) * len(sac.SIZES)
    sph = sac.spheres_of(sac.base_objects())
    by_ray = {r.tobytes(): k for k in sac.RARE for r in cls[k].rays}
    for label, rays, m in lists:
        rare = label.split("/")[0]
        assert len(rays) == int(label.split("/")[2]) and [by_ray.get(r.tobytes()) == rare for r in rays] == m.tolist(), label
    assert sph.shape == (8, 4)
