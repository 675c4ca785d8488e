"""Hittable.Reflection on the vertex classes of tests/reflection_cases.py: the oracle (oracle/oracle.cpp) against the line-by-line
restatement of Sphere.fs:150-300 and InfinitePlane.fs:43-99 (tests/fsharp_literal.py) -- absorbed flag, colour, outgoing ray (NaN
equal to NaN) and generator state, bit for bit -- and the coverage conditions that keep the classes where they claim to be.  The
conditions are computed from the inputs (reflection_cases.probe) and the oracle's outputs; the counts are conditions on the
EXPECTED values, not measurements of the code under test.  CPU only.  tests/test_gpu_reflection.py holds the device to the oracle
on the same vertices."""
import numpy as np
import pytest

import fsharp_literal as L
import reflection_cases as rc
from test_oracle_vs_literal import to_literal

A = rc.A
NAMES = [name for name, _ in rc.CLASSES]
LITERAL_PER_CLASS = 220


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


_RESULTS = {}


def oracle_results(orc, name):
    if name not in _RESULTS:
        v = rc.vertices(orc, name)
        _RESULTS[name] = rc.oracle_zoo(orc).reflection(v.idx, v.rays, v.colour, v.strike, v.state)
    return _RESULTS[name]


def test_state_for_gives_the_chosen_draws(orc):
    rng = np.random.default_rng(3)
    want = np.concatenate([[[0.0, 1.0, 0.5], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [rc.ABOVE_HALF, 0.3, 0.7]], rng.random((200, 3))])
    words = np.concatenate([[0x9E3779B9, 1, 0xFFFFFFFF, 2], rng.integers(1, 2 ** 32, 200)])
    for r, w in zip(want, words):
        st = rc.state_for(*r, w=int(w))
        assert st.dtype == np.uint32 and st.shape == (4,) and st.any()
        got = orc.float_producer(st, 3)
        assert np.array_equal(_bits(got), _bits(rc.attainable(r))), (r, w)
        assert np.all(np.abs(got - r) <= 0.5 / 4294967295.0 + 1e-17)
        g = L.FloatProducer(*(int(x) for x in st))
        assert np.array_equal(_bits(g.GetThree()), _bits(got))
    assert np.array_equal(rc.attainable([0.0, 1.0]), [0.0, 1.0])  # FloatProducer is inclusive at both ends
    st = rc.states_for(want, words)
    assert np.array_equal(_bits(rc.first_draw(st)), _bits(rc.attainable(want[:, 0])))
    after = np.array([[g.x, g.y, g.z, g.w] for g in (L.FloatProducer(*(int(x) for x in s)) for s in st) if g.GetThree()], np.uint32)
    assert np.array_equal(rc.draws(st, after), np.full(len(st), 3))


def test_the_zoo_holds_what_it_claims(orc):
    z = rc.zoo()
    hs, n, tex, ntex, _ = rc.rt.raytracing.flatten_hittables(rc.zoo(True).objs)
    assert n == len(z.objs) < 16384 and 20 < ntex < 254
    sph = ~z.is_plane
    assert set(z.style[sph]) == set(range(7)) and set(z.style[z.is_plane]) == set(range(4))
    for style in range(7):
        m = sph & (z.style == style)
        assert {(int(k), float(r)) for k, r in zip(z.kind[m], z.r[m])} >= {(A.RT_HITTABLE_SPHERE if b else A.RT_HITTABLE_UNBOUNDED_SPHERE, r) for b, r, _ in rc.GEOMETRIES}
        assert (np.abs(z.c[m]).max(axis=1) < 50).any() and (np.abs(z.c[m]).min(axis=1) > 900).any()
    refl = sph & (z.style >= 2)
    assert set(z.albedo[refl]) == set(rc.ALBEDO)
    assert set(z.fuzz[sph & (z.style == A.RT_SPHERE_FUZZED_REFLECTION)]) == set(rc.FUZZ)
    for style in (A.RT_SPHERE_DIELECTRIC, A.RT_SPHERE_GLASS):
        assert set(z.ior[sph & (z.style == style)]) == set(rc.IOR)
    assert set(z.prob[sph & (z.style == A.RT_SPHERE_DIELECTRIC)]) == set(rc.PROB)
    # the witnesses leave every vertex's first hit where it is
    allv = rc.concat([rc.vertices(orc, name).spread(300) for name in NAMES])
    for kind in ("tex", "planes"):
        objs = rc.witness(kind, cluster=True)
        assert [o.kind for o in objs[:len(z.objs)]] == [o.kind for o in z.objs] and len(objs) == len(z.objs) + 1000 + (1 if kind == "tex" else 6)
        hit, strike, _ = orc.OracleScene(objs).hit_object(allv.rays)
        assert np.array_equal(hit, allv.idx) and same_f64(strike, allv.strike)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_restatement(orc, name):
    v = rc.vertices(orc, name)
    print(f"{name}: {len(v)} vertices of {rc.CANDIDATES.get(name, rc.PER_CLASS)} candidates")
    assert len(v) >= rc.LEAST.get(name, 1500)
    # every vertex is where the kernel would find it: the ray's first hit, the strike the walk returns, a fixed point of Ray.make'
    hit, strike, _ = rc.oracle_zoo(orc).hit_object(v.rays)
    assert np.array_equal(hit, v.idx) and same_f64(strike, v.strike)
    sub = v.spread(80)
    assert all(same_f64(orc.ray_make(r[:3], r[3:]), r) for r in sub.rays)
    a, c, r, g = oracle_results(orc, name)
    lit = to_literal(rc.zoo().objs)
    pick = np.unique(np.concatenate([np.linspace(0, len(v) - 1, LITERAL_PER_CLASS).astype(np.int64), np.flatnonzero(np.isnan(r).any(axis=1))[:100]]))
    assert len(pick) >= 200
    for i in pick:
        obj = lit[int(v.idx[i])]
        light = {"Ray": L.Ray(tuple(v.rays[i, :3]), tuple(v.rays[i, 3:])), "Colour": tuple(int(x) for x in v.colour[i])}
        rand = L.FloatProducer(*(int(x) for x in v.state[i]))
        strike_i = tuple(v.strike[i])
        stop = L.plane_reflection(obj, light, strike_i, rand) if obj["kind"] == "plane" else L.sphere_reflection(obj, light, strike_i, rand)
        where = (name, int(i), int(v.idx[i]), obj["style"])
        assert (stop is not None) == bool(a[i]), where
        assert tuple(int(x) for x in c[i]) == (stop if stop is not None else light["Colour"]), where
        assert same_f64(np.array(light["Ray"].Origin + light["Ray"].Vector), r[i]), where
        assert [rand.x, rand.y, rand.z, rand.w] == [int(x) for x in g[i]], where


def _count(label, mask, least=50):
    k = int(mask) if isinstance(mask, (int, np.integer)) else int(np.count_nonzero(mask))
    print(f"  {label}: {k}")
    assert k >= least, label
    return k


def test_coverage_conditions(orc):
    z = rc.zoo()
    res = {}
    for name in NAMES:
        v = rc.vertices(orc, name)
        a, c, r, g = oracle_results(orc, name)
        res[name] = (v, rc.probe(z, v.idx, v.rays, v.strike), a, c, r, g, z.style[v.idx], z.is_plane[v.idx])
    flip = straight = tir = 0
    for name, (v, p, a, c, r, g, style, plane) in res.items():
        d_in = v.rays[:, 3:]
        at_strike = (_bits(r[:, :3]) == _bits(v.strike)).all(axis=1)
        flipped = (_bits(r[:, 3:]) == _bits(-1.0 * d_in)).all(axis=1) & at_strike & (a == 0)
        mirror = np.where(plane, np.isin(style, (1, 3)), np.isin(style, rc.MIRRORS))
        flip += np.count_nonzero(~p.have_v2 & mirror & flipped)
        through = ~p.have_v2 & ~plane & np.isin(style, (5, 6)) & ~flipped & at_strike & (np.abs(r[:, 3:] - d_in).max(axis=1) < 1e-15)
        straight += np.count_nonzero(through)
        # total internal reflection: the refract arm was drawn (Dielectric r <= prob, Glass r >= reflectionProb; the class draws
        # 0.0 and 1.0) and Float.compare sinO 1.0 = Greater; the outgoing ray then leaves on the side it came from
        if name == "tir":
            gl = style == A.RT_SPHERE_GLASS  # (on a sphere of negative radius cosI < 0 and reflectionProb > 1: Glass reflects there)
            thr = z.prob[v.idx].copy()
            thr[gl] = rc.glass_reflection_prob(z, v.idx[gl], rc._take_probe(p, gl))
            refract_arm = np.where(gl, rc.first_draw(v.state) >= thr, rc.first_draw(v.state) <= thr)
            taken = refract_arm & p.have_v2 & (rc.fcmp(p.sin_o, np.ones(len(v))) == rc.GT)
            came, left = rc.dot3(d_in, p.n), rc.dot3(r[:, 3:], p.n)
            assert np.all(np.sign(left[taken]) == -np.sign(came[taken]))
            band = refract_arm & p.have_v2 & (p.sin_o > 1.0) & ~taken
            assert np.array_equal(np.isnan(r[:, 3:]).all(axis=1), band) and not np.isnan(r[:, :3]).any()
            passed = refract_arm & p.have_v2 & (p.sin_o <= 1.0)
            assert np.all(left[passed] < 1e-9)  # refracted: -cosO (0 at sinO = 1) along the normal as used, whichever way that points on a sphere of negative radius
            tir += np.count_nonzero(taken)
            print("tir:")
            _count("sinO in (1, 1 + 1e-8]: NaN outgoing ray", band)
            _count("sinO <= 1: refracted", passed)
            for k in range(5):
                _count(f"aimed at 1 +- {k} ulp and within 4 ulp of it", (v.tag == k) & (np.abs(p.sin_o - 1.0) <= (k + 4) * 2.0 ** -52))
    print("all classes:")
    _count("flip branch (mirror, d along the normal)", flip)
    _count("straight-through branch (refraction, d along the normal)", straight)
    _count("total internal reflection taken", tir)
    nan_classes = {name for name, t in res.items() if np.isnan(t[4]).any()}
    print(f"  classes with NaN outgoing rays: {sorted(nan_classes)}")
    assert nan_classes == set(rc.NAN_CLASSES)

    v, p, a, c, r, g, style, plane = res["normal"]
    print("normal:")
    _count("exact pole, no v2", (v.tag == 0) & ~p.have_v2)
    _count("tilted, no v2", (v.tag > 0) & ~p.have_v2)
    _count("tilted, v2", (v.tag > 0) & p.have_v2)
    _count("from inside", p.inside)
    _count("from outside", ~p.inside)

    v, p, a, c, r, g, style, plane = res["grazing"]
    print("grazing:")
    cos = np.abs(p.cos_d)
    _count("|cosI| < 1e-6", cos < 1e-6)
    _count("cosI exactly 0 at a pole", (v.tag == 1) & (cos == 0.0))

    v, p, a, c, r, g, style, plane = res["surface_origin"]
    print("surface_origin:")
    for radius_sign in (1.0, -1.0):
        m = np.sign(z.r[v.idx]) == radius_sign
        _count(f"radius sign {radius_sign:+.0f}: inside decided by the Equal arm", m & (p.cmp == rc.EQ))
        _count(f"radius sign {radius_sign:+.0f}: Greater", m & (p.cmp == rc.GT))
        _count(f"radius sign {radius_sign:+.0f}: Less", m & (p.cmp == rc.LT))
    co = z.c[v.idx] - v.rays[:, :3]
    diff = rc.dot3(co, co) - z.r[v.idx] * z.r[v.idx]
    _count("|c - o|^2 - r^2 exactly 0", diff == 0.0)
    _count("within 4 ulp of r^2, not 0", (diff != 0.0) & (np.abs(diff) <= 4 * np.spacing(z.r[v.idx] ** 2)))

    v, p, a, c, r, g, style, plane = res["cap_band"]
    print("cap_band:")
    assert (style == A.RT_SPHERE_LIGHT_SOURCE_CAP).all() and a.all()
    for radius_sign in (1.0, -1.0):
        m = np.sign(z.r[v.idx]) == radius_sign
        for arm, label in ((rc.GT, "Greater"), (rc.EQ, "Equal"), (rc.LT, "Less")):
            _count(f"radius sign {radius_sign:+.0f}: {label}", m & (p.cap == arm))
    assert not c[p.cap != rc.GT].any()  # Black below the cap and inside the band
    _count("strike.x exactly lower", v.strike[:, 0] == p.lower)
    _count("strike.x within 4 ulp of lower, not equal", (v.strike[:, 0] != p.lower) & (np.abs(v.strike[:, 0] - p.lower) <= 4 * np.spacing(np.abs(p.lower))))

    v, p, a, c, r, g, style, plane = res["plane"]
    print("plane:")
    dn = rc.dot3(v.rays[:, 3:], p.n)
    _count("hit from the back", dn > 0.0)
    _count("no v2 (flip)", ~p.have_v2 & np.isin(style, (1, 3)))
    _count("|d.n| < 1e-6", np.abs(dn) < 1e-6)
    for st in range(4):
        _count(f"plane style {st}", style == st)

    v, p, a, c, r, g, style, plane = res["rng_edges"]
    print("rng_edges:")
    r1, prob = rc.first_draw(v.state), z.prob[v.idx]
    die = style == A.RT_SPHERE_DIELECTRIC
    above = (rc.attainable_int(prob).astype(np.float64) + 1.0) / 4294967295.0
    at_threshold = die & (r1 == prob)
    just_above = die & (rc.attainable(prob) == prob) & (r1 == above)
    _count("Dielectric refract arm at r = prob exactly", at_threshold)
    _count("Dielectric reflect arm at the draw just above prob", just_above)
    _count("Dielectric r = 0.0", die & (r1 == 0.0))
    _count("Dielectric r = 1.0", die & (r1 == 1.0))
    came, left = rc.dot3(v.rays[:, 3:], p.n), rc.dot3(r[:, 3:], p.n)
    no_tir = p.have_v2 & (p.sin_o < 0.99)
    assert np.all(left[at_threshold & no_tir] < 0.0)                                              # refracted: -cosO along the normal
    assert np.all(np.sign(left[just_above]) == -np.sign(came[just_above]))                        # came back
    gl = style == A.RT_SPHERE_GLASS
    thr = np.zeros(len(v))
    thr[gl] = rc.glass_reflection_prob(z, v.idx[gl], rc._take_probe(p, gl))
    # (reflectionProb > 1 on spheres of negative radius, where cosI < 0: every draw reflects there, 1.0 included)
    _count("Glass reflect arm at r = 1.0 < reflectionProb", gl & (r1 == 1.0) & (thr > 1.0))
    below = _count("Glass reflect arm at the draw just below reflectionProb", gl & (v.tag == 5) & (r1 < thr) & (thr <= 1.0))
    _count("Glass refract arm at the draw just above (or at) reflectionProb", gl & (r1 >= thr) & (r1 - thr <= 1.0 / 4294967295.0))
    m = gl & (v.tag == 5) & (r1 < thr) & (thr <= 1.0)
    assert below and np.all(thr[m] - r1[m] <= 1.0 / 4294967295.0) and np.all(np.sign(left[m]) == -np.sign(came[m]))
    assert (rc.draws(v.state, g) == 1).all()

    v, p, a, c, r, g, style, plane = res["retries"]
    print("retries:")
    n_draws = rc.draws(v.state, g)
    assert (n_draws >= 3).all() and (n_draws % 3 == 0).all()
    lambert_plane = plane & (style == A.RT_PLANE_LAMBERT_REFLECTION)
    _count("random_unit drew again (every |2 r - 1| < 5e-5)", (v.tag == 0) & (n_draws >= 6))
    assert np.array_equal((v.tag == 0), (v.tag == 0) & (n_draws >= 6))
    _count("sphere Lambert drew again (offset = -n)", (v.tag == 1) & ~plane & (n_draws >= 6))
    black = (v.tag == 1) & lambert_plane & (a == 1) & ~c.any(axis=1) & (n_draws == 3)
    _count("plane Lambert absorbed Black", black)
    assert np.array_equal(black, (v.tag == 1) & lambert_plane)
    _count("sphere fuzz loop drew again (fuzz = 1.0, d = n)", (v.tag == 2) & ~plane & (n_draws >= 6))
    _count("plane fuzz loop drew again (fuzz = 1.0, d = n)", (v.tag == 2) & plane & (n_draws >= 6))
    assert np.array_equal((v.tag == 2), (v.tag == 2) & (n_draws >= 6))

    v, p, a, c, r, g, style, plane = res["ordinary"]
    print("ordinary:")
    hit = np.unique(v.idx)
    never = np.flatnonzero((z.kind == A.RT_HITTABLE_SPHERE) & (z.r < 0))
    assert set(hit) == set(range(len(z.objs))) - set(never)
    assert len(v) >= 1500
    assert (rc.draws(v.state, g) <= 3).mean() > 0.99  # a control: the retry loops are all but never reached by chance

    v, p, a, c, r, g, style, plane = res["schlick"]
    print("schlick:")
    assert (style == A.RT_SPHERE_GLASS).all() and (z.r[v.idx] > 0.0).all()
    r1 = rc.first_draw(v.state)
    own, other = rc.glass_reflection_prob(z, v.idx, p), rc.glass_reflection_prob(z, v.idx, p, other_side=True)
    apart = (r1 < own) != (r1 < other)
    assert apart.all()
    _count("from outside (the term of sr = ior decides)", apart & ~p.inside)
    _count("from inside (the term of sr = 1 / ior decides)", apart & p.inside)
    _count("the draw reflects with the side's own Schlick term, refracts with the other side's", apart & (r1 < own))
    _count("the draw refracts with the side's own Schlick term, reflects with the other side's", apart & (r1 >= own))
    for ior in np.unique(z.ior[v.idx]):
        _count(f"ior {float(ior)!r}", z.ior[v.idx] == ior)
    # (where the refraction is a total internal reflection both decisions give the same ray: only the other vertices show the term)
    for side, m in (("outside", ~p.inside), ("inside", p.inside)):
        _count(f"from {side}, and the outgoing ray depends on the decision (sinO not above 1)", m & (rc.fcmp(p.sin_o, np.ones(len(v))) != rc.GT))
    # the oracle took the decision of the side's own term: a reflected ray leaves on the side it came from, a refracted one does not
    came, left = rc.dot3(v.rays[:, 3:], p.n), rc.dot3(r[:, 3:], p.n)
    no_tir = p.sin_o < 0.99
    assert np.all(left[r1 < own] > 0.0) and np.all(left[(r1 >= own) & no_tir] < 0.0) and np.all(came < 0.0)
    assert (rc.draws(v.state, g) == 1).all()
