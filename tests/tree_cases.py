"""Named box sets for BoundingBoxTree.make's builders (tests/test_tree_cases.py without a GPU, tests/test_gpu_tree.py on one).

A case is (name, boxes [n, 6] float64 as minx, maxx, miny, maxy, minz, maxz, spheres or None).  `spheres` -- an [n, 4] array of centre and
radius -- is there for the cases a sphere can express: its box is Sphere.make's (centre + (-r) .. centre + r, Sphere.fs:333-336)."""
import numpy as np

S = 2048  # rt_tree_lds_boxes(): the largest segment one workgroup finishes in LDS (tests/test_tree_host.py holds the library to it)
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3, 20011]
MODES = ["random", "tied_y", "identical", "lattice", "negative", "zeros_sphere", "zeros_raw", "inf"]


def sphere_boxes(sp):
    c, r = sp[:, :3], sp[:, 3:4]
    b = np.empty((len(sp), 6))
    b[:, 0::2] = c + (-r)
    b[:, 1::2] = c + r
    return b


def _spheres(mode, n, rng):
    c = np.stack([rng.uniform(-9, 9, n), rng.uniform(0, 4, n), rng.uniform(-3, 15, n)], 1)
    r = rng.uniform(0.05, 0.4, n)
    if mode == "tied_y":  # the final scene's small spheres: centre.y = radius, so every Min.y is 0.0
        c[:, 1] = r
    elif mode == "identical":
        c[:], r[:] = c[0], r[0]
    elif mode == "lattice":  # a 3 x 2 x 3 lattice of centres, one radius: many ties on every axis
        k = np.arange(n)
        c = np.stack([(k % 3) * 1.5, ((k // 3) % 2) * 2.0, ((k // 6) % 3) * 1.25], 1)[rng.permutation(n)]
        r[:] = 0.5
    elif mode == "negative":  # inverted boxes
        r[::7] *= -1.0
    elif mode == "zeros_sphere":  # centre -0.0 or +0.0 on every axis, radius 0: minima and maxima of both zeros
        c = np.where(rng.integers(0, 2, (n, 3)) == 1, -0.0, 0.0)
        r[:] = 0.0
        r[::5] = rng.uniform(0.1, 1.0, len(r[::5]))
    return np.concatenate([c, r[:, None]], 1)


def make(mode, n, seed=0):
    rng = np.random.default_rng(seed * 1000003 + n * 17 + MODES.index(mode))
    if mode == "zeros_raw":  # raw boxes: every coordinate from {-0.0, +0.0, -1, 1}, so minima and maxima tie with either zero
        b = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0]), (n, 6), p=[0.35, 0.35, 0.15, 0.15])
        return b, None
    if mode == "inf":
        b = sphere_boxes(_spheres("random", n, rng))
        k = rng.integers(0, 8, n)
        b[k == 0, 0] = -np.inf
        b[k == 1, 1] = np.inf
        b[k == 2, 2] = np.inf  # an inverted infinite box
        b[k == 3, 4] = -np.inf
        b[k == 3, 5] = np.inf
        return b, None
    sp = _spheres(mode, n, rng)
    return sphere_boxes(sp), sp


def names():
    return [f"{m}-{n}" for n in SIZES for m in MODES]


def case(name):
    mode, n = name.rsplit("-", 1)
    boxes, spheres = make(mode, int(n))
    return boxes, spheres
