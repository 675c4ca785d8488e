"""Named box sets for the surface-area build of the tree the device walks (csrc/rt_walk_plan.h; tests/test_walk_tree_host.py without a GPU,
tests/test_gpu_walk_tree.py on one).  The modes are tests/tree_cases.py's own generator (imported and left untouched) at sizes on both
sides of the 4096-box threshold between the full sweep and the binned split, plus one construction that reaches the median arm above it.

A case is (boxes [n, 6] float64 as minx, maxx, miny, maxy, minz, maxz, spheres [n, 4] or None)."""
import numpy as np

import tree_cases

SWEEP = 4096  # RTW_SWEEP
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 3, 20011]
MODES = ["random", "tied_y", "identical", "lattice", "negative", "zeros_sphere", "zeros_raw"]
OUTLIER = "outlier-4255"
PEEL = ["peel-64", "peel-4096"]


def outlier():
    """4200 small spheres in the unit cube plus 55 spheres at x = 64^k, k = 1..55, r = 0.25: every binned level peels the farthest
    outlier (it alone is in the last bin), so a node of 4208 boxes arrives at depth 48 and is halved by the median arm above 4096."""
    rng = np.random.default_rng(4255)
    small = np.concatenate([rng.uniform(0.0, 1.0, (4200, 3)), rng.uniform(0.005, 0.02, (4200, 1))], 1)
    far = np.array([[64.0 ** k, 0.5, 0.5, 0.25] for k in range(1, 56)])
    sp = np.concatenate([small, far], 0)[rng.permutation(4255)]
    return tree_cases.sphere_boxes(sp), sp


def peel(n):
    """n identical spheres of radius 0.5: the half area is exactly 3 and every product of a cost is exact, so every split of a sweep
    costs the same, the first minimum peels one box per level, and from depth 48 on the depth guard halves (64 boxes: depth 53).  The
    "identical" mode's random radius rounds the products differently from split to split, so its costs do not tie."""
    sp = np.tile(np.array([[1.0, 2.0, 3.0, 0.5]]), (n, 1))
    return tree_cases.sphere_boxes(sp), sp


def names():
    return [f"{m}-{n}" for n in SIZES for m in MODES] + [OUTLIER] + PEEL


_CASES = {}


def case(name):  # made once per name, shared and left unchanged
    if name not in _CASES:
        if name == OUTLIER:
            _CASES[name] = outlier()
        elif name in PEEL:
            _CASES[name] = peel(int(name.rsplit("-", 1)[1]))
        else:
            mode, n = name.rsplit("-", 1)
            _CASES[name] = tree_cases.make(mode, int(n))
    return _CASES[name]


def sphere_names():
    return [n for n in names() if case(n)[1] is not None]


def sphere_objects(rt, scenes, spheres):
    style = scenes.S.LambertReflection(0.5, scenes.Tex(scenes.Px(9, 9, 9)))
    return [scenes.H.Sphere(rt.Sphere.make(style, scenes.P(float(c[0]), float(c[1]), float(c[2])), float(c[3]))) for c in spheres]
