"""Every refusal the Python layer raises by itself -- type and full text -- against a table recorded from the layer as it was when each
Scene call still had one half for numpy arrays and one for torch tensors (tests/golden/wrapper_refusals.json).  The first fault found
decides what is raised, so the ORDER of the checks inside a method is behaviour: besides one fault at a time, every method gets every
pair of faults that do not touch the same argument.  Refusals of the library (RtError) are tests/test_refusal_messages.py's.

Three parts.  "arrays" and "cpu tensors" need no GPU: an array fault is refused before the library is called, and a tensor that is not
on a GPU is refused for that at the latest.  "gpu tensors" holds what only a tensor on a GPU reaches (the checks of the arguments
behind the leading one, and device=); each of its calls also carries options whose struct_size is 0, which every device entry point
refuses before it enters a device, so a call the layer failed to refuse would still launch nothing.

    python tests/test_wrapper_refusals.py --record     # rewrites the table; without a GPU the "gpu tensors" part is kept as it was
"""
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wrapper_refusals.json")
MAX_W, MAX_H = 4, 3
COLS, ROWS = 2 * MAX_W + 1, 2 * MAX_H + 1
N = 5


def valid():
    """The arguments of a valid call, by name; a method takes those its entry in METHODS lists."""
    return dict(accum=np.full((2, COLS, 4), 12, np.int32), targets=np.full((2, COLS), 15, np.int32), rays=np.ones((N, 6)),
                rng=np.full((N, 4), 11, np.uint32), footprints=np.ones((N, 12)), pixels=np.array([0, 7, ROWS * COLS - 1, 7, 30], np.int32),
                list_accum=np.full((N, 4), 12, np.int32), list_targets=np.full(N, 15, np.int32), image=np.zeros((ROWS, COLS, 3), np.uint8),
                present=np.ones((ROWS, COLS), np.uint8), data=np.zeros(16, np.uint8))


# what an array of each name becomes under "dtype" (rng: the tensor route takes int32 bits, the array route does not)
WRONG_DTYPE = dict(accum=np.int64, targets=np.int64, rays=np.float32, rng=np.int32, footprints=np.float32, pixels=np.int64, list_accum=np.int64,
                   list_targets=np.int64, image=np.int8, present=np.float32, data=np.int8)

F = (MAX_W, MAX_H)
# method -> (its array arguments, the leading one first; the call).  s: the scene or the module, c: the camera, v: the arguments, kw: keywords
METHODS = {
    "extend_rows": ("accum", lambda s, c, v, kw: s.extend_rows(*F, c, v["accum"], 12, **kw)),
    "extend_rows_map": ("accum targets", lambda s, c, v, kw: s.extend_rows_map(*F, c, v["accum"], v["targets"], **kw)),
    "hitObject": ("rays", lambda s, c, v, kw: s.hitObject(v["rays"], **kw)),
    "traceRays": ("rays rng", lambda s, c, v, kw: s.traceRays(v["rays"], 3, rng=v["rng"], **kw)),
    "renderFootprints": ("footprints", lambda s, c, v, kw: s.renderFootprints(v["footprints"], 20, 3, **kw)),
    "renderFootprints extend": ("footprints list_accum", lambda s, c, v, kw: s.renderFootprints(v["footprints"], 20, 3, extend=(v["list_accum"], 12), **kw)),
    "renderFootprints extend_map": ("footprints list_accum list_targets",
                                    lambda s, c, v, kw: s.renderFootprints(v["footprints"], 20, 3, extend_map=(v["list_accum"], v["list_targets"]), **kw)),
    "renderPixels": ("pixels", lambda s, c, v, kw: s.renderPixels(*F, c, v["pixels"], **kw)),
    "renderPixels extend": ("pixels list_accum", lambda s, c, v, kw: s.renderPixels(*F, c, v["pixels"], extend=(v["list_accum"], 12), **kw)),
    "cameraHits": ("pixels", lambda s, c, v, kw: s.cameraHits(*F, c, v["pixels"], **kw)),
    "cameraPaths": ("pixels", lambda s, c, v, kw: s.cameraPaths(*F, c, v["pixels"], **kw)),
    "tracePaths": ("rays rng", lambda s, c, v, kw: s.tracePaths(v["rays"], 3, rng=v["rng"], **kw)),
}
# the output classes: no scene, no keywords
OUTPUTS = {
    "PixelOutput.correctImage": ("image", lambda rt, v: rt.PixelOutput.correctImage(v["image"])),
    "ImageOutput.formatPpm": ("image", lambda rt, v: rt.ImageOutput.formatPpm(True, v["image"])),
    "ImageOutput.formatPpmDevice": ("image", lambda rt, v: rt.ImageOutput.formatPpmDevice(True, v["image"])),
    "ImageOutput.formatPixelMap": ("image", lambda rt, v: rt.ImageOutput.formatPixelMap(v["image"])),
    "ImageOutput.writePpm": ("image", lambda rt, v: rt.ImageOutput.writePpm(True, lambda _: None, v["image"], os.devnull)),
    "ImageOutput.parsePixelMap": ("data", lambda rt, v: rt.ImageOutput.parsePixelMap(v["data"], ROWS, COLS)),
    "ImageOutput.missingPixels": ("present", lambda rt, v: rt.ImageOutput.missingPixels(v["present"])),
    "Png.format": ("image", lambda rt, v: rt.Png.format(True, v["image"])),
    "Png.formatDevice": ("image", lambda rt, v: rt.Png.formatDevice(True, v["image"])),
    "Png.write": ("image", lambda rt, v: rt.Png.write(True, lambda _: None, v["image"], os.devnull)),
}
# keyword faults: (name, the methods it is a fault for, keywords, arguments replaced)
KEYWORD_FAULTS = [
    ("options", list(METHODS), dict(options="set"), {}),
    ("extend and extend_map", ["renderFootprints extend"], dict(extend_map=(np.full((N, 4), 12, np.int32), np.full(N, 15, np.int32))), {}),
    ("n with pixels", ["cameraHits", "cameraPaths"], dict(n=3), {}),
    ("n_samples 2.0", ["cameraHits", "cameraPaths"], dict(n_samples=2.0), {}),
    ("sample_first 0.0", ["cameraHits", "cameraPaths"], dict(sample_first=0.0), {}),
    ("max_vertices 8.0", ["cameraPaths", "tracePaths"], dict(max_vertices=8.0), {}),
    ("n -1", ["cameraHits", "cameraPaths"], dict(n=-1), dict(pixels=None)),
]


def array_faults(key, leading):
    """(name, what the valid array becomes, whether the fault also goes into the pairs)."""
    out = [("a list", lambda a: a.tolist(), False), ("dtype", lambda a: a.astype(WRONG_DTYPE[key]), True),
           ("one dimension more", lambda a: a[None], False)]
    if valid()[key].ndim >= 2:
        out += [("one dimension fewer", lambda a: a[0], False), ("trailing width", lambda a: a[..., :-1], False)]
    if key == "accum":
        out.append(("columns", lambda a: a[:, :-1], False))
    if not leading:  # one entry MORE than the leading argument has: a call that went through would stay inside every buffer
        out.append(("length", lambda a: np.concatenate([a, a[:1]]), True))
    return out


def scene_faults(method):
    """One method's single faults: (name, arguments replaced, keywords, whether it goes into the pairs)."""
    keys = METHODS[method][0].split()
    out = []
    for i, key in enumerate(keys):
        for name, change, pairs in array_faults(key, i == 0):
            out.append((f"{key} {name}", {key: change(valid()[key])}, {}, pairs))
    for name, methods, kw, replaced in KEYWORD_FAULTS:
        if method in methods:
            out.append((name, replaced, kw, True))
    return out


def _pairs(faults):
    for (na, va, ka, pa), (nb, vb, kb, pb) in itertools.combinations(faults, 2):
        if pa and pb and not set(va) & set(vb) and not set(ka) & set(kb):
            yield f"{na} + {nb}", {**va, **vb}, {**ka, **kb}


def array_cases():
    """(case name, method, arguments replaced, keywords) of the array route."""
    out = []
    for method in METHODS:
        faults = scene_faults(method)
        out += [(f"{method}: {name}", method, v, kw) for name, v, kw, _ in faults]
        out += [(f"{method}: two: {name}", method, v, kw) for name, v, kw in _pairs(faults)]
    for method, (key, _) in OUTPUTS.items():
        if key == "image" and method.split(".")[1] not in ("correctImage", "formatPpmDevice", "formatDevice"):
            out.append((f"{method}: image one dimension fewer twice", method, {"image": valid()["image"][0, 0]}, {}))  # [3]: no rows and columns to read
    return out


def cpu_tensor_cases():
    """The tensor route with every array a tensor that is NOT on a GPU: the leading argument as it should be and with each fault, alone
    and with each keyword fault.  (A fault behind the leading argument is never reached: see gpu_tensor_cases.)"""
    out = []
    for method in METHODS:
        lead = METHODS[method][0].split()[0]
        leads = [("valid", {})] + [(f"{lead} {name}", {lead: change(valid()[lead])}) for name, change, _ in array_faults(lead, True) if name != "a list"]
        keywords = [("", {})] + [(" + " + name, kw) for name, methods, kw, replaced in KEYWORD_FAULTS if method in methods and not replaced]
        out += [(f"{method}: {ln}{kn}", method, v, kw) for (ln, v), (kn, kw) in itertools.product(leads, keywords)]
    for method, (key, _) in OUTPUTS.items():
        out.append((f"{method}: valid", method, {}, {}))
        out += [(f"{method}: {key} {name}", method, {key: change(valid()[key])}, {}) for name, change, _ in array_faults(key, True) if name != "a list"]
    return out


def _strided(a):
    """The same values behind a stride: a view of every other element of the last axis of a buffer twice as wide."""
    wide = np.repeat(a, 2, axis=-1)
    return ("strided", wide)


def gpu_tensor_cases():
    """What only a leading tensor on a GPU reaches.  A replaced argument is ("numpy" | "cpu" | "strided" | "gpu", array): where it lives."""
    out = []
    for method in METHODS:
        keys = METHODS[method][0].split()
        faults = [("device=1", {}, dict(device=1), True)]
        if keys[0] == "accum":
            faults.append(("accum not contiguous", {"accum": _strided(valid()["accum"])}, {}, False))
        for key in keys[1:]:
            a = valid()[key]
            faults += [(f"{key} not a tensor", {key: ("numpy", a)}, {}, True), (f"{key} not on a GPU", {key: ("cpu", a)}, {}, False),
                       (f"{key} length", {key: ("gpu", np.concatenate([a, a[:1]]))}, {}, True),
                       (f"{key} dtype", {key: ("gpu", a.astype(np.float32))}, {}, False)]
            if key != "rng":  # (rng is cloned, so it may be strided)
                faults.append((f"{key} not contiguous", {key: _strided(a)}, {}, False))
        if method == "renderFootprints extend":
            faults.append(("extend and extend_map", {}, dict(extend_map="tensors"), True))
        out += [(f"{method}: {name}", method, v, kw) for name, v, kw, _ in faults]
        out += [(f"{method}: two: {name}", method, v, kw) for name, v, kw in _pairs(faults)]
    return out


class Replay:
    def __init__(self, rt):
        P, S, H = rt.Point.make, rt.SphereStyle, rt.Hittable
        self.rt = rt
        self.scene = rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, rt.Texture.Colour(rt.Pixel(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])
        self.camera = rt.Camera.makeBasic(20, 1.0, COLS / ROWS, P(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)), rt.Vector.make(0.0, 1.0, 0.0))
        self.unset = rt._abi.rt_render_options()
        self.unset.struct_size = 0

    def place(self, x, where):
        """An argument of a case on its route: where = None (arrays as they are), "cpu" or "gpu" (arrays become tensors there)."""
        import torch
        if isinstance(x, tuple):
            kind, a = x
            if kind == "numpy":
                return a
            if kind == "strided":
                return torch.from_numpy(a).to("cuda")[..., ::2]
            return torch.from_numpy(a).to("cuda" if kind == "gpu" else "cpu")
        if where is None or not isinstance(x, np.ndarray):
            return x
        return torch.from_numpy(x).to("cuda" if where == "gpu" else "cpu")

    def __call__(self, method, replaced, kw, where=None):
        """[exception type, text] of one case ("nothing raised" if it went through)."""
        v = {k: self.place(a, where) for k, a in {**valid(), **replaced}.items()}
        kw = dict(kw)
        if kw.get("options") == "set":
            kw["options"] = self.rt._abi.rt_render_options()
        if kw.get("extend_map") == "tensors":
            kw["extend_map"] = (v["list_accum"], v["list_targets"])
        if where == "gpu":
            kw["options"] = self.unset
        try:
            if method in METHODS:
                METHODS[method][1](self.scene, self.camera, v, kw)
            else:
                OUTPUTS[method][1](self.rt, v)
        except Exception as e:  # noqa: BLE001  (the type is what is compared)
            return [type(e).__name__, str(e)]
        return ["nothing raised", ""]


PARTS = {"arrays": (array_cases, None), "cpu tensors": (cpu_tensor_cases, "cpu"), "gpu tensors": (gpu_tensor_cases, "gpu")}


def replay(rt, part):
    make, where = PARTS[part]
    run = Replay(rt)
    return {name: run(method, replaced, kw, where) for name, method, replaced, kw in make()}


def _compare(rt, part):
    want = json.load(open(TABLE))[part]
    got = replay(rt, part)
    assert sorted(got) == sorted(want)
    wrong = [(name, got[name], want[name]) for name in want if got[name] != want[name]]
    assert not wrong, wrong[:10]


def test_the_cases_have_distinct_names_and_every_method_has_pairs():
    for make, _ in PARTS.values():
        names = [name for name, _, _, _ in make()]
        assert len(set(names)) == len(names)
    for method in METHODS:
        assert any(name.startswith(method + ": two: ") for name, _, _, _ in array_cases()), method


def test_the_table_holds_only_the_layers_own_refusals():
    table = json.load(open(TABLE))
    assert sorted(table) == sorted(PARTS)
    for part in table.values():
        assert {kind for kind, _ in part.values()} <= {"TypeError", "ValueError", "IndexError"}
        assert all(text for _, text in part.values())


def test_array_refusals(rt):
    _compare(rt, "arrays")


def test_cpu_tensor_refusals(rt):
    _compare(rt, "cpu tensors")


@pytest.mark.gpu
def test_gpu_tensor_refusals(rt):
    _compare(rt, "gpu tensors")


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, ROOT)
    import ray_tracing_fsharp_amd as rt_

    old_ = json.load(open(TABLE)) if os.path.exists(TABLE) else {}
    table_ = {}
    for part_ in PARTS:
        if part_ == "gpu tensors" and rt_.device_count() < 1:
            table_[part_] = old_.get(part_, {})
            print(f"{part_}: no GPU, {len(table_[part_])} cases kept as they were")
            continue
        table_[part_] = replay(rt_, part_)
        # only a refusal of the layer's own may be recorded: anything else went on into the library with this case's arguments
        bad_ = {k: r for k, r in table_[part_].items() if r[0] not in ("TypeError", "ValueError", "IndexError")}
        assert not bad_, bad_
        print(f"{part_}: {len(table_[part_])} cases recorded")
    with open(os.environ.get("WRAPPER_TABLE_OUT", TABLE), "w") as f_:
        json.dump(table_, f_, indent=0, sort_keys=True)
        f_.write("\n")
