"""Every argument refusal of the launching entry points, code and text, against a table recorded from the library as it was before
the entry points were rebuilt on shared pieces (tests/golden/refusal_messages.json).  The first fault found decides what
rt_last_error() says, so the ORDER of the checks inside each entry point is behaviour: besides one fault at a time, every entry
point gets inputs with two faults that different families test in different orders.  Nothing here needs a GPU: every case is refused
before a device is entered, and nothing a refused call was given is written.  The exception is the oldest entry points:
rt_render_device(_ex) enter the device before they test anything, and rt_render before it tests the scene, so without a device (or
with a bad device index) THAT is what they report.  The table holds what they say once a device is there; without one this test expects
RT_ERR_NO_DEVICE of exactly those cases.

    python tests/test_refusal_messages.py --record     # rewrites the table from the library RTFS_LIB selects
"""
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "refusal_messages.json")
MAX_W, MAX_H = 4, 3
COLS, ROWS = 2 * MAX_W + 1, 2 * MAX_H + 1
FRAME = COLS * ROWS
N, N_SAMPLES = 5, 2

_FRAME_HEAD = "scene cam max_w max_h seed device row_first row_stride n_rows flags"
_FP_HEAD = "scene device n footprints spp depth seed stream_base flags"
_PX_HEAD = "scene cam max_w max_h seed device n pixels flags"
_DEV = "stream options stats"
# entry point -> (family, extension kind, its arguments in order)
ENTRIES = {
    "rt_render": ("frame", None, _FRAME_HEAD + " accum rgb stats"),
    "rt_render_device": ("frame", None, _FRAME_HEAD + " accum rgb stream stats"),
    "rt_render_device_ex": ("frame", None, _FRAME_HEAD + " accum rgb " + _DEV),
    "rt_render_extend": ("frame", "extend", _FRAME_HEAD + " done accum rgb stats"),
    "rt_render_extend_device": ("frame", "extend", _FRAME_HEAD + " done accum rgb " + _DEV),
    "rt_render_extend_map": ("frame", "map", _FRAME_HEAD + " targets accum rgb stats"),
    "rt_render_extend_map_device": ("frame", "map", _FRAME_HEAD + " targets accum rgb " + _DEV),
    "rt_hit_objects": ("rays", None, "scene device n rays flags hit strike stats"),
    "rt_hit_objects_device": ("rays", None, "scene device n rays flags hit strike " + _DEV),
    "rt_trace_rays": ("rays", None, "scene device n rays rng seed stream_base sample depth flags colour stats"),
    "rt_trace_rays_device": ("rays", None, "scene device n rays rng seed stream_base sample depth flags colour " + _DEV),
    "rt_render_footprints": ("footprints", None, _FP_HEAD + " accum rgb stats"),
    "rt_render_footprints_device": ("footprints", None, _FP_HEAD + " accum rgb " + _DEV),
    "rt_render_footprints_extend": ("footprints", "extend", _FP_HEAD + " done accum rgb stats"),
    "rt_render_footprints_extend_device": ("footprints", "extend", _FP_HEAD + " done accum rgb " + _DEV),
    "rt_render_footprints_extend_map": ("footprints", "map", _FP_HEAD + " targets accum rgb stats"),
    "rt_render_footprints_extend_map_device": ("footprints", "map", _FP_HEAD + " targets accum rgb " + _DEV),
    "rt_render_pixels": ("pixels", None, _PX_HEAD + " accum rgb stats"),
    "rt_render_pixels_device": ("pixels", None, _PX_HEAD + " accum rgb " + _DEV),
    "rt_render_pixels_extend": ("pixels", "extend", _PX_HEAD + " done accum rgb stats"),
    "rt_render_pixels_extend_device": ("pixels", "extend", _PX_HEAD + " done accum rgb " + _DEV),
    "rt_camera_hits": ("camera_hits", None, "scene cam max_w max_h seed device n pixels sample_first n_samples flags hit strike rays_out stats"),
    "rt_camera_hits_device": ("camera_hits", None, "scene cam max_w max_h seed device n pixels sample_first n_samples flags hit strike rays_out " + _DEV),
}
OUTPUTS = ("accum", "rgb", "hit", "strike", "rays_out", "colour", "rng")


@dataclasses.dataclass(frozen=True)
class Entry:
    name: str
    family: str
    ext: str
    args: tuple

    def has(self, key):
        return key in self.args

    @property
    def host(self):
        return "stream" not in self.args

    @property
    def output(self):  # the ray lists' one mandatory output
        return "hit" if self.has("hit") else "colour"


def entries():
    return [Entry(k, fam, ext, tuple(args.split())) for k, (fam, ext, args) in ENTRIES.items()]


def _list_with(entry):
    px = np.array([0, 7, FRAME - 1, 7, 30], np.int32)
    px[3] = entry
    return px


BIG = 2**31            # one more than INT32_MAX
SHARD = dict(max_w=1 << 20, max_h=1 << 20, n_rows=2049)  # 2049 rows of 2097153 pixels: just above 2^32
UNSET = "options with struct_size 0"
has_camera = lambda e: e.has("cam")        # noqa: E731
has_options = lambda e: e.has("options")   # noqa: E731
frame = lambda e: e.family == "frame"      # noqa: E731
rays = lambda e: e.family == "rays"        # noqa: E731
counted = lambda e: e.has("n")             # noqa: E731
extend = lambda e: e.ext == "extend"       # noqa: E731
by_map = lambda e: e.ext == "map"          # noqa: E731
host_list = lambda e: e.host and e.has("pixels")  # noqa: E731
hits = lambda e: e.family == "camera_hits"  # noqa: E731

# (name, what differs from the valid call, the entry points it is a fault for).  A key an entry point does not take is ignored, so a
# case is listed only where at least its FIRST key is an argument of the entry point.
ONE_FAULT = [
    ("scene NULL", dict(scene=None), lambda e: True),
    ("camera NULL", dict(cam=None), has_camera),
    ("max_w 0", dict(max_w=0), has_camera),
    ("max_h negative", dict(max_h=-2), has_camera),
    ("image too large", dict(max_w=(1 << 20) + 1), has_camera),
    ("spp 0", dict(spp=0), lambda e: not rays(e)),
    ("spp too large", dict(spp=8000001), lambda e: not rays(e)),
    ("depth negative", dict(depth=-1), lambda e: has_camera(e) or e.has("depth")),
    ("depth too large", dict(depth=0x1000000), lambda e: has_camera(e) or e.has("depth")),
    ("row_stride 0", dict(row_stride=0), frame),
    ("row_first negative", dict(row_first=-1), frame),
    ("n_rows negative", dict(n_rows=-1), frame),
    ("rows past the image", dict(row_first=ROWS - 1, n_rows=2), frame),
    ("accum NULL", dict(accum=None), lambda e: e.has("accum")),
    ("rays NULL", dict(rays=None), rays),
    ("output NULL", dict(output=None), rays),
    ("footprints NULL", dict(footprints=None), lambda e: e.has("footprints")),
    ("pixels NULL", dict(pixels=None), lambda e: e.family == "pixels"),
    ("count above INT32_MAX", dict(n=BIG), counted),
    ("samples_done 11", dict(done=11), extend),
    ("samples_done 0", dict(done=0), extend),
    ("samples_done above the target", dict(done=21), extend),
    ("shard of 2^32 pixels", SHARD, lambda e: frame(e) and e.ext),
    ("cap 11", dict(spp=11), by_map),
    ("targets NULL", dict(targets=None), by_map),
    ("frame above INT32_MAX", dict(max_w=40000, max_h=40000), lambda e: e.has("pixels")),
    ("entry -1", dict(pixels=_list_with(-1)), host_list),
    ("entry past the frame", dict(pixels=_list_with(FRAME)), host_list),
    ("sample_first negative", dict(sample_first=-1), hits),
    ("n_samples 0", dict(n_samples=0), hits),
    ("sample range past 8000000", dict(sample_first=7999999, n_samples=2), hits),
    ("slots above INT32_MAX", dict(n=2**30, n_samples=2), hits),
    ("hit_index NULL", dict(hit=None), hits),
    ("no list and n past the frame", dict(pixels=None, n=FRAME + 1), hits),
    ("struct_size unset", dict(options=UNSET), has_options),
    ("block_threads 100", dict(options=dict(block_threads=100)), has_options),
    ("passes 3", dict(options=dict(passes=3)), has_options),
    ("chunk_pixels 65", dict(options=dict(chunk_pixels=65)), has_options),
]
# two faults at once: which one is reported differs between the families (and between host and device variants)
TWO_FAULTS = [
    ("accum NULL + spp 0", dict(accum=None, spp=0), lambda e: e.has("accum")),                # geometry first; footprints: the pointer first
    ("accum NULL + count above INT32_MAX", dict(accum=None, n=BIG), lambda e: e.has("accum") and counted(e)),
    ("count above INT32_MAX + spp 0", dict(n=BIG, spp=0), lambda e: counted(e) and not rays(e)),
    ("scene NULL + camera NULL", dict(scene=None, cam=None), has_camera),                   # rt_render: the camera
    ("scene NULL + count above INT32_MAX", dict(scene=None, n=BIG), lambda e: counted(e) and not has_camera(e)),
    ("accum NULL + rows past the image", dict(accum=None, row_first=ROWS - 1, n_rows=2), frame),
    ("accum NULL + struct_size unset", dict(accum=None, options=UNSET), lambda e: e.has("accum") and has_options(e)),
    ("struct_size unset + samples_done 0", dict(options=UNSET, done=0), lambda e: extend(e) and has_options(e)),
    ("struct_size unset + cap 11", dict(options=UNSET, spp=11), lambda e: by_map(e) and has_options(e)),
    ("samples_done 0 + shard of 2^32 pixels", dict(done=0, **SHARD), lambda e: frame(e) and extend(e)),
    ("targets NULL + shard of 2^32 pixels", dict(targets=None, **SHARD), lambda e: frame(e) and by_map(e)),
    ("depth negative + samples_done 0", dict(depth=-1, done=0), extend),
    ("samples_done above the target + count above INT32_MAX", dict(done=21, n=BIG), lambda e: extend(e) and counted(e)),
    ("targets NULL + spp too large", dict(targets=None, spp=8000001), by_map),
    ("rays NULL + count above INT32_MAX", dict(rays=None, n=BIG), rays),
    ("output NULL + depth negative", dict(output=None, depth=-1), rays),
    ("count above INT32_MAX + depth too large", dict(n=BIG, depth=0x1000000), rays),
    ("depth negative + struct_size unset", dict(depth=-1, options=UNSET), lambda e: has_options(e) and (has_camera(e) or e.has("depth"))),
    ("pixels NULL + frame above INT32_MAX", dict(pixels=None, max_w=40000, max_h=40000), lambda e: e.family == "pixels"),
    ("entry -1 + samples_done 0", dict(pixels=_list_with(-1), done=0), lambda e: host_list(e) and extend(e)),
    ("entry -1 + accum NULL", dict(pixels=_list_with(-1), accum=None), lambda e: host_list(e) and e.has("accum")),
    ("entry -1 + hit_index NULL", dict(pixels=_list_with(-1), hit=None), lambda e: host_list(e) and hits(e)),
    ("hit_index NULL + n_samples 0", dict(hit=None, n_samples=0), hits),
    ("hit_index NULL + slots above INT32_MAX", dict(hit=None, n=2**30, n_samples=2), hits),
    ("hit_index NULL + no list and n past the frame", dict(hit=None, pixels=None, n=FRAME + 1), hits),
    ("hit_index NULL + struct_size unset", dict(hit=None, options=UNSET), lambda e: hits(e) and has_options(e)),
    ("frame above INT32_MAX + sample_first negative", dict(max_w=40000, max_h=40000, sample_first=-1), hits),
]

# Every fail(RT_ERR_INVALID_ARGUMENT, "...") text of the entry points and of the check functions they call, as the library had them
# when the table was recorded: each occurs in the table at least once.
REFUSALS = [
    "scene is NULL", "camera is NULL", "max_width_coord and max_height_coord must be positive", "image too large",
    "samples_per_pixel must be >= 1", "samples_per_pixel too large for int32 sums (255*spp)", "bounce_depth must be >= 0", "bounce_depth too large",
    "bad row shard", "row shard exceeds the image", "d_accum is NULL", "accum_host is NULL", "accum is NULL",
    "rt_render_options.struct_size is not set", "rays is NULL", "output is NULL", "more than INT32_MAX rays",
    "footprints is NULL", "more than INT32_MAX footprints",
    "samples_done must be >= 12 (below, firstTrial differs and Count cannot tell a stopped pixel from a finished one)",
    "the target samples_per_pixel is below samples_done", "an extension takes shards of fewer than 2^32 pixels",
    "a map's samples_per_pixel (the bound on every target) must be >= 12 (a buffer rendered below cannot be continued)", "targets is NULL",
    "pixels is NULL", "more than INT32_MAX list entries", "a pixel list indexes frames of at most INT32_MAX pixels",
    "the pixel list has an entry outside the frame", "sample_first must be >= 0", "n_samples must be >= 1",
    "sample_first + n_samples exceeds 8000000", "more than INT32_MAX output slots (n * n_samples)", "hit_index is NULL",
    "pixels is NULL and n exceeds the frame's pixels",
    # check_settings' own (rt_launch_plan.h), through fail(RT_ERR_INVALID_ARGUMENT, m)
    "block_threads must be 0, 256, 512, 768 or 1024", "chunk_pixels must be in [0, 64]", "passes must be 0 (auto), 1 (fused) or 2 (two-pass)",
]
# Refusals only a device can produce: collect_stats reads them from the launch's scratch after the list builder's seal has run, so no
# call without a GPU reaches them (tests/test_gpu_extend.py, test_gpu_extend_map.py and test_gpu_pixels.py provoke them).
DEVICE_ONLY = [
    "the pixel list has an entry outside the frame, or accum is not a buffer of samples_done samples per entry; left unchanged",
    "the pixel list has an entry outside the frame; nothing was rendered",
    "accum or targets are not what the arguments say (a Count below 11, or a target above the cap); left unchanged",
    "accum is not a buffer of samples_done samples per pixel (a Count that is neither samples_done nor 11); left unchanged",
]


def enters_device_first(e, message):
    """The cases that are refused only after the device has been entered (see the module's docstring)."""
    return e.name in ("rt_render_device", "rt_render_device_ex") or (e.name == "rt_render" and message == "scene is NULL")


def cases():
    """(case name, entry point, what differs from the valid call), in a fixed order."""
    out = []
    for e in entries():
        for kind, table in (("", ONE_FAULT), ("two: ", TWO_FAULTS)):
            for name, change, applies in table:
                if applies(e):
                    out.append((f"{e.name}: {kind}{name}", e, change))
    return out


class Call:
    """One entry point's valid call over sentinel-filled buffers, with the changes of one case applied."""

    def __init__(self, rt, scene):
        self.rt, self.scene = rt, scene

    def values(self, e, change):
        rt, A = self.rt, self.rt._abi
        cam = rt.Camera.makeBasic(20, 1.0, COLS / ROWS, rt.Point.make(0.0, 0.0, -1.0), rt.Vector.unitise(rt.Vector.make(0.0, 0.0, 1.0)),
                                  rt.Vector.make(0.0, 1.0, 0.0)).to_abi()
        cam.bounce_depth = 3
        slots = N * N_SAMPLES
        v = dict(scene=self.scene.handle, cam=cam, max_w=MAX_W, max_h=MAX_H, seed=1, device=0, row_first=0, row_stride=1, n_rows=2, flags=0,
                 n=N, spp=20, depth=3, stream_base=0, sample=0, done=12, sample_first=0, n_samples=N_SAMPLES, stream=None, options=None,
                 rays=np.ones((N, 6)), footprints=np.ones((N, 12)), pixels=_list_with(7), targets=np.full(2 * COLS, 15, np.int32),
                 accum=np.full((2 * COLS, 4), 77, np.int32), rgb=np.full((2 * COLS, 3), 3, np.uint8), hit=np.full(slots, -7, np.int32),
                 strike=np.full((slots, 3), 2.5), rays_out=np.full((slots, 6), 4.5), colour=np.full((N, 3), 9, np.uint8),
                 rng=np.full((N, 4), 11, np.uint32), stats=A.rt_stats(rays=5, samples=9, pixels=4, kernel_ms=3.0))
        change = dict(change)
        if "output" in change:
            change[e.output] = change.pop("output")
        if "spp" in change and v["cam"] is not None:
            cam.samples_per_pixel = change["spp"]
        if "depth" in change:
            cam.bounce_depth = change["depth"]
        opt = change.pop("options", None)
        if opt == UNSET:
            v["options"] = A.rt_render_options()
            v["options"].struct_size = 0
        elif opt is not None:
            v["options"] = A.rt_render_options(**opt)
        v.update(change)
        return v

    def __call__(self, e, change):
        from ray_tracing_fsharp_amd import _lib
        v = self.values(e, change)
        before = {k: v[k].copy() for k in OUTPUTS if v[k] is not None}
        argv = []
        for key, ctype in zip(e.args, _lib.SIGNATURES[e.name][1]):
            x = v[key]
            if isinstance(x, np.ndarray):
                x = x.ctypes.data_as(ctype)
            elif isinstance(x, C.Structure):
                x = C.byref(x)
            argv.append(x)
        assert len(argv) == len(_lib.SIGNATURES[e.name][1])
        code = getattr(self.rt.lib, e.name)(*argv)
        message = (self.rt.lib.rt_last_error() or b"").decode()
        untouched = all(np.array_equal(v[k], b) for k, b in before.items())
        st = v["stats"]
        untouched = untouched and (st.rays, st.samples, st.pixels, st.kernel_ms) == (5, 9, 4, 3.0)
        return code, message, untouched


def _scene(rt):
    P, S, H, Tex, Px = rt.Point.make, rt.SphereStyle, rt.Hittable, rt.Texture.Colour, rt.Pixel
    return rt.Scene.make([H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, Tex(Px(200, 100, 50))), P(0.0, 0.0, 3.0), 1.0))])


def test_the_cases_cover_every_entry_point_and_family():
    all_cases = cases()
    assert len({name for name, _, _ in all_cases}) == len(all_cases)
    assert len(ENTRIES) == 23  # 11 host / device pairs, and rt_render_device_ex
    for e in entries():
        assert len([name for name, _, _ in all_cases if name.startswith(e.name + ": two: ")]) >= 3, e.name


def test_every_refusal_text_is_in_the_table():
    table = json.load(open(TABLE))
    recorded = {message for _, message in table.values()}
    assert all(code == 1 for code, _ in table.values())  # RT_ERR_INVALID_ARGUMENT
    for text in REFUSALS:
        assert text in recorded, text
    assert not recorded & set(DEVICE_ONLY)
    assert recorded <= set(REFUSALS), recorded - set(REFUSALS)
    # and the list is the library's: each text is in its source (the recorded one's; later sources may build them from pieces)
    assert len(set(REFUSALS)) == len(REFUSALS) and not set(REFUSALS) & set(DEVICE_ONLY)


def test_every_refusal_keeps_its_code_and_its_text_and_writes_nothing(rt):
    assert rt._abi.RT_ERR_INVALID_ARGUMENT == 1
    table = json.load(open(TABLE))
    call = Call(rt, _scene(rt))
    all_cases = cases()
    assert sorted(table) == sorted(name for name, _, _ in all_cases)
    no_device = rt.device_count() < 1
    wrong = []
    for name, e, change in all_cases:
        code, message, untouched = call(e, change)
        want = list(table[name])
        if no_device and enters_device_first(e, want[1]):
            want = [rt._abi.RT_ERR_NO_DEVICE, "no HIP device visible: the render path has no CPU fallback"]
        if [code, message] != want or not untouched:
            wrong.append((name, code, message, want, untouched))
    assert not wrong, wrong[:10]


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, ROOT)
    import ray_tracing_fsharp_amd as rt_

    call_ = Call(rt_, _scene(rt_))
    out_ = os.environ.get("REFUSAL_TABLE_OUT", TABLE)
    old_ = json.load(open(TABLE)) if os.path.exists(TABLE) else {}
    table_, kept_ = {}, 0
    for name_, e_, change_ in cases():
        code_, message_, untouched_ = call_(e_, change_)
        if code_ == rt_._abi.RT_ERR_NO_DEVICE and rt_.device_count() < 1 and (e_.name != "rt_render" or "scene" in change_):
            if name_ in old_:  # recorded where there is a device: kept
                table_[name_] = old_[name_]
                kept_ += 1
            continue
        # only a refusal may be recorded: anything else went on towards a device with this case's arguments
        assert code_ == rt_._abi.RT_ERR_INVALID_ARGUMENT and untouched_, (name_, code_, message_, untouched_)
        table_[name_] = [code_, message_]
    print(f"{kept_} cases of the entry points that enter the device first kept as they were")
    with open(out_, "w") as f_:
        json.dump(table_, f_, indent=0, sort_keys=True)
        f_.write("\n")
    print(f"{len(table_)} cases recorded from {rt_.LIB_PATH}")
