"""Host-side mirror of the reference's scene-construction / render API over the C ABI (include/rtfs_amd.h).

Same names, argument order and error behaviour as the F# library (paths relative to /root/reference/RayTracing):
`Point.make`, `Vector.unitise`, `Colour.*`, `Texture.Colour`, `ParameterisedTexture.*`, `SphereStyle.*`, `Sphere.make`,
`InfinitePlaneStyle.*`, `InfinitePlane.make`, `Hittable.*`, `Camera.makeBasic`, `Scene.make`, `Scene.render`,
`Image.render`, `ImageOutput.writePpm`, `PixelOutput.correct`, `FloatProducer`.

Nothing here computes pixels: `Scene.render` hands the flattened scene to the HIP library.  Two things cannot cross
a C ABI and are mapped instead: the `FloatProducer` arguments of the styles are accepted and ignored
(randomness comes from `seed`), and `Texture.Arbitrary` closures must be one of the enumerated texture kinds.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import threading
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi as A
from ._lib import RtError, check, lib

TOLERANCE = 0.00000001  # Float.fs:82


# ---- Float.fs:31-76 --------------------------------------------------------------------------------------------
class FloatProducer:
    """xorshift128 + byte reversal + /UInt32.MaxValue (Float.fs:14-47).  `seed` is anything with four
    `.Next()`-style draws or an explicit (x, y, z, w); used host-side only, to build scenes reproducibly."""

    def __init__(self, state: Sequence[int]):
        self.x, self.y, self.z, self.w = (int(v) & 0xFFFFFFFF for v in state)

    def _next(self) -> int:
        t = (self.x ^ ((self.x << 11) & 0xFFFFFFFF)) & 0xFFFFFFFF
        self.x, self.y, self.z = self.y, self.z, self.w
        self.w = (self.w ^ (self.w >> 19) ^ (t ^ (t >> 8))) & 0xFFFFFFFF
        return self.w

    def Get(self) -> float:
        w = self._next()
        i = ((w & 0xFF) << 24) ^ (((w >> 8) & 0xFF) << 16) ^ (((w >> 16) & 0xFF) << 8) ^ ((w >> 24) & 0xFF)
        return float(i) / float(0xFFFFFFFF)

    def GetTwo(self) -> Tuple[float, float]:
        return self.Get(), self.Get()

    def GetThree(self) -> Tuple[float, float, float]:
        return self.Get(), self.Get(), self.Get()


# ---- Point.fs -----------------------------------------------------------------------------------------------------
class Point(NamedTuple):
    x: float
    y: float
    z: float

    @staticmethod
    def make(x: float, y: float, z: float) -> "Point":
        return Point(float(x), float(y), float(z))

    @staticmethod
    def differenceToThenFrom(p: "Point", q: "Point") -> "Vector":  # Point.fs:94
        return Vector(p.x - q.x, p.y - q.y, p.z - q.z)


class Vector(NamedTuple):
    x: float
    y: float
    z: float

    @staticmethod
    def make(x: float, y: float, z: float) -> "Vector":
        return Vector(float(x), float(y), float(z))

    @staticmethod
    def dot(a: "Vector", b: "Vector") -> float:  # Point.fs:18
        return a.x * b.x + a.y * b.y + a.z * b.z

    @staticmethod
    def unitise(v: "Vector") -> Optional["Vector"]:  # Point.fs:28-35 -> UnitVector voption
        d = Vector.dot(v, v)
        if abs(d - 0.0) < TOLERANCE:
            return None
        f = 1.0 / math.sqrt(d)
        return Vector(f * v.x, f * v.y, f * v.z)


UnitVector = Vector


# ---- Pixel.fs -----------------------------------------------------------------------------------------------------
class Pixel(NamedTuple):
    Red: int
    Green: int
    Blue: int


class Colour:  # Pixel.fs:18-76
    Black = Pixel(0, 0, 0)
    White = Pixel(255, 255, 255)
    Red = Pixel(255, 0, 0)
    Green = Pixel(0, 255, 0)
    Blue = Pixel(0, 0, 255)
    Yellow = Pixel(255, 255, 0)
    HotPink = Pixel(205, 105, 180)


# ---- Texture.fs ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class _ParamTex:
    kind: int
    pixel: Pixel = Colour.Black
    even: Optional["_ParamTex"] = None
    odd: Optional["_ParamTex"] = None
    grid: float = 0.0
    image: Optional[np.ndarray] = None  # [H, W, 3] uint8, img.[y].[x] order (Texture.fs:63-67)
    ramp: Tuple[int, int, int] = (0, 0, 0)


class ParameterisedTexture:  # Texture.fs:19-24
    @staticmethod
    def Colour(p: Pixel) -> _ParamTex:
        return _ParamTex(A.RT_TEXTURE_COLOUR, pixel=Pixel(*p))

    @staticmethod
    def Checkered(even: _ParamTex, odd: _ParamTex, gridSize: float) -> _ParamTex:
        return _ParamTex(A.RT_TEXTURE_CHECKERED, even=even, odd=odd, grid=float(gridSize))

    @staticmethod
    def Image(rows: np.ndarray) -> _ParamTex:
        img = np.ascontiguousarray(rows, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("Image texture must be [height, width, 3] uint8")
        return _ParamTex(A.RT_TEXTURE_IMAGE, image=img)

    @staticmethod
    def ofImage(bitmap_rows_top_first: np.ndarray) -> _ParamTex:
        """ParameterisedTexture.ofImage (Texture.fs:30-48): rows are reversed (y = Height - y - 1)."""
        return ParameterisedTexture.Image(np.ascontiguousarray(bitmap_rows_top_first[::-1]))

    @staticmethod
    def UvRamp(red, green, blue) -> _ParamTex:
        """The closed forms of the `ParameterisedTexture.Arbitrary` closures in RayTracing.App/SampleImages.fs:606-627:
        each channel is a constant byte, "u" (= byte (x * 255.0)) or "v" (= byte (y * 255.0))."""
        src, const = [], []
        for ch in (red, green, blue):
            if ch == "u":
                src.append(A.RT_RAMP_U); const.append(0)
            elif ch == "v":
                src.append(A.RT_RAMP_V); const.append(0)
            else:
                src.append(A.RT_RAMP_CONST); const.append(int(ch))
        return _ParamTex(A.RT_TEXTURE_UV_RAMP, pixel=Pixel(*const), ramp=tuple(src))

    @staticmethod
    def Arbitrary(_f: Callable) -> _ParamTex:
        raise RtError(A.RT_ERR_UNSUPPORTED, "Texture.Arbitrary closures cannot cross the C ABI; use UvRamp/Checkered/Image")

    @staticmethod
    def toTexture(interpret: Tuple[float, Point], texture: _ParamTex) -> "Texture":
        """ParameterisedTexture.toTexture (Texture.fs:69-72).  `interpret` is the pair (radius, centre) that the
        reference passes as `Sphere.planeMapInverse radius centre`."""
        radius, centre = interpret
        return Texture(param=texture, map_radius=float(radius), map_centre=Point(*centre))


@dataclasses.dataclass(frozen=True)
class Texture:  # Texture.fs:6-8
    pixel: Optional[Pixel] = None
    param: Optional[_ParamTex] = None
    map_radius: float = 1.0
    map_centre: Point = Point(0.0, 0.0, 0.0)

    @staticmethod
    def Colour(p: Pixel) -> "Texture":
        return Texture(pixel=Pixel(*p))


# ---- Sphere.fs / InfinitePlane.fs / Hittable.fs ------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class _Style:
    style: int
    albedo: float = 1.0
    texture: Optional[Texture] = None
    colour: Pixel = Colour.Black
    fuzz: float = 0.0
    ior: float = 1.0
    prob: float = 0.0


class SphereStyle:  # Sphere.fs:10-37
    @staticmethod
    def LightSource(texture: Texture) -> _Style:
        return _Style(A.RT_SPHERE_LIGHT_SOURCE, texture=texture)

    @staticmethod
    def LightSourceCap(colour: Pixel) -> _Style:
        return _Style(A.RT_SPHERE_LIGHT_SOURCE_CAP, colour=Pixel(*colour))

    @staticmethod
    def PureReflection(albedo: float, texture: Texture) -> _Style:
        return _Style(A.RT_SPHERE_PURE_REFLECTION, albedo=float(albedo), texture=texture)

    @staticmethod
    def FuzzedReflection(albedo: float, texture: Texture, fuzz: float, rand=None) -> _Style:
        return _Style(A.RT_SPHERE_FUZZED_REFLECTION, albedo=float(albedo), texture=texture, fuzz=float(fuzz))

    @staticmethod
    def LambertReflection(albedo: float, texture: Texture, rand=None) -> _Style:
        return _Style(A.RT_SPHERE_LAMBERT_REFLECTION, albedo=float(albedo), texture=texture)

    @staticmethod
    def Dielectric(albedo: float, texture: Texture, boundaryRefractance: float, refraction: float, rand=None) -> _Style:
        return _Style(A.RT_SPHERE_DIELECTRIC, albedo=float(albedo), texture=texture, ior=float(boundaryRefractance),
                      prob=float(refraction))

    @staticmethod
    def Glass(albedo: float, texture: Texture, ior: float, rand=None) -> _Style:
        return _Style(A.RT_SPHERE_GLASS, albedo=float(albedo), texture=texture, ior=float(ior))


class InfinitePlaneStyle:  # InfinitePlane.fs:3-13
    @staticmethod
    def LightSource(texture: Texture) -> _Style:
        return _Style(A.RT_PLANE_LIGHT_SOURCE, texture=texture)

    @staticmethod
    def PureReflection(albedo: float, colour: Pixel) -> _Style:
        return _Style(A.RT_PLANE_PURE_REFLECTION, albedo=float(albedo), colour=Pixel(*colour))

    @staticmethod
    def LambertReflection(albedo: float, colour: Pixel, rand=None) -> _Style:
        return _Style(A.RT_PLANE_LAMBERT_REFLECTION, albedo=float(albedo), colour=Pixel(*colour))

    @staticmethod
    def FuzzedReflection(albedo: float, colour: Pixel, fuzz: float, rand=None) -> _Style:
        return _Style(A.RT_PLANE_FUZZED_REFLECTION, albedo=float(albedo), colour=Pixel(*colour), fuzz=float(fuzz))


@dataclasses.dataclass(frozen=True)
class Sphere:  # Sphere.fs:302-337
    Style: _Style
    Centre: Point
    Radius: float

    @staticmethod
    def make(style: _Style, centre: Point, radius: float) -> "Sphere":
        return Sphere(style, Point(*centre), float(radius))


@dataclasses.dataclass(frozen=True)
class InfinitePlane:  # InfinitePlane.fs:101-119
    Style: _Style
    Normal: UnitVector
    Point: Point

    @staticmethod
    def make(style: _Style, pointOnPlane: Point, normal: UnitVector) -> "InfinitePlane":
        return InfinitePlane(style, Vector(*normal), Point(*pointOnPlane))


@dataclasses.dataclass(frozen=True)
class Hittable:  # Hittable.fs:3-6
    kind: int
    sphere: Optional[Sphere] = None
    plane: Optional[InfinitePlane] = None

    @staticmethod
    def Sphere(s: Sphere) -> "Hittable":
        return Hittable(A.RT_HITTABLE_SPHERE, sphere=s)

    @staticmethod
    def UnboundedSphere(s: Sphere) -> "Hittable":
        return Hittable(A.RT_HITTABLE_UNBOUNDED_SPHERE, sphere=s)

    @staticmethod
    def InfinitePlane(p: InfinitePlane) -> "Hittable":
        return Hittable(A.RT_HITTABLE_INFINITE_PLANE, plane=p)


# ---- Camera.fs ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Camera:  # Camera.fs:3-28; `dataclasses.replace(camera, BounceDepth=50)` is F#'s `{ camera with BounceDepth = 50 }`
    abi: A.rt_camera = dataclasses.field(repr=False, compare=False)
    SamplesPerPixel: int = 1
    BounceDepth: int = 150

    @staticmethod
    def makeBasic(samplesPerPixel: int, focalLength: float, aspectRatio: float, origin: Point, viewDirection: UnitVector,
                  viewUp: Vector) -> "Camera":
        out = A.rt_camera()
        check(lib.rt_camera_make_basic(int(samplesPerPixel), float(focalLength), float(aspectRatio), (C.c_double * 3)(*origin),
                                       (C.c_double * 3)(*viewDirection), (C.c_double * 3)(*viewUp), C.byref(out)))
        return Camera(out, SamplesPerPixel=int(samplesPerPixel), BounceDepth=int(out.bounce_depth))

    def to_abi(self) -> A.rt_camera:
        c = A.rt_camera()
        C.memmove(C.byref(c), C.byref(self.abi), C.sizeof(A.rt_camera))
        c.samples_per_pixel = int(self.SamplesPerPixel)
        c.bounce_depth = int(self.BounceDepth)
        return c

    ViewportWidth = property(lambda self: self.abi.viewport_width)
    ViewportHeight = property(lambda self: self.abi.viewport_height)
    FocalLength = property(lambda self: self.abi.focal_length)


# ---- flatten hittables into the ABI arrays --------------------------------------------------------------------------
def flatten_hittables(objects: Sequence[Hittable]):
    """-> (rt_hittable array, rt_texture array, keepalive list)."""
    texs: List[A.rt_texture] = []
    keep: List[np.ndarray] = []

    def add_param(t: _ParamTex) -> int:
        r = A.rt_texture()
        r.kind = t.kind
        r.even = r.odd = -1
        r.map_radius = 1.0
        if t.kind == A.RT_TEXTURE_CHECKERED:
            e, o = add_param(t.even), add_param(t.odd)  # children first: indices smaller than the parent's
            r.even, r.odd, r.grid_size = e, o, t.grid
        elif t.kind == A.RT_TEXTURE_IMAGE:
            keep.append(t.image)
            r.height, r.width = int(t.image.shape[0]), int(t.image.shape[1])
            r.texels = t.image.ctypes.data
        elif t.kind == A.RT_TEXTURE_UV_RAMP:
            r.ramp_src[:] = t.ramp
        r.rgb[:] = t.pixel
        texs.append(r)
        return len(texs) - 1

    hs = (A.rt_hittable * max(1, len(objects)))()
    for i, h in enumerate(objects):
        o = hs[i]
        o.kind = h.kind
        o.texture = -1
        st = h.plane.Style if h.kind == A.RT_HITTABLE_INFINITE_PLANE else h.sphere.Style
        o.style = st.style
        o.albedo, o.fuzz, o.ior, o.prob = st.albedo, st.fuzz, st.ior, st.prob
        colour = st.colour
        if st.texture is not None:
            if st.texture.pixel is not None:
                colour = st.texture.pixel
            else:
                idx = add_param(st.texture.param)
                texs[idx].map_radius = st.texture.map_radius
                texs[idx].map_centre[:] = st.texture.map_centre
                o.texture = idx
        o.rgb[:] = colour
        if h.kind == A.RT_HITTABLE_INFINITE_PLANE:
            o.point[:] = h.plane.Point
            o.normal[:] = h.plane.Normal
        else:
            o.point[:] = h.sphere.Centre
            o.radius = h.sphere.Radius
    tex_arr = (A.rt_texture * max(1, len(texs)))(*texs) if texs else (A.rt_texture * 1)()
    return hs, len(objects), tex_arr, len(texs), keep


# ---- Domain.fs ----------------------------------------------------------------------------------------------------
class Image:  # Domain.fs:9-31: rows are produced lazily, on first use
    def __init__(self, rowCount: int, colCount: int, force: Callable[[], np.ndarray]):
        self.RowCount, self.ColCount = rowCount, colCount
        self._force, self._rows = force, None

    @staticmethod
    def rowCount(i: "Image") -> int:
        return i.RowCount

    @staticmethod
    def colCount(i: "Image") -> int:
        return i.ColCount

    @staticmethod
    def make(rowCount: int, colCount: int, pixels) -> "Image":
        arr = np.asarray(pixels, dtype=np.uint8).reshape(rowCount, colCount, 3)
        return Image(rowCount, colCount, lambda: arr)

    @staticmethod
    def render(i: "Image") -> np.ndarray:
        """Image.render (Domain.fs:23-24): forces the rows; [RowCount, ColCount, 3] uint8, row 0 = top."""
        if i._rows is None:
            i._rows = i._force()
        return i._rows


# ---- Scene.fs -----------------------------------------------------------------------------------------------------
class RenderResult(NamedTuple):
    accum: np.ndarray  # [n_rows, cols, 4] int32: PixelStats {Count; SumRed; SumGreen; SumBlue}
    rgb: np.ndarray    # [n_rows, cols, 3] uint8: PixelStats.mean
    stats: dict


class CameraHits(NamedTuple):
    hit_index: np.ndarray  # [n, n_samples] int32: index into Scene.make's objects, -1 none, -2 where Ray.make' gave ValueNone
    strike: Optional[np.ndarray]  # [n, n_samples, 3] float64, NaN where hit_index < 0; None if not asked for
    rays: Optional[np.ndarray]    # [n, n_samples, 6] float64: the camera ray, origin then unit direction, NaN at -2; None if not asked for
    stats: Optional[dict]


class CameraPaths(NamedTuple):
    """Path records of camera paths, [n, n_samples, ...] in list order (a field not asked for is None)."""
    n_vertices: np.ndarray             # [n, n_samples] int32: vertices the path has (not capped by max_vertices)
    end: np.ndarray                    # [n, n_samples] int32: RT_PATH_MISS 0, STOPPED 1, BOUNCE_LIMIT 2, NO_RAY 3
    colour: np.ndarray                 # [n, n_samples, 3] uint8: Scene.traceRay's result
    first_ray: Optional[np.ndarray]    # [n, n_samples, 6] float64: the camera ray, NaN at NO_RAY
    hit_index: Optional[np.ndarray]    # [n, n_samples, K] int32, -1 past the path's end
    strike: Optional[np.ndarray]       # [n, n_samples, K, 3] float64
    colour_after: Optional[np.ndarray] # [n, n_samples, K, 3] uint8
    ray_after: Optional[np.ndarray]    # [n, n_samples, K, 6] float64, NaN where Reflection gave ValueSome
    summary: Optional[np.ndarray]      # [n, 16] int32 (include/rtfs_amd.h: RT_PATH_SUMMARY_WORDS)
    stats: Optional[dict]


class TracePaths(NamedTuple):
    """Path records of a ray list, [n, ...]; rng is the advanced states (None without rng)."""
    n_vertices: np.ndarray
    end: np.ndarray
    colour: np.ndarray
    rng: Optional[np.ndarray]
    hit_index: Optional[np.ndarray]
    strike: Optional[np.ndarray]
    colour_after: Optional[np.ndarray]
    ray_after: Optional[np.ndarray]
    stats: Optional[dict]


class Scene:
    def __init__(self, handle: int, keep):
        self._h = C.c_void_p(handle)
        self._keep = keep
        self._local = threading.local()

    @property
    def last_stats(self) -> Optional[dict]:
        """The statistics of the calling THREAD's last render_rows / hitObject / traceRays / renderFootprints / renderPixels / cameraHits on this scene (None before its first,
        or after a device call with stats=False).  Per thread, like rt_last_error: a scene may be used from many threads at once."""
        return getattr(self._local, "stats", None)

    @last_stats.setter
    def last_stats(self, value: Optional[dict]) -> None:
        self._local.stats = value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.rt_scene_destroy(h)

    @staticmethod
    def make(objects: Sequence[Hittable], walk_tree: Optional[str] = None) -> "Scene":  # Scene.fs:15-28
        """walk_tree: None = the process default (set_walk_tree), "sah" or "reference" = this scene's own choice (rt_scene_create_ex)."""
        hs, n, tex, ntex, keep = flatten_hittables(objects)
        out = C.c_void_p()
        if walk_tree is None:
            check(lib.rt_scene_create(hs, n, tex, ntex, C.byref(out)))
        else:
            opt = A.rt_scene_options({"sah": A.RT_WALK_TREE_SAH, "reference": A.RT_WALK_TREE_REFERENCE}[walk_tree])
            check(lib.rt_scene_create_ex(hs, n, tex, ntex, C.byref(opt), C.byref(out)))
        return Scene(out.value, keep)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> dict:
        i = A.rt_scene_info()
        check(lib.rt_scene_get_info(self._h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in i._fields_}

    def tree(self):
        n = self.info()["n_nodes"]
        skip = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); boxes = np.zeros((n, 6), np.float64)
        check(lib.rt_scene_get_tree(self._h, _i32(skip), _i32(prim), _f64(boxes)))
        return skip, prim, boxes

    def walk_tree(self):
        """The tree the device image holds (rt_set_walk_tree): same arrays as tree()."""
        n = self.info()["walk_tree_nodes"]
        skip = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); boxes = np.zeros((n, 6), np.float64)
        check(lib.rt_scene_get_walk_tree(self._h, _i32(skip), _i32(prim), _f64(boxes)))
        return skip, prim, boxes

    def filter_tree(self):
        """rt_scene_get_filter_tree: the timed kernel's single-precision records in the device image's (depth) order:
        boxes [n, 6] float32 (lo, hi per axis, rounded outward), links [n, 5] int32 (on hit, on miss, queue entry, shift, hittable)."""
        n = self.info()["walk_tree_nodes"]
        boxes = np.zeros((n, 6), np.float32); links = np.zeros((n, 5), np.int32)
        check(lib.rt_scene_get_filter_tree(self._h, boxes.ctypes.data_as(C.POINTER(C.c_float)), _i32(links)))
        return boxes, links

    def tune(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, *, seed: int = 0, device: int = 0) -> dict:
        """rt_scene_tune: the walk tree rebuilt from the rays of a small probe render with this camera (same pixels, fewer box tests)."""
        info = A.rt_tune_info()
        check(lib.rt_scene_tune(self._h, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_ if n != "struct_size"}

    def tune_rays(self, rays: np.ndarray) -> dict:
        """rt_scene_tune_rays: the host half of tune() with the caller's own probe rays [n, 6] (origin, direction)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        info = A.rt_tune_info()
        check(lib.rt_scene_tune_rays(self._h, _f64(r), r.shape[0], C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_ if n != "struct_size"}

    def render_rows(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, *, seed: int = 0, device: int = 0,
                    row_first: int = 0, row_stride: int = 1, n_rows: Optional[int] = None, counters: bool = False) -> RenderResult:
        """rt_render for the image rows row_first + i*row_stride (the whole frame by default)."""
        rows = 2 * maxHeightCoord + 1
        cols = 2 * maxWidthCoord + 1
        if n_rows is None:
            n_rows = max(0, (rows - row_first + row_stride - 1) // row_stride)
        accum = np.zeros((n_rows, cols, 4), np.int32)
        rgb = np.zeros((n_rows, cols, 3), np.uint8)
        st = A.rt_stats()
        cam = camera.to_abi()
        check(lib.rt_render(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, device, row_first, row_stride, n_rows,
                            A.RT_RENDER_COUNTERS if counters else 0, _i32(accum), _u8(rgb), C.byref(st)))
        self.last_stats = st.as_dict()
        return RenderResult(accum, rgb, self.last_stats)

    def renderPpm(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False) -> dict:
        """rt_render_ppm: Scene.render |> ImageOutput.writePpm in one call -- the frame rendered, formatted as P3 text on the device and
        written to `path`; byte for byte ImageOutput.writePpm of render_rows' rgb.  Returns the statistics (total_ms covers the file)."""
        st = A.rt_stats()
        cam = camera.to_abi()
        check(lib.rt_render_ppm(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, device, A.RT_RENDER_COUNTERS if counters else 0,
                                int(bool(gammaCorrect)), str(path).encode(), None, C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def renderPng(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False) -> dict:
        """rt_render_png: Scene.render |> Png.write (Program.fs:47-50) in one call -- the frame rendered, encoded as a PNG on the device and
        written to `path`; byte for byte Png.format of render_rows' rgb.  Returns the statistics (total_ms covers the file)."""
        st = A.rt_stats()
        cam = camera.to_abi()
        check(lib.rt_render_png(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, device, A.RT_RENDER_COUNTERS if counters else 0,
                                int(bool(gammaCorrect)), str(path).encode(), None, C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def resume(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, data: bytes, *, seed: int = 0, device: int = 0, counters: bool = False,
               options: Optional[A.rt_render_options] = None) -> np.ndarray:
        """rt_resume_pixel_map: Program.fs:45-49 for an interrupted frame -- the pixel map `data` (bytes) parsed on the device, the pixels
        it lacks rendered alone and scattered in -> rgb [rows, cols, 3] uint8.  For a map of render_rows' own records (any order, any
        subset, duplicated or truncated) that is render_rows' rgb byte for byte.  last_stats: pixels = the number rendered."""
        data = bytes(data)
        rgb = np.zeros((2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1, 3), np.uint8)
        st = A.rt_stats()
        cam = camera.to_abi()
        check(lib.rt_resume_pixel_map(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, device, A.RT_RENDER_COUNTERS if counters else 0,
                                      data, len(data), _u8(rgb), _ref(options), C.byref(st)))
        self.last_stats = st.as_dict()
        return rgb

    def resumePng(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, mapPath: str, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False, options: Optional[A.rt_render_options] = None) -> dict:
        """rt_resume_png: Program.fs:45-50 with the missing pixels rendered where ImageOutput.assertComplete would throw -- the spill at
        mapPath resumed on the device, encoded there and written to `path`; byte for byte Png.format of resume()'s rgb."""
        return self._resume_file(lib.rt_resume_png, maxWidthCoord, maxHeightCoord, camera, mapPath, path, gammaCorrect, seed, device, counters, options)

    def resumePpm(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, mapPath: str, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False, options: Optional[A.rt_render_options] = None) -> dict:
        """rt_resume_ppm: resumePng with ImageOutput.writePpm's P3 text."""
        return self._resume_file(lib.rt_resume_ppm, maxWidthCoord, maxHeightCoord, camera, mapPath, path, gammaCorrect, seed, device, counters, options)

    def _resume_file(self, fn, maxWidthCoord, maxHeightCoord, camera, mapPath, path, gammaCorrect, seed, device, counters, options) -> dict:
        st = A.rt_stats()
        cam = camera.to_abi()
        check(fn(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, device, A.RT_RENDER_COUNTERS if counters else 0, str(mapPath).encode(),
                 int(bool(gammaCorrect)), str(path).encode(), _ref(options), C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def extend_rows(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, accum, samplesDone: int, *, seed: int = 0,
                    device: Optional[int] = None, row_first: int = 0, row_stride: int = 1, counters: bool = False, stats: bool = True,
                    options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_extend: continues `accum` -- the PixelStats of the rows row_first + i*row_stride, rendered or last extended with
        samplesDone (>= 12) samples per pixel -- to camera.SamplesPerPixel; the result is, bit for bit, a render at that count.
        Everything but the sample count as in the call that made the buffer.  A numpy array [n_rows, cols, 4] int32 is left as it
        is and a new one returned; a torch tensor on a GPU is extended IN PLACE through rt_render_extend_device on
        torch.cuda.current_stream() (stats=False: no wait for the device; a malformed buffer then goes unreported and unchanged)."""
        cols = 2 * maxWidthCoord + 1
        flags = A.RT_RENDER_COUNTERS if counters else 0
        cam = camera.to_abi()
        if _is_torch(accum):
            torch = _torch()
            if accum.dtype != torch.int32 or accum.dim() != 3 or tuple(accum.shape[1:]) != (cols, 4) or not accum.is_cuda or not accum.is_contiguous():
                raise ValueError(f"accum must be a contiguous int32 tensor [n_rows, {cols}, 4] on a GPU")
            dev = _tensor_device(accum, device)
            n_rows = accum.shape[0]
            rgb = torch.empty((n_rows, cols, 3), dtype=torch.uint8, device=accum.device)
            st = A.rt_stats() if stats else None
            check(lib.rt_render_extend_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, row_first, row_stride, n_rows, flags,
                                              samplesDone, accum.data_ptr(), rgb.data_ptr(), torch.cuda.current_stream(accum.device).cuda_stream,
                                              _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return RenderResult(accum, rgb, self.last_stats)
        _no_options(options)
        if not isinstance(accum, np.ndarray) or accum.dtype != np.int32 or accum.ndim != 3 or accum.shape[1:] != (cols, 4):
            raise ValueError(f"accum must be an int32 array [n_rows, {cols}, 4] or such a tensor on a GPU")
        out = np.array(accum, dtype=np.int32, order="C")
        n_rows = out.shape[0]
        rgb = np.zeros((n_rows, cols, 3), np.uint8)
        st = A.rt_stats()
        check(lib.rt_render_extend(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, row_first, row_stride,
                                   n_rows, flags, samplesDone, _i32(out), _u8(rgb), C.byref(st)))
        self.last_stats = st.as_dict()
        return RenderResult(out, rgb, self.last_stats)

    def extend_rows_map(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, accum, targets, *, seed: int = 0,
                        device: Optional[int] = None, row_first: int = 0, row_stride: int = 1, counters: bool = False, stats: bool = True,
                        options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_extend_map: continues every pixel of `accum` -- the PixelStats of the rows row_first + i*row_stride of a buffer that
        began as a render at >= 12 samples per pixel -- from its own Count to targets[row, col] (int32 [n_rows, cols]); a pixel whose
        target is not above its Count is left as it is, one that stopped early (Count 11) is final.  camera.SamplesPerPixel is the upper
        bound on every target.  Each pixel is then, bit for bit, that pixel of a render at its Count.  Arrays and tensors as for
        extend_rows: an array is copied, a GPU tensor (with `targets` a tensor on the same device) is extended in place on the
        current stream."""
        cols = 2 * maxWidthCoord + 1
        flags = A.RT_RENDER_COUNTERS if counters else 0
        cam = camera.to_abi()
        if _is_torch(accum):
            torch = _torch()
            if accum.dtype != torch.int32 or accum.dim() != 3 or tuple(accum.shape[1:]) != (cols, 4) or not accum.is_cuda or not accum.is_contiguous():
                raise ValueError(f"accum must be a contiguous int32 tensor [n_rows, {cols}, 4] on a GPU")
            n_rows = accum.shape[0]
            if (not _is_torch(targets) or targets.dtype != torch.int32 or tuple(targets.shape) != (n_rows, cols) or targets.device != accum.device
                    or not targets.is_contiguous()):
                raise ValueError(f"targets must be a contiguous int32 tensor [n_rows, {cols}] on accum's device")
            dev = _tensor_device(accum, device)
            rgb = torch.empty((n_rows, cols, 3), dtype=torch.uint8, device=accum.device)
            st = A.rt_stats() if stats else None
            check(lib.rt_render_extend_map_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, row_first, row_stride, n_rows, flags,
                                                  targets.data_ptr(), accum.data_ptr(), rgb.data_ptr(),
                                                  torch.cuda.current_stream(accum.device).cuda_stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return RenderResult(accum, rgb, self.last_stats)
        _no_options(options)
        if not isinstance(accum, np.ndarray) or accum.dtype != np.int32 or accum.ndim != 3 or accum.shape[1:] != (cols, 4):
            raise ValueError(f"accum must be an int32 array [n_rows, {cols}, 4] or such a tensor on a GPU")
        out = np.array(accum, dtype=np.int32, order="C")
        n_rows = out.shape[0]
        if not isinstance(targets, np.ndarray) or targets.dtype != np.int32 or targets.shape != (n_rows, cols):
            raise ValueError(f"targets must be an int32 array [n_rows, {cols}]")
        tg = np.ascontiguousarray(targets)
        rgb = np.zeros((n_rows, cols, 3), np.uint8)
        st = A.rt_stats()
        check(lib.rt_render_extend_map(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, row_first,
                                       row_stride, n_rows, flags, _i32(tg), _i32(out), _u8(rgb), C.byref(st)))
        self.last_stats = st.as_dict()
        return RenderResult(out, rgb, self.last_stats)

    def render_frame(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, *, seed: int = 0, devices: Sequence[int] = (0,),
                     gather: int = A.RT_GATHER_AUTO, counters: bool = False, options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_frame: the whole frame on several GPUs from this one process (rows interleaved over `devices`, one gather);
        stats is a list with one dict per device."""
        rows, cols = 2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1
        accum = np.zeros((rows, cols, 4), np.int32)
        rgb = np.zeros((rows, cols, 3), np.uint8)
        devs = (C.c_int32 * len(devices))(*devices)
        st = (A.rt_stats * len(devices))()
        cam = camera.to_abi()
        check(lib.rt_render_frame(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, devs, len(devices),
                                  A.RT_RENDER_COUNTERS if counters else 0, gather, C.byref(options) if options is not None else None,
                                  _i32(accum), _u8(rgb), st))
        return RenderResult(accum, rgb, [x.as_dict() for x in st])

    def hitObject(self, rays, *, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                  options: Optional[A.rt_render_options] = None):
        """Scene.hitObject (Scene.fs:62-91) for the caller's rays [n, 6] float64 (origin, vector; Ray.make' is applied on the
        device) -> (hit_index int32 [n]: index into Scene.make's objects, -1 none, -2 where Ray.make' fails; strike float64 [n, 3],
        NaN where hit_index < 0).  A numpy array goes through rt_hit_objects; a torch tensor on a GPU through rt_hit_objects_device
        on torch.cuda.current_stream(), and the results are tensors on that device (stats=False: no wait for the device, and
        last_stats is None).  The statistics go to last_stats, which is per thread.  device: the GPU (default 0, or the tensor's)."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        if _is_torch(rays):
            torch = _torch()
            r = _tensor_arg(rays, "rays", (torch.float64,), 6)
            dev = _tensor_device(r, device)
            n = r.shape[0]
            hit = torch.empty(n, dtype=torch.int32, device=r.device)
            strike = torch.empty((n, 3), dtype=torch.float64, device=r.device)
            st = A.rt_stats() if stats else None
            check(lib.rt_hit_objects_device(self._h, dev, n, r.data_ptr(), flags, hit.data_ptr(), strike.data_ptr(),
                                            torch.cuda.current_stream(r.device).cuda_stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return hit, strike
        _no_options(options)
        r = _array_arg(rays, "rays", np.float64, 6)
        n = r.shape[0]
        hit = np.zeros(n, np.int32)
        strike = np.zeros((n, 3), np.float64)
        st = A.rt_stats()
        check(lib.rt_hit_objects(self._h, 0 if device is None else device, n, _f64(r), flags, _i32(hit), _f64(strike), C.byref(st)))
        self.last_stats = st.as_dict()
        return hit, strike

    def traceRays(self, rays, bounceDepth: int, *, rng=None, seed: int = 0, stream_base: int = 0, sample: int = 0,
                  device: Optional[int] = None, counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None):
        """Scene.traceRay (Scene.fs:93-114) from LightRay {Ray.make'(origin, vector); Colour.White} for the caller's rays [n, 6],
        at most bounceDepth+1 hits -> (colour uint8 [n, 3], rng_out).  rng: [n, 4] uint32 xorshift128 states (FloatProducer), which
        are not modified: rng_out holds them advanced.  rng=None: ray i draws from the stream keyed (seed, stream_base + i, sample),
        as a render's (pixel, sample), and rng_out is None.  numpy arrays / torch tensors as for hitObject (a tensor rng may be
        uint32 or int32: the bits are the state)."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        if _is_torch(rays):
            torch = _torch()
            r = _tensor_arg(rays, "rays", (torch.float64,), 6)
            dev = _tensor_device(r, device)
            n = r.shape[0]
            g = None
            if rng is not None:
                if not _is_torch(rng):
                    raise TypeError("rng must be a torch tensor when rays is one")
                g = _tensor_arg(rng, "rng", (torch.uint32, torch.int32), 4).clone()
                if g.shape[0] != n or g.device != r.device:
                    raise ValueError("rng must be [n, 4] on the rays' device")
            colour = torch.empty((n, 3), dtype=torch.uint8, device=r.device)
            st = A.rt_stats() if stats else None
            check(lib.rt_trace_rays_device(self._h, dev, n, r.data_ptr(), g.data_ptr() if g is not None else None, seed, stream_base, sample,
                                           bounceDepth, flags, colour.data_ptr(), torch.cuda.current_stream(r.device).cuda_stream,
                                           _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return colour, g
        _no_options(options)
        r = _array_arg(rays, "rays", np.float64, 6)
        n = r.shape[0]
        g = None
        if rng is not None:
            g = _array_arg(rng, "rng", np.uint32, 4).copy()
            if g.shape[0] != n:
                raise ValueError("rng must be [n, 4] for n rays")
        colour = np.zeros((n, 3), np.uint8)
        st = A.rt_stats()
        check(lib.rt_trace_rays(self._h, 0 if device is None else device, n, _f64(r), _u32(g) if g is not None else None, seed, stream_base,
                                sample, bounceDepth, flags, _u8(colour), C.byref(st)))
        self.last_stats = st.as_dict()
        return colour, g

    def renderFootprints(self, footprints, samplesPerPixel: int, bounceDepth: int, *, seed: int = 0, stream_base: int = 0,
                         device: Optional[int] = None, counters: bool = False, stats: bool = True,
                         options: Optional[A.rt_render_options] = None, extend=None, extend_map=None) -> RenderResult:
        """Scene.renderPixel (Scene.fs:157-194) for caller-defined cameras: footprints [n, 12] float64, per pixel origin, base, du,
        dv.  Sample s of pixel i draws (r1, r2) from the stream keyed (seed, stream_base + i, s) and traces
        Ray.make'(origin, (base + r1*du) + r2*dv) at most bounceDepth+1 hits; the adaptive stop is the reference's, with
        samplesPerPixel -> RenderResult(accum [n, 4] int32, rgb [n, 3] uint8, stats).  numpy arrays / torch tensors as for hitObject:
        a tensor goes through rt_render_footprints_device on torch.cuda.current_stream() and the results are tensors (stats=False: no
        wait for the device, stats and last_stats are None).
        extend=(accum, samplesDone): rt_render_footprints_extend -- `accum` [n, 4] int32, these footprints' PixelStats at samplesDone
        (>= 12) samples, is continued to samplesPerPixel; bit for bit a render at that count.  An array is copied, a tensor (on the
        footprints' device) extended in place.
        extend_map=(accum, targets): rt_render_footprints_extend_map -- every footprint from its own Count to targets[i] (int32 [n]), at
        most samplesPerPixel; the classes and the array / tensor rules of extend_rows_map."""
        if extend is not None and extend_map is not None:
            raise ValueError("extend and extend_map exclude each other")
        flags = A.RT_RENDER_COUNTERS if counters else 0
        if _is_torch(footprints):
            torch = _torch()
            f = _tensor_arg(footprints, "footprints", (torch.float64,), 12)
            dev = _tensor_device(f, device)
            n = f.shape[0]
            rgb = torch.empty((n, 3), dtype=torch.uint8, device=f.device)
            st = A.rt_stats() if stats else None
            stream = torch.cuda.current_stream(f.device).cuda_stream
            if extend is not None:
                accum, done = extend
                _accum_tensor(accum, n, f.device, "extend=(accum, samplesDone)", "the footprints' device")
                check(lib.rt_render_footprints_extend_device(self._h, dev, n, f.data_ptr(), samplesPerPixel, bounceDepth, seed, stream_base, flags,
                                                             done, accum.data_ptr(), rgb.data_ptr(), stream, _ref(options), _ref(st)))
            elif extend_map is not None:
                accum, tg = extend_map
                _accum_tensor(accum, n, f.device, "extend_map=(accum, targets)", "the footprints' device")
                if not _is_torch(tg) or tg.dtype != torch.int32 or tuple(tg.shape) != (n,) or tg.device != f.device or not tg.is_contiguous():
                    raise ValueError("extend_map=(accum, targets): targets must be a contiguous int32 tensor [n] on the footprints' device")
                check(lib.rt_render_footprints_extend_map_device(self._h, dev, n, f.data_ptr(), samplesPerPixel, bounceDepth, seed, stream_base, flags,
                                                                 tg.data_ptr(), accum.data_ptr(), rgb.data_ptr(), stream, _ref(options), _ref(st)))
            else:
                accum = torch.empty((n, 4), dtype=torch.int32, device=f.device)
                check(lib.rt_render_footprints_device(self._h, dev, n, f.data_ptr(), samplesPerPixel, bounceDepth, seed, stream_base, flags,
                                                      accum.data_ptr(), rgb.data_ptr(), stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return RenderResult(accum, rgb, self.last_stats)
        _no_options(options)
        f = _array_arg(footprints, "footprints", np.float64, 12)
        n = f.shape[0]
        rgb = np.zeros((n, 3), np.uint8)
        st = A.rt_stats()
        if extend is not None:
            accum = np.array(_array_arg(extend[0], "extend's accum", np.int32, 4), order="C")
            if accum.shape[0] != n:
                raise ValueError("extend=(accum, samplesDone): accum must be [n, 4] for n footprints")
            check(lib.rt_render_footprints_extend(self._h, 0 if device is None else device, n, _f64(f), samplesPerPixel, bounceDepth, seed,
                                                  stream_base, flags, extend[1], _i32(accum), _u8(rgb), C.byref(st)))
        elif extend_map is not None:
            accum = np.array(_array_arg(extend_map[0], "extend_map's accum", np.int32, 4), order="C")
            tg = extend_map[1]
            if accum.shape[0] != n:
                raise ValueError("extend_map=(accum, targets): accum must be [n, 4] for n footprints")
            if not isinstance(tg, np.ndarray) or tg.dtype != np.int32 or tg.shape != (n,):
                raise ValueError("extend_map=(accum, targets): targets must be an int32 array [n]")
            tg = np.ascontiguousarray(tg)
            check(lib.rt_render_footprints_extend_map(self._h, 0 if device is None else device, n, _f64(f), samplesPerPixel, bounceDepth, seed,
                                                      stream_base, flags, _i32(tg), _i32(accum), _u8(rgb), C.byref(st)))
        else:
            accum = np.zeros((n, 4), np.int32)
            check(lib.rt_render_footprints(self._h, 0 if device is None else device, n, _f64(f), samplesPerPixel, bounceDepth, seed, stream_base,
                                           flags, _i32(accum), _u8(rgb), C.byref(st)))
        self.last_stats = st.as_dict()
        return RenderResult(accum, rgb, self.last_stats)

    def renderPixels(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, pixels, *, seed: int = 0, device: Optional[int] = None,
                     counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None, extend=None) -> RenderResult:
        """Scene.renderPixel (Scene.fs:157-194) for a caller-chosen list of the FRAME's pixels: pixels [n] int32, each a global pixel
        index row * (2*maxWidthCoord+1) + col (row 0 = top) -> RenderResult(accum [n, 4] int32, rgb [n, 3] uint8, stats), in list
        order.  Entry i is, bit for bit, that pixel of render_rows of the whole frame with the same camera, geometry and seed, for any
        order or subset; duplicates are allowed.  numpy arrays / torch tensors as for renderFootprints: a tensor goes through
        rt_render_pixels_device on torch.cuda.current_stream() and the results are tensors (stats=False: no wait for the device, stats
        and last_stats are None; a list with an entry outside the frame then goes unreported and renders nothing).
        extend=(accum, samplesDone): rt_render_pixels_extend -- `accum` [n, 4] int32, this list's PixelStats at samplesDone (>= 12)
        samples, is continued to camera.SamplesPerPixel; bit for bit a list render at that count.  An array is copied, a tensor (on the
        list's device) extended in place."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        cam = camera.to_abi()
        if _is_torch(pixels):
            torch = _torch()
            px = _list_tensor(pixels)
            dev = _tensor_device(px, device)
            n = px.shape[0]
            rgb = torch.empty((n, 3), dtype=torch.uint8, device=px.device)
            st = A.rt_stats() if stats else None
            stream = torch.cuda.current_stream(px.device).cuda_stream
            if extend is not None:
                accum, done = extend
                _accum_tensor(accum, n, px.device, "extend=(accum, samplesDone)", "the list's device")
                check(lib.rt_render_pixels_extend_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, n, px.data_ptr(), flags, done,
                                                         accum.data_ptr(), rgb.data_ptr(), stream, _ref(options), _ref(st)))
            else:
                accum = torch.empty((n, 4), dtype=torch.int32, device=px.device)
                check(lib.rt_render_pixels_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, n, px.data_ptr(), flags,
                                                  accum.data_ptr(), rgb.data_ptr(), stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return RenderResult(accum, rgb, self.last_stats)
        _no_options(options)
        px = _list_array(pixels)
        n = px.shape[0]
        rgb = np.zeros((n, 3), np.uint8)
        st = A.rt_stats()
        if extend is not None:
            accum = np.array(_array_arg(extend[0], "extend's accum", np.int32, 4), order="C")
            if accum.shape[0] != n:
                raise ValueError("extend=(accum, samplesDone): accum must be [n, 4] for n list entries")
            check(lib.rt_render_pixels_extend(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, n, _i32(px),
                                              flags, extend[1], _i32(accum), _u8(rgb), C.byref(st)))
        else:
            accum = np.zeros((n, 4), np.int32)
            check(lib.rt_render_pixels(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, n, _i32(px), flags,
                                       _i32(accum), _u8(rgb), C.byref(st)))
        self.last_stats = st.as_dict()
        return RenderResult(accum, rgb, self.last_stats)

    def cameraHits(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, pixels=None, *, sample_first: int = 0, n_samples: int = 1,
                   seed: int = 0, n: Optional[int] = None, strike: bool = True, rays: bool = True, tensors: bool = False, device: Optional[int] = None,
                   counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None) -> CameraHits:
        """What each pixel sample's camera ray strikes first: Scene.hitObject (Scene.fs:62-91) of the ray Scene.traceOnce
        (Scene.fs:129-143) builds for samples sample_first .. sample_first + n_samples - 1 of the FRAME's pixels in `pixels` ([n] int32
        global pixel indices row * (2*maxWidthCoord+1) + col, as for renderPixels; None: pixels 0 .. n-1, n defaulting to the whole
        frame) -> CameraHits(hit_index [n, n_samples], strike [n, n_samples, 3], rays [n, n_samples, 6], stats), in list order.  It is the
        very ray that sample starts with in render_rows and renderPixels with the same camera, geometry and seed; duplicates are
        allowed.  strike=False / rays=False: that output is not computed (None).  numpy arrays / torch tensors as for renderPixels: a
        tensor goes through rt_camera_hits_device on torch.cuda.current_stream() and the results are tensors (stats=False: no wait for
        the device; a list with an entry outside the frame then goes unreported and nothing is written); with pixels=None,
        tensors=True does the same on `device` (default: torch's current one)."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        cam = camera.to_abi()
        frame = (2 * maxWidthCoord + 1) * (2 * maxHeightCoord + 1)
        if not isinstance(n_samples, int) or not isinstance(sample_first, int):
            raise TypeError("sample_first and n_samples must be ints")
        if pixels is not None and n is not None:
            raise ValueError("n applies to pixels=None")
        if _is_torch(pixels) or (pixels is None and tensors):
            torch = _torch()
            if pixels is None:
                tdev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
                dev, count, ptr = tdev.index, frame if n is None else int(n), None
            else:
                px = _list_tensor(pixels)
                tdev, dev, count, ptr = px.device, _tensor_device(px, device), px.shape[0], px.data_ptr()
            per = max(n_samples, 0)
            hit = torch.empty((count, per), dtype=torch.int32, device=tdev)
            sk = torch.empty((count, per, 3), dtype=torch.float64, device=tdev) if strike else None
            ry = torch.empty((count, per, 6), dtype=torch.float64, device=tdev) if rays else None
            st = A.rt_stats() if stats else None
            check(lib.rt_camera_hits_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, count, ptr, sample_first, n_samples, flags,
                                            hit.data_ptr(), sk.data_ptr() if strike else None, ry.data_ptr() if rays else None,
                                            torch.cuda.current_stream(tdev).cuda_stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return CameraHits(hit, sk, ry, self.last_stats)
        _no_options(options, "set_launch_config")
        if pixels is None:
            px, count = None, frame if n is None else int(n)
        else:
            px = _list_array(pixels)
            count = px.shape[0]
        if count < 0:
            raise ValueError("n must be >= 0")
        per = max(n_samples, 0)
        big = count * per > 2**31 - 1  # (refused by the library: no buffers are made for it)
        shape = (0, 0) if big else (count, per)
        hit = np.zeros(shape, np.int32)
        sk = np.zeros(shape + (3,), np.float64) if strike else None
        ry = np.zeros(shape + (6,), np.float64) if rays else None
        st = A.rt_stats()
        check(lib.rt_camera_hits(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, count,
                                 _i32(px) if px is not None else None, sample_first, n_samples, flags, _i32(hit), _f64(sk) if strike else None,
                                 _f64(ry) if rays else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return CameraHits(hit, sk, ry, self.last_stats)

    @staticmethod
    def _path_buffers(lead, k, records, make, first_ray=False, summary_entries=None):
        """The output buffers of a path call, shaped lead + (...): make(shape, kind) allocates, kind one of "i32", "u8", "f64"."""
        bufs = {"n_vertices": make(lead, "i32"), "end": make(lead, "i32"), "colour": make(lead + (3,), "u8")}
        bufs["first_ray"] = make(lead + (6,), "f64") if first_ray else None
        rec = records and k > 0
        bufs["hit_index"] = make(lead + (k,), "i32") if rec else None
        bufs["strike"] = make(lead + (k, 3), "f64") if rec else None
        bufs["colour_after"] = make(lead + (k, 3), "u8") if rec else None
        bufs["ray_after"] = make(lead + (k, 6), "f64") if rec else None
        bufs["summary"] = make((summary_entries, A.RT_PATH_SUMMARY_WORDS), "i32") if summary_entries is not None else None
        return bufs

    def cameraPaths(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, pixels=None, *, sample_first: int = 0, n_samples: int = 1,
                    max_vertices: int = 8, records: bool = True, first_ray: bool = True, summary: bool = False, seed: int = 0,
                    n: Optional[int] = None, tensors: bool = False, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                    options: Optional[A.rt_render_options] = None) -> CameraPaths:
        """The path behind every sample: Scene.traceRay (Scene.fs:93-114) of the ray Scene.traceOnce builds for samples sample_first ..
        sample_first + n_samples - 1 of the FRAME's pixels in `pixels` (as cameraHits: [n] int32 global pixel indices; None: pixels
        0 .. n-1), with the sample's own generator -- the very path that sample follows in render_rows and renderPixels -> CameraPaths.
        max_vertices (K): records kept per path; n_vertices counts them all.  records=False / first_ray=False: not computed (None);
        summary=True adds the per-entry reduction [n, 16].  numpy arrays / torch tensors as for cameraHits (a tensor list, or
        pixels=None with tensors=True, goes through rt_camera_paths_device on torch.cuda.current_stream())."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        cam = camera.to_abi()
        frame = (2 * maxWidthCoord + 1) * (2 * maxHeightCoord + 1)
        if not isinstance(n_samples, int) or not isinstance(sample_first, int) or not isinstance(max_vertices, int):
            raise TypeError("sample_first, n_samples and max_vertices must be ints")
        if pixels is not None and n is not None:
            raise ValueError("n applies to pixels=None")
        per, k = max(n_samples, 0), max(max_vertices, 0)
        if _is_torch(pixels) or (pixels is None and tensors):
            torch = _torch()
            if pixels is None:
                tdev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
                dev, count, ptr = tdev.index, frame if n is None else int(n), None
            else:
                px = _list_tensor(pixels)
                tdev, dev, count, ptr = px.device, _tensor_device(px, device), px.shape[0], px.data_ptr()
            kinds = {"i32": torch.int32, "u8": torch.uint8, "f64": torch.float64}
            bufs = Scene._path_buffers((count, per), k, records, lambda shape, kind: torch.empty(shape, dtype=kinds[kind], device=tdev), first_ray,
                                       count if summary else None)
            out = A.rt_path_outputs(max_vertices=max_vertices, **{f: (b.data_ptr() if b is not None else None) for f, b in bufs.items()})
            st = A.rt_stats() if stats else None
            check(lib.rt_camera_paths_device(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, dev, count, ptr, sample_first, n_samples, flags,
                                             C.byref(out), torch.cuda.current_stream(tdev).cuda_stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
            return CameraPaths(stats=self.last_stats, **bufs)
        _no_options(options, "set_launch_config")
        if pixels is None:
            px, count = None, frame if n is None else int(n)
        else:
            px = _list_array(pixels)
            count = px.shape[0]
        if count < 0:
            raise ValueError("n must be >= 0")
        big = count * per * max(k, 1) > 2**31 - 1  # (refused by the library: no buffers are made for it)
        kinds = {"i32": np.int32, "u8": np.uint8, "f64": np.float64}
        bufs = Scene._path_buffers((0, 0) if big else (count, per), k, records, lambda shape, kind: np.zeros(shape, kinds[kind]), first_ray,
                                   (0 if big else count) if summary else None)
        out = A.rt_path_outputs(max_vertices=max_vertices, **{f: (b.ctypes.data if b is not None else None) for f, b in bufs.items()})
        st = A.rt_stats()
        check(lib.rt_camera_paths(self._h, C.byref(cam), maxWidthCoord, maxHeightCoord, seed, 0 if device is None else device, count,
                                  _i32(px) if px is not None else None, sample_first, n_samples, flags, C.byref(out), C.byref(st)))
        self.last_stats = st.as_dict()
        return CameraPaths(stats=self.last_stats, **bufs)

    def tracePaths(self, rays, bounceDepth: int, *, rng=None, seed: int = 0, stream_base: int = 0, sample: int = 0, max_vertices: int = 8,
                   records: bool = True, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                   options: Optional[A.rt_render_options] = None) -> TracePaths:
        """traceRays with the path written down: rays, rng, seed, stream_base, sample and bounceDepth are traceRays' (colour and the
        advanced states equal its) -> TracePaths.  numpy arrays / torch tensors as for traceRays."""
        flags = A.RT_RENDER_COUNTERS if counters else 0
        if not isinstance(max_vertices, int):
            raise TypeError("max_vertices must be an int")
        k = max(max_vertices, 0)
        if _is_torch(rays):
            torch = _torch()
            r = _tensor_arg(rays, "rays", (torch.float64,), 6)
            dev = _tensor_device(r, device)
            n = r.shape[0]
            g = None
            if rng is not None:
                if not _is_torch(rng):
                    raise TypeError("rng must be a torch tensor when rays is one")
                g = _tensor_arg(rng, "rng", (torch.uint32, torch.int32), 4).clone()
                if g.shape[0] != n or g.device != r.device:
                    raise ValueError("rng must be [n, 4] on the rays' device")
            kinds = {"i32": torch.int32, "u8": torch.uint8, "f64": torch.float64}
            bufs = Scene._path_buffers((n,), k, records, lambda shape, kind: torch.empty(shape, dtype=kinds[kind], device=r.device))
            out = A.rt_path_outputs(max_vertices=max_vertices, **{f: (b.data_ptr() if b is not None else None) for f, b in bufs.items()})
            st = A.rt_stats() if stats else None
            check(lib.rt_trace_paths_device(self._h, dev, n, r.data_ptr(), g.data_ptr() if g is not None else None, seed, stream_base, sample,
                                            bounceDepth, flags, C.byref(out), torch.cuda.current_stream(r.device).cuda_stream, _ref(options), _ref(st)))
            self.last_stats = st.as_dict() if st is not None else None
        else:
            _no_options(options)
            r = _array_arg(rays, "rays", np.float64, 6)
            n = r.shape[0]
            g = None
            if rng is not None:
                g = _array_arg(rng, "rng", np.uint32, 4).copy()
                if g.shape[0] != n:
                    raise ValueError("rng must be [n, 4] for n rays")
            big = n * max(k, 1) > 2**31 - 1
            kinds = {"i32": np.int32, "u8": np.uint8, "f64": np.float64}
            bufs = Scene._path_buffers((0,) if big else (n,), k, records, lambda shape, kind: np.zeros(shape, kinds[kind]))
            out = A.rt_path_outputs(max_vertices=max_vertices, **{f: (b.ctypes.data if b is not None else None) for f, b in bufs.items()})
            st = A.rt_stats()
            check(lib.rt_trace_paths(self._h, 0 if device is None else device, n, _f64(r), _u32(g) if g is not None else None, seed, stream_base,
                                     sample, bounceDepth, flags, C.byref(out), C.byref(st)))
            self.last_stats = st.as_dict()
        return TracePaths(bufs["n_vertices"], bufs["end"], bufs["colour"], g, bufs["hit_index"], bufs["strike"], bufs["colour_after"], bufs["ray_after"],
                          self.last_stats)

    @staticmethod
    def render(progressIncrement: Callable[[float], None], log: Callable[[str], None], maxWidthCoord: int, maxHeightCoord: int,
               camera: Camera, s: "Scene", *, seed: int = 0, device: int = 0, row_block: Optional[int] = None) -> Tuple[float, Image]:
        """Scene.render (Scene.fs:196-236): returns (rows as progress units, lazy Image).  The work happens when the
        Image is forced, exactly as in the reference, and `progressIncrement 1.0` is called once per row (Scene.fs:232) -- after
        each block of `row_block` rows has come back (row_first/n_rows of the ABI), or after the whole frame when row_block is
        None (one launch: fastest; at 0.2 s per frame the bar just jumps)."""
        rowsIter = 2 * maxHeightCoord + 1
        colsIter = 2 * maxWidthCoord + 1

        def force() -> np.ndarray:
            block = rowsIter if not row_block else max(1, int(row_block))
            out = np.zeros((rowsIter, colsIter, 3), np.uint8)
            for first in range(0, rowsIter, block):
                n = min(block, rowsIter - first)
                out[first:first + n] = s.render_rows(maxWidthCoord, maxHeightCoord, camera, seed=seed, device=device, row_first=first,
                                                     row_stride=1, n_rows=n).rgb
                for _ in range(n):
                    progressIncrement(1.0)
            return out

        return float(rowsIter), Image(rowsIter, colsIter, force)


# ---- ImageOutput.fs -------------------------------------------------------------------------------------------------
class PixelOutput:
    @staticmethod
    def correct(b: int) -> int:  # ImageOutput.fs:11-18
        return int(lib.rt_gamma_correct(int(b)))

    @staticmethod
    def correctImage(pixels):
        """PixelOutput.correct over every byte of `pixels` (uint8, any shape); a new array.  A torch tensor on a GPU goes through
        rt_gamma_correct_device on torch.cuda.current_stream() (no wait for the device), a numpy array through a table of rt_gamma_correct."""
        if _is_torch(pixels):
            t = _bytes_tensor(pixels)
            out = _torch().empty_like(t)
            check(lib.rt_gamma_correct_device(t.device.index, t.numel(), t.data_ptr(), out.data_ptr(), _torch().cuda.current_stream(t.device).cuda_stream))
            return out
        lut = np.array([lib.rt_gamma_correct(b) for b in range(256)], np.uint8)
        return lut[np.ascontiguousarray(pixels, dtype=np.uint8)]


class ImageOutput:
    @staticmethod
    def formatPpm(gammaCorrect: bool, pixels) -> bytes:
        """ImageOutput.writePpm's bytes.  A numpy array takes rt_format_ppm on the host; a contiguous uint8 torch tensor [rows, cols, 3] on a
        GPU is formatted there (formatPpmDevice) and only the text is copied back."""
        if _is_torch(pixels):
            text, length = ImageOutput.formatPpmDevice(gammaCorrect, pixels)
            return text[: int(length)].cpu().numpy().tobytes()
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        rows, cols = px.shape[0], px.shape[1]
        n = lib.rt_format_ppm(_u8(px), rows, cols, int(bool(gammaCorrect)), None, 0)
        if n < 0:
            check(int(-n))
        buf = C.create_string_buffer(int(n) + 1)
        lib.rt_format_ppm(_u8(px), rows, cols, int(bool(gammaCorrect)), buf, int(n) + 1)
        return buf.raw[: int(n)]

    @staticmethod
    def formatPpmDevice(gammaCorrect: bool, pixels):
        """rt_format_ppm_device on torch.cuda.current_stream(), without waiting for the device: (text, length) -- a uint8 tensor of
        rt_ppm_max_bytes(rows, cols) bytes whose first `length` (an int64 tensor) are ImageOutput.writePpm's; the rest is not written."""
        t = _image_tensor(pixels)
        torch = _torch()
        rows, cols = int(t.shape[0]), int(t.shape[1])
        cap = lib.rt_ppm_max_bytes(rows, cols)
        if cap < 0:
            check(int(-cap))
        text = torch.empty(int(cap), dtype=torch.uint8, device=t.device)
        length = torch.empty((), dtype=torch.int64, device=t.device)
        check(lib.rt_format_ppm_device(t.device.index, t.data_ptr(), rows, cols, int(bool(gammaCorrect)), text.data_ptr(), int(cap), length.data_ptr(),
                                       torch.cuda.current_stream(t.device).cuda_stream, None))
        return text, length

    @staticmethod
    def formatPixelMap(pixels) -> bytes:
        """The pixel-map bytes of ImageOutput.resume / toPpm (ImageOutput.fs:115-161): per pixel `<row>,<col>\n` (0 as NO digits) and the
        three raw colour bytes.  numpy: rt_format_pixel_map on the host; a torch tensor on a GPU: rt_format_pixel_map_device."""
        if _is_torch(pixels):
            t = _image_tensor(pixels)
            torch = _torch()
            rows, cols = int(t.shape[0]), int(t.shape[1])
            cap = lib.rt_pixel_map_bytes(rows, cols)
            if cap < 0:
                check(int(-cap))
            out = torch.empty(int(cap), dtype=torch.uint8, device=t.device)
            n = C.c_int64(0)
            check(lib.rt_format_pixel_map_device(t.device.index, t.data_ptr(), rows, cols, out.data_ptr(), int(cap), None,
                                                 torch.cuda.current_stream(t.device).cuda_stream, C.byref(n)))
            return out[: n.value].cpu().numpy().tobytes()
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        n = lib.rt_format_pixel_map(_u8(px), px.shape[0], px.shape[1], None, 0)
        if n < 0:
            check(int(-n))
        buf = C.create_string_buffer(int(n))
        lib.rt_format_pixel_map(_u8(px), px.shape[0], px.shape[1], buf, int(n))
        return buf.raw[: int(n)]

    @staticmethod
    def toPpm(progressIncrement: Callable[[float], None], image: "Image", path: str) -> str:
        """ImageOutput.toPpm = resume (ImageOutput.fs:131-161, 205): force the image and spill it as `<row>,<col>\\nRGB` records."""
        px = np.ascontiguousarray(Image.render(image), dtype=np.uint8)
        n = lib.rt_format_pixel_map(_u8(px), px.shape[0], px.shape[1], None, 0)
        if n < 0:
            check(int(-n))
        buf = C.create_string_buffer(int(n))
        lib.rt_format_pixel_map(_u8(px), px.shape[0], px.shape[1], buf, int(n))
        with open(path, "wb") as f:
            f.write(buf.raw[: int(n)])
        for _ in range(px.shape[0]):
            progressIncrement(1.0)
        return path

    @staticmethod
    def readPixelMap(path: str, numRows: int, numCols: int):
        """ImageOutput.readPixelMap (ImageOutput.fs:68-113) -> (pixels [rows, cols, 3] uint8, present [rows, cols] bool)."""
        data = open(path, "rb").read()
        rgb = np.zeros((numRows, numCols, 3), np.uint8)
        present = np.zeros((numRows, numCols), np.uint8)
        n = lib.rt_parse_pixel_map(data, len(data), numRows, numCols, _u8(rgb), _u8(present))
        if n < 0:
            check(int(-n))
        return rgb, present.astype(bool)

    @staticmethod
    def parsePixelMap(data, numRows: int, numCols: int):
        """rt_parse_pixel_map_device: ImageOutput.readPixelMap (ImageOutput.fs:46-113) of map bytes that are on a GPU -- `data` a uint8 torch
        tensor [n] there -> (pixels [rows, cols, 3] uint8, present [rows, cols] bool), tensors on that GPU, on torch.cuda.current_stream().
        Pixels the map does not name are 0.  Waits for the device; a map naming a pixel outside the image raises RtError."""
        torch = _torch()
        t = _bytes_tensor(data).reshape(-1)
        rgb = torch.zeros((numRows, numCols, 3), dtype=torch.uint8, device=t.device)
        present = torch.empty((numRows, numCols), dtype=torch.uint8, device=t.device)
        n = C.c_int64(0)
        check(lib.rt_parse_pixel_map_device(t.device.index, t.data_ptr() if t.numel() else None, t.numel(), numRows, numCols, rgb.data_ptr(), present.data_ptr(),
                                            None, torch.cuda.current_stream(t.device).cuda_stream, C.byref(n)))
        return rgb, present.bool()

    @staticmethod
    def missingPixels(present):
        """rt_missing_pixels_device: the global pixel indices row * cols + col of the pixels a presence map [rows, cols] (bool or uint8 tensor
        on a GPU) lacks, ascending, as an int32 tensor there -- what Scene.renderPixels takes.  Waits for the device."""
        torch = _torch()
        if present.dim() != 2:
            raise ValueError(f"present must have shape [rows, cols], not {list(present.shape)}")
        t = _bytes_tensor(present.to(torch.uint8) if present.dtype == torch.bool else present)
        rows, cols = int(t.shape[0]), int(t.shape[1])
        stream = torch.cuda.current_stream(t.device).cuda_stream
        n = C.c_int64(0)
        check(lib.rt_missing_pixels_device(t.device.index, t.data_ptr(), rows, cols, None, 0, None, stream, C.byref(n)))
        pixels = torch.empty(n.value, dtype=torch.int32, device=t.device)
        if n.value:
            check(lib.rt_missing_pixels_device(t.device.index, t.data_ptr(), rows, cols, pixels.data_ptr(), n.value, None, stream, C.byref(n)))
        return pixels

    @staticmethod
    def assertComplete(pixel_map) -> np.ndarray:
        """ImageOutput.assertComplete (ImageOutput.fs:199-200): ValueOption.get on every pixel."""
        rgb, present = pixel_map
        if not present.all():
            raise ValueError("ValueOption.get: the pixel map is incomplete")
        return rgb

    @staticmethod
    def writePpm(gammaCorrect: bool, incrementProgress: Callable[[float], None], pixels, output: str) -> None:
        """ImageOutput.writePpm (ImageOutput.fs:163-197).  A torch tensor on a GPU is formatted there (rt_write_ppm_device, on
        torch.cuda.current_stream()); a numpy array takes rt_write_ppm."""
        if _is_torch(pixels):
            t = _image_tensor(pixels)
            check(lib.rt_write_ppm_device(str(output).encode(), t.device.index, t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(bool(gammaCorrect)),
                                          _torch().cuda.current_stream(t.device).cuda_stream))
            for _ in range(int(t.shape[0]) * int(t.shape[1])):
                incrementProgress(1.0)
            return
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        check(lib.rt_write_ppm(str(output).encode(), _u8(px), px.shape[0], px.shape[1], int(bool(gammaCorrect))))
        for _ in range(px.shape[0] * px.shape[1]):
            incrementProgress(1.0)


class Png:
    """Png.write (ImageOutput.fs:214-251).  The reference's file comes out of Skia's encoder; here the PIXELS are the reference's
    (PixelOutput.toSkia, ImageOutput.fs:32-39: R, G, B after PixelOutput.correct or as they are, alpha 255 -- written as 8-bit RGB without an
    alpha channel, which a decoder reports as opaque) and the container bytes are this library's own (csrc/rt_png.h)."""

    @staticmethod
    def format(gammaCorrect: bool, pixels) -> bytes:
        """The file's bytes.  A numpy array takes rt_format_png on the host; a contiguous uint8 torch tensor [rows, cols, 3] on a GPU is
        encoded there (formatDevice) and only the file is copied back."""
        if _is_torch(pixels):
            data, length = Png.formatDevice(gammaCorrect, pixels)
            return data[: int(length)].cpu().numpy().tobytes()
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        rows, cols = px.shape[0], px.shape[1]
        cap = lib.rt_png_max_bytes(rows, cols)
        if cap < 0:
            check(int(-cap))
        buf = np.empty(int(cap), np.uint8)
        n = lib.rt_format_png(_u8(px), rows, cols, int(bool(gammaCorrect)), buf.ctypes.data, int(cap))
        if n < 0:
            check(int(-n))
        return buf[: int(n)].tobytes()

    @staticmethod
    def formatDevice(gammaCorrect: bool, pixels):
        """rt_format_png_device on torch.cuda.current_stream(), without waiting for the device: (data, length) -- a uint8 tensor of
        rt_png_max_bytes(rows, cols) bytes whose first `length` (an int64 tensor) are the file; the rest is not written."""
        t = _image_tensor(pixels)
        torch = _torch()
        rows, cols = int(t.shape[0]), int(t.shape[1])
        cap = lib.rt_png_max_bytes(rows, cols)
        if cap < 0:
            check(int(-cap))
        data = torch.empty(int(cap), dtype=torch.uint8, device=t.device)
        length = torch.empty((), dtype=torch.int64, device=t.device)
        check(lib.rt_format_png_device(t.device.index, t.data_ptr(), rows, cols, int(bool(gammaCorrect)), data.data_ptr(), int(cap), length.data_ptr(),
                                       torch.cuda.current_stream(t.device).cuda_stream, None))
        return data, length

    @staticmethod
    def write(gammaCorrect: bool, incrementProgress: Callable[[float], None], pixels, output: str) -> None:
        """Png.write (ImageOutput.fs:216-251).  A torch tensor on a GPU is encoded there (rt_write_png_device, on
        torch.cuda.current_stream()); a numpy array takes rt_write_png.  Progress as the reference counts it: once per pixel but a row's
        last (ImageOutput.fs:230-233), once per row but the last (:239-241) -- rows * cols - 1 in all."""
        if _is_torch(pixels):
            t = _image_tensor(pixels)
            rows, cols = int(t.shape[0]), int(t.shape[1])
            check(lib.rt_write_png_device(str(output).encode(), t.device.index, t.data_ptr(), rows, cols, int(bool(gammaCorrect)),
                                          _torch().cuda.current_stream(t.device).cuda_stream))
        else:
            px = np.ascontiguousarray(pixels, dtype=np.uint8)
            rows, cols = px.shape[0], px.shape[1]
            check(lib.rt_write_png(str(output).encode(), _u8(px), rows, cols, int(bool(gammaCorrect))))
        for _ in range(rows * cols - 1):
            incrementProgress(1.0)


def _f64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _u8(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _u32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _u64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


# ---- argument checks of the ray-list calls (Scene.hitObject / Scene.traceRays) ----------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _torch():
    import torch
    return torch


def _array_arg(a, name: str, dtype, width: int) -> np.ndarray:
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{name} must be a numpy array or a torch tensor on a GPU, not {type(a).__name__}")
    if a.dtype != dtype:
        raise TypeError(f"{name} must have dtype {np.dtype(dtype).name}, not {a.dtype}")
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{name} must have shape [n, {width}], not {list(a.shape)}")
    return np.ascontiguousarray(a)


def _tensor_arg(t, name: str, dtypes, width: int):
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must have dtype {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name} must have shape [n, {width}], not {list(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a GPU (a numpy array takes the host entry point)")
    return t.contiguous()


def _bytes_tensor(t):
    """Bytes on a GPU, any shape (PixelOutput.correctImage)."""
    if t.dtype != _torch().uint8:
        raise TypeError(f"pixels must have dtype torch.uint8, not {t.dtype}")
    if not t.is_cuda:
        raise ValueError("pixels must be on a GPU (a numpy array takes the host route)")
    return t.contiguous()


def _image_tensor(t):
    """An image [rows, cols, 3] uint8 for the device output entry points."""
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"pixels must have shape [rows, cols, 3], not {list(t.shape)}")
    return _bytes_tensor(t)


def _list_array(a) -> np.ndarray:
    """A pixel list [n] int32 for the host entry points."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"pixels must be a numpy array or a torch tensor on a GPU, not {type(a).__name__}")
    if a.dtype != np.int32:
        raise TypeError(f"pixels must have dtype int32, not {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"pixels must have shape [n], not {list(a.shape)}")
    return np.ascontiguousarray(a)


def _list_tensor(t):
    """A pixel list [n] int32 for the device entry points."""
    if t.dtype != _torch().int32:
        raise TypeError(f"pixels must have dtype torch.int32, not {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"pixels must have shape [n], not {list(t.shape)}")
    if not t.is_cuda:
        raise ValueError("pixels must be on a GPU (a numpy array takes the host entry point)")
    return t.contiguous()


def _accum_tensor(accum, n: int, device, what: str, where: str) -> None:
    """The buffer an extension of n list entries continues in place: `what` names the argument, `where` the device it must be on."""
    if not _is_torch(accum) or accum.dtype != _torch().int32 or tuple(accum.shape) != (n, 4) or accum.device != device or not accum.is_contiguous():
        raise ValueError(f"{what}: accum must be a contiguous int32 tensor [n, 4] on {where}")


def _no_options(options, instead: str = "set_launch_config / set_park") -> None:
    if options is not None:
        raise ValueError(f"options apply to the device entry point (torch tensors); use {instead} for arrays")


def _tensor_device(t, device: Optional[int]) -> int:
    if device is not None and device != t.device.index:
        raise ValueError(f"device={device} but the tensors are on {t.device}")
    return t.device.index


def _ref(x):
    return C.byref(x) if x is not None else None
