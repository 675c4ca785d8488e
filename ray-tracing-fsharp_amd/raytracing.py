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
from . import texprog
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
    bitmap: object = None          # ofImageDevice: a torch uint8 [H, W, 3] tensor on a GPU, rows top first (the device reverses them)
    jpeg: Optional[bytes] = None   # ofJpeg: a baseline JPEG file's bytes (decoded on the device, rows reversed there)
    size: Tuple[int, int] = (0, 0)  # (height, width) of a bitmap / jpeg image
    program: Optional[bytes] = None  # Program: the bytes of csrc/rt_texprog.h (texprog.compile_program)


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
        """ParameterisedTexture.ofImage (Texture.fs:30-48): rows are reversed (y = Height - y - 1).  A bitmap that LoadImage left on a GPU
        comes back to the host here: rt_texture.texels is a host pointer."""
        if _is_torch(bitmap_rows_top_first):
            bitmap_rows_top_first = bitmap_rows_top_first.cpu().numpy()
        return ParameterisedTexture.Image(np.ascontiguousarray(bitmap_rows_top_first[::-1]))

    @staticmethod
    def ofImageDevice(bitmap) -> _ParamTex:
        """ofImage for a bitmap that is in device memory: a torch uint8 tensor [height, width, 3] on a GPU, rows top first as LoadImage
        leaves them.  It is made contiguous on its device and kept; the rows are reversed on the GPU when the scene is made (Scene.make ->
        rt_scene_create_textures), so the texels never visit the host."""
        if not _is_torch(bitmap):
            raise TypeError(f"bitmap must be a torch tensor on a GPU, not {type(bitmap).__name__} (ofImage takes numpy arrays)")
        if bitmap.dtype != _torch().uint8:
            raise TypeError(f"bitmap must have dtype torch.uint8, not {bitmap.dtype}")
        if bitmap.ndim != 3 or bitmap.shape[2] != 3 or bitmap.shape[0] < 1 or bitmap.shape[1] < 1:
            raise ValueError(f"bitmap must have shape [height, width, 3], not {list(bitmap.shape)}")
        if not bitmap.is_cuda:
            raise ValueError("bitmap must be on a GPU (ofImage takes a bitmap in host memory)")
        return _ParamTex(A.RT_TEXTURE_IMAGE, bitmap=bitmap.contiguous(), size=(int(bitmap.shape[0]), int(bitmap.shape[1])))

    @staticmethod
    def ofJpeg(data: bytes) -> _ParamTex:
        """ofImage (LoadImage.fromBytes data) without the bitmap ever being in host memory: the file is decoded on the GPU when the scene is
        made.  The header is read here (rt_jpeg_get_info), so a file LoadImage refuses is refused here, with the same text."""
        data = bytes(data)
        info = LoadImage.info(data)
        return _ParamTex(A.RT_TEXTURE_IMAGE, jpeg=data, size=(int(info["height"]), int(info["width"])))

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
    def Program(red, green, blue) -> _ParamTex:
        """`ParameterisedTexture.Arbitrary (fun x y -> Texture.Arbitrary (fun p -> pixel))` as three expressions (texprog: U, V, PX, PY,
        PZ, numbers, operators, sin, floor, sqrt, abs, minimum, maximum, lt, le, flt, select), one per channel; each value becomes a byte
        as F#'s `byte` does.  Compiled here and checked by the library (rt_texture_program_check); evaluated on the GPU."""
        return _ParamTex(A.RT_TEXTURE_PROGRAM, program=texprog.compile_program(red, green, blue))

    @staticmethod
    def Arbitrary(f: Callable) -> _ParamTex:
        """`f` is called once with the symbolic U and V.  A (red, green, blue) triple of expressions, a Texture.Program or a
        Texture.Colour is lowered to a record; a closure that gives anything else cannot cross the C ABI."""
        try:
            got = f(texprog.U, texprog.V)
            if isinstance(got, Texture) and got.pixel is not None:
                return ParameterisedTexture.Colour(got.pixel)
            if isinstance(got, Texture) and got.param is not None and got.param.kind == A.RT_TEXTURE_PROGRAM:
                return got.param
            if isinstance(got, (tuple, list)) and not isinstance(got, Pixel) and len(got) == 3:
                return ParameterisedTexture.Program(*got)
        except texprog.NotAnExpression:  # (only the language's own refusals: any other error of the closure is the caller's to see)
            pass
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

    @staticmethod
    def Program(red, green, blue) -> "Texture":
        """`Texture.Arbitrary (fun p -> pixel)`: three expressions over the strike point (texprog.PX, PY, PZ); there is no (u, v) map,
        so U and V are those of the unit sphere at the origin."""
        return Texture(param=ParameterisedTexture.Program(red, green, blue))


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
    """-> (rt_hittable array, count, rt_texture array, count, keepalive list).  Textures made by ofImageDevice / ofJpeg need the sources
    that hittable_records(objects, textures=True) returns with them."""
    return _flatten(objects)[:5]


def _flatten(objects: Sequence[Hittable]):
    """flatten_hittables' five, then the rt_texels_source array (None when every image's texels are host arrays) and {id(texture): index of
    its first record, the texture)}."""
    texs: List[A.rt_texture] = []
    keep: list = []
    srcs: List[A.rt_texels_source] = []
    index: dict = {}

    def add_param(t: _ParamTex) -> int:
        r = A.rt_texture()
        r.kind = t.kind
        r.even = r.odd = -1
        r.map_radius = 1.0
        src = A.rt_texels_source()
        if t.kind == A.RT_TEXTURE_CHECKERED:
            e, o = add_param(t.even), add_param(t.odd)  # children first: indices smaller than the parent's
            r.even, r.odd, r.grid_size = e, o, t.grid
        elif t.kind == A.RT_TEXTURE_IMAGE and t.bitmap is not None:
            keep.append(t.bitmap)
            r.height, r.width = t.size
            src = A.rt_texels_source(A.RT_TEXELS_DEVICE, A.RT_TEXELS_TOP_FIRST, t.bitmap.data_ptr(), t.bitmap.numel())
        elif t.kind == A.RT_TEXTURE_IMAGE and t.jpeg is not None:
            keep.append(t.jpeg)
            r.height, r.width = t.size
            src = A.rt_texels_source(A.RT_TEXELS_JPEG, A.RT_TEXELS_TOP_FIRST, C.cast(C.c_char_p(t.jpeg), C.c_void_p), len(t.jpeg))
        elif t.kind == A.RT_TEXTURE_IMAGE:
            keep.append(t.image)
            r.height, r.width = int(t.image.shape[0]), int(t.image.shape[1])
            r.texels = t.image.ctypes.data
        elif t.kind == A.RT_TEXTURE_UV_RAMP:
            r.ramp_src[:] = t.ramp
        elif t.kind == A.RT_TEXTURE_PROGRAM:
            buf = np.frombuffer(t.program, dtype=np.uint8)
            keep.append(buf)
            r.height, r.width = 1, len(t.program)
            r.texels = buf.ctypes.data
        r.rgb[:] = t.pixel
        texs.append(r)
        srcs.append(src)
        index.setdefault(id(t), (len(texs) - 1, t))  # (t is held so that its id stays its own)
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
    sources = (A.rt_texels_source * len(srcs))(*srcs) if any(q.kind != A.RT_TEXELS_RECORD for q in srcs) else None
    return hs, len(objects), tex_arr, len(texs), keep, sources, index


# rt_hittable as a numpy structured dtype: what Scene.make_device takes (a numpy array of it, or its bytes as a uint8 tensor [n, itemsize]
# on a GPU).  Held to the library as compiled, like the ctypes mirrors in _lib.py.
HITTABLE_DTYPE = np.dtype([("kind", "<u4"), ("style", "<u4"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("radius", "<f8"), ("albedo", "<f8"),
                           ("fuzz", "<f8"), ("ior", "<f8"), ("prob", "<f8"), ("rgb", "u1", (3,)), ("reserved", "u1"), ("texture", "<i4")], align=True)
if lib.rt_abi_sizeof(0) != HITTABLE_DTYPE.itemsize:
    raise ImportError(f"ABI mismatch for HITTABLE_DTYPE: library {lib.rt_abi_sizeof(0)} vs numpy {HITTABLE_DTYPE.itemsize}")
for _k, _name in enumerate(HITTABLE_DTYPE.names):
    if lib.rt_abi_offsetof(0, _k) != HITTABLE_DTYPE.fields[_name][1]:
        raise ImportError(f"ABI mismatch for HITTABLE_DTYPE.{_name}: library offset {lib.rt_abi_offsetof(0, _k)} vs numpy {HITTABLE_DTYPE.fields[_name][1]}")
if lib.rt_abi_offsetof(0, len(HITTABLE_DTYPE.names)) != C.c_size_t(-1).value:
    raise ImportError("ABI mismatch for HITTABLE_DTYPE: the library has more fields than the numpy dtype")


class TextureTable(NamedTuple):
    """The rt_texture records of a list of hittables (hittable_records(..., textures=True)), for Scene.make_device(textures=...)."""
    records: object  # a ctypes array of rt_texture
    count: int
    keep: list       # the texel arrays the records point into
    sources: object = None  # a ctypes array of rt_texels_source, one per record, when a texture came from ofImageDevice / ofJpeg
    index: object = None    # {id(ParameterisedTexture value): (index of its first record, the value)} (Scene.texture_index)


def hittable_records(objects: Sequence[Hittable], textures: bool = False):
    """The rt_hittable array Scene.make builds from `objects`, as a numpy array of HITTABLE_DTYPE (a copy).  textures=True: (records, the
    TextureTable their texture indices refer to)."""
    hs, n, tex, ntex, keep, sources, index = _flatten(objects)
    rec = np.frombuffer(hs, dtype=HITTABLE_DTYPE, count=n).copy()
    return (rec, TextureTable(tex, ntex, keep, sources, index)) if textures else rec


def _sources_device(keep) -> Optional[int]:
    """The device the ofImageDevice bitmaps of a table are on (None: it has none); ValueError when they are on several."""
    devices = sorted({t.device.index for t in keep if _is_torch(t)})
    if len(devices) > 1:
        raise ValueError(f"the textures' bitmaps are on different devices: {devices}")
    return devices[0] if devices else None


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


class Surfaces(NamedTuple):
    """Surface records, one per slot in the shape of the hits they belong to (a field not asked for is None)."""
    normal: Optional[np.ndarray]  # [..., 3] float64: the normal Reflection uses (flipped when inside); NaN at a no-surface slot
    inside: Optional[np.ndarray]  # [...] uint8: 1 where the incoming ray's origin counts as inside the sphere
    colour: Optional[np.ndarray]  # [..., 3] uint8: Texture.colourAt strike / the Pixel / the cap rule
    tint: Optional[np.ndarray]    # [..., 3] uint8: the colour Reflection leaves a White ray with
    uv: Optional[np.ndarray]      # [..., 2] float64: Sphere.planeMapInverse of the strike where a parameterised texture is evaluated, else NaN
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
    def __init__(self, handle: int, keep, texture_index=None):
        self._h = C.c_void_p(handle)
        self._keep = keep
        self._texture_index = texture_index or {}
        self._images = {}  # texture index -> the tensor set_image last enqueued from
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
    def make(objects: Sequence[Hittable], walk_tree: Optional[str] = None, tree_device: Optional[int] = None,
             walk_tree_device: Optional[int] = None) -> "Scene":  # Scene.fs:15-28
        """walk_tree: None = the process default (set_walk_tree), "sah" or "reference" = this scene's own choice (rt_scene_create_ex).
        tree_device: None = BoundingBoxTree.make's tree is built on the host; a device index = on that GPU (rt_scene_create_gpu_tree): the
        same scene, node for node.  walk_tree_device: a device index = the surface-area walk tree is built on that GPU too
        (rt_scene_create_gpu_trees; tree_device defaults to the same device and must be it): the same scene again.
        With textures from ofImageDevice / ofJpeg the scene is made by rt_scene_create_textures on the bitmaps' device (0 when there are
        only JPEGs) and torch's current stream there: both trees on that GPU, the texels placed there without a host trip; a tree_device /
        walk_tree_device that is given must be that device."""
        hs, n, tex, ntex, keep, sources, index = _flatten(objects)
        out = C.c_void_p()
        opt = None if walk_tree is None else A.rt_scene_options({"sah": A.RT_WALK_TREE_SAH, "reference": A.RT_WALK_TREE_REFERENCE}[walk_tree])
        if sources is not None:
            device = _sources_device(keep)
            device = 0 if device is None else device
            for name, given in (("tree_device", tree_device), ("walk_tree_device", walk_tree_device)):
                if given is not None and int(given) != device:
                    raise ValueError(f"{name} {given} is not the textures' device {device}")
            st = _torch().cuda.current_stream(_torch().device("cuda", device)).cuda_stream
            check(lib.rt_scene_create_textures(hs, n, tex, ntex, sources, _ref(opt), device, st, C.byref(out)))
        elif walk_tree_device is not None:
            if tree_device is not None and int(tree_device) != int(walk_tree_device):
                raise ValueError(f"tree_device {tree_device} and walk_tree_device {walk_tree_device} must be the same device")
            check(lib.rt_scene_create_gpu_trees(hs, n, tex, ntex, _ref(opt), int(walk_tree_device), C.byref(out)))
        elif tree_device is not None:
            check(lib.rt_scene_create_gpu_tree(hs, n, tex, ntex, _ref(opt), int(tree_device), C.byref(out)))
        elif opt is None:
            check(lib.rt_scene_create(hs, n, tex, ntex, C.byref(out)))
        else:
            check(lib.rt_scene_create_ex(hs, n, tex, ntex, C.byref(opt), C.byref(out)))
        return Scene(out.value, keep, index)

    @staticmethod
    def make_device(records, textures=(), walk_tree: Optional[str] = None, device: Optional[int] = None, stream: Optional[int] = None) -> "Scene":
        """Scene.make from rt_hittable records that live in device memory (rt_scene_create_device): partition, boxes, both trees, ranks and
        the device image are computed on the GPU; the host never passes over the objects.  records: a torch uint8 tensor
        [n, HITTABLE_DTYPE.itemsize] on a GPU, used in place on its device and torch's current stream there (or `stream`, a HIP stream
        handle); or a numpy array of HITTABLE_DTYPE, which is staged onto `device` (0 by default) first.  textures: a TextureTable
        (hittable_records(objects, textures=True)) or nothing.  A Scene holds no Python list of its objects on any route (only the texel
        arrays its texture records point into), so nothing else changes for a scene made this way."""
        opt = None if walk_tree is None else A.rt_scene_options({"sah": A.RT_WALK_TREE_SAH, "reference": A.RT_WALK_TREE_REFERENCE}[walk_tree])
        sources, index = None, None
        if isinstance(textures, TextureTable):
            tex, ntex, keep, sources, index = textures.records, textures.count, list(textures.keep), textures.sources, textures.index
        elif len(textures) == 0:
            tex, ntex, keep = None, 0, []
        else:
            raise TypeError(f"textures must be a TextureTable (hittable_records(objects, textures=True)), not {type(textures).__name__}")
        size = HITTABLE_DTYPE.itemsize
        if _is_torch(records):
            t = _tensor_arg(records, "records", ("u8",), size)
            route = _Tensors(t.device, device)
        else:
            if not isinstance(records, np.ndarray):
                raise TypeError(f"records must be a numpy array or a torch tensor on a GPU, not {type(records).__name__}")
            if records.dtype != HITTABLE_DTYPE:
                raise TypeError(f"records must have dtype HITTABLE_DTYPE, not {records.dtype}")
            if records.ndim != 1:
                raise ValueError(f"records must have shape [n], not {list(records.shape)}")
            torch = _torch()
            where = torch.device("cuda", _Arrays(device).device)
            # (the staged tensor lives until this function returns: rt_scene_create_device copies the records into the scene's own
            # memory and returns only after the stream has finished the build, so nothing reads it afterwards)
            t = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, size)).to(where)
            route = _Tensors(where)
        st = _torch().cuda.current_stream(route.where).cuda_stream if stream is None else int(stream)
        out = C.c_void_p()
        if sources is not None:  # (textures from ofImageDevice / ofJpeg: rt_scene_create_device_textures, the bitmaps on the records' device)
            held = _sources_device(keep)
            if held is not None and held != route.device:
                raise ValueError(f"the textures' bitmaps are on device {held}, the records on device {route.device}")
            check(lib.rt_scene_create_device_textures(route.device, route.ptr(t) if t.shape[0] else None, t.shape[0], tex, ntex, sources, _ref(opt), st,
                                                      C.byref(out)))
        else:
            check(lib.rt_scene_create_device(route.device, route.ptr(t) if t.shape[0] else None, t.shape[0], tex, ntex, _ref(opt), st, C.byref(out)))
        return Scene(out.value, keep, index)

    def texture_index(self, texture) -> int:
        """The index of the texture record Scene.make / hittable_records made for a ParameterisedTexture value (its first, when several
        hittables share it): what set_image takes.  Records are numbered in the order of the hittables, a Checkered's children before it."""
        try:
            return self._texture_index[id(texture)][0]
        except KeyError:
            raise KeyError("this scene was not made from that texture value") from None

    def set_image(self, texture_index: int, bitmap, top_first: bool = True, stream: Optional[int] = None) -> None:
        """rt_scene_set_texels_device: replace the texels of image record `texture_index` by `bitmap`, a torch uint8 [height, width, 3]
        tensor on a GPU of the record's own size (top_first: rows as a decoder leaves them; False: already img.[y]).  Enqueued on torch's
        current stream on the bitmap's device (or `stream`); renders enqueued there afterwards see the new texels.  The scene keeps the
        tensor until the next set_image of that record."""
        t = ParameterisedTexture.ofImageDevice(bitmap).bitmap
        st = _torch().cuda.current_stream(t.device).cuda_stream if stream is None else int(stream)
        check(lib.rt_scene_set_texels_device(self._h, int(texture_index), t.device.index, t.data_ptr(), t.numel(),
                                             A.RT_TEXELS_TOP_FIRST if top_first else 0, st))
        self._images[int(texture_index)] = t

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

    def _call(self, fn, *args, stats: bool = True) -> Optional[dict]:
        """fn(scene, *args, stats), checked.  The statistics go to last_stats and are returned (None where none were asked for)."""
        st = A.rt_stats() if stats else None
        check(fn(self._h, *args, _ref(st)))
        self.last_stats = st.as_dict() if st is not None else None
        return self.last_stats

    def _launch(self, route, base: str, *args, stats: bool, options) -> Optional[dict]:
        """The entry point `base` of the route (base itself for arrays, base_device for tensors) with the arguments between the scene
        and the tail, which is the route's: stats for arrays, which always collect them; stream, options, stats for tensors."""
        assert base in _ROUTED, base
        return self._call(getattr(lib, base + route.suffix), *args, *route.tail(options), stats=stats or not route.suffix)

    def render_rows(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, *, seed: int = 0, device: int = 0,
                    row_first: int = 0, row_stride: int = 1, n_rows: Optional[int] = None, counters: bool = False) -> RenderResult:
        """rt_render for the image rows row_first + i*row_stride (the whole frame by default)."""
        rows = 2 * maxHeightCoord + 1
        cols = 2 * maxWidthCoord + 1
        if n_rows is None:
            n_rows = max(0, (rows - row_first + row_stride - 1) // row_stride)
        accum = np.zeros((n_rows, cols, 4), np.int32)
        rgb = np.zeros((n_rows, cols, 3), np.uint8)
        st = self._call(lib.rt_render, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, row_first, row_stride, n_rows,
                        _flags(counters), _i32(accum), _u8(rgb))
        return RenderResult(accum, rgb, st)

    def renderPpm(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False) -> dict:
        """rt_render_ppm: Scene.render |> ImageOutput.writePpm in one call -- the frame rendered, formatted as P3 text on the device and
        written to `path`; byte for byte ImageOutput.writePpm of render_rows' rgb.  Returns the statistics (total_ms covers the file)."""
        return self._call(lib.rt_render_ppm, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, _flags(counters),
                          int(bool(gammaCorrect)), str(path).encode(), None)

    def renderPng(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, path: str, *, gammaCorrect: bool = True, seed: int = 0,
                  device: int = 0, counters: bool = False) -> dict:
        """rt_render_png: Scene.render |> Png.write (Program.fs:47-50) in one call -- the frame rendered, encoded as a PNG on the device and
        written to `path`; byte for byte Png.format of render_rows' rgb.  Returns the statistics (total_ms covers the file)."""
        return self._call(lib.rt_render_png, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, _flags(counters),
                          int(bool(gammaCorrect)), str(path).encode(), None)

    def resume(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, data: bytes, *, seed: int = 0, device: int = 0, counters: bool = False,
               options: Optional[A.rt_render_options] = None) -> np.ndarray:
        """rt_resume_pixel_map: Program.fs:45-49 for an interrupted frame -- the pixel map `data` (bytes) parsed on the device, the pixels
        it lacks rendered alone and scattered in -> rgb [rows, cols, 3] uint8.  For a map of render_rows' own records (any order, any
        subset, duplicated or truncated) that is render_rows' rgb byte for byte.  last_stats: pixels = the number rendered."""
        data = bytes(data)
        rgb = np.zeros((2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1, 3), np.uint8)
        self._call(lib.rt_resume_pixel_map, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, _flags(counters), data, len(data),
                   _u8(rgb), _ref(options))
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
        return self._call(fn, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, device, _flags(counters), str(mapPath).encode(),
                          int(bool(gammaCorrect)), str(path).encode(), _ref(options))

    def extend_rows(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, accum, samplesDone: int, *, seed: int = 0,
                    device: Optional[int] = None, row_first: int = 0, row_stride: int = 1, counters: bool = False, stats: bool = True,
                    options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_extend: continues `accum` -- the PixelStats of the rows row_first + i*row_stride, rendered or last extended with
        samplesDone (>= 12) samples per pixel -- to camera.SamplesPerPixel; the result is, bit for bit, a render at that count.
        Everything but the sample count as in the call that made the buffer.  A numpy array [n_rows, cols, 4] int32 is left as it
        is and a new one returned; a torch tensor on a GPU is extended IN PLACE through rt_render_extend_device on
        torch.cuda.current_stream() (stats=False: no wait for the device; a malformed buffer then goes unreported and unchanged)."""
        cols = 2 * maxWidthCoord + 1
        route, out, _ = _frame(accum, cols, device, options)
        n_rows = out.shape[0]
        rgb = route.make((n_rows, cols, 3), "u8")
        st = self._launch(route, "rt_render_extend", C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, row_first, row_stride,
                          n_rows, _flags(counters), samplesDone, route.ptr(out), route.ptr(rgb), stats=stats, options=options)
        return RenderResult(out, rgb, st)

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
        route, out, tg = _frame(accum, cols, device, options, mapped=True, targets=targets)
        n_rows = out.shape[0]
        rgb = route.make((n_rows, cols, 3), "u8")
        st = self._launch(route, "rt_render_extend_map", C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, row_first,
                          row_stride, n_rows, _flags(counters), route.ptr(tg), route.ptr(out), route.ptr(rgb), stats=stats, options=options)
        return RenderResult(out, rgb, st)

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
        route, r = _route(rays, "rays", "f64", 6, device, options)
        n = r.shape[0]
        hit, strike = route.make((n,), "i32"), route.make((n, 3), "f64")
        self._launch(route, "rt_hit_objects", route.device, n, route.ptr(r), _flags(counters), route.ptr(hit), route.ptr(strike), stats=stats, options=options)
        return hit, strike

    def traceRays(self, rays, bounceDepth: int, *, rng=None, seed: int = 0, stream_base: int = 0, sample: int = 0,
                  device: Optional[int] = None, counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None):
        """Scene.traceRay (Scene.fs:93-114) from LightRay {Ray.make'(origin, vector); Colour.White} for the caller's rays [n, 6],
        at most bounceDepth+1 hits -> (colour uint8 [n, 3], rng_out).  rng: [n, 4] uint32 xorshift128 states (FloatProducer), which
        are not modified: rng_out holds them advanced.  rng=None: ray i draws from the stream keyed (seed, stream_base + i, sample),
        as a render's (pixel, sample), and rng_out is None.  numpy arrays / torch tensors as for hitObject (a tensor rng may be
        uint32 or int32: the bits are the state)."""
        route, r = _route(rays, "rays", "f64", 6, device, options)
        n = r.shape[0]
        g = _rng(route, rng, n)
        colour = route.make((n, 3), "u8")
        self._launch(route, "rt_trace_rays", route.device, n, route.ptr(r), route.ptr(g), seed, stream_base, sample, bounceDepth, _flags(counters),
                     route.ptr(colour), stats=stats, options=options)
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
        route, f = _route(footprints, "footprints", "f64", 12, device, options)
        n = f.shape[0]
        kind, before, accum = _list_extension(route, n, extend, extend_map, "footprints", "the footprints' device")
        rgb = route.make((n, 3), "u8")
        st = self._launch(route, "rt_render_footprints" + kind, route.device, n, route.ptr(f), samplesPerPixel, bounceDepth, seed, stream_base,
                          _flags(counters), *before, route.ptr(accum), route.ptr(rgb), stats=stats, options=options)
        return RenderResult(accum, rgb, st)

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
        route, px = _route(pixels, "pixels", "i32", None, device, options)
        n = px.shape[0]
        kind, before, accum = _list_extension(route, n, extend, None, "list entries", "the list's device")
        rgb = route.make((n, 3), "u8")
        st = self._launch(route, "rt_render_pixels" + kind, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, n, route.ptr(px),
                          _flags(counters), *before, route.ptr(accum), route.ptr(rgb), stats=stats, options=options)
        return RenderResult(accum, rgb, st)

    def renderViews(self, maxWidthCoord: int, maxHeightCoord: int, cameras: Sequence[Camera], *, seeds: Optional[Sequence[int]] = None, seed: int = 0,
                    device: Optional[int] = None, counters: bool = False, accum=None, options: Optional[A.rt_render_options] = None,
                    stats: bool = True) -> RenderResult:
        """rt_render_views: Scene.render (Scene.fs:157-236) for K cameras over this scene in ONE launch -> RenderResult(accum [K, rows,
        cols, 4] int32, rgb [K, rows, cols, 3] uint8, stats).  View v is, in every PixelStats word and every rgb byte, render_rows of
        the whole frame with cameras[v] and seed seeds[v] (seeds=None: `seed` for every view); the cameras share SamplesPerPixel and
        BounceDepth.  stats sums the views' (pixels = K * rows * cols).  accum: a contiguous int32 torch tensor [K, rows, cols, 4] on
        a GPU -- the batch renders INTO it through rt_render_views_device on torch.cuda.current_stream() and rgb is a tensor there
        (stats=False: no wait for the device); view v's slice is a frame's buffer, which extend_rows continues with cameras[v].
        Otherwise arrays come back.  A scene that holds a texture program is refused (RT_ERR_UNSUPPORTED)."""
        cams = list(cameras)
        k = len(cams)
        rows, cols = 2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1
        if seeds is not None and len(seeds) != k:
            raise ValueError(f"seeds must hold one seed per camera ({k}), not {len(seeds)}")
        if accum is None:
            _no_options(options)
            big = k * rows * cols > 2**31 - 1 or rows <= 0 or cols <= 0  # (refused by the library: nothing to zero first)
            route = _Arrays(device)
            out = route.make((0, 0, 0, 4) if big else (k, rows, cols, 4), "i32")
        else:
            if (not _is_torch(accum) or accum.dtype != _torch().int32 or tuple(accum.shape) != (k, rows, cols, 4) or not accum.is_cuda
                    or not accum.is_contiguous()):
                raise ValueError(f"accum must be a contiguous int32 tensor [{k}, {rows}, {cols}, 4] on a GPU")
            route, out = _Tensors(accum.device, device), accum
        rgb = route.make(tuple(out.shape[:3]) + (3,), "u8")
        abi = (A.rt_camera * max(k, 1))(*[c.to_abi() for c in cams])
        keys = None if seeds is None else (C.c_uint64 * max(k, 1))(*[int(s) for s in seeds])
        # (the route's entry point and tail, as Scene._launch gives them; the pair is not in _ROUTED, whose twelve pairs tests/test_abi.py pins)
        st = self._call(getattr(lib, "rt_render_views" + route.suffix), abi if k else None, k, maxWidthCoord, maxHeightCoord, keys, seed, route.device,
                        _flags(counters), route.ptr(out) if k else None, route.ptr(rgb) if k else None, *route.tail(options), stats=stats or not route.suffix)
        return RenderResult(out, rgb, st)

    def renderViewsPng(self, maxWidthCoord: int, maxHeightCoord: int, cameras: Sequence[Camera], paths: Sequence[str], *, gammaCorrect: bool = True,
                       seeds: Optional[Sequence[int]] = None, seed: int = 0, device: Optional[int] = None, counters: bool = False,
                       options: Optional[A.rt_render_options] = None) -> dict:
        """rt_render_views_png: renderViews |> Png.writeViews in one call -- the K views rendered in one launch, encoded as K PNGs in the
        four launches one image takes, copied out once and written to paths[v]; file v is byte for byte Png.format of renderViews' rgb[v]
        for the same arguments, and the pixels never visit the host as rgb.  Returns the statistics (total_ms covers the files)."""
        cams, names = list(cameras), [str(p) for p in paths]
        k = len(cams)
        _one_path_per_view(names, k)
        if seeds is not None and len(seeds) != k:
            raise ValueError(f"seeds must hold one seed per camera ({k}), not {len(seeds)}")
        abi = (A.rt_camera * max(k, 1))(*[c.to_abi() for c in cams])
        keys = None if seeds is None else (C.c_uint64 * max(k, 1))(*[int(s) for s in seeds])
        return self._call(lib.rt_render_views_png, abi if k else None, k, maxWidthCoord, maxHeightCoord, keys, seed, 0 if device is None else device,
                          _flags(counters), int(bool(gammaCorrect)), _path_array(names), _ref(options))

    def extendViews(self, maxWidthCoord: int, maxHeightCoord: int, cameras: Sequence[Camera], accum, samplesDone: int, *,
                    seeds: Optional[Sequence[int]] = None, seed: int = 0, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                    options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_views_extend: continues `accum` -- renderViews' buffer [K, rows, cols, 4] int32 (or K frames of render_rows stacked),
        rendered or last extended with samplesDone (>= 12) samples per pixel -- to the cameras' shared SamplesPerPixel, all K views in
        ONE launch (Scene.fs:157-236 at the higher count); view v is then, bit for bit, render_rows with cameras[v] and seed seeds[v] at that
        count.  Everything but the sample count as in the call that made the buffer.  A numpy array is copied and a new one returned; a
        contiguous int32 torch tensor on a GPU is continued IN PLACE through rt_render_views_extend_device on torch.cuda.current_stream()
        (stats=False: no wait for the device; a malformed buffer then goes unreported and unchanged).  stats describe the extension alone."""
        return self._extend_views("rt_render_views_extend", maxWidthCoord, maxHeightCoord, cameras, accum, None, (samplesDone,), seeds, seed, device,
                                  counters, stats, options)

    def extendViewsMap(self, maxWidthCoord: int, maxHeightCoord: int, cameras: Sequence[Camera], accum, targets, *,
                       seeds: Optional[Sequence[int]] = None, seed: int = 0, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                       options: Optional[A.rt_render_options] = None) -> RenderResult:
        """rt_render_views_extend_map: continues every pixel of `accum` [K, rows, cols, 4] from its own Count to targets[v, row, col] (int32
        [K, rows, cols]) in ONE launch; the classes of extend_rows_map, the cameras' shared SamplesPerPixel the upper bound on every target.
        Every view may have a budget of its own.  Each pixel is then, bit for bit, that pixel of render_rows of its view at its Count.
        Arrays and tensors as for extendViews; with a tensor accum, `targets` must be a tensor on the same device."""
        return self._extend_views("rt_render_views_extend_map", maxWidthCoord, maxHeightCoord, cameras, accum, targets, None, seeds, seed, device,
                                  counters, stats, options)

    def _extend_views(self, base, maxWidthCoord, maxHeightCoord, cameras, accum, targets, done, seeds, seed, device, counters, stats, options):
        cams = list(cameras)
        k = len(cams)
        rows, cols = 2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1
        if seeds is not None and len(seeds) != k:
            raise ValueError(f"seeds must hold one seed per camera ({k}), not {len(seeds)}")
        if _is_torch(accum):
            if accum.dtype != _torch().int32 or tuple(accum.shape) != (k, rows, cols, 4) or not accum.is_cuda or not accum.is_contiguous():
                raise ValueError(f"accum must be a contiguous int32 tensor [{k}, {rows}, {cols}, 4] on a GPU")
            route, out = _Tensors(accum.device, device), accum
        else:
            _no_options(options)
            if not isinstance(accum, np.ndarray) or accum.dtype != np.int32 or accum.shape != (k, rows, cols, 4):
                raise ValueError(f"accum must be an int32 array [{k}, {rows}, {cols}, 4] or such a tensor on a GPU")
            route, out = _Arrays(device), np.array(accum, dtype=np.int32, order="C")
        before = done if done is not None else (route.ptr(_targets(route, targets, (k, rows, cols), f"[{k}, {rows}, {cols}]", "accum's device")),)
        rgb = route.make((k, rows, cols, 3), "u8")
        abi = (A.rt_camera * max(k, 1))(*[c.to_abi() for c in cams])
        keys = None if seeds is None else (C.c_uint64 * max(k, 1))(*[int(s) for s in seeds])
        # (the route's entry point and tail, as Scene._launch gives them; the pairs are not in _ROUTED, whose twelve pairs tests/test_abi.py pins)
        st = self._call(getattr(lib, base + route.suffix), abi if k else None, k, maxWidthCoord, maxHeightCoord, keys, seed, route.device, _flags(counters),
                        *before, route.ptr(out) if k else None, route.ptr(rgb) if k else None, *route.tail(options), stats=stats or not route.suffix)
        return RenderResult(out, rgb, st)

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
        if not isinstance(n_samples, int) or not isinstance(sample_first, int):
            raise TypeError("sample_first and n_samples must be ints")
        route, px, count = _pixel_list(pixels, n, tensors, maxWidthCoord, maxHeightCoord, device, options)
        per = max(n_samples, 0)
        shape = _lead(route, (count, per), count * per)
        hit = route.make(shape, "i32")
        sk = route.make(shape + (3,), "f64") if strike else None
        ry = route.make(shape + (6,), "f64") if rays else None
        st = self._launch(route, "rt_camera_hits", C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, count, route.ptr(px),
                          sample_first, n_samples, _flags(counters), route.ptr(hit), route.ptr(sk), route.ptr(ry), stats=stats, options=options)
        return CameraHits(hit, sk, ry, st)

    def cameraHitsViews(self, maxWidthCoord: int, maxHeightCoord: int, cameras: Sequence[Camera], pixels=None, *, seeds: Optional[Sequence[int]] = None,
                        seed: int = 0, sample_first: int = 0, n_samples: int = 1, n: Optional[int] = None, strike: bool = True, rays: bool = True,
                        tensors: bool = False, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                        options: Optional[A.rt_render_options] = None) -> CameraHits:
        """rt_camera_hits_views: cameraHits for K cameras over this scene and ONE list of pixels in ONE launch -> CameraHits(hit_index
        [K, n, n_samples], strike [K, n, n_samples, 3], rays [K, n, n_samples, 6], stats).  View v's slice is, bit for bit, cameraHits
        with cameras[v], seed seeds[v] (seeds=None: `seed` for every view) and the same pixels, sample range and geometry; the cameras
        need not share SamplesPerPixel or BounceDepth, and a scene that holds a texture program is taken.  stats sums the views'
        (pixels = K * n).  Arrays and tensors exactly as for cameraHits: a tensor list goes through rt_camera_hits_views_device on
        torch.cuda.current_stream() and the results are tensors (stats=False: no wait for the device; a list with an entry outside
        the frame then goes unreported and nothing is written in any view)."""
        if not isinstance(n_samples, int) or not isinstance(sample_first, int):
            raise TypeError("sample_first and n_samples must be ints")
        cams = list(cameras)
        k = len(cams)
        if seeds is not None and len(seeds) != k:
            raise ValueError(f"seeds must hold one seed per camera ({k}), not {len(seeds)}")
        route, px, count = _pixel_list(pixels, n, tensors, maxWidthCoord, maxHeightCoord, device, options)
        per = max(n_samples, 0)
        shape = _lead(route, (k, count, per), k * count * per)
        hit = route.make(shape, "i32")
        sk = route.make(shape + (3,), "f64") if strike else None
        ry = route.make(shape + (6,), "f64") if rays else None
        abi = (A.rt_camera * max(k, 1))(*[c.to_abi() for c in cams])
        keys = None if seeds is None else (C.c_uint64 * max(k, 1))(*[int(s) for s in seeds])
        # (the route's entry point and tail, as Scene._launch gives them; the pair is not in _ROUTED, whose twelve pairs tests/test_abi.py pins)
        st = self._call(getattr(lib, "rt_camera_hits_views" + route.suffix), abi if k else None, k, maxWidthCoord, maxHeightCoord, keys, seed, route.device,
                        count, route.ptr(px), sample_first, n_samples, _flags(counters), route.ptr(hit), route.ptr(sk), route.ptr(ry), *route.tail(options),
                        stats=stats or not route.suffix)
        return CameraHits(hit, sk, ry, st)

    @staticmethod
    def _surface_buffers(route, lead, normal, inside, colour, tint, uv):
        """The output buffers of a surface call, shaped lead + (...), and the rt_surface_outputs that names them."""
        bufs = {"normal": route.make(lead + (3,), "f64") if normal else None, "inside": route.make(lead, "u8") if inside else None,
                "colour": route.make(lead + (3,), "u8") if colour else None, "tint": route.make(lead + (3,), "u8") if tint else None,
                "uv": route.make(lead + (2,), "f64") if uv else None}
        return bufs, A.rt_surface_outputs(**{f: C.cast(route.ptr(b), C.c_void_p).value for f, b in bufs.items()})

    def surfaces(self, hit_index, strike, rays, *, normal: bool = True, inside: bool = True, colour: bool = True, tint: bool = True, uv: bool = False,
                 device: Optional[int] = None, counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None) -> Surfaces:
        """rt_surfaces: what the surface is like at a list of hits -- hit_index [n] int32 (as hitObject returns it), strike [n, 3] and
        rays [n, 6] float64 (only the origins are read) -> Surfaces(normal [n, 3], inside [n], colour [n, 3], tint [n, 3], uv [n, 2],
        stats): the normal and the inside flag Hittable.Reflection forms, the surface's colour (Texture.colourAt strike, the Pixel, the
        cap rule), the colour a White ray leaves with, and the texture coordinates.  A slot with hit_index < 0 or a strike or origin
        that is not finite has no surface: NaN normal and uv, zeros elsewhere.  numpy arrays / torch tensors exactly as for hitObject
        (tensors: rt_surfaces_device on torch.cuda.current_stream(); stats=False: no wait for the device, and an index outside the
        scene's objects then goes unreported and nothing is written)."""
        route, h = _route(hit_index, "hit_index", "i32", None, device, options)
        n = h.shape[0]
        if route.suffix:
            sk, r = _tensor_arg(strike, "strike", ("f64",), 3), _tensor_arg(rays, "rays", ("f64",), 6)
            if sk.device != route.where or r.device != route.where:
                raise ValueError("strike and rays must be on hit_index's device")
        else:
            sk, r = _array_arg(strike, "strike", "f64", 3), _array_arg(rays, "rays", "f64", 6)
        if sk.shape[0] != n or r.shape[0] != n:
            raise ValueError("strike must be [n, 3] and rays [n, 6] for n hits")
        bufs, out = Scene._surface_buffers(route, (n,), normal, inside, colour, tint, uv)
        # (the route's entry point and tail, as Scene._launch gives them; the pair is not in _ROUTED, whose twelve pairs tests/test_abi.py pins)
        st = self._call(getattr(lib, "rt_surfaces" + route.suffix), route.device, n, route.ptr(h), route.ptr(sk), route.ptr(r), _flags(counters),
                        C.byref(out), *route.tail(options), stats=stats or not route.suffix)
        return Surfaces(stats=st, **bufs)

    def cameraSurfaces(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, pixels=None, *, sample_first: int = 0, n_samples: int = 1,
                       seed: int = 0, n: Optional[int] = None, hit_index: bool = True, strike: bool = True, normal: bool = True, inside: bool = True,
                       colour: bool = True, tint: bool = True, uv: bool = False, tensors: bool = False, device: Optional[int] = None,
                       counters: bool = False, stats: bool = True, options: Optional[A.rt_render_options] = None):
        """rt_camera_surfaces: cameraHits and the surface record of every hit in one call -> (CameraHits(hit_index [n, n_samples], strike
        [n, n_samples, 3], None, stats), Surfaces([n, n_samples, ...])): albedo, normal and uv buffers of a frame without a host trip.
        hit_index and strike are cameraHits' bit for bit (hit_index=False / strike=False: not returned, None).  Lists, tensors=,
        device=, stats= and options= exactly as for cameraHits."""
        if not isinstance(n_samples, int) or not isinstance(sample_first, int):
            raise TypeError("sample_first and n_samples must be ints")
        route, px, count = _pixel_list(pixels, n, tensors, maxWidthCoord, maxHeightCoord, device, options)
        per = max(n_samples, 0)
        shape = _lead(route, (count, per), count * per)
        hit = route.make(shape, "i32") if hit_index else None
        sk = route.make(shape + (3,), "f64") if strike else None
        bufs, out = Scene._surface_buffers(route, shape, normal, inside, colour, tint, uv)
        st = self._call(getattr(lib, "rt_camera_surfaces" + route.suffix), C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, count,
                        route.ptr(px), sample_first, n_samples, _flags(counters), route.ptr(hit), route.ptr(sk), C.byref(out), *route.tail(options),
                        stats=stats or not route.suffix)
        return CameraHits(hit, sk, None, st), Surfaces(stats=st, **bufs)

    @staticmethod
    def _path_buffers(route, lead, max_vertices, records, first_ray=False, summary_entries=None):
        """The output buffers of a path call, shaped lead + (...), and the rt_path_outputs that names them."""
        k = max(max_vertices, 0)
        bufs = {"n_vertices": route.make(lead, "i32"), "end": route.make(lead, "i32"), "colour": route.make(lead + (3,), "u8")}
        bufs["first_ray"] = route.make(lead + (6,), "f64") if first_ray else None
        rec = records and k > 0
        bufs["hit_index"] = route.make(lead + (k,), "i32") if rec else None
        bufs["strike"] = route.make(lead + (k, 3), "f64") if rec else None
        bufs["colour_after"] = route.make(lead + (k, 3), "u8") if rec else None
        bufs["ray_after"] = route.make(lead + (k, 6), "f64") if rec else None
        bufs["summary"] = route.make((summary_entries, A.RT_PATH_SUMMARY_WORDS), "i32") if summary_entries is not None else None
        return bufs, A.rt_path_outputs(max_vertices=max_vertices, **{f: C.cast(route.ptr(b), C.c_void_p).value for f, b in bufs.items()})

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
        if not isinstance(n_samples, int) or not isinstance(sample_first, int) or not isinstance(max_vertices, int):
            raise TypeError("sample_first, n_samples and max_vertices must be ints")
        route, px, count = _pixel_list(pixels, n, tensors, maxWidthCoord, maxHeightCoord, device, options)
        per = max(n_samples, 0)
        lead = _lead(route, (count, per), count * per * max(max_vertices, 1))
        bufs, out = Scene._path_buffers(route, lead, max_vertices, records, first_ray, lead[0] if summary else None)
        st = self._launch(route, "rt_camera_paths", C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, count, route.ptr(px),
                          sample_first, n_samples, _flags(counters), C.byref(out), stats=stats, options=options)
        return CameraPaths(stats=st, **bufs)

    def tracePaths(self, rays, bounceDepth: int, *, rng=None, seed: int = 0, stream_base: int = 0, sample: int = 0, max_vertices: int = 8,
                   records: bool = True, device: Optional[int] = None, counters: bool = False, stats: bool = True,
                   options: Optional[A.rt_render_options] = None) -> TracePaths:
        """traceRays with the path written down: rays, rng, seed, stream_base, sample and bounceDepth are traceRays' (colour and the
        advanced states equal its) -> TracePaths.  numpy arrays / torch tensors as for traceRays."""
        if not isinstance(max_vertices, int):
            raise TypeError("max_vertices must be an int")
        route, r = _route(rays, "rays", "f64", 6, device, options)
        n = r.shape[0]
        g = _rng(route, rng, n)
        bufs, out = Scene._path_buffers(route, _lead(route, (n,), n * max(max_vertices, 1)), max_vertices, records)
        st = self._launch(route, "rt_trace_paths", route.device, n, route.ptr(r), route.ptr(g), seed, stream_base, sample, bounceDepth, _flags(counters),
                          C.byref(out), stats=stats, options=options)
        return TracePaths(bufs["n_vertices"], bufs["end"], bufs["colour"], g, bufs["hit_index"], bufs["strike"], bufs["colour_after"], bufs["ray_after"], st)

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

    def render_job(self, maxWidthCoord: int, maxHeightCoord: int, camera: Camera, *, seed: int = 0, device: Optional[int] = None,
                   row_first: int = 0, row_stride: int = 1, n_rows: Optional[int] = None, accum=None, rgb=True, present=None,
                   options: Optional[A.rt_render_options] = None) -> "RenderJob":
        """rt_render_job_start: render_rows' shard as a JOB -- launched and left running, with progress(), stop(), wait() and finish()
        (Scene.fs:196-236 watched and interrupted; ImageOutput.fs:131-161's spill).  The job's buffers live on the GPU: with `accum` a
        contiguous int32 torch tensor [n_rows, cols, 4] there the job renders INTO it on torch's current stream and its accum / rgb /
        present are tensors; with accum None or a numpy array of that shape the buffers are the job's own and accum / rgb / present
        come back as arrays (a given array is filled by wait() and finish()).  rgb: False for no colour buffer; on the tensor route
        `rgb` and `present` may be the caller's own contiguous uint8 tensors [n_rows, cols, 3] and [n_rows, cols] on accum's device."""
        torch = _torch()
        rows, cols = 2 * maxHeightCoord + 1, 2 * maxWidthCoord + 1
        if n_rows is None:
            n_rows = max(0, (rows - row_first + row_stride - 1) // row_stride)
        host_out = None
        if accum is not None and _is_torch(accum):
            route, buf, _ = _frame(accum, cols, device, options)
            if buf.shape[0] != n_rows:
                raise ValueError(f"accum must hold the shard's {n_rows} rows")
        else:
            if accum is not None and (not isinstance(accum, np.ndarray) or accum.dtype != np.int32 or accum.shape != (n_rows, cols, 4)):
                raise ValueError(f"accum must be an int32 array [{n_rows}, {cols}, 4] or such a tensor on a GPU")
            host_out = accum
            route = _Tensors(torch.device("cuda", torch.cuda.current_device() if device is None else device))
            buf = route.make((n_rows, cols, 4), "i32")
        def own(t, shape, name):
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or t.device != route.where or not t.is_contiguous() or host_out is not None or accum is None:
                raise ValueError(f"{name} must be a contiguous uint8 tensor {list(shape)} on accum's device, with accum a tensor")
            return t

        colour = own(rgb, (n_rows, cols, 3), "rgb") if _is_torch(rgb) else (route.make((n_rows, cols, 3), "u8") if rgb else None)
        present = own(present, (n_rows, cols), "present") if present is not None else route.make((n_rows, cols), "u8")
        handle = C.c_void_p()
        stream = torch.cuda.current_stream(route.where).cuda_stream
        check(lib.rt_render_job_start(self._h, C.byref(camera.to_abi()), maxWidthCoord, maxHeightCoord, seed, route.device, row_first, row_stride, n_rows,
                                      0, route.ptr(buf), route.ptr(colour), route.ptr(present), stream, _ref(options), C.byref(handle)))
        return RenderJob(self, handle, route, stream, buf, colour, present, host_out, accum is not None and _is_torch(accum))

    def render_watch(self, progressIncrement: Callable[[float], None], should_stop: Callable[[], bool], maxWidthCoord: int, maxHeightCoord: int,
                     camera: Camera, *, seed: int = 0, device: Optional[int] = None, poll_seconds: float = 0.0005,
                     options: Optional[A.rt_render_options] = None):
        """Scene.render watched (Scene.fs:196-236): the frame as a render job, polled while the GPU works.  `progressIncrement 1.0` is
        called once per row's worth of final pixels (Scene.fs:232) -- `rows` times in all when the frame completes, fewer when it is
        stopped -- and the job is asked to stop as soon as should_stop() answers true.  Returns (rgb [rows, cols, 3] with absent
        pixels zero, present [rows, cols] bool, the partial pixel map's bytes -- ImageOutput.resume's spill, which Scene.resume takes)."""
        import time

        cols = 2 * maxWidthCoord + 1
        ticks = 0
        with self.render_job(maxWidthCoord, maxHeightCoord, camera, seed=seed, device=device, options=options) as job:
            while True:
                pr = job.progress()
                while ticks < pr["pixels_final"] // cols:
                    progressIncrement(1.0)
                    ticks += 1
                if pr["state"] == 2:
                    break
                if pr["state"] == 0 and should_stop():
                    job.stop()
                time.sleep(poll_seconds)
            res = job.wait()
            while ticks < res["n_present"] // cols:
                progressIncrement(1.0)
                ticks += 1
            return job.rgb, job.present, job.pixel_map()


class RenderJob:
    """A render job (rt_render_job_*; DESIGN.md "Render jobs").  Use as a context manager, or call close()."""

    def __init__(self, scene: Scene, handle, route, stream, accum, rgb, present, host_out, tensors: bool):
        self._scene, self._h, self._route, self._stream = scene, handle, route, stream  # (the scene must outlive the job)
        self._accum, self._rgb, self._present, self._host_out, self._tensors = accum, rgb, present, host_out, tensors
        self.result: Optional[dict] = None

    def progress(self) -> dict:
        """rt_render_job_progress: {state (0 running, 1 stop requested, 2 finished), pixels_total, pixels_final}; never blocks."""
        p = A.rt_job_progress()
        check(lib.rt_render_job_progress(self._h, C.byref(p)))
        return {"state": p.state, "pixels_total": p.pixels_total, "pixels_final": p.pixels_final}

    def stop(self) -> None:
        """rt_render_job_stop: from any thread, also while another sits in wait()."""
        check(lib.rt_render_job_stop(self._h))

    def wait(self) -> dict:
        """rt_render_job_wait -> {complete, stop_requested, pixels_total, n_present, stats}."""
        r, st = A.rt_job_result(), A.rt_stats()
        check(lib.rt_render_job_wait(self._h, C.byref(r), C.byref(st)))
        self.result = {"complete": bool(r.complete), "stop_requested": bool(r.stop_requested), "pixels_total": r.pixels_total,
                       "n_present": r.n_present, "stats": st.as_dict()}
        self._copy_out()
        return self.result

    def finish(self) -> dict:
        """rt_render_job_finish: the absent pixels rendered and scattered in; afterwards the buffers are render_rows' -> the statistics."""
        st = A.rt_stats()
        check(lib.rt_render_job_finish(self._h, self._stream, C.byref(st)))
        if self.result is not None:
            self.result = dict(self.result, complete=True, n_present=self.result["pixels_total"])
        self._copy_out()
        return st.as_dict()

    def plan(self) -> dict:
        """rt_dev_last_job_plan of the calling thread (this job's after its wait())."""
        w = (C.c_int64 * 8)()
        check(lib.rt_dev_last_job_plan(w))
        return dict(zip(("passes", "chunk", "units_a", "n_list", "done_a", "done_b", "block", "textured"), (int(x) for x in w)))

    def _copy_out(self) -> None:
        if self._host_out is not None:
            self._host_out[...] = self._accum.cpu().numpy()

    def _out(self, t):
        if t is None or self._tensors:
            return t
        return t.cpu().numpy()

    @property
    def accum(self):
        return self._out(self._accum)

    @property
    def rgb(self):
        return self._out(self._rgb)

    @property
    def present(self):
        """[n_rows, cols] bool (after wait()): the pixels that have every sample the frame gives them."""
        p = self._present.bool()
        return p if self._tensors else p.cpu().numpy()

    def pixel_map(self) -> bytes:
        """rt_format_pixel_map_present_device: ImageOutput.resume's records of the present pixels, row-major -- the partial spill.
        (A shard's rows are numbered as the shard's own: use whole frames for a map Scene.resume is to take.)"""
        if self._rgb is None:
            raise ValueError("the job was started with rgb=False")
        torch = _torch()
        rows, cols = int(self._present.shape[0]), int(self._present.shape[1])
        if rows == 0:
            return b""
        cap = _size(lib.rt_pixel_map_bytes(rows, cols))
        out = torch.empty(cap, dtype=torch.uint8, device=self._route.where)
        n = C.c_int64(0)
        check(lib.rt_format_pixel_map_present_device(self._route.device, self._rgb.data_ptr(), self._present.data_ptr(), rows, cols, out.data_ptr(), cap,
                                                     None, self._stream, C.byref(n)))
        return out[: n.value].cpu().numpy().tobytes()

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            lib.rt_render_job_destroy(h)

    def __enter__(self) -> "RenderJob":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        self.close()


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
        return _format_host(lib.rt_format_ppm, pixels, int(bool(gammaCorrect)), spare=1)

    @staticmethod
    def formatPpmDevice(gammaCorrect: bool, pixels):
        """rt_format_ppm_device on torch.cuda.current_stream(), without waiting for the device: (text, length) -- a uint8 tensor of
        rt_ppm_max_bytes(rows, cols) bytes whose first `length` (an int64 tensor) are ImageOutput.writePpm's; the rest is not written."""
        return _format_device(lib.rt_ppm_max_bytes, lib.rt_format_ppm_device, gammaCorrect, pixels)

    @staticmethod
    def formatPixelMap(pixels) -> bytes:
        """The pixel-map bytes of ImageOutput.resume / toPpm (ImageOutput.fs:115-161): per pixel `<row>,<col>\n` (0 as NO digits) and the
        three raw colour bytes.  numpy: rt_format_pixel_map on the host; a torch tensor on a GPU: rt_format_pixel_map_device."""
        if _is_torch(pixels):
            t = _image_tensor(pixels)
            torch = _torch()
            rows, cols = int(t.shape[0]), int(t.shape[1])
            cap = _size(lib.rt_pixel_map_bytes(rows, cols))
            out = torch.empty(cap, dtype=torch.uint8, device=t.device)
            n = C.c_int64(0)
            check(lib.rt_format_pixel_map_device(t.device.index, t.data_ptr(), rows, cols, out.data_ptr(), cap, None,
                                                 torch.cuda.current_stream(t.device).cuda_stream, C.byref(n)))
            return out[: n.value].cpu().numpy().tobytes()
        return _format_host(lib.rt_format_pixel_map, pixels)

    @staticmethod
    def formatPixelMapPresent(pixels, present) -> bytes:
        """rt_format_pixel_map_present: formatPixelMap's records for the pixels with present[row, col] set only, row-major -- the spill an
        interrupted ImageOutput.resume (ImageOutput.fs:131-161) leaves.  numpy arrays [rows, cols, 3] uint8 and [rows, cols] bool or uint8."""
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        pr = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
        if px.ndim != 3 or px.shape[2] != 3 or pr.shape != px.shape[:2]:
            raise ValueError("pixels must be [rows, cols, 3] and present [rows, cols]")
        head = (_u8(px), _u8(pr), px.shape[0], px.shape[1])
        n = _size(lib.rt_format_pixel_map_present(*head, None, 0))
        buf = C.create_string_buffer(max(n, 1))
        lib.rt_format_pixel_map_present(*head, buf, n)
        return buf.raw[:n]

    @staticmethod
    def toPpm(progressIncrement: Callable[[float], None], image: "Image", path: str) -> str:
        """ImageOutput.toPpm = resume (ImageOutput.fs:131-161, 205): force the image and spill it as `<row>,<col>\\nRGB` records."""
        px = Image.render(image)
        with open(path, "wb") as f:
            f.write(_format_host(lib.rt_format_pixel_map, px))
        for _ in range(px.shape[0]):
            progressIncrement(1.0)
        return path

    @staticmethod
    def readPixelMap(path: str, numRows: int, numCols: int):
        """ImageOutput.readPixelMap (ImageOutput.fs:68-113) -> (pixels [rows, cols, 3] uint8, present [rows, cols] bool)."""
        data = open(path, "rb").read()
        rgb = np.zeros((numRows, numCols, 3), np.uint8)
        present = np.zeros((numRows, numCols), np.uint8)
        _size(lib.rt_parse_pixel_map(data, len(data), numRows, numCols, _u8(rgb), _u8(present)))
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
        for _ in range(_write_image("ppm", gammaCorrect, pixels, output)):
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
        cap = _size(lib.rt_png_max_bytes(rows, cols))
        buf = np.empty(cap, np.uint8)
        n = _size(lib.rt_format_png(_u8(px), rows, cols, int(bool(gammaCorrect)), buf.ctypes.data, cap))
        return buf[:n].tobytes()

    @staticmethod
    def formatDevice(gammaCorrect: bool, pixels):
        """rt_format_png_device on torch.cuda.current_stream(), without waiting for the device: (data, length) -- a uint8 tensor of
        rt_png_max_bytes(rows, cols) bytes whose first `length` (an int64 tensor) are the file; the rest is not written."""
        return _format_device(lib.rt_png_max_bytes, lib.rt_format_png_device, gammaCorrect, pixels)

    @staticmethod
    def write(gammaCorrect: bool, incrementProgress: Callable[[float], None], pixels, output: str) -> None:
        """Png.write (ImageOutput.fs:216-251).  A torch tensor on a GPU is encoded there (rt_write_png_device, on
        torch.cuda.current_stream()); a numpy array takes rt_write_png.  Progress as the reference counts it: once per pixel but a row's
        last (ImageOutput.fs:230-233), once per row but the last (:239-241) -- rows * cols - 1 in all."""
        for _ in range(_write_image("png", gammaCorrect, pixels, output) - 1):
            incrementProgress(1.0)

    @staticmethod
    def formatViewsDevice(gammaCorrect: bool, pixels):
        """rt_format_png_views_device on torch.cuda.current_stream(), without waiting for the device: the K images of a contiguous uint8
        tensor [K, rows, cols, 3] on a GPU (renderViews' rgb) encoded in the four launches one image takes -> (data, offsets): a uint8
        tensor of rt_png_views_max_bytes(K, rows, cols) bytes and an int64 tensor of K + 1; file v is data[offsets[v]:offsets[v + 1]],
        byte for byte Png.format of image v, and nothing at or beyond offsets[K] is written."""
        t = _views_tensor(pixels)
        torch = _torch()
        k, rows, cols = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
        cap = _size(lib.rt_png_views_max_bytes(k, rows, cols))
        data = torch.empty(cap, dtype=torch.uint8, device=t.device)
        offsets = torch.empty(k + 1, dtype=torch.int64, device=t.device)
        check(lib.rt_format_png_views_device(t.device.index, t.data_ptr() if k else None, k, rows, cols, int(bool(gammaCorrect)), data.data_ptr() if cap else None,
                                             cap, offsets.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream, None))
        return data, offsets

    @staticmethod
    def formatViews(gammaCorrect: bool, pixels) -> List[bytes]:
        """The K files of a batch [K, rows, cols, 3].  A torch tensor on a GPU is encoded there (formatViewsDevice) and only the files are
        copied back; a numpy array is Png.format image by image on the host, which needs no GPU."""
        if _is_torch(pixels):
            data, offsets = Png.formatViewsDevice(gammaCorrect, pixels)
            at = offsets.cpu().tolist()
            files = data[: at[-1]].cpu().numpy().tobytes()
            return [files[a:b] for a, b in zip(at[:-1], at[1:])]
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        if px.ndim != 4 or px.shape[3] != 3:
            raise ValueError(f"pixels must have shape [K, rows, cols, 3], not {list(px.shape)}")
        return [Png.format(gammaCorrect, image) for image in px]

    @staticmethod
    def writeViews(gammaCorrect: bool, pixels, paths: Sequence[str]) -> None:
        """paths[v] = the PNG of image v of a batch [K, rows, cols, 3].  A torch tensor on a GPU goes through rt_write_png_views_device on
        torch.cuda.current_stream(): one encode and one copy for all files; a numpy array takes rt_write_png per image."""
        names = [str(p) for p in paths]
        if _is_torch(pixels):
            t = _views_tensor(pixels)
            k = int(t.shape[0])
            _one_path_per_view(names, k)
            check(lib.rt_write_png_views_device(_path_array(names), t.device.index, t.data_ptr() if k else None, k, int(t.shape[1]), int(t.shape[2]),
                                                int(bool(gammaCorrect)), _torch().cuda.current_stream(t.device).cuda_stream))
            return
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        if px.ndim != 4 or px.shape[3] != 3:
            raise ValueError(f"pixels must have shape [K, rows, cols, 3], not {list(px.shape)}")
        _one_path_per_view(names, px.shape[0])
        for image, name in zip(px, names):
            _write_image("png", gammaCorrect, image, name)


class LoadImage:
    """LoadImage.fromResource (RayTracing.App/LoadImage.fs:9-18): a baseline JPEG to the bitmap ParameterisedTexture.ofImage takes --
    [height, width, 3] uint8, rows top first.  The reference embeds its file as a resource and hands it to Skia; here the bytes or a path are
    given, and the decode is csrc/rt_jpeg.h's, bit for bit libjpeg's.  device=None: the first GPU when one is visible, the host decoder
    otherwise; device="host": the host decoder; an index: that GPU (RT_ERR_NO_DEVICE without one, never the host decoder instead).
    tensor=True: a torch uint8 tensor that stays on the GPU it was decoded on (decoded on torch.cuda.current_stream(), and waited for: the
    status of the entropy-coded data is the device's to find)."""

    @staticmethod
    def info(data: bytes) -> dict:
        """rt_jpeg_get_info: width, height, components, sampling ("grey", "4:4:4", "4:2:2", "4:2:0"), restart_interval, entropy_bytes."""
        i = A.rt_jpeg_info()
        data = bytes(data)
        check(lib.rt_jpeg_get_info(data, len(data), C.byref(i)))
        return {"width": i.width, "height": i.height, "components": i.components, "sampling": ("grey", "4:4:4", "4:2:2", "4:2:0")[i.sampling],
                "restart_interval": i.restart_interval, "entropy_bytes": i.entropy_bytes}

    @staticmethod
    def fromBytes(data: bytes, device=None, tensor: bool = False):
        data = bytes(data)
        i = LoadImage.info(data)
        shape = (i["height"], i["width"], 3)
        if device is None:
            device = 0 if tensor or lib.rt_device_count() > 0 else "host"
        if device == "host":
            if tensor:
                raise ValueError('tensor=True needs a GPU: device="host" gives a numpy array')
            out = np.empty(shape, np.uint8)
            check(lib.rt_decode_jpeg(data, len(data), out.ctypes.data, out.size))
            return out
        if lib.rt_device_count() < 1:
            raise RtError(A.RT_ERR_NO_DEVICE, "no HIP device visible: LoadImage on a device has no CPU fallback (device=\"host\" is the host decoder)")
        torch = _torch()
        where = torch.device("cuda", int(device))
        out = torch.empty(shape, dtype=torch.uint8, device=where)
        stats = A.rt_jpeg_stats()
        check(lib.rt_decode_jpeg_device(int(device), data, len(data), out.data_ptr(), out.numel(), torch.cuda.current_stream(where).cuda_stream, C.byref(stats)))
        return out if tensor else out.cpu().numpy()

    @staticmethod
    def fromFile(path: str, device=None, tensor: bool = False):
        with open(path, "rb") as f:
            return LoadImage.fromBytes(f.read(), device, tensor)


# ---- the output classes' shared pieces ----------------------------------------------------------------------------------
def _size(n: int) -> int:
    """A byte count of the library's, which is minus the error code where it refuses."""
    if n < 0:
        check(int(-n))
    return int(n)


def _format_host(fn, pixels, *args, spare: int = 0) -> bytes:
    """A host formatter's two calls: ask for the size, make a buffer of it (and `spare` bytes for a terminator), call again."""
    px = np.ascontiguousarray(pixels, dtype=np.uint8)
    head = (_u8(px), px.shape[0], px.shape[1]) + args
    n = _size(fn(*head, None, 0))
    buf = C.create_string_buffer(n + spare)
    fn(*head, buf, n + spare)
    return buf.raw[:n]


def _format_device(size_fn, format_fn, gammaCorrect: bool, pixels):
    """An image on a GPU to (bytes, length): a uint8 tensor of size_fn(rows, cols) bytes and an int64 tensor, both filled by format_fn on
    torch.cuda.current_stream() without waiting for the device."""
    t = _image_tensor(pixels)
    torch = _torch()
    rows, cols = int(t.shape[0]), int(t.shape[1])
    cap = _size(size_fn(rows, cols))
    data = torch.empty(cap, dtype=torch.uint8, device=t.device)
    length = torch.empty((), dtype=torch.int64, device=t.device)
    check(format_fn(t.device.index, t.data_ptr(), rows, cols, int(bool(gammaCorrect)), data.data_ptr(), cap, length.data_ptr(),
                    torch.cuda.current_stream(t.device).cuda_stream, None))
    return data, length


def _write_image(kind: str, gammaCorrect: bool, pixels, output: str) -> int:
    """rt_write_<kind> of a numpy array, rt_write_<kind>_device of a torch tensor on a GPU (on torch.cuda.current_stream()) -> rows * cols."""
    if _is_torch(pixels):
        t = _image_tensor(pixels)
        rows, cols = int(t.shape[0]), int(t.shape[1])
        check(getattr(lib, f"rt_write_{kind}_device")(str(output).encode(), t.device.index, t.data_ptr(), rows, cols, int(bool(gammaCorrect)),
                                                      _torch().cuda.current_stream(t.device).cuda_stream))
    else:
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        rows, cols = px.shape[0], px.shape[1]
        check(getattr(lib, f"rt_write_{kind}")(str(output).encode(), _u8(px), rows, cols, int(bool(gammaCorrect))))
    return rows * cols


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


# ---- BoundingBoxTree.make over caller-supplied boxes (BoundingBoxTree.fs:9-43) ----------------------------------------------------
def _tree_boxes(boxes) -> np.ndarray:
    b = np.asarray(boxes)
    if b.dtype != np.float64 or b.ndim != 2 or b.shape[1] != 6:
        raise ValueError(f"boxes must be float64 [n, 6] (minx, maxx, miny, maxy, minz, maxz), got {b.dtype} {tuple(b.shape)}")
    return np.ascontiguousarray(b)


def tree_make_host(boxes):
    """rt_tree_make_host: the host builder over boxes [n, 6] (minx, maxx, miny, maxy, minz, maxz); no device.  Returns (skip, prim, boxes,
    order): skip and prim [2n-1] int32 (prim: the input index of a Leaf's box, -1 for a Branch), the node boxes [2n-1, 6], and the
    depth-first leaf order [n]."""
    b = _tree_boxes(boxes)
    n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
    skip, prim, nb, order = np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6), np.float64), np.zeros(n, np.int32)
    check(lib.rt_tree_make_host(n, _f64(b), _i32(skip), _i32(prim), _f64(nb), _i32(order)))
    return skip, prim, nb, order


def tree_make(boxes, device: Optional[int] = None):
    """The same four arrays from the device build: a numpy array goes through rt_tree_make (on `device`, 0 by default) and comes back as
    arrays; a float64 torch tensor on a GPU through rt_tree_make_device on torch's current stream there, and comes back as tensors."""
    if not _is_torch(boxes):
        b = _tree_boxes(boxes)
        n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
        skip, prim, nb, order = np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6), np.float64), np.zeros(n, np.int32)
        check(lib.rt_tree_make(0 if device is None else int(device), n, _f64(b), _i32(skip), _i32(prim), _f64(nb), _i32(order)))
        return skip, prim, nb, order
    torch = _torch()
    if not boxes.is_cuda:
        raise ValueError(f"boxes must be on a GPU, got {boxes.device} (use a numpy array for the host route)")
    if boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 6:
        raise ValueError(f"boxes must be float64 [n, 6] (minx, maxx, miny, maxy, minz, maxz), got {boxes.dtype} {tuple(boxes.shape)}")
    where = boxes.device
    _tensor_device(where, device)
    b = boxes.contiguous()
    n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
    skip, prim = torch.empty(nn, dtype=torch.int32, device=where), torch.empty(nn, dtype=torch.int32, device=where)
    nb, order = torch.empty((nn, 6), dtype=torch.float64, device=where), torch.empty(n, dtype=torch.int32, device=where)
    check(lib.rt_tree_make_device(where.index, n, b.data_ptr(), skip.data_ptr(), prim.data_ptr(), nb.data_ptr(), order.data_ptr(),
                                  torch.cuda.current_stream(where).cuda_stream))
    return skip, prim, nb, order


# ---- the surface-area walk tree over caller-supplied boxes (csrc/rt_walk_plan.h) ----------------------------------------------------
def walk_tree_make_host(boxes):
    """rt_walk_tree_make_host: the host builder of the tree the device walks over boxes [n, 6] (minx, maxx, miny, maxy, minz, maxz); no
    device.  Returns (skip, prim, boxes): skip and prim [2n-1] int32 (prim: the input index of a Leaf's box, -1 for a Branch) and the node
    boxes [2n-1, 6]."""
    b = _tree_boxes(boxes)
    n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
    skip, prim, nb = np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6), np.float64)
    check(lib.rt_walk_tree_make_host(n, _f64(b), _i32(skip), _i32(prim), _f64(nb)))
    return skip, prim, nb


def walk_tree_make(boxes, device: Optional[int] = None):
    """The same three arrays from the device build: a numpy array goes through rt_walk_tree_make (on `device`, 0 by default) and comes back
    as arrays; a float64 torch tensor on a GPU through rt_walk_tree_make_device on torch's current stream there, and comes back as tensors."""
    if not _is_torch(boxes):
        b = _tree_boxes(boxes)
        n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
        skip, prim, nb = np.zeros(nn, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 6), np.float64)
        check(lib.rt_walk_tree_make(0 if device is None else int(device), n, _f64(b), _i32(skip), _i32(prim), _f64(nb)))
        return skip, prim, nb
    torch = _torch()
    if not boxes.is_cuda:
        raise ValueError(f"boxes must be on a GPU, got {boxes.device} (use a numpy array for the host route)")
    if boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 6:
        raise ValueError(f"boxes must be float64 [n, 6] (minx, maxx, miny, maxy, minz, maxz), got {boxes.dtype} {tuple(boxes.shape)}")
    where = boxes.device
    _tensor_device(where, device)
    b = boxes.contiguous()
    n, nn = b.shape[0], int(lib.rt_tree_nodes(b.shape[0]))
    skip, prim = torch.empty(nn, dtype=torch.int32, device=where), torch.empty(nn, dtype=torch.int32, device=where)
    nb = torch.empty((nn, 6), dtype=torch.float64, device=where)
    check(lib.rt_walk_tree_make_device(where.index, n, b.data_ptr(), skip.data_ptr(), prim.data_ptr(), nb.data_ptr(),
                                       torch.cuda.current_stream(where).cuda_stream))
    return skip, prim, nb


# ---- the two routes of a launching Scene call -------------------------------------------------------------------------
# Every entry point Scene._launch serves: NAME takes numpy arrays, NAME_device tensors on a GPU, and NAME_device's arguments are NAME's
# with `stream, options` in front of the trailing `stats` (tests/test_abi.py holds _lib.SIGNATURES to that).
_ROUTED = ("rt_hit_objects", "rt_trace_rays", "rt_render_footprints", "rt_render_footprints_extend", "rt_render_footprints_extend_map",
           "rt_render_pixels", "rt_render_pixels_extend", "rt_camera_hits", "rt_camera_paths", "rt_trace_paths", "rt_render_extend",
           "rt_render_extend_map")
# a buffer's kind -> its dtype's name (numpy's and torch's) and how an array of it is handed to the library
_KINDS = {"i32": ("int32", _i32), "u8": ("uint8", _u8), "f64": ("float64", _f64), "u32": ("uint32", _u32)}
_TYPED = {name: typed for name, typed in _KINDS.values()}


class _Arrays:
    """The array route: numpy buffers through the host entry point, on device 0 unless told otherwise; statistics always."""
    suffix = ""

    def __init__(self, device: Optional[int]):
        self.device = 0 if device is None else device

    def make(self, shape, kind: str) -> np.ndarray:
        return np.zeros(shape, _KINDS[kind][0])

    def ptr(self, a: Optional[np.ndarray]):
        return None if a is None else _TYPED[a.dtype.name](a)

    def tail(self, options) -> tuple:
        return ()


class _Tensors:
    """The tensor route: torch buffers on the GPU `where` through the _device entry point, on torch's current stream there."""
    suffix = "_device"

    def __init__(self, where, device: Optional[int] = None):
        _tensor_device(where, device)
        self.where, self.device = where, where.index

    def make(self, shape, kind: str):
        torch = _torch()
        return torch.empty(shape, dtype=getattr(torch, _KINDS[kind][0]), device=self.where)

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def tail(self, options) -> tuple:
        return _torch().cuda.current_stream(self.where).cuda_stream, _ref(options)


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _torch():
    import torch
    return torch


def _ref(x):
    return C.byref(x) if x is not None else None


def _tensor_device(where, device: Optional[int]) -> None:
    if device is not None and device != where.index:
        raise ValueError(f"device={device} but the tensors are on {where}")


def _flags(counters: bool) -> int:
    return A.RT_RENDER_COUNTERS if counters else 0


def _no_options(options, instead: str = "set_launch_config / set_park") -> None:
    if options is not None:
        raise ValueError(f"options apply to the device entry point (torch tensors); use {instead} for arrays")


def _shape_text(width: Optional[int]) -> str:
    return "[n]" if width is None else f"[n, {width}]"


def _is_list_shape(shape, width: Optional[int]) -> bool:
    return len(shape) == 1 if width is None else len(shape) == 2 and shape[1] == width


def _array_arg(a, name: str, kind: str, width: Optional[int]) -> np.ndarray:
    """A list argument of the array route, [n, width] or (width None) [n], made contiguous."""
    dtype = np.dtype(_KINDS[kind][0])
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{name} must be a numpy array or a torch tensor on a GPU, not {type(a).__name__}")
    if a.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype.name}, not {a.dtype}")
    if not _is_list_shape(a.shape, width):
        raise ValueError(f"{name} must have shape {_shape_text(width)}, not {list(a.shape)}")
    return np.ascontiguousarray(a)


def _tensor_arg(t, name: str, kinds: Sequence[str], width: Optional[int]):
    """A list argument of the tensor route (of one of `kinds`), made contiguous."""
    dtypes = [getattr(_torch(), _KINDS[k][0]) for k in kinds]
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must have dtype {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if not _is_list_shape(t.shape, width):
        raise ValueError(f"{name} must have shape {_shape_text(width)}, not {list(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a GPU (a numpy array takes the host entry point)")
    return t.contiguous()


def _route(x, name: str, kind: str, width: Optional[int], device: Optional[int], options, instead: str = "set_launch_config / set_park"):
    """The route of a call, chosen from its leading argument x, and x checked: (route, x made contiguous).  Arrays refuse options
    (`instead` names what to use), tensors a device= that is not theirs."""
    if _is_torch(x):
        t = _tensor_arg(x, name, (kind,), width)
        return _Tensors(t.device, device), t
    _no_options(options, instead)
    return _Arrays(device), _array_arg(x, name, kind, width)


def _pixel_list(pixels, n: Optional[int], tensors: bool, maxWidthCoord: int, maxHeightCoord: int, device: Optional[int], options):
    """The pixel list of cameraHits / cameraPaths: (route, the list or None, its count).  pixels=None stands for the frame's first n
    pixels (all of them by default), on the tensor route if `tensors`, there on `device` or torch's current one."""
    if pixels is not None and n is not None:
        raise ValueError("n applies to pixels=None")
    if pixels is not None:
        route, px = _route(pixels, "pixels", "i32", None, device, options, "set_launch_config")
        return route, px, px.shape[0]
    count = (2 * maxWidthCoord + 1) * (2 * maxHeightCoord + 1) if n is None else int(n)
    if tensors:
        torch = _torch()
        return _Tensors(torch.device("cuda", torch.cuda.current_device() if device is None else device)), None, count
    _no_options(options, "set_launch_config")
    if count < 0:
        raise ValueError("n must be >= 0")
    return _Arrays(device), None, count


def _lead(route, shape: tuple, slots: int) -> tuple:
    """The leading shape of a call's outputs.  More than INT32_MAX slots are refused by the library, so the array route, which would
    have to zero them first, makes empty buffers for that call."""
    return (0,) * len(shape) if not route.suffix and slots > 2**31 - 1 else shape


def _rng(route, rng, n: int):
    """The caller's generator states [n, 4] for n rays, copied for the call to advance (None: none given).  A tensor's may be uint32 or int32."""
    if rng is None:
        return None
    if route.suffix:
        if not _is_torch(rng):
            raise TypeError("rng must be a torch tensor when rays is one")
        g = _tensor_arg(rng, "rng", ("u32", "i32"), 4).clone()
        if g.shape[0] != n or g.device != route.where:
            raise ValueError("rng must be [n, 4] on the rays' device")
    else:
        g = _array_arg(rng, "rng", "u32", 4).copy()
        if g.shape[0] != n:
            raise ValueError("rng must be [n, 4] for n rays")
    return g


def _targets(route, targets, shape: tuple, text: str, owner: str, prefix: str = ""):
    """The int32 targets of a map extension, `text` their shape in words; a tensor must be contiguous and on the device of `owner`."""
    if route.suffix:
        if (not _is_torch(targets) or targets.dtype != _torch().int32 or tuple(targets.shape) != shape or targets.device != route.where
                or not targets.is_contiguous()):
            raise ValueError(f"{prefix}targets must be a contiguous int32 tensor {text} on {owner}")
        return targets
    if not isinstance(targets, np.ndarray) or targets.dtype != np.int32 or targets.shape != shape:
        raise ValueError(f"{prefix}targets must be an int32 array {text}")
    return np.ascontiguousarray(targets)


def _frame(accum, cols: int, device: Optional[int], options, mapped: bool = False, targets=None):
    """The buffer a frame extension continues, [n_rows, cols, 4] int32, and (mapped) its targets [n_rows, cols]: (route, buffer, targets).
    An array is copied and the copy extended; a tensor is extended in place, so it must be contiguous already."""
    if _is_torch(accum):
        if accum.dtype != _torch().int32 or accum.dim() != 3 or tuple(accum.shape[1:]) != (cols, 4) or not accum.is_cuda or not accum.is_contiguous():
            raise ValueError(f"accum must be a contiguous int32 tensor [n_rows, {cols}, 4] on a GPU")
        route, out = _Tensors(accum.device), accum
    else:
        _no_options(options)
        if not isinstance(accum, np.ndarray) or accum.dtype != np.int32 or accum.ndim != 3 or accum.shape[1:] != (cols, 4):
            raise ValueError(f"accum must be an int32 array [n_rows, {cols}, 4] or such a tensor on a GPU")
        route, out = _Arrays(device), np.array(accum, dtype=np.int32, order="C")
    tg = _targets(route, targets, (out.shape[0], cols), f"[n_rows, {cols}]", "accum's device") if mapped else None
    if route.suffix:
        _tensor_device(route.where, device)  # (after the targets, as it always was)
    return route, out, tg


def _list_accum(route, accum, n: int, what: str, entries: str, owner: str):
    """The buffer an extension of n list entries continues, [n, 4] int32: an array is copied, a tensor extended in place.  `what` names
    the argument, `entries` what the list holds, `owner` the device a tensor must be on."""
    if route.suffix:
        if not _is_torch(accum) or accum.dtype != _torch().int32 or tuple(accum.shape) != (n, 4) or accum.device != route.where or not accum.is_contiguous():
            raise ValueError(f"{what}: accum must be a contiguous int32 tensor [n, 4] on {owner}")
        return accum
    out = np.array(_array_arg(accum, what.split("=")[0] + "'s accum", "i32", 4), order="C")
    if out.shape[0] != n:
        raise ValueError(f"{what}: accum must be [n, 4] for n {entries}")
    return out


def _list_extension(route, n: int, extend, extend_map, entries: str, owner: str):
    """What extend= / extend_map= make of a list call: (the entry point's suffix, the arguments in front of accum, accum)."""
    if extend is not None:
        accum, done = extend
        return "_extend", (done,), _list_accum(route, accum, n, "extend=(accum, samplesDone)", entries, owner)
    if extend_map is not None:
        accum, targets = extend_map
        accum = _list_accum(route, accum, n, "extend_map=(accum, targets)", entries, owner)
        targets = _targets(route, targets, (n,), "[n]", owner, "extend_map=(accum, targets): ")
        return "_extend_map", (route.ptr(targets),), accum
    return "", (), route.make((n, 4), "i32")


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


def _views_tensor(t):
    """A batch of images [K, rows, cols, 3] uint8 for the batch's device output entry points."""
    if t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"pixels must have shape [K, rows, cols, 3], not {list(t.shape)}")
    return _bytes_tensor(t)


def _one_path_per_view(paths, k: int) -> None:
    if len(paths) != k:
        raise ValueError(f"paths must hold one path per view ({k}), not {len(paths)}")


def _path_array(paths):
    """const char *const paths[] for the batch's file-writing entry points (never an empty array: the library looks at the pointer)."""
    return (C.c_char_p * max(len(paths), 1))(*[p.encode() for p in paths])
