"""Frames of texture programs that no existing texture kind expresses, rendered by tests/fsharp_literal.py with the closure each program
denotes, and recorded in tests/golden/texprog_cases.npz (the literal needs mpmath, which a GPU machine may not have).

    python tests/golden/make_texprog_cases.py        # rewrites texprog_cases.npz

tests/test_texprog_literal.py regenerates the frames on the CPU and compares; tests/test_gpu_texprog.py holds every device route to them.
The closure is written here from the rules of DESIGN.md "Texture programs" over Python floats, with the literal's own sine, square root and
Float.compare -- not from csrc/rt_texprog.h and not from the numpy model."""
import dataclasses
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]  # the repository (the package, the oracle) and tests/

import ray_tracing_fsharp_amd as rt  # noqa: E402
import scenes  # noqa: E402
import texprog_model as M  # noqa: E402
import texture_cases as tc  # noqa: E402
from ray_tracing_fsharp_amd import _abi as A  # noqa: E402
from ray_tracing_fsharp_amd import texprog as T  # noqa: E402

PATH = os.path.join(HERE, "texprog_cases.npz")
MAX_W, MAX_H, SPP, DEPTH, SEED = 4, 3, 12, 6, 21  # 9 x 7 px
NAN, INF = float("nan"), float("inf")


# ---- the closure a program denotes ---------------------------------------------------------------------------------------------------------
def fdiv(a, b):
    if b != 0.0:
        return a / b
    if a != a or b != b or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def ffloor(a):
    return a if (a != a or abs(a) == INF) else float(math.floor(a)) if a != 0.0 else a


def fbyte(v):
    """F#'s `byte v` in range; NaN -> 0; otherwise clamped to int32, truncated toward zero, the low 8 bits."""
    if v != v:
        return 0
    return int(max(-2147483648.0, min(2147483647.0, v))) & 0xFF


def closure_of(program, L):
    """(x, y) -> Texture.Arbitrary (point -> pixel), as ParameterisedTexture.Arbitrary takes it (Texture.fs:24)."""
    ins, consts = T.decode(program)

    def channels(x, y, p):
        s = []
        for name, arg in ins:
            if name in ("U", "V", "PX", "PY", "PZ"):
                s.append({"U": x, "V": y, "PX": p[0], "PY": p[1], "PZ": p[2]}[name])
            elif name == "CONST":
                s.append(consts[arg])
            elif name == "SELECT":
                b, a, c = s.pop(), s.pop(), s.pop()
                s.append(a if c != 0.0 else b)
            elif T.ARITY[name] == 1:
                b = s.pop()
                s.append(-b if name == "NEG" else abs(b) if name == "ABS" else L.fsqrt(b) if name == "SQRT" else ffloor(b) if name == "FLOOR" else
                         (L.fsin(b) if abs(b) < 1048576.0 else NAN))
            else:
                b, a = s.pop(), s.pop()
                s.append(a + b if name == "ADD" else a - b if name == "SUB" else a * b if name == "MUL" else fdiv(a, b) if name == "DIV" else
                         (a if a < b else b) if name == "MIN" else (a if a > b else b) if name == "MAX" else
                         (1.0 if a < b else 0.0) if name == "LT" else (1.0 if a <= b else 0.0) if name == "LE" else
                         (1.0 if L.f_compare(a, b) == "Less" else 0.0))
        return tuple(fbyte(v) for v in s)
    return lambda x, y: ("Arbitrary", lambda p: channels(x, y, p))


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------
def programs():
    """The model's family (every opcode, 64 instructions, depth 8, SIN's edges, DIV by zero, bytes that wrap) and three pictures: stripes
    along the strike point, rings, and a checker by floor parity instead of sin * sin."""
    U, V, PX, PY, PZ = T.U, T.V, T.PX, T.PY, T.PZ
    fam = dict(M.family())
    par = lambda e: e - 2.0 * T.floor(e / 2.0)  # noqa: E731
    fam["stripes"] = T.compile_program(T.select(T.lt(par(T.floor(PX * 6.0)), 0.5), 230.0, 30.0), T.abs(PY) * 200.0, 40.0 + T.minimum(T.maximum(PZ, -1.0), 1.0) * 30.0)
    fam["rings"] = T.compile_program(T.sin(T.sqrt(PX * PX + PZ * PZ) * 9.0) * 127.0 + 128.0, V * 255.0, T.le(U, 0.5) * 200.0)
    cell = par(T.floor(U * 16.0) + T.floor(V * 8.0))  # 0 or 1: a checker by floor parity
    fam["parity"] = T.compile_program(cell * 230.0 + 20.0, T.floor(V * 8.0) * 30.0 + 10.0, 200.0 - T.floor(U * 16.0) * 12.0)
    return fam


def scene_of(names, fam):
    """A row of spheres wearing the named programs (every texture-carrying style in turn), the last one below a Checkered, on a ground
    sphere that wears the parity checker, under a sky light."""
    PT, H, S = rt.ParameterisedTexture, rt.Hittable, rt.SphereStyle
    prog = lambda name: dataclasses.replace(PT.Program(1.0, 2.0, 3.0), program=fam[name])  # noqa: E731
    styles = [lambda t: S.LightSource(t), lambda t: S.LambertReflection(0.85, t), lambda t: S.PureReflection(0.9, t), lambda t: S.FuzzedReflection(0.85, t, 0.3),
              lambda t: S.Dielectric(0.9, t, 1.4, 0.6), lambda t: S.Glass(0.95, t, 1.5)]
    objs = []
    for i, name in enumerate(names):
        c = (2.2 * (i - (len(names) - 1) / 2.0), 0.0, 0.0)
        param = prog(name) if i + 1 < len(names) else PT.Checkered(prog(name), PT.Checkered(prog("parity"), PT.Colour(tc.colour_of(i)), 11.0), 7.0)
        objs.append(H.Sphere(rt.Sphere.make(styles[i % len(styles)](PT.toTexture((1.0, tc.P(*c)), param)), tc.P(*c), 1.0)))
    g = tc.P(0.0, -101.0, 0.0)
    objs.append(H.Sphere(rt.Sphere.make(S.LambertReflection(0.8, PT.toTexture((100.0, g), prog("parity"))), g, 100.0)))
    objs.append(tc.sky())
    span = 2.2 * len(names)
    cam = dataclasses.replace(rt.Camera.makeBasic(SPP, 1.0, 9.0 / 7.0, tc.P(0.0, 1.0, -span * 0.45), scenes.unit(0.0, -0.25, 1.0), rt.Vector.make(0.0, 1.0, 0.0)), BounceDepth=DEPTH)
    return objs, cam


def cases():
    """name -> (objects, camera); frames of 9 x 7 px, 12 samples, depth 6."""
    fam = programs()
    names = sorted(fam)
    return {f"row{k}": scene_of(names[k::6], fam) for k in range(6)}


def render_literal(objs, cam):
    import fsharp_literal as L
    import test_oracle_vs_literal as OL
    plain = OL.literal_param

    def param(t):
        return ("Arbitrary", closure_of(t.program, L)) if t.kind == A.RT_TEXTURE_PROGRAM else plain(t)
    OL.literal_param = param  # (Checkered children are converted through the module's name)
    try:
        return OL.literal_render(objs, cam, MAX_W, MAX_H, seed=SEED).astype(np.int32)
    finally:
        OL.literal_param = plain


def generate():
    return {name: render_literal(objs, cam) for name, (objs, cam) in cases().items()}


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print(PATH, os.path.getsize(PATH), "bytes")
