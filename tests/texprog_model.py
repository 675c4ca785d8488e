"""A numpy model of texture programs (csrc/rt_texprog.h), written from the rules in DESIGN.md "Texture programs" and not from the
header: (u, v) from oracle.plane_map_inverse, the sine from the oracle's correctly rounded one (oracle.arith(8, ...)), everything
else one numpy double operation per instruction.  tests/test_texprog_model.py holds it to the compiled C++ eval on the CPU and shows that
each of three mutants of it is caught; tests/test_gpu_texprog.py holds the device to it.  Also the program families both share."""
import numpy as np

import oracle
from ray_tracing_fsharp_amd import texprog as T

TRIG_MAX = 2.0 ** 20
MUTANTS = ("min_commutative_nan", "byte_by_rounding", "flt_without_band")


def to_byte(v, mutant=None):
    """NaN -> 0; otherwise clamp to [INT32_MIN, INT32_MAX], truncate toward zero, low 8 bits of the two's-complement value."""
    v = np.asarray(v, np.float64)
    nan = np.isnan(v)
    c = np.clip(np.where(nan, 0.0, v), -2147483648.0, 2147483647.0)
    c = np.rint(c) if mutant == "byte_by_rounding" else np.trunc(c)
    return np.where(nan, 0, c.astype(np.int64) & 0xFF).astype(np.uint8)


def cr_sin(a):
    a = np.asarray(a, np.float64)
    ok = np.abs(a) < TRIG_MAX  # (false for NaN)
    out = np.full(a.shape, np.nan)
    if ok.any():
        out[ok] = oracle.arith(8, np.ascontiguousarray(a[ok]))
    return out


def uv_of(radius, centre, points):
    """interpret = Sphere.planeMapInverse radius centre, point by point, from the oracle."""
    return np.array([oracle.plane_map_inverse(float(radius), tuple(float(c) for c in centre), tuple(float(x) for x in p)) for p in points]).reshape(-1, 2)


def run(program: bytes, u, v, points, mutant=None):
    """-> [n, 3] uint8: the program's colour at every (u[i], v[i], points[i])."""
    ins, consts = T.decode(program)
    u, v, points = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(points, np.float64).reshape(-1, 3)
    n = len(u)
    stack = []
    with np.errstate(all="ignore"):
        for name, arg in ins:
            if name in ("U", "V", "PX", "PY", "PZ"):
                stack.append({"U": u, "V": v, "PX": points[:, 0], "PY": points[:, 1], "PZ": points[:, 2]}[name].copy())
                continue
            if name == "CONST":
                stack.append(np.full(n, consts[arg]))
                continue
            if T.ARITY[name] == 1:
                b = stack.pop()
                r = {"NEG": lambda: -b, "ABS": lambda: np.abs(b), "SQRT": lambda: np.sqrt(b), "FLOOR": lambda: np.floor(b), "SIN": lambda: cr_sin(b)}[name]()
            elif T.ARITY[name] == 2:
                b = stack.pop()
                a = stack.pop()
                if name == "MIN":
                    r = np.fmin(a, b) if mutant == "min_commutative_nan" else np.where(a < b, a, b)
                elif name == "MAX":
                    r = np.where(a > b, a, b)
                elif name == "LT":
                    r = np.where(a < b, 1.0, 0.0)
                elif name == "LE":
                    r = np.where(a <= b, 1.0, 0.0)
                elif name == "FLT":  # Float.compare a b = Less (Float.fs:90-96)
                    band = np.zeros(n, bool) if mutant == "flt_without_band" else np.abs(a - b) < 1e-8
                    r = np.where(~band & (a < b), 1.0, 0.0)
                else:
                    r = {"ADD": lambda: a + b, "SUB": lambda: a - b, "MUL": lambda: a * b, "DIV": lambda: a / b}[name]()
            else:  # SELECT: c, a, b pushed in this order
                b = stack.pop()
                a = stack.pop()
                c = stack.pop()
                r = np.where(c != 0.0, a, b)
            stack.append(np.asarray(r, np.float64))
    assert len(stack) == 3
    return np.stack([to_byte(s, mutant) for s in stack], axis=-1)


def colour_at(program, radius, centre, points, mutant=None):
    uv = uv_of(radius, centre, points)
    return uv, run(program, uv[:, 0], uv[:, 1], points, mutant)


# ---- the program family both the CPU and the GPU tests evaluate --------------------------------------------------------------------------
def raw(instructions, constants=()):
    """Bytes from (opcode name, operand) pairs: for programs the expression compiler would not write."""
    return T.encode([(T.OP[name], arg) for name, arg in instructions], list(constants))


def family():
    """name -> program bytes.  Every opcode; exactly 64 instructions; depth exactly 8; SIN at 0, -0.0, just below and at 2^20, inf and NaN;
    DIV by zero; SQRT of a negative; bytes that wrap; the three mutants' witnesses (a NaN as MIN's second operand, fractions above .5,
    differences inside the 1e-8 band)."""
    U, V, PX, PY, PZ = T.U, T.V, T.PX, T.PY, T.PZ
    out = {}
    out["ramp"] = T.compile_program(U * 255.0, V * 255.0, 77.0)
    out["arith"] = T.compile_program((U + V) * 127.5, T.abs(PX - PY) * 100.0, -(PZ / (U - 0.5)))
    out["roots"] = T.compile_program(T.sqrt(U - 0.5) * 255.0, T.floor(V * 10.0) * 25.5, T.sqrt(T.abs(PX)) * 200.0)
    nan = T.sqrt(U - 2.0)  # always NaN
    out["minmax"] = T.compile_program(T.minimum(U * 300.0, nan) + 5.0, T.minimum(nan, V * 300.0), T.maximum(T.maximum(nan, PX * 100.0), -PY * 0.0))
    out["compare"] = T.compile_program(T.lt(U, V) * 255.0, T.le(T.floor(U * 4.0), T.floor(V * 4.0)) * 200.0 + T.lt(nan, U) * 55.0,
                                       T.flt(T.sin(40.0 * U) * T.sin(40.0 * V), 0.0) * 255.0)
    out["band"] = T.compile_program(T.flt(U, U + 5e-9) * 255.0, T.flt(U, U + 2e-8) * 255.0, T.flt(V * 1e-9, 4e-9) * 255.0)
    out["select"] = T.compile_program(T.select(T.lt(U, 0.5), 10.0, 20.0), T.select(nan, 30.0, 40.0), T.select(V - V, 50.0, T.select(-0.0, 60.0, 70.0)))
    out["sines"] = T.compile_program(T.sin(0.0) + T.sin(-0.0) + T.sin(U * 6.0) * 127.0 + 128.0, T.sin((1.0 - U * 2.0 ** -30) * TRIG_MAX) * 127.0 + 128.0,
                                     T.select(T.lt(V, 0.5), T.sin(U * TRIG_MAX), T.sin(1.0 / (V - V))) + T.sin(nan))
    out["sin_edges"] = T.compile_program(T.sin(TRIG_MAX) + 7.0, T.sin(np.nextafter(TRIG_MAX, 0.0)) * 100.0 + 100.0, T.sin(-1.0 / (U - U)) + 9.0)
    out["div0"] = T.compile_program(1.0 / (U - U), -1.0 / (V - V), (U - U) / (V - V))
    out["wrap"] = T.compile_program(U * 1000.0, -V * 1000.0, PX * 1e12 + U * 3e9)
    out["rounding"] = T.compile_program(U * 255.0 + 0.75, V * 10.0 + 0.5, 0.999999 + T.floor(U * 3.0))
    # depth exactly 8: red and green are on the stack while blue = (2 + (U + (V + (U + (V + PX))))) * 20 holds six more before its first ADD
    out["depth8"] = raw([("CONST", 0), ("CONST", 0), ("CONST", 1), ("U", 0), ("V", 0), ("U", 0), ("V", 0), ("PX", 0)] + [("ADD", 0)] * 5 + [("CONST", 2), ("MUL", 0)],
                        (0.0, 2.0, 20.0))
    # exactly 64 instructions: red = U with 28 (CONST, ADD) behind it, scaled; green, blue short
    ins = [("U", 0)] + [("CONST", 0), ("ADD", 0)] * 28 + [("CONST", 1), ("MUL", 0)] + [("V", 0), ("CONST", 2), ("MUL", 0)] + [("CONST", 3), ("NEG", 0)]
    out["len64"] = raw(ins, (0.125, 50.0, 255.0, 3.0))
    assert len(ins) == 64
    return out


def depth_of(program: bytes) -> int:
    d = m = 0
    for name, _ in T.decode(program)[0]:
        d += 1 - T.ARITY[name]
        m = max(m, d)
    return m


def seam_points(rng, radius, centre, n):
    """Points of the map sphere: uniform, the seam (u next to 0 and 1), the poles, and the axis points with both signs of zero."""
    import texture_cases as tc
    u, v = tc.seam_uv(rng, n)
    return np.concatenate([tc.plane_map(radius, centre, u, v), np.asarray(centre) + tc.axis_points(radius)])
