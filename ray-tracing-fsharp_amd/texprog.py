"""Texture programs: the expression language of ParameterisedTexture.Program / Texture.Program and its compiler to the bytes of
csrc/rt_texprog.h (the definition: encoding, check, evaluation).

    from ray_tracing_fsharp_amd.texprog import U, V, PX, PY, PZ, sin, floor, sqrt, abs, minimum, maximum, lt, le, flt, select
    stripes = select(lt(floor(U * 10.0) - 2.0 * floor(U * 5.0), 0.5), 255.0, 0.0)

An expression is a tree; `compile_program(red, green, blue)` writes the three trees in postfix, left operand first, sharing equal
constants, and has the library check the result (rt_texture_program_check): a tree that needs more than 8 stack slots, more than 64
instructions or 32 constants is refused there, with the library's text.  Every operation is one IEEE double operation or the correctly
rounded sine; a channel's value becomes a byte as F#'s `byte` does (NaN -> 0, clamped to int32, truncated, low 8 bits)."""
import builtins
import struct
from typing import Sequence, Tuple, Union

OPCODES = ("U", "V", "PX", "PY", "PZ", "CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "FLOOR", "MIN", "MAX", "LT", "LE", "FLT",
           "SELECT", "SIN")
OP = {name: i for i, name in enumerate(OPCODES)}
ARITY = {name: 0 for name in OPCODES[:6]}
ARITY.update({name: 1 for name in ("NEG", "ABS", "SQRT", "FLOOR", "SIN")})
ARITY.update({name: 2 for name in ("ADD", "SUB", "MUL", "DIV", "MIN", "MAX", "LT", "LE", "FLT")})
ARITY["SELECT"] = 3
MAX_INSTR, MAX_CONST, MAX_DEPTH = 64, 32, 8


class NotAnExpression(TypeError):
    """Something that is no texture expression was used as one (a string, a truth test of an expression, ...)."""


class Expr:
    """A node: (op name, operands) or ("CONST", value)."""
    __slots__ = ("op", "args", "value")

    def __init__(self, op: str, args: Tuple["Expr", ...] = (), value: float = 0.0):
        self.op, self.args, self.value = op, tuple(args), float(value)

    def __add__(self, o): return Expr("ADD", (self, lift(o)))
    def __radd__(self, o): return Expr("ADD", (lift(o), self))
    def __sub__(self, o): return Expr("SUB", (self, lift(o)))
    def __rsub__(self, o): return Expr("SUB", (lift(o), self))
    def __mul__(self, o): return Expr("MUL", (self, lift(o)))
    def __rmul__(self, o): return Expr("MUL", (lift(o), self))
    def __truediv__(self, o): return Expr("DIV", (self, lift(o)))
    def __rtruediv__(self, o): return Expr("DIV", (lift(o), self))
    def __neg__(self): return Expr("NEG", (self,))
    def __abs__(self): return Expr("ABS", (self,))

    def __bool__(self):
        raise NotAnExpression("a texture expression has no truth value: use select(lt(a, b), x, y) instead of `if` / `and` / `<`")

    def __float__(self):
        raise NotAnExpression("a texture expression is no number: use texprog.sin / sqrt / floor / abs, not math's")

    def _no_order(self, o):
        raise NotAnExpression("texture expressions are compared with lt(a, b), le(a, b) or flt(a, b), not with < and <=")
    __lt__ = __le__ = __gt__ = __ge__ = _no_order

    def __repr__(self):
        return f"{self.value!r}" if self.op == "CONST" else self.op if not self.args else f"{self.op}({', '.join(map(repr, self.args))})"


Operand = Union[Expr, float, int]


def lift(x: Operand) -> Expr:
    if isinstance(x, Expr):
        return x
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise NotAnExpression(f"a texture expression is built from U, V, PX, PY, PZ and numbers, not {type(x).__name__}")
    return Expr("CONST", value=float(x))


U, V, PX, PY, PZ = Expr("U"), Expr("V"), Expr("PX"), Expr("PY"), Expr("PZ")


def sin(a): return Expr("SIN", (lift(a),))
def floor(a): return Expr("FLOOR", (lift(a),))
def sqrt(a): return Expr("SQRT", (lift(a),))
def abs(a): return Expr("ABS", (lift(a),))  # noqa: A001  (the language's name)
def minimum(a, b): return Expr("MIN", (lift(a), lift(b)))
def maximum(a, b): return Expr("MAX", (lift(a), lift(b)))
def lt(a, b): return Expr("LT", (lift(a), lift(b)))
def le(a, b): return Expr("LE", (lift(a), lift(b)))
def flt(a, b): return Expr("FLT", (lift(a), lift(b)))
def select(c, a, b): return Expr("SELECT", (lift(c), lift(a), lift(b)))


def const_offset(n_instr: int) -> int:
    return (4 + 2 * n_instr + 7) & ~7


def encode(instructions: Sequence[Tuple[int, int]], constants: Sequence[float]) -> bytes:
    """The bytes of rt_texprog.h for (opcode, operand) pairs and constants; nothing is checked here."""
    head = bytes([len(instructions) & 0xFF, len(constants) & 0xFF, 0, 0]) + b"".join(bytes([op & 0xFF, arg & 0xFF]) for op, arg in instructions)
    return head + b"\0" * (const_offset(len(instructions)) - len(head)) + b"".join(struct.pack("<d", c) for c in constants)


def decode(program: bytes):
    """-> ([(opcode name, operand)], [constants]) of bytes that encode() wrote."""
    ni, nc = program[0], program[1]
    ins = [(OPCODES[program[4 + 2 * i]], program[5 + 2 * i]) for i in range(ni)]
    at = const_offset(ni)
    return ins, [struct.unpack_from("<d", program, at + 8 * k)[0] for k in range(nc)]


def compile_program(red: Operand, green: Operand, blue: Operand, check: bool = True) -> bytes:
    ins, consts, where = [], [], {}

    def emit(e: Expr):
        if e.op == "CONST":
            key = struct.pack("<d", e.value)  # (by bits: -0.0 and 0.0 are two constants)
            if key not in where:
                where[key] = len(consts)
                consts.append(e.value)
            ins.append((OP["CONST"], where[key]))
            return
        for a in e.args:
            emit(a)
        ins.append((OP[e.op], 0))

    for ch in (red, green, blue):
        emit(lift(ch))
    if len(ins) > 255 or len(consts) > 255:
        raise ValueError(f"texture program too long: {len(ins)} instructions, {len(consts)} constants (at most {MAX_INSTR} and {MAX_CONST})")
    program = encode(ins, consts)
    if check:
        check_program(program)
    return program


def check_program(program: bytes) -> None:
    """rt_texture_program_check: raises RtError(RT_ERR_INVALID_ARGUMENT) with the library's reason for bytes a scene would refuse."""
    from ._lib import check, lib
    check(lib.rt_texture_program_check(builtins.bytes(program), len(program)))
