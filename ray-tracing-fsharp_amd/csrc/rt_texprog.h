// rt_texprog.h -- texture programs: Texture.Arbitrary of (Point -> Pixel) and ParameterisedTexture.Arbitrary of (float -> float -> Texture)
// (Texture.fs:8,24) as a small postfix expression program over a stack of doubles.  Plain C++17 for host and device (no HIP calls), like
// rt_texture_plan.h: the host check (rt_scene.h, rt_texture_program_check), the kernels (rt_device.h) and tests/c/texprog_table.cpp
// include this one definition; nothing else evaluates a program.
//
// Encoding (n bytes, little-endian; a scene stores it in its texel blob on a 16-byte boundary):
//   byte 0      n_instr, 1..64          byte 1   n_const, 0..32          bytes 2, 3   zero
//   bytes 4 ..  n_instr instructions of two bytes {opcode, operand}; operand is the constant's index for CONST and 0 otherwise
//   (zero bytes up to the next multiple of 8)
//   then        n_const IEEE doubles
// n is exactly const_offset(n_instr) + 8 * n_const.  There are no branches and no loops, so the stack depth in front of and behind every
// instruction is known from the text alone: check() follows it, refuses a pop from an empty stack and a depth above 8, and wants exactly
// three values -- red, green, blue, pushed in that order -- at the end.  eval() may therefore keep the stack in eight registers that it
// shifts on push and pop, without a bound to test.
//
// Constants must be finite (the choice the issue left open): a NaN's payload and sign are not portable text, and infinities and NaNs
// that a program wants it can compute (1/0, 0/0).
//
// Every operation is one IEEE double operation, unfused (the build has -ffp-contract=off), or rt_trig.h's correctly rounded sine:
//   ADD SUB MUL DIV NEG ABS SQRT FLOOR  as IEEE 754 has them
//   MIN, MAX   a < b ? a : b  and  a > b ? a : b   (a: pushed first): b when either is a NaN or the two compare equal (+0 and -0)
//   LT, LE     a < b, a <= b as 1.0 or 0.0 (false with a NaN)
//   FLT        Float.compare a b = Less (Float.fs:90-96): !(|a - b| < 1e-8) && a < b, as 1.0 or 0.0
//   SELECT     c, a, b pushed in this order: c != 0.0 ? a : b (a NaN c selects a)
//   SIN        rtt::cr_sin(a) for |a| < 2^20, NaN for every other argument (beyond 2^20 cr_sin falls back to the C library)
// Output: to_byte() of the three results, packed r | g << 8 | b << 16.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h> /* (a host-only hipcc build of a test program: rt_trig.h wants the attributes) */
#endif
#include "rt_trig.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTXP_HD __host__ __device__ __forceinline__
#else
#define RTXP_HD static inline
#endif

#define RTXP_MAX_INSTR 64
#define RTXP_MAX_CONST 32
#define RTXP_MAX_DEPTH 8
#define RTXP_TOL 0.00000001 /* Float.fs:82 */

namespace rtxp {

enum Op : uint8_t {
    OP_U = 0, OP_V, OP_PX, OP_PY, OP_PZ, OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_ABS, OP_SQRT, OP_FLOOR, OP_MIN, OP_MAX, OP_LT,
    OP_LE, OP_FLT, OP_SELECT, OP_SIN, OP_COUNT
};
enum Reason : int {
    OK = 0, UNKNOWN_OPCODE, CONST_RANGE, UNDERFLOW, TOO_DEEP, RESULTS, TOO_LONG, NONFINITE_CONST, BAD_SIZE, REASON_COUNT
};
static inline const char *reason_text(int r) {
    switch (r) {
    case OK: return "ok";
    case UNKNOWN_OPCODE: return "unknown opcode";
    case CONST_RANGE: return "constant index out of range";
    case UNDERFLOW: return "stack underflow";
    case TOO_DEEP: return "stack depth above 8";
    case RESULTS: return "not exactly three results";
    case TOO_LONG: return "too long (at most 64 instructions and 32 constants)";
    case NONFINITE_CONST: return "non-finite constant";
    case BAD_SIZE: return "byte count does not match the header";
    default: return "?";
    }
}

// values popped by an opcode (every opcode pushes one)
RTXP_HD int arity(int op) { return op <= OP_CONST ? 0 : (op == OP_NEG || op == OP_ABS || op == OP_SQRT || op == OP_FLOOR || op == OP_SIN) ? 1 : op == OP_SELECT ? 3 : 2; }
RTXP_HD size_t const_offset(size_t n_instr) { return (4u + 2u * n_instr + 7u) & ~(size_t) 7u; }
RTXP_HD size_t program_bytes(size_t n_instr, size_t n_const) { return const_offset(n_instr) + 8u * n_const; }

// The check.  Reads bytes[0, n) only.  *where (may be null): the instruction (or, for NONFINITE_CONST, the constant) the reason is about, -1
// for a reason about the whole program.
static inline int check(const uint8_t *bytes, size_t n, int *where = nullptr) {
    int dummy;
    int &at = where ? *where : dummy;
    at = -1;
    if (!bytes || n < 4u) return BAD_SIZE;
    const size_t ni = bytes[0], nc = bytes[1];
    if (ni > RTXP_MAX_INSTR || nc > RTXP_MAX_CONST) return TOO_LONG;
    if (ni == 0u) return RESULTS;
    if (bytes[2] != 0u || bytes[3] != 0u || n != program_bytes(ni, nc)) return n > program_bytes(RTXP_MAX_INSTR, RTXP_MAX_CONST) ? TOO_LONG : BAD_SIZE;
    for (size_t b = 4u + 2u * ni; b < const_offset(ni); ++b)
        if (bytes[b] != 0u) return BAD_SIZE;
    int depth = 0;
    for (size_t i = 0; i < ni; ++i) {
        const int op = bytes[4u + 2u * i], arg = bytes[5u + 2u * i];
        at = (int) i;
        if (op >= OP_COUNT) return UNKNOWN_OPCODE;
        if (op == OP_CONST ? (size_t) arg >= nc : arg != 0) return CONST_RANGE;
        if (depth < arity(op)) return UNDERFLOW;
        depth += 1 - arity(op);
#ifndef RTXP_MUTANT_NO_DEPTH_CHECK
        if (depth > RTXP_MAX_DEPTH) return TOO_DEEP;
#endif
    }
    at = -1;
    if (depth != 3) return RESULTS;
    for (size_t k = 0; k < nc; ++k) {
        uint64_t w;
        memcpy(&w, bytes + const_offset(ni) + 8u * k, 8);
        if (((w >> 52) & 0x7FFu) == 0x7FFu) { at = (int) k; return NONFINITE_CONST; }
    }
    return OK;
}

// F#'s `byte v` for a value in range, and the stated rule outside it: NaN -> 0; otherwise clamp to [INT32_MIN, INT32_MAX], truncate toward
// zero, the low 8 bits of the two's-complement value.  No out-of-range double -> int conversion is made (undefined on the host, saturating
// on the device).  For v = x * 255.0 with x in [0, 1] this is ramp_byte (rt_device.h).
RTXP_HD uint32_t to_byte(double v) {
    if (!(v == v)) return 0u;
#ifndef RTXP_MUTANT_NO_CLAMP
    if (v >= 2147483647.0) return 0xFFu;  // INT32_MAX & 0xFF
    if (v <= -2147483648.0) return 0x00u; // INT32_MIN & 0xFF
#endif
    return ((uint32_t) (int32_t) v) & 0xFFu;
}

RTXP_HD uint32_t rd16(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint16_t *) p; // (a scene's program starts on a 16-byte boundary; instructions are 2 bytes from byte 4 on)
#else
    return (uint32_t) p[0] | ((uint32_t) p[1] << 8);
#endif
}
RTXP_HD double rd_f64(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const double *) p; // (constants start on a multiple of 8)
#else
    double d;
    memcpy(&d, p, 8);
    return d;
#endif
}

// Runs a program that check() accepted; (u, v): interpret's (x, y); (px, py, pz): the strike point.  Returns r | g << 8 | b << 16.
// The stack: s0 is the top.  A push moves every register one down, a pop one up -- eight named registers and no array, so that the device
// keeps them in VGPRs (an array indexed at run time would live in scratch memory).
RTXP_HD uint32_t eval(const uint8_t *prog, double u, double v, double px, double py, double pz) {
    const uint32_t ni = prog[0];
    const uint8_t *consts = prog + const_offset(ni);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    for (uint32_t i = 0; i < ni; ++i) {
        const uint32_t w = rd16(prog + 4u + 2u * i);
        const uint32_t op = w & 0xFFu, arg = w >> 8;
        // a: the operand pushed first of a binary operation (below the top), b: the top
        const double a = s1, b = s0;
        double r = 0.0;
        switch (op) {
        case OP_U: r = u; break;
        case OP_V: r = v; break;
        case OP_PX: r = px; break;
        case OP_PY: r = py; break;
        case OP_PZ: r = pz; break;
        case OP_CONST: r = rd_f64(consts + 8u * arg); break;
        case OP_ADD: r = a + b; break;
        case OP_SUB: r = a - b; break;
        case OP_MUL: r = a * b; break;
        case OP_DIV: r = a / b; break;
        case OP_NEG: r = -b; break;
        case OP_ABS: r = __builtin_fabs(b); break;
        case OP_SQRT: r = sqrt(b); break;
        case OP_FLOOR: r = floor(b); break;
        case OP_MIN: r = a < b ? a : b; break;
        case OP_MAX: r = a > b ? a : b; break;
        case OP_LT: r = a < b ? 1.0 : 0.0; break;
        case OP_LE: r = a <= b ? 1.0 : 0.0; break;
        case OP_FLT: r = (!(__builtin_fabs(a - b) < RTXP_TOL) && a < b) ? 1.0 : 0.0; break;
#ifdef RTXP_MUTANT_SELECT_ORDER
        case OP_SELECT: r = s2 != 0.0 ? s0 : s1; break;
#else
        case OP_SELECT: r = s2 != 0.0 ? s1 : s0; break; // c = s2, a = s1, b = s0
#endif
        default: r = __builtin_fabs(b) < RTT_TRIG_MAX ? rtt::cr_sin(b) : __builtin_nan(""); break; // OP_SIN
        }
        const int pops = arity((int) op);
        if (pops == 0) { s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; }
        else if (pops == 2) { s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7; }
        else if (pops == 3) { s1 = s3; s2 = s4; s3 = s5; s4 = s6; s5 = s7; }
        s0 = r;
    }
    return to_byte(s2) | (to_byte(s1) << 8) | (to_byte(s0) << 16);
}

} // namespace rtxp
