// texprog_table.cpp -- csrc/rt_texprog.h on the host: check over every reason, eval on programs whose values are known by hand, every
// program of at most three instructions checked or refused (and evaluated when accepted) without a fault, and the byte rule at its edges.
// Every program is a heap block of exactly its size, so that a read past it is the sanitizer's to find.  Stand-alone: built plainly,
// with -fsanitize=address,undefined, and once per deliberate fault of the header (RTXP_MUTANT_*), each of which must make it fail.
// Plain C++ (not a HIP translation unit: in the host pass of one rt_trig.h keeps stubs for the sine's tables).
// `texprog_table eval` reads "hexbytes u v px py pz" lines (doubles as 16 hex digits) and prints "r g b" per line: the numpy model's
// other side (tests/test_texprog_model.py).
#include "../../ray-tracing-fsharp_amd/csrc/rt_texprog.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK(%s) failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

using namespace rtxp;

struct Ins { int op, arg; };
struct Block { // exactly n bytes on the heap
    uint8_t *p; size_t n;
    Block(const std::vector<Ins> &ins, const std::vector<double> &consts, int extra = 0) {
        n = program_bytes(ins.size(), consts.size()) + (size_t) extra;
        p = (uint8_t *) malloc(n);
        memset(p, 0, n);
        p[0] = (uint8_t) ins.size(); p[1] = (uint8_t) consts.size();
        for (size_t i = 0; i < ins.size(); ++i) { p[4 + 2 * i] = (uint8_t) ins[i].op; p[5 + 2 * i] = (uint8_t) ins[i].arg; }
        for (size_t k = 0; k < consts.size(); ++k) memcpy(p + const_offset(ins.size()) + 8 * k, &consts[k], 8);
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
};
static int why(const std::vector<Ins> &ins, const std::vector<double> &c, int *where = nullptr) { Block b(ins, c); return check(b.p, b.n, where); }
static uint32_t run(const std::vector<Ins> &ins, const std::vector<double> &c, double u = 0.25, double v = 0.75, double x = 1.0, double y = -2.0, double z = 3.0) {
    Block b(ins, c);
    CHECK(check(b.p, b.n) == OK);
    return eval(b.p, u, v, x, y, z);
}
static uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

static void stage_check() {
    int at = 0;
    const std::vector<Ins> three = {{OP_U, 0}, {OP_V, 0}, {OP_PX, 0}};
    CHECK(why(three, {}) == OK);
    CHECK(why({{OP_U, 0}, {OP_V, 0}, {OP_COUNT, 0}}, {}, &at) == UNKNOWN_OPCODE && at == 2);
    CHECK(why({{OP_U, 0}, {255, 0}, {OP_V, 0}}, {}, &at) == UNKNOWN_OPCODE && at == 1);
    CHECK(why({{OP_CONST, 1}, {OP_V, 0}, {OP_PX, 0}}, {1.0}, &at) == CONST_RANGE && at == 0);
    CHECK(why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {}, &at) == CONST_RANGE && at == 0);
    CHECK(why({{OP_U, 1}, {OP_V, 0}, {OP_PX, 0}}, {}, &at) == CONST_RANGE && at == 0); // an operand on an opcode that takes none
    CHECK(why({{OP_U, 0}, {OP_ADD, 0}}, {}, &at) == UNDERFLOW && at == 1);
    CHECK(why({{OP_NEG, 0}}, {}, &at) == UNDERFLOW && at == 0);
    CHECK(why({{OP_U, 0}, {OP_V, 0}, {OP_SELECT, 0}}, {}, &at) == UNDERFLOW && at == 2);
    std::vector<Ins> deep(9, Ins{OP_U, 0}); // nine pushes, then back down to three
    for (int i = 0; i < 6; ++i) deep.push_back({OP_ADD, 0});
    CHECK(why(deep, {}, &at) == TOO_DEEP && at == 8);
    std::vector<Ins> eight(8, Ins{OP_U, 0});
    for (int i = 0; i < 5; ++i) eight.push_back({OP_ADD, 0});
    CHECK(why(eight, {}) == OK); // depth exactly 8
    CHECK(why({{OP_U, 0}, {OP_V, 0}}, {}, &at) == RESULTS && at == -1);
    CHECK(why({{OP_U, 0}, {OP_V, 0}, {OP_PX, 0}, {OP_PY, 0}}, {}) == RESULTS);
    std::vector<Ins> l64 = three, l65;
    while (l64.size() < 64) l64.push_back({OP_NEG, 0});
    l65 = l64; l65.push_back({OP_NEG, 0});
    CHECK(why(l64, {}) == OK);
    CHECK(why(l65, {}) == TOO_LONG);
    CHECK(why(three, std::vector<double>(32, 1.0)) == OK);
    CHECK(why(three, std::vector<double>(33, 1.0)) == TOO_LONG);
    CHECK(why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {INFINITY}, &at) == NONFINITE_CONST && at == 0);
    CHECK(why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {1.0, -INFINITY}, &at) == NONFINITE_CONST && at == 1);
    CHECK(why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {NAN}) == NONFINITE_CONST);
    CHECK(why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {5e-324}) == OK && why({{OP_CONST, 0}, {OP_V, 0}, {OP_PX, 0}}, {-0.0}) == OK);
    { Block b(three, {}, 8); CHECK(check(b.p, b.n) == BAD_SIZE); }  // bytes behind the program
    { Block b(three, {1.0}); CHECK(check(b.p, b.n - 8) == BAD_SIZE && check(b.p, 3) == BAD_SIZE && check(b.p, 0) == BAD_SIZE && check(nullptr, 16) == BAD_SIZE); }
    { Block b(three, {}); b.p[2] = 1; CHECK(check(b.p, b.n) == BAD_SIZE); }
    { Block b(three, {}); b.p[10] = 1; CHECK(check(b.p, b.n) == BAD_SIZE); } // padding in front of the constants is zero
    { Block b({}, {}); CHECK(check(b.p, b.n) == RESULTS); }
    for (int r = 0; r < REASON_COUNT; ++r) CHECK(strcmp(reason_text(r), "?") != 0);
    puts("check ok");
}

static void stage_eval() {
    const double c255 = 255.0;
    CHECK(run({{OP_U, 0}, {OP_CONST, 0}, {OP_MUL, 0}, {OP_V, 0}, {OP_CONST, 0}, {OP_MUL, 0}, {OP_CONST, 1}}, {c255, 77.0}, 0.5, 1.0) == rgb(127, 255, 77));
    // inputs in their places: u v px | py pz, a - b with a pushed first
    CHECK(run({{OP_PX, 0}, {OP_PY, 0}, {OP_SUB, 0}, {OP_PZ, 0}, {OP_PY, 0}, {OP_DIV, 0}, {OP_NEG, 0}, {OP_V, 0}, {OP_U, 0}, {OP_SUB, 0}, {OP_CONST, 0}, {OP_MUL, 0}}, {100.0}) ==
          rgb(3, 1, 50));
    // SELECT: c, a, b in this order; a NaN c selects a; -0.0 selects b
    CHECK(run({{OP_CONST, 0}, {OP_CONST, 1}, {OP_CONST, 2}, {OP_SELECT, 0}, {OP_CONST, 3}, {OP_CONST, 1}, {OP_CONST, 2}, {OP_SELECT, 0}, {OP_CONST, 3}, {OP_NEG, 0}, {OP_SQRT, 0},
               {OP_CONST, 1}, {OP_CONST, 2}, {OP_SELECT, 0}},
              {1.0, 10.0, 20.0, 0.0}) == rgb(10, 20, 20)); // (sqrt(-0.0) = -0.0: b)
    CHECK(run({{OP_CONST, 0}, {OP_NEG, 0}, {OP_SQRT, 0}, {OP_CONST, 1}, {OP_CONST, 2}, {OP_SELECT, 0}, {OP_U, 0}, {OP_V, 0}}, {1.0, 10.0, 20.0}) == rgb(10, 0, 0)); // NaN c
    // MIN / MAX: b when either is a NaN
    const std::vector<double> mm = {1.0, 7.0, 9.0};
    CHECK(run({{OP_CONST, 1}, {OP_CONST, 0}, {OP_NEG, 0}, {OP_SQRT, 0}, {OP_MIN, 0}, {OP_CONST, 0}, {OP_NEG, 0}, {OP_SQRT, 0}, {OP_CONST, 1}, {OP_MIN, 0}, {OP_CONST, 1}, {OP_CONST, 2},
               {OP_MIN, 0}}, mm) == rgb(0, 7, 7));
    CHECK(run({{OP_CONST, 1}, {OP_CONST, 0}, {OP_NEG, 0}, {OP_SQRT, 0}, {OP_MAX, 0}, {OP_CONST, 0}, {OP_NEG, 0}, {OP_SQRT, 0}, {OP_CONST, 1}, {OP_MAX, 0}, {OP_CONST, 1}, {OP_CONST, 2},
               {OP_MAX, 0}}, mm) == rgb(0, 7, 9));
    // LT, LE, FLT with its band; x 255
    const std::vector<double> cmp = {1.0, 1.0 + 5e-9, 2.0, 255.0};
    CHECK(run({{OP_CONST, 0}, {OP_CONST, 1}, {OP_LT, 0}, {OP_CONST, 3}, {OP_MUL, 0}, {OP_CONST, 0}, {OP_CONST, 1}, {OP_FLT, 0}, {OP_CONST, 3}, {OP_MUL, 0}, {OP_CONST, 0}, {OP_CONST, 2},
               {OP_FLT, 0}, {OP_CONST, 3}, {OP_MUL, 0}}, cmp) == rgb(255, 0, 255));
    CHECK(run({{OP_CONST, 0}, {OP_CONST, 0}, {OP_LE, 0}, {OP_CONST, 3}, {OP_MUL, 0}, {OP_CONST, 0}, {OP_CONST, 0}, {OP_LT, 0}, {OP_CONST, 3}, {OP_MUL, 0}, {OP_CONST, 2}, {OP_CONST, 0},
               {OP_LE, 0}, {OP_CONST, 3}, {OP_MUL, 0}}, cmp) == rgb(255, 0, 0));
    // SIN: 0 at 0, NaN at and beyond 2^20 (and for inf), the correctly rounded value below; ABS, FLOOR, SQRT, DIV by zero
    CHECK(run({{OP_CONST, 0}, {OP_SIN, 0}, {OP_CONST, 1}, {OP_ADD, 0}, {OP_CONST, 2}, {OP_SIN, 0}, {OP_CONST, 1}, {OP_ADD, 0}, {OP_CONST, 1}, {OP_CONST, 0}, {OP_DIV, 0}, {OP_SIN, 0},
               {OP_CONST, 1}, {OP_ADD, 0}}, {0.0, 5.0, 1048576.0}) == rgb(5, 0, 0));
    CHECK(run({{OP_CONST, 0}, {OP_SIN, 0}, {OP_CONST, 1}, {OP_MUL, 0}, {OP_CONST, 2}, {OP_FLOOR, 0}, {OP_ABS, 0}, {OP_CONST, 3}, {OP_SQRT, 0}}, {1.5707963267948966, 200.0, -2.5, 49.0}) ==
          rgb(200, 3, 7));
    CHECK(run({{OP_CONST, 0}, {OP_CONST, 1}, {OP_DIV, 0}, {OP_CONST, 0}, {OP_NEG, 0}, {OP_CONST, 1}, {OP_DIV, 0}, {OP_CONST, 1}, {OP_CONST, 1}, {OP_DIV, 0}}, {1.0, 0.0}) == rgb(255, 0, 0));
    // sin(20) = 0.91294525..., sin(10) = -0.54402111...: x 100 + 100
    CHECK(run({{OP_CONST, 0}, {OP_SIN, 0}, {OP_CONST, 2}, {OP_MUL, 0}, {OP_CONST, 2}, {OP_ADD, 0}, {OP_CONST, 1}, {OP_SIN, 0}, {OP_CONST, 2}, {OP_MUL, 0}, {OP_CONST, 2}, {OP_ADD, 0}, {OP_U, 0}},
              {20.0, 10.0, 100.0}) == rgb(191, 45, 0));
    puts("eval ok");
}

static void stage_enumerate() {
    // every program of 1, 2 or 3 instructions over the opcodes (one unknown one among them) and operands 0 and 1, with one constant
    const int NOP = OP_COUNT + 1;
    unsigned long accepted = 0, refused = 0;
    for (int len = 1; len <= 3; ++len) {
        const long total = (long) pow((double) (NOP * 2), len);
        for (long code = 0; code < total; ++code) {
            std::vector<Ins> ins;
            long c = code;
            for (int i = 0; i < len; ++i) { ins.push_back({(int) (c % NOP), (int) ((c / NOP) % 2)}); c /= NOP * 2; }
            Block b(ins, {0.5});
            if (check(b.p, b.n) == OK) { ++accepted; (void) eval(b.p, 0.3, 0.6, 1.0, 2.0, 3.0); }
            else ++refused;
        }
    }
    CHECK(accepted == 6ul * 6ul * 6ul + 0ul); // three pushes, each one of U V PX PY PZ (operand 0) or CONST 0: nothing else leaves three values
    CHECK(refused > 0);
    puts("enumerate ok");
}

static double opaque(double v) { volatile double x = v; return x; } // (no constant folding of the conversions)
#define B(v) to_byte(opaque(v))
static void stage_bytes() {
    CHECK(B(0.0) == 0 && B(-0.0) == 0 && B(255.0) == 255 && B(255.999) == 255 && B(256.0) == 0 && B(257.5) == 1);
    CHECK(B(-1.0) == 255 && B(-0.999) == 0 && B(-256.0) == 0 && B(-257.0) == 255);
    CHECK(B(2147483647.0) == 255 && B(2147483648.0) == 255 && B(2147483646.0) == 254 && B(4294967296.0 + 5.0) == 255);
    CHECK(B(-2147483648.0) == 0 && B(-2147483649.0) == 0 && B(-2147483647.0) == 1);
    CHECK(B(1e300) == 255 && B(-1e300) == 0 && B(INFINITY) == 255 && B(-INFINITY) == 0 && B(NAN) == 0 && B(-NAN) == 0);
    for (int i = 0; i <= 255; ++i) { // ramp_byte: byte (x * 255.0)
        const double x = i / 255.0, t = x * 255.0;
        CHECK(to_byte(t) == (((uint32_t) (int32_t) t) & 0xFFu));
    }
    puts("bytes ok");
}

static int eval_lines() {
    char line[8192];
    while (fgets(line, sizeof line, stdin)) {
        char *sp = strchr(line, ' ');
        if (!sp) return 2;
        const size_t n = (size_t) (sp - line) / 2;
        uint8_t *prog = (uint8_t *) malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) { unsigned v; sscanf(line + 2 * i, "%2x", &v); prog[i] = (uint8_t) v; }
        unsigned long long w[5];
        if (sscanf(sp, " %llx %llx %llx %llx %llx", &w[0], &w[1], &w[2], &w[3], &w[4]) != 5) return 2;
        double d[5];
        memcpy(d, w, sizeof d);
        if (check(prog, n) != OK) { puts("refused"); free(prog); continue; }
        const uint32_t c = eval(prog, d[0], d[1], d[2], d[3], d[4]);
        printf("%u %u %u\n", c & 0xFFu, (c >> 8) & 0xFFu, (c >> 16) & 0xFFu);
        free(prog);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "eval") == 0) return eval_lines();
    stage_check();
    stage_eval();
    stage_enumerate();
    stage_bytes();
    return 0;
}
