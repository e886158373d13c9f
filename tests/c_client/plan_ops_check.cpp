/* The routing of csrc/plan_ops.h on the CPU: no launcher is called and no GPU is needed.
 * 1. entry<fn> applied to FAKE functions with the shapes the real table has: every p[] / i[] / f[] slot of an lvae_op holds its own
 *    sentinel, and each fake checks that every parameter received the slot its place in the prototype says, and the stream.
 * 2. For every row of the real table: "kind name classes" (classes: one of p / i / f per argument, in call order), then the kind of
 *    LVAE_OP_ORDER -- tests/test_abi.py::test_plan_ops_routing_matches_the_python_side compares them with lvae._native.
 * Returns 0, or 1 after naming the first mismatch. */
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "plan_ops.h"

namespace {

void* P(int j) { return (void*)(std::uintptr_t)(0x1000 + 16 * j); }
constexpr long I(int j) { return 101 + j; }
constexpr double F(int j) { return 0.25 + j; }
constexpr long BIG = (1L << 33) + 5;               // does not fit an int
void* const STREAM = (void*)(std::uintptr_t)0x5eed;
int calls = 0;

lvae_op sentinels() {
    lvae_op o;
    std::memset(&o, 0, sizeof o);
    for (int j = 0; j < 8; ++j) o.p[j] = P(j);
    for (int j = 0; j < 6; ++j) o.i[j] = I(j);
    for (int j = 0; j < 2; ++j) o.f[j] = F(j);
    return o;
}

#define EXPECT(cond)                                      \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("%s: %s\n", __func__, #cond);     \
            return 1;                                     \
        }                                                 \
    } while (0)

/* descriptor only (lvae_gemm_f32, lvae_mlp_h2f, lvae_mlp_sk) */
int fake_desc(const lvae_gemm_desc* d, void* st) {
    ++calls;
    EXPECT(d == P(0) && st == STREAM);
    return 0;
}
/* 8 pointers + 5 ints (lvae_dwconv_ln_*) */
int fake_dwln(const void* x, const float* wt, const float* bias, const float* ln_w, const float* ln_b, const float* shift, const float* scale1p,
              void* y, int B, int H, int W, int C, int k, void* st) {
    ++calls;
    EXPECT(x == P(0) && wt == P(1) && bias == P(2) && ln_w == P(3) && ln_b == P(4) && shift == P(5) && scale1p == P(6) && y == P(7));
    EXPECT(B == I(0) && H == I(1) && W == I(2) && C == I(3) && k == I(4) && st == STREAM);
    return 0;
}
/* 6 pointers + 5 ints + 1 long (lvae_dwconv_ln_*_v) */
int fake_dwln_v(const float* x, const float* wt, const float* bias, const float* shift, const float* scale1p, float* y, int B, int H, int W,
                int C, int k, long vstride, void* st) {
    ++calls;
    EXPECT(x == P(0) && wt == P(1) && bias == P(2) && shift == P(3) && scale1p == P(4) && y == P(5));
    EXPECT(B == I(0) && H == I(1) && W == I(2) && C == I(3) && k == I(4) && vstride == BIG && st == STREAM);
    return 0;
}
/* 7 pointers + 5 ints + 1 float, interleaved (lvae_prior_index_sk_f32) */
int fake_index_sk(const float* ws, int S, const float* bias, float* prm, float* pm, uint8_t* idx, const float* table, int n_scales, float bound,
                  int B, int HW, int z, int* status, void* st) {
    ++calls;
    EXPECT(ws == P(0) && bias == P(1) && prm == P(2) && pm == P(3) && idx == P(4) && table == P(5) && status == P(6));
    EXPECT(S == I(0) && n_scales == I(1) && B == I(2) && HW == I(3) && z == I(4) && bound == (float)F(0) && st == STREAM);
    return 0;
}
/* 2 floats between ints and a trailing pointer (lvae_stem_*) */
int fake_stem(const float* im, const float* wt, const float* bias, void* out, int B, int H, int W, int Cout, float im_shift, float im_scale,
              int* range_flag, void* st) {
    ++calls;
    EXPECT(im == P(0) && wt == P(1) && bias == P(2) && out == P(3) && range_flag == P(4));
    EXPECT(B == I(0) && H == I(1) && W == I(2) && Cout == I(3) && im_shift == (float)F(0) && im_scale == (float)F(1) && st == STREAM);
    return 0;
}
/* a long above 2^32 in front of an int (lvae_bias_expand_*: M) */
int fake_bias_expand(const float* bias, float* out, long M, int C, void* st) {
    ++calls;
    EXPECT(bias == P(0) && out == P(1) && M == BIG && C == I(1) && st == STREAM);
    return 0;
}
/* every class interleaved, a double among the floats */
int fake_mixed(void* a, int b, const double* c, long d, float e, char* f, int g, double h, void* st) {
    ++calls;
    EXPECT(a == P(0) && c == P(1) && f == P(2) && b == I(0) && d == BIG && g == I(2) && e == (float)F(0) && h == F(1) && st == STREAM);
    return 0;
}
/* the launcher's return code is the trampoline's */
int fake_rc(void* a, void* st) {
    ++calls;
    return a == P(0) && st == STREAM ? 7 : 1;
}

template <auto Fn>
int route(const char* classes, int long_slot, int want_rc) {
    using E = lvae_plan::entry<Fn>;
    EXPECT(std::strcmp(E::classes.data(), classes) == 0);
    lvae_op o = sentinels();
    if (long_slot >= 0) o.i[long_slot] = BIG;
    const int before = calls;
    int (*run)(const lvae_op&, void*) = &E::run;
    EXPECT(run(o, STREAM) == want_rc && calls == before + 1);
    return 0;
}

}  // namespace

int main() {
    if (route<fake_desc>("p", -1, 0) || route<fake_dwln>("ppppppppiiiii", -1, 0) || route<fake_dwln_v>("ppppppiiiiii", 5, 0) ||
        route<fake_index_sk>("pipppppifiiip", -1, 0) || route<fake_stem>("ppppiiiiffp", -1, 0) || route<fake_bias_expand>("ppii", 0, 0) ||
        route<fake_mixed>("pipifpif", 1, 0) || route<fake_rc>("p", -1, 7))
        return 1;
    for (const lvae_plan::op_row& r : lvae_plan::op_table) std::printf("%d %s %s\n", r.kind, r.name, r.classes);
    std::printf("%d ORDER -\n", (int)LVAE_OP_ORDER);
    return 0;
}
