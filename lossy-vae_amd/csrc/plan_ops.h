// plan_ops.h -- how lvae_run_ops (plan_runtime.cpp) gets from a recorded lvae_op to a call: derived from the entry points' prototypes.
//
// A launch plan stores an entry point's arguments by class, each class in call order: pointers in p[], integers in i[], floats in f[]
// (include/lvae_hip.h: lvae_op; lvae/engine.py: Plan._segment sorts them by the ctypes argtypes).  entry<fn> walks fn's parameter list
// left to right with the same rule: every parameter comes from the next slot of its class, cast to the parameter's type, and the stream
// goes last -- so the prototype is the only place that says which slot an argument comes from.  The same walk gives the class string
// ("ppii": one letter per argument) that tests/c_client/plan_ops_check.cpp prints for the comparison with the Python side.
// Needs no HIP: this header, the C header and the standard library.
#ifndef LVAE_PLAN_OPS_H
#define LVAE_PLAN_OPS_H

#include <array>
#include <cstddef>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../../include/lvae_hip.h"

namespace lvae_plan __attribute__((visibility("hidden"))) {      // (hidden: the instances are no part of the library's exports)

template <class T>
constexpr char arg_class() {
    static_assert(std::is_pointer_v<T> || std::is_floating_point_v<T> || std::is_integral_v<T>, "an lvae_op carries pointers, integers and floats");
    return std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f' : 'i';
}
template <class Params, std::size_t... K>
constexpr std::array<char, sizeof...(K) + 1> classes_of(std::index_sequence<K...>) {
    return {{arg_class<std::tuple_element_t<K, Params>>()..., '\0'}};
}

struct cursor {                       // the next slot of each class
    const lvae_op& o;
    int p = 0, i = 0, f = 0;
    template <class T>
    T next() {
        if constexpr (std::is_pointer_v<T>) return static_cast<T>(o.p[p++]);
        else if constexpr (std::is_floating_point_v<T>) return static_cast<T>(o.f[f++]);
        else return static_cast<T>(o.i[i++]);
    }
};

template <auto Fn>
struct entry;
template <class... A, int (*Fn)(A...)>
struct entry<Fn> {
    using params = std::tuple<A...>;
    static constexpr std::size_t N = sizeof...(A) - 1;                 // the stream comes from the call, not from the op
    static constexpr std::size_t n_p = (std::is_pointer_v<A> + ...) - 1, n_f = (std::is_floating_point_v<A> + ...), n_i = N - n_p - n_f;
    static_assert(std::is_same_v<std::tuple_element_t<N, params>, void*>, "an entry point's last parameter is the stream");
    static_assert(n_p <= std::extent_v<decltype(lvae_op::p)> && n_i <= std::extent_v<decltype(lvae_op::i)> && n_f <= std::extent_v<decltype(lvae_op::f)>,
                  "more arguments of one class than an lvae_op holds");
    static constexpr std::array<char, N + 1> classes = classes_of<params>(std::make_index_sequence<N>{});

    template <std::size_t... K>
    static int call(const lvae_op& o, void* stream, std::index_sequence<K...>) {
        cursor c{o};
        std::tuple<std::tuple_element_t<K, params>...> a{c.next<std::tuple_element_t<K, params>>()...};   // braces: evaluated left to right
        return Fn(std::get<K>(a)..., stream);
    }
    static int run(const lvae_op& o, void* stream) { return call(o, stream, std::make_index_sequence<N>{}); }
};

struct op_row { int kind; const char* name; int (*run)(const lvae_op&, void* stream); const char* classes; };

// One row per kind, in the enum's order (row k has kind k + 1); LVAE_OP_ORDER is not an entry point and has no row.
#define LVAE_PLAN_ROW(kind, fn) {kind, #fn, &entry<fn>::run, entry<fn>::classes.data()}
inline constexpr op_row op_table[] = {
    LVAE_PLAN_ROW(LVAE_OP_GEMM, lvae_gemm_f32),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_F32, lvae_dwconv_ln_f32),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_H2, lvae_dwconv_ln_h2),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_BF16, lvae_dwconv_ln_bf16),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_Q8, lvae_dwconv_ln_q8),
    LVAE_PLAN_ROW(LVAE_OP_STEM_F32, lvae_stem_f32),
    LVAE_PLAN_ROW(LVAE_OP_STEM_BF16, lvae_stem_bf16),
    LVAE_PLAN_ROW(LVAE_OP_BIAS_EXPAND_F32, lvae_bias_expand_f32),
    LVAE_PLAN_ROW(LVAE_OP_BIAS_EXPAND_BF16, lvae_bias_expand_bf16),
    LVAE_PLAN_ROW(LVAE_OP_PRIOR_INDEX, lvae_prior_index_f32),
    LVAE_PLAN_ROW(LVAE_OP_QUANTIZE, lvae_quantize_f32),
    LVAE_PLAN_ROW(LVAE_OP_DEQUANTIZE, lvae_dequantize_f32),
    LVAE_PLAN_ROW(LVAE_OP_GAUSSIAN_NLL, lvae_gaussian_nll_f32),
    LVAE_PLAN_ROW(LVAE_OP_LOSSLESS_PARAMS, lvae_lossless_params_f32),
    LVAE_PLAN_ROW(LVAE_OP_LOSSLESS_OUTPUT, lvae_lossless_output_f32),
    LVAE_PLAN_ROW(LVAE_OP_MLP_H2F, lvae_mlp_h2f),
    LVAE_PLAN_ROW(LVAE_OP_MLP_SK, lvae_mlp_sk),
    LVAE_PLAN_ROW(LVAE_OP_PRIOR_INDEX_SK, lvae_prior_index_sk_f32),
    LVAE_PLAN_ROW(LVAE_OP_QUANTIZE_SK, lvae_quantize_sk_f32),
    LVAE_PLAN_ROW(LVAE_OP_GAUSSIAN_NLL_CHAN, lvae_gaussian_nll_chan_f32),
    LVAE_PLAN_ROW(LVAE_OP_RD_IMAGE, lvae_rd_image_f32),
    LVAE_PLAN_ROW(LVAE_OP_PIXEL_NLL, lvae_pixel_nll_f32),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_F32_V, lvae_dwconv_ln_f32_v),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_H2_V, lvae_dwconv_ln_h2_v),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_BF16_V, lvae_dwconv_ln_bf16_v),
    LVAE_PLAN_ROW(LVAE_OP_DWCONV_LN_Q8_V, lvae_dwconv_ln_q8_v),
};
#undef LVAE_PLAN_ROW
inline constexpr int n_ops = (int)(sizeof(op_table) / sizeof(op_table[0]));
static_assert([] { for (int k = 0; k < n_ops; ++k) if (op_table[k].kind != k + 1) return false; return true; }() && LVAE_OP_ORDER == n_ops + 1,
              "op_table is indexed by kind - 1 and covers every kind below LVAE_OP_ORDER");

}  // namespace lvae_plan
#endif  // LVAE_PLAN_OPS_H
