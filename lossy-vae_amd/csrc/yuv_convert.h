// yuv_convert.h -- the RGB -> YUV side of the YUV kernels, shared by the kernels that end in YUV planes (yuv_io.hip: from an fp32 image;
// tile_stitch_yuv.hip: from the tiles of a tiled image): the constants of a conversion, the per-pixel matrix, the chroma down-sampling of
// one lane's block, the rounding to codes and the stores, planar or semi-planar.  One definition, hence one set of bits
// (lvae/utils/yuv.py::rgb_to_yuv_expr2 states them as torch expressions).  Every product and sum here is rounded on its own: each device
// function switches floating-point contraction off in its own body, so it holds whatever the including file compiles under.  The host
// half: the enum checks and the kernel variant of a (depth, subsampling, siting, layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/lvae_hip.h"

namespace {

// the fp32 constants of a conversion: the matrix (a = 2(1 - Kr), b = 2(1 - Kb), d = 2 Kb (1 - Kb) / Kg, e = 2 Kr (1 - Kr) / Kg, the literals of
// lvae/utils/yuv.py), the range at this depth (all integers, exact) and the sample mask 2^depth - 1 (peak is the same number as a float)
// -- and, for the semi-planar variants, the position (bits of the container) - depth of a code inside its sample
struct YuvParams { float kr, kg, kb, a, b, d, e, yo, ys, co, cs, peak; unsigned mask, shift; };

inline YuvParams yuv_params(int matrix, int range, int depth) {
    YuvParams k = matrix == LVAE_YUV_BT601   ? YuvParams{0.299f, 0.587f, 0.114f, 1.402f, 1.772f, 0.344136286f, 0.714136286f}
                  : matrix == LVAE_YUV_BT709 ? YuvParams{0.2126f, 0.7152f, 0.0722f, 1.5748f, 1.8556f, 0.187324273f, 0.468124273f}
                                             : YuvParams{0.2627f, 0.678f, 0.0593f, 1.4746f, 1.8814f, 0.164553127f, 0.571353127f};
    const float s = (float)(1 << (depth - 8)), peak = (float)((1 << depth) - 1);
    const bool full = range == LVAE_YUV_FULL;
    k.yo = full ? 0.0f : 16.0f * s;
    k.ys = full ? peak : 219.0f * s;
    k.co = 128.0f * s;
    k.cs = full ? peak : 224.0f * s;
    k.peak = peak;
    k.mask = (1u << depth) - 1u;
    k.shift = (depth == 8 ? 8u : 16u) - (unsigned)depth;     // (read by the SP variants only: 0 for NV12's bytes)
    return k;
}

inline bool enums_ok(int depth, int subsampling, int siting, int matrix, int range) {
    return (depth == 8 || depth == 10 || depth == 12) &&
           (subsampling == LVAE_YUV_SUB_420 || subsampling == LVAE_YUV_SUB_422 || subsampling == LVAE_YUV_SUB_444) &&
           (siting == LVAE_YUV_SITING_CENTER || siting == LVAE_YUV_SITING_LEFT) &&
           (matrix == LVAE_YUV_BT601 || matrix == LVAE_YUV_BT709 || matrix == LVAE_YUV_BT2020) &&
           (range == LVAE_YUV_LIMITED || range == LVAE_YUV_FULL);
}

inline bool sp_layout_ok(int depth, int subsampling) {       // the P010 family
    return (depth == 10 || depth == 12) && (subsampling == LVAE_YUV_SUB_420 || subsampling == LVAE_YUV_SUB_422);
}

// the 8-bit 4:2:0 entries: I420 | NV12, and BT.601 | BT.709 only
inline bool yuv420_enums_ok(int fmt, int matrix, int range) {
    return (fmt == LVAE_YUV_I420 || fmt == LVAE_YUV_NV12) && (matrix == LVAE_YUV_BT601 || matrix == LVAE_YUV_BT709) &&
           (range == LVAE_YUV_LIMITED || range == LVAE_YUV_FULL);
}

// the variant of KERNEL for (depth, subsampling, siting, semi-planar) -- siting has no effect without horizontal subsampling; the
// semi-planar ones are the P010 family (16-bit words, 4:2:0 / 4:2:2) and NV12 (bytes, 4:2:0, centre)
#define YUV_PICK_SUB(KERNEL, T, sub, left, SP)                                                                                          \
    ((sub) == LVAE_YUV_SUB_422 ? ((left) ? KERNEL<T, 1, 0, 1, SP> : KERNEL<T, 1, 0, 0, SP>)                                             \
                               : ((left) ? KERNEL<T, 1, 1, 1, SP> : KERNEL<T, 1, 1, 0, SP>))
#define YUV_PICK(KERNEL, depth, sub, left, sp)                                                                                          \
    ((sp)                            ? ((depth) == 8 ? KERNEL<uint8_t, 1, 1, 0, 1> : YUV_PICK_SUB(KERNEL, uint16_t, sub, left, 1))      \
     : (sub) == LVAE_YUV_SUB_444     ? ((depth) == 8 ? KERNEL<uint8_t, 0, 0, 0, 0> : KERNEL<uint16_t, 0, 0, 0, 0>)                      \
     : (depth) == 8                  ? YUV_PICK_SUB(KERNEL, uint8_t, sub, left, 0)                                                      \
                                     : YUV_PICK_SUB(KERNEL, uint16_t, sub, left, 0))

__device__ __forceinline__ float clamp01(float x) {          // NaN -> 0: both comparisons are false for a NaN
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}

// the first n (1..4) of 4 codes to consecutive samples
template <typename T>
__device__ __forceinline__ void store4(T* __restrict__ p, const unsigned v[4], int n) {
    if (n == 4 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 1) *(uint32_t*)p = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else *(uint2*)p = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    } else {
        for (int i = 0; i < n; ++i) p[i] = (T)v[i];
    }
}

// Semi-planar chroma: the first n (2 or 4) of the samples U V U V -- all four at once (store4's whole store), or a chroma pixel's U and V
// as one store of twice a sample, where the address allows
template <typename T>
__device__ __forceinline__ void store_uv(T* __restrict__ p, const unsigned v[4], int n) {
    using Pair = typename std::conditional<sizeof(T) == 1, uint16_t, uint32_t>::type;
    constexpr int BITS = 8 * sizeof(T);
    if (n == 4 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        store4(p, v, 4);
    } else if (((uintptr_t)p & (2 * sizeof(T) - 1)) == 0) {
        *(Pair*)p = (Pair)(v[0] | (v[1] << BITS));
        if (n == 4) *(Pair*)(p + 2) = (Pair)(v[2] | (v[3] << BITS));
    } else {
        for (int i = 0; i < n; ++i) p[i] = (T)v[i];
    }
}

// rint(v), ties to even, clamped to 0..peak (v is finite: its inputs were clamped)
__device__ __forceinline__ unsigned code_of(float v, float peak) {
    v = rintf(v);
    v = v > 0.0f ? v : 0.0f;
    v = v < peak ? v : peak;
    return (unsigned)(int)v;
}

// one pixel: clamped r, g, b -> y' and the two colour differences
__device__ __forceinline__ void ycc(float r, float g, float b, const YuvParams& k, float& yn, float& cb, float& cr) {
#pragma clang fp contract(off)
    const float R = clamp01(r), G = clamp01(g), B = clamp01(b);
    yn = (k.kr * R + k.kg * G) + k.kb * B;
    cb = __fdiv_rn(B - yn, k.b);
    cr = __fdiv_rn(R - yn, k.a);
}

// One lane's block of (SY ? 2 : 1) rows x 4 columns, of which the first n (2 or 4 where SX) exist: p[c][r][i] is its RGB, pl[c][r] the RGB
// of the column before the block (left siting only; the block's own first column where there is none before it) -> the codes of its
// luma samples at yp + r * yrow and of its chroma samples at up / vp, which point at the block's first one (semi-planar: up at its U V
// pair, vp is not read).  SX, SY: the chroma planes are (h >> SY, w >> SX); LEFT: the chroma sample lies on the even luma column (SX only;
// vertically it is centred); SP: semi-planar words, the code in the high bits
template <typename T, int SX, int SY, int LEFT, int SP>
__device__ __forceinline__ void yuv_block_store(const float (&p)[3][SY ? 2 : 1][4], const float (&pl)[3][SY ? 2 : 1], int n, const YuvParams& k,
                                                T* yp, long yrow, T* up, T* vp) {
#pragma clang fp contract(off)
    static_assert(SX || !SY, "4:4:0 is not a layout of this file");
    static_assert(!SP || SX, "semi-planar frames are 4:2:0 / 4:2:2");
    constexpr int R = SY ? 2 : 1;                            // rows of a block
    unsigned Yc[R][4];
    float cb[R][4], cr[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float yn;
            ycc(p[0][r][i], p[1][r][i], p[2][r][i], k, yn, cb[r][i], cr[r][i]);
            Yc[r][i] = code_of(yn * k.ys + k.yo, k.peak);
            if constexpr (SP) Yc[r][i] <<= k.shift;
        }
#pragma unroll
    for (int r = 0; r < R; ++r) store4(yp + r * yrow, Yc[r], n);
    if constexpr (!SX) {                                     // 4:4:4: a chroma sample per pixel
        unsigned Uc[4], Vc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Uc[i] = code_of(cb[0][i] * k.cs + k.co, k.peak);
            Vc[i] = code_of(cr[0][i] * k.cs + k.co, k.peak);
        }
        store4(up, Uc, n);
        store4(vp, Vc, n);
    } else {
        float pb[R], pr[R];                                  // left siting: the colour differences of the column before, another lane's pixel
        if constexpr (LEFT) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float yn;
                ycc(pl[0][r], pl[1][r], pl[2][r], k, yn, pb[r], pr[r]);
            }
        }
        [[maybe_unused]] unsigned UV[4];                                      // SP: the words U V U V of the block's two chroma pixels
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float hu[R], hv[R];                              // the horizontal step per row
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if constexpr (LEFT) {                        // ((c[2k - 1] + c[2k + 1]) + (c[2k] + c[2k])) / 4, c[-1] = c[0]
                    const float mu = j ? cb[r][1] : pb[r], mv = j ? cr[r][1] : pr[r];
                    hu[r] = ((mu + cb[r][2 * j + 1]) + (cb[r][2 * j] + cb[r][2 * j])) * 0.25f;
                    hv[r] = ((mv + cr[r][2 * j + 1]) + (cr[r][2 * j] + cr[r][2 * j])) * 0.25f;
                } else {
                    hu[r] = cb[r][2 * j] + cb[r][2 * j + 1];
                    hv[r] = cr[r][2 * j] + cr[r][2 * j + 1];
                }
            }
            float mu, mv;
            if constexpr (LEFT) {
                mu = SY ? (hu[0] + hu[R - 1]) * 0.5f : hu[0];
                mv = SY ? (hv[0] + hv[R - 1]) * 0.5f : hv[0];
            } else {
                mu = SY ? (hu[0] + hu[R - 1]) * 0.25f : hu[0] * 0.5f;
                mv = SY ? (hv[0] + hv[R - 1]) * 0.25f : hv[0] * 0.5f;
            }
            if constexpr (SP) {
                UV[2 * j] = code_of(mu * k.cs + k.co, k.peak) << k.shift;
                UV[2 * j + 1] = code_of(mv * k.cs + k.co, k.peak) << k.shift;
            } else if (2 * j < n) {
                up[j] = (T)code_of(mu * k.cs + k.co, k.peak);
                vp[j] = (T)code_of(mv * k.cs + k.co, k.peak);
            }
        }
        if constexpr (SP) store_uv(up, UV, n);               // n (2 or 4) columns are n samples of the UV row
    }
}

}  // namespace
