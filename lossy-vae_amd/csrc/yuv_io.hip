// YUV frames in and out of the codec on the device -- planar, 8, 10 or 12 bits at 4:2:0 / 4:2:2 / 4:4:4, with centre- or left-sited
// (co-sited) chroma, and semi-planar (NV12; P010, P012, P210, P212) -- and the exact squared error of 8- and 16-bit planes for PSNR-YUV.
// include/lvae_hip.h states the contract of the eight entries; lvae/utils/yuv.py states the two conversions as torch expressions
// (yuv_to_rgb_expr2 / rgb_to_yuv_expr2), and the kernels here reproduce their bits: floating-point contraction is switched off for this
// file (the pragma below), so every product and sum is rounded on its own and nothing becomes a fused multiply-add, and divisions are
// IEEE divisions (__fdiv_rn, as in image_io.hip), never a multiplication by a reciprocal.  (The __fmul_rn / __fadd_rn wrappers of the HIP
// headers do NOT serve here: they are plain products and sums compiled under the default contraction, and fuse after inlining.)
//
// The RGB -> YUV half -- constants, matrix, chroma down-sampling of a lane's block, rounding, stores -- lives in yuv_convert.h, which
// tile_stitch_yuv.hip is written against as well; its functions switch contraction off in their own bodies, so they round alike there.
// The YUV -> RGB half of ONE pixel -- its rows, its codes, the conversion -- and the frames' descriptors live in yuv_fetch.h, which
// resample_yuv.hip is written against as well: yuv_to_f32_kernel keeps the 4-pixel loads and calls it for the rest.
//
// All are streaming kernels in the mould of image_io.hip: up to YUV_CHUNK frames (plane pairs) per launch, their descriptors in the
// kernel arguments -- no copy to the device, no scratch.  Samples of more than 8 bits are the low bits of 16-bit words (yuv420p10le ...);
// the kernels mask every sample to `depth` bits.  Row strides are in samples.  Kernels are templates on the sample type, the two
// subsampling shifts and the siting, so a variant has no branch on any of them.  yuv_to_f32: one lane owns 4 consecutive canvas pixels of
// one row (one 4- or 8-byte luma load where the address allows, one float4 per RGB plane); the chroma filter runs on integers: per
// subsampled axis the weights are quarters, so 4 (or 16) times the filtered value is an integer of at most 16 * 4095 and exact in any
// order.  f32_to_yuv: one lane owns a block of (2 or 1 rows) x 4 columns; left siting needs the column before the block, which is one more
// scalar load per row and plane.  sse: one lane owns 16 consecutive bytes of one row of both planes; integer sums from the lane to the one
// 64-bit atomic per wave.
//
// Semi-planar frames are one more template parameter, SP, of the same two kernels: a chroma pixel is two neighbouring samples, U then V, of
// one plane, and a sample's code is the HIGH `depth` bits of its container (>> (8 * sizeof(T) - depth) in, << the same out: 6 or 4 bits for
// the 16-bit words of the P010 family, none for the bytes of NV12).  The host passes the UV plane as u, the same plane one sample on as v,
// and the UV row stride for both, so the only new addressing is the chroma column c at sample 2c.  A lane's two chroma pixels are 4
// consecutive samples: one 4- or 8-byte access where the address allows.  The arithmetic is the planar variants', hence so are the bits.
// lvae_image_yuv420_to_f32 / lvae_image_f32_to_yuv420 are the <uint8_t, 4:2:0, centre> instances, planar for I420 and SP for NV12.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/lvae_hip.h"
#include "yuv_convert.h"
#include "yuv_fetch.h"

#pragma clang fp contract(off)

namespace {

constexpr int YUV_WG = 256;                                  // (YUV_CHUNK frames per launch, their PlaneDesc in a PlaneBatch: yuv_fetch.h)

// 4 consecutive samples: one 4-byte (8-bit) or 8-byte (16-bit) access where the address allows, scalars where not
// (SP: the code is the word's high bits)
template <typename T, int SP = 0>
__device__ __forceinline__ void load4(const T* __restrict__ p, const YuvParams& k, unsigned o[4]) {
    if (((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t q = *(const uint32_t*)p;
            o[0] = q & 255u; o[1] = (q >> 8) & 255u; o[2] = (q >> 16) & 255u; o[3] = q >> 24;
        } else {
            const uint2 q = *(const uint2*)p;
            o[0] = q.x & 0xffffu; o[1] = q.x >> 16; o[2] = q.y & 0xffffu; o[3] = q.y >> 16;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = p[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (SP ? o[i] >> k.shift : o[i]) & k.mask;
}

// SX, SY: the chroma planes are (h >> SY, w >> SX); LEFT: the chroma sample lies on the even luma column (SX only; vertically it is centred);
// SP: semi-planar words (the head of the file)
template <typename T, int SX, int SY, int LEFT, int SP = 0>
__global__ __launch_bounds__(YUV_WG) void yuv_to_f32_kernel(PlaneBatch fb, float* __restrict__ dst, long dst_img, int H, int W, int quads,
                                                            int vec_ok, YuvParams k, int bilinear) {
    static_assert(SX || !SY, "4:4:0 is not a layout of this file");
    static_assert(!SP || SX, "semi-planar frames are 4:2:0 / 4:2:2");
    constexpr int CS = SP ? 2 : 1;                           // samples from one chroma column to the next
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)H * quads) return;
    const int y = (int)(idx / quads), x0 = (int)(idx - (long)y * quads) * 4;
    const PlaneDesc im = fb.d[blockIdx.y];
    auto code = [&](unsigned word) -> unsigned { return yuv_code<SP>(word, k); };
    const int ys = min(y, im.h - 1);                         // rows below the extent repeat its last row
    const YuvRows<T> rw = yuv_rows<T, SX, SY>(im, ys, bilinear);
    const int cw = rw.cw;
    const T* __restrict__ yr = rw.yr;
    const T* __restrict__ ua = rw.ua;
    const T* __restrict__ ub = rw.ub;
    const T* __restrict__ va = rw.va;
    const T* __restrict__ vb = rw.vb;
    // Y and CU, CV = (SX ? 4 : 1) * (SY ? 4 : 1) times the upsampled chroma, exact
    unsigned Y[4], CU[4], CV[4];
    if (x0 + 3 < im.w) {                                     // 4 valid pixels
        load4<T, SP>(yr + x0, k, Y);
        if constexpr (!SX) {
            load4(ua + x0, k, CU);
            load4(va + x0, k, CV);
        } else {
            const int c0 = x0 >> 1;                          // c0 + 1 <= cw - 1 because x0 + 3 <= w - 1
            auto vert = [&](const T* __restrict__ a, const T* __restrict__ b, int c) -> unsigned {
                const unsigned p = code(a[c * CS]);
                return SY ? 3u * p + code(b[c * CS]) : p;    // (nearest: b == a, 4 p)
            };
            unsigned u1, u2, v1, v2;
            if constexpr (SP) {                              // U V U V of columns c0, c0 + 1: 4 consecutive words per chroma row
                unsigned qa[4], qb[4];
                load4<T, 1>(ua + 2 * c0, k, qa);
                if constexpr (SY) load4<T, 1>(ub + 2 * c0, k, qb);
                auto vert4 = [&](int i) -> unsigned { return SY ? 3u * qa[i] + qb[i] : qa[i]; };
                u1 = vert4(0); v1 = vert4(1); u2 = vert4(2); v2 = vert4(3);
            } else {
                u1 = vert(ua, ub, c0); u2 = vert(ua, ub, c0 + 1); v1 = vert(va, vb, c0); v2 = vert(va, vb, c0 + 1);
            }
            if (bilinear) {
                const int cp = min(c0 + 2, cw - 1);
                const unsigned u3 = vert(ua, ub, cp), v3 = vert(va, vb, cp);
                if constexpr (LEFT) {                        // column 2k: sample k; column 2k + 1: (c[k] + c[k + 1]) / 2
                    CU[0] = 4u * u1; CU[1] = 2u * (u1 + u2); CU[2] = 4u * u2; CU[3] = 2u * (u2 + u3);
                    CV[0] = 4u * v1; CV[1] = 2u * (v1 + v2); CV[2] = 4u * v2; CV[3] = 2u * (v2 + v3);
                } else {                                     // 3/4 of the sample the pixel lies in, 1/4 of the neighbour on its side
                    const int cm = max(c0 - 1, 0);
                    const unsigned u0 = vert(ua, ub, cm), v0 = vert(va, vb, cm);
                    CU[0] = 3u * u1 + u0; CU[1] = 3u * u1 + u2; CU[2] = 3u * u2 + u1; CU[3] = 3u * u2 + u3;
                    CV[0] = 3u * v1 + v0; CV[1] = 3u * v1 + v2; CV[2] = 3u * v2 + v1; CV[3] = 3u * v2 + v3;
                }
            } else {
                CU[0] = CU[1] = 4u * u1; CU[2] = CU[3] = 4u * u2;
                CV[0] = CV[1] = 4u * v1; CV[2] = CV[3] = 4u * v2;
            }
        }
    } else {                                                 // at or beyond the right edge: every pixel from its nearest valid one
#pragma unroll
        for (int i = 0; i < 4; ++i) yuv_pixel_codes<T, SX, SY, LEFT, SP>(rw, min(x0 + i, im.w - 1), bilinear, k, Y[i], CU[i], CV[i]);
    }
    float o3[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) yuv_codes_to_rgb<SX, SY>(Y[i], CU[i], CV[i], k, o3[0][i], o3[1][i], o3[2][i]);
    float* o = dst + (long)blockIdx.y * dst_img + (long)y * W + x0;
    const long plane = (long)H * W;
    if (vec_ok) {                                            // W % 4 == 0: the quad is whole and 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(o + c * plane) = make_float4(o3[c][0], o3[c][1], o3[c][2], o3[c][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) o[c * plane + i] = o3[c][i];
    }
}

template <typename T, int SX, int SY, int LEFT, int SP = 0>
__global__ __launch_bounds__(YUV_WG) void f32_to_yuv_kernel(const float* __restrict__ src, long src_img, long src_plane, long src_row,
                                                            PlaneBatch fb, int quads, int hblocks, int vec_ok, YuvParams k) {
    constexpr int R = SY ? 2 : 1;                            // rows of a block
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)hblocks * quads) return;
    const int by = (int)(idx / quads), x0 = (int)(idx - (long)by * quads) * 4;
    const int y0 = by << SY;
    const PlaneDesc im = fb.d[blockIdx.y];
    if (y0 >= im.h || x0 >= im.w) return;                    // h (w) is even where subsampled: the block's R rows (a column pair) are inside
    const int n = min(4, im.w - x0);                         // valid columns of this block (2 or 4 where SX)
    const float* __restrict__ s = src + (long)blockIdx.y * src_img + (long)y0 * src_row + x0;
    float p[3][R][4];
    if (vec_ok && n == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 f = *(const float4*)(s + c * src_plane + r * src_row);
                p[c][r][0] = f.x; p[c][r][1] = f.y; p[c][r][2] = f.z; p[c][r][3] = f.w;
            }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][r][i] = i < n ? s[c * src_plane + r * src_row + i] : 0.0f;
    }
    [[maybe_unused]] float pl[3][R];                         // left siting: column max(x0 - 1, 0), another lane's pixel
    if constexpr (SX && LEFT) {
        const int off = x0 > 0 ? -1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) pl[c][r] = s[c * src_plane + r * src_row + off];
    }
    // the block's first chroma sample: column x0 >> SX of chroma row by -- semi-planar: the U of its U V pair, sample 2 (x0 >> 1) = x0
    yuv_block_store<T, SX, SY, LEFT, SP>(p, pl, n, k, (T*)im.y + (long)y0 * im.yrow + x0, im.yrow, (T*)im.u + (long)by * im.urow + (SP ? x0 : x0 >> SX),
                                         (T*)im.v + (long)by * im.vrow + (x0 >> SX));
}

template <typename T> struct SsePair { const T *a, *b; long arow, brow; int h, w; };
template <typename T> struct SseBatch { SsePair<T> d[YUV_CHUNK]; };

template <typename T>
__global__ __launch_bounds__(YUV_WG) void sse_kernel(SseBatch<T> pb, unsigned long long* __restrict__ out, int chunks) {
    constexpr int N = 16 / sizeof(T), BITS = 8 * sizeof(T);  // samples per lane, bits per sample
    // bytes: <= 16 * 255^2 per lane, <= 64 * that per wave: fits 32 bits.  words: 64 bits from the lane on: 8 * 65535^2 does not fit 32
    using Acc = typename std::conditional<sizeof(T) == 1, unsigned, unsigned long long>::type;
    const SsePair<T> pr = pb.d[blockIdx.y];
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    Acc acc = 0;
    const int y = (int)(idx / chunks), x0 = (int)(idx - (long)y * chunks) * N;
    if (y < pr.h && x0 < pr.w) {                             // (no early return: every lane takes part in the wave's sum below)
        const T* __restrict__ a = pr.a + (long)y * pr.arow + x0;
        const T* __restrict__ b = pr.b + (long)y * pr.brow + x0;
        auto sq = [](unsigned p, unsigned q) -> Acc {
            const unsigned d = p > q ? p - q : q - p;
            return (Acc)(d * d);                             // 65535^2 < 2^32
        };
        if (x0 + N - 1 < pr.w && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
            const uint4 va = *(const uint4*)a, vb = *(const uint4*)b;
            const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int s = 0; s < 32; s += BITS) acc += sq((wa[j] >> s) & ((1u << BITS) - 1u), (wb[j] >> s) & ((1u << BITS) - 1u));
        } else {
            const int n = min(N, pr.w - x0);
            for (int i = 0; i < n; ++i) acc += sq(a[i], b[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out + blockIdx.y, (unsigned long long)acc);
}

// Frames -> the fp32 canvas: every check of the three entries' common arguments, then one launch per YUV_CHUNK frames
int yuv_to_f32(const Planes& p, int B, int depth, int subsampling, int siting, int matrix, int range, int chroma, float* dst, long dst_img,
               int H, int W, void* stream) {
    if (!dst || B <= 0 || H <= 0 || W <= 0 || !enums_ok(depth, subsampling, siting, matrix, range) ||
        (chroma != LVAE_YUV_NEAREST && chroma != LVAE_YUV_BILINEAR))
        return -22;
    const int sx = subsampling != LVAE_YUV_SUB_444, sy = subsampling == LVAE_YUV_SUB_420;
    const int quads = (W + 3) / 4;
    if ((long)H * quads > (long)INT_MAX || (B > 1 && dst_img < 3L * H * W)) return -22;
    if (!frames_ok(p, B, sx, sy, H, W)) return -22;
    const int vec_ok = W % 4 == 0 && dst_img % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const unsigned gx = (unsigned)(((long)H * quads + YUV_WG - 1) / YUV_WG);
    const YuvParams k = yuv_params(matrix, range, depth);
    auto kernel = YUV_PICK(yuv_to_f32_kernel, depth, subsampling, siting == LVAE_YUV_SITING_LEFT, p.sp);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)n), dim3(YUV_WG), 0, (hipStream_t)stream, plane_batch(p, b0, n), dst + (long)b0 * dst_img,
                           dst_img, H, W, quads, vec_ok, k, chroma == LVAE_YUV_BILINEAR);
    }
    return (int)hipGetLastError();
}

// The inverse, with the same division of labour
int f32_to_yuv(const float* src, long src_img, long src_plane, long src_row, int H, int W, int B, int depth, int subsampling, int siting,
               int matrix, int range, const Planes& p, void* stream) {
    if (!src || B <= 0 || H <= 0 || W <= 0 || !enums_ok(depth, subsampling, siting, matrix, range)) return -22;
    if (src_row < W || src_plane < (long)(H - 1) * src_row + W || (B > 1 && src_img < 2 * src_plane + (long)(H - 1) * src_row + W)) return -22;
    const int sx = subsampling != LVAE_YUV_SUB_444, sy = subsampling == LVAE_YUV_SUB_420;
    if (!frames_ok(p, B, sx, sy, H, W)) return -22;
    int hmax = 0, wmax = 0;
    for (int b = 0; b < B; ++b) {
        hmax = p.hw[2 * b] > hmax ? p.hw[2 * b] : hmax;
        wmax = p.hw[2 * b + 1] > wmax ? p.hw[2 * b + 1] : wmax;
    }
    const int quads = (wmax + 3) / 4, hblocks = hmax >> sy;
    if ((long)hblocks * quads > (long)INT_MAX) return -22;
    const int vec_ok = src_img % 4 == 0 && src_plane % 4 == 0 && src_row % 4 == 0 && ((uintptr_t)src & 15) == 0;
    const unsigned gx = (unsigned)(((long)hblocks * quads + YUV_WG - 1) / YUV_WG);
    const YuvParams k = yuv_params(matrix, range, depth);
    auto kernel = YUV_PICK(f32_to_yuv_kernel, depth, subsampling, siting == LVAE_YUV_SITING_LEFT, p.sp);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)n), dim3(YUV_WG), 0, (hipStream_t)stream, src + (long)b0 * src_img, src_img, src_plane,
                           src_row, plane_batch(p, b0, n), quads, hblocks, vec_ok, k);
    }
    return (int)hipGetLastError();
}

template <typename T>
int sse(const T* const* a, const long* a_row, const T* const* b, const long* b_row, const int* hw, int n, uint64_t* out, void* stream) {
    constexpr int N = 16 / sizeof(T);                        // samples per lane
    if (!a || !a_row || !b || !b_row || !hw || !out || n <= 0) return -22;
    int hmax = 0, wmax = 0;
    for (int k = 0; k < n; ++k) {
        const int h = hw[2 * k], w = hw[2 * k + 1];
        if (!a[k] || !b[k] || h <= 0 || w <= 0 || a_row[k] < w || b_row[k] < w) return -22;
        hmax = h > hmax ? h : hmax;
        wmax = w > wmax ? w : wmax;
    }
    const int chunks = (wmax - 1) / N + 1;                   // one grid shape for every launch of the call: the largest plane's
    const long most = (long)hmax * chunks;
    if (most > (long)INT_MAX) return -22;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)n, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const unsigned gx = (unsigned)((most + YUV_WG - 1) / YUV_WG);
    for (int k0 = 0; k0 < n; k0 += YUV_CHUNK) {
        const int m = n - k0 < YUV_CHUNK ? n - k0 : YUV_CHUNK;
        SseBatch<T> pb = {};
        for (int i = 0; i < m; ++i) {
            const int k = k0 + i;
            pb.d[i] = {a[k], b[k], a_row[k], b_row[k], hw[2 * k], hw[2 * k + 1]};
        }
        hipLaunchKernelGGL(sse_kernel<T>, dim3(gx, (unsigned)m), dim3(YUV_WG), 0, (hipStream_t)stream, pb, (unsigned long long*)out + k0, chunks);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int lvae_image_yuv_to_f32(const void* const* y, const void* const* u, const void* const* v, const long* y_row, const long* u_row,
                                     const long* v_row, const int* hw, int B, int depth, int subsampling, int siting, int matrix, int range,
                                     int chroma, float* dst, long dst_img, int H, int W, void* stream) {
    return yuv_to_f32({y, u, v, y_row, u_row, v_row, hw, depth == 8 ? 1 : 2, 0}, B, depth, subsampling, siting, matrix, range, chroma, dst,
                      dst_img, H, W, stream);
}

extern "C" int lvae_image_f32_to_yuv(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B, int depth,
                                     int subsampling, int siting, int matrix, int range, void* const* y, void* const* u, void* const* v,
                                     const long* y_row, const long* u_row, const long* v_row, void* stream) {
    return f32_to_yuv(src, src_img, src_plane, src_row, H, W, B, depth, subsampling, siting, matrix, range,
                      {y, u, v, y_row, u_row, v_row, hw, depth == 8 ? 1 : 2, 0}, stream);
}

extern "C" int lvae_image_yuvsp_to_f32(const uint16_t* const* y, const uint16_t* const* uv, const long* y_row, const long* uv_row, const int* hw,
                                       int B, int depth, int subsampling, int siting, int matrix, int range, int chroma, float* dst, long dst_img,
                                       int H, int W, void* stream) {
    if (!sp_layout_ok(depth, subsampling)) return -22;
    return yuv_to_f32({(const void* const*)y, (const void* const*)uv, nullptr, y_row, uv_row, nullptr, hw, 2, 1}, B, depth, subsampling, siting,
                      matrix, range, chroma, dst, dst_img, H, W, stream);
}

extern "C" int lvae_image_f32_to_yuvsp(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B, int depth,
                                       int subsampling, int siting, int matrix, int range, uint16_t* const* y, uint16_t* const* uv,
                                       const long* y_row, const long* uv_row, void* stream) {
    if (!sp_layout_ok(depth, subsampling)) return -22;
    return f32_to_yuv(src, src_img, src_plane, src_row, H, W, B, depth, subsampling, siting, matrix, range,
                      {(const void* const*)y, (const void* const*)uv, nullptr, y_row, uv_row, nullptr, hw, 2, 1}, stream);
}

// The 8-bit 4:2:0 entries: depth 8, 4:2:0, centre siting; I420 is the planar instance and NV12 the semi-planar one (v / v_row may be NULL)
extern "C" int lvae_image_yuv420_to_f32(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, const long* y_row,
                                        const long* u_row, const long* v_row, const int* hw, int B, int fmt, int matrix, int range,
                                        int chroma, float* dst, long dst_img, int H, int W, void* stream) {
    if (!yuv420_enums_ok(fmt, matrix, range)) return -22;
    return yuv_to_f32({(const void* const*)y, (const void* const*)u, (const void* const*)v, y_row, u_row, v_row, hw, 1, fmt == LVAE_YUV_NV12}, B,
                      8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, matrix, range, chroma, dst, dst_img, H, W, stream);
}

extern "C" int lvae_image_f32_to_yuv420(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B,
                                        int fmt, int matrix, int range, uint8_t* const* y, uint8_t* const* u, uint8_t* const* v,
                                        const long* y_row, const long* u_row, const long* v_row, void* stream) {
    if (!yuv420_enums_ok(fmt, matrix, range)) return -22;
    return f32_to_yuv(src, src_img, src_plane, src_row, H, W, B, 8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, matrix, range,
                      {(const void* const*)y, (const void* const*)u, (const void* const*)v, y_row, u_row, v_row, hw, 1, fmt == LVAE_YUV_NV12},
                      stream);
}

extern "C" int lvae_sse_u8(const uint8_t* const* a, const long* a_row, const uint8_t* const* b, const long* b_row, const int* hw, int n,
                           uint64_t* out, void* stream) {
    return sse(a, a_row, b, b_row, hw, n, out, stream);
}

extern "C" int lvae_sse_u16(const uint16_t* const* a, const long* a_row, const uint16_t* const* b, const long* b_row, const int* hw, int n,
                            uint64_t* out, void* stream) {
    return sse(a, a_row, b, b_row, hw, n, out, stream);
}

