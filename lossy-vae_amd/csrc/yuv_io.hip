// 8-bit YUV 4:2:0 frames in and out of the codec on the device, and the exact squared error of byte planes for PSNR-YUV.
// include/lvae_hip.h (lvae_image_yuv420_to_f32 / lvae_image_f32_to_yuv420 / lvae_sse_u8) states the contract; lvae/utils/yuv.py states
// the two conversions as torch expressions, and the kernels here reproduce their bits: floating-point contraction is switched off for
// this file (the pragma below), so every product and sum is rounded on its own and nothing becomes a fused multiply-add, and divisions are
// IEEE divisions (__fdiv_rn, as in image_io.hip), never a multiplication by a reciprocal.  (The __fmul_rn / __fadd_rn wrappers of the HIP
// headers do NOT serve here: they are plain products and sums compiled under the default contraction, and fuse after inlining.)
//
// All three are streaming kernels in the mould of image_io.hip: up to YUV_CHUNK frames (SSE_CHUNK plane pairs) per launch, their
// descriptors in the kernel arguments -- no copy to the device, no scratch.  yuv420_to_f32: one lane owns 4 consecutive canvas pixels of
// one row (4 luma bytes, the 2 x 4 chroma samples under and beside them, one float4 per RGB plane); the chroma filter runs on integers
// (its weights are sixteenths, so it is exact in any order).  f32_to_yuv420: one lane owns a 2-row x 4-column block (six float4, two
// luma dwords, two chroma samples per plane).  sse_u8: one lane owns 16 consecutive bytes of one row of both planes; sums are integers
// from the lane to the one 64-bit atomic per wave.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int YUV_CHUNK = 16;                                // frames per launch
constexpr int SSE_CHUNK = 16;                                // plane pairs per launch
constexpr int YUV_WG = 256;

// one frame: planes, row strides in bytes, valid extent.  NV12: u = the UV plane, v = u + 1, urow == vrow; the sample step is 2
struct YuvDesc { uint8_t *y, *u, *v; long yrow, urow, vrow; int h, w; };
struct YuvBatch { YuvDesc d[YUV_CHUNK]; };

// fp32 constants of a matrix: a = 2(1 - Kr), b = 2(1 - Kb), d = 2 Kb (1 - Kb) / Kg, e = 2 Kr (1 - Kr) / Kg -- the literals of lvae/utils/yuv.py
struct YuvCoef { float kr, kg, kb, a, b, d, e; };
__host__ __device__ inline YuvCoef yuv_coef(int matrix) {
    return matrix == LVAE_YUV_BT601 ? YuvCoef{0.299f, 0.587f, 0.114f, 1.402f, 1.772f, 0.344136286f, 0.714136286f}
                                    : YuvCoef{0.2126f, 0.7152f, 0.0722f, 1.5748f, 1.8556f, 0.187324273f, 0.468124273f};
}

__device__ __forceinline__ float clamp01(float x) {          // NaN -> 0: both comparisons are false for a NaN
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}

// (Y, C16 = 16 * the upsampled chroma, exact) -> RGB in [0, 1]
__device__ __forceinline__ void yuv_to_rgb(unsigned Y, unsigned U16, unsigned V16, const YuvCoef k, int full, float& r, float& g, float& b) {
    const float yo = full ? 0.0f : 16.0f, ys = full ? 255.0f : 219.0f, cs = full ? 255.0f : 224.0f;
    const float yn = __fdiv_rn((float)Y - yo, ys);
    const float cb = __fdiv_rn((float)U16 * 0.0625f - 128.0f, cs);      // U16 / 16 is exact
    const float cr = __fdiv_rn((float)V16 * 0.0625f - 128.0f, cs);
    r = clamp01(yn + k.a * cr);
    b = clamp01(yn + k.b * cb);
    g = clamp01((yn - k.d * cb) - k.e * cr);
}

__global__ __launch_bounds__(YUV_WG) void yuv420_to_f32_kernel(YuvBatch fb, float* __restrict__ dst, long dst_img, int H, int W, int quads,
                                                               int vec_ok, int cstep, int matrix, int full, int bilinear) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)H * quads) return;
    const int y = (int)(idx / quads), x0 = (int)(idx - (long)y * quads) * 4;
    const YuvDesc im = fb.d[blockIdx.y];
    const YuvCoef k = yuv_coef(matrix);
    const int ch = im.h >> 1, cw = im.w >> 1;
    const int ys = min(y, im.h - 1);                         // rows below the extent repeat its last row
    const int cy = ys >> 1;
    // the second chroma row of the vertical filter: the neighbour on the pixel's side, clamped (weight 0 for nearest: cyb = cy)
    const int cyb = bilinear ? min(max(cy + ((ys & 1) ? 1 : -1), 0), ch - 1) : cy;
    const uint8_t* __restrict__ yr = im.y + (long)ys * im.yrow;
    const uint8_t* __restrict__ ua = im.u + (long)cy * im.urow;
    const uint8_t* __restrict__ ub = im.u + (long)cyb * im.urow;
    const uint8_t* __restrict__ va = im.v + (long)cy * im.vrow;
    const uint8_t* __restrict__ vb = im.v + (long)cyb * im.vrow;
    unsigned Y[4], U16[4], V16[4];
    if (x0 + 3 < im.w) {                                     // 4 valid pixels: chroma columns c0 - 1 .. c0 + 2 (clamped) cover them
        if (((uintptr_t)(yr + x0) & 3) == 0) {
            const uint32_t q = *(const uint32_t*)(yr + x0);
            Y[0] = q & 255u; Y[1] = (q >> 8) & 255u; Y[2] = (q >> 16) & 255u; Y[3] = q >> 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[i] = yr[x0 + i];
        }
        const int c0 = x0 >> 1;                              // c0 + 1 <= cw - 1 because x0 + 3 <= w - 1
        if (bilinear) {
            const int cm = max(c0 - 1, 0), cp = min(c0 + 2, cw - 1);
            const int col[4] = {cm, c0, c0 + 1, cp};
            unsigned tu[4], tv[4];                           // 4 * the vertically filtered column
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long o = (long)col[j] * cstep;
                tu[j] = 3u * ua[o] + ub[o];
                tv[j] = 3u * va[o] + vb[o];
            }
            U16[0] = 3u * tu[1] + tu[0]; U16[1] = 3u * tu[1] + tu[2]; U16[2] = 3u * tu[2] + tu[1]; U16[3] = 3u * tu[2] + tu[3];
            V16[0] = 3u * tv[1] + tv[0]; V16[1] = 3u * tv[1] + tv[2]; V16[2] = 3u * tv[2] + tv[1]; V16[3] = 3u * tv[2] + tv[3];
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const long o = (long)(c0 + j) * cstep;
                U16[2 * j] = U16[2 * j + 1] = 16u * ua[o];
                V16[2 * j] = V16[2 * j + 1] = 16u * va[o];
            }
        }
    } else {                                                 // at or beyond the right edge: every pixel from its nearest valid one
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xs = min(x0 + i, im.w - 1);
            Y[i] = yr[xs];
            const int cx = xs >> 1;
            const int cxb = bilinear ? min(max(cx + ((xs & 1) ? 1 : -1), 0), cw - 1) : cx;
            const long oa = (long)cx * cstep, ob = (long)cxb * cstep;
            if (bilinear) {
                U16[i] = 3u * (3u * ua[oa] + ub[oa]) + (3u * ua[ob] + ub[ob]);
                V16[i] = 3u * (3u * va[oa] + vb[oa]) + (3u * va[ob] + vb[ob]);
            } else {
                U16[i] = 16u * ua[oa];
                V16[i] = 16u * va[oa];
            }
        }
    }
    float v[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) yuv_to_rgb(Y[i], U16[i], V16[i], k, full, v[0][i], v[1][i], v[2][i]);
    float* o = dst + (long)blockIdx.y * dst_img + (long)y * W + x0;
    const long plane = (long)H * W;
    if (vec_ok) {                                            // W % 4 == 0: the quad is whole and 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) o[c * plane + i] = v[c][i];
    }
}

// rint(v), ties to even, clamped to 0..255 (v is finite: its inputs were clamped)
__device__ __forceinline__ unsigned byte_of(float v) {
    v = rintf(v);
    v = v > 0.0f ? v : 0.0f;
    v = v < 255.0f ? v : 255.0f;
    return (unsigned)(int)v;
}

__global__ __launch_bounds__(YUV_WG) void f32_to_yuv420_kernel(const float* __restrict__ src, long src_img, long src_plane, long src_row,
                                                               YuvBatch fb, int quads, int hmax2, int vec_ok, int cstep, int matrix, int full) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)hmax2 * quads) return;
    const int by = (int)(idx / quads), x0 = (int)(idx - (long)by * quads) * 4;
    const int y0 = 2 * by;
    const YuvDesc im = fb.d[blockIdx.y];
    if (y0 >= im.h || x0 >= im.w) return;                    // h and w are even: rows y0, y0 + 1 and columns x0, x0 + 1 are inside
    const YuvCoef k = yuv_coef(matrix);
    const int n = x0 + 3 < im.w ? 4 : 2;                     // valid columns of this block
    const float* __restrict__ s = src + (long)blockIdx.y * src_img + (long)y0 * src_row + x0;
    float p[3][2][4];
    if (vec_ok && n == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float4 f = *(const float4*)(s + c * src_plane + r * src_row);
                p[c][r][0] = f.x; p[c][r][1] = f.y; p[c][r][2] = f.z; p[c][r][3] = f.w;
            }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][r][i] = i < n ? s[c * src_plane + r * src_row + i] : 0.0f;
    }
    const float ys = full ? 255.0f : 219.0f, yo = full ? 0.0f : 16.0f, cs = full ? 255.0f : 224.0f;
    unsigned Yb[2][4];
    float cb[2][4], cr[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float R = clamp01(p[0][r][i]), G = clamp01(p[1][r][i]), B = clamp01(p[2][r][i]);
            const float yn = (k.kr * R + k.kg * G) + k.kb * B;
            cb[r][i] = __fdiv_rn(B - yn, k.b);
            cr[r][i] = __fdiv_rn(R - yn, k.a);
            Yb[r][i] = byte_of(yn * ys + yo);
        }
    unsigned Ub[2], Vb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float mu = ((cb[0][2 * j] + cb[0][2 * j + 1]) + (cb[1][2 * j] + cb[1][2 * j + 1])) * 0.25f;
        const float mv = ((cr[0][2 * j] + cr[0][2 * j + 1]) + (cr[1][2 * j] + cr[1][2 * j + 1])) * 0.25f;
        Ub[j] = byte_of(mu * cs + 128.0f);
        Vb[j] = byte_of(mv * cs + 128.0f);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* o = im.y + (long)(y0 + r) * im.yrow + x0;
        if (n == 4 && ((uintptr_t)o & 3) == 0) {
            *(uint32_t*)o = Yb[r][0] | (Yb[r][1] << 8) | (Yb[r][2] << 16) | (Yb[r][3] << 24);
        } else {
            for (int i = 0; i < n; ++i) o[i] = (uint8_t)Yb[r][i];
        }
    }
    const long co = (long)(x0 >> 1) * cstep;
    uint8_t* ou = im.u + (long)by * im.urow + co;
    uint8_t* ov = im.v + (long)by * im.vrow + co;
    if (cstep == 2 && n == 4 && ((uintptr_t)ou & 3) == 0) {  // NV12: U V U V is one dword
        *(uint32_t*)ou = Ub[0] | (Vb[0] << 8) | (Ub[1] << 16) | (Vb[1] << 24);
    } else {
        for (int j = 0; 2 * j < n; ++j) {
            ou[(long)j * cstep] = (uint8_t)Ub[j];
            ov[(long)j * cstep] = (uint8_t)Vb[j];
        }
    }
}

struct SsePair { const uint8_t *a, *b; long arow, brow; int h, w; };
struct SseBatch { SsePair d[SSE_CHUNK]; };

__global__ __launch_bounds__(YUV_WG) void sse_u8_kernel(SseBatch pb, unsigned long long* __restrict__ out, int chunks) {
    const SsePair pr = pb.d[blockIdx.y];
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    unsigned acc = 0;                                        // <= 16 * 255^2 per lane, <= 64 * that per wave: fits 32 bits
    const int y = (int)(idx / chunks), x0 = (int)(idx - (long)y * chunks) * 16;
    if (y < pr.h && x0 < pr.w) {                             // (no early return: every lane takes part in the wave's sum below)
        const uint8_t* __restrict__ a = pr.a + (long)y * pr.arow + x0;
        const uint8_t* __restrict__ b = pr.b + (long)y * pr.brow + x0;
        if (x0 + 15 < pr.w && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
            const uint4 va = *(const uint4*)a, vb = *(const uint4*)b;
            const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int s = 0; s < 32; s += 8) {
                    const int d = (int)((wa[j] >> s) & 255u) - (int)((wb[j] >> s) & 255u);
                    acc += (unsigned)(d * d);
                }
        } else {
            const int n = min(16, pr.w - x0);
            for (int i = 0; i < n; ++i) {
                const int d = (int)a[i] - (int)b[i];
                acc += (unsigned)(d * d);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out + blockIdx.y, (unsigned long long)acc);
}

bool yuv_enums_ok(int fmt, int matrix, int range) {
    return (fmt == LVAE_YUV_I420 || fmt == LVAE_YUV_NV12) && (matrix == LVAE_YUV_BT601 || matrix == LVAE_YUV_BT709) &&
           (range == LVAE_YUV_LIMITED || range == LVAE_YUV_FULL);
}

// The frames' descriptors are valid: planes non-null, extents even, positive and inside (H, W), rows that hold their plane's width
bool yuv_frames_ok(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, const long* y_row, const long* u_row,
                   const long* v_row, const int* hw, int B, int fmt, int H, int W) {
    const bool nv12 = fmt == LVAE_YUV_NV12;
    if (!y || !u || !y_row || !u_row || !hw || (!nv12 && (!v || !v_row))) return false;
    for (int b = 0; b < B; ++b) {
        const int h = hw[2 * b], w = hw[2 * b + 1];
        if (h <= 0 || w <= 0 || (h & 1) || (w & 1) || h > H || w > W) return false;
        if (!y[b] || !u[b] || y_row[b] < w || u_row[b] < (nv12 ? w : w / 2)) return false;
        if (!nv12 && (!v[b] || v_row[b] < w / 2)) return false;
    }
    return true;
}

YuvDesc yuv_desc(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, const long* y_row, const long* u_row,
                 const long* v_row, const int* hw, int b, int fmt) {
    const bool nv12 = fmt == LVAE_YUV_NV12;
    uint8_t* up = const_cast<uint8_t*>(u[b]);
    return {const_cast<uint8_t*>(y[b]), up, nv12 ? up + 1 : const_cast<uint8_t*>(v[b]), y_row[b], u_row[b], nv12 ? u_row[b] : v_row[b],
            hw[2 * b], hw[2 * b + 1]};
}

}  // namespace

extern "C" int lvae_image_yuv420_to_f32(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, const long* y_row,
                                        const long* u_row, const long* v_row, const int* hw, int B, int fmt, int matrix, int range,
                                        int chroma, float* dst, long dst_img, int H, int W, void* stream) {
    if (!dst || B <= 0 || H <= 0 || W <= 0 || !yuv_enums_ok(fmt, matrix, range) || (chroma != LVAE_YUV_NEAREST && chroma != LVAE_YUV_BILINEAR))
        return -22;
    const int quads = (W + 3) / 4;
    if ((long)H * quads > (long)INT_MAX || (B > 1 && dst_img < 3L * H * W)) return -22;
    if (!yuv_frames_ok(y, u, v, y_row, u_row, v_row, hw, B, fmt, H, W)) return -22;
    const int vec_ok = W % 4 == 0 && dst_img % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const unsigned gx = (unsigned)(((long)H * quads + YUV_WG - 1) / YUV_WG);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        YuvBatch fb = {};
        for (int i = 0; i < n; ++i) fb.d[i] = yuv_desc(y, u, v, y_row, u_row, v_row, hw, b0 + i, fmt);
        hipLaunchKernelGGL(yuv420_to_f32_kernel, dim3(gx, (unsigned)n), dim3(YUV_WG), 0, (hipStream_t)stream, fb, dst + (long)b0 * dst_img,
                           dst_img, H, W, quads, vec_ok, fmt == LVAE_YUV_NV12 ? 2 : 1, matrix, range == LVAE_YUV_FULL, chroma == LVAE_YUV_BILINEAR);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_image_f32_to_yuv420(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B,
                                        int fmt, int matrix, int range, uint8_t* const* y, uint8_t* const* u, uint8_t* const* v,
                                        const long* y_row, const long* u_row, const long* v_row, void* stream) {
    if (!src || B <= 0 || H <= 0 || W <= 0 || !yuv_enums_ok(fmt, matrix, range)) return -22;
    if (src_row < W || src_plane < (long)(H - 1) * src_row + W || (B > 1 && src_img < 2 * src_plane + (long)(H - 1) * src_row + W)) return -22;
    if (!yuv_frames_ok(y, u, v, y_row, u_row, v_row, hw, B, fmt, H, W)) return -22;
    int hmax = 0, wmax = 0;
    for (int b = 0; b < B; ++b) {
        hmax = hw[2 * b] > hmax ? hw[2 * b] : hmax;
        wmax = hw[2 * b + 1] > wmax ? hw[2 * b + 1] : wmax;
    }
    const int quads = (wmax + 3) / 4, hmax2 = hmax / 2;
    if ((long)hmax2 * quads > (long)INT_MAX) return -22;
    const int vec_ok = src_img % 4 == 0 && src_plane % 4 == 0 && src_row % 4 == 0 && ((uintptr_t)src & 15) == 0;
    const unsigned gx = (unsigned)(((long)hmax2 * quads + YUV_WG - 1) / YUV_WG);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        YuvBatch fb = {};
        for (int i = 0; i < n; ++i) fb.d[i] = yuv_desc(y, u, v, y_row, u_row, v_row, hw, b0 + i, fmt);
        hipLaunchKernelGGL(f32_to_yuv420_kernel, dim3(gx, (unsigned)n), dim3(YUV_WG), 0, (hipStream_t)stream, src + (long)b0 * src_img, src_img,
                           src_plane, src_row, fb, quads, hmax2, vec_ok, fmt == LVAE_YUV_NV12 ? 2 : 1, matrix, range == LVAE_YUV_FULL);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_sse_u8(const uint8_t* const* a, const long* a_row, const uint8_t* const* b, const long* b_row, const int* hw, int n,
                           uint64_t* out, void* stream) {
    if (!a || !a_row || !b || !b_row || !hw || !out || n <= 0) return -22;
    int hmax = 0, wmax = 0;
    for (int k = 0; k < n; ++k) {
        const int h = hw[2 * k], w = hw[2 * k + 1];
        if (!a[k] || !b[k] || h <= 0 || w <= 0 || a_row[k] < w || b_row[k] < w) return -22;
        hmax = h > hmax ? h : hmax;
        wmax = w > wmax ? w : wmax;
    }
    const int chunks = (wmax - 1) / 16 + 1;                  // one grid shape for every launch of the call: the largest plane's
    const long most = (long)hmax * chunks;
    if (most > (long)INT_MAX) return -22;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)n, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const unsigned gx = (unsigned)((most + YUV_WG - 1) / YUV_WG);
    for (int k0 = 0; k0 < n; k0 += SSE_CHUNK) {
        const int m = n - k0 < SSE_CHUNK ? n - k0 : SSE_CHUNK;
        SseBatch pb = {};
        for (int i = 0; i < m; ++i) {
            const int k = k0 + i;
            pb.d[i] = {a[k], b[k], a_row[k], b_row[k], hw[2 * k], hw[2 * k + 1]};
        }
        hipLaunchKernelGGL(sse_u8_kernel, dim3(gx, (unsigned)m), dim3(YUV_WG), 0, (hipStream_t)stream, pb,
                           (unsigned long long*)out + k0, chunks);
    }
    return (int)hipGetLastError();
}
