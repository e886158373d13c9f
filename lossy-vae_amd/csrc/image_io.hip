// 8-bit images in and out of the codec on the device: interleaved RGB bytes (HWC) -> the fp32 NCHW planes an encode plan reads
// (replicate-padded to the plan's canvas), and fp32 NCHW reconstructions -> interleaved RGB bytes.  include/lvae_hip.h
// (lvae_image_u8_to_f32 / lvae_image_f32_to_u8) states the contract.
//
// Both are streaming kernels: one lane owns 4 consecutive pixels of one row -- 12 interleaved bytes on the u8 side, one float4 per plane
// on the fp32 side.  The u8 side moves as 3 dwords when the 12 bytes start on a dword boundary (rows of 3*w bytes and view offsets
// generally do not), as bytes otherwise; the fp32 side as 16-byte vectors when base, strides and width allow it, as scalars otherwise.
// Nothing outside an image's extent is read or written.  Up to IMG_CHUNK images go into one launch: their descriptors (pointer, row
// stride, extent) travel in the kernel arguments, so a call copies nothing to the device and needs no scratch.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"

namespace {

constexpr int IMG_CHUNK = 16;                                // images per launch
constexpr int IMG_WG = 256;

struct ImgDesc { uint8_t* p; long row; int h, w; };          // one u8 image: base, row stride in bytes, valid extent
struct ImgBatch { ImgDesc d[IMG_CHUNK]; };

// v / 255 with the bits of torch's .to(float32).div(255): an IEEE division (v * (1 / 255.f) differs in 126 of the 256 values)
__device__ __forceinline__ float u8_unit(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

// rint(clamp(x, 0, 1) * 255): the product in fp32, ties to even; NaN -> 0 (both comparisons are false for a NaN)
__device__ __forceinline__ unsigned unit_u8(float x) {
    x = x > 0.0f ? x : 0.0f;
    x = x < 1.0f ? x : 1.0f;
    return (unsigned)(int)rintf(x * 255.0f);
}

__global__ __launch_bounds__(IMG_WG) void image_u8_to_f32_kernel(ImgBatch ib, float* __restrict__ dst, long dst_img, int H, int W, int quads,
                                                                 int vec_ok) {
    const long idx = (long)blockIdx.x * IMG_WG + threadIdx.x;
    if (idx >= (long)H * quads) return;
    const int y = (int)(idx / quads), x0 = (int)(idx - (long)y * quads) * 4;
    const ImgDesc im = ib.d[blockIdx.y];
    const uint8_t* __restrict__ row = im.p + (long)min(y, im.h - 1) * im.row;
    float v[3][4];
    if (x0 + 3 < im.w) {                                     // 4 valid pixels: 12 bytes of this row, all inside the extent
        const uint8_t* s = row + 3 * x0;
        unsigned by[12];
        if (((uintptr_t)s & 3) == 0) {
            const uint32_t* s4 = (const uint32_t*)s;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t u = s4[k];
                by[4 * k] = u & 255u; by[4 * k + 1] = (u >> 8) & 255u; by[4 * k + 2] = (u >> 16) & 255u; by[4 * k + 3] = u >> 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) by[k] = s[k];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][i] = u8_unit(by[3 * i + c]);
    } else {                                                 // at or beyond the right edge: the nearest valid pixel of the row
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint8_t* s = row + 3 * min(x0 + i, im.w - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][i] = u8_unit(s[c]);
        }
    }
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

__global__ __launch_bounds__(IMG_WG) void image_f32_to_u8_kernel(const float* __restrict__ src, long src_img, long src_plane, long src_row,
                                                                 ImgBatch ib, int quads, int hmax, int vec_ok) {
    const long idx = (long)blockIdx.x * IMG_WG + threadIdx.x;
    if (idx >= (long)hmax * quads) return;
    const int y = (int)(idx / quads), x0 = (int)(idx - (long)y * quads) * 4;
    const ImgDesc im = ib.d[blockIdx.y];
    if (y >= im.h || x0 >= im.w) return;
    const float* __restrict__ s = src + (long)blockIdx.y * src_img + (long)y * src_row + x0;
    uint8_t* o = im.p + (long)y * im.row + 3 * x0;
    if (x0 + 3 < im.w) {
        float v[3][4];
        if (vec_ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 f = *(const float4*)(s + c * src_plane);
                v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = s[c * src_plane + i];
        }
        unsigned by[12];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) by[3 * i + c] = unit_u8(v[c][i]);
        if (((uintptr_t)o & 3) == 0) {
            uint32_t* o4 = (uint32_t*)o;
#pragma unroll
            for (int k = 0; k < 3; ++k) o4[k] = by[4 * k] | (by[4 * k + 1] << 8) | (by[4 * k + 2] << 16) | (by[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = (uint8_t)by[k];
        }
    } else {                                                 // the last, partial quad of a row
        for (int i = 0; x0 + i < im.w; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * i + c] = (uint8_t)unit_u8(s[c * src_plane + i]);
    }
}

}  // namespace

extern "C" int lvae_image_u8_to_f32(const uint8_t* const* src, const long* src_row, const int* hw, int B, float* dst, long dst_img, int H,
                                    int W, void* stream) {
    if (!src || !src_row || !hw || !dst || B <= 0 || H <= 0 || W <= 0) return -22;
    const int quads = (W + 3) / 4;
    if ((long)H * quads > (long)INT_MAX || (B > 1 && dst_img < 3L * H * W)) return -22;
    for (int b = 0; b < B; ++b) {
        const int h = hw[2 * b], w = hw[2 * b + 1];
        if (!src[b] || h <= 0 || w <= 0 || h > H || w > W || src_row[b] < 3L * w) return -22;
    }
    const int vec_ok = W % 4 == 0 && dst_img % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const unsigned gx = (unsigned)(((long)H * quads + IMG_WG - 1) / IMG_WG);
    for (int b0 = 0; b0 < B; b0 += IMG_CHUNK) {
        const int n = B - b0 < IMG_CHUNK ? B - b0 : IMG_CHUNK;
        ImgBatch ib = {};
        for (int i = 0; i < n; ++i) ib.d[i] = {const_cast<uint8_t*>(src[b0 + i]), src_row[b0 + i], hw[2 * (b0 + i)], hw[2 * (b0 + i) + 1]};
        hipLaunchKernelGGL(image_u8_to_f32_kernel, dim3(gx, (unsigned)n), dim3(IMG_WG), 0, (hipStream_t)stream, ib, dst + (long)b0 * dst_img,
                           dst_img, H, W, quads, vec_ok);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_image_f32_to_u8(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B,
                                    uint8_t* const* dst, const long* dst_row, void* stream) {
    if (!src || !hw || !dst || !dst_row || B <= 0 || H <= 0 || W <= 0) return -22;
    if (src_row < W || src_plane < (long)(H - 1) * src_row + W || (B > 1 && src_img < 2 * src_plane + (long)(H - 1) * src_row + W)) return -22;
    int hmax = 0, wmax = 0;
    for (int b = 0; b < B; ++b) {
        const int h = hw[2 * b], w = hw[2 * b + 1];
        if (!dst[b] || h <= 0 || w <= 0 || h > H || w > W || dst_row[b] < 3L * w) return -22;
        hmax = h > hmax ? h : hmax;
        wmax = w > wmax ? w : wmax;
    }
    const int quads = (wmax + 3) / 4;
    if ((long)hmax * quads > (long)INT_MAX) return -22;
    const int vec_ok = src_img % 4 == 0 && src_plane % 4 == 0 && src_row % 4 == 0 && ((uintptr_t)src & 15) == 0;
    const unsigned gx = (unsigned)(((long)hmax * quads + IMG_WG - 1) / IMG_WG);
    for (int b0 = 0; b0 < B; b0 += IMG_CHUNK) {
        const int n = B - b0 < IMG_CHUNK ? B - b0 : IMG_CHUNK;
        ImgBatch ib = {};
        for (int i = 0; i < n; ++i) ib.d[i] = {dst[b0 + i], dst_row[b0 + i], hw[2 * (b0 + i)], hw[2 * (b0 + i) + 1]};
        hipLaunchKernelGGL(image_f32_to_u8_kernel, dim3(gx, (unsigned)n), dim3(IMG_WG), 0, (hipStream_t)stream, src + (long)b0 * src_img,
                           src_img, src_plane, src_row, ib, quads, hmax, vec_ok);
    }
    return (int)hipGetLastError();
}
