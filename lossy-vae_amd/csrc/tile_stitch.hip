// Putting decoded tiles back together (lvae/utils/tiling.py states the grid and the weights, include/lvae_hip.h the contract of
// lvae_tile_stitch): a window of the image from the fp32 reconstructions of the tiles that cover it, overlaps blended with ramp weights,
// as fp32 NCHW planes or rounded to interleaved RGB bytes.
//
// Output-centric: one lane owns 4 consecutive pixels of one window row.  It finds the tiles that cover them from the per-axis origin
// arrays (at most 3 per axis: origins ascend, a tile is at most two steps long) and accumulates their weighted values in ascending
// tile number -- no atomics, nothing depends on scheduling.  The bulk of an image is covered by one tile: there the quad is a copy,
// one 16-byte load per plane where the tile's address allows it, and a 16-byte store per plane (fp32) or 3 dwords (u8) where the
// destination's does; seams and the window's last partial quad go pixel by pixel.  Only tiles that meet the window are read, nothing
// outside the window is written.  The tile table and the origins reach the device as ONE small host-to-device copy into the caller's
// scratch, followed by ONE launch, whatever the number of tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"
#include "stitch_blend.h"

namespace {

constexpr int ST_WG = 256;

// rint(clamp(x, 0, 1) * 255), ties to even, NaN -> 0: the rounding of lvae_image_f32_to_u8
__device__ __forceinline__ unsigned unit_u8(float x) {
    x = x > 0.0f ? x : 0.0f;
    x = x < 1.0f ? x : 1.0f;
    return (unsigned)(int)rintf(x * 255.0f);
}

template <bool U8>
__global__ __launch_bounds__(ST_WG) void tile_stitch_kernel(StitchTiles a, void* dst, long dplane, long drow, int quads) {   // fp32: strides in
    const long idx = (long)blockIdx.x * ST_WG + threadIdx.x;                                                                 // elements; u8: drow in bytes
    if (idx >= (long)a.hh * quads) return;
    const int wy = (int)(idx / quads), wx = (int)(idx - (long)wy * quads) * 4;      // window coordinates of the quad
    const int y = a.y0 + wy, x = a.x0 + wx;
    const int nx = a.ww - wx < 4 ? a.ww - wx : 4;                                    // pixels of the quad inside the window
    const Cover cy = cover(a.oy, a.rows, a.th, a.ov, a.h, y);
    float v[3][4];
    int q;
    if (nx == 4 && cy.n == 1 && quad_in_one_tile(a, x, q)) {
        copy_quad(a, only(cy), q, y, x, v);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= nx) break;
            const Cover cx = cover(a.ox, a.cols, a.tw, a.ov, a.w, x + i);
            float px[3];
            blend_pixel(a, cy, cx, y, x + i, px);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][i] = px[c];
        }
    }
    if (U8) {
        uint8_t* o = (uint8_t*)dst + (long)wy * drow + 3 * wx;
        if (nx == 4 && ((uintptr_t)o & 3) == 0) {
            unsigned by[12];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) by[3 * i + c] = unit_u8(v[c][i]);
            uint32_t* o4 = (uint32_t*)o;
#pragma unroll
            for (int k = 0; k < 3; ++k) o4[k] = by[4 * k] | (by[4 * k + 1] << 8) | (by[4 * k + 2] << 16) | (by[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i < nx) o[3 * i + c] = (uint8_t)unit_u8(v[c][i]);
        }
    } else {
        float* o = (float*)dst + (long)wy * drow + wx;
        if (nx == 4 && (((uintptr_t)o | (uintptr_t)(dplane * 4)) & 15) == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *(float4*)(o + c * dplane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i < nx) o[c * dplane + i] = v[c][i];
        }
    }
}

}  // namespace

extern "C" size_t lvae_tile_stitch_workspace_bytes(int rows, int cols) { return stitch_workspace_bytes(rows, cols); }

extern "C" int lvae_tile_stitch(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols,
                                int th, int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, void* dst, long dst_plane,
                                long dst_row, int out_u8, void* ws, size_t ws_bytes, void* stream) {
    if (!dst || !stitch_tiles_ok(tiles, tile_plane, tile_row, oy, ox, rows, cols, th, tw, overlap, h, w, y0, x0, hh, ww, x0, ws, ws_bytes))
        return -22;
    if (out_u8 ? dst_row < 3L * ww : (dst_row < ww || dst_plane < (long)(hh - 1) * dst_row + ww)) return -22;
    const int quads = (ww + 3) / 4;
    if ((long)hh * quads > (long)INT_MAX) return -22;
    hipStream_t st = (hipStream_t)stream;
    StitchTiles a;
    hipError_t e = stitch_stage(tiles, tile_plane, tile_row, oy, ox, rows, cols, th, tw, overlap, h, w, y0, x0, hh, ww, ws, st, a);
    if (e != hipSuccess) return (int)e;
    const unsigned gx = (unsigned)(((long)hh * quads + ST_WG - 1) / ST_WG);
    if (out_u8)
        hipLaunchKernelGGL(tile_stitch_kernel<true>, dim3(gx), dim3(ST_WG), 0, st, a, dst, dst_plane, dst_row, quads);
    else
        hipLaunchKernelGGL(tile_stitch_kernel<false>, dim3(gx), dim3(ST_WG), 0, st, a, dst, dst_plane, dst_row, quads);
    return (int)hipGetLastError();
}
