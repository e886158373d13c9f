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
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lvae_hip.h"

namespace {

constexpr int ST_WG = 256;

struct StitchArgs {
    const float* const* tiles;     // [rows * cols] device addresses, row-major; null = not decoded
    const int* oy;                 // [rows] tile origins, ascending
    const int* ox;                 // [cols]
    long plane, row;               // strides of every tile, in elements
    int rows, cols, th, tw, ov, h, w;
    int y0, x0, hh, ww;            // the window
    void* dst;
    long dplane, drow;             // fp32: elements; u8: drow in bytes
};

// rint(clamp(x, 0, 1) * 255), ties to even, NaN -> 0: the rounding of lvae_image_f32_to_u8
__device__ __forceinline__ unsigned unit_u8(float x) {
    x = x > 0.0f ? x : 0.0f;
    x = x < 1.0f ? x : 1.0f;
    return (unsigned)(int)rintf(x * 255.0f);
}

struct Cover { int k[3]; float wt[3]; int n; };       // slot d: candidate tile kf - 1 + d, k < 0 where it does not hold x (all loops over
                                                      // the slots are unrolled, so the arrays stay in registers); n: how many do

// The tiles of one axis that hold coordinate x with their ramp weights.  Candidates: floor(x / step) - 1 .. + 1 (origin k is at most
// k * step and above (k - 1) * step; a tile spans at most 2 steps because overlap <= T / 2).
__device__ __forceinline__ Cover cover(const int* __restrict__ org, int n, int T, int ov, int size, int x) {
    Cover c;
    c.n = 0;
    const int kf = n > 1 ? x / (T - ov) : 0;                     // (one tile: the overlap plays no part and may exceed T / 2)
    const float r = (float)(ov > 1 ? ov : 1);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int k = kf - 1 + d;
        c.k[d] = -1;
        c.wt[d] = 0.0f;
        if (k < 0 || k >= n) continue;
        const int o = org[k];
        if (o > x || x >= o + T) continue;
        const float u = (float)(x - o);
        float wl = 1.0f, wr = 1.0f;
        if (o > 0) wl = fminf(1.0f, __fdiv_rn(u + 0.5f, r));
        if (o + T < size) wr = fminf(1.0f, __fdiv_rn((float)T - u - 0.5f, r));
        c.k[d] = k;
        c.wt[d] = fminf(wl, wr);
        ++c.n;
    }
    return c;
}

__device__ __forceinline__ int only(const Cover& c) { return c.k[0] >= 0 ? c.k[0] : c.k[1] >= 0 ? c.k[1] : c.k[2]; }   // for c.n == 1

// One output pixel, all three channels: the value of its only tile, or sum(w v) / sum(w) in ascending tile number, fp32, every
// product and sum rounded on its own.
__device__ __forceinline__ void blend_pixel(const StitchArgs& a, const Cover& cy, const Cover& cx, int y, int x, float v[3]) {
    if (cy.n == 1 && cx.n == 1) {
        const int r = only(cy), q = only(cx);
        const float* p = a.tiles[r * a.cols + q] + (long)(y - a.oy[r]) * a.row + (x - a.ox[q]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = p[c * a.plane];
        return;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (cy.k[i] < 0 || cx.k[j] < 0) continue;
            const float wgt = __fmul_rn(cy.wt[i], cx.wt[j]);
            const float* p = a.tiles[cy.k[i] * a.cols + cx.k[j]] + (long)(y - a.oy[cy.k[i]]) * a.row + (x - a.ox[cx.k[j]]);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(wgt, p[c * a.plane]));
            wsum = __fadd_rn(wsum, wgt);
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(acc[c], wsum);
}

template <bool U8>
__global__ __launch_bounds__(ST_WG) void tile_stitch_kernel(StitchArgs a, int quads) {
    const long idx = (long)blockIdx.x * ST_WG + threadIdx.x;
    if (idx >= (long)a.hh * quads) return;
    const int wy = (int)(idx / quads), wx = (int)(idx - (long)wy * quads) * 4;      // window coordinates of the quad
    const int y = a.y0 + wy, x = a.x0 + wx;
    const int nx = a.ww - wx < 4 ? a.ww - wx : 4;                                    // pixels of the quad inside the window
    const Cover cy = cover(a.oy, a.rows, a.th, a.ov, a.h, y);
    float v[3][4];
    bool whole = false;
    if (nx == 4 && cy.n == 1 && a.tw >= 4) {
        const Cover c0 = cover(a.ox, a.cols, a.tw, a.ov, a.w, x), c3 = cover(a.ox, a.cols, a.tw, a.ov, a.w, x + 3);
        if (c0.n == 1 && c3.n == 1 && only(c0) == only(c3)) {                         // one tile holds the quad (a tile that held an inner
            whole = true;                                                            // pixel would, 4 or more wide, hold an end too)
            const int r = only(cy), q = only(c0);
            const float* p = a.tiles[r * a.cols + q] + (long)(y - a.oy[r]) * a.row + (x - a.ox[q]);
            if ((((uintptr_t)p | (uintptr_t)(a.plane * 4)) & 15) == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 f = *(const float4*)(p + c * a.plane);
                    v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[c][i] = p[c * a.plane + i];
            }
        }
    }
    if (!whole) {
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
        uint8_t* o = (uint8_t*)a.dst + (long)wy * a.drow + 3 * wx;
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
        float* o = (float*)a.dst + (long)wy * a.drow + wx;
        if (nx == 4 && (((uintptr_t)o | (uintptr_t)(a.dplane * 4)) & 15) == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *(float4*)(o + c * a.dplane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i < nx) o[c * a.dplane + i] = v[c][i];
        }
    }
}

// The grid rule of lvae/utils/tiling.py::tile_grid for one axis: the origin of tile k of n.
bool axis_ok(const int* org, int n, int T, int ov, int size) {
    if (size <= T) return n == 1 && org[0] == 0;
    const int step = T - ov;
    if (n != (size - ov + step - 1) / step) return false;
    for (int k = 0; k < n; ++k)
        if (org[k] != (k < n - 1 ? k * step : size - T)) return false;
    return true;
}

}  // namespace

extern "C" size_t lvae_tile_stitch_workspace_bytes(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)rows * cols * sizeof(void*) + ((size_t)rows + cols) * sizeof(int);
}

extern "C" int lvae_tile_stitch(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols,
                                int th, int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, void* dst, long dst_plane,
                                long dst_row, int out_u8, void* ws, size_t ws_bytes, void* stream) {
    if (!tiles || !oy || !ox || !dst || !ws || rows <= 0 || cols <= 0 || th <= 0 || tw <= 0 || h <= 0 || w <= 0) return -22;
    if (overlap < 0 || (h > th && overlap > th / 2) || (w > tw && overlap > tw / 2)) return -22;          // (an axis with one tile: any)
    if (y0 < 0 || x0 < 0 || hh <= 0 || ww <= 0 || hh > h - y0 || ww > w - x0) return -22;                  // a window outside the image
    if (tile_row < tw || tile_plane < (long)(th - 1) * tile_row + tw) return -22;                          // strides that do not hold (th, tw)
    if (out_u8 ? dst_row < 3L * ww : (dst_row < ww || dst_plane < (long)(hh - 1) * dst_row + ww)) return -22;
    if ((long)rows * cols > (long)INT_MAX / 2 || !axis_ok(oy, rows, th, overlap, h) || !axis_ok(ox, cols, tw, overlap, w)) return -22;
    const size_t need = lvae_tile_stitch_workspace_bytes(rows, cols);
    if (ws_bytes < need || ((uintptr_t)ws & 7) != 0) return -22;
    for (int r = 0; r < rows; ++r) {                                                                       // every tile that meets the window
        if (oy[r] >= y0 + hh || oy[r] + th <= y0) continue;
        for (int c = 0; c < cols; ++c) {
            if (ox[c] >= x0 + ww || ox[c] + tw <= x0) continue;
            if (!tiles[r * cols + c]) return -22;
        }
    }
    const int quads = (ww + 3) / 4;
    if ((long)hh * quads > (long)INT_MAX) return -22;

    // tile addresses, then the row and column origins: one staging buffer, one copy
    const size_t n_t = (size_t)rows * cols;
    char* stage = new char[need];
    memcpy(stage, tiles, n_t * sizeof(void*));
    memcpy(stage + n_t * sizeof(void*), oy, (size_t)rows * sizeof(int));
    memcpy(stage + n_t * sizeof(void*) + (size_t)rows * sizeof(int), ox, (size_t)cols * sizeof(int));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws, stage, need, hipMemcpyHostToDevice, st);       // pageable source: staged before the call returns
    delete[] stage;
    if (e != hipSuccess) return (int)e;

    StitchArgs a;
    a.tiles = (const float* const*)ws;
    a.oy = (const int*)((char*)ws + n_t * sizeof(void*));
    a.ox = a.oy + rows;
    a.plane = tile_plane; a.row = tile_row;
    a.rows = rows; a.cols = cols; a.th = th; a.tw = tw; a.ov = overlap; a.h = h; a.w = w;
    a.y0 = y0; a.x0 = x0; a.hh = hh; a.ww = ww;
    a.dst = dst; a.dplane = dst_plane; a.drow = dst_row;
    const unsigned gx = (unsigned)(((long)hh * quads + ST_WG - 1) / ST_WG);
    if (out_u8)
        hipLaunchKernelGGL(tile_stitch_kernel<true>, dim3(gx), dim3(ST_WG), 0, st, a, quads);
    else
        hipLaunchKernelGGL(tile_stitch_kernel<false>, dim3(gx), dim3(ST_WG), 0, st, a, quads);
    return (int)hipGetLastError();
}
