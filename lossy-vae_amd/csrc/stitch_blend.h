// stitch_blend.h -- the tile side of the stitch kernels (tile_stitch.hip: fp32 / RGB bytes; tile_stitch_yuv.hip: YUV planes): which tiles
// cover a pixel, their ramp weights and the blended value, plus the host's checks of the tile arguments and the one copy that brings the
// tile table to the device.  One definition, so both kernels blend to the same bits (include/lvae_hip.h states the arithmetic under
// lvae_tile_stitch).  The products and sums of the blend are the __fmul_rn / __fadd_rn wrappers of the HIP headers, which carry the
// default floating-point contraction whatever pragma the including file sets: the blend rounds alike in every kernel that inlines it.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

namespace {

struct StitchTiles {
    const float* const* tiles;     // [rows * cols] device addresses, row-major; null = not decoded
    const int* oy;                 // [rows] tile origins, ascending
    const int* ox;                 // [cols]
    long plane, row;               // strides of every tile, in elements
    int rows, cols, th, tw, ov, h, w;
    int y0, x0, hh, ww;            // the window
};

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
__device__ __forceinline__ void blend_pixel(const StitchTiles& a, const Cover& cy, const Cover& cx, int y, int x, float v[3]) {
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

// Does one tile hold the 4 pixels x .. x + 3 of a row whose only row of tiles is cy's?  Then q is its column.
__device__ __forceinline__ bool quad_in_one_tile(const StitchTiles& a, int x, int& q) {
    if (a.tw < 4) return false;
    const Cover c0 = cover(a.ox, a.cols, a.tw, a.ov, a.w, x), c3 = cover(a.ox, a.cols, a.tw, a.ov, a.w, x + 3);
    if (c0.n != 1 || c3.n != 1 || only(c0) != only(c3)) return false;       // (a tile that held an inner pixel would, 4 or more wide,
    q = only(c0);                                                           // hold an end too)
    return true;
}

// The quad (y, x .. x + 3) of tile (r, q), which holds all of it: one 16-byte load per plane where the tile's address allows it
__device__ __forceinline__ void copy_quad(const StitchTiles& a, int r, int q, int y, int x, float v[3][4]) {
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

// The grid rule of lvae/utils/tiling.py::tile_grid for one axis: the origin of tile k of n.
inline bool axis_ok(const int* org, int n, int T, int ov, int size) {
    if (size <= T) return n == 1 && org[0] == 0;
    const int step = T - ov;
    if (n != (size - ov + step - 1) / step) return false;
    for (int k = 0; k < n; ++k)
        if (org[k] != (k < n - 1 ? k * step : size - T)) return false;
    return true;
}

inline size_t stitch_workspace_bytes(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)rows * cols * sizeof(void*) + ((size_t)rows + cols) * sizeof(int);
}

// The checks the stitch entries share, before any HIP call: the grid, the window, the tiles' strides, the scratch, and a tile for every
// grid cell that meets the columns xl .. x0 + ww - 1 of the window's rows (xl = x0, or x0 - 1 where the kernel reads the column before).
inline bool stitch_tiles_ok(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols, int th,
                            int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, int xl, const void* ws, size_t ws_bytes) {
    if (!tiles || !oy || !ox || !ws || rows <= 0 || cols <= 0 || th <= 0 || tw <= 0 || h <= 0 || w <= 0) return false;
    if (overlap < 0 || (h > th && overlap > th / 2) || (w > tw && overlap > tw / 2)) return false;         // (an axis with one tile: any)
    if (y0 < 0 || x0 < 0 || hh <= 0 || ww <= 0 || hh > h - y0 || ww > w - x0) return false;                 // a window outside the image
    if (tile_row < tw || tile_plane < (long)(th - 1) * tile_row + tw) return false;                         // strides that do not hold (th, tw)
    if ((long)rows * cols > (long)INT_MAX / 2 || !axis_ok(oy, rows, th, overlap, h) || !axis_ok(ox, cols, tw, overlap, w)) return false;
    if (ws_bytes < stitch_workspace_bytes(rows, cols) || ((uintptr_t)ws & 7) != 0) return false;
    for (int r = 0; r < rows; ++r) {                                                                        // every tile that meets the window
        if (oy[r] >= y0 + hh || oy[r] + th <= y0) continue;
        for (int c = 0; c < cols; ++c) {
            if (ox[c] >= x0 + ww || ox[c] + tw <= xl) continue;
            if (!tiles[r * cols + c]) return false;
        }
    }
    return true;
}

// Tile addresses, then the row and column origins: one staging buffer, one copy into ws; `a` then names them on the device.
inline hipError_t stitch_stage(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols,
                               int th, int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, void* ws, hipStream_t st,
                               StitchTiles& a) {
    const size_t n_t = (size_t)rows * cols, need = stitch_workspace_bytes(rows, cols);
    char* stage = new char[need];
    memcpy(stage, tiles, n_t * sizeof(void*));
    memcpy(stage + n_t * sizeof(void*), oy, (size_t)rows * sizeof(int));
    memcpy(stage + n_t * sizeof(void*) + (size_t)rows * sizeof(int), ox, (size_t)cols * sizeof(int));
    hipError_t e = hipMemcpyAsync(ws, stage, need, hipMemcpyHostToDevice, st);       // pageable source: staged before the call returns
    delete[] stage;
    a.tiles = (const float* const*)ws;
    a.oy = (const int*)((char*)ws + n_t * sizeof(void*));
    a.ox = a.oy + rows;
    a.plane = tile_plane; a.row = tile_row;
    a.rows = rows; a.cols = cols; a.th = th; a.tw = tw; a.ov = overlap; a.h = h; a.w = w;
    a.y0 = y0; a.x0 = x0; a.hh = hh; a.ww = ww;
    return e;
}

}  // namespace
