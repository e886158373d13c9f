// Decoded tiles straight into YUV planes (include/lvae_hip.h states the contract of lvae_tile_stitch_yuv): a window of a tiled image as
// the planes of a frame -- planar or semi-planar, 8 / 10 / 12 bits, 4:2:0 / 4:2:2 / 4:4:4, centre- or left-sited chroma -- with no fp32 image
// in between.  It is the composition of two existing kernels with the memory between them taken out, and gives their bits:
// tile_stitch_kernel<fp32> (tile_stitch.hip) followed by f32_to_yuv_kernel (yuv_io.hip) on the window.
//
// One lane owns the block f32_to_yuv_kernel's lane owns: (2 or 1 rows) x 4 columns of the window, plus, where the chroma is left-sited,
// the column before it.  Its RGB values come from the stitch's blend (stitch_blend.h) where the other kernel loads them from an image:
// per row, one 16-byte load per plane where a single tile holds the quad, pixel by pixel through blend_pixel on seams and in the window's
// last partial quad.  From there on it is yuv_block_store (yuv_convert.h): matrix, chroma down-sampling, rounding, stores.  The two
// halves round differently on purpose: the blend under the default contraction, as in lvae_tile_stitch (its products and sums are the HIP
// headers' wrappers, which fuse), the conversion with contraction off (each function of yuv_convert.h says so in its body), and this
// kernel's own body has no floating-point arithmetic.
//
// Left siting, window column 0 with x0 > 0: the column before is column x0 - 1 OF THE IMAGE, blended like any other pixel, so a window is
// the crop of the full frame; the host refuses a window whose column x0 - 1 lies in a tile that was not decoded.
// The tile table and the origins reach the device as lvae_tile_stitch's do: one small copy into the caller's scratch, one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"
#include "stitch_blend.h"
#include "yuv_convert.h"

namespace {

constexpr int SY_WG = 256;

// the window's planes: row strides in samples; semi-planar: u is the UV plane, v is not read
struct YuvDst { void *y, *u, *v; long yrow, urow, vrow; };

template <typename T, int SX, int SY, int LEFT, int SP = 0>
__global__ __launch_bounds__(SY_WG) void tile_stitch_yuv_kernel(StitchTiles a, YuvDst d, int quads, int hblocks, YuvParams k) {
    constexpr int R = SY ? 2 : 1;                            // rows of a block
    const long idx = (long)blockIdx.x * SY_WG + threadIdx.x;
    if (idx >= (long)hblocks * quads) return;
    const int by = (int)(idx / quads), wx = (int)(idx - (long)by * quads) * 4;       // window coordinates of the block
    const int wy = by << SY;
    const int y = a.y0 + wy, x = a.x0 + wx;                  // hh (ww) is even where subsampled: the block's R rows (a column pair) are inside
    const int n = a.ww - wx < 4 ? a.ww - wx : 4;             // columns of the block inside the window (2 or 4 where SX)
    Cover cy[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cy[r] = cover(a.oy, a.rows, a.th, a.ov, a.h, y + r);
    int q = 0;
    const bool xwhole = n == 4 && quad_in_one_tile(a, x, q);
    float p[3][R][4];
    bool seam = !xwhole;                                     // a row of the block that is not one tile's
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (xwhole && cy[r].n == 1) {
            float v[3][4];
            copy_quad(a, only(cy[r]), q, y + r, x, v);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) p[c][r][i] = v[c][i];
        } else {
            seam = true;
        }
    }
    if (seam) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {
                const Cover cx = cover(a.ox, a.cols, a.tw, a.ov, a.w, x + i);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (xwhole && cy[r].n == 1) continue;
                    float px[3];
                    blend_pixel(a, cy[r], cx, y + r, x + i, px);
#pragma unroll
                    for (int c = 0; c < 3; ++c) p[c][r][i] = px[c];
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) p[c][r][i] = 0.0f;       // beyond the window: computed on, never stored
            }
        }
    }
    [[maybe_unused]] float pl[3][R];                         // left siting: image column max(x - 1, 0), another lane's pixel or, at the
    if constexpr (SX && LEFT) {                              // window's first column, one outside the window
        if (x > 0) {
            const Cover cx = cover(a.ox, a.cols, a.tw, a.ov, a.w, x - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float px[3];
                blend_pixel(a, cy[r], cx, y + r, x - 1, px);
#pragma unroll
                for (int c = 0; c < 3; ++c) pl[c][r] = px[c];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) pl[c][r] = p[c][r][0];
        }
    }
    yuv_block_store<T, SX, SY, LEFT, SP>(p, pl, n, k, (T*)d.y + (long)wy * d.yrow + wx, d.yrow, (T*)d.u + (long)by * d.urow + (SP ? wx : wx >> SX),
                                         (T*)d.v + (long)by * d.vrow + (wx >> SX));
}

}  // namespace

extern "C" int lvae_tile_stitch_yuv(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols,
                                    int th, int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, int depth, int subsampling,
                                    int siting, int matrix, int range, int layout, void* y, void* u, void* v, long y_row, long u_row, long v_row,
                                    void* ws, size_t ws_bytes, void* stream) {
    if (!enums_ok(depth, subsampling, siting, matrix, range) || (layout != LVAE_YUV_LAYOUT_PLANAR && layout != LVAE_YUV_LAYOUT_SEMIPLANAR)) return -22;
    const int sp = layout == LVAE_YUV_LAYOUT_SEMIPLANAR;
    if (sp && (depth == 8 ? subsampling != LVAE_YUV_SUB_420 || siting != LVAE_YUV_SITING_CENTER || matrix == LVAE_YUV_BT2020       // NV12: what
                          : !sp_layout_ok(depth, subsampling)))                                                                  // lvae_image_f32_to_yuv420 has
        return -22;
    const int sx = subsampling != LVAE_YUV_SUB_444, sy = subsampling == LVAE_YUV_SUB_420;
    if ((sy && ((y0 | hh) & 1)) || (sx && ((x0 | ww) & 1))) return -22;                                      // a window off the chroma grid
    const int left = sx && siting == LVAE_YUV_SITING_LEFT;
    if (!y || !u || (!sp && !v) ||
        !stitch_tiles_ok(tiles, tile_plane, tile_row, oy, ox, rows, cols, th, tw, overlap, h, w, y0, x0, hh, ww, left && x0 > 0 ? x0 - 1 : x0, ws,
                         ws_bytes))
        return -22;
    if (y_row < ww || u_row < (sp ? ww : ww >> sx) || (!sp && v_row < (ww >> sx))) return -22;                // strides that do not hold the window
    const int quads = (ww + 3) / 4, hblocks = hh >> sy;
    if ((long)hblocks * quads > (long)INT_MAX) return -22;
    hipStream_t st = (hipStream_t)stream;
    StitchTiles a;
    hipError_t e = stitch_stage(tiles, tile_plane, tile_row, oy, ox, rows, cols, th, tw, overlap, h, w, y0, x0, hh, ww, ws, st, a);
    if (e != hipSuccess) return (int)e;
    const YuvDst d = {y, u, sp ? u : v, y_row, u_row, sp ? u_row : v_row};
    const unsigned gx = (unsigned)(((long)hblocks * quads + SY_WG - 1) / SY_WG);
    auto kernel = YUV_PICK(tile_stitch_yuv_kernel, depth, subsampling, siting == LVAE_YUV_SITING_LEFT, sp);
    hipLaunchKernelGGL(kernel, dim3(gx), dim3(SY_WG), 0, st, a, d, quads, hblocks, yuv_params(matrix, range, depth));
    return (int)hipGetLastError();
}
