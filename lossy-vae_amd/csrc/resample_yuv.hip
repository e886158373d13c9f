// Reduced-resolution coding of YUV frames: the resampler of resample.hip fused with the two colour conversions of yuv_io.hip
// (include/lvae_hip.h -- lvae_resample_yuv_to_f32 / lvae_resample_f32_to_yuv -- the contract).  Neither direction puts a full-resolution
// fp32 RGB image into memory, and each gives the bits of the composition of the existing entries:
//   in :  lvae_image_yuv*_to_f32 into an (h_in, w_in) canvas, then lvae_resample_f32(clamp = 1) into the canvas (H, W);
//   out:  lvae_resample_f32(clamp = 0) into an (h_out, w_out) image, then lvae_image_f32_to_yuv*.
// The geometry, the tables, the tile (RS_TY x TX outputs per workgroup, the horizontally filtered rows in LDS, 64 KiB at most) and the two
// passes -- fp32 fmaf, taps ascending, from 0 -- are resample.hip's; the conversions are the single definitions of yuv_fetch.h (one
// pixel's codes -> RGB) and yuv_convert.h (a lane's block of RGB -> codes and stores).
//
// In.  A source pixel is converted ONCE per tile and source row, not once per tap: the source columns the tile's outputs read --
// xstart[first] .. xstart[last] + xtaps, at most cap_cols, which the host bounds from `xspan` -- are converted RY_SR rows at a time into
// an LDS staging buffer (one lane per source pixel: its codes with the chroma filter on integers, three IEEE divisions, the matrix, the
// clamp), and the horizontal pass reads the staging buffer.  The vertical pass, the clamp and the replicate padding follow unchanged.
//
// Out.  Phase 1 is the horizontal pass over the fp32 source (a strided NCHW view: the decoder's padded batch, read in place).  In phase 2
// one lane owns the block f32_to_yuv_kernel's lane owns -- (2 or 1 rows) x 4 columns -- runs the vertical pass for its pixels, unclamped,
// and hands them to yuv_block_store.  RS_TY is even and TX a multiple of 8, so a block never straddles tiles; with left-sited chroma a
// block's first chroma sample reads the column before it, so phase 1 filters one more column on the tile's left.  (A 16 x 32 tile has 64
// to 128 blocks for 256 lanes.  Running the vertical pass one pixel per lane into LDS first, and the blocks after a barrier, kept every
// lane busy and was measured 3 to 6 % SLOWER on 2160p frames (README); presumably the other workgroups of the CU fill the idle lanes.)
//
// Every table entry, row and column index is clamped to its extent before use, and every LDS index to what was filled: no table, however
// wrong, reads or writes outside an extent.  No atomics: two calls give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"
#include "yuv_convert.h"
#include "yuv_fetch.h"

namespace {

constexpr int RS_WG = 256;
constexpr int RS_TY = 16;                                    // output rows of a tile
constexpr int RS_MAX_TAPS = 64;
constexpr int RS_MAX_RATIO = 8;
constexpr long RS_LDS_BYTES = 64 * 1024;                     // per workgroup: two or more fit a CU's 160 KiB
constexpr int RY_SR = 8;                                     // source rows converted per staging step: 8 x 32 outputs, one per lane
constexpr int RY_XSPAN_OUTPUTS = 8;                          // `xspan` is the span of this many consecutive outputs

struct RyTables {
    const int* ystart; const float* ywgt; const int* xstart; const float* xwgt;
    int ytaps, xtaps;                                        // 0: the axis is not filtered
    int h_in, w_in, h_out, w_out, H, W;                      // (H, W): the destination's canvas, >= (h_out, w_out) (out: equal)
    int tx, cap_rows, cap_cols;
};
struct RyIn { PlaneBatch fb; RyTables t; float* dst; long d_img; YuvParams k; int bilinear; };
struct RyOut { PlaneBatch fb; RyTables t; const float* src; long s_img, s_plane, s_row; YuvParams k; };

// the input rows of a tile: those of its first and last source rows of the destination (rows below h_out repeat row h_out - 1)
__device__ __forceinline__ void tile_rows(const RyTables& t, int ty0, int th, int& row_lo, int& nrows) {
    const int oy_first = min(ty0, t.h_out - 1), oy_last = min(ty0 + th - 1, t.h_out - 1);
    int row_hi;
    if (t.ytaps) {
        row_lo = t.ystart[oy_first];
        row_hi = t.ystart[oy_last] + t.ytaps;
    } else {
        row_lo = oy_first;
        row_hi = oy_last + 1;
    }
    row_lo = max(0, min(row_lo, t.h_in - 1));
    nrows = max(1, min(min(row_hi, t.h_in) - row_lo, t.cap_rows));
}

template <typename T, int SX, int SY, int LEFT, int SP = 0>
__global__ __launch_bounds__(RS_WG) void resample_yuv_in_kernel(RyIn a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RyTables& t = a.t;
    float* stage = smem;                                     // [RY_SR][3][cap_cols] converted source pixels
    float* rows = smem + RY_SR * 3 * t.cap_cols;             // [nrows][3][TX] horizontally filtered input rows
    const int tid = threadIdx.x, TX = t.tx, SC = t.cap_cols, b = blockIdx.z;
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * RS_TY;
    const int tw = min(TX, t.W - tx0), th = min(RS_TY, t.H - ty0);
    int row_lo, nrows;
    tile_rows(t, ty0, th, row_lo, nrows);
    // the source columns of this tile: those of its first and last source columns of the destination (columns beyond w_out repeat column w_out - 1)
    const int ox_first = min(tx0, t.w_out - 1), ox_last = min(tx0 + tw - 1, t.w_out - 1);
    int col_lo, col_hi;
    if (t.xtaps) {
        col_lo = t.xstart[ox_first];
        col_hi = t.xstart[ox_last] + t.xtaps;
    } else {
        col_lo = ox_first;
        col_hi = ox_last + 1;
    }
    col_lo = max(0, min(col_lo, t.w_in - 1));
    const int ncols = max(1, min(min(col_hi, t.w_in) - col_lo, SC));
    const PlaneDesc im = a.fb.d[b];

    for (int r0 = 0; r0 < nrows; r0 += RY_SR) {
        const int nr = min(RY_SR, nrows - r0);
        // ---- staging: source rows row_lo + r0 .. + nr at columns col_lo .. + ncols, converted once
        for (int idx = tid; idx < nr * ncols; idx += RS_WG) {
            const int r = idx / ncols, c = idx - r * ncols;
            const int ys = min(row_lo + r0 + r, t.h_in - 1), xs = min(col_lo + c, t.w_in - 1);
            const YuvRows<T> rw = yuv_rows<T, SX, SY>(im, ys, a.bilinear);
            unsigned Y, CU, CV;
            yuv_pixel_codes<T, SX, SY, LEFT, SP>(rw, xs, a.bilinear, a.k, Y, CU, CV);
            float v[3];
            yuv_codes_to_rgb<SX, SY>(Y, CU, CV, a.k, v[0], v[1], v[2]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) stage[(r * 3 + ch) * SC + c] = v[ch];
        }
        __syncthreads();
        // ---- phase 1: horizontal pass of those rows at the tile's columns
        for (int idx = tid; idx < nr * TX; idx += RS_WG) {
            const int r = idx / TX, x = idx - r * TX;
            if (x >= tw) continue;
            const int ox = min(tx0 + x, t.w_out - 1);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            const int taps = t.xtaps ? t.xtaps : 1;
            const int s = t.xtaps ? t.xstart[ox] : ox;
            const float* __restrict__ wr = t.xwgt + (long)ox * t.xtaps;
            for (int j = 0; j < taps; ++j) {
                const int xi = max(0, min(max(0, min(s + j, t.w_in - 1)) - col_lo, ncols - 1));
                if (t.xtaps) {
                    const float w = wr[j];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(w, stage[(r * 3 + ch) * SC + xi], acc[ch]);
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = stage[(r * 3 + ch) * SC + xi];
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rows[((long)(r0 + r) * 3 + ch) * TX + x] = acc[ch];
        }
        __syncthreads();
    }

    // ---- phase 2: vertical pass out of LDS, one destination pixel (3 channels) per step
    for (int idx = tid; idx < th * TX; idx += RS_WG) {
        const int ty = idx / TX, x = idx - ty * TX;
        if (x >= tw) continue;
        const int y = ty0 + ty, oy = min(y, t.h_out - 1);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        if (t.ytaps) {
            const int s = t.ystart[oy];
            const float* __restrict__ wr = t.ywgt + (long)oy * t.ytaps;
            for (int j = 0; j < t.ytaps; ++j) {
                const int r = max(0, min(min(s + j, t.h_in - 1) - row_lo, nrows - 1));
                const float w = wr[j];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(w, rows[((long)r * 3 + ch) * TX + x], acc[ch]);
            }
        } else {
            const int r = max(0, min(oy - row_lo, nrows - 1));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] = rows[((long)r * 3 + ch) * TX + x];
        }
        float* o = a.dst + (long)b * a.d_img + (long)y * t.W + (tx0 + x);
        const long plane = (long)t.H * t.W;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch * plane] = clamp01(acc[ch]);
    }
}

template <typename T, int SX, int SY, int LEFT, int SP = 0>
__global__ __launch_bounds__(RS_WG) void resample_yuv_out_kernel(RyOut a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = SY ? 2 : 1;                            // rows of a lane's block
    constexpr int E = (SX && LEFT) ? 1 : 0;                  // columns filtered on the tile's left: the column before its first block
    const RyTables& t = a.t;
    float* rows = smem;                                      // [nrows][3][TX + E]: LDS column E + x is tile column x
    const int tid = threadIdx.x, TX = t.tx, TXS = TX + E, b = blockIdx.z;
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * RS_TY;
    const int tw = min(TX, t.w_out - tx0), th = min(RS_TY, t.h_out - ty0);
    int row_lo, nrows;
    tile_rows(t, ty0, th, row_lo, nrows);
    const float* __restrict__ sf = a.src + (long)b * a.s_img;

    // ---- phase 1: horizontal pass of rows row_lo .. row_lo + nrows - 1 at the tile's columns (and, E, the one before them)
    for (int idx = tid; idx < nrows * TXS; idx += RS_WG) {
        const int r = idx / TXS, xe = idx - r * TXS;
        if (xe >= tw + E) continue;
        const int ox = max(0, min(tx0 - E + xe, t.w_out - 1)), y = row_lo + r;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        const int taps = t.xtaps ? t.xtaps : 1;
        const int s = t.xtaps ? t.xstart[ox] : ox;
        const float* __restrict__ wr = t.xwgt + (long)ox * t.xtaps;
        for (int j = 0; j < taps; ++j) {
            const int xi = max(0, min(s + j, t.w_in - 1));
            const float* p = sf + (long)y * a.s_row + xi;
            float v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = p[ch * a.s_plane];
            if (t.xtaps) {
                const float w = wr[j];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(w, v[ch], acc[ch]);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = v[ch];
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rows[((long)r * 3 + ch) * TXS + xe] = acc[ch];
    }
    __syncthreads();

    // ---- phase 2: one block of R rows x 4 columns per step: the vertical pass of its pixels, unclamped, then the codes and the stores
    const PlaneDesc im = a.fb.d[b];
    const int nbx = TX / 4;
    for (int idx = tid; idx < (RS_TY / R) * nbx; idx += RS_WG) {
        const int by = idx / nbx, xl = (idx - by * nbx) * 4;
        const int y0 = ty0 + by * R, x0 = tx0 + xl;
        if (y0 >= t.h_out || x0 >= t.w_out) continue;        // h_out (w_out) is even where subsampled: the block's R rows (a column pair) are inside
        const int n = min(4, t.w_out - x0);                  // valid columns of this block (2 or 4 where SX)
        int col[5];                                          // LDS columns of the block's pixels (beyond n: the last valid one, not used) and of pl
#pragma unroll
        for (int i = 0; i < 4; ++i) col[i] = E + min(xl + i, tw - 1);
        col[4] = x0 > 0 ? E + xl - 1 : E + xl;               // left siting: column max(x0 - 1, 0) (E == 1 there: the index is >= 0)
        float p[3][R][4];
        [[maybe_unused]] float pl[3][R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int oy = min(y0 + r, t.h_out - 1);
            float acc[3][5];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int i = 0; i < 5; ++i) acc[ch][i] = 0.0f;
            if (t.ytaps) {
                const int s = t.ystart[oy];
                const float* __restrict__ wr = t.ywgt + (long)oy * t.ytaps;
                for (int j = 0; j < t.ytaps; ++j) {
                    const int rr = max(0, min(min(s + j, t.h_in - 1) - row_lo, nrows - 1));
                    const float w = wr[j];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                        for (int i = 0; i < 4 + E; ++i) acc[ch][i] = fmaf(w, rows[((long)rr * 3 + ch) * TXS + col[i]], acc[ch][i]);
                }
            } else {
                const int rr = max(0, min(oy - row_lo, nrows - 1));
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int i = 0; i < 4 + E; ++i) acc[ch][i] = rows[((long)rr * 3 + ch) * TXS + col[i]];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[ch][r][i] = i < n ? acc[ch][i] : 0.0f;
                pl[ch][r] = acc[ch][4];
            }
        }
        const int cy = y0 >> SY;
        yuv_block_store<T, SX, SY, LEFT, SP>(p, pl, n, a.k, (T*)im.y + (long)y0 * im.yrow + x0, im.yrow,
                                             (T*)im.u + (long)cy * im.urow + (SP ? x0 : x0 >> SX), (T*)im.v + (long)cy * im.vrow + (x0 >> SX));
    }
}

// The checks the two entries share; fills the geometry and the tables of `t` (not the tile).  -> 0 or -22
int tables_setup(RyTables& t, int B, int h_in, int w_in, int h_out, int w_out, const int* ystart, const float* ywgt, int ytaps, int yspan,
                 const int* xstart, const float* xwgt, int xtaps, int H, int W) {
    if (B <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || H < h_out || W < w_out) return -22;
    if (ytaps < 0 || ytaps > RS_MAX_TAPS || xtaps < 0 || xtaps > RS_MAX_TAPS) return -22;
    if (ytaps ? (!ystart || !ywgt || yspan <= 0) : (h_out != h_in || ystart || ywgt)) return -22;
    if (xtaps ? (!xstart || !xwgt) : (w_out != w_in || xstart || xwgt)) return -22;
    if ((long)h_in > (long)RS_MAX_RATIO * h_out || (long)h_out > (long)RS_MAX_RATIO * h_in || (long)w_in > (long)RS_MAX_RATIO * w_out ||
        (long)w_out > (long)RS_MAX_RATIO * w_in)
        return -22;
    t.ystart = ystart; t.ywgt = ywgt; t.xstart = xstart; t.xwgt = xwgt;
    t.ytaps = ytaps; t.xtaps = xtaps;
    t.h_in = h_in; t.w_in = w_in; t.h_out = h_out; t.w_out = w_out; t.H = H; t.W = W;
    t.cap_rows = ytaps ? (yspan < h_in ? yspan : h_in) : RS_TY;
    return 0;
}

bool grid_ok(const RyTables& t) { return (t.W + t.tx - 1) / t.tx <= INT_MAX / 2 && (t.H + RS_TY - 1) / RS_TY <= 65535; }

// depth, subsampling, siting, matrix, range and layout name a kind of frame the YUV entries have: planar, NV12, the P010 family
bool kind_ok(int depth, int subsampling, int siting, int matrix, int range, int layout) {
    if (!enums_ok(depth, subsampling, siting, matrix, range)) return false;
    if (layout == LVAE_YUV_LAYOUT_PLANAR) return true;
    if (layout != LVAE_YUV_LAYOUT_SEMIPLANAR) return false;
    if (depth == 8) return subsampling == LVAE_YUV_SUB_420 && siting == LVAE_YUV_SITING_CENTER && matrix != LVAE_YUV_BT2020;
    return sp_layout_ok(depth, subsampling);
}

// every frame has the call's one size
bool sizes_are(const int* hw, int B, int h, int w) {
    for (int b = 0; hw && b < B; ++b)
        if (hw[2 * b] != h || hw[2 * b + 1] != w) return false;
    return hw != nullptr;
}

}  // namespace

extern "C" int lvae_resample_yuv_to_f32(const void* const* y, const void* const* u, const void* const* v, const long* y_row, const long* u_row,
                                        const long* v_row, const int* hw, int B, int depth, int subsampling, int siting, int matrix, int range,
                                        int chroma, int layout, int h_in, int w_in, int h_out, int w_out, const int* ystart, const float* ywgt,
                                        int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps, int xspan, float* dst,
                                        long dst_img, int H, int W, void* stream) {
    if (!dst || !kind_ok(depth, subsampling, siting, matrix, range, layout) || (chroma != LVAE_YUV_NEAREST && chroma != LVAE_YUV_BILINEAR))
        return -22;
    RyIn a = {};
    RyTables& t = a.t;
    if (tables_setup(t, B, h_in, w_in, h_out, w_out, ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps, H, W)) return -22;
    if ((xtaps && xspan <= 0) || (B > 1 && dst_img < 3L * H * W)) return -22;
    const int sp = layout == LVAE_YUV_LAYOUT_SEMIPLANAR;
    const Planes p = {y, u, v, y_row, u_row, v_row, hw, depth == 8 ? 1 : 2, sp};
    const int sx = subsampling != LVAE_YUV_SUB_444, sy = subsampling == LVAE_YUV_SUB_420;
    if (!sizes_are(hw, B, h_in, w_in) || !frames_ok(p, B, sx, sy, h_in, w_in)) return -22;
    // The tile: the widest TX whose staging buffer and rows fit the budget.  TX consecutive outputs read at most xspan columns (the first
    // RY_XSPAN_OUTPUTS of them) plus the advance of the window's start over the rest, which the window rule bounds by ratio * outputs + 1
    int tx = 32;
    long cols = 0;
    for (; tx >= 8; tx /= 2) {
        cols = xtaps ? xspan + ((long)(tx - RY_XSPAN_OUTPUTS) * w_in + w_out - 1) / w_out + 1 : tx;
        cols = cols < w_in ? cols : w_in;
        if (((long)RY_SR * 3 * cols + (long)t.cap_rows * 3 * tx) * 4 <= RS_LDS_BYTES) break;
    }
    if (tx < 8) return -22;                                  // the tile of this geometry does not fit the LDS budget
    t.tx = tx;
    t.cap_cols = (int)cols;
    if (!grid_ok(t)) return -22;
    a.d_img = dst_img;
    a.k = yuv_params(matrix, range, depth);
    a.bilinear = chroma == LVAE_YUV_BILINEAR;
    const size_t lds = (size_t)((long)RY_SR * 3 * t.cap_cols + (long)t.cap_rows * 3 * tx) * 4;
    auto kernel = YUV_PICK(resample_yuv_in_kernel, depth, subsampling, siting == LVAE_YUV_SITING_LEFT, sp);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        a.fb = plane_batch(p, b0, n);
        a.dst = dst + (long)b0 * dst_img;
        const dim3 grid((unsigned)((W + tx - 1) / tx), (unsigned)((H + RS_TY - 1) / RS_TY), (unsigned)n);
        hipLaunchKernelGGL(kernel, grid, dim3(RS_WG), lds, (hipStream_t)stream, a);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_resample_f32_to_yuv(const float* src, long src_img, long src_plane, long src_row, const int* hw, int B, int depth,
                                        int subsampling, int siting, int matrix, int range, int layout, int h_in, int w_in, int h_out, int w_out,
                                        const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt,
                                        int xtaps, void* const* y, void* const* u, void* const* v, const long* y_row, const long* u_row,
                                        const long* v_row, void* stream) {
    if (!src || !kind_ok(depth, subsampling, siting, matrix, range, layout)) return -22;
    RyOut a = {};
    RyTables& t = a.t;
    if (tables_setup(t, B, h_in, w_in, h_out, w_out, ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps, h_out, w_out)) return -22;
    const long span = (long)(h_in - 1) * src_row + w_in;
    if (src_row < w_in || src_plane < span || (B > 1 && src_img < 2 * src_plane + span)) return -22;
    const int sp = layout == LVAE_YUV_LAYOUT_SEMIPLANAR;
    const Planes p = {(const void* const*)y, (const void* const*)u, (const void* const*)v, y_row, u_row, v_row, hw, depth == 8 ? 1 : 2, sp};
    const int sx = subsampling != LVAE_YUV_SUB_444, sy = subsampling == LVAE_YUV_SUB_420;
    if (!sizes_are(hw, B, h_out, w_out) || !frames_ok(p, B, sx, sy, h_out, w_out)) return -22;
    const int e = sx && siting == LVAE_YUV_SITING_LEFT;
    int tx = 32;
    while (tx >= 8 && (long)t.cap_rows * 3 * (tx + e) * 4 > RS_LDS_BYTES) tx /= 2;
    if (tx < 8) return -22;                                  // the tile of this geometry does not fit the LDS budget
    t.tx = tx;
    if (!grid_ok(t)) return -22;
    a.s_img = src_img; a.s_plane = src_plane; a.s_row = src_row;
    a.k = yuv_params(matrix, range, depth);
    const size_t lds = (size_t)((long)t.cap_rows * 3 * (tx + e)) * 4;
    auto kernel = YUV_PICK(resample_yuv_out_kernel, depth, subsampling, e, sp);
    for (int b0 = 0; b0 < B; b0 += YUV_CHUNK) {
        const int n = B - b0 < YUV_CHUNK ? B - b0 : YUV_CHUNK;
        a.fb = plane_batch(p, b0, n);
        a.src = src + (long)b0 * src_img;
        const dim3 grid((unsigned)((w_out + tx - 1) / tx), (unsigned)((h_out + RS_TY - 1) / RS_TY), (unsigned)n);
        hipLaunchKernelGGL(kernel, grid, dim3(RS_WG), lds, (hipStream_t)stream, a);
    }
    return (int)hipGetLastError();
}
