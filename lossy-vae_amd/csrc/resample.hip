// The separable, antialiased resampler of reduced-resolution coding (lvae/utils/resample.py states the definition; include/lvae_hip.h --
// lvae_resample_u8_to_f32 / lvae_resample_f32_to_u8 / lvae_resample_f32 -- the contract).  All images of a call share one geometry
// (h_in, w_in) -> (h_out, w_out) and one pair of device-resident tap tables (start, weights) per axis; an axis whose size does not change
// has no table and is not filtered.
//
// One launch resamples up to RS_CHUNK images; no intermediate image goes to HBM.  A workgroup owns an RS_TY x TX tile of the
// destination.  Phase 1 filters the input rows its tile needs horizontally, for the tile's TX columns and the 3 channels, into LDS
// (taps ascending, fp32 fmaf); phase 2 filters them vertically out of LDS (taps ascending, fp32 fmaf) and stores.  TX is chosen by the host
// from `yspan` -- the largest number of input rows 16 consecutive output rows read, which the caller derives from its table -- so
// that a workgroup's LDS stays at or below 64 KiB (at least two workgroups per CU).  The kernel clamps every table entry it uses to the source extent
// and every LDS row to the rows it filled: no table, however wrong, makes it read or write outside an extent.
// The three entry points instantiate one body: the 8-bit input is v / 255 by IEEE division (a 256-entry table in LDS, the bits of
// lvae_image_u8_to_f32), the 8-bit output rint(clamp(x, 0, 1) * 255) (the rounding of lvae_image_f32_to_u8), so each equals the fp32
// entry composed with that conversion, bit for bit.  Every access is a byte or an aligned fp32 scalar: any base and any row stride work.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"

namespace {

constexpr int RS_CHUNK = 16;                                 // images per launch
constexpr int RS_WG = 256;
constexpr int RS_TY = 16;                                    // output rows of a tile
constexpr int RS_MAX_TAPS = 64;
constexpr int RS_MAX_RATIO = 8;
constexpr long RS_LDS_BYTES = 64 * 1024;                     // per workgroup: two or more fit a CU's 160 KiB

struct RsU8 { uint8_t* p; long row; };                       // one 8-bit image: base, row stride in bytes
struct RsArgs {
    RsU8 u8[RS_CHUNK];                                       // the 8-bit side (source or destination)
    const float* src; long s_img, s_plane, s_row;            // fp32 source view (elements)
    float* dst; long d_img;                                  // fp32 destination: planes of H * W
    const int* ystart; const float* ywgt; const int* xstart; const float* xwgt;
    int ytaps, xtaps;                                        // 0: the axis is not filtered
    int h_in, w_in, h_out, w_out, H, W;                      // (H, W): the destination's canvas, >= (h_out, w_out)
    int tx, cap_rows, clamp;
};

__device__ __forceinline__ float clamp01(float x) {          // NaN -> 0 (both comparisons are false for a NaN)
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}

template <bool IN_U8, bool OUT_U8>
__global__ __launch_bounds__(RS_WG) void resample_kernel(RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lut = smem;                                       // [256] v / 255 (8-bit input only)
    float* rows = smem + (IN_U8 ? 256 : 0);                  // [nrows][3][TX] horizontally filtered input rows
    const int tid = threadIdx.x, TX = a.tx, b = blockIdx.z;
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * RS_TY;
    const int tw = min(TX, a.W - tx0), th = min(RS_TY, a.H - ty0);
    // the input rows of this tile: those of its first and last source rows of the destination (rows below h_out repeat row h_out - 1)
    const int oy_first = min(ty0, a.h_out - 1), oy_last = min(ty0 + th - 1, a.h_out - 1);
    int row_lo, row_hi;
    if (a.ytaps) {
        row_lo = a.ystart[oy_first];
        row_hi = a.ystart[oy_last] + a.ytaps;
    } else {
        row_lo = oy_first;
        row_hi = oy_last + 1;
    }
    row_lo = max(0, min(row_lo, a.h_in - 1));
    const int nrows = max(1, min(min(row_hi, a.h_in) - row_lo, a.cap_rows));

    if (IN_U8) {
        for (int v = tid; v < 256; v += RS_WG) lut[v] = __fdiv_rn((float)v, 255.0f);
        __syncthreads();
    }
    const uint8_t* __restrict__ s8 = IN_U8 ? a.u8[b].p : nullptr;
    const long s8_row = IN_U8 ? a.u8[b].row : 0;
    const float* __restrict__ sf = IN_U8 ? nullptr : a.src + (long)b * a.s_img;

    // ---- phase 1: horizontal pass of rows row_lo .. row_lo + nrows - 1 at the tile's columns
    for (int idx = tid; idx < nrows * TX; idx += RS_WG) {
        const int r = idx / TX, x = idx - r * TX;
        if (x >= tw) continue;
        const int ox = min(tx0 + x, a.w_out - 1), y = row_lo + r;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        const int taps = a.xtaps ? a.xtaps : 1;
        const int s = a.xtaps ? a.xstart[ox] : ox;
        const float* __restrict__ wr = a.xwgt + (long)ox * a.xtaps;
        for (int j = 0; j < taps; ++j) {
            const int xi = max(0, min(s + j, a.w_in - 1));
            float v[3];
            if (IN_U8) {
                const uint8_t* p = s8 + (long)y * s8_row + 3L * xi;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = lut[p[c]];
            } else {
                const float* p = sf + (long)y * a.s_row + xi;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = p[c * a.s_plane];
            }
            if (a.xtaps) {
                const float w = wr[j];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = fmaf(w, v[c], acc[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = v[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) rows[((long)r * 3 + c) * TX + x] = acc[c];
    }
    __syncthreads();

    // ---- phase 2: vertical pass out of LDS, one destination pixel (3 channels) per step
    for (int idx = tid; idx < th * TX; idx += RS_WG) {
        const int ty = idx / TX, x = idx - ty * TX;
        if (x >= tw) continue;
        const int y = ty0 + ty, oy = min(y, a.h_out - 1);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        if (a.ytaps) {
            const int s = a.ystart[oy];
            const float* __restrict__ wr = a.ywgt + (long)oy * a.ytaps;
            for (int j = 0; j < a.ytaps; ++j) {
                const int r = max(0, min(min(s + j, a.h_in - 1) - row_lo, nrows - 1));
                const float w = wr[j];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = fmaf(w, rows[((long)r * 3 + c) * TX + x], acc[c]);
            }
        } else {
            const int r = max(0, min(oy - row_lo, nrows - 1));
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = rows[((long)r * 3 + c) * TX + x];
        }
        if (OUT_U8) {
            uint8_t* o = a.u8[b].p + (long)y * a.u8[b].row + 3L * (tx0 + x);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(unsigned)(int)rintf(clamp01(acc[c]) * 255.0f);
        } else {
            float* o = a.dst + (long)b * a.d_img + (long)y * a.W + (tx0 + x);
            const long plane = (long)a.H * a.W;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * plane] = a.clamp ? clamp01(acc[c]) : acc[c];
        }
    }
}

// The checks the three entries share; fills the geometry, the tables and the tile of `a`.  -> 0 or -22
int resample_setup(RsArgs& a, bool in_u8, int B, int h_in, int w_in, int h_out, int w_out, const int* ystart, const float* ywgt, int ytaps,
                   int yspan, const int* xstart, const float* xwgt, int xtaps, int H, int W) {
    if (B <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || H < h_out || W < w_out) return -22;
    if (ytaps < 0 || ytaps > RS_MAX_TAPS || xtaps < 0 || xtaps > RS_MAX_TAPS) return -22;
    if (ytaps ? (!ystart || !ywgt || yspan <= 0) : (h_out != h_in || ystart || ywgt)) return -22;
    if (xtaps ? (!xstart || !xwgt) : (w_out != w_in || xstart || xwgt)) return -22;
    if ((long)h_in > (long)RS_MAX_RATIO * h_out || (long)h_out > (long)RS_MAX_RATIO * h_in || (long)w_in > (long)RS_MAX_RATIO * w_out ||
        (long)w_out > (long)RS_MAX_RATIO * w_in)
        return -22;
    const int span = ytaps ? (yspan < h_in ? yspan : h_in) : RS_TY;
    const long fixed = in_u8 ? 256 * 4 : 0;
    int tx = 32;
    while (tx >= 8 && fixed + (long)span * 3 * tx * 4 > RS_LDS_BYTES) tx /= 2;
    if (tx < 8) return -22;                                  // the tile of this geometry does not fit the LDS budget
    if ((W + tx - 1) / tx > INT_MAX / 2 || (H + RS_TY - 1) / RS_TY > 65535) return -22;
    a.ystart = ystart; a.ywgt = ywgt; a.xstart = xstart; a.xwgt = xwgt;
    a.ytaps = ytaps; a.xtaps = xtaps;
    a.h_in = h_in; a.w_in = w_in; a.h_out = h_out; a.w_out = w_out; a.H = H; a.W = W;
    a.tx = tx; a.cap_rows = span; a.clamp = 0;
    return 0;
}

template <bool IN_U8, bool OUT_U8>
void resample_launch(const RsArgs& a, int n, bool in_u8, void* stream) {
    const size_t lds = (size_t)((in_u8 ? 256 : 0) + (long)a.cap_rows * 3 * a.tx) * 4;
    const dim3 grid((unsigned)((a.W + a.tx - 1) / a.tx), (unsigned)((a.H + RS_TY - 1) / RS_TY), (unsigned)n);
    hipLaunchKernelGGL((resample_kernel<IN_U8, OUT_U8>), grid, dim3(RS_WG), lds, (hipStream_t)stream, a);
}

bool f32_view_ok(long img, long plane, long row, int B, int h, int w) {
    const long span = (long)(h - 1) * row + w;
    return row >= w && plane >= span && (B == 1 || img >= 2 * plane + span);
}

}  // namespace

extern "C" int lvae_resample_u8_to_f32(const uint8_t* const* src, const long* src_row, int B, int h_in, int w_in, int h_out, int w_out,
                                       const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt,
                                       int xtaps, float* dst, long dst_img, int H, int W, void* stream) {
    if (!src || !src_row || !dst) return -22;
    RsArgs a = {};
    if (resample_setup(a, true, B, h_in, w_in, h_out, w_out, ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps, H, W)) return -22;
    if (B > 1 && dst_img < 3L * H * W) return -22;
    for (int b = 0; b < B; ++b)
        if (!src[b] || src_row[b] < 3L * w_in) return -22;
    a.clamp = 1;
    a.d_img = dst_img;
    for (int b0 = 0; b0 < B; b0 += RS_CHUNK) {
        const int n = B - b0 < RS_CHUNK ? B - b0 : RS_CHUNK;
        for (int i = 0; i < n; ++i) a.u8[i] = {const_cast<uint8_t*>(src[b0 + i]), src_row[b0 + i]};
        a.dst = dst + (long)b0 * dst_img;
        resample_launch<true, false>(a, n, true, stream);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_resample_f32_to_u8(const float* src, long src_img, long src_plane, long src_row, int B, int h_in, int w_in, int h_out,
                                       int w_out, const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart,
                                       const float* xwgt, int xtaps, uint8_t* const* dst, const long* dst_row, void* stream) {
    if (!src || !dst || !dst_row) return -22;
    RsArgs a = {};
    if (resample_setup(a, false, B, h_in, w_in, h_out, w_out, ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps, h_out, w_out)) return -22;
    if (!f32_view_ok(src_img, src_plane, src_row, B, h_in, w_in)) return -22;
    for (int b = 0; b < B; ++b)
        if (!dst[b] || dst_row[b] < 3L * w_out) return -22;
    a.s_img = src_img; a.s_plane = src_plane; a.s_row = src_row;
    for (int b0 = 0; b0 < B; b0 += RS_CHUNK) {
        const int n = B - b0 < RS_CHUNK ? B - b0 : RS_CHUNK;
        for (int i = 0; i < n; ++i) a.u8[i] = {dst[b0 + i], dst_row[b0 + i]};
        a.src = src + (long)b0 * src_img;
        resample_launch<false, true>(a, n, false, stream);
    }
    return (int)hipGetLastError();
}

extern "C" int lvae_resample_f32(const float* src, long src_img, long src_plane, long src_row, int B, int h_in, int w_in, int h_out, int w_out,
                                 const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps,
                                 int clamp, float* dst, long dst_img, int H, int W, void* stream) {
    if (!src || !dst) return -22;
    RsArgs a = {};
    if (resample_setup(a, false, B, h_in, w_in, h_out, w_out, ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps, H, W)) return -22;
    if (!f32_view_ok(src_img, src_plane, src_row, B, h_in, w_in) || (B > 1 && dst_img < 3L * H * W)) return -22;
    a.clamp = clamp != 0;
    a.s_img = src_img; a.s_plane = src_plane; a.s_row = src_row;
    a.d_img = dst_img;
    for (int b0 = 0; b0 < B; b0 += RS_CHUNK) {
        const int n = B - b0 < RS_CHUNK ? B - b0 : RS_CHUNK;
        a.src = src + (long)b0 * src_img;
        a.dst = dst + (long)b0 * dst_img;
        resample_launch<false, false>(a, n, false, stream);
    }
    return (int)hipGetLastError();
}
