// yuv_fetch.h -- the YUV -> RGB side of the YUV kernels, shared by the kernels that start from YUV planes (yuv_io.hip: into an fp32 canvas;
// resample_yuv.hip: into the resampler's staging rows): the frames of a call as the entries take them and as a launch carries them, the
// rows a pixel's samples lie in, the codes of ONE pixel -- luma, and the chroma filter as exact integers -- and the conversion of those
// codes to clamped fp32 RGB.  One definition, hence one set of bits (lvae/utils/yuv.py::yuv_to_rgb_expr2 states them as torch
// expressions).  yuv_codes_to_rgb switches floating-point contraction off in its own body, so every product and sum is rounded on its own
// whatever the including file compiles under; its divisions are IEEE divisions.  The counterpart of yuv_convert.h, which it builds on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yuv_convert.h"

namespace {

constexpr int YUV_CHUNK = 16;                                // frames (plane pairs) per launch

// one frame: planes, row strides in samples, valid extent
struct PlaneDesc { void *y, *u, *v; long yrow, urow, vrow; int h, w; };
struct PlaneBatch { PlaneDesc d[YUV_CHUNK]; };

// The frames of a call as the entries take them: HOST arrays of plane addresses and row strides in samples, `bytes` per sample.  Planar:
// three planes.  Semi-planar (sp): u is the UV plane, whose rows hold 2 * (w / 2) = w samples; v and v_row are not read.
struct Planes { const void *const *y, *const *u, *const *v; const long *y_row, *u_row, *v_row; const int* hw; int bytes, sp; };

// The frames' descriptors are valid: planes non-null, extents positive, even where subsampled and inside (H, W), rows that hold their plane's width
inline bool frames_ok(const Planes& p, int B, int sx, int sy, int H, int W) {
    if (!p.y || !p.u || !p.y_row || !p.u_row || !p.hw || (!p.sp && (!p.v || !p.v_row))) return false;
    for (int b = 0; b < B; ++b) {
        const int h = p.hw[2 * b], w = p.hw[2 * b + 1];
        if (h <= 0 || w <= 0 || (h & sy) || (w & sx) || h > H || w > W) return false;
        if (!p.y[b] || !p.u[b] || p.y_row[b] < w || p.u_row[b] < (p.sp ? w : w >> sx)) return false;
        if (!p.sp && (!p.v[b] || p.v_row[b] < (w >> sx))) return false;
    }
    return true;
}

// frames b0 .. b0 + n for one launch.  Semi-planar: v = the UV plane one sample on, with the UV row stride: what the SP variants index with column * 2
inline PlaneBatch plane_batch(const Planes& p, int b0, int n) {
    PlaneBatch fb = {};
    for (int i = 0; i < n; ++i) {
        const int b = b0 + i;
        void* u = const_cast<void*>(p.u[b]);
        fb.d[i] = {const_cast<void*>(p.y[b]), u, p.sp ? (char*)u + p.bytes : const_cast<void*>(p.v[b]), p.y_row[b], p.u_row[b],
                   p.sp ? p.u_row[b] : p.v_row[b], p.hw[2 * b], p.hw[2 * b + 1]};
    }
    return fb;
}

// the code of a sample: the low `depth` bits of its word, or -- semi-planar -- the high ones
template <int SP>
__device__ __forceinline__ unsigned yuv_code(unsigned word, const YuvParams& k) {
    return (SP ? word >> k.shift : word) & k.mask;
}

// The rows the samples of luma row ys (inside the extent) lie in: the luma row, the chroma row cy = ys >> SY and the second chroma row of
// the vertical filter -- the neighbour on the pixel's side, clamped (nearest, or no vertical subsampling: cy itself) -- and the chroma width
template <typename T> struct YuvRows { const T *yr, *ua, *ub, *va, *vb; int cw; };

template <typename T, int SX, int SY>
__device__ __forceinline__ YuvRows<T> yuv_rows(const PlaneDesc& im, int ys, int bilinear) {
    const int ch = im.h >> SY;
    const int cy = ys >> SY;
    const int cyb = (SY && bilinear) ? min(max(cy + ((ys & 1) ? 1 : -1), 0), ch - 1) : cy;
    return {(const T*)im.y + (long)ys * im.yrow, (const T*)im.u + (long)cy * im.urow, (const T*)im.u + (long)cyb * im.urow,
            (const T*)im.v + (long)cy * im.vrow, (const T*)im.v + (long)cyb * im.vrow, im.w >> SX};
}

// The codes of the pixel at column xs (inside the extent) of those rows: Y, and CU, CV = (SX ? 4 : 1) * (SY ? 4 : 1) times the upsampled
// chroma -- per subsampled axis the weights are quarters, so the products are integers of at most 16 * 4095, exact in any order.
// SX, SY: the chroma planes are (h >> SY, w >> SX); LEFT: the chroma sample lies on the even luma column (SX only; vertically it is
// centred); SP: semi-planar words -- a chroma pixel is two neighbouring samples, U then V, and va / vb point one sample behind ua / ub
template <typename T, int SX, int SY, int LEFT, int SP>
__device__ __forceinline__ void yuv_pixel_codes(const YuvRows<T>& r, int xs, int bilinear, const YuvParams& k, unsigned& Y, unsigned& CU,
                                                unsigned& CV) {
    static_assert(SX || !SY, "4:4:0 is not a layout of this file");
    static_assert(!SP || SX, "semi-planar frames are 4:2:0 / 4:2:2");
    constexpr int CS = SP ? 2 : 1;                           // samples from one chroma column to the next
    Y = yuv_code<SP>(r.yr[xs], k);
    if constexpr (!SX) {
        CU = yuv_code<SP>(r.ua[xs], k);
        CV = yuv_code<SP>(r.va[xs], k);
    } else {
        const int cx = (xs >> 1) * CS;                       // in samples, as cxb
        int cxb = cx;                                        // the second tap and the weight of the first, in quarters
        unsigned wa = 4u;
        if (bilinear) {
            if (LEFT) {
                if (xs & 1) { cxb = min((xs >> 1) + 1, r.cw - 1) * CS; wa = 2u; }
            } else {
                cxb = min(max((xs >> 1) + ((xs & 1) ? 1 : -1), 0), r.cw - 1) * CS;
                wa = 3u;
            }
        }
        const unsigned wb = 4u - wa;
        const unsigned pa = yuv_code<SP>(r.ua[cx], k), pb = yuv_code<SP>(r.ua[cxb], k), qa = yuv_code<SP>(r.va[cx], k),
                       qb = yuv_code<SP>(r.va[cxb], k);
        if (SY) {
            CU = wa * (3u * pa + yuv_code<SP>(r.ub[cx], k)) + wb * (3u * pb + yuv_code<SP>(r.ub[cxb], k));
            CV = wa * (3u * qa + yuv_code<SP>(r.vb[cx], k)) + wb * (3u * qb + yuv_code<SP>(r.vb[cxb], k));
        } else {
            CU = wa * pa + wb * pb;
            CV = wa * qa + wb * qb;
        }
    }
}

// Codes as yuv_pixel_codes gives them -> R, G, B in [0, 1]: y' = (Y - yoff) / yscale, c = (C - 128 s) / cscale, the inverse matrix, the
// clamp (NaN -> 0); C / 16 (/ 4) is exact
template <int SX, int SY>
__device__ __forceinline__ void yuv_codes_to_rgb(unsigned Y, unsigned CU, unsigned CV, const YuvParams& k, float& r, float& g, float& b) {
#pragma clang fp contract(off)
    constexpr float inv = 1.0f / (float)((SX ? 4 : 1) * (SY ? 4 : 1));
    const float yn = __fdiv_rn((float)Y - k.yo, k.ys);
    const float cb = __fdiv_rn((float)CU * inv - k.co, k.cs);
    const float cr = __fdiv_rn((float)CV * inv - k.co, k.cs);
    r = clamp01(yn + k.a * cr);
    b = clamp01(yn + k.b * cb);
    g = clamp01((yn - k.d * cb) - k.e * cr);
}

}  // namespace
