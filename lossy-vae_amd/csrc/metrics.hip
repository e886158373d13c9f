// Image-quality metrics on the device: MS-SSIM (Wang, Simoncelli, Bovik 2003) in the form learned-compression evaluations use -- data
// range 1, K1 = 0.01, K2 = 0.03, 11-tap Gaussian window (sigma 1.5) as a valid correlation, 5 scales, 2x2 mean pool with zero padding of
// size % 2 between them.  include/lvae_hip.h (lvae_msssim_f32) states the contract; DESIGN.md the tiling.
//
// One call = 5 launches of msssim_scale_kernel (scale s reads the planes of scale s, writes the planes of scale s + 1 and one fp64
// (ssim, cs) partial per workgroup) + 1 launch of msssim_finish_kernel, whatever B is.  Inputs are fp32 and exact; the pooled planes are
// stored as fp32; the windowed moments, the maps and every sum are fp64, so E[x^2] - E[x]^2 on a flat region (black against white) does
// not lose the 9e-4 of C2 to fp32 rounding.  No atomics: every partial has a slot of its own and is added in a fixed order.
//
// The scale kernel is a template over the SAMPLE LOADER of its tile load: fp32 planes addressed by strides (lvae_msssim_f32, and the pooled
// planes of scales >= 1 of every call), and the planes of lvae_msssim_planes -- one image of one channel per pair, each with its own
// address, row stride and pixel stride -- as fp32, bytes, or 16-bit words with the code in the low or in the high bits.  Integer samples
// enter the LDS tile as their code (<= 4095: exact as a float) and the arithmetic stays in code units: C1 = (0.01 L)^2 and C2 = (0.03 L)^2
// are arguments, nothing is divided by L.  With scales = 1 the first scale is the last: its ssim-map mean is the single-scale SSIM.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/lvae_hip.h"

namespace {

constexpr int MS_SCALES = 5;
constexpr int MS_TAPS = 11;
constexpr int MS_HALO = MS_TAPS - 1;
constexpr int MS_TH = 28, MS_TW = 32;                       // output tile (both even: the pool's ownership rule below needs it)
constexpr int MS_IH = MS_TH + MS_HALO, MS_IW = MS_TW + MS_HALO;
constexpr int MS_IWP = MS_IW + 1;                           // LDS row pitch of the input tiles
constexpr int MS_WG = 256;
constexpr int MS_MIN_SIDE = 161;                            // smallest legal side: 161 -> 81 -> 41 -> 21 -> 11 keeps one valid pixel
constexpr int MS_MIN_SIDE1 = MS_TAPS;                       // ... of a single scale: one valid pixel
constexpr size_t MS_ALIGN = 256;

struct MsWeights { double g[MS_TAPS]; };

struct MsPair {                                             // one plane pair of lvae_msssim_planes, as the kernel reads it from the workspace
    const void* x; const void* y;
    long x_row, y_row;                                      // in samples
    int pix, pad;                                           // samples from one pixel to the next
};

struct MsLayout {                                           // the workspace of one (B, C, Hmax, Wmax, scales): byte offsets
    int H[MS_SCALES], W[MS_SCALES];                         // plane size of each scale (of the largest image)
    int ntx[MS_SCALES], tiles[MS_SCALES];                   // tile columns / tiles per plane of each scale
    size_t off_hw, off_pairs, off_part[MS_SCALES], off_x[MS_SCALES], off_y[MS_SCALES], total;
};

inline size_t ms_up(size_t v) { return (v + MS_ALIGN - 1) / MS_ALIGN * MS_ALIGN; }

__host__ __device__ inline int ms_tiles_1d(int n, int t) { return (n - MS_HALO + t - 1) / t; }

// S scales (5, or 1: SSIM); pairs: the MsPair table of lvae_msssim_planes follows hw (lvae_msssim_f32 has none: its layout is unchanged)
bool ms_layout(int B, int C, int Hmax, int Wmax, MsLayout* L, int S = MS_SCALES, bool pairs = false) {
    const int side = S == 1 ? MS_MIN_SIDE1 : MS_MIN_SIDE;
    if ((S != 1 && S != MS_SCALES) || B <= 0 || C <= 0 || B > 65535 || C > 65535 || Hmax < side || Wmax < side || Hmax > (1 << 20) || Wmax > (1 << 20)) return false;
    const size_t planes = (size_t)B * (size_t)C;
    size_t off = 0;
    L->off_hw = off;
    off += ms_up((size_t)B * 2 * sizeof(int));
    L->off_pairs = off;
    if (pairs) off += ms_up((size_t)B * sizeof(MsPair));
    int h = Hmax, w = Wmax;
    for (int s = 0; s < S; ++s) {
        L->H[s] = h; L->W[s] = w;
        L->ntx[s] = ms_tiles_1d(w, MS_TW);
        const long tiles = (long)L->ntx[s] * ms_tiles_1d(h, MS_TH);
        if (tiles > 0x7fffffffL) return false;
        L->tiles[s] = (int)tiles;
        L->off_part[s] = off;
        off += ms_up(planes * (size_t)tiles * 2 * sizeof(double));
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    L->off_x[0] = L->off_y[0] = 0;
    for (int s = 1; s < S; ++s) {
        const size_t bytes = ms_up(planes * (size_t)L->H[s] * (size_t)L->W[s] * sizeof(float));
        L->off_x[s] = off; off += bytes;
        L->off_y[s] = off; off += bytes;
    }
    L->total = off;
    return true;
}

__device__ __forceinline__ void ms_extent(const int* __restrict__ hw, int b, int s, int& h, int& w) {
    h = hw[2 * b]; w = hw[2 * b + 1];
    for (int i = 0; i < s; ++i) { h = (h + 1) >> 1; w = (w + 1) >> 1; }
}

// Sample loaders: view(b, c) gives the two planes of image b, channel c; its x(r, q) / y(r, q) the sample at row r, pixel q as a float.
struct MsLdStrided {                                        // fp32 NCHW planes by strides: element (b, c, r, q) at b*img + c*plane + r*row + q
    const float* xp; long x_img, x_plane, x_row;
    const float* yp; long y_img, y_plane, y_row;
    struct View {
        const float* xp; const float* yp; long x_row, y_row;
        __device__ __forceinline__ float x(int r, int q) const { return xp[(long)r * x_row + q]; }
        __device__ __forceinline__ float y(int r, int q) const { return yp[(long)r * y_row + q]; }
    };
    __device__ __forceinline__ View view(int b, int c) const {
        return {xp + (long)b * x_img + (long)c * x_plane, yp + (long)b * y_img + (long)c * y_plane, x_row, y_row};
    }
};

struct MsCodeF32 { using T = float; static __device__ __forceinline__ float code(float v, int) { return v; } };
struct MsCodeU8 { using T = uint8_t; static __device__ __forceinline__ float code(uint8_t v, int) { return (float)v; } };
struct MsCodeLow { using T = uint16_t; static __device__ __forceinline__ float code(uint16_t v, int mask) { return (float)(v & mask); } };
struct MsCodeHigh { using T = uint16_t; static __device__ __forceinline__ float code(uint16_t v, int shift) { return (float)(v >> shift); } };

template <class Code>
struct MsLdPairs {                                          // the table of lvae_msssim_planes: image b is pair b, one channel
    const MsPair* pairs; int arg;                           // arg: the mask (low-bit words) or the shift (high-bit words) of Code
    struct View {
        const typename Code::T* xp; const typename Code::T* yp; long x_row, y_row; int pix, arg;
        __device__ __forceinline__ float x(int r, int q) const { return Code::code(xp[(long)r * x_row + (long)q * pix], arg); }
        __device__ __forceinline__ float y(int r, int q) const { return Code::code(yp[(long)r * y_row + (long)q * pix], arg); }
    };
    __device__ __forceinline__ View view(int b, int) const {
        const MsPair p = pairs[b];
        return {(const typename Code::T*)p.x, (const typename Code::T*)p.y, p.x_row, p.y_row, p.pix, arg};
    }
};

// The two maps at one pixel from its five windowed moments -> the ssim value; cv: the contrast-structure value.
// lvae_msssim_f32's form: the expressions as that entry has always had them (the compiler contracts products into the sums).
__device__ __forceinline__ double ms_pixel(double mx, double my, double mxx, double myy, double mxy, double C1, double C2, double& cv) {
    const double sxx = mxx - mx * mx, syy = myy - my * my, sxy = mxy - mx * my;
    cv = (2.0 * sxy + C2) / (sxx + syy + C2);
    return ((2.0 * mx * my + C1) / (mx * mx + my * my + C1)) * cv;
}

// lvae_msssim_planes' form: every product and sum rounded on its own, so that for x == y numerator and denominator of both ratios are
// the same number -- (t + t) + C and (t + t) + C -- and identical planes give exactly 1 (a contracted 2 mx my + C1 is rounded once,
// mx mx + my my + C1 twice: an ulp apart now and then).
__device__ __forceinline__ double ms_pixel_sym(double mx, double my, double mxx, double myy, double mxy, double C1, double C2, double& cv) {
#pragma clang fp contract(off)
    const double pxx = mx * mx, pyy = my * my, pxy = mx * my;
    const double sxx = mxx - pxx, syy = myy - pyy, sxy = mxy - pxy;
    cv = ((sxy + sxy) + C2) / ((sxx + syy) + C2);
    return (((pxy + pxy) + C1) / ((pxx + pyy) + C1)) * cv;
}

// Scale s of every image and channel.  grid (tiles of the largest plane, C, B); a workgroup whose tile lies outside its image's extent exits.
// ld: the planes of this scale behind a sample loader (above); only [0, h) x [0, w) of an image is read.  C1, C2: the constants of the
// maps, in the units of the samples.
// nx / ny (null at the last scale): planes of the next scale, [B*C][nH][nW] dense.  The tile owns the pooled pixels whose window STARTS
// in its MS_TH x MS_TW output rectangle (the last tile of an axis: to the end; the first: the window that starts at -1 as well); a window
// ends at most one pixel further, inside the halo the workgroup holds anyway.
// part: double[B*C][tiles_max][2]; tile (ty, tx) of an image writes slot ty*ntx(image) + tx, so an image's slots and their order depend
// on its own extent alone.  SYM: the maps by ms_pixel_sym.
template <class Ld, bool SYM>
__global__ __launch_bounds__(MS_WG) void msssim_scale_kernel(Ld ld, const int* __restrict__ hw, int s, int ntx_max, int tiles_max,
                                                              float* __restrict__ nx, float* __restrict__ ny, int nH, int nW,
                                                              double* __restrict__ part, MsWeights wt, double C1, double C2) {
    __shared__ float tx_[MS_IH][MS_IWP];
    __shared__ float ty_[MS_IH][MS_IWP];
    __shared__ double hm[5][MS_IH][MS_TW];                  // row-filtered x, y, x^2, y^2, xy
    __shared__ double red[MS_WG / 64][2];
    const int tid = threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z, C = gridDim.y;
    int h, w;
    ms_extent(hw, b, s, h, w);
    const int vh = h - MS_HALO, vw = w - MS_HALO;           // valid outputs
    const int ntx = ms_tiles_1d(w, MS_TW), nty = ms_tiles_1d(h, MS_TH);
    const int tyi = blockIdx.x / ntx_max, txi = blockIdx.x - tyi * ntx_max;
    if (txi >= ntx || tyi >= nty) return;
    const int r0 = tyi * MS_TH, c0 = txi * MS_TW;
    const auto src = ld.view(b, c);

    for (int i = tid; i < MS_IH * MS_IW; i += MS_WG) {
        const int r = i / MS_IW, q = i - r * MS_IW;
        const int gr = r0 + r, gq = c0 + q;
        const bool in = gr < h && gq < w;
        tx_[r][q] = in ? src.x(gr, gq) : 0.f;
        ty_[r][q] = in ? src.y(gr, gq) : 0.f;
    }
    __syncthreads();

    if (nx) {                                               // 2x2 mean pool, zero padding of size % 2 in front, zeros counted
        int oh = (h + 1) >> 1, ow = (w + 1) >> 1;
        const int ph = h & 1, pw = w & 1;
        const int i_lo = r0 == 0 ? 0 : r0 / 2 + ph, i_hi = tyi == nty - 1 ? oh : (r0 + MS_TH) / 2 + ph;
        const int j_lo = c0 == 0 ? 0 : c0 / 2 + pw, j_hi = txi == ntx - 1 ? ow : (c0 + MS_TW) / 2 + pw;
        const int nj = j_hi - j_lo, n = (i_hi - i_lo) * nj;
        float* ox = nx + ((long)b * C + c) * nH * nW;
        float* oy = ny + ((long)b * C + c) * nH * nW;
        for (int k = tid; k < n; k += MS_WG) {
            const int i = i_lo + k / nj, j = j_lo + k % nj;
            const int lr = 2 * i - ph - r0, lq = 2 * j - pw - c0;      // -1 only for the padded first row / column
            float sx = 0.f, sy = 0.f;
#pragma unroll
            for (int dr = 0; dr < 2; ++dr)
#pragma unroll
                for (int dq = 0; dq < 2; ++dq) {
                    const int rr = lr + dr, qq = lq + dq;
                    if (rr >= 0 && qq >= 0 && rr < MS_IH && qq < MS_IW) { sx += tx_[rr][qq]; sy += ty_[rr][qq]; }
                }
            ox[(long)i * nW + j] = sx * 0.25f;
            oy[(long)i * nW + j] = sy * 0.25f;
        }
    }

    // rows: thread = (tile row, pair of output columns)
    for (int it = tid; it < MS_IH * (MS_TW / 2); it += MS_WG) {
        const int r = it / (MS_TW / 2), q = (it - r * (MS_TW / 2)) * 2;
        double a[5][2] = {};
#pragma unroll
        for (int k = 0; k < MS_TAPS + 1; ++k) {
            const double xv = (double)tx_[r][q + k], yv = (double)ty_[r][q + k];
            const double v[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                if (k < MS_TAPS) a[m][0] = fma(wt.g[k], v[m], a[m][0]);
                if (k > 0) a[m][1] = fma(wt.g[k - 1], v[m], a[m][1]);
            }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) { hm[m][r][q] = a[m][0]; hm[m][r][q + 1] = a[m][1]; }
    }
    __syncthreads();

    // columns: thread = (output column, group of 4 output rows); then the maps on the valid pixels
    double ss = 0.0, cs = 0.0;
    if (tid < MS_TW * (MS_TH / 4)) {
        const int q = tid % MS_TW, rg = (tid / MS_TW) * 4;
        double mo[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double col[MS_TAPS + 3];
#pragma unroll
            for (int k = 0; k < MS_TAPS + 3; ++k) col[k] = hm[m][rg + k][q];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < MS_TAPS; ++k) acc = fma(wt.g[k], col[o + k], acc);
                mo[m][o] = acc;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (r0 + rg + o < vh && c0 + q < vw) {
                double cv;
                const double sv = SYM ? ms_pixel_sym(mo[0][o], mo[1][o], mo[2][o], mo[3][o], mo[4][o], C1, C2, cv)
                                      : ms_pixel(mo[0][o], mo[1][o], mo[2][o], mo[3][o], mo[4][o], C1, C2, cv);
                cs += cv;
                ss += sv;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ss += __shfl_xor(ss, o, 64); cs += __shfl_xor(cs, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = ss; red[tid >> 6][1] = cs; }
    __syncthreads();
    if (tid == 0) {
        double* p = part + (((long)b * C + c) * tiles_max + ((long)tyi * ntx + txi)) * 2;
        p[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        p[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

struct MsFinishArgs {
    const double* part[MS_SCALES];
    int tiles_max[MS_SCALES];
    double weight[MS_SCALES];
};

// One workgroup per image: wave k adds the partials of (scale, channel) pairs k, k + 4, ... -- lane j the tiles j, j + 64, ... in tile
// order, then the fixed xor tree -- and divides by the number of valid pixels; thread 0 forms prod_s relu(mean)^w_s per channel and the
// channel mean.  means[b][s][c]: the cs mean of scales 0..S-2 and the ssim mean of scale S-1, before the relu.  S = 1: the value is the
// channel mean of the ssim means themselves (the mean SSIM map; no relu, no power).
__global__ __launch_bounds__(MS_WG) void msssim_finish_kernel(MsFinishArgs fa, const int* __restrict__ hw, int C, int S, double* __restrict__ out,
                                                               double* __restrict__ means) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* mb = means + (long)b * S * C;
    for (int sc = wave; sc < S * C; sc += MS_WG / 64) {
        const int s = sc / C, c = sc - s * C;
        int h, w;
        ms_extent(hw, b, s, h, w);
        const int n = ms_tiles_1d(w, MS_TW) * ms_tiles_1d(h, MS_TH);
        const double* p = fa.part[s] + ((long)b * C + c) * fa.tiles_max[s] * 2 + (s == S - 1 ? 0 : 1);
        double acc = 0.0;
        for (int k = lane; k < n; k += 64) acc += p[2 * (long)k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) mb[sc] = acc / ((double)(h - MS_HALO) * (double)(w - MS_HALO));
    }
    __syncthreads();                                        // the workgroup's own global writes are visible to it after the barrier
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int c = 0; c < C; ++c) {
            double pr = 1.0;
            if (S == 1) pr = mb[c];
            else
                for (int s = 0; s < S; ++s) {
                    const double v = mb[s * C + c];
                    pr *= pow(v > 0.0 ? v : 0.0, fa.weight[s]);
                }
            tot += pr;
        }
        out[b] = tot / (double)C;
    }
}

template <bool SYM, class Ld>
void ms_launch_scale(const Ld& ld, const MsLayout& L, char* base, int s, int S, int B, int C, MsWeights wt, double C1, double C2, hipStream_t st) {
    const bool last = s == S - 1;
    hipLaunchKernelGGL((msssim_scale_kernel<Ld, SYM>), dim3((unsigned)L.tiles[s], (unsigned)C, (unsigned)B), dim3(MS_WG), 0, st,
                       ld, (const int*)(base + L.off_hw), s, L.ntx[s], L.tiles[s],
                       last ? (float*)nullptr : (float*)(base + L.off_x[s + 1]), last ? (float*)nullptr : (float*)(base + L.off_y[s + 1]),
                       last ? 0 : L.H[s + 1], last ? 0 : L.W[s + 1], (double*)(base + L.off_part[s]), wt, C1, C2);
}

// The launch sequence of both entries, after hw (and the pair table) reached the workspace: scale 0 through `first`, the pooled fp32 planes
// of scales 1 .. S-1 through the strided loader, then the finish kernel.
template <bool SYM, class Ld>
int ms_run(const Ld& first, const MsLayout& L, char* base, int S, int B, int C, double C1, double C2, double* out, double* scale_means,
           hipStream_t st) {
    MsWeights wt;
    double sum = 0.0;
    for (int k = 0; k < MS_TAPS; ++k) {
        const double d = (double)(k - MS_TAPS / 2);
        wt.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += wt.g[k];
    }
    for (int k = 0; k < MS_TAPS; ++k) wt.g[k] /= sum;

    MsFinishArgs fa = {};
    const double w5[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int s = 0; s < S; ++s) {
        fa.part[s] = (const double*)(base + L.off_part[s]); fa.tiles_max[s] = L.tiles[s]; fa.weight[s] = w5[s];
        if (s == 0) {
            ms_launch_scale<SYM>(first, L, base, s, S, B, C, wt, C1, C2, st);
        } else {
            const long pl = (long)L.H[s] * L.W[s];
            const MsLdStrided ld = {(const float*)(base + L.off_x[s]), pl * C, pl, (long)L.W[s], (const float*)(base + L.off_y[s]), pl * C, pl, (long)L.W[s]};
            ms_launch_scale<SYM>(ld, L, base, s, S, B, C, wt, C1, C2, st);
        }
    }
    hipLaunchKernelGGL(msssim_finish_kernel, dim3((unsigned)B), dim3(MS_WG), 0, st, fa, (const int*)(base + L.off_hw), C, S, out, scale_means);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t lvae_msssim_workspace_bytes(int B, int C, int Hmax, int Wmax) {
    MsLayout L;
    return ms_layout(B, C, Hmax, Wmax, &L) ? L.total : 0;
}

extern "C" int lvae_msssim_f32(const float* x, long x_img, long x_plane, long x_row, const float* y, long y_img, long y_plane, long y_row,
                               const int* hw, int B, int C, int Hmax, int Wmax, double* out, double* scale_means, void* ws, size_t ws_bytes,
                               void* stream) {
    if (!x || !y || !hw || !out || !scale_means || !ws) return -22;
    MsLayout L;
    if (!ms_layout(B, C, Hmax, Wmax, &L) || ws_bytes < L.total || ((uintptr_t)ws & 7)) return -22;
    const long strides[2][3] = {{x_img, x_plane, x_row}, {y_img, y_plane, y_row}};
    for (int b = 0; b < B; ++b) {
        const int h = hw[2 * b], w = hw[2 * b + 1];
        if (h < MS_MIN_SIDE || w < MS_MIN_SIDE || h > Hmax || w > Wmax) return -22;
        for (const long* st : strides) {                    // the extent has to fit the strides: rows in a plane, planes in an image
            if (w > st[2] || (long)(h - 1) * st[2] + w > st[1]) return -22;
            if (B > 1 && (long)(C - 1) * st[1] + (long)(h - 1) * st[2] + w > st[0]) return -22;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    hipError_t e = hipMemcpyAsync(base + L.off_hw, hw, (size_t)B * 2 * sizeof(int), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    const MsLdStrided ld = {x, x_img, x_plane, x_row, y, y_img, y_plane, y_row};
    return ms_run<false>(ld, L, base, MS_SCALES, B, C, 1e-4, 9e-4, out, scale_means, st);
}

namespace {

// The checks of lvae_msssim_planes that need no layout; fills (Hmax, Wmax).
bool ms_planes_args(const void* const* x, const long* x_row, const void* const* y, const long* y_row, const int* hw, const int* pix, int n,
                    int kind, int depth, double data_range, int scales, int* Hmax, int* Wmax) {
    if (!x || !x_row || !y || !y_row || !hw || !pix || n <= 0 || n > 65535) return false;
    if (scales != 1 && scales != MS_SCALES) return false;
    if (!(data_range > 0.0) || !(data_range <= 65535.0)) return false;
    if (kind < LVAE_SAMPLE_F32 || kind > LVAE_SAMPLE_U16_HIGH) return false;
    if (kind == LVAE_SAMPLE_U8 ? depth != 8 : kind != LVAE_SAMPLE_F32 && depth != 8 && depth != 10 && depth != 12) return false;
    const int side = scales == 1 ? MS_MIN_SIDE1 : MS_MIN_SIDE;
    int H = 0, W = 0;
    for (int k = 0; k < n; ++k) {
        const int h = hw[2 * k], w = hw[2 * k + 1];
        if (!x[k] || !y[k] || h < side || w < side || h > (1 << 20) || w > (1 << 20)) return false;
        if ((pix[k] != 1 && pix[k] != 2) || (long)w * pix[k] > x_row[k] || (long)w * pix[k] > y_row[k]) return false;
        H = h > H ? h : H; W = w > W ? w : W;
    }
    *Hmax = H; *Wmax = W;
    return true;
}

}  // namespace

extern "C" size_t lvae_msssim_planes_workspace_bytes(int n, int Hmax, int Wmax, int scales) {
    MsLayout L;
    return ms_layout(n, 1, Hmax, Wmax, &L, scales, true) ? L.total : 0;
}

extern "C" int lvae_msssim_planes(const void* const* x, const long* x_row, const void* const* y, const long* y_row, const int* hw,
                                  const int* pixstride, int n, int kind, int depth, double data_range, int scales, double* out,
                                  double* scale_means, void* ws, size_t ws_bytes, void* stream) {
    int Hmax = 0, Wmax = 0;
    if (!out || !scale_means || !ws || !ms_planes_args(x, x_row, y, y_row, hw, pixstride, n, kind, depth, data_range, scales, &Hmax, &Wmax)) return -22;
    MsLayout L;
    if (!ms_layout(n, 1, Hmax, Wmax, &L, scales, true) || ws_bytes < L.total || ((uintptr_t)ws & 7)) return -22;
    // hw and the pair table travel to the workspace in ONE copy, laid out as the workspace holds them
    const size_t head = L.off_pairs + (size_t)n * sizeof(MsPair);
    std::vector<char> host(head, 0);
    memcpy(host.data() + L.off_hw, hw, (size_t)n * 2 * sizeof(int));
    MsPair* tab = (MsPair*)(host.data() + L.off_pairs);
    for (int k = 0; k < n; ++k) tab[k] = {x[k], y[k], x_row[k], y_row[k], pixstride[k], 0};
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    hipError_t e = hipMemcpyAsync(base, host.data(), head, hipMemcpyHostToDevice, st);       // pageable source: staged before the call returns
    if (e != hipSuccess) return (int)e;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const MsPair* pairs = (const MsPair*)(base + L.off_pairs);
    switch (kind) {
        case LVAE_SAMPLE_F32: return ms_run<true>(MsLdPairs<MsCodeF32>{pairs, 0}, L, base, scales, n, 1, c1, c2, out, scale_means, st);
        case LVAE_SAMPLE_U8: return ms_run<true>(MsLdPairs<MsCodeU8>{pairs, 0}, L, base, scales, n, 1, c1, c2, out, scale_means, st);
        case LVAE_SAMPLE_U16_LOW: return ms_run<true>(MsLdPairs<MsCodeLow>{pairs, (1 << depth) - 1}, L, base, scales, n, 1, c1, c2, out, scale_means, st);
        default: return ms_run<true>(MsLdPairs<MsCodeHigh>{pairs, 16 - depth}, L, base, scales, n, 1, c1, c2, out, scale_means, st);
    }
}
