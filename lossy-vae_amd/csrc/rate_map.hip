// rate_map.hip -- where an image's bits go: the rate terms of the eval-mode statistics kept by POSITION instead of summed per image, and
// their composition to one map at image resolution.  include/lvae_hip.h (lvae_gaussian_nll_pos_f32 / lvae_pixel_nll_pos_f32 /
// lvae_rate_map_f32) states the contract.  The terms are those of pointwise.hip (rate_terms.h: one definition); every sum here has a
// fixed order and no atomics, in fp64 with explicitly rounded operations, so a torch fp64 expression of the definition gives the bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lvae_hip.h"
#include "rate_terms.h"

namespace {

// Correctly rounded fp64 add / multiply that stay two operations.  (The toolchain's __dadd_rn / __dmul_rn are a plain + and * compiled
// under the default contraction mode: inlined next to each other they may come out as one fused multiply-add, which a torch expression
// of the definition does not compute.)
__device__ __forceinline__ double dadd_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double dmul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

// Position-wise latent rate.  One lane owns one position m = b*HW + p of the batch and adds its z terms in ascending channel order.
// The NCHW symbols are read along positions (coalesced).  The NHWC log-scale parameters -- row m holds 2z floats, the log-scales in
// its second half -- go through LDS: a workgroup stages the [RP_NT rows][RP_CH channels] panel with lanes running along the channels
// of a row (a 32-channel run is one 128-byte line: two lines per wave load) and each lane then walks its own row.  Chosen on
// reasoning, not on a measurement of the two forms: the direct read (lane m at row m, channel c) would touch 64 lines per wave load and
// come back to each line 16 times, with a working set per wave (64 rows x 4z bytes, up to 24 KB) that a 32 KB L1 is not expected to
// hold once several waves share a CU.  Row pitch RP_CH + 1 floats: the row walk (lane t at word t*33 + c) hits 32 distinct banks per
// half wave.
constexpr int RP_NT = 64, RP_CH = 32, RP_LD = RP_CH + 1;

__global__ __launch_bounds__(RP_NT) void gaussian_nll_pos_kernel(const float* __restrict__ prm, const int32_t* __restrict__ sym,
                                                                 double* __restrict__ out, float bound, long M, int HW, int z,
                                                                 int cdf_form) {
    __shared__ float tile[RP_NT * RP_LD];
    const long m0 = (long)blockIdx.x * RP_NT;
    const int rows = (M - m0) < RP_NT ? (int)(M - m0) : RP_NT;
    const bool live = (int)threadIdx.x < rows;
    const long m = live ? m0 + threadIdx.x : m0;                   // (idle lanes of the last workgroup address a valid row and store nothing)
    const long b = m / HW;
    const int p = (int)(m - b * HW);
    const int32_t* sp = sym + b * z * HW + p;
    double acc = 0.0;
    for (int c0 = 0; c0 < z; c0 += RP_CH) {
        const int nc = (z - c0) < RP_CH ? (z - c0) : RP_CH;
        __syncthreads();                                           // the previous panel has been read
        for (int j = threadIdx.x; j < rows * nc; j += RP_NT) {
            const int r = j / nc, cc = j - r * nc;
            tile[r * RP_LD + cc] = prm[(m0 + r) * 2 * z + z + c0 + cc];
        }
        __syncthreads();
        if (live)
            for (int cc = 0; cc < nc; ++cc) {
                const float t = -gaussian_logp(tile[threadIdx.x * RP_LD + cc], sp[(long)(c0 + cc) * HW], bound, cdf_form);
                acc = dadd_rn(acc, (double)t);
            }
    }
    if (live) out[m] = acc;
}

// The same for the lossless model's pixel stage: one lane per pixel of the batch, its three channels in ascending order.
__global__ __launch_bounds__(256) void pixel_nll_pos_kernel(const float* __restrict__ raw, const float* __restrict__ im,
                                                            double* __restrict__ out, long total, int HW, int* __restrict__ status) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long b = e / HW;
    const int p = (int)(e - b * HW);
    const float* r6 = raw + e * 6;
    const float* xi = im + b * 3 * HW + p;
    double acc = 0.0;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = r6[c];
        const float lp = pixel_logp(m, r6[3 + c], xi[(long)c * HW]);
        bad |= !(fabsf(m) <= 3.4028234664e38f) || !(fabsf(lp) <= 3.4028234664e38f);
        acc = dadd_rn(acc, (double)(-lp));
    }
    if (status && bad) atomicOr(status, LVAE_STATUS_NONFINITE_IMAGE);
    out[e] = acc;
}

// Composition.  Block i's map holds lat_h x lat_w positions per image, each standing for s x s pixels (s = 2^sh): a pixel takes
// pos * LOG2E / s^2 from every block, added in block order, then the pixel stage's own term.
constexpr int RM_MAX_BLOCKS = 32;
struct RmBlocks {
    const double* pos[RM_MAX_BLOCKS];
    long img[RM_MAX_BLOCKS];                // positions per image
    int lw[RM_MAX_BLOCKS], sh[RM_MAX_BLOCKS];
    double inv[RM_MAX_BLOCKS];              // 2^(-2 sh), exact
};

__global__ __launch_bounds__(256) void rate_map_kernel(RmBlocks blk, int n_blocks, const double* __restrict__ pix, int H, int W,
                                                       float* __restrict__ out, long out_img, long out_row, int crop_h, int crop_w) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)crop_h * crop_w) return;
    const int b = blockIdx.y;
    const int Y = (int)(e / crop_w), X = (int)(e - (long)Y * crop_w);
    const double log2e = 1.4426950408889634;
    double acc = 0.0;
    for (int i = 0; i < n_blocks; ++i) {
        const double v = blk.pos[i][b * blk.img[i] + (long)(Y >> blk.sh[i]) * blk.lw[i] + (X >> blk.sh[i])];
        acc = dadd_rn(acc, dmul_rn(dmul_rn(v, log2e), blk.inv[i]));
    }
    if (pix) acc = dadd_rn(acc, dmul_rn(pix[((long)b * H + Y) * W + X], log2e));
    out[b * out_img + (long)Y * out_row + X] = (float)acc;
}

}  // namespace

extern "C" int lvae_gaussian_nll_pos_f32(const float* prm, const int32_t* sym, double* out, float scale_bound, int B, int HW, int z,
                                         int cdf_form, void* stream) {
    if (!prm || !sym || !out || B <= 0 || HW <= 0 || z <= 0 || (cdf_form != 0 && cdf_form != 1)) return -22;
    const long M = (long)B * HW;
    if ((M + RP_NT - 1) / RP_NT > 0x7fffffffL) return -22;
    hipLaunchKernelGGL(gaussian_nll_pos_kernel, dim3((unsigned)((M + RP_NT - 1) / RP_NT)), dim3(RP_NT), 0, (hipStream_t)stream, prm, sym,
                       out, scale_bound, M, HW, z, cdf_form);
    return (int)hipGetLastError();
}

extern "C" int lvae_pixel_nll_pos_f32(const float* raw6, const float* im, double* out, int B, int H, int W, int* status, void* stream) {
    if (!raw6 || !im || !out || B <= 0 || H <= 0 || W <= 0 || (long)H * W * 6 > 0x7fffffffL) return -22;
    const long total = (long)B * H * W;
    if ((total + 255) / 256 > 0x7fffffffL) return -22;
    hipLaunchKernelGGL(pixel_nll_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw6, im, out, total,
                       H * W, status);
    return (int)hipGetLastError();
}

extern "C" int lvae_rate_map_f32(const double* const* pos, const int* lat_h, const int* lat_w, int n_blocks, const double* pix, int B, int H,
                                 int W, float* out, long out_img, long out_row, int crop_h, int crop_w, void* stream) {
    if (!out || B <= 0 || B > 65535 || H <= 0 || W <= 0 || n_blocks < 0 || n_blocks > RM_MAX_BLOCKS || (n_blocks == 0 && !pix)) return -22;
    if (n_blocks > 0 && (!pos || !lat_h || !lat_w)) return -22;
    if (crop_h <= 0 || crop_h > H || crop_w <= 0 || crop_w > W || out_row < crop_w) return -22;
    if (B > 1 && out_img < (long)(crop_h - 1) * out_row + crop_w) return -22;
    RmBlocks blk = {};
    for (int i = 0; i < n_blocks; ++i) {
        const int lh = lat_h[i], lw = lat_w[i];
        if (!pos[i] || lh <= 0 || lw <= 0 || H % lh || W % lw || H / lh != W / lw) return -22;
        const int s = H / lh;
        if (s & (s - 1)) return -22;
        int sh = 0;
        while ((1 << sh) < s) ++sh;
        blk.pos[i] = pos[i];
        blk.img[i] = (long)lh * lw;
        blk.lw[i] = lw;
        blk.sh[i] = sh;
        blk.inv[i] = 1.0 / ((double)s * (double)s);
    }
    const long per = (long)crop_h * crop_w;
    hipLaunchKernelGGL(rate_map_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, blk, n_blocks,
                       pix, H, W, out, out_img, out_row, crop_h, crop_w);
    return (int)hipGetLastError();
}
