// dwconv_cl.hip -- depthwise k x k conv + bias -> LayerNorm(C) -> per-channel affine (LN weight/bias or AdaLN scale/shift) over an
// NHWC map, "channel-per-lane" form (lvae/models/common.py:145-152; qresvae/model.py:168-176).
//
// The sliding-window kernel of pointwise.hip (and the LDS-tiled forms that preceded this file) give every pixel to a few lanes that
// hold ALL its channels, because the LayerNorm wants them together; the k*k weights of so many channels do not fit in registers, so
// the tap loop is fed from memory / LDS and is bound by fragment reads (17 ds_read_b128 per 56 packed FMAs: DESIGN.md 5b).  Here
// the roles are swapped:
//   * a lane owns ONE CHANNEL of an 8-pixel-wide column strip and keeps its k*k weights in registers (49 weights in 25 register pairs
//     at k = 7); a wave is 64 channels of one strip, a workgroup the C/64 waves of that strip.  Two horizontally adjacent output
//     pixels share one v_pk_fma_f32 (the weight is broadcast to both halves with op_sel_hi; at k = 7 every second weight sits in a
//     high half and is applied with two scalar FMAs -- see pk_fma_wlo); the pixel pairs that start at an odd column are assembled
//     with two moves -- 64-bit operands must be even-aligned;
//   * a workgroup produces tiles of 8 x TH output pixels: the TH + k - 1 input rows of a tile are visited ONCE, top to bottom
//     (8 + k - 1 pixels per lane and row), and each feeds the up to k output rows it belongs to; TH x 8 accumulators per lane.  A tile
//     is straight-line code (every register index static).  No memory access in the tap loop.  Rows reach the registers through
//     wave-private LDS row buffers filled by DMA two rows ahead (dma_row / read_row).  Taps are visited column-major inside a row,
//     which leaves every output's accumulation order -- bias, then taps (i, j) ascending -- unchanged;
//   * a finished output row is transposed through a wave-private LDS tile into a pixel-major layout (8 lanes per pixel, 8 channels
//     per lane: 16-B accesses, 128 B contiguous per pixel and store) for the LayerNorm: 7 adds + 3 DPP steps per lane and
//     statistic; the C/64 waves exchange per-pixel (mean, M2) pairs through LDS -- ONE workgroup barrier per output row, and the
//     part after it is placed inside the next row's taps (ln_local / ln_finish).
// Zero padding comes from the buffer unit: a row's resource descriptor covers exactly that image row (num_records = 0 for rows outside
// the image), so columns left / right of the image and rows above / below read as hardware zeros without masks on the data path
// (LDS-DMA writes zeros for out-of-range lanes: tools/ubench/lds_dma_oob.hip).
// TH (8, 4 or 1 output rows per tile; k - 1 halo rows are re-read per tile, from L2) and the tiles per workgroup only change the
// parallelism, never an output bit, so the launcher picks them from the map size.
//
// Arithmetic: the conv chain is the earlier kernels' (same bits); the LayerNorm uses THIS kernel's association (per wave: mean and
// centred sum of squares of its 64 channels -- 8 channels in a lane, 8 lanes by xor 1, xor 2, half-mirror -- merged over the waves in
// ascending order by the parallel-variance identity) and rstd = v_rsq_f32 refined by one Newton step (the other kernel: 1 / sqrtf),
// so the operator is dispatched to this kernel by (C, k) alone -- never by batch or map size: batch-of-8 == 8 single images, and the
// encoder and the decoder see the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/lvae_hip.h"
#include "dwconv_choice.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sum8(float s) {          // total over the 8 lanes of a pixel group, the same bits in all of them
    s += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0xB1, 0xF, 0xF, true));       // quad_perm [1,0,3,2]
    s += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0x4E, 0xF, 0xF, true));       // quad_perm [2,3,0,1]
    s += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0x141, 0xF, 0xF, true));      // row_half_mirror
    return s;
}
// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope fence, i.e. s_waitcnt vmcnt(0): it would
// wait, twice per output row, for the row DMA issued a moment ago and for the previous row's stores.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// f16x2 operand split (csrc/gemm_common.h::split_pair_h2, lvae.models.base.split_f16x2): hi = f16(x), lo' = f16((x - hi) * 2048)
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair_h2(float x0, float x1, unsigned& hi, unsigned& lo) {
    const f32x2 x = {x0, x1};
    const f16x2_t h = __builtin_convertvector(x, f16x2_t);
    const f32x2 t = x * 2048.0f;
    f16x2_t l;
    l[0] = (_Float16)__builtin_fmaf((float)h[0], -2048.0f, t[0]);
    l[1] = (_Float16)__builtin_fmaf((float)h[1], -2048.0f, t[1]);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ unsigned f2bf_rne(float x) {
    const unsigned u = __float_as_uint(x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// acc += x * w in both halves (two adjacent pixels): v_pk_fma_f32 with the weight in the LOW half of its register pair, broadcast by
// op_sel_hi (the high lane selects the low dword: the form hipcc itself emits for scalar broadcasts).  Inline asm because hipcc gives
// every broadcast scalar a 64-bit pair of its own; at k = 7 the 49 weights must share 25 pairs (98 registers would cost the third wave
// per SIMD), and the weights in the HIGH halves are applied with two scalar v_fmac_f32 instead:
// **a packed op whose LOW lane selects the HIGH dword of an operand (`op_sel` = 1) returned occasional wrong low-lane results on MI355X
// whenever MFMA kernels shared the CUs.**  With the weight pair as src1 (`op_sel:[0,1,0]`) 20-30 % of the launches beside split-K GEMMs
// on a second stream had a few pixels off (always even columns = low lanes; run-to-run different bitstreams in the bf16x3 model only,
// whose GEMMs are MFMA-dense enough), 0 of 400 alone; as src0 (`op_sel:[1,0,0]`) 0 of 1600 -- not trusted either: hipcc never emits
// that selection for packed f32 arithmetic, and the scalar form costs 2 %; its `v_pk_mov_b32 ... op_sel:[1,0]` for a pair assembled from two odd halves
// is the same selection, so those pairs are assembled with two v_mov_b32 here.  tests/test_gpu_kernels.py::test_dwconv_ln_beside_gemms.
// Round 4 settled it at ISA level: tools/ubench/pk_opsel_probe.hip (50 lines: chains of `v_pk_fma_f32 ... op_sel:[0,1,0]` against the
// same chain in scalar v_fma_f32, an MFMA-only kernel on a second stream) -> profiles/r04_ubench_pk_opsel_erratum_probe.txt:
// 832 - 1360 wrong LOW-lane results in 1.0e11 chains with the selection on src1 beside the MFMA kernel, 0 alone; 0 with the selection on
// src0, 0 in the high lane, 0 for the op_sel_hi-only broadcast used here.  A hardware erratum (MI355X, ROCm 7.2), not a race of this
// kernel.  What an all-packed tap loop would buy was timed as well (profiles/r04_dw_bench_all_packed_taps_ab.txt):
// 90.2 -> 87.5 us on the 128x192x192 map, -3 ... -8 % on the k = 7 layers -- too little to stand next to an erratum for, even on the src0 form.
__device__ __forceinline__ void pk_fma_wlo(f32x2& a, f32x2 x, f32x2 w) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(a) : "v"(x), "v"(w));
}
__device__ __forceinline__ void fmac_whi(f32x2& a, float x0, float x1, f32x2 w) {
    asm("v_fmac_f32 %0, %1, %2" : "+v"(a[0]) : "v"(x0), "v"(w[1]));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(a[1]) : "v"(x1), "v"(w[1]));
}
__device__ __forceinline__ f32x2 pair_of(float lo, float hi) {     // two plain moves (never v_pk_mov_b32 with op_sel)
    f32x2 p;
    asm("v_mov_b32 %0, %1" : "=v"(p[0]) : "v"(lo));
    asm("v_mov_b32 %0, %1" : "=v"(p[1]) : "v"(hi));
    return p;
}

// static_for<N>(f): f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>).  The row / pixel loops MUST be unrolled (every
// accumulator and weight index has to be static); `#pragma unroll` gives up above ~10 rows (the accumulators then land in scratch).
template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

using lvae_dwln::CL_SW;                      // output pixels per lane along W
using lvae_dwln::CL_TILE;                    // floats of a wave's transpose tile (dwconv_choice.h: the launcher's estimate needs the LDS footprint)

// amdgpu_waves_per_eu pins the register budget: three waves per SIMD (168 VGPRs) for the k >= 5, TH = 8 tiles, four (128) for the others.
// Measured at k = 7, C = 192: 85 us at three waves, 106 us when two more registers push the kernel to two.
template <int KS, bool BF> struct ClGeom {
    static constexpr int XW = lvae_dwln::cl_xw(KS);                 // input pixels per lane and row
    static constexpr int PPI = lvae_dwln::cl_ppi(BF);               // pixels per LDS-DMA instruction (64 lanes x 16 B = 64 channels x PPI pixels)
    static constexpr int NG = lvae_dwln::cl_ng(KS, BF);             // DMA instructions per row
    static constexpr int ROWF = lvae_dwln::cl_rowf(KS, BF);         // floats of one row buffer (NG KiB)
};

template <int KS, int NW, bool BF> constexpr int cl_lds_bytes() { return lvae_dwln::cl_lds_bytes(KS, NW, BF); }
// waves per SIMD the kernel is compiled for: what the registers allow (above), capped by what 160 KB of LDS lets reside on a CU
template <int KS, int NW, int TH, bool BF> constexpr int cl_waves() {
    const int by_regs = (KS >= 5 && TH == 8) ? 3 : 4;              // k = 5: 25 unpacked weights = 50 registers too
    const int by_lds = ((160 * 1024) / cl_lds_bytes<KS, NW, BF>()) * NW / 4;
    return by_lds < 1 ? 1 : (by_lds < by_regs ? by_lds : by_regs);
}

// OF: output format.  0: like the input map (fp32 / bf16).  1 (fp32 maps only): pre-split for the f16x2 GEMM that consumes it
// (lvae_gemm_desc.a_h2; H2K32 = [pixel][C/32][2][32] fp16: per 32 channels 32 hi terms, then 32 lo' terms -- 4 bytes per element like
// fp32).  2 (bf16 maps, reduced-precision mode): quantised to MX-fp8 for csrc/gemm_q8.hip (format Q8: [pixel][C] e4m3 bytes, then the
// E8M0 block scales as [C/64][pixels][2]; `mtot` = number of pixels of the whole batch).
template <int KS, int NW, int TH, bool BF, int OF = 0>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(cl_waves<KS, NW, TH, BF>(), cl_waves<KS, NW, TH, BF>()))) void dwconv_ln_cl_kernel(
    const void* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias, const float* __restrict__ aw,
    const float* __restrict__ ab, void* __restrict__ y, int H, int W, int n_sx, int n_sy, int tpw, long mtot, long vstride) {
    using G = ClGeom<KS, BF>;
    constexpr bool H2 = OF == 1, Q8 = OF == 2;
    static_assert(!(H2 && BF) && !(Q8 && !BF), "H2 planes come from fp32 maps, Q8 from bf16 maps");
    constexpr int C = 64 * NW, P = (KS - 1) / 2, SW = CL_SW, XW = G::XW, ES = BF ? 2 : 4, KK = KS * KS, NR = TH + KS - 1;
    constexpr int NG = G::NG, ROWF = G::ROWF, PPI = G::PPI;
    static_assert(XW % 2 == 0, "pixel pairs");
    // per wave: the LayerNorm transpose tile and two row buffers; then the waves' statistics [row parity][pixel][wave (8)][mean, M2] and the affine parameters
    constexpr int WAVEF = CL_TILE + 2 * ROWF;
    __shared__ __attribute__((aligned(16))) float lds[NW * WAVEF + 2 * 8 * 8 * 2 + 2 * C];
    static_assert(sizeof(float) * (NW * WAVEF + 2 * 8 * 8 * 2 + 2 * C) == cl_lds_bytes<KS, NW, BF>(), "LDS size formula");
    float* const red = lds + NW * WAVEF;
    float* const prm = red + 2 * 8 * 8 * 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p8 = lane >> 3, blk = lane & 7;          // LayerNorm layout: pixel of the strip, 4-channel block (and block + 8)
    long wg;
    {
        const long nb = gridDim.x, b = blockIdx.x, q = nb / 8, r = nb % 8, xcd = b % 8, loc = b / 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;      // XCD-aware: neighbours in (sy, sx) share an L2
    }
    const int sx = (int)(wg % n_sx), sy = (int)((wg / n_sx) % n_sy);
    const long b = wg / ((long)n_sx * n_sy);
    const int c0 = 64 * wave + lane;                   // conv layout: this lane's channel
    const int x0 = sx * SW;
    int y0 = sy * tpw * TH;                            // this workgroup: tpw vertically consecutive tiles of TH rows (n_sy counts workgroups)
    const int rowbytes = W * C * ES;
    const char* const xin = (const char*)x + b * (long)H * rowbytes;
    char* const yout = (char*)y + b * (long)H * rowbytes;

    auto row_rsrc = [&](const char* base, int r) {     // rows outside the image: an empty descriptor (loads give 0, stores are dropped)
        const bool ok = r >= 0 && r < H;
        return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)(ok ? r : 0) * rowbytes), 0, ok ? rowbytes : 0, 0x00020000);
    };
    // Input rows travel global -> LDS by DMA (buffer_load_dwordx4 ... lds: 16 B per lane, PPI pixels x 64 channels per instruction, no
    // staging registers) and LDS -> registers as one dword per lane and pixel.  Per-lane dword loads straight from global memory are
    // bound by the texture-address unit (one wave instruction per ~16 cycles whatever its width: 16 B/clk/CU at 4 B per lane -- measured
    // 85 us of which 35 were the loads); the DMA form needs 4x fewer vector-memory instructions.
    // A negative offset (left of the image) wraps to a huge unsigned one: out of range like the columns right of the image -> zeros.
    const int dvoff0 = ((x0 - P + lane / (64 / PPI)) * C + 64 * wave + (lane % (64 / PPI)) * (16 / ES)) * ES;
    float* const rowbuf = lds + wave * WAVEF + CL_TILE;
    auto dma_row = [&](int r, int buf) {
        const __amdgpu_buffer_rsrc_t rs = row_rsrc(xin, r);
#pragma unroll
        for (int g = 0; g < NG; ++g)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(rowbuf + buf * ROWF + g * 256), 16,
                                                     dvoff0 + g * PPI * C * ES, 0, 0, 0);
    };
    // k = 7: tap t in wp[t / 2][t % 2] (two weights per register pair); k <= 5: tap t in wp[t][0] (every weight broadcastable)
    constexpr bool PACKW = KS == 7;
    f32x2 wp[PACKW ? (KK + 1) / 2 : KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        if constexpr (PACKW) wp[t / 2][t % 2] = wt[(long)t * C + c0];
        else wp[t] = (f32x2){wt[(long)t * C + c0], 0.f};
    }
    if (PACKW && KK % 2) wp[KK / 2][1] = 0.f;
    const float bias1 = bias[c0];
    // image b's affine vectors start b * vstride elements behind aw / ab (0: one pair for the whole batch); b is wave-uniform, so the
    // base moves in scalar registers and the copy below is the only place that sees it
    prm[tid] = aw ? aw[b * vstride + tid] : 1.f;       // blockDim.x == C
    prm[C + tid] = ab ? ab[b * vstride + tid] : 0.f;
    const int chA = 64 * wave + 4 * blk, chB = chA + 32;

    f32x2 acc[TH][SW / 2];

    // LDS -> registers: the row buffer is read with inline asm (hipcc would guard every LDS load that may alias an LDS-DMA in flight with
    // s_waitcnt vmcnt(0), i.e. wait for the row AFTER the one being read); the vmcnt waits below are exact.  bf16 maps: d16_hi loads
    // put the 16 bits into the upper half of a register whose lower half is (and stays) zero -- the fp32 value, no conversion.
    f32x2 xp[XW / 2];                                  // the input row: pixel m in xp[m / 2][m % 2]
#pragma unroll
    for (int m = 0; m < XW / 2; ++m) xp[m] = (f32x2){0.f, 0.f};
    const unsigned raddr = (unsigned)(unsigned long)(__attribute__((address_space(3))) float*)rowbuf + lane * ES;
    auto read_row = [&](auto buf_tag) {
        constexpr int buf = decltype(buf_tag)::value;
        static_for<XW>([&](auto m_tag) {
            constexpr int m = decltype(m_tag)::value;
            float v = xp[m / 2][m % 2];
            if constexpr (BF) asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "+v"(v) : "v"(raddr), "n"(buf * ROWF * 4 + m * 64 * ES));
            else asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(raddr), "n"(buf * ROWF * 4 + m * 64 * ES));
            xp[m / 2][m % 2] = v;
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the weights are consumed by inline asm: no compiler-placed wait covers them
    __syncthreads();                                   // prm visible
    const float inv_c = 1.0f / (float)C;
    float* const tile = lds + wave * WAVEF;

    // LayerNorm + affine + store of a finished output row, in two phases around ONE workgroup barrier.  ln_local (right after the
    // row's last taps): transpose through the wave's tile, then the statistics of THIS wave's 64 channels -- mean_w and the centred
    // sum of squares M2_w -- go to LDS.  ln_finish (after the barrier, placed a few pixel steps into the NEXT row's taps so that the
    // LDS round trips and the barrier skew hide behind FMAs): the waves' statistics are merged with the parallel-variance identity
    // M2 = sum_w M2_w + 64 sum_w (mean_w - mean)^2 (no cancellation, unlike E[x^2] - mean^2), fixed order over the waves.
    f32x4 lnA, lnB;                                    // the row's values minus mean_w, LayerNorm layout
    float ln_mw;
    auto ln_local = [&](const f32x2 (&a)[SW / 2], int par) {
#pragma unroll
        for (int q = 0; q < SW; ++q) tile[q * 96 + lane] = a[q / 2][q % 2];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // wave-private tile: LDS executes a wave's accesses in order
        f32x4 vA = *(const f32x4*)(tile + p8 * 96 + 4 * blk), vB = *(const f32x4*)(tile + p8 * 96 + 32 + 4 * blk);
        float s = ((vA[0] + vA[1]) + (vA[2] + vA[3])) + ((vB[0] + vB[1]) + (vB[2] + vB[3]));
        s = sum8(s);
        const float mw = s * (1.0f / 64.0f);
        float m2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { vA[e] -= mw; m2 = fmaf(vA[e], vA[e], m2); }
#pragma unroll
        for (int e = 0; e < 4; ++e) { vB[e] -= mw; m2 = fmaf(vB[e], vB[e], m2); }
        m2 = sum8(m2);
        if (blk == 0) *(f32x2*)(red + par * 128 + (p8 * 8 + wave) * 2) = (f32x2){mw, m2};
        lnA = vA; lnB = vB; ln_mw = mw;
    };
    auto ln_finish = [&](int ya, int par) {
        const float* r = red + par * 128 + p8 * 16;                    // [wave][mean_w, M2_w]
        float msum = r[0], m2 = r[1];
#pragma unroll
        for (int v = 1; v < NW; ++v) { msum += r[2 * v]; m2 += r[2 * v + 1]; }
        const float mean = msum * (1.0f / (float)NW);
        float dev = 0.f;
#pragma unroll
        for (int v = 0; v < NW; ++v) { const float dm = r[2 * v] - mean; dev = fmaf(dm, dm, dev); }
        // the affine parameters come from LDS: in registers across the tap loop they would cost 16 VGPRs (what separates the k = 7,
        // TH = 8 instance from three waves per SIMD), and global loads here would share the in-order vmcnt with the row DMA
        const f32x4 awA = *(const f32x4*)(prm + chA), awB = *(const f32x4*)(prm + chB);
        const f32x4 abA = *(const f32x4*)(prm + C + chA), abB = *(const f32x4*)(prm + C + chB);
        const float var = fmaf(fmaf(64.0f, dev, m2), inv_c, 1e-6f);    // >= 1e-6: no special cases for the reciprocal square root
        float rstd = __builtin_amdgcn_rsqf(var);
        rstd = rstd * fmaf(-0.5f * var, rstd * rstd, 1.5f);            // one Newton step
        const float sh = ln_mw - mean;                                 // x - mean = (x - mean_w) + (mean_w - mean)
        const int xs = x0 + p8;
        const __amdgpu_buffer_rsrc_t ro = row_rsrc(yout, ya);
        f32x4 oA, oB;
#pragma unroll
        for (int e = 0; e < 4; ++e) { oA[e] = fmaf((lnA[e] + sh) * rstd, awA[e], abA[e]); oB[e] = fmaf((lnB[e] + sh) * rstd, awB[e], abB[e]); }
        if constexpr (Q8) {
            // MX-fp8: the 8 lanes of a pixel hold one 32-channel block each in oA (block 2 wave) and oB (block 2 wave + 1): block amax by
            // DPP, scale = 2^e with amax / 2^e in (224, 448] (the rule of gemm_lp.hip::lp_quant8 / pack_mxfp8), 4 bytes per lane and block
            auto max8 = [](float m) {
                m = fmaxf(m, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(m), 0xB1, 0xF, 0xF, true)));
                m = fmaxf(m, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(m), 0x4E, 0xF, 0xF, true)));
                m = fmaxf(m, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(m), 0x141, 0xF, 0xF, true)));
                return m;
            };
            auto quant4 = [&](const f32x4& o, unsigned& eb_out) {
                const unsigned ab = __float_as_uint(max8(fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3])))));
                int eb = (int)((ab >> 23) & 0xffu) - 8;
                if ((ab & 0x7fffffu) > 0x600000u) eb += 1;
                eb = eb < 1 ? 1 : (eb > 254 ? 254 : eb);
                const float inv = __uint_as_float((unsigned)(254 - eb) << 23);
                int w = 0;
                w = __builtin_amdgcn_cvt_pk_fp8_f32(o[0] * inv, o[1] * inv, w, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(o[2] * inv, o[3] * inv, w, true);
                eb_out = (unsigned)eb;
                return (unsigned)w;
            };
            unsigned eA, eB;
            const unsigned wA = quant4(oA, eA), wB = quant4(oB, eB);
            const bool rok = ya >= 0 && ya < H;
            const long m0r = (b * H + (rok ? ya : 0)) * (long)W;                                   // first pixel of this image row
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)y + m0r * C), 0, rok ? W * C : 0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsq = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)y + mtot * C + ((long)wave * mtot + m0r) * 2), 0,
                                                                                   rok ? W * 2 : 0, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b32(wA, rq, xs * C + 64 * wave + 4 * blk, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(wB, rq, xs * C + 64 * wave + 32 + 4 * blk, 0, 0);
            if (blk == 0) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(eA | (eB << 8)), rsq, xs * 2, 0, 0);
        } else if constexpr (H2) {
            // this lane's channels chA .. chA + 3 sit at position 4 blk of 32-channel block 2 wave, chB .. + 3 at the same position of
            // block 2 wave + 1; a block is 64 B of hi terms followed by 64 B of lo' terms
            unsigned h0, l0, h1, l1;
            const int base = (xs * C + 64 * wave) * 4 + 8 * blk;
            split_pair_h2(oA[0], oA[1], h0, l0); split_pair_h2(oA[2], oA[3], h1, l1);
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){h0, h1}, ro, base, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){l0, l1}, ro, base + 64, 0, 0);
            split_pair_h2(oB[0], oB[1], h0, l0); split_pair_h2(oB[2], oB[3], h1, l1);
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){h0, h1}, ro, base + 128, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){l0, l1}, ro, base + 192, 0, 0);
        } else if (BF) {
            const u32x2 qa = {f2bf_rne(oA[0]) | (f2bf_rne(oA[1]) << 16), f2bf_rne(oA[2]) | (f2bf_rne(oA[3]) << 16)};
            const u32x2 qb = {f2bf_rne(oB[0]) | (f2bf_rne(oB[1]) << 16), f2bf_rne(oB[2]) | (f2bf_rne(oB[3]) << 16)};
            __builtin_amdgcn_raw_buffer_store_b64(qa, ro, (xs * C + chA) * 2, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(qb, ro, (xs * C + chB) * 2, 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, oA), ro, (xs * C + chA) * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, oB), ro, (xs * C + chB) * 4, 0, 0);
        }
    };
    constexpr int LN_AT = 3;                           // pixel step of the next row at which the previous row's LayerNorm is finished

    // The k x k weights (49 dword loads per lane, as many vector-memory instructions as 12 rows of DMA) are loaded once per workgroup and
    // serve tpw tiles; the launcher picks tpw so that the workgroups still fill the chip in whole rounds.
    for (int it = 0; it < tpw && y0 < H; ++it, y0 += TH) {
    dma_row(y0 - P, 0);
    if constexpr (NR > 1) dma_row(y0 - P + 1, 1);
#pragma unroll
    for (int th = 0; th < TH; ++th)
#pragma unroll
        for (int q = 0; q < SW / 2; ++q) acc[th][q] = (f32x2){bias1, bias1};
    // row 0 has landed (row 1 may still be in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NR > 1 ? NG : 0) : "memory");
    read_row(std::integral_constant<int, 0>{});
    static_for<NR>([&](auto t_tag) {                                 // input row y0 - P + t feeds output rows th = t - i, 0 <= i < k
        constexpr int t = decltype(t_tag)::value;
        // row t + 2 -> the buffer row t came from (it is in registers since the end of the previous step)
        if constexpr (t + 2 < NR) dma_row(y0 - P + t + 2, t % 2);
        __builtin_amdgcn_sched_barrier(0);
        static_for<XW - 1>([&](auto s_tag) {                         // the pixel pair (s, s + 1)
            constexpr int s = decltype(s_tag)::value;
            if constexpr (s == LN_AT && t - 1 >= KS - 1) {
                lds_barrier();
                ln_finish(y0 + t - 1 - (KS - 1), (t - 1) % 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            const float x0 = xp[s / 2][s % 2], x1 = xp[(s + 1) / 2][(s + 1) % 2];
            f32x2 xv;
            if constexpr (s % 2 == 0) xv = xp[s / 2];
            else xv = pair_of(x0, x1);
#pragma unroll
            for (int th = 0; th < TH; ++th) {
                const int i = t - th;
                if (i < 0 || i >= KS) continue;
#pragma unroll
                for (int j = 0; j < KS; ++j) {
                    const int q = s - j;
                    if (q >= 0 && q < SW && q % 2 == 0) {
                        const int tap = i * KS + j;
                        if (!PACKW) pk_fma_wlo(acc[th][q / 2], xv, wp[tap]);
                        else if (tap % 2 == 0) pk_fma_wlo(acc[th][q / 2], xv, wp[tap / 2]);
                        else fmac_whi(acc[th][q / 2], x0, x1, wp[tap / 2]);
                    }
                }
            }
        });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (t + 1 < NR) {
            // Row t + 1 has landed once at most NG vector-memory operations are outstanding: loads retire in order among loads, so
            // row t + 2's NG DMA instructions cannot complete before row t + 1's.  Stores retire independently of loads (a store may
            // overtake an older load), so they must NOT be added to the allowance: an earlier form that allowed NG + 2 for a row's
            // two stores read half-landed rows under memory load.
            // (Reading the row pixel by pixel behind the taps, each into the register of the pixel that just died, was tried: no gain.
            //  Round 5: warming L2 with one dword per 128-B line of the tile's rows 2 .. NR - 1 at the tile's start -- LDS-DMA touches older than the
            //  row DMAs, so that those hit L2 -- was measured SLOWER on every shape, 88 -> 95 us at k = 7 / C = 192, 61 -> 82 at C = 384:
            //  profiles/r05_dw_l2_touch_not_taken.txt.  The first wait of a tile then waits for all of them.)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(t + 2 < NR ? NG : 0) : "memory");
            read_row(std::integral_constant<int, (t + 1) % 2>{});
        }
        if constexpr (t >= KS - 1) ln_local(acc[t - (KS - 1)], t % 2);
    });
    lds_barrier();
    ln_finish(y0 + TH - 1, (NR - 1) % 2);
    lds_barrier();                                     // the statistics buffers are free for the next tile
    }
}

template <int KS, int NW, int TH, bool BF, int OF>
int launch_cl_th(const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y, int B, int H, int W,
                 int tpw, long vs, hipStream_t st) {
    const int n_sx = (W + CL_SW - 1) / CL_SW, n_ty = (H + TH - 1) / TH, n_sy = (n_ty + tpw - 1) / tpw;
    const long grid = (long)B * n_sx * n_sy;
    if (grid > 0x7fffffffL || (long)H * W * 64 * NW * (BF ? 2 : 4) > 0x7fffffffL) return -22;
    hipLaunchKernelGGL((dwconv_ln_cl_kernel<KS, NW, TH, BF, OF>), dim3((unsigned)grid), dim3(64 * NW), 0, st, x, wt, bias, aw, ab, y, H, W,
                       n_sx, n_sy, tpw, (long)B * H * W, vs);
    return (int)hipGetLastError();
}

// TH (output rows per tile) and tpw (tiles per workgroup) come from dwconv_choice.h::choose -- the function lvae_dwconv_ln_choice
// reports -- and only select the instance here.
template <int KS, int NW, bool BF, int OF>
int launch_cl(const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y, int B, int H, int W,
              int th, int tpw, long vs, hipStream_t st) {
    if constexpr (KS > 1) {
        if (th == 8) return launch_cl_th<KS, NW, 8, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, tpw, vs, st);
        if (th == 4) return launch_cl_th<KS, NW, 4, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, tpw, vs, st);
    }
    if (th == 1) return launch_cl_th<KS, NW, 1, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, tpw, vs, st);
    return -22;                                                        // not an instance (the choice never names one)
}

template <int KS, bool BF, int OF = 0>
int launch_cl_c(int C, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y, int B, int H,
                int W, int th, int tpw, long vs, hipStream_t st) {
    switch (C) {
        case 128: return launch_cl<KS, 2, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 192: return launch_cl<KS, 3, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 256: return launch_cl<KS, 4, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 384: return launch_cl<KS, 6, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 512: return launch_cl<KS, 8, BF, OF>(x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
    }
    return -22;
}

}  // namespace

// This source is compiled three times (build_native.py): as is (fp32 maps + the entry point), through dwconv_cl_bf16.hip with
// LVAE_CL_BF16_TU (the bf16-map instances) and through dwconv_cl_h2.hip with LVAE_CL_H2_TU (fp32 maps in, pre-split f16x2 planes out)
// and through dwconv_cl_q8.hip with LVAE_CL_Q8_TU (bf16 maps in, MX-fp8 out) -- the translation units compile in parallel, the
// instances take minutes otherwise.
#if defined(LVAE_CL_Q8_TU)
int lvae_dwln_cl_launch_q8(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                           int B, int H, int W, int th, int tpw, long vs, hipStream_t st) {
    switch (k) {
        case 1: return launch_cl_c<1, true, 2>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 3: return launch_cl_c<3, true, 2>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 5: return launch_cl_c<5, true, 2>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 7: return launch_cl_c<7, true, 2>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
    }
    return -22;
}
#elif defined(LVAE_CL_H2_TU)
int lvae_dwln_cl_launch_h2(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                           int B, int H, int W, int th, int tpw, long vs, hipStream_t st) {
    switch (k) {
        case 1: return launch_cl_c<1, false, 1>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 3: return launch_cl_c<3, false, 1>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 5: return launch_cl_c<5, false, 1>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 7: return launch_cl_c<7, false, 1>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
    }
    return -22;
}
#elif defined(LVAE_CL_BF16_TU)
int lvae_dwln_cl_launch_bf16(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                             int B, int H, int W, int th, int tpw, long vs, hipStream_t st) {
    switch (k) {
        case 1: return launch_cl_c<1, true>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 3: return launch_cl_c<3, true>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 5: return launch_cl_c<5, true>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 7: return launch_cl_c<7, true>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
    }
    return -22;
}
#else
int lvae_dwln_cl_launch_bf16(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                             int B, int H, int W, int th, int tpw, long vs, hipStream_t st);
int lvae_dwln_cl_launch_h2(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                           int B, int H, int W, int th, int tpw, long vs, hipStream_t st);
int lvae_dwln_cl_launch_q8(int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                           int B, int H, int W, int th, int tpw, long vs, hipStream_t st);

// Entry point for pointwise.hip's dispatcher, for the launches that dwconv_choice.h::choose gives to this kernel (family 0: C in
// {128, 192, 256, 384, 512}, k in {1, 3, 5, 7}, at most ONE per-channel affine aw / ab after the normalisation); th / tpw are that
// choice's tile rows and tiles per workgroup.  fmt: 0 fp32 maps, 1 bf16 maps, 2 fp32 in / f16x2 planes out, 3 bf16 in / MX-fp8 out.
// vs: element stride between consecutive images' affine vectors (0: one pair for the batch -- the lvae_dwconv_ln_* entry points; > 0:
// the lvae_dwconv_ln_*_v ones, image b reads ab + b * vs / aw + b * vs).
int lvae_dwln_cl_launch(int fmt, int C, int k, const void* x, const float* wt, const float* bias, const float* aw, const float* ab, void* y,
                        int B, int H, int W, int th, int tpw, long vs, hipStream_t st) {
    switch (fmt) {
        case 3: return lvae_dwln_cl_launch_q8(C, k, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 1: return lvae_dwln_cl_launch_bf16(C, k, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 2: return lvae_dwln_cl_launch_h2(C, k, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
        case 0:
            switch (k) {
                case 1: return launch_cl_c<1, false>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
                case 3: return launch_cl_c<3, false>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
                case 5: return launch_cl_c<5, false>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
                case 7: return launch_cl_c<7, false>(C, x, wt, bias, aw, ab, y, B, H, W, th, tpw, vs, st);
            }
    }
    return -22;
}
#endif
