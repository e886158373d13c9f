/*
 * include/lvae_hip.h -- C ABI of liblvae_hip.so, the MI355X-native (gfx950) drop-in for the native code the
 * reference's QARV / QRes-VAE encode+decode hot path reaches.
 *
 * The reference (duanzhiihao/lossy-vae) is 100% Python; its hot path crosses into native code only through
 * third-party packages:
 *   - CompressAI pybind11 entry points  RansEncoder.encode_with_indexes / RansDecoder.decode_with_indexes /
 *     pmf_to_quantized_cdf, reached at  lvae/models/qarv/model.py:107,113,124  and
 *     lvae/models/qresvae/model.py:325,339,356  -> replaced by the `lvae_rans_*` / `lvae_pmf_*` host functions;
 *   - ATen/cuDNN/cuBLAS kernels behind  lvae/models/common.py:142-161 (ConvNeXtBlockAdaLN.forward),
 *     common.py:29-38 (patch_downsample / patch_upsample), qarv/model.py:36-39,44-75 (prior / posterior /
 *     z_proj convs, softplus/exp, build_indexes, quantize)  -> replaced by the `lvae_*_f32` device launchers.
 *
 * Conventions
 *   - Plain C: raw pointers + sizes; no torch types.  Device pointers are owned by the caller (in the Python
 *     host they are torch tensors' data_ptr()); all device launchers are asynchronous on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream) and return a hipError_t as int (0 = success),
 *     or a negative value for argument errors detected on the host.
 *   - Activations are NHWC fp32 ([B][H][W][C], C contiguous); a "row" m is one pixel (b,h,w).
 *   - Host coder functions are thread-safe and stateless (no globals); caller owns all buffers.
 *   - Entropy-coder streams are byte-compatible with the oracle restatement of CompressAI's rANS
 *     (oracle/rans_oracle.c): 64-bit rANS (ryg rans64), 16-bit precision, 4-bit bypass escapes.
 */
#ifndef LVAE_HIP_H
#define LVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ meta */
int lvae_abi_version(void);          /* bumps on any signature change */
const char* lvae_build_info(void);   /* "gfx950 hipcc <ver> ..." */

/* ------------------------------------------------------------------------------------------------ host coder
 * Replaces compressai._CXX.pmf_to_quantized_cdf(list[float], int) -> list[int]
 * (called from GaussianConditional.update(): qarv/model.py:123-124, qresvae/model.py:317-325).
 * cdf_out has n+1 entries.  Returns 0, or -1 (negative / non-finite pmf), -2 (zero total), -3 (cannot fix up). */
int lvae_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* cdf_out);

/* Whole-table builder (GaussianConditional.update() semantics): for each of n_scales scales
 * c=ceil(scale*m), len=2c+1, pmf[k]=Phi((.5-|k-c|)/s)-Phi((-.5-|k-c|)/s) in fp32, tail=2*lower[0],
 * row=pmf_to_quantized_cdf([pmf, tail]).  cdf_form: 0 = erf form 0.5*(1+erf(x/sqrt2)) (DiscretizedGaussian,
 * lvae/models/entropy_coding.py:81-82), 1 = erfc form 0.5*erfc(-x/sqrt2) (stock GaussianConditional, qres34m).
 * `multiplier` = -ppf(tail_mass/2) (6.10941... for 1e-9).  qcdf is [n_scales][row_stride] int32, zero-filled
 * beyond each row's length; cdf_len[i]=len_i+2; offset[i]=-c_i.  Returns max row length (+2) or <0.
 * NOTE: uses the C library's erff/erfcf; the Python host's update() uses torch ops exactly like the reference
 * so that tables are bit-identical to it -- this entry point is for non-Python integrators. */
int lvae_build_gaussian_tables(const float* scale_table, int n_scales, double multiplier, int cdf_form,
                               int32_t* qcdf, int row_stride, int32_t* cdf_len, int32_t* offset);

/* Replaces RansEncoder().encode_with_indexes(symbols, indexes, cdfs, cdf_sizes, offsets) -> bytes
 * (qarv/model.py:107 via GaussianConditional.compress).  One call = one self-contained stream.
 * Returns bytes written (multiple of 4, >= 8) or <0: -2 = out_cap too small, -4 = bad index. */
long lvae_rans_encode_with_indexes(const int32_t* sym, const uint8_t* idx, size_t n,
                                   const int32_t* qcdf, int row_stride, const int32_t* cdf_len,
                                   const int32_t* offset, uint8_t* out, size_t out_cap);

/* Test hook of the encoder's division-free step: lvae_rans_encode_with_indexes computes x' = ((x / freq) << 16) + (x % freq) + start with
 * a per-symbol reciprocal (Alverson; the form of ryg's rans64.h -- the published coder divides).  This applies ONE encode step to the
 * state x both ways (division / reciprocal) and returns both next states; 0 if the renormalisation decisions agree too.  1 <= freq <= 65535. */
int lvae_rans_enc_step_selftest(uint64_t x, uint32_t start, uint32_t freq, uint64_t* by_division, uint64_t* by_reciprocal);

/* Replaces RansDecoder().decode_with_indexes(bytes, indexes, cdfs, cdf_sizes, offsets) -> list[int]
 * (qarv/model.py:113 via GaussianConditional.decompress).  Returns 0 or <0 (-1 malformed, -3 overrun). */
int lvae_rans_decode_with_indexes(const uint8_t* in, size_t in_len, const uint8_t* idx, size_t n,
                                  const int32_t* qcdf, int row_stride, const int32_t* cdf_len,
                                  const int32_t* offset, int32_t* sym_out);

/* Batched variants: n_streams independent streams coded by up to n_threads host threads (0 = hardware
 * concurrency).  Stream s uses sym[s]/idx[s]/n[s]; outputs land in out[s] (capacity out_cap[s]) and
 * out_len[s] receives the byte count (or the negative error).  Returns 0 if all streams succeeded. */
int lvae_rans_encode_batch(int n_streams, const int32_t* const* sym, const uint8_t* const* idx, const size_t* n,
                           const int32_t* qcdf, int row_stride, const int32_t* cdf_len, const int32_t* offset,
                           uint8_t* const* out, const size_t* out_cap, long* out_len, int n_threads);
int lvae_rans_decode_batch(int n_streams, const uint8_t* const* in, const size_t* in_len,
                           const uint8_t* const* idx, const size_t* n,
                           const int32_t* qcdf, int row_stride, const int32_t* cdf_len, const int32_t* offset,
                           int32_t* const* sym_out, int* status, int n_threads);

/* ------------------------------------------------------------------------------------------------ status word
 * One device int per launch plan, zeroed by the caller, OR-ed into by the kernels that are handed its address, copied to the host at
 * synchronisation points the codec already has (lvae_encode_blocks / lvae_decode_blocks do it per latent block).
 *   RANGE            an input pixel outside [0, 1] or NaN -- the reference's `assert 0 <= im.min() <= im.max() <= 1`
 *                    (qarv/model.py:219-220, qresvae/model.py:492), raised by the stem / range kernels;
 *   NONFINITE_PRIOR  a prior parameter (mean or log-scale, qarv/model.py:51-53) is NaN / inf        (lvae_prior_index_f32,
 *                    lvae_lossless_params_f32);
 *   NONFINITE_LATENT a posterior mean / quantised latent is NaN / inf or does not fit an int32      (lvae_quantize_f32);
 *   NONFINITE_IMAGE  a reconstruction value is NaN / inf before the final clamp                     (ST_IMAGE store, lvae_lossless_output_f32).
 * Why: the reference computes its 1x1 convs / MLPs in fp32 (common.py:154, qarv/model.py:36-39) and cannot overflow at 65504; the default
 * arithmetic here (prec 4, "f16x2") splits every operand into fp16 terms, so an activation >= 65520 becomes inf in its hi term.  An
 * inf / NaN never turns back into a finite value on the way (MFMA sums, GELU, residual adds, LayerNorm all propagate it), and every
 * tensor of the codec ends in one of the three sinks above -- the encoder's features in a posterior mean, the top-down state in the next
 * prior or in the image -- so checking the sinks catches every overflow before a byte string or an image is returned.  The Python host
 * raises lvae.NonFiniteError naming `model.set_gemm_precision('bf16x3')` (bf16 terms have fp32's exponent range). */
enum {
    LVAE_STATUS_RANGE = 1, LVAE_STATUS_NONFINITE_PRIOR = 2, LVAE_STATUS_NONFINITE_LATENT = 4, LVAE_STATUS_NONFINITE_IMAGE = 8
};

/* ------------------------------------------------------------------------------------------------ device kernels
 * GEMM family: out[m][n] = epilogue( sum_k A[m][k] * Wt[n][k] + bias[n] ), fp32 in / fp32 accumulate on
 * v_mfma_f32_32x32x2_f32.  Replaces timm Mlp fc1/fc2 (common.py:131-132,154), conv 1x1 (qarv/model.py:36,38,39;
 * common.py:33-38), conv k=s patch_downsample (common.py:29-30) and the 3x3 posterior head (qarv/model.py:37). */
enum {
    LVAE_A_PLAIN  = 0,  /* A row m = [A0[m*lda0 .. +K0) , A1[m*lda1 .. +K1)]   (A1 optional: fused torch.cat) */
    LVAE_A_PATCH2 = 1,  /* 2x2/stride-2 patches of an NHWC [B][2H][2W][Cin] map; K = 4*Cin, order (i,j,ci)    */
    LVAE_A_CONV3  = 2   /* 3x3/pad-1 taps of an NHWC [B][H][W][Cin] map;       K = 9*Cin, order (i,j,ci)      */
};
enum {
    LVAE_EPI_BIAS       = 0,  /* acc + bias                                                                   */
    LVAE_EPI_BIAS_GELU  = 1,  /* gelu_erf(acc + bias)                 (fc1, common.py:132 nn.GELU exact form) */
    LVAE_EPI_GAMMA_RES  = 2,  /* res + gamma[n]*(acc + bias)          (fc2 + layer-scale + shortcut, :157-160) */
    LVAE_EPI_RES        = 3   /* res + acc + bias                     (fuse_feature_and_z, qarv/model.py:72-75) */
};
enum {
    LVAE_ST_ROWMAJOR    = 0,  /* out[m*ldo + n]                                                               */
    LVAE_ST_SHUFFLE     = 2,  /* PixelShuffle(r) into NHWC [B][H*r][W*r][N/r^2]; columns pre-permuted to
                                 n' = (i*r+j)*Cout + c  (common.py:33-38)                                     */
    LVAE_ST_IMAGE       = 3   /* final layer: PixelShuffle(r) + clamp(-1,1)*0.5+0.5 into NCHW [B][N/r^2][H*r][W*r];
                                 columns in the reference order n = c*r^2 + i*r + j (qarv/model.py:224-232)  */
};
typedef struct {
    const float* A0; const float* A1;     /* A sources (A1 may be NULL) */
    long lda0, lda1;                      /* row strides in floats (PLAIN) */
    int  K0, K1;                          /* PLAIN: lengths of the two sources; PATCH2/CONV3: K0 = Cin */
    int  H, W;                            /* PATCH2/CONV3/SHUFFLE/IMAGE: spatial size of the row grid (rows = B*H*W) */
    const float* Wt; long ldw;            /* weights [N][K], K contiguous */
    const float* bias;                    /* [N] */
    const float* gamma;                   /* [N]  (EPI_GAMMA_RES) */
    const float* res; long ldres;         /* residual rows (EPI_GAMMA_RES / EPI_RES); may alias out */
    float* out; long ldo;
    int  M, N, K;                         /* K = total reduction length */
    int  a_mode, epi, store, r;           /* r = pixel-shuffle factor */
    int  a_gelu;                          /* 1: apply gelu_erf to every A element on load (VDBlock's c1(gelu(x)),
                                             lvae/models/qresvae/model.py:143-144) */
    int  prec;                            /* 0: fp32 MFMA (v_mfma_f32_32x32x2_f32, an exact fmaf chain);
                                             1: operands rounded to bf16 (RNE), fp32 accumulate on v_mfma_f32_32x32x16_bf16
                                                (BASELINE config 5, not the parity path);
                                             2: "bf16x3": each fp32 operand split exactly into hi+mid+lo bf16 terms, six
                                                cross-term bf16 MFMAs per step, fp32 accumulate -- fp32-class accuracy
                                                (relative error of a product <= 2^-24).  prec 1/2 need Wt16, K % 8 == 0 */
                                          /* 3: REDUCED precision (BASELINE config 5): activations stored as bf16, operands quantised to
                                                OCP MX-fp8 (e4m3 + one E8M0 scale per 32 k) on v_mfma_scale_f32_32x32x64_f8f6f4, fp32
                                                accumulate; Wt16 = [N][ldw] e4m3 bytes then [N][ldw/32] scale bytes, ldw = K rounded
                                                up to 64 (zero padded; lvae.models.base.pack_mxfp8).  Not a parity path */
                                          /* 4: "f16x2": each fp32 operand split into hi + lo' * 2^-11 fp16 terms (23 of fp32's 24
                                                significant bits), three cross-term fp16 MFMAs per step (hi*hi | hi*lo' + lo'*hi in a
                                                second fp32 accumulator) -- fp32-class accuracy at half the matrix-pipe time of prec 2;
                                                operands must stay below 65504 in magnitude.  PLAIN (incl. [A0 | A1]), CONV3 and PATCH2 A
                                                modes, K % 32 == 0 -- or K % 16 == 0 with N <= 96, one PLAIN / CONV3 source, no a_gelu
                                                (csrc/gemm_h2n.hip) -- ldw == K; Wt16 = [N][K/16][2][16] fp16 (lvae.models.base.pack_f16x2).
                                                Selected by the host per GEMM (csrc/gemm_h2.hip; cfg: 0 = the library chooses kernel and
                                                tile, 1 / 2 = gemm_h2_kernel with 64 / 128-wide tiles, 3 = gemm_h2n_kernel wherever it
                                                applies -- every choice gives the same bits) */
    const unsigned short* Wt16;           /* prec 1: weights as bf16 bit patterns, [N][K], row stride ldw;
                                             prec 2: three such planes hi | mid | lo, plane stride N*ldw elements,
                                             followed -- when K % 32 == 0 and ldw == K -- by the same values in
                                             k16-interleaved order [N][K/16][3][16] (lvae.models.base.pack_bf16x3) */
    int  cfg;                             /* tile configuration (prec 0 / 1 / 2): 0 = library heuristic, k>0 = candidate k-1 of
                                             lvae_gemm_num_configs(), -22 beyond it (results are bit-identical for every choice;
                                             the Python host passes 0; tests/test_gpu_gemm_configs.py forces the others).  The two
                                             64-deep candidates (k = 11, 12) exist for prec 0 without split-K only: elsewhere they
                                             run the 32-deep tile of the same shape (k = 3, 2), and k = 8 (128 x 256) runs k = 4
                                             (256 x 256) under prec 2.  prec 3 reads its own codes here (see `prec`).
                                             prec 4 (every choice gives the same bits; tests/test_gpu_h2_instances.py forces each):
                                             a_h2 = 0: 0 = the library chooses kernel and tile; 1 / 2 = gemm_h2_kernel with
                                             128 x 64 / 128 x 128 tiles (TN = 1 / 2; -22 where K % 32 != 0); 3 = gemm_h2n_kernel
                                             wherever it applies (N <= 96, one PLAIN / CONV3 source, no a_gelu / out_h2), else as 0.
                                             a_h2 = 1 (csrc/gemm_h2p.hip, rows x columns): 42 = 256 x 128, 41 = 256 x 64,
                                             22 = 128 x 128, 21 = 128 x 64 with three LDS stages, 23 = 128 x 64 with two; any other
                                             value = the library's choice; ignored under ksplit > 1, where the serial form runs
                                             128 x 64 tiles with loader waves while ceil(M/128) * ceil(N/64) <= CU count and
                                             without them beyond */
    int  ksplit;                          /* split-K: S > 1 cuts K into S equal slices (K % (32*S) == 0) computed by S x tiles
                                             workgroups into `ws`, then reduced IN SLICE ORDER and passed through the epilogue by a
                                             second kernel -- deterministic; for the few-tile, long-K layers (stride 32/64 MLPs, 3x3
                                             heads).  Row-major store only, N % 4 == 0.  The host must choose S independently of
                                             the batch size (per-image rows), so that batched and single-image calls agree */
    float* ws;                            /* split-K workspace, S*M*N floats (unused when ksplit <= 1) */
    int  a_bf16, out_bf16;                /* prec 3 only: A (both sources) / out and res are bf16 bit patterns (2-byte elements;
                                             lda, ldo, ldres stay in ELEMENTS); 0 = fp32.  The final NCHW image is always fp32 */
    int* cnt;                             /* split-K arrival counters, one int per output tile (>= ceil(M/64)*ceil(N/32) entries covers
                                             every tile shape), ZERO before the first launch; each launch leaves them zero again.
                                             Non-NULL: the last slice workgroup of a tile to arrive reduces the S slabs in slice order
                                             inside the GEMM launch (no second kernel; same bits).  NULL: separate reduce launch */
    int* status;                          /* optional device status word (LVAE_STATUS_* bits, above): the final-image store (ST_IMAGE) ORs
                                             LVAE_STATUS_NONFINITE_IMAGE into it when a value is NaN / inf before the clamp (the clamp would
                                             hide it).  NULL = no check */
    int  a_h2, out_h2;                    /* prec 4 only, "pre-split" operands in the f16x2 plane format H2K32 = [rows][K/32][2][32] fp16
                                             (per 32 k: 32 hi terms, then 32 lo' terms; a row is K*4 bytes like its fp32 form;
                                             lvae.models.base.pack_f16x2_k32): a_h2 = 1: A0 is such a buffer (PLAIN, K1 = 0, lda0 = K,
                                             K % 32 == 0), written by a producer with out_h2 (lvae_dwconv_ln_h2, a GEMM) -- the GEMM then
                                             streams both operands global -> LDS by DMA with no conversion in its main loop
                                             (csrc/gemm_h2p.hip; Wt16 must be H2K32 as well).  out_h2 = 1: the result (ROWMAJOR,
                                             EPI_BIAS / EPI_BIAS_GELU, N % 32 == 0, ldo = N) is stored split in that format instead
                                             of fp32.  Same bits as splitting inside the consumer: the split is exact and unique.
                                             prec 3 (reduced-precision mode): the same two flags with the MX-fp8 operand format Q8 of an
                                             [R][K] matrix (K % 64 == 0): R*K e4m3 bytes row-major, then the E8M0 block scales as
                                             [K/64][R][2] bytes (lvae.models.base.pack_mxfp8_q8): a_h2 = 1: A0 (and Wt16) are Q8 buffers,
                                             written by lvae_dwconv_ln_q8 / a GEMM with out_h2 (csrc/gemm_q8.hip: no quantiser in the main
                                             loop); out_h2 = 1: the result (EPI_BIAS / EPI_BIAS_GELU, N % 64 == 0, ldo = N) is stored as Q8 */
    int  defer_reduce;                    /* ksplit > 1, parallel form only: 1 = the launch writes the S partial-sum planes to `ws` and does NOT
                                             run the reduce pass (no bias / epilogue is applied): a consumer that reads the planes itself
                                             finishes the job -- lvae_prior_index_sk_f32 sums them in slice order, adds the bias and goes on to
                                             the scale indexes: one launch less per latent block, the bits of the two-launch form (round 6) */
} lvae_gemm_desc;
int lvae_gemm_f32(const lvae_gemm_desc* d, void* stream);

/* The MLP of a ConvNeXt block as ONE launch (f16x2 arithmetic, pre-split operands; csrc/mlp_h2c.hip; common.py:131-132,154-158):
 *     out[m][c] = res[m][c] + gamma[c] * ( fc2( gelu_erf( fc1(y)[m] + b1 ) )[c] + b2[c] )
 * One persistent 512-thread workgroup per CU walks 128-row (C = 384: 64-row) tiles; per tile the hidden dimension is walked in chunks
 * that stay in the CU's LDS, both weight matrices are STREAMED by LDS-DMA (they do not fit a CU).  Instances: (C, hid) = (128, 192) -- the
 * decoder's stride-4 blocks (qarv/zoo.py:86-87; since round 5 the tile's A rows are resident in LDS: fetched once per tile, one tile ahead), (192, 384) -- the encoder's stride-4 blocks (qarv/zoo.py:38-40) and qres34m's,
 * (384, 768) -- the stride-8 blocks, taken by the host from M = 49152 rows on (lvae.engine.Plan.FUSED_MLP_MIN_ROWS).  -22 for any other
 * (C, hid) and for M * C * 4 >= 2^31 (32-bit row offsets: the host cuts larger maps into row ranges).
 * y: H2K32 planes [M][C] (lvae_dwconv_ln_h2); w1: H2K32 [hid][C]; w2: H2K32 [C][hid] (lvae.models.base.pack_f16x2_k32); res / out: fp32
 * [M][C] (may alias).  Every output bit equals the two lvae_gemm_f32 launches (prec 4, a_h2 / out_h2, ksplit = 1) it replaces. */
typedef struct {
    const void* y; const void* w1; const float* b1; const void* w2; const float* b2; const float* gamma;
    const float* res; float* out;
    int M, C, hid;
} lvae_mlp_desc;
int lvae_mlp_h2f(const lvae_mlp_desc* d, void* stream);

/* The MLP of a ConvNeXt block on the SMALL maps (stride 32 / 64: both GEMMs run split-K there), csrc/mlp_sk.hip (round 6):
 * out = res + gamma * (fc2(gelu(fc1(y) + b1)) + b2) with fc1's K = C in S1 slices and fc2's K = hid in S2 >= 2 slices, as TWO launches
 * instead of three or four -- workgroup (32 rows, slice c) computes the hid / S2 hidden columns of fc2's slice c itself (fc1's S1
 * slices folded in order), keeps them in LDS and writes fc2's partial sums to plane c of `ws` (S2 planes of M x C floats); the
 * split-K reduce launch then finishes.  Every output bit equals the lvae_gemm_f32 launches it replaces (prec 4, a_h2 / out_h2,
 * ksplit = S1 for fc1 and S2 for fc2: reference lvae/models/common.py:154-158 computes the same MLP in fp32).  y / w1 / w2 in H2K32
 * ([M][C], [hid][C], [C][hid]); res and out may alias.  Shapes: lvae_mlp_sk_supported(C, hid, S1, S2) != 0. */
typedef struct {
    const void* y; const void* w1; const float* b1; const void* w2; const float* b2; const float* gamma;
    const float* res; float* out; float* ws;
    int M, C, hid, S1, S2;
} lvae_mlp_sk_desc;
int lvae_mlp_sk(const lvae_mlp_sk_desc* d, void* stream);
int lvae_mlp_sk_supported(int C, int hid, int S1, int S2);
int lvae_gemm_num_configs(void);      /* number of selectable tile configurations */

/* Native replay of a recorded launch-plan segment (csrc/plan_runtime.cpp; lvae/engine.py: Plan.run): ONE foreign call instead of one
 * per launch.  Every entry names an entry point of this header (`kind`) and carries its arguments by class in call order: pointers in
 * p[], integers (int / long) in i[], floats in f[]; the stream argument comes from the call (`side` != 0: the side stream).  That rule
 * is all there is: the library walks the entry point's prototype above / below, left to right, and takes each parameter from the next
 * slot of its class, cast to the parameter's type (csrc/plan_ops.h) -- no per-kind argument layout exists beside the prototypes.
 * LVAE_OP_ORDER: p[0] = event, i[0] != 0: side stream waits for main (fork), else main waits for side (join).
 * Returns 0, or the first failing launch's code with its index in *failed_index (may be NULL). */
enum {
    LVAE_OP_GEMM = 1, LVAE_OP_DWCONV_LN_F32, LVAE_OP_DWCONV_LN_H2, LVAE_OP_DWCONV_LN_BF16, LVAE_OP_DWCONV_LN_Q8, LVAE_OP_STEM_F32, LVAE_OP_STEM_BF16,
    LVAE_OP_BIAS_EXPAND_F32, LVAE_OP_BIAS_EXPAND_BF16, LVAE_OP_PRIOR_INDEX, LVAE_OP_QUANTIZE, LVAE_OP_DEQUANTIZE, LVAE_OP_GAUSSIAN_NLL,
    LVAE_OP_LOSSLESS_PARAMS, LVAE_OP_LOSSLESS_OUTPUT, LVAE_OP_MLP_H2F, LVAE_OP_MLP_SK, LVAE_OP_PRIOR_INDEX_SK, LVAE_OP_QUANTIZE_SK,
    LVAE_OP_GAUSSIAN_NLL_CHAN, LVAE_OP_RD_IMAGE, LVAE_OP_PIXEL_NLL,
    LVAE_OP_DWCONV_LN_F32_V, LVAE_OP_DWCONV_LN_H2_V, LVAE_OP_DWCONV_LN_BF16_V, LVAE_OP_DWCONV_LN_Q8_V, LVAE_OP_ORDER
};
typedef struct { int kind; int side; void* p[8]; long i[6]; double f[2]; } lvae_op;
#define LVAE_TRACE_MAGIC 1985229328.0      /* lvae_decode_blocks: seconds[1] of a timeline request */
int lvae_run_ops(const lvae_op* ops, int n, void* stream, void* side_stream, int* failed_index);

/* One pipeline group's DECODE as a single foreign call (replaces the per-latent-block Python loop around the reference's
 * `block.decompress` calls, qarv/model.py:531-557; qresvae/model.py:446-454): for every latent block, in order --
 *   launch its plan segment (up to its prior / index kernel) -> copy its scale indexes to pinned host memory -> wait for the stream ->
 *   rANS-decode the block's n_images streams (lvae_rans_decode_batch) into pinned host memory -> copy the symbols to the device --
 * then launch the tail segment (no wait: the caller synchronises).  `strings` / `string_len` are block-major: entry b * n_images + i is
 * image i's stream of block b.  Index / symbol buffers hold n_images * per_image entries per block, image after image.
 * `status_dev` / `status_host` (optional; status_host = one pinned int): the plan's status word (LVAE_STATUS_*) is copied ONCE, behind the
 * tail (the per-block chain is latency-bound and carries no extra copy: scale indexes are valid table rows whatever the prior parameters
 * were, so the coder cannot be hurt by them).  The CALLER reads *status_host after its own synchronisation and before it hands the
 * reconstruction on: non-zero = non-finite prior parameters / reconstruction -- an fp16 overflow of the default arithmetic, or a stream
 * written under another arithmetic.  A stream that fails to decode (-74) is reported as -75 (EOVERFLOW) when the word is set at that
 * point (garbage indexes, not a corrupt stream).  The caller zeroes the device word again.
 * Returns 0, a launch error (failed_block = block, failed_op = index in its segment; block n_blocks = the tail), -75 (above), or -74
 * (EBADMSG) when a stream is corrupt / truncated (failed_block = its block).  seconds[0] / [1] (optional: an array of TWO doubles or more,
 * output) receive the time spent waiting for the GPU segments and inside the coder.  Timeline (measurement; IN/out): with BOTH
 * seconds[0] = -(capacity of the array in doubles, 8 ... 4096) and seconds[1] = LVAE_TRACE_MAGIC on entry -- an uninitialised output array
 * never is -- absolute steady-clock stamps (s) follow the two totals, clamped to that capacity: per block b, seconds[2 + 4 b ..] = segment launch begins / segment + index copy issued /
 * indexes on the host / block decoded and its symbols on their way to the device; seconds[2 + 4 n_blocks] = tail issued. */
typedef struct {
    const lvae_op* ops; int n_ops;
    const uint8_t* idx_dev; uint8_t* idx_host;        /* n_images * per_image bytes.  idx_dev = NULL: the segment's prior-index launch was recorded
                                                         with idx_host (pinned, device-mapped host memory) as its output -- no copy is issued */
    int32_t* sym_host; int32_t* sym_dev;              /* n_images * per_image int32.  sym_dev = NULL: the NEXT segment's dequantize launch reads
                                                         sym_host itself (written by the coder before that segment is issued) -- no copy */
    size_t per_image;
} lvae_dec_block;
int lvae_decode_blocks(const lvae_dec_block* blocks, int n_blocks, int n_images, const uint8_t* const* strings, const size_t* string_len,
                       const int32_t* qcdf, int row_stride, const int32_t* cdf_len, const int32_t* offset,
                       const lvae_op* tail_ops, int n_tail, const int* status_dev, int* status_host, void* stream, void* side_stream,
                       int n_threads, int* failed_block, int* failed_op, double* seconds);

/* One pipeline group's ENCODE as a single foreign call (the loop around `block.compress`, qarv/model.py:516-529): launch every block's
 * segment (through its quantize kernel), each followed by the copies of its symbols / scale indexes to pinned host memory and an event;
 * then, block by block, wait for its event and rANS-encode its n_images streams (lvae_rans_encode_batch) into out[b * n_images + i]
 * (capacity out_cap[b * n_images + i]), while the GPU computes the later blocks.  out_len[b * n_images + i] receives the byte count.
 * `status_dev` / `status_host` (optional; status_host = one pinned int): the plan's status word (LVAE_STATUS_*), copied ONCE behind the last
 * block's segment and checked before that block is coded: LVAE_STATUS_RANGE set returns -34 (ERANGE: the reference's input assert), any
 * other bit -75 (EOVERFLOW: non-finite prior parameters / posterior means -- an fp16 overflow of the default arithmetic), with
 * failed_block = n_blocks - 1; the strings of the earlier blocks are to be discarded (the coder accepts any int32 symbol, and every scale
 * index is a valid table row, so coding them was harmless).  The caller zeroes the device word again.  Events are created and destroyed
 * inside the call. */
typedef struct {
    const lvae_op* ops; int n_ops;
    const int32_t* sym_dev; int32_t* sym_host;        /* sym_dev / idx_dev = NULL: the segment's quantize / prior-index launches wrote the pinned */
    const uint8_t* idx_dev; uint8_t* idx_host;        /* host arrays themselves (as lvae_dec_block) -- no copies, the event follows the segment  */
    size_t per_image;
} lvae_enc_block;
int lvae_encode_blocks(const lvae_enc_block* blocks, int n_blocks, int n_images, uint8_t* const* out, const size_t* out_cap, long* out_len,
                       const int32_t* qcdf, int row_stride, const int32_t* cdf_len, const int32_t* offset,
                       const int* status_dev, int* status_host, void* stream, void* side_stream, int n_threads,
                       int* failed_block, int* failed_op, double* seconds);

/* Depthwise kxk conv (+bias) -> LayerNorm over C (eps 1e-6, biased variance, no affine) -> AdaLN
 * y*(1+scale)+shift, one pass over an NHWC map (common.py:145-152).  wt is [k*k][C] (tap-major), `ln_w`/`ln_b`
 * (optional, may be NULL) are the LayerNorm affine of qres34m's MyConvNeXtBlock (qresvae/model.py:168-182);
 * `shift`/`scale1p` (optional) are the per-lambda AdaLN vectors with scale1p = 1+scale.
 * Supported: k in {1,3,5,7}; C in {128,144,192,256,288,384,512}.  Returns -22 for unsupported shapes.
 * The bits of an output pixel depend on (C, k, which affines are given) only -- not on B, H, W or the launch geometry:
 * C in {128,192,256,384,512} with at most one affine runs csrc/dwconv_cl.hip, everything else the sliding-window kernel. */
int lvae_dwconv_ln_f32(const float* x, const float* wt, const float* bias, const float* ln_w, const float* ln_b,
                       const float* shift, const float* scale1p, float* y,
                       int B, int H, int W, int C, int k, void* stream);

/* The same operator with the result stored PRE-SPLIT for the f16x2 GEMM that consumes it (lvae_gemm_desc.a_h2): y is an H2K32 buffer
 * [B*H*W][C/32][2][32] fp16 (B*H*W*C*4 bytes, like the fp32 map); value = split of exactly the fp32 result lvae_dwconv_ln_f32 gives.
 * C in {128,192,256,384,512}, k in {1,3,5,7}, at most one affine (the csrc/dwconv_cl.hip instances); -22 otherwise. */
int lvae_dwconv_ln_h2(const float* x, const float* wt, const float* bias, const float* ln_w, const float* ln_b,
                      const float* shift, const float* scale1p, void* y,
                      int B, int H, int W, int C, int k, void* stream);

/* Reduced-precision mode: bf16 map in, result quantised to MX-fp8 (format Q8 of lvae_gemm_desc: [B*H*W][C] e4m3 bytes, then
 * [C/64][B*H*W][2] E8M0 scales) for the GEMM that consumes it (prec 3, a_h2 = 1).  Same shape rule as lvae_dwconv_ln_h2. */
int lvae_dwconv_ln_q8(const void* x, const float* wt, const float* bias, const float* ln_w, const float* ln_b,
                      const float* shift, const float* scale1p, void* y,
                      int B, int H, int W, int C, int k, void* stream);

/* bf16-storage forms of the reduced-precision mode (BASELINE config 5; prec 3 of lvae_gemm_f32): x / y / out are bf16 bit patterns
 * (NHWC, 2-byte elements), arithmetic in fp32 registers, parameters fp32.  Same semantics as the _f32 entry points otherwise. */
int lvae_dwconv_ln_bf16(const void* x, const float* wt, const float* bias, const float* ln_w, const float* ln_b,
                        const float* shift, const float* scale1p, void* y,
                        int B, int H, int W, int C, int k, void* stream);

/* Per-image AdaLN vectors (a batch whose images are coded at different lambdas): the four forms above with an element stride between
 * consecutive images' vectors -- image b is modulated by shift[b * vstride + c] and scale1p[b * vstride + c] (vstride >= 0; 0 = one
 * pair for the batch).  No LayerNorm affine.  Image b's output is, bit for bit, what the form without the stride gives for that image
 * alone with that image's vectors.  C in {128,192,256,384,512}, k in {1,3,5,7} (the csrc/dwconv_cl.hip instances); -22 otherwise --
 * also for _f32_v / _bf16_v, whose shapes outside that set would run another kernel family. */
int lvae_dwconv_ln_f32_v(const float* x, const float* wt, const float* bias, const float* shift, const float* scale1p, float* y,
                         int B, int H, int W, int C, int k, long vstride, void* stream);
int lvae_dwconv_ln_h2_v(const float* x, const float* wt, const float* bias, const float* shift, const float* scale1p, void* y,
                        int B, int H, int W, int C, int k, long vstride, void* stream);
int lvae_dwconv_ln_bf16_v(const void* x, const float* wt, const float* bias, const float* shift, const float* scale1p, void* y,
                          int B, int H, int W, int C, int k, long vstride, void* stream);
int lvae_dwconv_ln_q8_v(const void* x, const float* wt, const float* bias, const float* shift, const float* scale1p, void* y,
                        int B, int H, int W, int C, int k, long vstride, void* stream);

/* Which kernel a lvae_dwconv_ln_<fmt>[_v] call with these arguments would launch.  Host arithmetic only, no HIP call.
 * fmt: 0 f32, 1 bf16, 2 h2, 3 q8.  affines: 0 none, 1 LayerNorm affine or AdaLN (one of them), 2 both.
 * *family: 0 = csrc/dwconv_cl.hip, 1 = sliding window (pointwise.hip).  *tile_rows: TH.  *tiles_per_wg: tpw (1 for family 1).
 * Returns 0, or -22 exactly where the launch would return -22 for its (fmt, C, k, affines, sizes).  The launchers switch on the
 * same function (csrc/dwconv_choice.h), so this is what they run; the outputs may be NULL. */
int lvae_dwconv_ln_choice(int fmt, int affines, int per_image_vectors, int B, int H, int W, int C, int k,
                          int* family, int* tile_rows, int* tiles_per_wg);

/* Which kernel instance lvae_gemm_f32 would launch for a prec 4 (f16x2) descriptor on a device of cu_count compute units, and how its
 * split-K slices are reduced.  Host arithmetic only, no HIP call.  Reads the shape and mode fields of *d and the PRESENCE of A1, ws,
 * cnt, res and gamma; never A0, Wt, Wt16, out, bias or status (they may be unset).
 * *kernel: 1 gemm_h2_kernel, 2 gemm_h2n_kernel, 3 gemm_h2p_kernel.  params[5]: the instance's template arguments -- kernel 1: {TN,
 * AGELU, AMODE}; 2: {NB, AMODE}; 3: {WM, TN, NBUF, FOLD, NLOAD}; unused slots 0.  *splitk: 0 none, 1 serial (inside gemm_h2n / the FOLD
 * form of gemm_h2p), 2 parallel with in-kernel counters, 3 parallel + reduce launch, 4 parallel, reduction left to the consumer.
 * Returns 0, or -22 for d == NULL, d->prec != 4, cu_count <= 0 and exactly where lvae_gemm_f32 returns -22 for these fields.  The
 * launch path switches on the same function (csrc/gemm_h2_choice.h), so this is what it runs; the outputs may be NULL. */
int lvae_gemm_h2_choice(const lvae_gemm_desc* d, int cu_count, int* kernel, int* params /* 5 ints */, int* splitk);

int lvae_stem_bf16(const float* im, const float* wt, const float* bias, void* out,
                   int B, int H, int W, int Cout, float im_shift, float im_scale, int* range_flag, void* stream);
int lvae_bias_expand_bf16(const float* bias, void* out, long M, int C, void* stream);

/* Stem: NCHW image [B][3][H][W] in [0,1] -> (im+shift)*scale (qarv/model.py:221) -> conv 4x4/stride 4
 * (zoo.py:37) -> NHWC [B][H/4][W/4][Cout].  wt is [48][Cout] with k = (ci*4+i)*4+j. Cout <= 256, multiple of 64. */
int lvae_stem_f32(const float* im, const float* wt, const float* bias, float* out,
                  int B, int H, int W, int Cout, float im_shift, float im_scale, int* range_flag, void* stream);
/* range_flag (device int, may be NULL): bit 0 is OR-ed in when any input value lies outside [0, 1] or is NaN -- the reference's
 * `assert 0 <= im.min() <= im.max() <= 1` (qarv/model.py:219-220, qresvae/model.py:492) without its device sync: the caller zeroes
 * the flag once and reads it at a synchronisation point it already has.  lvae_range_flag_f32 is the same check as a stand-alone
 * pass over n floats (n % 4 == 0) for encoders whose first layer is not this stem (qres17m). */
int lvae_range_flag_f32(const float* x, long n, float lo, float hi, int* flag, void* stream);

/* y[n] = (gelu_out? gelu : id)( sum_k Wt[n][k] * (gelu_in? gelu(x[k]) : x[k]) + b[n] ) -- the lambda-embedding
 * MLP (qarv/model.py:206-210) and all AdaLN `embedding_layer`s (common.py:123-127) as one concatenated GEMV. */
int lvae_gemv_f32(const float* Wt, const float* b, const float* x, float* y, int N, int K,
                  int gelu_in, int gelu_out, void* stream);
/* The same for nvec input vectors: x is [nvec][K], y is [nvec][N] (dense rows).  Every weight row is read from memory once and
 * applied to all nvec inputs (K <= 1024: the row is held in registers; a longer row is re-fetched once per 8 inputs); row i of y
 * equals lvae_gemv_f32 on row i of x bit for bit (same product order, reduction, bias, GELU). */
int lvae_gemv_batch_f32(const float* Wt, const float* b, const float* x, float* y, int N, int K, int nvec,
                        int gelu_in, int gelu_out, void* stream);

/* Prior epilogue (qarv/model.py:51-53 + GaussianConditional.build_indexes, :106,112): prm is the `prior` conv
 * output [M][2z] (NHWC rows; first z = mean, last z = log-scale).  Writes pm [M][z] and, per image b, the scale
 * index of every latent element in the coder's NCHW raster order idx[b][c][h][w] (uint8 0..n_scales-1):
 *   pv = exp(softplus(x+2.3)-2.3); s = max(pv, bound); idx = #{i < n_scales-1 : table[i] < s}. */
int lvae_prior_index_f32(const float* prm, float* pm, uint8_t* idx, const float* scale_table, int n_scales,
                         float scale_bound, int B, int HW, int z, int* status, void* stream);
/* status (optional): LVAE_STATUS_NONFINITE_PRIOR is OR-ed in when a mean or log-scale parameter is NaN / inf (see "status word"). */
/* The same behind a split-K `prior` GEMM whose reduce pass was deferred (lvae_gemm_desc.defer_reduce): prm[m][c] = ((ws[0] + ws[1]) + ...
 * + ws[S-1])[m][c] + bias[c] -- planes of [B*HW][2z] floats, summed in slice order like splitk_reduce does -- is written (other consumers
 * read it: lvae_gaussian_nll_f32, lvae_prior_sample_f32) and indexed in ONE launch. */
int lvae_prior_index_sk_f32(const float* ws, int S, const float* bias, float* prm, float* pm, uint8_t* idx, const float* scale_table,
                            int n_scales, float scale_bound, int B, int HW, int z, int* status, void* stream);

/* GaussianConditional.quantize (qarv/model.py:107-108): sym = int32(rint_half_even(qm - pm)) in NCHW raster order
 * per image, zhat = float(sym) + pm in NHWC (row stride ldz, see below). */
int lvae_quantize_f32(const float* qm, const float* pm, int32_t* sym, float* zhat, int B, int HW, int z, int ldz,
                      int* status, void* stream);
/* The same behind a split-K `posterior` GEMM whose reduce pass was deferred: qm[m][c] = ((ws[0] + ws[1]) + ... + ws[S-1])[m][c] + bias[c]
 * (planes of [B*HW][z] floats, slice order) is written and quantised in ONE launch. */
int lvae_quantize_sk_f32(const float* ws, int S, const float* bias, float* qm, const float* pm, int32_t* sym, float* zhat, int B, int HW,
                         int z, int ldz, int* status, void* stream);
/* status (optional): LVAE_STATUS_NONFINITE_LATENT is OR-ed in when qm - pm is NaN / inf or |rint(qm - pm)| >= 2^31. */
/* GaussianConditional.dequantize (qarv/model.py:113): zhat = float(sym) + pm; sym in NCHW raster order.
 * In both, zhat rows have stride ldz >= z floats; columns [z, ldz) are written as zeros (lets a following 3x3 conv
 * consume a channel count rounded up to a multiple of 4: qres34m z = 14, 10). */
int lvae_dequantize_f32(const int32_t* sym, const float* pm, float* zhat, int B, int HW, int z, int ldz, void* stream);

/* Sampling branch of a latent block (qarv/model.py:98-100, mode='sampling' with latent=None; conditional_sample /
 * unconditional_sample :365-404): z = pm + pv * N(0,1) * t + U(-0.5, 0.5) * t, with pm / pv derived from the prior conv output
 * `prm` exactly as in lvae_prior_index_f32 (pv = exp(softplus(lv + 2.3) - 2.3), NOT lower-bounded).  Device RNG: Philox4x32-10
 * keyed by `seed`, one counter per element (`offset` + element index), Box-Muller for the normal -- reproducible for a given
 * (seed, offset) whatever the launch geometry; t = 0 gives z = pm exactly.  z rows have stride ldz >= zdim (pad written as 0). */
int lvae_prior_sample_f32(const float* prm, float* z, long M, int zdim, int ldz, float t, unsigned long long seed,
                          unsigned long long offset, void* stream);

/* The sampler of one QRes-VAE latent block (qresvae/model.py QLatentBlockX.forward_uncond: cond_sample / uncond_sample / inpaint).
 * Writes z rows [B*h*w][ldz] (pad columns [zdim, ldz) = 0).  Inside the box rows [r0, r1) x columns [c0, c1) of the h x w map -- and
 * everywhere when lat == NULL -- an element is drawn exactly as lvae_prior_sample_f32 draws it (same arithmetic, counter offset +
 * m*zdim + c): a full box equals lvae_prior_sample_f32 bit for bit.  Outside the box the given latent lat, NCHW (B, zdim, h, w), is
 * copied verbatim: an empty box (r0 == r1) is its NHWC transpose. */
int lvae_latent_sample_box_f32(const float* prm, const float* lat, float* z, int B, int h, int w, int zdim, int ldz, int r0, int r1,
                               int c0, int c1, float t, unsigned long long seed, unsigned long long offset, void* stream);

/* GaussianNLLOutputNet.sample (qresvae/model.py:44-57, continuous mode) + process_output of qres34m_lossless: raw as for
 * lvae_lossless_params_f32 ([B*H*W][6], mean c0..2 | log-scale c0..2); for every (b, c, y, x) of the NCHW output, counter offset + its
 * raster index: out = clamp(mean + (exp(ls)*t)*N(0,1), -1, 1)*0.5 + 0.5 (Philox4x32-10 variates of lvae_prior_sample_f32).  t = 0 gives
 * clamp(mean)*0.5 + 0.5 exactly.  status (optional): LVAE_STATUS_NONFINITE_IMAGE when a sample is NaN / inf before the clamp. */
int lvae_pixel_sample_f32(const float* raw, float* out, int B, int H, int W, float t, unsigned long long seed, unsigned long long offset,
                          int* status, void* stream);

/* GaussianNLLOutputNet coding parameters of qres34m_lossless (qresvae/model.py:69-94).  raw = the fused conv_mean | conv_scale
 * output after PixelShuffle, NHWC [B*H*W][6] (mean c0..2, log-scale c0..2), H x W = image size.  For every (b, c, y, x) in the
 * coder's NCHW raster order, with bin = 1/127.5 and the reference's fp32 operation order:
 *   pm  = (rint(m*127.5 + 127.5)/127.5 - 1) / bin          ("workaround to make sure lossless", :72)
 *   s   = exp(ls - ln(bin));  idx = #{i < n_scales-1 : table[i] < max(s, bound)}          (build_indexes)
 *   sym = rint(((im - 0.5)*2)/bin - pm)        only when im != NULL (encoder); im is (B,3,H,W) in [0,1]. */
int lvae_lossless_params_f32(const float* raw, const float* im, float* pm, uint8_t* idx, int32_t* sym, const float* table,
                             int n_scales, float bound, int B, int H, int W, int* status, void* stream);
/* status (optional): LVAE_STATUS_NONFINITE_PRIOR when a mean / log-scale parameter is NaN / inf. */

/* ... and its decoder side (:86-94 + process_output :496-504): out = clamp((sym + pm)*bin, -1, 1)*0.5 + 0.5, NCHW. */
int lvae_lossless_output_f32(const int32_t* sym, const float* pm, float* out, long n, int* status, void* stream);
/* status (optional): LVAE_STATUS_NONFINITE_IMAGE when sym + pm is NaN / inf (the clamp would hide it). */

/* Eval-mode rate estimate of one latent block (qarv/model.py:95-96 = CompressAI GaussianConditional.forward in eval mode):
 * out_nats[b] += sum over the block's elements of -ln max(P, 1e-9), P = Phi((.5-|sym|)/s) - Phi((-.5-|sym|)/s) in fp32 with
 * s from the prior conv output `prm` as in lvae_prior_index_f32; cdf_form 0 = erf (QARV), 1 = erfc (QRes).  sym is in the
 * coder's NCHW raster order; out_nats (double[B]) must be zeroed by the caller. */
int lvae_gaussian_nll_f32(const float* prm, const int32_t* sym, double* out_nats, float scale_bound, int B, int HW, int z,
                          int cdf_form, void* stream);

/* The per-element terms of lvae_gaussian_nll_f32 (same arithmetic), stored instead of summed: out[(b*z + c)*HW + p] = -ln max(P, 1e-9)
 * as float, NCHW -- the `kl` map of the reference's forward_get_latents (qresvae/model.py:257-282 in eval mode). */
int lvae_gaussian_nll_map_f32(const float* prm, const int32_t* sym, float* out, float scale_bound, int B, int HW, int z, int cdf_form,
                              void* stream);

/* ---- eval-mode statistics of model.forward (ABI 26).  Deterministic: no float atomics, every sum in a fixed order (fp64 per thread,
 * fixed xor tree per wave, waves in order), so two calls on the same input return the same bits.  Each output is overwritten.
 * The two image entry points split each image into LVAE_EVAL_CHUNKS pixel ranges fixed by H*W alone (one workgroup each, all images at
 * once), write per-chunk fp64 partials to the caller's `ws` (double[B][LVAE_EVAL_CHUNKS][2], scratch) and add them in chunk order in a
 * second launch. */
#define LVAE_EVAL_CHUNKS 256

/* Per-channel latent rate: out[b*z + c] = sum over the h*w map of -ln max(P, 1e-9), each term the float lvae_gaussian_nll_map_f32 stores
 * (same arithmetic), added in fp64.  prm NHWC [B*HW][2z] as for lvae_gaussian_nll_f32, sym NCHW (the coder's raster order).  The sum over
 * c is the image's rate in nats; the per-channel values are the reference's `_stats_log['*_channels']` before the bits conversion. */
int lvae_gaussian_nll_chan_f32(const float* prm, const int32_t* sym, double* out, float scale_bound, int B, int HW, int z, int cdf_form,
                               void* stream);

/* Lossy reconstruction and distortion.  raw = the decoder's final conv output BEFORE the clamp, NHWC [B*H*W][3]; im NCHW in [0, 1].
 * im_hat (NCHW) = fminf(fmaxf(v, -1), 1)*0.5f + 0.5f -- the expression of the ST_IMAGE store, so it equals the codec's output bit for
 * bit.  sums[2b] = sum (v - (im - 0.5)*2)^2 (the reference's unclamped mse_loss(x_hat, x_target)), sums[2b + 1] = sum (im_hat - im)^2
 * (for PSNR).  status (optional): LVAE_STATUS_NONFINITE_IMAGE when a v is NaN / inf. */
int lvae_rd_image_f32(const float* raw, const float* im, float* im_hat, double* sums, double* ws, int B, int H, int W, int* status,
                      void* stream);

/* Lossless pixel likelihood: GaussianNLLOutputNet.forward_loss (qresvae/model.py:24-38) with gaussian_log_prob_mass (entropy_coding.py:
 * 18-49) in fp32: logscale = softplus(l + 16) - 16, s = exp(logscale), bin 1/127.5, x = (im - 0.5)*2, P = Phi((x + bin/2 - m)/s) -
 * Phi((x - bin/2 - m)/s); log P = log(max(P, 1e-8)) where P > 1e-6, else the Gaussian log-density + log(bin).  The mean m is NOT rounded.
 * raw6 as for lvae_lossless_params_f32 ([B*H*W][6], mean c0..2 | log-scale c0..2).  im_hat = clamp(m, -1, 1)*0.5 + 0.5 (NCHW);
 * sums[2b] = sum -log P, sums[2b + 1] = sum (im_hat - im)^2.  status (optional): LVAE_STATUS_NONFINITE_IMAGE for a NaN / inf mean or term. */
int lvae_pixel_nll_f32(const float* raw6, const float* im, float* im_hat, double* sums, double* ws, int B, int H, int W, int* status,
                       void* stream);

/* y = gelu_erf(x) elementwise: the exact-erf GELU used by every fused epilogue, exposed for numerics tests. */
int lvae_gelu_f32(const float* x, float* y, long n, void* stream);

/* Broadcast a [C] vector to all M rows (get_bias, qarv/model.py:289-292). */
int lvae_bias_expand_f32(const float* bias, float* out, long M, int C, void* stream);

/* sum over all elements of (a-b)^2 per image into out[b] (double), for PSNR (lvae/evaluation.py:47-49);
 * out must be zeroed by the caller. */
int lvae_sqerr_sum_f32(const float* a, const float* b, double* out, int B, long n_per_image, void* stream);
/* Deterministic form for ONE image pair of n floats: block i of n_partials writes partials[i] = its share of sum((a-b)^2) in fp64
 * (fixed element -> thread map, no atomics); the caller adds the partials in index order.  Run-to-run and process-to-process
 * identical, which the sharded evaluation needs to reproduce the single-process means bit for bit. */
int lvae_sqerr_partials_f32(const float* a, const float* b, double* partials, int n_partials, long n, void* stream);

/* ---- MS-SSIM (Wang, Simoncelli, Bovik 2003) of B image pairs in one call: data range 1, K1 = 0.01, K2 = 0.03, 11-tap Gaussian window
 * (sigma 1.5, sum 1) as a valid correlation, 5 scales weighted (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), 2x2 mean pool between scales
 * with zero padding of size % 2 in front of that axis (the zeros counted), per channel prod_s relu(cs_s)^w_s (ssim_4 at the last scale),
 * mean over channels.
 * x, y: fp32 NCHW planes with unit column stride; element (b, c, r, q) of x at x[b*x_img + c*x_plane + r*x_row + q] (strides in
 * elements, likewise y).  hw: HOST array int[B][2], the valid extent (h_b, w_b) of image b inside its planes -- images of one call may
 * differ in size (crops of one padded batch); nothing outside an extent is read.  Hmax / Wmax: at least every h_b / w_b.
 * out[b] (device, double): the value of image b.  scale_means (device, double[B][5][C]): the cs-map mean of scales 0..3 and the
 * ssim-map mean of scale 4 of every channel, before the relu.  ws: device scratch of at least lvae_msssim_workspace_bytes(B, C, Hmax,
 * Wmax) bytes, 8-byte aligned; ws_bytes its size.
 * Fixed launch sequence on `stream`, whatever B: one small host-to-device copy of hw, 5 scale launches (each also writes the next
 * scale's planes), 1 finishing launch.  Windowed moments, maps and sums are fp64; no atomics, every sum in a fixed order that depends
 * on the image's own extent alone, so a value neither depends on scheduling nor on what else is in the batch.
 * -22 before any HIP call: a null pointer, B <= 0, C <= 0, min(h_b, w_b) <= 160 (the fifth scale would have no valid pixel), an extent
 * beyond Hmax / Wmax or beyond what the strides hold, ws_bytes too small. */
int lvae_msssim_f32(const float* x, long x_img, long x_plane, long x_row, const float* y, long y_img, long y_plane, long y_row,
                    const int* hw, int B, int C, int Hmax, int Wmax, double* out, double* scale_means, void* ws, size_t ws_bytes,
                    void* stream);
/* Bytes of scratch lvae_msssim_f32 needs for these arguments; 0 when they are not acceptable (B, C <= 0, Hmax or Wmax <= 160). */
size_t lvae_msssim_workspace_bytes(int B, int C, int Hmax, int Wmax);

/* ---- SSIM / MS-SSIM of n PLANE pairs in one call (the same kernels behind another sample loader): every pair is an image of one
 * channel with its own size, so the Y, U and V planes of video frames -- of different sizes -- go in one call, read where they lie.
 * x, y, x_row, y_row, hw, pixstride: HOST arrays of n entries (hw: int[n][2] = (h_k, w_k)), read before the call returns: pair k is the
 * planes at the DEVICE addresses x[k], y[k], rows x_row[k] / y_row[k] SAMPLES apart, pixel q of a row at sample q * pixstride[k]
 * (1, or 2 for one half of an interleaved chroma plane: the UV plane of NV12 / P010 read at the address of its first U or V sample).
 * kind, for the whole call: LVAE_SAMPLE_F32 (floats; depth is not read), LVAE_SAMPLE_U8 (bytes; depth 8), LVAE_SAMPLE_U16_LOW (16-bit words,
 * the code in the low bits: word & (2^depth - 1), as lvae_image_yuv_to_f32 reads them), LVAE_SAMPLE_U16_HIGH (the code in the high bits:
 * word >> (16 - depth), the P010 family).  depth: 8, 10 or 12.
 * data_range: L > 0 in the units of the samples (1 for floats in [0, 1], 2^depth - 1 for codes); C1 = (0.01 L)^2, C2 = (0.03 L)^2.  The
 * samples are NOT divided by L: the arithmetic is lvae_msssim_f32's on the codes (exact as floats), fp64 moments and sums.
 * scales: 5 = MS-SSIM as above, min(h_k, w_k) > 160; 1 = the mean of the SSIM map (Wang et al. 2004, the Gaussian window above) over
 * the (h - 10) x (w - 10) valid pixels, min(h_k, w_k) >= 11: one scale launch and the finishing launch.
 * out[k] (device, double): the value of pair k.  scale_means (device, double[n][scales]): as scale_means of lvae_msssim_f32; with
 * scales = 1 it repeats out.  ws: device scratch of at least lvae_msssim_planes_workspace_bytes(n, max h_k, max w_k, scales) bytes,
 * 8-byte aligned.  One small host-to-device copy (hw and the plane table), `scales` scale launches, 1 finishing launch; no atomics; a
 * value depends on its own pair alone.
 * -22 before any HIP call: a null pointer (an entry of x / y included), n <= 0, a side below the minimum, w_k * pixstride[k] beyond a
 * row stride, a pixel stride other than 1 or 2, an unknown kind, a depth other than 8, 10, 12 (other than 8 for bytes), scales other than
 * 1 or 5, data_range <= 0, above 65535 or not a number, ws_bytes too small.
 * Both entries were added without a change to lvae_abi_version(). */
enum { LVAE_SAMPLE_F32 = 0, LVAE_SAMPLE_U8 = 1, LVAE_SAMPLE_U16_LOW = 2, LVAE_SAMPLE_U16_HIGH = 3 };
int lvae_msssim_planes(const void* const* x, const long* x_row, const void* const* y, const long* y_row, const int* hw,
                       const int* pixstride, int n, int kind, int depth, double data_range, int scales, double* out, double* scale_means,
                       void* ws, size_t ws_bytes, void* stream);
/* Bytes of scratch lvae_msssim_planes needs; 0 when the arguments are not acceptable. */
size_t lvae_msssim_planes_workspace_bytes(int n, int Hmax, int Wmax, int scales);

/* ---- 8-bit images in and out of the codec (csrc/image_io.hip).  Both entries take B images whose 8-bit side is interleaved RGB
 * (HWC, 3 bytes per pixel) and whose fp32 side is NCHW planes with unit column stride, and read HOST arrays describing the 8-bit side:
 * image b at the DEVICE address u8[b], its rows u8_row[b] bytes apart (>= 3 * w_b), its valid extent hw[2b], hw[2b + 1] = (h_b, w_b) --
 * passed like the hw array of lvae_msssim_f32; the arrays are read before the call returns (they travel as kernel arguments, 16 images
 * per launch: no copy to the device, no scratch).  Base addresses and row strides may have any alignment: the 12 bytes of 4 pixels move
 * as dwords where they start on a dword boundary, as bytes where not; the fp32 side moves as 16-byte vectors where base, strides and
 * width are multiples of 4 elements, as scalars where not.  Nothing outside an extent is read (u8_to_f32) or written (f32_to_u8).
 * -22 before any HIP call: a null pointer (an entry of src / dst included), B <= 0, H or W <= 0, an extent that is 0 or beyond (H, W),
 * a row stride below 3 * w_b, image / plane / row strides that do not hold (H, W).
 * Both entries were added without a change to lvae_abi_version() (no existing signature changed): a client built against an older
 * library of the same version probes for the symbols (dlsym) before it relies on them.
 *
 * lvae_image_u8_to_f32: dst[b*dst_img + c*H*W + y*W + x] = (float)v / 255 (IEEE division: the bits of torch's .to(float32).div(255);
 * a multiplication by 1/255 differs in 126 of the 256 values), v = byte c of pixel (min(y, h_b - 1), min(x, w_b - 1)) of image b, for
 * the whole canvas (H, W): pixels right of / below the extent repeat the nearest valid one (np.pad mode='edge', the padding of
 * lvae/utils/coding.py::pad_divisible_by).  dst_img (elements, >= 3*H*W) lets the planes land in an encode plan's input buffer or in a
 * larger batch tensor; nothing between the images' planes is written. */
int lvae_image_u8_to_f32(const uint8_t* const* src, const long* src_row, const int* hw, int B, float* dst, long dst_img, int H, int W,
                         void* stream);
/* lvae_image_f32_to_u8: byte c of pixel (y, x) of image b, y < h_b, x < w_b, = rint(clamp(s, 0, 1) * 255) with
 * s = src[b*src_img + c*src_plane + y*src_row + x] (strides in elements: views of a decoder's padded batch (B, 3, H, W) are read in
 * place), the product formed in fp32, ties to even -- torch.round(x.clamp(0, 1) * 255) -- and NaN -> 0. */
int lvae_image_f32_to_u8(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B,
                         uint8_t* const* dst, const long* dst_row, void* stream);

/* ---- 8-bit YUV 4:2:0 frames in and out of the codec (csrc/yuv_io.hip, which holds all eight YUV entries: these two are its 8-bit 4:2:0
 * centre-sited kernels, planar for I420 and semi-planar for NV12, behind their own argument contract), with the conventions of the image entries above: HOST arrays
 * of DEVICE plane addresses and row strides in bytes, hw[2b], hw[2b + 1] = (h_b, w_b), all read before the call returns (16 frames per
 * launch, descriptors as kernel arguments); fp32 side NCHW RGB planes with unit column stride; any alignment (dword / 16-byte accesses
 * where the addresses allow, bytes / scalars where not).  A frame is a luma plane of (h, w) bytes and chroma at (h/2, w/2); h and w even.
 * fmt LVAE_YUV_I420: u[b], v[b] are the two chroma planes; LVAE_YUV_NV12: u[b] is the interleaved UV plane (row stride >= w) and the
 * arrays v / v_row are not read (they may be null).  matrix: LVAE_YUV_BT601 (Kr, Kb = 0.299, 0.114) / LVAE_YUV_BT709 (0.2126, 0.0722);
 * range: LVAE_YUV_LIMITED (Y 16..235, C 16..240) / LVAE_YUV_FULL (0..255).  Chroma siting is centre (JPEG / MPEG-1): a chroma sample
 * sits in the middle of its 2x2 luma block; co-sited chroma is not supported.
 * The colour parameters are the caller's: no stream or container records them.
 * -22 before any HIP call: a null pointer (an entry of a plane array included), B <= 0, H or W <= 0, an extent that is 0, odd or beyond
 * (H, W), a row stride below its plane's width in bytes, fp32 strides that do not hold (H, W), an unknown fmt / matrix / range / chroma.
 *
 * lvae_image_yuv420_to_f32: the whole canvas (H, W) of dst[b*dst_img + c*H*W + y*W + x], c = R, G, B, from the luma pixel
 * (min(y, h_b - 1), min(x, w_b - 1)) (replicate padding, as lvae_image_u8_to_f32).  Chroma at a luma pixel (y, x): chroma
 * LVAE_YUV_NEAREST: sample (y/2, x/2); LVAE_YUV_BILINEAR: per axis 3/4 of sample x/2 and 1/4 of its neighbour on the pixel's side
 * (x/2 - 1 for even x, x/2 + 1 for odd x, clamped to the plane) -- exact on bytes.  Then, every operation rounded to fp32 on its own (IEEE
 * division, no fused multiply-add): y' = (Y - 16) / 219, c = (C - 128) / 224 (limited) or Y / 255, (C - 128) / 255 (full);
 * R = y' + a*cr, B = y' + b*cb, G = (y' - d*cb) - e*cr with a = 2(1 - Kr), b = 2(1 - Kb), d = 2 Kb (1 - Kb) / Kg, e = 2 Kr (1 - Kr) / Kg as fp32
 * constants; clamped to [0, 1].  lvae/utils/yuv.py states the same expression with torch ops; the bits agree. */
enum { LVAE_YUV_I420 = 0, LVAE_YUV_NV12 = 1 };
enum { LVAE_YUV_BT601 = 0, LVAE_YUV_BT709 = 1 };
enum { LVAE_YUV_LIMITED = 0, LVAE_YUV_FULL = 1 };
enum { LVAE_YUV_NEAREST = 0, LVAE_YUV_BILINEAR = 1 };
int lvae_image_yuv420_to_f32(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, const long* y_row,
                             const long* u_row, const long* v_row, const int* hw, int B, int fmt, int matrix, int range, int chroma,
                             float* dst, long dst_img, int H, int W, void* stream);
/* lvae_image_f32_to_yuv420: the inverse, for reconstructions; src addressed as in lvae_image_f32_to_u8 (crops of a decoder's padded
 * batch are read in place).  Per pixel, in fp32 with every operation rounded on its own: r, g, b clamped to [0, 1] (NaN -> 0);
 * y' = (Kr*r + Kg*g) + Kb*b; cb = (b - y') / (2(1 - Kb)), cr = (r - y') / (2(1 - Kr)).  A chroma sample is the mean of its 2x2 block,
 * ((tl + tr) + (bl + br)) * 0.25.  Bytes: rint(y' * 219 + 16), rint(c * 224 + 128) (limited) or rint(y' * 255), rint(c * 255 + 128)
 * (full), ties to even, clamped to 0..255.  Nothing outside a plane's extent is written. */
int lvae_image_f32_to_yuv420(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B, int fmt,
                             int matrix, int range, uint8_t* const* y, uint8_t* const* u, uint8_t* const* v, const long* y_row,
                             const long* u_row, const long* v_row, void* stream);
/* lvae_sse_u8: out[k] (DEVICE, one 64-bit unsigned integer per pair) = sum over the (h_k, w_k) bytes of (a_k - b_k)^2 for n pairs of byte
 * planes (HOST arrays of DEVICE addresses, row strides in bytes >= w_k, hw as above), in integer arithmetic throughout: exact, whatever
 * the scheduling.  `out` is zeroed by the call (a memset on `stream`), then every wave adds its share with one integer atomic.
 * -22 before any HIP call: a null pointer or entry, n <= 0, a plane of 0 rows or columns, a row stride below w_k. */
int lvae_sse_u8(const uint8_t* const* a, const long* a_row, const uint8_t* const* b, const long* b_row, const int* hw, int n,
                uint64_t* out, void* stream);
/* The three entries above were added without a change to lvae_abi_version() (no existing signature changed). */

/* ---- Planar YUV frames of 8, 10 or 12 bits at 4:2:0 / 4:2:2 / 4:4:4 (csrc/yuv_io.hip): the general form of the three entries above,
 * which are instances of the same kernels; the conventions (HOST arrays of DEVICE plane addresses, hw, 16 frames per launch, fp32 side, alignment) are
 * theirs.  depth: 8, 10 or 12.  A sample is a byte at depth 8 and otherwise a 16-bit word with the value in its LOW bits (yuv420p10le,
 * yuv422p12le ...; P010-style layouts with the value in the high bits: the two entries further down); every sample read is masked to `depth` bits.
 * Row strides are in SAMPLES.  subsampling: LVAE_YUV_SUB_420: chroma planes of (h/2, w/2), h and w even; LVAE_YUV_SUB_422: (h, w/2), w even;
 * LVAE_YUV_SUB_444: (h, w), any extent.  Planar only: u[b] and v[b] are separate planes.  siting: LVAE_YUV_SITING_CENTER: a chroma sample
 * lies in the middle of the luma samples it covers (JPEG / MPEG-1); LVAE_YUV_SITING_LEFT: horizontally it lies ON the even luma column and
 * vertically it stays centred (H.264 / HEVC chroma_sample_loc_type 0); siting has no effect on an axis that is not subsampled.
 * matrix: LVAE_YUV_BT601 / LVAE_YUV_BT709 / LVAE_YUV_BT2020 (non-constant luminance, Kr, Kb = 0.2627, 0.0593; these entries only).
 * range, with s = 2^(depth - 8): LVAE_YUV_LIMITED: Y = 16 s + 219 s y', C = 128 s + 224 s c; LVAE_YUV_FULL: Y = (2^depth - 1) y',
 * C = 128 s + (2^depth - 1) c.  The colour parameters, depth and siting are the caller's: no stream or container records them.
 * -22 before any HIP call: a null pointer (an entry of a plane array included), B <= 0, H or W <= 0, an extent that is 0, odd on a subsampled
 * axis or beyond (H, W), a row stride below its plane's width, fp32 strides that do not hold (H, W), a depth other than 8, 10, 12, an
 * unknown subsampling / siting / matrix / range / chroma.
 *
 * lvae_image_yuv_to_f32: as lvae_image_yuv420_to_f32 (the whole canvas, replicate padding).  Chroma at luma pixel (y, x), per SUBSAMPLED
 * axis: LVAE_YUV_NEAREST: sample x/2; LVAE_YUV_BILINEAR, centre: 3/4 of sample x/2 and 1/4 of its neighbour on the pixel's side, clamped to
 * the plane; left (horizontal axis only): column 2k takes sample k, column 2k + 1 takes (c[k] + c[min(k + 1, cw - 1)]) / 2 -- exact on
 * integers.  Then, every operation rounded to fp32 on its own: y' = (Y - yoff) / yscale, c = (C - 128 s) / cscale, and R, G, B as in
 * lvae_image_yuv420_to_f32; at depth 8, 4:2:0, centre siting it is that entry's kernel. */
enum { LVAE_YUV_SUB_420 = 0, LVAE_YUV_SUB_422 = 1, LVAE_YUV_SUB_444 = 2 };
enum { LVAE_YUV_SITING_CENTER = 0, LVAE_YUV_SITING_LEFT = 1 };
enum { LVAE_YUV_BT2020 = 2 };
int lvae_image_yuv_to_f32(const void* const* y, const void* const* u, const void* const* v, const long* y_row, const long* u_row,
                          const long* v_row, const int* hw, int B, int depth, int subsampling, int siting, int matrix, int range, int chroma,
                          float* dst, long dst_img, int H, int W, void* stream);
/* lvae_image_f32_to_yuv: the inverse; src addressed as in lvae_image_f32_to_yuv420, y' / cb / cr per pixel as there.  Chroma samples from
 * the per-pixel fp32 cb / cr, the order of the sums as written: centre 4:2:0 ((a + b) + (c + d)) * 0.25 over the 2x2 block; centre 4:2:2
 * (a + b) * 0.5; left: per row h[k] = ((c[max(2k - 1, 0)] + c[2k + 1]) + (c[2k] + c[2k])) * 0.25, for 4:2:0 followed by (h_row0 + h_row1) * 0.5;
 * 4:4:4: the pixel's own.  Codes: rint(y' * yscale + yoff), rint(c * cscale + 128 s), ties to even, clamped to 0 .. 2^depth - 1.  Nothing
 * outside a plane's extent is written. */
int lvae_image_f32_to_yuv(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B, int depth,
                          int subsampling, int siting, int matrix, int range, void* const* y, void* const* u, void* const* v,
                          const long* y_row, const long* u_row, const long* v_row, void* stream);
/* lvae_sse_u16: lvae_sse_u8 (the same kernel template) for planes of 16-bit words (row strides in samples): exact for ANY 16-bit values
 * -- sums are 64-bit integers from the lane on, one integer atomic per wave. */
int lvae_sse_u16(const uint16_t* const* a, const long* a_row, const uint16_t* const* b, const long* b_row, const int* hw, int n,
                 uint64_t* out, void* stream);
/* These three were added without a change to lvae_abi_version() either. */

/* ---- Semi-planar frames of 10 or 12 bits at 4:2:0 / 4:2:2 (P010, P012, P210, P212: what hardware video decoders deliver; the SP variants of
 * csrc/yuv_io.hip), with the conventions of the two planar entries above.  A frame is a luma plane y[b] of (h, w) 16-bit words and ONE
 * chroma plane uv[b] of (h/2, w/2) (LVAE_YUV_SUB_420) or (h, w/2) (LVAE_YUV_SUB_422) chroma pixels, a chroma pixel being two neighbouring words,
 * U then V: a UV row of cw chroma pixels has 2 cw samples.  Row strides are in SAMPLES (uv_row >= w).  A sample's code is the HIGH `depth`
 * bits of its word: word >> (16 - depth) on input, whatever the low bits hold; code << (16 - depth) on output, low bits zero.  depth: 10 or
 * 12; siting, matrix, range, chroma: as above; w is even, and h for 4:2:0.  LVAE_YUV_LAYOUT_* names the two plane layouts for callers (the
 * sequence container of lvae/utils/yuvseq.py records one); no entry takes it.
 * The contract is bit equality with the planar path: lvae_image_yuvsp_to_f32 gives what lvae_image_yuv_to_f32 gives for the deinterleaved,
 * shifted planes (replicate padding included), and lvae_image_f32_to_yuvsp writes the interleaved, shifted codes of lvae_image_f32_to_yuv.
 * The U and V of a chroma pixel leave as one 4-byte store (two chroma pixels as one 8-byte store) where the address allows; nothing
 * outside a plane's extent is written.
 * -22 before any HIP call: as above, with a depth other than 10 / 12 or a subsampling other than 4:2:0 / 4:2:2 among the unsupported values.
 * Added without a change to lvae_abi_version(). */
enum { LVAE_YUV_LAYOUT_PLANAR = 0, LVAE_YUV_LAYOUT_SEMIPLANAR = 1 };
int lvae_image_yuvsp_to_f32(const uint16_t* const* y, const uint16_t* const* uv, const long* y_row, const long* uv_row, const int* hw, int B,
                            int depth, int subsampling, int siting, int matrix, int range, int chroma, float* dst, long dst_img, int H, int W,
                            void* stream);
int lvae_image_f32_to_yuvsp(const float* src, long src_img, long src_plane, long src_row, int H, int W, const int* hw, int B, int depth,
                            int subsampling, int siting, int matrix, int range, uint16_t* const* y, uint16_t* const* uv, const long* y_row,
                            const long* uv_row, void* stream);

/* ---- Tiled images (csrc/tile_stitch.hip; lvae/utils/tiling.py states the grid rule and the weights): a window of an (h, w) image from
 * the fp32 reconstructions of the tiles that cover it.  The tiles form a rows x cols grid of common extent (th, tw) with origins oy[rows],
 * ox[cols] (HOST arrays; they must be what the grid rule gives for (h, th, overlap) and (w, tw, overlap): origin k * (T - overlap) for
 * every tile but the last of an axis, size - T for the last, a single origin 0 when size <= T -- the tile then holds `size` valid rows /
 * columns).  tiles: HOST array of rows * cols DEVICE addresses, row-major, null for a tile that was not decoded; element (c, r, q) of a
 * tile at tile[c*tile_plane + r*tile_row + q] (strides in elements, shared by all tiles: crops of a decoder's padded batch are read
 * in place).  All three arrays are read before the call returns.
 * Pixel (y, x) of the image, per axis and covering tile (origin o, u = x - o, r = max(overlap, 1)): wl = o > 0 ? min(1, (u + 0.5) / r) : 1,
 * wr = o + T < size ? min(1, (T - u - 0.5) / r) : 1, w_axis = min(wl, wr); a tile's weight is wy * wx.  A pixel covered by one tile
 * takes its value unchanged; otherwise sum_k(w_k v_k) / sum_k(w_k) over the (at most 3 x 3) covering tiles in ascending tile number,
 * every product, sum and the division rounded to fp32 on its own.  No atomics: two calls give the same bits.
 * The window (y0, x0, hh, ww) goes to dst: out_u8 == 0: fp32 planes, dst[c*dst_plane + (y - y0)*dst_row + (x - x0)] (elements);
 * out_u8 != 0: interleaved RGB bytes, dst[(y - y0)*dst_row + 3*(x - x0) + c] = rint(clamp(v, 0, 1) * 255), ties to even, NaN -> 0
 * (the rounding of lvae_image_f32_to_u8; dst_row in bytes, dst_plane unused).  Only tiles that meet the window are read; nothing outside
 * the window is written.  Any alignment is accepted: one-tile quads move as 16-byte vectors / 3 dwords where the addresses allow it.
 * ws: device scratch of at least lvae_tile_stitch_workspace_bytes(rows, cols) bytes, 8-byte aligned.
 * Fixed sequence on `stream`, whatever the number of tiles: one small host-to-device copy (addresses and origins into ws), one launch.
 * -22 before any HIP call: a null pointer, a null entry of `tiles` for a tile that meets the window, a window that is empty or not
 * inside the image, tile strides that do not hold (th, tw), destination strides that do not hold the window, overlap outside
 * [0, T / 2] on an axis with more than one tile, origins that are not the grid rule's, ws too small or misaligned.
 * Added without a change to lvae_abi_version(), like the image entries above. */
int lvae_tile_stitch(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols,
                     int th, int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, void* dst, long dst_plane,
                     long dst_row, int out_u8, void* ws, size_t ws_bytes, void* stream);
/* Bytes of scratch lvae_tile_stitch needs; 0 when rows or cols <= 0. */
size_t lvae_tile_stitch_workspace_bytes(int rows, int cols);
/* lvae_tile_stitch_yuv (csrc/tile_stitch_yuv.hip): the window of a tiled image as the planes of a YUV frame, with no fp32 image in between.
 * The tile arguments, the grid rule, the window and the scratch (lvae_tile_stitch_workspace_bytes; one small copy and one launch) are
 * lvae_tile_stitch's; depth, subsampling, siting, matrix and range are lvae_image_f32_to_yuv's.  layout LVAE_YUV_LAYOUT_PLANAR: y, u, v
 * are the planes; LVAE_YUV_LAYOUT_SEMIPLANAR: u is the interleaved UV plane and v / v_row are not read -- at depth 8 that is NV12 (4:2:0,
 * centre siting, BT.601 / BT.709: what lvae_image_f32_to_yuv420 has), at depth 10 / 12 P010 / P012 / P210 / P212 with the code in the high
 * bits.  The destination is the WINDOW's frame: y holds (hh, ww) samples, the chroma planes (hh >> sy, ww >> sx) (the UV plane
 * (hh >> sy, ww) samples); row strides in samples, which may exceed the extent; nothing outside the window's planes is written.
 * The contract is bit equality with the composition: lvae_tile_stitch(..., out_u8 = 0) of the image into fp32 planes, then the matching
 * lvae_image_f32_to_yuv / _yuvsp / _yuv420 entry -- blends of up to 9 covering tiles, NaN -> 0 and ties to even included -- and a window is
 * the crop of the whole frame.  So with left-sited chroma the column before a window with x0 > 0 is column x0 - 1 OF THE IMAGE, blended
 * like any other pixel (not a copy of column x0), and the tiles that hold it must have been decoded.
 * -22 before any HIP call: whatever lvae_tile_stitch refuses; a null plane; y0 or hh odd at 4:2:0, x0 or ww odd at 4:2:0 / 4:2:2; an unknown
 * depth / subsampling / siting / matrix / range / layout, or a semi-planar layout the entries named above do not have; row strides that do
 * not hold the window; a null entry of `tiles` for a tile that meets the window widened, where left-sited and x0 > 0, by column x0 - 1.
 * Added without a change to lvae_abi_version(); it has no launch-plan kind. */
int lvae_tile_stitch_yuv(const float* const* tiles, long tile_plane, long tile_row, const int* oy, const int* ox, int rows, int cols, int th,
                         int tw, int overlap, int h, int w, int y0, int x0, int hh, int ww, int depth, int subsampling, int siting, int matrix,
                         int range, int layout, void* y, void* u, void* v, long y_row, long u_row, long v_row, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- Reduced-resolution coding: a separable, antialiased resampler (csrc/resample.hip; lvae/utils/resample.py states the window rule,
 * the filters and the tables, and holds the fp64 reference).  All B images of a call share the geometry (h_in, w_in) -> (h_out, w_out)
 * and one pair of DEVICE-resident tables, which the caller owns.  Per axis n_in -> n_out: start[n_out] (int32) and wgt[n_out][taps]
 * (fp32, rows zero-padded to `taps`); output i of the axis is sum_j wgt[i][j] * x[min(start[i] + j, n_in - 1)], j ascending.  start
 * must not decrease.  An axis with n_out == n_in is NOT filtered: its table pointers are null and its taps 0 (a bit copy on that
 * axis); any other axis needs 1 <= taps <= 64.  yspan: the largest number of input rows any 16 consecutive output rows read,
 * max_i(min(start[min(i + 15, h_out - 1)] + ytaps, h_in) - start[i]) (ignored when ytaps == 0): the host sizes a workgroup's tile from
 * it so that its LDS stays within 64 KiB (two or more workgroups per CU), and a geometry whose narrowest tile does not fit returns -22.
 * A resized pixel is the horizontal pass (fp32, taps ascending, one fused multiply-add per tap from 0) followed by the vertical pass
 * (the same) over the horizontally filtered rows, which stay in LDS: no intermediate image goes to memory and there are no atomics, so
 * two calls give the same bits.  One launch per 16 images (descriptors as kernel arguments, as the image entries above).
 * Whatever the tables hold, nothing outside a source or destination extent is read or written: every index is clamped to its extent
 * (a table that breaks the rules above gives wrong pixels, not a fault).  Every access is a byte or an fp32 scalar: bases and row
 * strides may have any alignment.
 * The 8-bit side is interleaved RGB (HOST arrays of DEVICE addresses and row strides in bytes, read before the call returns); an fp32
 * source is a strided NCHW view, element (b, c, y, x) at src[b*src_img + c*src_plane + y*src_row + x] (crops of a decoder's padded batch
 * are read in place); an fp32 destination is B images of 3 planes of the canvas (H, W) >= (h_out, w_out), dst_img elements apart:
 * canvas pixel (y, x) holds resized pixel (min(y, h_out - 1), min(x, w_out - 1)) (replicate padding, as lvae_image_u8_to_f32).
 * -22 before any HIP call: a null pointer (an entry of a HOST array included), B <= 0, a size <= 0, a canvas below (h_out, w_out), taps
 * outside the rules above or table pointers that do not go with them, yspan <= 0 on a filtered vertical axis, a ratio n_in / n_out
 * outside [1/8, 8], strides that do not hold their extents, a tile that does not fit.
 * Added without a change to lvae_abi_version(), like the image entries above.
 *
 * lvae_resample_u8_to_f32: source pixels are (float)v / 255 (IEEE division); the result is clamped to [0, 1].  Equal, bit for bit, to
 * lvae_resample_f32 with clamp != 0 applied to the output of lvae_image_u8_to_f32. */
int lvae_resample_u8_to_f32(const uint8_t* const* src, const long* src_row, int B, int h_in, int w_in, int h_out, int w_out,
                            const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps,
                            float* dst, long dst_img, int H, int W, void* stream);
/* lvae_resample_f32_to_u8: byte c of pixel (y, x) of image b = rint(clamp(v, 0, 1) * 255), ties to even, NaN -> 0, for y < h_out,
 * x < w_out (dst_row[b] >= 3 * w_out bytes).  Equal, bit for bit, to lvae_image_f32_to_u8 applied to the output of lvae_resample_f32. */
int lvae_resample_f32_to_u8(const float* src, long src_img, long src_plane, long src_row, int B, int h_in, int w_in, int h_out, int w_out,
                            const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps,
                            uint8_t* const* dst, const long* dst_row, void* stream);
/* lvae_resample_f32: fp32 in, fp32 out; clamp != 0 clamps the result to [0, 1] (NaN -> 0). */
int lvae_resample_f32(const float* src, long src_img, long src_plane, long src_row, int B, int h_in, int w_in, int h_out, int w_out,
                      const int* ystart, const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps,
                      int clamp, float* dst, long dst_img, int H, int W, void* stream);

/* ---- Reduced-resolution coding of YUV frames (csrc/resample_yuv.hip): the resampler above fused with the colour conversions of the YUV
 * entries, so that no full-resolution fp32 RGB image goes to memory.  All B frames of a call share one size and one kind: depth,
 * subsampling, siting, matrix, range (and chroma, on the way in) are lvae_image_yuv_to_f32's, the plane arrays, row strides (in samples) and
 * hw -- B (h, w) pairs, each of which must be the call's (h_in, w_in) on the way in, (h_out, w_out) on the way out -- too.  layout:
 * LVAE_YUV_LAYOUT_PLANAR: y, u, v are the planes; LVAE_YUV_LAYOUT_SEMIPLANAR: u is the interleaved UV plane and v / v_row are not read -- at
 * depth 8 that is NV12 (4:2:0, centre siting, BT.601 / BT.709), at depth 10 / 12 P010 / P012 / P210 / P212 with the code in the high bits.
 * The geometry and the seven table arguments are lvae_resample_f32's, with its rules.
 * The contract is bit equality with the composition of the existing entries:
 *   lvae_resample_yuv_to_f32 = the layout's lvae_image_yuv*_to_f32 into an (h_in, w_in) canvas, then lvae_resample_f32 with clamp != 0 into
 *     the canvas (H, W), replicate padding included.  A source pixel is converted once per tile and source row (into LDS), never per tap.
 *     xspan: the largest number of source columns any 8 consecutive output columns read, max_i(min(xstart[min(i + 7, w_out - 1)] + xtaps,
 *     w_in) - xstart[i]) (ignored when xtaps == 0): with yspan it sizes a workgroup's tile within the 64 KiB of LDS.
 *   lvae_resample_f32_to_yuv = lvae_resample_f32 with clamp == 0 into an (h_out, w_out) image, then the layout's lvae_image_f32_to_yuv*: the
 *     values are clamped where the codes are made (NaN -> 0), left-sited chroma reads the resized column before its own.  src is the
 *     strided NCHW view of lvae_resample_f32; nothing outside a plane's extent is written.
 * Whatever the tables, xspan and yspan hold, nothing outside an extent is read or written (wrong pixels, not a fault).  No atomics.  One
 * launch per 16 frames.
 * -22 before any HIP call: whatever lvae_resample_f32 and the YUV entry of the layout refuse; an unknown layout or one these parameters do
 * not have; a frame whose size is not the call's; xspan <= 0 on a filtered horizontal axis; a tile that does not fit.
 * Added without a change to lvae_abi_version(); they have no launch-plan kind. */
int lvae_resample_yuv_to_f32(const void* const* y, const void* const* u, const void* const* v, const long* y_row, const long* u_row,
                             const long* v_row, const int* hw, int B, int depth, int subsampling, int siting, int matrix, int range, int chroma,
                             int layout, int h_in, int w_in, int h_out, int w_out, const int* ystart, const float* ywgt, int ytaps, int yspan,
                             const int* xstart, const float* xwgt, int xtaps, int xspan, float* dst, long dst_img, int H, int W, void* stream);
int lvae_resample_f32_to_yuv(const float* src, long src_img, long src_plane, long src_row, const int* hw, int B, int depth, int subsampling,
                             int siting, int matrix, int range, int layout, int h_in, int w_in, int h_out, int w_out, const int* ystart,
                             const float* ywgt, int ytaps, int yspan, const int* xstart, const float* xwgt, int xtaps, void* const* y,
                             void* const* u, void* const* v, const long* y_row, const long* u_row, const long* v_row, void* stream);

/* ---- rate maps (csrc/rate_map.hip): where an image's estimated bits go.  Deterministic: no atomics, every sum in the order stated, each
 * fp64 operation rounded on its own (no fused multiply-add), so a torch fp64 expression of the definitions gives the same bits and two
 * calls agree.  Every output is overwritten.  Launched by the callers between the ranges of a launch plan: the entries have no
 * lvae_op kind, because the table of kinds is part of what a client sees and stays at its 26 rows with LVAE_OP_ORDER where it is (a new
 * kind in front of it would renumber it).  lvae_gaussian_nll_pos_f32 would fit an lvae_op; lvae_rate_map_f32 would not (eight integers).
 * Added without a change to lvae_abi_version() (no existing signature changed).
 *
 * lvae_gaussian_nll_pos_f32: the position-wise latent rate of one block.  out[b*HW + p] = the sum over c = 0 .. z-1, in ascending c, of
 * the float lvae_gaussian_nll_map_f32 stores at (b, c, p) -- the same arithmetic; prm NHWC [B*HW][2z], sym NCHW, cdf_form 0 erf | 1 erfc --
 * each term widened to fp64 and added to the running sum (from 0).  Nats.  The sum of out over p is the image's rate in that block. */
int lvae_gaussian_nll_pos_f32(const float* prm, const int32_t* sym, double* out, float scale_bound, int B, int HW, int z, int cdf_form,
                              void* stream);
/* lvae_pixel_nll_pos_f32: the same for the lossless model's pixel stage.  out[b*H*W + y*W + x] = the sum over the 3 channels, ascending,
 * in fp64, of the -log P terms of lvae_pixel_nll_f32 (raw6, im and status as there). */
int lvae_pixel_nll_pos_f32(const float* raw6, const float* im, double* out, int B, int H, int W, int* status, void* stream);
/* lvae_rate_map_f32: the block maps composed at image resolution, one launch for the batch.  pos / lat_h / lat_w: HOST arrays of n_blocks
 * (<= 32) entries, read before the call returns: pos[i] = DEVICE address of block i's map, double[B][lat_h[i]][lat_w[i]] (nats); block i
 * stands at stride s_i = H / lat_h[i].  pix (optional, DEVICE): double[B][H][W] (nats).  For Y < crop_h, X < crop_w:
 *   out[b*out_img + Y*out_row + X] = (float)( sum over i ascending, from 0, of (pos[i][b, Y / s_i, X / s_i] * LOG2E) * 2^(-2 log2 s_i),
 *                                             then + pix[b, Y, X] * LOG2E when pix is given ),   LOG2E = 1.4426950408889634 (fp64):
 * bits per pixel at that pixel; over an uncropped map the sum of out is the image's estimated size in bits.  Nothing outside the crop
 * is written (out_row >= crop_w; out_img is ignored for B == 1).
 * -22: a null pointer, B outside 1 .. 65535, n_blocks outside 0 .. 32 (0 only with pix), a crop outside 1 .. H x 1 .. W, strides that do
 * not hold the crop, H % lat_h[i] or W % lat_w[i] non-zero, H / lat_h[i] != W / lat_w[i], a ratio that is no power of two. */
int lvae_rate_map_f32(const double* const* pos, const int* lat_h, const int* lat_w, int n_blocks, const double* pix, int B, int H, int W,
                      float* out, long out_img, long out_row, int crop_h, int crop_w, void* stream);

/* Stream ordering for launch plans with independent branches (lvae/engine.py: Plan.fork / Plan.join): an event without timing, and
 * "work enqueued on to_stream from now on runs after the work enqueued on from_stream so far" (hipEventRecord + hipStreamWaitEvent). */
void* lvae_event_create(void);
int   lvae_event_destroy(void* event);
int   lvae_stream_order(void* from_stream, void* to_stream, void* event);

#ifdef __cplusplus
}
#endif
#endif /* LVAE_HIP_H */
