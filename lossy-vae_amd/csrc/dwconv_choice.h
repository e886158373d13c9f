// dwconv_choice.h -- which kernel a depthwise + LayerNorm launch runs: the ONE implementation of that choice.  Host arithmetic only.
// The launchers (pointwise.hip::dwln -> dwconv_cl.hip::launch_cl / pointwise.hip::launch_dwln) switch on its result, and
// lvae_dwconv_ln_choice (include/lvae_hip.h) reports it, so what a test observes is what a launch does.
// The choice depends on (k, C, bf16 map or not, which affines, B, H, W) only -- never on the output format of the channel-per-lane
// kernel, whose four translation units (dwconv_cl*.hip) therefore share this header.
#pragma once

namespace lvae_dwln {

// ---- geometry of the channel-per-lane kernel (csrc/dwconv_cl.hip) that the estimate needs: its LDS footprint
constexpr int CL_SW = 8;                    // output pixels per lane along W
constexpr int CL_TILE = 8 * 96;             // floats of a wave's transpose tile: 8 pixels x 384 B (64 channels + pad: conflict-free b128 reads)
constexpr int cl_xw(int ks) { return CL_SW + ks - 1; }                                   // input pixels per lane and row
constexpr int cl_ppi(bool bf) { return bf ? 8 : 4; }                                     // pixels per LDS-DMA instruction (64 lanes x 16 B = 64 channels x PPI pixels)
constexpr int cl_ng(int ks, bool bf) { return (cl_xw(ks) + cl_ppi(bf) - 1) / cl_ppi(bf); }   // DMA instructions per row
constexpr int cl_rowf(int ks, bool bf) { return cl_ng(ks, bf) * 256; }                   // floats of one row buffer (NG KiB)
// per wave: the LayerNorm transpose tile and two row buffers; then the waves' statistics and the affine parameters (the kernel
// static_asserts that its LDS array has this size)
constexpr int cl_lds_bytes(int ks, int nw, bool bf) { return (nw * (CL_TILE + 2 * cl_rowf(ks, bf)) + 256 + 128 * nw) * 4; }

struct Choice {
    int family;         // 0: csrc/dwconv_cl.hip (channel per lane), 1: the sliding-window kernel of csrc/pointwise.hip
    int tile_rows;      // TH: output rows per tile (family 0: 1 / 4 / 8) or per pixel group (family 1: 1 / 2)
    int tiles_per_wg;   // tpw: vertically consecutive tiles one workgroup produces (family 1: always 1)
};

// Channel-per-lane kernel: output rows per tile (TH) and tiles per workgroup (tpw), the pair with the least estimated time.  A
// workgroup costs ~3 row steps for its weights plus, per tile, TH + k - 1 row steps and ~2 for the first rows' latency; the chip runs
// `slots` workgroups at a time (3 / 4 waves per SIMD -- the register budgets -- and 160 KB of LDS per CU), in whole rounds.
inline void cl_choice(int ks, int nw, bool bf, int B, int H, int W, int* tile_rows, int* tiles_per_wg) {
    const int ldsb = cl_lds_bytes(ks, nw, bf);
    const int n_sx = (W + CL_SW - 1) / CL_SW;
    int best_th = 1, best_tpw = 1;
    double best_t = 1e300;
    for (int th = 1; th <= 8; th *= 2) {
        if (ks == 1 && th > 1) break;                                  // k = 1: nothing is shared between rows
        if (th == 2) continue;                                         // not instantiated (1 / 4 / 8 cover the map sizes)
        const int by_waves = (ks >= 5 && th == 8 ? 12 : 16) / nw, by_lds = (160 * 1024) / ldsb;
        const long slots = 256L * (by_waves < by_lds ? by_waves : by_lds);
        const int n_ty = (H + th - 1) / th;
        // (tpw > 1 only pays at k = 1, where a tile is one row step: measured 63 -> 50 us on the 128 x 192 map; for k >= 3 it was
        //  within noise at best -- the weight loads are not what bounds the kernel -- and cost 15 % where it unbalanced the rounds)
        for (int tpw = 1; tpw <= (ks == 1 ? 8 : 1); ++tpw) {
            const long wgs = (long)B * n_sx * ((n_ty + tpw - 1) / tpw);
            const double t = (double)((wgs + slots - 1) / slots) * (3 + tpw * (th + ks - 1 + 2));
            if (t < best_t * 0.999) { best_t = t; best_th = th; best_tpw = tpw; }
            if (tpw >= n_ty) break;
        }
    }
    *tile_rows = best_th;
    *tiles_per_wg = best_tpw;
}

// Sliding-window kernel, fp32 maps: two output rows per group (measured, B = 8): +12..17 % on the stride-4 maps (C <= 192, ~200k
// pixels, L2-bandwidth-bound); slower on the C >= 256 layers, where 200+ VGPRs halve the occupancy, and C = 144 / 288 (9 channel
// chunks per lane) have no registers for a second row.  bf16 maps: one row.  Same accumulation order => same bits either way.
inline int sw_tile_rows(int ks, int C, bool bf, long px) {
    return (!bf && ks == 7 && (C == 128 || C == 192) && px >= 100000) ? 2 : 1;
}

inline bool cl_width(int C) { return C == 128 || C == 192 || C == 256 || C == 384 || C == 512; }

// The kernel a lvae_dwconv_ln_<fmt>[_v] call runs.  fmt: 0 fp32 maps, 1 bf16 maps, 2 fp32 in / f16x2 planes out, 3 bf16 in / MX-fp8
// out.  affines: how many per-channel affines follow the normalisation (LayerNorm affine, AdaLN).  per_image: the _v forms.
// Returns 0, or -22 where the launch is an argument error: the channel-per-lane kernel takes C in {128, 192, 256, 384, 512} with at
// most one affine -- a rule in (C, k, affines) only, because its LayerNorm association differs from the other kernel's -- and is the
// only one with the pre-split / quantised formats and the per-image form; the sliding-window kernel takes the two-affine case of those
// widths (fp32 and bf16 maps) and C = 144 / 288 (fp32 maps).
inline int choose(int fmt, int affines, int per_image, int B, int H, int W, int C, int k, Choice* out) {
    if (fmt < 0 || fmt > 3 || affines < 0 || affines > 2 || B <= 0 || H <= 0 || W <= 0) return -22;
    if (per_image && affines != 1) return -22;
    if (!(k == 1 || k == 3 || k == 5 || k == 7)) return -22;
    const bool bf = fmt == 1 || fmt == 3;
    if (cl_width(C) && affines < 2) {
        // one image's map must fit a buffer descriptor (2 GiB, > 44 Mpixels at stride 4): an argument error, NOT a silent switch to the
        // other kernel family (whose bits differ)
        if ((long)H * W * C * (bf ? 2 : 4) > 0x7fffffffL) return -22;
        int th, tpw;
        cl_choice(k, C / 64, bf, B, H, W, &th, &tpw);
        const int n_sx = (W + CL_SW - 1) / CL_SW, n_ty = (H + th - 1) / th, n_sy = (n_ty + tpw - 1) / tpw;
        if ((long)B * n_sx * n_sy > 0x7fffffffL) return -22;
        *out = Choice{0, th, tpw};
        return 0;
    }
    if (per_image || fmt >= 2) return -22;
    if (!(cl_width(C) || (!bf && (C == 144 || C == 288)))) return -22;
    *out = Choice{1, sw_tile_rows(k, C, bf, (long)B * H * W), 1};
    return 0;
}

}  // namespace lvae_dwln
