// gemm_h2_choice.h -- which kernel instance an f16x2 GEMM launch (lvae_gemm_desc.prec == 4) runs, whether the family takes the GEMM at
// all, and how its split-K slices are reduced: the ONE implementation of that choice.  Host arithmetic only, no HIP header.
// lvae_gemm_f32 (gemm_f32.hip) switches on its result -- the launchers of gemm_h2.hip / gemm_h2n.hip / gemm_h2p.hip only map the template
// arguments it names to an instantiation -- and lvae_gemm_h2_choice (include/lvae_hip.h) reports it, so what a test or the host
// (lvae/engine.py: Plan.gemm asks it whether a GEMM runs f16x2 or falls back to bf16x3) observes is what a launch does.
// Every form the family offers gives the same bits, so every rule below picks by speed alone; whether the family takes a GEMM is a
// rule in the GEMM's shape and modes.  The function reads the shape and mode fields of the descriptor and the PRESENCE of A1, ws, cnt,
// res and gamma; never A0, Wt, Wt16, out, bias or status (the host asks before it has filled them).
#pragma once

#include "../../include/lvae_hip.h"

namespace lvae_h2 {

struct Choice {
    int kernel;      // 1 gemm_h2_kernel, 2 gemm_h2n_kernel, 3 gemm_h2p_kernel
    int params[5];   // h2: {TN, AGELU, AMODE}; h2n: {NB, AMODE}; h2p: {WM, TN, NBUF, FOLD, NLOAD} -- the template arguments, unused slots 0
    int splitk;      // 0 none, 1 serial (inside h2n / h2p FOLD), 2 parallel + in-kernel counters, 3 parallel + reduce launch,
                     // 4 parallel, reduction deferred to the consumer
};

inline int slices(const lvae_gemm_desc& d) { return d.ksplit > 1 ? d.ksplit : 1; }

// gemm_h2n_kernel (gemm_h2n.hip): N <= 96 columns, fp32 A in plain rows or the 3x3-tap gather, any whole number of k16 steps; split-K
// in its serial form.  force: take it whenever the kernel CAN (cfg = 3: tests); otherwise where it is the faster form (shape rule
// below; same bits either way).
inline bool h2n_takes(const lvae_gemm_desc& d, bool force, Choice* c) {
    const bool conv3 = d.a_mode == LVAE_A_CONV3;
    if (d.prec != 4 || d.a_h2 || d.a_gelu || d.out_h2 || (d.a_mode != LVAE_A_PLAIN && !conv3) || d.N > 96 || (d.K & 15) || d.ldw != d.K) return false;
    if (!conv3 && (d.K1 != 0 || d.K0 != d.K || (d.lda0 & 3) || (long)d.M * d.lda0 * 4 > 0x7ffffff0L)) return false;
    if (conv3 && ((d.K0 & 15) || d.K != 9 * d.K0 || d.K1 != 0 || d.H <= 0 || d.W <= 0 || (long)d.M * d.K0 * 4 > 0x7ffffff0L)) return false;
    if ((long)d.N * d.K * 4 > 0x7ffffff0L) return false;
    const int S = slices(d);
    if (S > 1 && ((d.K / 16) % S || d.store != LVAE_ST_ROWMAJOR || (d.N & 3) || (d.ldo & 3) || (d.ldres & 3))) return false;
    // shape rule: K = 16 (mod 32) has no other f16x2 kernel (gemm_h2_kernel walks the k16 steps in pairs) -- always; otherwise where it is
    // the faster of the two (256-row workgroups: fewer than 128 of them leave the chip idle)
    // (measured, profiles/r04_gemm_h2n_narrow_output.txt: 3x3 gathers and N = 65..96 from M = 49152 on: 1.1 - 1.25x; N <= 64 plain rows and
    //  the split-K launches: gemm_h2_kernel is as fast or faster)
    if (!force && !(d.K & 16) && !(d.M >= 32768 && S == 1 && (conv3 || d.N > 64))) return false;
    *c = Choice{2, {(d.N + 31) / 32, conv3 ? LVAE_A_CONV3 : LVAE_A_PLAIN, 0, 0, 0}, 0};
    return true;
}

// fp32 A (a_h2 = 0).  force (d.cfg): 0 = choose kernel and tile width; 1..2 = gemm_h2_kernel (gemm_h2.hip) with that TN; 3 = gemm_h2n_kernel
// wherever it applies.
inline bool h2_takes(const lvae_gemm_desc& d, int force, Choice* c) {
    if ((force == 0 || force == 3) && h2n_takes(d, force == 3, c)) return true;    // force 3: wherever that kernel can
    const bool conv3 = d.a_mode == LVAE_A_CONV3, patch2 = d.a_mode == LVAE_A_PATCH2;
    if (d.prec != 4 || (d.a_mode != LVAE_A_PLAIN && !conv3 && !patch2) || (d.K & 31) || d.ldw != d.K) return false;
    if (patch2 && ((d.K0 & 7) || d.K != 4 * d.K0 || d.K1 != 0 || d.H <= 0 || d.W <= 0 || d.a_gelu || (long)d.M * 4 * d.K0 * 4 > 0x7ffffff0L))
        return false;
    if (!conv3 && !patch2 && ((d.lda0 & 3) || d.K0 + d.K1 != d.K)) return false;
    if (conv3 && ((d.K0 & 15) || d.K != 9 * d.K0 || d.K1 != 0 || d.H <= 0 || d.W <= 0 || (long)d.M * d.K0 * 4 > 0x7ffffff0L)) return false;
    const bool cat = d.K1 != 0 && !patch2;
    if (cat && (!d.A1 || (d.K0 & 15) || (d.lda1 & 3) || (long)256 * d.lda1 * 4 > 0x7fffffffL)) return false;
    if ((long)128 * d.lda0 * 4 > 0x7fffffffL || (long)192 * 4 * d.K > 0x7fffffffL) return false;
    const int S = slices(d);
    if (S > 1 && (d.K % (32 * S))) return false;
    const int M = d.M, N = d.N, K = d.K / S;
    int sel = force;
    if (sel <= 0 || sel > 2) {
        // rounds of 128 x 64c tiles over 2 x 256 workgroup slots x per-tile work / relative efficiency of the tile width
        double best = 1e300;
        const double eff[3] = {0, 0.70, 1.00};
        for (int tn = 1; tn <= 2; ++tn) {
            const long tiles = (long)((M + 127) / 128) * ((N + 64 * tn - 1) / (64 * tn)) * S;
            const long rounds = (tiles + 511) / 512;
            const double cost = rounds * (128.0 * 64 * tn) * (K + 96.0) / eff[tn];
            if (cost < best) { best = cost; sel = tn; }
        }
    }
    *c = Choice{1, {sel, d.a_gelu ? 1 : 0, d.a_mode, 0, 0}, 0};
    return true;
}

// Both operands pre-split (a_h2 = 1): gemm_h2p_kernel (gemm_h2p.hip).  force (d.cfg): 0 = choose; 10 * WM + TN = that tile (42 = 256 x 128,
// 41 = 256 x 64, 22 = 128 x 128, 21 = 128 x 64; 23 = 128 x 64 with two ring slots).
inline bool h2p_takes(const lvae_gemm_desc& d, int force, int cu_count, Choice* c) {
    if (d.prec != 4 || !d.a_h2 || d.a_mode != LVAE_A_PLAIN || d.K1 != 0 || d.K0 != d.K || (d.K & 31) || d.lda0 != d.K ||
        d.ldw != d.K || d.a_gelu || (long)256 * d.K * 4 > 0x7fffffffL)
        return false;
    const int M = d.M, N = d.N;
    if (d.ksplit > 1) {
        // serial split-K (FOLD): S slices of whole 32-deep stages, row-major fp32 / pre-split output with 16-B rows (what the reduce
        // kernel's epilogue function stores), 128 x 64 tiles (the running sum lives beside two accumulator sets)
        if ((d.K / 32) % d.ksplit || d.store != LVAE_ST_ROWMAJOR || (N & 3) || (d.ldo & 3) || (d.ldres & 3)) return false;
        // up to one workgroup per CU: eight loader waves beside the four compute waves (gemm_h2p.hip, NLOAD); more tiles: two
        // workgroups per CU hide each other's DMA issue as before
        const int tiles = ((M + 127) / 128) * ((N + 63) / 64);
        const bool loaders = tiles <= cu_count;
        *c = Choice{3, {2, 1, 3, 1, loaders ? 8 : 0}, 0};
        return true;
    }
    int sel = force;
    if (sel != 42 && sel != 41 && sel != 22 && sel != 21 && sel != 23) {
        // Tile by measurement (profiles/r03_gemm_h2p_tile_sweep.txt: every MLP shape of the model at batch 4 and 8 under each tile):
        // least padded width first (N = 192: three 64-wide tiles, not two 128-wide); 64-wide: 128 x 64 everywhere; 128-wide: 128 x 64
        // while 128 x 128 tiles would be fewer than ~4 per CU (the mid-size launches of one pipeline group: more, smaller workgroups
        // fill the chip and overlap their epilogues), 256 x 128 only for the largest (stride-4, batch 8) launches
        const int tn = (N % 128 == 0 || ((N + 127) / 128) * 128 - N < ((N + 63) / 64) * 64 - N + 1) ? 2 : 1;
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        sel = tn == 1 ? 21 : (t128 < 1024 ? 21 : (t128 >= 4096 ? 42 : 22));
        // Round 5: the 128 x 64 tile with TWO ring slots (48 KB of LDS: three workgroups per CU instead of two; its 164 registers allow
        // three waves per SIMD anyway).  One stage less of DMA look-ahead against a third workgroup whose epilogue can run under the
        // other two's main loops: -2 ... -7 % where the K loop is short and the tiles are many, +5 ... +60 % on the few-tile long-K
        // layers (profiles/r05_gemm_h2p_three_workgroups_per_cu.txt) -- taken for K <= 512 with at least two tiles per slot-pair
        const long t64 = (long)((M + 127) / 128) * ((N + 63) / 64);
        if (d.K <= 512 && t64 >= 512 && (sel == 21 || (sel == 22 && t128 < 2048))) sel = 23;
    }
    switch (sel) {
        case 42: *c = Choice{3, {4, 2, 3, 0, 0}, 0}; break;
        case 41: *c = Choice{3, {4, 1, 3, 0, 0}, 0}; break;
        case 22: *c = Choice{3, {2, 2, 2, 0, 0}, 0}; break;
        case 23: *c = Choice{3, {2, 1, 2, 0, 0}, 0}; break;      // 128 x 64, two ring slots (48 KB): three workgroups per CU
        default: *c = Choice{3, {2, 1, 3, 0, 0}, 0}; break;
    }
    return true;
}

// One kernel family: pre-split A -> gemm_h2p, fp32 A -> gemm_h2 / gemm_h2n.  The pre-split store (out_h2) exists for row-major outputs
// of whole 32-column groups behind a bias or bias + GELU epilogue, and under split-K in the serial form of gemm_h2p only.
inline int family(const lvae_gemm_desc& d, int cu_count, Choice* c) {
    if (d.out_h2 && (d.store != LVAE_ST_ROWMAJOR || (d.epi != LVAE_EPI_BIAS && d.epi != LVAE_EPI_BIAS_GELU) || (d.N & 31) ||
                     d.ldo != d.N || (d.ksplit > 1 && !d.a_h2)))
        return -22;
    const int force = d.cfg > 0 ? d.cfg : 0;
    if (d.a_h2) return h2p_takes(d, force, cu_count, c) ? 0 : -22;     // cfg = 10 WM + TN: force a tile
    return h2_takes(d, force, c) ? 0 : -22;                            // cfg: 1 / 2 = TN, 3 = gemm_h2n
}

// The launch a prec 4 descriptor gets on a device of cu_count compute units.  Returns 0 with *out filled, or -22 exactly where
// lvae_gemm_f32 returns -22 for these fields (which include what lvae_gemm_f32 checks for every arithmetic: sizes, 16-B operand rows,
// the epilogue's operands, the store's geometry).
inline int choose(const lvae_gemm_desc& d, int cu_count, Choice* out) {
    if (d.prec != 4 || d.M <= 0 || d.N <= 0 || d.K <= 0 || (d.K & 7) || (d.ldw & 7)) return -22;       // 16-B loads of the packed weights
    if ((d.epi == LVAE_EPI_GAMMA_RES || d.epi == LVAE_EPI_RES) && !d.res) return -22;
    if (d.epi == LVAE_EPI_GAMMA_RES && !d.gamma) return -22;
    if (d.store != LVAE_ST_ROWMAJOR && (d.r <= 0 || d.N % (d.r * d.r) || d.H <= 0 || d.W <= 0)) return -22;
    const int S = slices(d);
    Choice c{};
    int rc;
    if (S == 1) {
        rc = family(d, cu_count, &c);
    } else if (d.a_h2) {
        // pre-split operands: SERIAL split-K inside gemm_h2p_kernel (one workgroup adds the S slice sums in slice order: the parallel
        // form's bits without workspace or reduce launch)
        if (d.store != LVAE_ST_ROWMAJOR || (d.N & 3) || (d.ldo & 3) || (d.ldres & 3) || d.K % (32 * S)) return -22;
        rc = family(d, cu_count, &c);
        c.splitk = 1;
    } else if ((d.cfg == 0 || d.cfg == 3) && h2n_takes(d, d.cfg == 3, &c)) {
        // narrow outputs over large maps: gemm_h2n_kernel walks the slices serially too (same bits, no workspace traffic, no reduction)
        rc = 0;
        c.splitk = 1;
    } else {
        // parallel split-K: gridDim.y = S slice workgroups per tile write their partial sums to the workspace
        if (!d.ws || d.store != LVAE_ST_ROWMAJOR || (d.N & 3) || (d.ldo & 3) || (d.ldres & 3) || d.K % (32 * S)) return -22;
        rc = family(d, cu_count, &c);
        // In-kernel reduction (cnt: each tile's last-arriving slice reduces in place) only when no 128-B line of the workspace can hold
        // columns of two different tiles (N % 32 == 0, or one n-tile): a tile's reducer acquires at agent scope, which drops its CU's
        // L1 but not lines its XCD's L2 fetched earlier in this launch for a NEIGHBOURING tile's reduction.  Otherwise the counters
        // are not used: the reduce launch, or (defer_reduce) the consumer, sums the planes.
        c.splitk = (d.cnt && ((d.N & 31) == 0 || d.N <= 32)) ? 2 : d.defer_reduce ? 4 : 3;
    }
    if (rc) return rc;
    *out = c;
    return 0;
}

}  // namespace lvae_h2
