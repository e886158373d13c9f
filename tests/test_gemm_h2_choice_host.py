"""not-gpu: lvae_gemm_h2_choice -- which kernel instance of the f16x2 GEMM family (prec 4) a launch runs and how its split-K slices are
reduced (host arithmetic, no HIP call; csrc/gemm_h2_choice.h, the function lvae_gemm_f32 switches on).  Pins of the policy at its
thresholds, each from both sides, and the contract lvae/engine.py::Plan.gemm relies on: whether the family takes a GEMM does not depend
on M.  tests/test_h2_cases_host.py puts every form of the case table to the same function.

Every expected value below is worked out from the rule as it stood in the sources before the query existed (the comment at each pin
says how), not read off the function."""
import ctypes
import itertools

import pytest

import h2_cases as hc
from lvae import _native

H2P_42, H2P_41, H2P_22, H2P_23, H2P_21 = (hc.instance_of(t) for t in hc.H2P_TILES)
FOLD_LOADERS, FOLD_PLAIN = hc.instance_of(hc.FOLD_LOADERS), hc.instance_of(hc.FOLD_PLAIN)


@pytest.fixture(scope='module')
def L():
    return _native.lib()


def _desc(M, N, K, **kw):
    """A plain-rows descriptor with contiguous operands, a bias epilogue and a row-major store; kw overrides fields (pointers: 1 = present)."""
    d = _native.GemmDesc()
    d.M, d.N, d.K, d.K0, d.lda0, d.ldw, d.ldo, d.prec = M, N, K, K, K, K, N, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ask(L, M, N, K, cu=256, **kw):
    return hc.choice(L, _desc(M, N, K, **kw), cu)


def _h2p(L, M, N, K, **kw):
    rc, inst, splitk = _ask(L, M, N, K, a_h2=1, **kw)
    assert rc == 0 and inst[0] == 'h2p'
    return inst


def _conv3(M, Cin):
    return dict(a_mode=hc.A_CONV3, K0=Cin, lda0=Cin, H=128, W=M // 128 + 1)       # H, W only have to be positive here


# ------------------------------------------------------------------------------------------------ gemm_h2p: the tile rule
def test_h2p_tile_rule_at_its_thresholds(L):
    """gemm_h2p.hip's rule: tn = 2 where N % 128 == 0 or 128-wide tiles pad no more than 64-wide ones, else 1.  t128 = ceil(M / 128) *
    ceil(N / 128).  tn 1 -> 21; tn 2 -> 21 below 1024 tiles, 42 from 4096 on, 22 between.  Then, for K <= 512 and t64 = ceil(M / 128) *
    ceil(N / 64) >= 512: 21 -> 23, and 22 -> 23 while t128 < 2048.  N = 128 below: t128 = ceil(M / 128), t64 = 2 t128."""
    rows = lambda tiles: 128 * tiles                               # noqa: E731
    # K = 544 > 512: the two-slot tile is out of the picture
    assert _h2p(L, rows(1023), 128, 544) == H2P_21 and _h2p(L, rows(1023) + 1, 128, 544) == H2P_22        # t128 = 1023 | 1024
    assert _h2p(L, rows(4095), 128, 544) == H2P_22 and _h2p(L, rows(4095) + 1, 128, 544) == H2P_42        # 4095 | 4096
    assert _h2p(L, rows(2047), 128, 544) == H2P_22 and _h2p(L, rows(2048), 128, 544) == H2P_22            # 2048 matters for K <= 512 only
    # K = 512: t64 = 2 t128 >= 512 throughout; 21 and (below 2048 tiles) 22 become 23
    assert _h2p(L, rows(1023), 128, 512) == H2P_23 and _h2p(L, rows(1024), 128, 512) == H2P_23
    assert _h2p(L, rows(2047), 128, 512) == H2P_23 and _h2p(L, rows(2047) + 1, 128, 512) == H2P_22        # t128 = 2047 | 2048
    assert _h2p(L, rows(4095), 128, 512) == H2P_22 and _h2p(L, rows(4096), 128, 512) == H2P_42
    # K at 512 | 544 (whole 32-deep stages) on one shape
    assert _h2p(L, rows(1024), 128, 512) == H2P_23 and _h2p(L, rows(1024), 128, 544) == H2P_22
    # t64 at 511 | 512: N = 64 is tn 1 (64 columns of padding against none), t64 = ceil(M / 128)
    assert _h2p(L, rows(511), 64, 512) == H2P_21 and _h2p(L, rows(511) + 1, 64, 512) == H2P_23
    assert _h2p(L, rows(512), 64, 544) == H2P_21
    # N = 192: 128-wide tiles pad 64 columns, 64-wide none -> tn 1 -> 128 x 64 whatever the tile count; N = 256: tn 2
    assert _h2p(L, rows(4096), 192, 544) == H2P_21 and _h2p(L, rows(4096), 256, 544) == H2P_42
    assert _h2p(L, rows(512), 256, 544) == H2P_22 and _h2p(L, rows(511), 256, 544) == H2P_21              # t128 = 1024 | 1022
    # N = 320: 128-wide pads 64, 64-wide none -> tn 1; N = 290: 128-wide pads 94, 64-wide 30 -> tn 1; N = 380: 4 < 4 + 1 -> tn 2
    assert _h2p(L, rows(4096), 320, 544) == H2P_21 and _h2p(L, rows(4096), 290, 544) == H2P_21 and _h2p(L, rows(4096), 380, 544) == H2P_42


def test_h2p_force_codes(L):
    """cfg = 42 / 41 / 22 / 23 / 21 names the tile; any other value chooses (small shape: 21)."""
    for t in hc.H2P_TILES:
        assert _h2p(L, 549, 292, 96, cfg=t.cfg) == hc.instance_of(t)
    for cfg in (0, 1, 2, 3, 24, 40, 43, -1):
        assert _h2p(L, 549, 292, 96, cfg=cfg) == H2P_21
    assert _h2p(L, 128 * 4096, 128, 544, cfg=41) == H2P_41           # a force code is kept at every size


# ------------------------------------------------------------------------------------------------ gemm_h2n: the shape rule
def test_h2n_shape_rule_at_its_thresholds(L):
    """gemm_h2n.hip's rule under cfg 0: K = 16 (mod 32) always (no other kernel); otherwise M >= 32768 without split-K and a 3x3 gather or
    N > 64 -- within what the kernel takes (N <= 96, no second source, no GELU on load).  Where it does not, gemm_h2_kernel runs."""
    plain = lambda nb: ('h2n', nb, hc.A_PLAIN)                      # noqa: E731
    kernel = lambda *a, **kw: _ask(L, *a, **kw)[1][:1]              # noqa: E731
    assert _ask(L, 32767, 96, 64)[1][0] == 'h2' and _ask(L, 32768, 96, 64)[1] == plain(3)                # M at 32767 | 32768
    assert _ask(L, 32768, 64, 64)[1][0] == 'h2' and _ask(L, 32768, 65, 64)[1] == plain(3)                # N at 64 | 65
    assert _ask(L, 32768, 97, 64)[1][0] == 'h2' and _ask(L, 1 << 20, 97, 64)[1][0] == 'h2'               # N at 96 | 97
    for N, nb in ((24, 1), (64, 2), (96, 3)):                                                             # the gather: any N <= 96
        assert _ask(L, 32768, N, 288, **_conv3(32768, 32))[1] == ('h2n', nb, hc.A_CONV3)
        assert _ask(L, 32767, N, 288, **_conv3(32767, 32))[1][0] == 'h2'
    assert _ask(L, 32768, 97, 288, **_conv3(32768, 32))[1][0] == 'h2'
    # K & 16: the only kernel, at any M; beyond 96 columns, with GELU on load or with a second source nothing takes it
    assert _ask(L, 63, 24, 48)[1] == plain(1) and _ask(L, 63, 96, 48)[1] == plain(3) and _ask(L, 1 << 20, 40, 272)[1] == plain(2)
    assert _ask(L, 63, 97, 48)[0] == -22 and _ask(L, 63, 24, 48, a_gelu=1)[0] == -22
    assert _ask(L, 63, 24, 48, K0=16, K1=32, lda0=16, lda1=32, A1=1)[0] == -22
    assert _ask(L, 63, 24, 40)[0] == -22 and _ask(L, 63, 24, 44)[0] == -22                                 # no whole number of k16 steps
    # what the kernel does not take stays with gemm_h2_kernel at any M: GELU on load, two sources, the 2x2 gather
    assert kernel(1 << 16, 96, 64, a_gelu=1) == ('h2',)
    assert kernel(1 << 16, 96, 64, K0=32, K1=32, lda0=32, lda1=32, A1=1) == ('h2',)
    assert kernel(1 << 16, 96, 64, a_mode=hc.A_PATCH2, K0=16, lda0=16, H=256, W=256) == ('h2',)
    # cfg 3 takes it wherever the kernel can; cfg 1 / 2 never
    assert _ask(L, 63, 24, 64, cfg=3)[1] == plain(1) and _ask(L, 32768, 96, 64, cfg=1)[1] == ('h2', 1, 0, hc.A_PLAIN)
    assert _ask(L, 63, 97, 64, cfg=3)[1][0] == 'h2'                # beyond it cfg 3 chooses like cfg 0
    # split-K: the shape rule needs S == 1, so cfg 0 goes parallel; cfg 3 takes the serial form
    kw = dict(ksplit=2, ws=1)
    rc, inst, splitk = _ask(L, 32768, 96, 256, **kw)
    assert (rc, inst[0], splitk) == (0, 'h2', hc.SPLITK_REDUCE_LAUNCH)
    assert _ask(L, 32768, 96, 256, cfg=3, **kw)[1:] == (plain(3), hc.SPLITK_SERIAL)
    assert _ask(L, 549, 24, 96, cfg=3, ksplit=2)[1:] == (plain(1), hc.SPLITK_SERIAL)       # K / 16 = 6 steps in 2 slices; no workspace needed
    assert _ask(L, 549, 24, 96, cfg=0, ksplit=2, ws=1)[0] == -22                           # parallel: K % (32 S) != 0
    assert _ask(L, 549, 24, 96, cfg=3, ksplit=4)[0] == -22                                 # 6 steps in 4 slices


# ------------------------------------------------------------------------------------------------ gemm_h2: the tile-width cost model
def test_h2_tile_width_flips_across_a_round(L):
    """gemm_h2.hip's cost model: cost(TN) = rounds(TN) x 64 TN / eff(TN) x (the same factor for both), rounds = ceil(tiles / 512), eff =
    0.70 / 1.00: TN 2 is taken iff 2 rounds(2) < rounds(1) / 0.7, i.e. unless rounds(2) >= 0.714 rounds(1).
    N = 128: tiles = 2 mt | mt.  mt = 256: 1 | 1 round -> TN 1; mt = 257: 2 | 1 -> TN 2; mt = 513: 3 | 2 rounds: 4.29 > 4 -> TN 2.
    N = 192: tiles = 3 mt | 2 mt.  mt = 170: 510 | 340 tiles: 1 | 1 -> TN 1; 171: 513 | 342: 2 | 1 -> TN 2; 256: 768 | 512: 2 | 1 -> TN 2;
    257: 771 | 514: 2 | 2 -> TN 1; 342: 1026 | 684: 3 | 2 -> TN 2.  N = 64: the same tiles either way -> TN 1 at every size."""
    tn = lambda mt, N, **kw: _ask(L, 128 * mt, N, 256, **kw)[1][:2]                 # noqa: E731
    for mt, N, want in ((256, 128, 1), (257, 128, 2), (512, 128, 2), (513, 128, 2), (170, 192, 1), (171, 192, 2), (256, 192, 2),
                        (257, 192, 1), (341, 192, 1), (342, 192, 2), (1, 64, 1), (513, 64, 1), (4096, 64, 1)):
        assert tn(mt, N) == ('h2', want), (mt, N)
    assert tn(256, 128) == tn(256, 128, cfg=-1) == tn(256, 128, cfg=7) == ('h2', 1)      # anything but 1 / 2 chooses
    assert tn(256, 128, cfg=2) == ('h2', 2) and tn(257, 128, cfg=1) == ('h2', 1)
    # the last row of a tile: M = 128 * 256 + 1 is 257 m-tiles
    assert _ask(L, 128 * 256 + 1, 128, 256)[1][:2] == ('h2', 2)
    # parallel split-K multiplies the tiles by S: mt = 128, N = 128, S = 2: 512 | 256 tiles -> TN 1; mt = 129: 516 | 258 -> TN 2
    assert tn(128, 128, ksplit=2, ws=1) == ('h2', 1) and tn(129, 128, ksplit=2, ws=1) == ('h2', 2)


# ------------------------------------------------------------------------------------------------ split-K forms
@pytest.mark.parametrize('cu', (64, 256, 304))
def test_fold_loader_rule(L, cu):
    """gemm_h2p.hip under ksplit > 1: ceil(M / 128) ceil(N / 64) <= CU count runs the FOLD instance with loader waves.  N = 64: one tile per
    128 rows; N = 512: eight."""
    fold = lambda M, N, **kw: _ask(L, M, N, 256, cu=cu, a_h2=1, ksplit=2, **kw)[1:]     # noqa: E731
    assert fold(128 * cu, 64) == (FOLD_LOADERS, hc.SPLITK_SERIAL) and fold(128 * cu + 1, 64) == (FOLD_PLAIN, hc.SPLITK_SERIAL)
    assert fold(128 * (cu // 8), 512) == (FOLD_LOADERS, hc.SPLITK_SERIAL) and fold(128 * (cu // 8) + 1, 512) == (FOLD_PLAIN, hc.SPLITK_SERIAL)
    for cfg in hc.H2P_FORCE_CODES:                                    # cfg is not read under split-K
        assert fold(128 * cu, 64, cfg=cfg)[0] == FOLD_LOADERS
    assert _ask(L, 549, 64, 256, cu=cu, a_h2=1, ksplit=3)[0] == -22   # 8 stages in 3 slices
    assert _ask(L, 549, 66, 256, cu=cu, a_h2=1, ksplit=2)[0] == -22   # rows of the output are no whole 16 bytes


def test_counters_are_used_where_tiles_share_no_line(L):
    """lvae_gemm_f32's rule: with arrival counters the last slice of a tile reduces in the kernel only for N % 32 == 0 or N <= 32;
    otherwise the counters are dropped and the reduce launch (or, with defer_reduce, the consumer) sums the planes."""
    sk = lambda N, **kw: _ask(L, 549, N, 256, cfg=1, ksplit=2, ws=1, **kw)[2]          # noqa: E731
    for N, with_cnt in ((32, 2), (36, 3), (64, 2), (24, 2), (96, 2), (100, 3)):
        assert sk(N, cnt=1) == with_cnt and sk(N) == hc.SPLITK_REDUCE_LAUNCH, N
        assert sk(N, defer_reduce=1) == hc.SPLITK_DEFERRED
        assert sk(N, cnt=1, defer_reduce=1) == (2 if with_cnt == 2 else hc.SPLITK_DEFERRED)
    assert _ask(L, 549, 64, 256, cfg=1, ksplit=2)[0] == -22                             # parallel split-K needs the workspace
    assert _ask(L, 549, 64, 256, cfg=1, ksplit=2, ws=1, ldo=66)[0] == -22
    assert _ask(L, 549, 64, 256, cfg=1, ksplit=3, ws=1)[0] == -22                       # K % (32 S)
    assert _ask(L, 549, 64, 256, cfg=1)[2] == _ask(L, 549, 64, 256, cfg=1, ksplit=1)[2] == hc.SPLITK_NONE


# ------------------------------------------------------------------------------------------------ the export
def test_return_codes_of_the_export(L):
    d = _desc(549, 64, 256)
    assert L.lvae_gemm_h2_choice(ctypes.byref(d), 256, None, None, None) == 0            # the outputs may be NULL
    assert L.lvae_gemm_h2_choice(None, 256, None, None, None) == -22
    assert L.lvae_gemm_h2_choice(ctypes.byref(d), 0, None, None, None) == -22 and L.lvae_gemm_h2_choice(ctypes.byref(d), -4, None, None, None) == -22
    for prec in (0, 1, 2, 3, 5):
        assert _ask(L, 549, 64, 256, prec=prec)[0] == -22
    # what lvae_gemm_f32 refuses for these fields: sizes, rows of the packed weights, the epilogue's operands, the store's geometry
    assert _ask(L, 0, 64, 256)[0] == -22 and _ask(L, 549, 0, 256)[0] == -22 and _ask(L, 549, 64, 0)[0] == -22
    assert _ask(L, 549, 64, 256, ldw=260)[0] == -22
    assert _ask(L, 549, 64, 256, epi=hc.EPI_RES)[0] == -22 and _ask(L, 549, 64, 256, epi=hc.EPI_RES, res=1)[0] == 0
    assert _ask(L, 549, 64, 256, epi=hc.EPI_GAMMA_RES, res=1)[0] == -22 and _ask(L, 549, 64, 256, epi=hc.EPI_GAMMA_RES, res=1, gamma=1)[0] == 0
    assert _ask(L, 549, 64, 256, store=_native.ST_SHUFFLE)[0] == -22
    assert _ask(L, 549, 64, 256, store=_native.ST_SHUFFLE, r=2, H=9, W=61)[0] == 0
    # the pre-split store: whole 32-column groups, dense rows, bias or bias + GELU, and under split-K the serial form of gemm_h2p only
    assert _ask(L, 549, 64, 256, out_h2=1)[0] == 0 and _ask(L, 549, 72, 256, out_h2=1)[0] == -22
    assert _ask(L, 549, 64, 256, out_h2=1, ldo=96)[0] == -22 and _ask(L, 549, 64, 256, out_h2=1, epi=hc.EPI_RES, res=1)[0] == -22
    assert _ask(L, 549, 64, 256, out_h2=1, ksplit=2, ws=1)[0] == -22 and _ask(L, 549, 64, 256, out_h2=1, ksplit=2, a_h2=1)[0] == 0
    # operands of gemm_h2p are dense: one source, rows of K
    assert _ask(L, 549, 64, 256, a_h2=1, lda0=260)[0] == -22 and _ask(L, 549, 64, 48, a_h2=1)[0] == -22


# ------------------------------------------------------------------------------------------------ the host's contract
def _plan_gemm_descs(M):
    """Descriptors as lvae/engine.py::Plan.gemm fills them before it asks (cfg 0, ksplit unset, no workspace): the shapes and modes of
    the models' GEMMs and, around them, what the family does not take."""
    out = []
    for N, K in itertools.product((3, 24, 48, 64, 96, 97, 128, 192, 384, 768), (8, 24, 48, 64, 144, 192, 272, 384, 432, 768)):
        for epi, a_gelu, out_h2 in ((hc.EPI_BIAS, 0, 0), (hc.EPI_BIAS_GELU, 0, 1), (hc.EPI_GAMMA_RES, 1, 0)):
            out.append(_desc(M, N, K, epi=epi, a_gelu=a_gelu, out_h2=out_h2, res=1, gamma=1))
        out.append(_desc(M, N, K, lda0=K + 4))
        if K % 16 == 0 and K >= 32:
            out.append(_desc(M, N, K, K0=K - 16, K1=16, lda0=K - 16, lda1=16, A1=1))
            out.append(_desc(M, N, K, K0=16, K1=K - 16, lda0=16, lda1=K - 16, A1=1))
            out.append(_desc(M, N, K, K0=K - 8, K1=8, lda0=K - 8, lda1=8, A1=1))
    for N, Cin in itertools.product((24, 48, 96, 192, 384), (8, 16, 24, 32, 48, 96)):
        out.append(_desc(M, N, 9 * Cin, **_conv3(M, Cin)))
        out.append(_desc(M, N, 9 * Cin, a_gelu=1, **_conv3(M, Cin)))
        out.append(_desc(M, N, 4 * Cin, a_mode=hc.A_PATCH2, K0=Cin, lda0=Cin, H=64, W=M // 64 + 1))
    return out


def test_eligibility_does_not_depend_on_m(L):
    """Plan.gemm decides between f16x2 and bf16x3 -- other output bits -- by the return code alone, and batched and single-image plans,
    encoder and decoder must agree: below the 2 GiB operand limits the code is the same for M and 8 M (and across the narrow-output
    kernel's M threshold, where the KERNEL changes), whatever the CU count."""
    taken = refused = 0
    for M in (1, 96, 4095, 4096, 6144, 32767, 49152):
        for a, b in zip(_plan_gemm_descs(M), _plan_gemm_descs(8 * M)):
            rcs = {L.lvae_gemm_h2_choice(ctypes.byref(d), cu, None, None, None) for d in (a, b) for cu in (1, 64, 256, 304)}
            assert rcs in ({0}, {-22}), (M, a.N, a.K, a.K0, a.K1, a.a_mode, a.a_gelu, a.out_h2)
            taken += rcs == {0}
            refused += rcs == {-22}
    assert taken > 500 and refused > 500                            # both answers are met
    # ... and with M it is the kernel that changes: the 3x3 head over 48 channels of a 512 x 768 image at batch 1 and 8
    assert _ask(L, 6144, 96, 432, **_conv3(6144, 48))[1] == _ask(L, 49152, 96, 432, **_conv3(49152, 48))[1] == ('h2n', 3, hc.A_CONV3)
    assert _ask(L, 6144, 96, 288, **_conv3(6144, 32))[1][0] == 'h2' and _ask(L, 49152, 96, 288, **_conv3(49152, 32))[1] == ('h2n', 3, hc.A_CONV3)
