"""The instance and case table of the f16x2 GEMM family (prec 4: csrc/gemm_h2.hip, csrc/gemm_h2n.hip, csrc/gemm_h2p.hip), shared by
tests/test_gpu_h2_instances.py (which launches every instance that can take a case and compares the forms bit for bit, and with fp64)
and tests/test_h2_cases_host.py (which checks, without a GPU, that every form of the table runs the instance the table names -- asked of
lvae_gemm_h2_choice, the function the launch path switches on -- and that every shape still straddles what it is listed for).
h2_takes / h2n_takes / h2p_takes below are the tests' own statement of what the family takes; the library's is csrc/gemm_h2_choice.h.

The family's contract: every launch form gives the same bits, so the dispatcher picks by speed alone.  A form is (a_h2, cfg, ksplit,
cnt); `forms(case, cu)` lists the ones a case can take together with the kernel instance each of them runs:

  gemm_h2_kernel<TN, AGELU, AMODE>          ('h2', TN, a_gelu, a_mode)       cfg = 1 / 2; 128 x 64 TN tiles; K % 32 == 0
  gemm_h2n_kernel<NB, AMODE>                ('h2n', NB, a_mode)              cfg = 3; NB = ceil(N / 32) <= 3; 256-row workgroups of
                                                                             eight 32-row waves; weight chunks of N_CS k16 steps; the
                                                                             only kernel for K = 16 (mod 32); serial split-K
  gemm_h2p_kernel<WM, TN, NBUF, FOLD, NLOAD> ('h2p', WM, TN, NBUF, FOLD, NLOAD)  a_h2 = 1; cfg = 42 / 41 / 22 / 23 / 21; 64 WM x 64 TN
                                                                             tiles; under ksplit > 1 cfg is ignored and one of the two
                                                                             FOLD instances runs, by fold_loaders()
"""
from collections import namedtuple

import gemm_cases as gc

A_PLAIN, A_PATCH2, A_CONV3 = gc.A_PLAIN, gc.A_PATCH2, gc.A_CONV3
EPI_BIAS, EPI_BIAS_GELU, EPI_GAMMA_RES, EPI_RES = gc.EPIS
EPIS = gc.EPIS
EINVAL = -22

# ------------------------------------------------------------------------------------------------ instances
# gemm_h2.hip: the five uses of LVAE_H2_LAUNCH(G, AM), in the order lvae_gemm_h2_launch writes them; each is two instances (TN = 1, 2)
H2_TNS = (1, 2)
H2_LAUNCHES = ((0, A_PATCH2), (1, A_CONV3), (0, A_CONV3), (1, A_PLAIN), (0, A_PLAIN))          # (a_gelu, a_mode)
H2_BM = 128


def h2_bn(tn):
    return 64 * tn


# gemm_h2n.hip
H2N_NBS = (1, 2, 3)
H2N_AMODES = (A_PLAIN, A_CONV3)
H2N_BM, H2N_WAVE_ROWS, H2N_MAX_N = 256, 32, 96
H2N_CHUNK = 8                                   # N_CS: k16 steps per weight chunk
H2N_PREFETCH = {1: 8, 2: 8, 3: 4}               # n_d<NB>(): k16 steps the A loads run ahead

# gemm_h2p.hip: launch_h2p<WM, TN, NBUF[, FOLD[, NLOAD]]>; cfg = the force code of gemm_h2_choice.h::h2p_takes, 21 its `default:`
Tile = namedtuple('Tile', 'cfg WM TN NBUF FOLD NLOAD')
H2P_TILES = (Tile(42, 4, 2, 3, False, 0), Tile(41, 4, 1, 3, False, 0), Tile(22, 2, 2, 2, False, 0), Tile(23, 2, 1, 2, False, 0),
             Tile(21, 2, 1, 3, False, 0))
H2P_DEFAULT = 21
H2P_FORCE_CODES = (42, 41, 22, 21, 23)          # the codes `sel` is kept for, in the order of the test in front of the tile rule
FOLD_LOADERS = Tile(None, 2, 1, 3, True, 8)     # ksplit > 1 and tiles <= CU count: eight loader waves
FOLD_PLAIN = Tile(None, 2, 1, 3, True, 0)       # more tiles than CUs
H2P_STAGE = 32                                  # k per LDS stage; NBUF - 1 stages in flight


def tile_bm(t):
    return 64 * t.WM


def tile_bn(t):
    return 64 * t.TN


def instance_of(t):
    return ('h2p', t.WM, t.TN, t.NBUF, t.FOLD, t.NLOAD)


def all_instances():
    """The 10 + 6 + 7 kernel instances a prec 4 launch can reach."""
    return ({('h2', tn, g, am) for tn in H2_TNS for g, am in H2_LAUNCHES} | {('h2n', nb, am) for nb in H2N_NBS for am in H2N_AMODES} |
            {instance_of(t) for t in H2P_TILES + (FOLD_LOADERS, FOLD_PLAIN)})


def fold_tiles(M, N):
    return -(-M // 128) * -(-N // 64)


def fold_loaders(M, N, cu):
    """gemm_h2p_kernel under ksplit > 1: as many 128 x 64 tiles as the device has CUs, or fewer, take the instance with loader waves."""
    return fold_tiles(M, N) <= cu


FOLD_THRESHOLD_N = 512


def fold_threshold_ms(cu, N=FOLD_THRESHOLD_N):
    """(M below, M above) the FOLD rule's threshold at N columns for a device of `cu` compute units, both with a cut last m-tile:
    549 rows are five m-tiles (N = 512: 40 tiles); the first m-tile count whose tiles exceed cu, less 5 rows, is above (256 CUs and
    N = 512: 33 * 128 - 5 rows, 264 tiles)."""
    tn = -(-N // 64)
    return gc.RAGGED_M, (cu // tn + 1) * 128 - 5


# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple('Case', 'a_mode M N K K0 K1 lda0 lda1 ldo B H W epi a_gelu out_h2 S')


def case_id(c):
    s = f"{('plain', 'patch2', 'conv3')[c.a_mode]}-M{c.M}-N{c.N}-K{c.K}-epi{c.epi}"
    if c.K1:
        s += f'-cat{c.K0}+{c.K1}'
    if c.a_mode == A_PLAIN and c.lda0 != c.K0:
        s += f'-lda{c.lda0}'
    if c.ldo != c.N:
        s += f'-ldo{c.ldo}'
    if c.a_mode != A_PLAIN:
        s += f'-{c.B}x{c.H}x{c.W}'
    if c.S > 1:
        s += f'-S{c.S}'
    return s + ('-agelu' if c.a_gelu else '') + ('-h2out' if c.out_h2 else '')


def _plain(M, N, K, epi, lda0=None, ldo=None, a_gelu=0, K1=0, lda1=0, out_h2=0, S=1):
    K0 = K - K1
    return Case(A_PLAIN, M, N, K, K0, K1, lda0 or K0, lda1, ldo or N, 0, 0, 0, epi, a_gelu, out_h2, S)


def _conv3(Cin, N, epi, a_gelu=0, bhw=gc.GATHER_MAP, S=1):
    B, H, W = bhw
    return Case(A_CONV3, B * H * W, N, 9 * Cin, Cin, 0, Cin, 0, N, B, H, W, epi, a_gelu, 0, S)


def _patch2(Cin, N, epi):
    B, Ho, Wo = gc.GATHER_MAP
    return Case(A_PATCH2, B * Ho * Wo, N, 4 * Cin, Cin, 0, Cin, 0, N, B, Ho, Wo, epi, 0, 0, 1)


# ---- what each kernel takes (gemm_h2_kernel / gemm_h2n_kernel when forced / gemm_h2p_kernel / the parallel split-K form), for the
# shapes of this table (the 2^31 byte limits are out of reach here): the contract as the tests state it, independent of the library's
# csrc/gemm_h2_choice.h
def h2_takes(c):
    """gemm_h2_kernel (cfg = 1 / 2): k16 steps in pairs; S > 1 is the parallel form (workspace + reduction)."""
    if c.K % 32 or (c.out_h2 and (c.S > 1 or c.N % 32 or c.ldo != c.N or c.epi not in (EPI_BIAS, EPI_BIAS_GELU))):
        return False
    if c.S > 1 and (c.K % (32 * c.S) or c.N % 4 or c.ldo % 4):
        return False
    if c.a_mode == A_PATCH2:
        return c.K0 % 8 == 0 and not c.a_gelu
    if c.a_mode == A_CONV3:
        return c.K0 % 16 == 0
    return c.lda0 % 4 == 0 and c.K0 + c.K1 == c.K and (not c.K1 or (c.K0 % 16 == 0 and c.lda1 % 4 == 0))


def h2n_takes(c):
    """gemm_h2n_kernel when forced (cfg = 3); S > 1 is its serial form."""
    if c.N > H2N_MAX_N or c.K % 16 or c.a_gelu or c.out_h2 or c.a_mode == A_PATCH2 or c.K1:
        return False
    if c.S > 1 and ((c.K // 16) % c.S or c.N % 4 or c.ldo % 4):
        return False
    return c.K0 % 16 == 0 if c.a_mode == A_CONV3 else c.lda0 % 4 == 0


def h2p_takes(c):
    """gemm_h2p_kernel (a_h2 = 1); S > 1 is FOLD."""
    if c.a_mode != A_PLAIN or c.K1 or c.K % 32 or c.lda0 != c.K or c.a_gelu:
        return False
    if c.out_h2 and (c.N % 32 or c.ldo != c.N or c.epi not in (EPI_BIAS, EPI_BIAS_GELU)):
        return False
    return c.S == 1 or ((c.K // 32) % c.S == 0 and c.K % (32 * c.S) == 0 and c.N % 4 == 0 and c.ldo % 4 == 0)


def h2_instance(c, tn):
    return ('h2', tn, c.a_gelu, c.a_mode)


def h2n_instance(c):
    return ('h2n', -(-c.N // 32), c.a_mode)


def cnt_in_kernel(c):
    """With arrival counters the tile's last slice reduces in the kernel only when no 128-B line of the workspace holds columns of two
    tiles; the other shapes go to the reduce launch."""
    return c.N % 32 == 0 or c.N <= 32


Form = namedtuple('Form', 'name a_h2 cfg cnt instance')


def forms(c, cu=256):
    """Every launch form that takes case c, with the instance it runs (None: the library's own choice among the instances the forced
    forms name).  The first form is the one the others are compared with."""
    out = []
    only_h2n = c.K % 32 != 0
    if c.S == 1:
        if h2_takes(c) or (only_h2n and h2n_takes(c)):
            out.append(Form('cfg 0', 0, 0, False, h2n_instance(c) if only_h2n else None))
        if h2_takes(c):
            out += [Form(f'cfg {tn}', 0, tn, False, h2_instance(c, tn)) for tn in H2_TNS]
        if h2n_takes(c):
            out.append(Form('cfg 3', 0, 3, False, h2n_instance(c)))
        if h2p_takes(c):
            out += [Form(f'h2p {t.cfg}', 1, t.cfg, False, instance_of(t)) for t in H2P_TILES]
            out.append(Form('h2p 0', 1, 0, False, None))
        return out
    if h2_takes(c):
        out.append(Form('cfg 0 reduce launch', 0, 0, False, None))
        for tn in H2_TNS:
            out.append(Form(f'cfg {tn} reduce launch', 0, tn, False, h2_instance(c, tn)))
            out.append(Form(f'cfg {tn} counters', 0, tn, True, h2_instance(c, tn)))
    if h2n_takes(c):
        out.append(Form('cfg 3 serial', 0, 3, False, h2n_instance(c)))
    if h2p_takes(c):
        t = FOLD_LOADERS if fold_loaders(c.M, c.N, cu) else FOLD_PLAIN
        out.append(Form('fold loaders' if t.NLOAD else 'fold', 1, 0, False, instance_of(t)))
    return out


# ---- gemm_h2_kernel and gemm_h2p_kernel, plain rows
# 549 = 2 * 256 + 37: more than one m-tile with a cut last one for 64, 128 and 256 rows; 63 < every tile; 1
PLAIN_MS = (1, 63, 549)
RAGGED_M = gc.RAGGED_M
# 24: narrower than every tile; 290: N % 4 != 0 (the scalar stores) and a cut last tile of several for 64 and 128 columns; 292: the
# same on the 16-byte path
PLAIN_NS = (24, 290, 292)
RAGGED_NS = (290, 292)
NARROW_N = 24
# 1, 2, 3, 4, 5 and 8 stages of 32: gemm_h2_kernel looks two k16 stages ahead of the one it stores (K = 32: the loop is shorter than
# that), gemm_h2p_kernel keeps NBUF - 1 = 1 or 2 stages in flight (1 stage: below it, the clamp of the DMA prologue; 2: on it for
# NBUF = 3); odd and even counts above.  128 is added to the issue's list, which leaves the three-slot ring's main loop (steps of
# NBUF stages, then 0 to 2 more) without a count = 1 (mod 3) above 3: 3, 5 and 8 end it after 0, 2 and 2 stages
PLAIN_KS = (32, 64, 96, 128, 160, 256)


def plain_cases():
    """The ragged M with every N, K and epilogue; the other M with every N and K, the epilogue rotating; one padded lda0; ldo > N on the
    16-byte path, on the scalar path with N % 4 == 0 (ldo % 4 != 0) and with N % 4 != 0; two A sources (K0 = 16, K1 = 48) with padded
    leading dimensions; GELU on load."""
    out = [_plain(RAGGED_M, N, K, epi) for N in PLAIN_NS for K in PLAIN_KS for epi in EPIS]
    n = 0
    for M in PLAIN_MS:
        if M == RAGGED_M:
            continue
        for N in PLAIN_NS:
            for K in PLAIN_KS:
                out.append(_plain(M, N, K, EPIS[n % 4]))
                n += 1
    out += [_plain(RAGGED_M, 292, 96, EPI_BIAS, lda0=100),
            _plain(RAGGED_M, 292, 64, EPI_RES, ldo=296),
            _plain(RAGGED_M, 292, 96, EPI_GAMMA_RES, ldo=293),
            _plain(RAGGED_M, 290, 96, EPI_BIAS_GELU, ldo=295),
            _plain(RAGGED_M, 292, 64, EPI_BIAS, K1=48, lda0=20, lda1=52),
            _plain(RAGGED_M, 290, 64, EPI_GAMMA_RES, K1=48, lda0=20, lda1=52),
            _plain(RAGGED_M, 292, 96, EPI_BIAS, a_gelu=1),
            _plain(RAGGED_M, 24, 32, EPI_BIAS_GELU, a_gelu=1)]
    return out


def h2p_cases():
    """The plain cases gemm_h2p_kernel takes: one contiguous source, no GELU on load."""
    return [c for c in plain_cases() if h2p_takes(c)]


# ---- gemm_h2_kernel, gathers.  GATHER_MAP = 2 x 9 x 17 = 306 rows: an image boundary inside a tile, a tile boundary inside an image
def conv3_cases():
    """Cin = 32 (two k16 stages per tap), with and without GELU on load, N narrower than a tile and cut for both widths; 1 x 1 maps,
    where only the centre tap is inside.  (Cin = 16: conv3_refusals.)"""
    out, n = [], 0
    for a_gelu in (0, 1):
        for N in (NARROW_N, 292):
            for epi in ((EPI_BIAS, EPI_BIAS_GELU), (EPI_GAMMA_RES, EPI_RES))[n % 2]:
                out.append(_conv3(32, N, epi, a_gelu))
            n += 1
    out.append(_conv3(32, NARROW_N, EPI_BIAS, 0, (3, 1, 1)))
    out.append(_conv3(32, 292, EPI_BIAS_GELU, 1, (3, 1, 1)))
    return out


def patch2_cases():
    out, n = [], 0
    for Cin in (8, 40):                                   # K = 32: one stage pair, i = 0 / 1 in one k16 stage each; K = 160
        for N in (NARROW_N, 292):
            for epi in ((EPI_BIAS, EPI_GAMMA_RES), (EPI_BIAS_GELU, EPI_RES))[n % 2]:
                out.append(_patch2(Cin, N, epi))
            n += 1
    return out


def conv3_refusals():
    """Cin = 16 gives K = 144 = 16 (mod 32): gemm_h2_kernel walks the k16 steps in pairs and does not take it -- an undocumented
    refusal, recorded here: (case, cfg, return code).  Without GELU on load and N <= 96 the library's choice is gemm_h2n_kernel (those
    shapes are h2n_conv3_cases)."""
    out = []
    for a_gelu in (0, 1):
        for N in (NARROW_N, 292):
            c = _conv3(16, N, EPI_BIAS, a_gelu)
            out += [(c, 1, EINVAL), (c, 2, EINVAL)]
            if not h2n_takes(c):
                out += [(c, 0, EINVAL), (c, 3, EINVAL)]
    return out


def h2_cases():
    return plain_cases() + conv3_cases() + patch2_cases()


# ---- gemm_h2n_kernel
# a full and a cut last 32-column block for every NB: 8, 24 | 32; 40 | 64; 68, 94 | 96; 30 and 94: N % 4 != 0, the scalar stores
H2N_NS = (8, 24, 30, 32, 40, 64, 68, 94, 96)
# 16: one step, below the A prefetch distance; 48: 3 steps, = 16 (mod 32); 128: exactly one weight chunk; 144: one chunk plus one
# step; 272: two chunks plus one step, = 16 (mod 32)
H2N_KS = (16, 48, 128, 144, 272)


def h2n_plain_cases():
    out = [_plain(RAGGED_M, N, K, epi) for N in H2N_NS for K in H2N_KS for epi in EPIS]
    n = 0
    for M in PLAIN_MS:
        if M == RAGGED_M:
            continue
        for N in H2N_NS:
            for K in H2N_KS:
                out.append(_plain(M, N, K, EPIS[n % 4]))
                n += 1
    out += [_plain(RAGGED_M, 68, 48, EPI_RES, ldo=72),
            _plain(RAGGED_M, 68, 144, EPI_GAMMA_RES, ldo=71),
            _plain(RAGGED_M, 30, 48, EPI_BIAS_GELU, ldo=33),
            _plain(RAGGED_M, 64, 144, EPI_BIAS, lda0=148)]
    return out


def h2n_conv3_cases():
    """Cin = 16: K = 144, one chunk plus one step; Cin = 48: K = 432, 27 steps, a short last chunk, three steps per tap.  One N per NB
    (94: a cut block on the scalar path), every epilogue; 1 x 1 maps."""
    out = [_conv3(Cin, N, epi) for Cin in (16, 48) for N in (24, 64, 94) for epi in EPIS]
    out.append(_conv3(16, 24, EPI_BIAS, 0, (3, 1, 1)))
    return out


def h2n_cases():
    return h2n_plain_cases() + h2n_conv3_cases()


# ---- out_h2: the result stored as H2K32 planes.  288 = 2 * 128 + 32 = 4 * 64 + 32: a cut last n-tile for both widths; 32 < every tile;
# 96: one full 64-wide tile and a cut second one.  S = 3 at K = 96 is FOLD with one stage per slice
OUT_H2_NS = (32, 96, 288)


def out_h2_cases():
    return [_plain(RAGGED_M, N, 96, epi, out_h2=1, S=S) for S in (1, 3) for N in OUT_H2_NS for epi in (EPI_BIAS, EPI_BIAS_GELU)]


# ---- split-K (N % 4 == 0 throughout)
def parallel_split_cases():
    """gemm_h2_kernel with S slice workgroups per tile: N = 64 takes the in-kernel reduction when counters are given, N = 292 goes to
    the reduce launch either way.  FOLD takes all of them, the serial form of gemm_h2n_kernel those with N = 64."""
    out, n = [], 0
    for M in (63, RAGGED_M):
        for N in (64, 292):
            for S in (2, 4):
                out.append(_plain(M, N, 256, EPIS[n % 4], S=S))
                n += 1
    return out


def fold_cases():
    """K = 256: 4, 2 and 1 stages per slice; K = 96 with S = 3: one stage per slice, three stages in all (= NBUF).  N = 292: full tiles
    (the straight-line tail) and a cut one (the reduce kernel's tail) in one launch."""
    out, n = [], 1
    for N in (64, 292):
        for K, S in ((256, 2), (256, 4), (256, 8), (96, 3)):
            out.append(_plain(RAGGED_M, N, K, EPIS[n % 4], S=S))
            n += 1
    return out


# (side, N, epilogue) of the cases on either side of `tiles <= CU count`; M follows from the device's count.  N = 512, EPI_BIAS_GELU is
# also run with the pre-split store (its straight-line tail), EPI_GAMMA_RES takes the other straight-line tail; N = 516 has a cut ninth
# n-tile (the reduce kernel's tail next to the straight-line one in one launch), EPI_BIAS carries the own-arithmetic bound
FOLD_THRESHOLD_SPECS = tuple((side, N, epi) for side in ('below', 'above')
                             for N, epi in ((512, EPI_BIAS_GELU), (512, EPI_GAMMA_RES), (516, EPI_RES), (516, EPI_BIAS)))


def fold_threshold_case(cu, side, N, epi):
    M = fold_threshold_ms(cu, N)[side == 'above']
    return _plain(M, N, 256, epi, S=2)


def h2n_serial_cases():
    """K = 96 with S = 2, 3: slices of 3 and 2 steps, shorter than a weight chunk; K = 288 with S = 2: the slice boundary (step 9)
    inside the second chunk; conv3 with Cin = 48 (K = 432) and S = 3: 9 steps per slice, three chunks and a short fourth.  Only K = 96
    with S = 3 has a second form (K % (32 S) == 0), so the others come with EPI_BIAS for the own-arithmetic bound and with one more
    epilogue each."""
    out = []
    for i, N in enumerate((24, 64, 96)):
        for K, S in ((96, 2), (96, 3), (288, 2)):
            out.append(_plain(RAGGED_M, N, K, EPI_BIAS, S=S))
            out.append(_plain(RAGGED_M, N, K, EPIS[1 + i], S=S))
        out.append(_conv3(48, N, EPI_BIAS, S=3))
        out.append(_conv3(48, N, EPIS[1 + i], S=3))
    return out


def split_cases():
    out = []
    for c in parallel_split_cases() + fold_cases() + h2n_serial_cases():
        if c not in out:
            out.append(c)
    return out


def split_cnt_entries(M, N):
    return gc.split_cnt_entries(M, N)


# ---- rows of the ragged launch against the same rows launched alone: a slice that starts mid-tile (100 is no multiple of 32), the
# single last row
ROW_SLICES = ((100, 63), (RAGGED_M - 1, 1))
ROW_CASES = {'h2': _plain(RAGGED_M, 292, 96, EPI_GAMMA_RES), 'h2p': _plain(RAGGED_M, 292, 96, EPI_GAMMA_RES),
             'h2n': _plain(RAGGED_M, 68, 144, EPI_GAMMA_RES)}

# ---- K = 16 (mod 32) has one kernel: gemm_h2_kernel refuses it, and so does the family beyond 96 columns
ODD_K_REFUSALS = [(_plain(63, 24, 48, EPI_BIAS), 1, EINVAL), (_plain(63, 24, 48, EPI_BIAS), 2, EINVAL),
                  (_plain(63, 200, 48, EPI_BIAS), 0, EINVAL), (_plain(63, 200, 48, EPI_BIAS), 3, EINVAL)]


def refusals():
    return conv3_refusals() + ODD_K_REFUSALS


def all_cases():
    """Every case of the table with the test that runs it."""
    return ([('h2', c) for c in h2_cases()] + [('h2p', c) for c in h2p_cases()] + [('h2n', c) for c in h2n_cases()] +
            [('out_h2', c) for c in out_h2_cases()] + [('split', c) for c in split_cases()])


# ---- asking the library: lvae_gemm_h2_choice (include/lvae_hip.h), the function lvae_gemm_f32 switches on
def desc(c, f, present=1):
    """The lvae_gemm_desc of form f of case c as tests/test_gpu_h2_instances.py launches it, operand addresses left out: the optional
    pointers the choice looks at (A1, res, gamma, ws, cnt) are `present` where that launch passes one."""
    from lvae._native import GemmDesc
    d = GemmDesc()
    d.M, d.N, d.K, d.K0, d.K1, d.H, d.W = c.M, c.N, c.K, c.K0, c.K1, c.H, c.W
    d.lda0, d.lda1 = (c.K, 0) if f.a_h2 else (c.lda0, c.lda1)
    d.ldw, d.ldo, d.ldres = c.K, c.ldo, c.ldo
    d.a_mode, d.epi, d.a_gelu, d.out_h2, d.prec, d.cfg, d.a_h2 = c.a_mode, c.epi, c.a_gelu, c.out_h2, 4, f.cfg, f.a_h2
    d.res = d.gamma = present
    d.A1 = present if c.K1 and not f.a_h2 else None
    if c.S > 1:
        d.ksplit, d.ws, d.cnt = c.S, present, (present if f.cnt else None)
    return d


def choice(L, d, cu):
    """lvae_gemm_h2_choice -> (return code, instance in the notation of all_instances(), split-K form); the last two None when rc != 0."""
    import ctypes
    kernel, params, splitk = ctypes.c_int(-1), (ctypes.c_int * 5)(), ctypes.c_int(-1)
    rc = L.lvae_gemm_h2_choice(ctypes.byref(d), cu, ctypes.byref(kernel), params, ctypes.byref(splitk))
    if rc != 0:
        return rc, None, None
    p = list(params)
    inst = {1: ('h2', p[0], p[1], p[2]), 2: ('h2n', p[0], p[1]), 3: ('h2p', p[0], p[1], p[2], bool(p[3]), p[4])}[kernel.value]
    assert not any(p[len(inst) - 1:]), p                   # unused slots are 0
    return rc, inst, splitk.value


SPLITK_NONE, SPLITK_SERIAL, SPLITK_COUNTERS, SPLITK_REDUCE_LAUNCH, SPLITK_DEFERRED = range(5)


def form_splitk(c, f):
    """The split-K form the table says form f of case c runs."""
    if c.S == 1:
        return SPLITK_NONE
    if f.a_h2 or 'serial' in f.name:
        return SPLITK_SERIAL
    return SPLITK_COUNTERS if f.cnt and cnt_in_kernel(c) else SPLITK_REDUCE_LAUNCH
