"""The case table of the fp32 / bf16 / bf16x3 GEMM family (csrc/gemm_f32.hip, compiled three times: plain rows, 2x2 patches, 3x3 taps),
shared by tests/test_gpu_gemm_configs.py (which runs every case under every forced tile configuration on the GPU) and
tests/test_gemm_cases_host.py (which checks, without a GPU, that the table is the one the source declares and that every shape still
straddles the tiles it is listed for).

A kernel instance is (translation unit = a_mode, arithmetic = prec, configuration id).  `cfg = id + 1` of lvae_gemm_desc forces id;
launch_mode then applies the remaps below, so the instance that runs is effective_id(id, prec, split)."""
from collections import namedtuple

A_PLAIN, A_PATCH2, A_CONV3 = 0, 1, 2
A_MODES = (A_PLAIN, A_PATCH2, A_CONV3)
PRECS = (0, 1, 2)                      # fp32 MFMA, bf16, bf16x3
EPI_BIAS, EPI_BIAS_GELU, EPI_GAMMA_RES, EPI_RES = 0, 1, 2, 3
EPIS = (EPI_BIAS, EPI_BIAS_GELU, EPI_GAMMA_RES, EPI_RES)
ST_ROWMAJOR, ST_SHUFFLE, ST_IMAGE = 0, 2, 3
NUM_CONFIGS = 12

Config = namedtuple('Config', 'id name BM BN BK stages')
# the `typedef Cfg<WGM, WGN, TM, TN, NBUF = 2, BK = 32>` lines (BM = 32 WGM TM, BN = 32 WGN TN) in the order of launch_mode's switch;
# id 6 is its `default:` branch
CONFIGS = (
    Config(0, 'CfgA', 128, 128, 32, 2),
    Config(1, 'CfgB', 128, 64, 32, 2),
    Config(2, 'CfgS', 64, 64, 32, 2),
    Config(3, 'CfgL256', 256, 256, 32, 2),
    Config(4, 'CfgL192', 256, 192, 32, 2),
    Config(5, 'CfgL224', 256, 224, 32, 2),
    Config(6, 'CfgL128', 256, 128, 32, 2),
    Config(7, 'CfgD256', 128, 256, 32, 1),
    Config(8, 'CfgD192', 128, 192, 32, 1),
    Config(9, 'CfgC', 128, 32, 32, 2),
    Config(10, 'CfgS64', 64, 64, 64, 2),
    Config(11, 'CfgB64', 128, 64, 64, 2),
)
DEFAULT_ID = 6

# (condition, from id, to id) as launch_mode writes them, in its order
REMAPS = (('prec != 0', 10, 2), ('prec != 0', 11, 1), ('prec == 2', 7, 3), ('split', 10, 2), ('split', 11, 1))


def effective_id(cid, prec, split=False):
    """The configuration that runs when id `cid` is forced (cfg = cid + 1)."""
    for cond, src, dst in REMAPS:
        holds = {'prec != 0': prec != 0, 'prec == 2': prec == 2, 'split': split}[cond]
        if holds and cid == src:
            cid = dst
    return cid


def k_tile(cfg, prec):
    """Depth of one k-tile of the main loop: the configuration's BK under prec 0; gemm_bf16_kernel walks 64, gemm_x3_kernel 32 (both
    exist for the BK = 32 configurations only)."""
    return cfg.BK if prec == 0 else (64 if prec == 1 else 32)


def reachable_instances():
    """Every (a_mode, prec, id) a forced or chosen launch can run.  The bf16x3 instance of CfgD256 is compiled but never launched (it
    spills; launch_mode sends id 7 to 3 under prec 2), and the two 64-deep configurations have no bf16 / bf16x3 kernels."""
    return {(a, p, effective_id(c.id, p)) for a in A_MODES for p in PRECS for c in CONFIGS}


# ------------------------------------------------------------------------------------------------ shapes
Case = namedtuple('Case', 'a_mode M N K K0 K1 lda0 lda1 ldo B H W epi a_gelu')


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
    return s + ('-agelu' if c.a_gelu else '')


def _plain(M, N, K, epi, lda0=None, ldo=None, a_gelu=0, K1=0, lda1=0):
    K0 = K - K1
    return Case(A_PLAIN, M, N, K, K0, K1, lda0 or K0, lda1, ldo or N, 0, 0, 0, epi, a_gelu)


# 549 = 2 * 256 + 37: more than one m-tile with a cut last one for BM = 64, 128 and 256
PLAIN_MS = (1, 63, 549)
RAGGED_M = 549
# 292: a cut last n-tile of at least two for every BN in {32, 64, 128, 192, 224, 256}, 16-byte stores; 290: the same with N % 4 != 0,
# the scalar store path; 24: narrower than every tile
PLAIN_NS = (24, 290, 292)
RAGGED_NS = (290, 292)
NARROW_N = 24
# 8 (fuse_feature_and_z) < every k-tile; 40 and 36 leave a cut last k-tile; 96 / 256 are 3 / 8 tiles of 32; 160 is 5 tiles of 32 and
# 3 tiles of 64 -- added to the issue's list, which has no odd count above one for the 64-deep tiles (96 and 256 give 2 and 4), so
# that those also refill both LDS stages and end on the first.  36 is prec 0 only (prec 1 / 2 need K % 8 == 0).
PLAIN_KS = {0: (8, 36, 40, 96, 160, 256), 1: (8, 40, 96, 160, 256), 2: (8, 40, 96, 160, 256)}


def plain_cases(prec):
    """The ragged M with every N, K and epilogue; the other M with every N and K, the epilogue rotating; one padded lda0; ldo > N on
    the 16-byte path, on the scalar path with N % 4 == 0 (ldo % 4 != 0) and with N % 4 != 0; two A sources with padded leading
    dimensions; GELU on load."""
    out = [_plain(RAGGED_M, N, K, epi) for N in PLAIN_NS for K in PLAIN_KS[prec] for epi in EPIS]
    n = 0
    for M in PLAIN_MS:
        if M == RAGGED_M:
            continue
        for N in PLAIN_NS:
            for K in PLAIN_KS[prec]:
                out.append(_plain(M, N, K, EPIS[n % 4]))
                n += 1
    out += [_plain(RAGGED_M, 292, 96, EPI_GAMMA_RES, lda0=100),
            _plain(RAGGED_M, 292, 40, EPI_RES, ldo=296),
            _plain(RAGGED_M, 292, 96, EPI_GAMMA_RES, ldo=293),
            _plain(RAGGED_M, 290, 96, EPI_BIAS_GELU, ldo=295),
            _plain(RAGGED_M, 292, 40, EPI_BIAS, K1=24, lda0=20, lda1=28),
            _plain(RAGGED_M, 290, 40, EPI_GAMMA_RES, K1=24, lda0=20, lda1=28),
            _plain(RAGGED_M, 292, 96, EPI_BIAS, a_gelu=1)]
    return out


# B = 2, 9 x 17 pixels = 306 rows: the pixel decomposition crosses a 256-row tile inside image 1 and an image boundary inside a tile
GATHER_MAP = (2, 9, 17)


def conv3_cases(prec):
    B, H, W = GATHER_MAP
    out, n = [], 0
    for Cin in (16, 32):
        for N in (24, 100):
            for epi in ((EPI_BIAS, EPI_BIAS_GELU), (EPI_GAMMA_RES, EPI_RES))[n % 2]:
                out.append(Case(A_CONV3, B * H * W, N, 9 * Cin, Cin, 0, Cin, 0, N, B, H, W, epi, 0))
            n += 1
    out.append(Case(A_CONV3, 3, 24, 144, 16, 0, 16, 0, 24, 3, 1, 1, EPI_BIAS, 0))             # 1 x 1 maps: only the centre tap is inside
    out.append(Case(A_CONV3, B * H * W, 100, 288, 32, 0, 32, 0, 100, B, H, W, EPI_BIAS_GELU, 1))
    return out


def patch2_cases(prec):
    B, Ho, Wo = GATHER_MAP
    out, n = [], 0
    for Cin in (8, 40):
        for N in (24, 292):
            for epi in ((EPI_BIAS, EPI_GAMMA_RES), (EPI_BIAS_GELU, EPI_RES))[n % 2]:
                out.append(Case(A_PATCH2, B * Ho * Wo, N, 4 * Cin, Cin, 0, Cin, 0, N, B, Ho, Wo, epi, 0))
            n += 1
    return out


def cases(prec, a_mode):
    return {A_PLAIN: plain_cases, A_PATCH2: patch2_cases, A_CONV3: conv3_cases}[a_mode](prec)


def all_cases():
    return [(p, c) for p in PRECS for a in A_MODES for c in cases(p, a)]


# ------------------------------------------------------------------------------------------------ split-K
SplitCase = namedtuple('SplitCase', 'prec M N K S epi')


def split_cases():
    """M in {63, 549} x N in {64, 292} x S in {2, 4} at K = 256 for each arithmetic, and K = 512 / S = 4 for prec 1 (two 64-deep
    k-tiles per slice).  N = 64 takes the in-kernel reduction when counters are given; N = 292 (N % 32 != 0, several n-tiles) is sent
    to the reduce launch either way."""
    out, n = [], 0
    for prec in PRECS:
        for M in (63, 549):
            for N in (64, 292):
                for S in (2, 4):
                    out.append(SplitCase(prec, M, N, 256, S, EPIS[n % 4]))
                    n += 1
    for M in (63, 549):
        for N in (64, 292):
            out.append(SplitCase(1, M, N, 512, 4, EPIS[n % 4]))
            n += 1
    return out


def split_cnt_entries(M, N):
    """Arrival counters that cover every tile shape (include/lvae_hip.h: lvae_gemm_desc.cnt)."""
    return -(-M // 64) * -(-N // 32)


# ------------------------------------------------------------------------------------------------ store forms
STORE_MAP = (2, 5, 7)                                   # B, H, W: 70 rows, a cut tile for every BM
STORE_KS = (32, 96)                                     # K % 32 == 0, so that prec 4 applies
STORE_PRECS = (0, 2, 4)
# (r, Cout): N = r^2 Cout.  (2, 72): N = 288, 16-byte stores, the group boundaries 72 / 144 / 216 inside the 128- to 256-wide tiles
# (and inside 32-column MFMA blocks); (2, 6): Cout % 4 != 0, the scalar path; (4, 8): 16 groups of 8 columns
SHUFFLE_SHAPES = ((2, 72), (2, 6), (4, 8))
# (r, N) of the final-image store, 3 channels
IMAGE_SHAPES = ((4, 48), (2, 12))
