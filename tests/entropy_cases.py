"""Inputs and plain-torch CPU references for tests/test_gpu_entropy_kernels.py: the lossless output net (lvae_lossless_params_f32,
lvae_lossless_output_f32), the scale indexes (lvae_prior_index_f32 / _sk_) and the rate term (lvae_gaussian_nll_map_f32, both CDF
forms).  Everything here runs on the CPU; tests/test_entropy_cases_host.py checks what the GPU file takes for granted (the constants,
the share of elements left out of the index comparison, that the restated codec is itself lossless on the mean sets used, that the
special points of the grids are where they are said to be), so the GPU assertions never ask more than these references deliver.

Three kinds of comparison:
  bits      values formed by correctly rounded fp32 operations alone (the rounded mean, the symbol, the reconstructed pixel): torch.equal.
  counts    scale indexes: the fp64 count #{i < n-1 : table[i] < s}, leaving out the elements whose exp() value lies within NEAR
            (relative) of a value it is compared with -- the device's expf is not the host's.  An element whose exp() value lies
            well below the bound is NOT left out: s is then the bound itself, exactly, on every machine.
  P space   the rate term: exp(-out) against the fp64 probability, absolute (rate_probability)."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from lvae.models.entropy_coding import log_spaced_table

BIN = torch.tensor(1.0 / 127.5, dtype=torch.float32)                 # GaussianNLLOutputNet.bin_size as the float32 the divisions see
LOG_BIN = torch.tensor(math.log(1.0 / 127.5), dtype=torch.float32)
NEAR, NEAR_CAP = 1e-5, 0.005
BOUND = float(np.float32(0.11))                                      # the models' scale bound as the float the entry points receive
F32_2P3 = float(np.float32(2.3))


def table(n):
    """The models' table shape, 0.11 .. 20 log-spaced, with n entries (the lossless model: 128, the lossy ones: 64)."""
    return torch.tensor([0.11], dtype=torch.float32) if n == 1 else log_spaced_table(0.11, 20.0, n)


def next_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def index_count(pv, tab, bound):
    """pv: fp64 scale before the bound.  Returns (idx, near): the fp64 count for s = max(pv, bound) and the elements to leave out."""
    t, b = tab.double(), float(bound)
    s = pv.clamp(min=b).contiguous()
    idx = torch.searchsorted(t[:-1].contiguous(), s, right=False)             # the entries strictly below s
    cmp = torch.sort(torch.cat([t, torch.tensor([b], dtype=torch.float64)])).values
    k = torch.searchsorted(cmp, pv.contiguous()).clamp(max=cmp.numel() - 1)   # the two values pv lies between
    below, above = cmp[(k - 1).clamp(min=0)], cmp[k]
    near = (((pv / below - 1).abs() < NEAR) | ((pv / above - 1).abs() < NEAR)) & (pv >= b * (1 - NEAR))
    return idx, near


# ------------------------------------------------------------------------------------------------ A. lossless output net
LosslessRef = namedtuple('LosslessRef', 'pm idx near sym')
LOSSLESS_SHAPES = ((1, 1, 1), (2, 3, 5), (3, 7, 13), (2, 33, 31), (1, 1, 257))
LOSSLESS_NS = (1, 2, 3, 255, 256)
TIE_KS = tuple(range(-300, 601))


def ref_lossless_params(raw, im, tab, bound):
    """raw: (B, HW, 6) float32, [pixel][mean r g b, log-scale r g b]; im: (B, 3, HW) in [0, 1] or None.  The operation order of
    GaussianNLLOutputNet._preapre_codec and CompressAI's build_indexes, in fp32; rasters come back as (B, 3, HW)."""
    r = raw[..., :3].permute(0, 2, 1).contiguous()
    l = raw[..., 3:].permute(0, 2, 1).contiguous()
    pm = torch.round(r * 127.5 + 127.5) / 127.5 - 1
    pm = pm / BIN
    ls = l - LOG_BIN
    idx, near = index_count(torch.exp(ls.double()), tab, bound)
    sym = None
    if im is not None:
        x = ((im - 0.5) * 2) / BIN
        sym = torch.round(x - pm).to(torch.int32)
    return LosslessRef(pm, idx, near, sym)


def ref_lossless_output(sym, pm):
    x = sym.to(torch.float32) + pm
    x = (x * BIN).clamp(-1.0, 1.0)
    return x * 0.5 + 0.5


def lossless_inputs(B, H, W):
    """Means in [-1.5, 1.5], log-scales that put s below, inside and above the table, u8 pixels; no value repeated where a swapped
    column, pixel or image index would need it (test_entropy_cases_host.py)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
    HW = H * W
    raw = torch.empty(B, HW, 6)
    raw[..., :3] = torch.rand(B, HW, 3, generator=g) * 3 - 1.5
    raw[..., 3:] = torch.rand(B, HW, 3, generator=g) * 7 - 8
    im = torch.randint(0, 256, (B, 3, HW), generator=g).float() / 255
    return raw, im


def tie_means():
    """r = (k + 0.5) / 127.5 - 1: r * 127.5 + 127.5 lands on k + 0.5, where round-half-even decides."""
    return torch.tensor([(k + 0.5) / 127.5 - 1 for k in TIE_KS], dtype=torch.float64).float()


def tie_inputs():
    """One row of len(TIE_KS) pixels: every tie as the mean of every channel (each channel starts elsewhere in the list)."""
    g = torch.Generator().manual_seed(77)
    t = tie_means()
    n = t.numel()
    raw = torch.empty(1, n, 6)
    for c in range(3):
        raw[0, :, c] = torch.roll(t, 300 * c)
    raw[..., 3:] = torch.rand(1, n, 3, generator=g) * 7 - 8
    im = torch.randint(0, 256, (1, 3, n), generator=g).float() / 255
    return raw, im


def domain_means():
    """The mean sets of the whole-domain round trip, one per channel: uniform in [-3, 3], the ties, magnitudes up to 1e4."""
    g = torch.Generator().manual_seed(5)
    n = len(TIE_KS)
    uni = torch.rand(n, generator=g) * 6 - 3
    mag = 10 ** (torch.rand(n, generator=g, dtype=torch.float64) * 6 - 2)
    mag = (mag * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()
    mag[:4] = torch.tensor([1e4, -1e4, 9999.99, -9999.99])
    return uni, tie_means(), mag.clamp(-1e4, 1e4)


def domain_inputs():
    """An image of 256 rows, row v holding the u8 value v / 255 in every column; column w has the means domain_means()[c][w]."""
    means = domain_means()
    W = means[0].numel()
    raw = torch.empty(1, 256, W, 6)
    for c in range(3):
        raw[0, :, :, c] = means[c][None, :]
        raw[0, :, :, 3 + c] = -6.0 + c
    v = torch.arange(256, dtype=torch.float32)
    im = (v / 255)[None, None, :, None].expand(1, 3, 256, W).contiguous()
    return raw.view(1, 256 * W, 6), im.view(1, 3, 256 * W), v[None, None, :, None].expand(1, 3, 256, W).reshape(1, 3, 256 * W)


def output_edge_inputs():
    """sym + pm on, beside and far beyond +-127.5, and inside; expected output 0.0 / 1.0 exactly beyond."""
    tot = torch.tensor([127.5, -127.5, 128.0, -128.0, 127.0, -127.0, 1e6, -1e6, 127.49999, -127.49999, 0.0, 0.5, -0.5, 3e9, -3e9, 64.25],
                       dtype=torch.float32)
    sym = torch.tensor([100, -100, 1, -1, 127, -127, 1000000, -1000000, 0, 0, 0, 7, -7, 2147483647, -2147483648, 64], dtype=torch.int32)
    pm = tot - sym.float()
    return sym, pm


# ------------------------------------------------------------------------------------------------ B. scale indexes
INDEX_NS = (2, 3, 64, 128, 255, 256)
INDEX_SHAPES = ((2, 65, 17), (2, 129, 33), (2, 65, 33), (2, 129, 17))        # (B, HW, z): ragged 64-pixel tiles and 16-channel chunks
CUT = np.float32(17.7)                                                       # lv + 2.3f crosses 20 here
BOUND_LVS = (-100.0, -90.0, -30.0, 100.0)                                    # exp(-2.3) three times (below every table), then inf


def cut_points():
    pts, lo, hi = [CUT], CUT, CUT
    for _ in range(3):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        pts += [lo, hi]
    return torch.tensor(np.array(sorted(pts), dtype=np.float32))


def index_inputs(B, HW, z):
    """prm (B*HW, 2z): means, then log-scales from a grid over [-100, 100] (half of it inside [-6, 6], where the table is), with the
    points around the softplus cut-over and the ones where expf underflows; shuffled, so that no two positions are alike."""
    g = torch.Generator().manual_seed(100 * HW + z)
    n = B * HW * z
    special = torch.cat([cut_points(), torch.tensor([-100.0, -97.0, -95.0, -90.0, -89.6, 100.0, 99.0, 17.0, 18.0])])
    wide = torch.linspace(-100, 100, n // 2)
    dense = torch.linspace(-6, 6, n - n // 2 - special.numel())
    lv = torch.cat([special, wide, dense])[torch.randperm(n, generator=g)].view(B * HW, z)
    mean = torch.randn(B * HW, z, generator=g) * 3
    return torch.cat([mean, lv], 1).contiguous()


def index_sk_inputs(B, HW, z, S):
    """(ws, bias, prm): S partial-sum planes and a bias whose sum in slice order, prm, lands on index_inputs' grid up to rounding."""
    g = torch.Generator().manual_seed(31)
    target = index_inputs(B, HW, z)
    ws = torch.randn(S, B * HW, 2 * z, generator=g)
    bias = torch.randn(2 * z, generator=g)
    rest = ws[1]
    for sl in range(2, S):
        rest = rest + ws[sl]
    ws[0] = target - (rest + bias)
    prm = ws[0]
    for sl in range(1, S):
        prm = prm + ws[sl]
    return ws, bias, (prm + bias).contiguous()


def ref_prior_index(prm, tab, bound, B, HW, z):
    """(pm, idx, near): pm the mean columns themselves, idx / near as NCHW rasters (B, z, HW).  lv + 2.3f is one correctly rounded fp32
    operation and decides the softplus branch, so it is formed in fp32; the transcendental part is fp64."""
    xs = prm[:, z:] + torch.tensor(2.3, dtype=torch.float32)
    x64 = xs.double()
    sp = torch.where(xs > 20.0, x64, torch.log1p(torch.exp(x64)))
    idx, near = index_count(torch.exp(sp - F32_2P3), tab, bound)
    ras = lambda t: t.view(B, HW, z).permute(0, 2, 1).contiguous()
    return prm[:, :z].contiguous(), ras(idx), ras(near)


# ------------------------------------------------------------------------------------------------ C. rate term
RATE_HW, RATE_Z, RATE_B = 2001, 81, 2
RATE_TOL_FACTOR = 4.0                 # device expf / log1pf / erfcf / lvae_erff: a few ulp each, where the host libm is below one
RATE_CAP = np.float32(-math.log(float(np.float32(1e-9))))                    # -logf(1e-9f): what max(P, 1e-9) turns into


def rate_inputs(step=1):
    """lv in [-30, 30] along the pixels, sym = -40 .. 40 along the channels; the second image has both reversed.  step > 1: every
    step-th pixel.  Returns prm (B*HW, 2z) with the log-scale columns filled, sym (B, z, HW) int32."""
    lv = torch.linspace(-30, 30, RATE_HW)[::step]
    hw = lv.numel()
    sy = torch.arange(-40, 41, dtype=torch.int32)
    lvs = torch.stack([lv, lv.flip(0)])                                        # (B, HW)
    sym = torch.stack([sy, sy.flip(0)])[:, :, None].expand(RATE_B, RATE_Z, hw).contiguous()
    g = torch.Generator().manual_seed(3)
    prm = torch.randn(RATE_B * hw, 2 * RATE_Z, generator=g)
    prm[:, RATE_Z:] = lvs.reshape(-1, 1)
    return prm.contiguous(), sym


def rate_probability(prm, sym, bound, cdf_form, dtype):
    """P of csrc/rate_terms.h gaussian_logp, max(., 1e-9) included, as a (B, z, HW) raster in `dtype`."""
    B, z, hw = sym.shape
    lv = prm[:, z:].to(dtype).view(B, hw, z).permute(0, 2, 1)
    s = torch.exp(F.softplus(lv + 2.3, beta=1, threshold=20) - 2.3).clamp(min=bound)
    v = sym.to(dtype).abs()
    a, d = (0.5 - v) / s, (-0.5 - v) / s
    if cdf_form == 0:
        up, lo = 0.5 * (1 + torch.erf(a * 0.70710678118654752440)), 0.5 * (1 + torch.erf(d * 0.70710678118654752440))
    else:
        up, lo = 0.5 * torch.erfc(-0.70710678118654752440 * a), 0.5 * torch.erfc(-0.70710678118654752440 * d)
    return (up - lo).clamp(min=1e-9)


def rate_reference(cdf_form, step=1):
    """(prm, sym, P64, err32): err32 is the largest |P32 - P64| of the same formula in fp32 torch on this grid -- the yardstick the
    kernel is allowed RATE_TOL_FACTOR times of."""
    prm, sym = rate_inputs(step)
    p64 = rate_probability(prm, sym, BOUND, cdf_form, torch.float64)
    p32 = rate_probability(prm, sym, BOUND, cdf_form, torch.float32)
    return prm, sym, p64, float((p32.double() - p64).abs().max())
