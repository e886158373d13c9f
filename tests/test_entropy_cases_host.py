"""not-gpu: what tests/test_gpu_entropy_kernels.py takes for granted about tests/entropy_cases.py -- the constants against the kernels'
text and against torch's own scalar arithmetic, the share of elements the index comparisons leave out (seeded inputs, so the cap is met
by the reference alone), the restated lossless codec being lossless on exactly the mean sets the GPU test uses, the special points of
the grids being where they are said to be -- and the -22 argument checks of the two lossless entry points, which precede any HIP call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import entropy_cases as ec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lossy-vae_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ constants
def test_constants_are_torchs_and_the_kernels():
    g = torch.Generator().manual_seed(0)
    t = torch.randn(100000, generator=g) * 50
    # a float32 tensor divided by / reduced by the Python floats of the reference is the fp32 operation with the float32 constant
    assert torch.equal(t / ec.BIN, t / (1 / 127.5))
    assert torch.equal(t - ec.LOG_BIN, t - math.log(1 / 127.5))
    src = _read('pointwise.hip')
    body = src[src.index('void lossless_params_kernel('):src.index('void lossless_output_kernel(')]
    assert 'const float bin = (float)(1.0 / 127.5);' in body and 'm = m / bin;' in body and 'x = x / bin;' in body
    (lit,) = re.findall(r'const float ls = r\[3 \+ c\] - \(float\)\((-[0-9.]+)\);', body)
    assert np.float32(float(lit)) == np.float32(ec.LOG_BIN.item()) == np.float32(math.log(1 / 127.5))
    out = src[src.index('void lossless_output_kernel('):src.index('// ----', src.index('void lossless_output_kernel('))]
    assert 'x = x * (float)(1.0 / 127.5);' in out and np.float32(1.0 / 127.5) == np.float32(ec.BIN.item())
    assert 'if (table[mid] < s) lo = mid + 1; else hi = mid;' in body                      # the comparison the boundary cases pin
    assert 'if (tab[mid] < sc) lo = mid + 1; else hi = mid;' in src
    rate = _read('rate_terms.h')
    assert 'const float P = fmaxf(up - lo, 1e-9f);' in rate and 'const float xs = lv + 2.3f;' in rate
    assert ec.BOUND == float(np.float32(0.11)) and ec.RATE_CAP == np.float32(20.723266) and ec.RATE_CAP.dtype == np.float32
    from lvae import _native
    assert (_native.STATUS_NONFINITE_PRIOR, _native.STATUS_NONFINITE_IMAGE) == (2, 8)
    hdr = _read(os.path.join('..', '..', 'include', 'lvae_hip.h'))
    assert 'LVAE_STATUS_NONFINITE_PRIOR = 2,' in hdr and re.search(r'LVAE_STATUS_NONFINITE_IMAGE = 8\b', hdr)


def test_device_math_names_a_test_that_exists():
    (cited,) = re.findall(r'checked against fp64 erf on a dense grid: (tests/\S+?)::(\w+)', _read('device_math.h'))
    path = os.path.join(os.path.dirname(CSRC), '..', cited[0])
    with open(path) as f:
        assert re.search(rf'^def {cited[1]}\(', f.read(), re.M), cited


@pytest.mark.parametrize('n', sorted(set(ec.LOSSLESS_NS + ec.INDEX_NS)))
def test_tables_carry_the_boundary_cases(n):
    """bound = table[j] with a scale far below gives s == table[j]; its fp32 successor lies below table[j + 1]."""
    t = ec.table(n)
    assert t.dtype == torch.float32 and t.numel() == n
    assert bool((t[1:] > t[:-1]).all())
    up = torch.tensor([ec.next_up(v) for v in t.tolist()], dtype=torch.float32)
    assert bool((up > t).all()) and bool((up[:-1] < t[1:]).all())
    lo = float(t[0])
    assert math.exp(-2.3) * (1 + 1e-3) < lo                    # B: exp(softplus(lv + 2.3) - 2.3) for lv <= -30
    assert math.exp(-80 - math.log(1 / 127.5)) < 1e-30 < lo    # A: exp(l - log bin) for l = -80
    assert 1e30 < math.exp(80 - math.log(1 / 127.5)) < 3e38 and float(t[-1]) <= 20.001       # and l = 80: finite, above every entry


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize('B,H,W', ec.LOSSLESS_SHAPES)
def test_lossless_inputs(B, H, W):
    HW, total = H * W, B * 3 * H * W
    assert total % 256 != 0 and HW % 2 == 1
    raw, im = ec.lossless_inputs(B, H, W)
    assert raw.shape == (B, HW, 6) and im.shape == (B, 3, HW)
    for a in range(6):                                          # no two columns alike at any pixel, no two images, no two neighbours
        for b in range(a + 1, 6):
            assert bool((raw[..., a] != raw[..., b]).all())
    for a in range(B):
        for b in range(a + 1, B):
            assert bool((raw[a] != raw[b]).all())
    assert bool((raw[:, 1:] != raw[:, :-1]).all())
    ref = ec.ref_lossless_params(raw, im, ec.table(128), ec.BOUND)
    assert float(ref.near.float().mean()) <= ec.NEAR_CAP
    assert ref.sym.dtype == torch.int32 and ref.pm.shape == ref.idx.shape == ref.sym.shape == (B, 3, HW)
    if total > 1000:                                            # the scales meet the bound, the table and its top
        assert {0, 127} < set(ref.idx.unique().tolist()) and len(ref.idx.unique()) > 64
    # the restated codec gives the image back
    out = ec.ref_lossless_output(ref.sym, ref.pm)
    assert torch.equal(torch.round(out * 255), torch.round(im * 255))


def test_ties_are_ties():
    """Most k + 0.5 survive the fp32 detour through r exactly; the rounded mean there is the even neighbour."""
    r = ec.tie_means()
    m = r * 127.5 + 127.5
    half = torch.tensor([k + 0.5 for k in ec.TIE_KS])
    hit = m == half
    assert int(hit.sum()) >= 600 and len(ec.TIE_KS) == 901
    ks = torch.tensor(ec.TIE_KS)
    for parity in (0, 1):
        for sign in (-1, 1):
            assert int((hit & (ks % 2 == parity) & (torch.sign(half) == sign)).sum()) >= 50
    rounded = torch.round(m)[hit]
    assert bool((rounded % 2 == 0).all()) and bool(((rounded - half[hit]).abs() == 0.5).all())
    raw, im = ec.tie_inputs()
    assert (3 * raw.shape[1]) % 256 != 0 and raw.shape[1] % 2 == 1
    for c in range(3):
        assert sorted(raw[0, :, c].tolist()) == sorted(r.tolist())
    assert bool((raw[0, :, 0] != raw[0, :, 1]).all()) and bool((raw[0, :, 1] != raw[0, :, 2]).all())
    assert float(ec.ref_lossless_params(raw, im, ec.table(128), ec.BOUND).near.float().mean()) <= ec.NEAR_CAP


def test_the_restated_codec_is_lossless_on_the_whole_domain():
    uni, tie, mag = ec.domain_means()
    assert uni.numel() == tie.numel() == mag.numel() == 901
    assert float(uni.abs().max()) <= 3 and float(mag.abs().max()) == 1e4 and float(mag.abs().min()) < 0.02
    assert int((mag.abs() > 1000).sum()) > 100 and {-1.0, 1.0} == set(torch.sign(mag).tolist())
    raw, im, v = ec.domain_inputs()
    assert raw.shape == (1, 256 * 901, 6) and im.shape == v.shape == (1, 3, 256 * 901)
    assert torch.equal(torch.round(im * 255), v) and sorted(v[0, 1].unique().tolist()) == list(range(256))
    ref = ec.ref_lossless_params(raw, im, ec.table(128), ec.BOUND)
    out = ec.ref_lossless_output(ref.sym, ref.pm)
    assert torch.equal(torch.round(out * 255), v)
    assert int(ref.sym.abs().max()) > 1_000_000                                  # symbols far outside any CDF: the kernels do not care


def test_output_edges():
    sym, pm = ec.output_edge_inputs()
    tot = sym.float() + pm
    out = ec.ref_lossless_output(sym, pm)
    assert bool((out[tot >= 127.5] == 1.0).all()) and bool((out[tot <= -127.5] == 0.0).all())
    inside = tot.abs() < 127.4
    assert bool(((out[inside] > 0) & (out[inside] < 1)).all())
    assert int((tot.abs() > 127.5).sum()) >= 6 and int((tot.abs() == 127.5).sum()) == 2 and int(inside.sum()) >= 4


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize('B,HW,z', ec.INDEX_SHAPES)
def test_index_inputs(B, HW, z):
    assert HW % 64 not in (0, 63) and HW > 64 and z % 16 != 0 and z > 16 and B == 2
    prm = ec.index_inputs(B, HW, z)
    assert prm.shape == (B * HW, 2 * z)
    lv = prm[:, z:]
    xs = lv + torch.tensor(2.3, dtype=torch.float32)
    at_cut = (lv - float(ec.CUT)).abs() < 1e-5
    assert int(at_cut.sum()) == 7 and bool((xs[at_cut] > 20).any()) and bool((xs[at_cut] <= 20).any())
    e = torch.exp(xs)
    assert bool((e < 1.1754944e-38).any()) and bool((xs < -87.4).any()) and bool(torch.isinf(torch.exp(xs[xs > 20] - 2.3)).any())
    assert float(lv.min()) == -100 and float(lv.max()) == 100 and int(((lv > -6) & (lv < 6)).sum()) > lv.numel() // 2
    for n in ec.INDEX_NS:
        t = ec.table(n)
        _, idx, near = ec.ref_prior_index(prm, t, float(t[0]), B, HW, z)
        assert float(near.float().mean()) <= ec.NEAR_CAP, n
        assert set(idx.unique().tolist()) == set(range(n)), n                                   # every index is asked for
        assert int((idx == 0).sum()) > idx.numel() // 5                                         # the bound holds a good share of them


def test_index_sk_inputs():
    B, HW, z, S = 2, 129, 33, 3
    ws, bias, prm = ec.index_sk_inputs(B, HW, z, S)
    assert ws.shape == (S, B * HW, 2 * z) and torch.equal(prm, ((ws[0] + ws[1]) + ws[2]) + bias)
    assert float((prm - ec.index_inputs(B, HW, z)).abs().max()) < 1e-4 and float(prm[:, z:].max()) > 99 and float(prm[:, z:].min()) < -99
    t = ec.table(64)
    _, idx, near = ec.ref_prior_index(prm, t, float(t[0]), B, HW, z)
    assert float(near.float().mean()) <= ec.NEAR_CAP and set(idx.unique().tolist()) == set(range(64))


# ------------------------------------------------------------------------------------------------ C
def test_rate_grid():
    prm, sym = ec.rate_inputs()
    B, z, HW = ec.RATE_B, ec.RATE_Z, ec.RATE_HW
    assert prm.shape == (B * HW, 2 * z) and sym.shape == (B, z, HW) and sym.dtype == torch.int32 and B * z * HW <= 350_000
    lv = prm[:, z:].view(B, HW, z)
    assert torch.equal(lv[0], lv[1].flip(0)) and torch.equal(sym[0], sym[1].flip(0)) and not torch.equal(sym[0], sym[1])
    assert float(lv.min()) == -30 and float(lv.max()) == 30 and sym[0, :, 0].tolist() == list(range(-40, 41))
    assert bool((lv[0] == lv[0][:, :1]).all())
    for form in (0, 1):
        _, _, p64, err32 = ec.rate_reference(form)
        assert p64.dtype == torch.float64 and 2e-8 < err32 < 5e-7, err32                       # fp32's own error: a few 2^-24
        # P reaches 1 and the floor; the floor is what |sym| = 40 gets at the bound
        assert float(p64.max()) > 0.999 and float(p64.min()) == 1e-9
        assert bool((p64[0, 0, :300] == 1e-9).all()) and bool((p64[0, -1, :300] == 1e-9).all())
        assert 0.05 < float(((p64 > 1e-6) & (p64 < 1 - 1e-6)).float().mean())
    sub, ssym = ec.rate_inputs(5)
    assert ssym.shape == (B, z, 401) and sub.shape == (B * 401, 2 * z)


# ------------------------------------------------------------------------------------------------ -22 before any HIP call
def test_lossless_argument_checks():
    """No pointer here is real: reaching a launch would not go unnoticed."""
    from lvae import _native
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    P = ctypes.addressof(buf)

    def params(**kw):
        a = dict(raw=P, im=P, pm=P, idx=P, sym=P, table=P, n=128, bound=0.11, B=1, H=2, W=2, status=None)
        a.update(kw)
        return L.lvae_lossless_params_f32(a['raw'], a['im'], a['pm'], a['idx'], a['sym'], a['table'], a['n'], a['bound'], a['B'], a['H'], a['W'],
                                          a['status'], None)

    for null in ('raw', 'pm', 'idx', 'table'):
        assert params(**{null: None}) == -22, null
        assert params(**{null: None}, im=None, sym=None) == -22, null
    assert params(n=0) == -22 and params(n=257) == -22 and params(n=-1) == -22
    assert params(B=0) == -22 and params(H=0) == -22 and params(W=0) == -22 and params(B=-1) == -22
    assert params(sym=None) == -22                                                  # an image to code, nowhere to put the symbols

    def output(**kw):
        a = dict(sym=P, pm=P, out=P, n=4, status=None)
        a.update(kw)
        return L.lvae_lossless_output_f32(a['sym'], a['pm'], a['out'], a['n'], a['status'], None)

    for null in ('sym', 'pm', 'out'):
        assert output(**{null: None}) == -22, null
    assert output(n=0) == -22 and output(n=-1) == -22
