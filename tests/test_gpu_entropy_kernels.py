"""-m gpu: the kernels that decide what the entropy coder sees, each called through the C ABI against the plain CPU references of
tests/entropy_cases.py -- the lossless output net (csrc/pointwise.hip lossless_params_kernel / lossless_output_kernel), the scale
indexes (prior_index_kernel, plain and behind a deferred split-K reduce) and the rate term in both CDF forms (csrc/rate_terms.h
gaussian_logp, through lvae_gaussian_nll_map_f32 and lvae_gaussian_nll_f32).

What is compared how (entropy_cases.py has the reasons; tests/test_entropy_cases_host.py checks, without a GPU, that the references
meet every precondition used here):
  * rounded means, symbols, reconstructed pixels: correctly rounded fp32 operations with contraction off -> torch.equal;
  * scale indexes: the fp64 count away from the table entries, and EXACTLY on them with bound = table[j], where no exp() takes part;
  * the rate term: exp(-out) against the fp64 probability, absolute, within RATE_TOL_FACTOR times the error of the same formula in fp32
    torch -- measured in the test, printed in the assertion message."""
import ctypes

import numpy as np
import pytest
import torch

import entropy_cases as ec

pytestmark = pytest.mark.gpu

SENTINEL = -123456789


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _params(L, raw, im, tab, bound, B, H, W, status=None, sym_fill=SENTINEL):
    """One lvae_lossless_params_f32 call on CPU inputs; returns (pm, idx, sym) on the CPU, sym pre-filled with sym_fill."""
    n = B * 3 * H * W
    raw_d, im_d, tab_d = raw.cuda(), None if im is None else im.cuda(), tab.cuda()
    pm = torch.full((B, 3, H * W), float('nan'), device='cuda')
    idx = torch.full((B, 3, H * W), 255, dtype=torch.uint8, device='cuda')
    sym = torch.full((B, 3, H * W), sym_fill, dtype=torch.int32, device='cuda')
    assert raw_d.numel() == 2 * n and raw_d.is_contiguous() and (im_d is None or (im_d.numel() == n and im_d.is_contiguous()))
    rc = L.lvae_lossless_params_f32(raw_d.data_ptr(), _ptr(im_d), pm.data_ptr(), idx.data_ptr(), sym.data_ptr(), tab_d.data_ptr(), tab.numel(),
                                    float(bound), B, H, W, _ptr(status), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return pm.cpu(), idx.cpu(), sym.cpu()


def _output(L, sym, pm, status=None):
    n = sym.numel()
    sym_d, pm_d = sym.contiguous().cuda(), pm.contiguous().cuda()
    out = torch.full((n + 64,), float('nan'), device='cuda')                # a guard band behind the n elements
    rc = L.lvae_lossless_output_f32(sym_d.data_ptr(), pm_d.data_ptr(), out.data_ptr(), n, _ptr(status), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    return out[:n].cpu().view(sym.shape)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


# ------------------------------------------------------------------------------------------------ A. lossless output net
def _check_params(L, raw, im, B, H, W, n_scales=128):
    tab = ec.table(n_scales)
    ref = ec.ref_lossless_params(raw, im, tab, ec.BOUND)
    flag = _flag()
    pm, idx, sym = _params(L, raw, im, tab, ec.BOUND, B, H, W, status=flag)
    assert int(flag) == 0
    assert torch.equal(pm, ref.pm), int((pm != ref.pm).sum())
    assert torch.equal(sym, ref.sym), int((sym != ref.sym).sum())
    assert float(ref.near.float().mean()) <= ec.NEAR_CAP
    bad = (idx.long() != ref.idx) & ~ref.near
    assert not bool(bad.any()), (int(bad.sum()), idx[bad][:8].tolist(), ref.idx[bad][:8].tolist())
    # the decode call: no image, the symbol buffer is not its to touch
    pm2, idx2, sym2 = _params(L, raw, None, tab, ec.BOUND, B, H, W, status=flag)
    assert int(flag) == 0 and torch.equal(pm2, pm) and torch.equal(idx2, idx) and bool((sym2 == SENTINEL).all())
    # and the way back
    out = _output(L, sym, pm, status=flag)
    assert int(flag) == 0 and torch.equal(out, ec.ref_lossless_output(ref.sym, ref.pm))
    assert torch.equal(torch.round(out * 255), torch.round(im * 255))
    return pm, idx, sym


@pytest.mark.parametrize('B,H,W', ec.LOSSLESS_SHAPES)
def test_lossless_params_and_output(L, B, H, W):
    """Ragged 256-thread launches with every column, pixel and image distinct: the [pixel][6] -> NCHW indexing, the mean's rounding,
    the symbol, the index, the decode call against the encode call, and the reconstruction."""
    raw, im = ec.lossless_inputs(B, H, W)
    _check_params(L, raw, im, B, H, W)


def test_lossless_mean_ties(L):
    """r = (k + 0.5) / 127.5 - 1 for k = -300 .. 600: r * 127.5 + 127.5 is k + 0.5 for most of them, and rintf must go to the even side."""
    raw, im = ec.tie_inputs()
    pm, _, _ = _check_params(L, raw, im, 1, 1, raw.shape[1])
    m = (raw[0, :, 0] * 127.5 + 127.5)
    tie = (m - torch.floor(m)) == 0.5
    assert int(tie.sum()) >= 600
    want = (2 * torch.round(m[tie] / 2) / 127.5 - 1) / ec.BIN                # the even neighbour, spelled out
    assert torch.equal(pm[0, 0][tie], want)


@pytest.mark.parametrize('n_scales', (128,) + ec.LOSSLESS_NS)
def test_lossless_index_boundaries(L, n_scales):
    """bound = table[j] with a log-scale of -80: s == table[j] without trusting expf, so idx == j (strict <); with the next float up,
    j + 1 (capped at n - 1); a log-scale of +80 gives n - 1.  Every j of the table, one launch each, one synchronisation."""
    tab = ec.table(n_scales)
    tab_d = tab.cuda()
    raw = torch.zeros(1, 2, 6)
    raw[0, :, :3] = torch.tensor([[0.25, -0.5, 0.75], [-0.125, 0.5, -0.75]])
    raw[0, 0, 3:], raw[0, 1, 3:] = -80.0, 80.0
    raw_d = raw.cuda()
    n = n_scales
    pm = torch.full((n, 2, 6), float('nan'), device='cuda')
    idx = torch.full((n, 2, 6), 255 if n < 256 else 7, dtype=torch.uint8, device='cuda')
    flag = _flag()
    for j in range(n):
        for up in (0, 1):
            bound = ec.next_up(tab[j]) if up else float(tab[j])
            assert L.lvae_lossless_params_f32(raw_d.data_ptr(), None, pm[j, up].data_ptr(), idx[j, up].data_ptr(), None, tab_d.data_ptr(), n, bound,
                                              1, 1, 2, flag.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert int(flag) == 0
    idx = idx.cpu().long().view(n, 2, 3, 2)                                  # [j][up][channel][pixel]
    j = torch.arange(n)
    for up in (0, 1):
        want = (j + up).clamp(max=n - 1)
        for c in range(3):
            assert torch.equal(idx[:, up, c, 0], want), (up, c)
            assert bool((idx[:, up, c, 1] == n - 1).all())
    assert torch.equal(pm.cpu()[0, 0].view(3, 2), ec.ref_lossless_params(raw, None, tab, ec.BOUND).pm[0])


def test_lossless_whole_domain_round_trip(L):
    """Every u8 value under every mean of three mean sets (uniform in [-3, 3], the ties, magnitudes up to 1e4) comes back: the property
    the model exists for.  256 x 901 pixels x 3 channels: the mean sets the host test shows the fp32 restatement to be lossless on."""
    raw, im, v = ec.domain_inputs()
    W = raw.shape[1] // 256
    tab = ec.table(128)
    flag = _flag()
    pm, idx, sym = _params(L, raw, im, tab, ec.BOUND, 1, 256, W, status=flag)
    out = _output(L, sym, pm, status=flag)
    assert int(flag) == 0
    got = torch.round(out * 255)
    assert torch.equal(got, v), (int((got != v).sum()), raw[0, :, :3].t().reshape(1, 3, -1)[got != v][:8].tolist())
    ref = ec.ref_lossless_params(raw, im, tab, ec.BOUND)
    assert torch.equal(pm, ref.pm) and torch.equal(sym, ref.sym) and torch.equal(out, ec.ref_lossless_output(ref.sym, ref.pm))


@pytest.mark.parametrize('n', (1, 255, 256, 257))
def test_lossless_output_sizes_and_clamp(L, n):
    """One thread, one short of a workgroup, a whole one, one more; values on, beside and beyond +-127.5 in every one of them."""
    esym, epm = ec.output_edge_inputs()
    g = torch.Generator().manual_seed(n)
    sym = torch.randint(-300, 301, (n,), generator=g, dtype=torch.int32)
    pm = (torch.rand(n, generator=g) * 2 - 1) * 127.5
    k = min(n, esym.numel())
    sym[n - k:], pm[n - k:] = esym[:k], epm[:k]                             # the edges sit at the END: the ragged tail of the launch
    flag = _flag()
    out = _output(L, sym, pm, status=flag)
    assert int(flag) == 0
    assert torch.equal(out, ec.ref_lossless_output(sym, pm))
    tot = sym.float() + pm
    assert bool((out[tot > 127.5] == 1.0).all()) and bool((out[tot < -127.5] == 0.0).all())
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert torch.equal(_output(L, sym, pm, status=None), out)


def test_lossless_status_bits(L):
    from lvae import _native
    PRIOR, IMAGE = _native.STATUS_NONFINITE_PRIOR, _native.STATUS_NONFINITE_IMAGE
    B, H, W = 2, 3, 5
    raw, im = ec.lossless_inputs(B, H, W)
    tab = ec.table(128)
    clean = _params(L, raw, im, tab, ec.BOUND, B, H, W, status=None)                 # status = NULL is accepted
    for col in range(6):                                                              # a mean or a log-scale column of any channel
        for bad in (float('nan'), float('inf'), float('-inf')):
            r = raw.clone()
            r[1, 7, col] = bad
            flag = _flag()
            pm, idx, sym = _params(L, r, im, tab, ec.BOUND, B, H, W, status=flag)
            assert int(flag) == PRIOR, (col, bad, int(flag))
            keep = torch.ones(B, 3, H * W, dtype=torch.bool)
            keep[1, col % 3, 7] = False                                               # every other element is what it was
            assert torch.equal(pm[keep], clean[0][keep]) and torch.equal(idx[keep], clean[1][keep]) and torch.equal(sym[keep], clean[2][keep])
            _params(L, r, im, tab, ec.BOUND, B, H, W, status=None)
    flag = _flag()
    got = _params(L, raw, im, tab, ec.BOUND, B, H, W, status=flag)
    assert int(flag) == 0 and all(torch.equal(a, b) for a, b in zip(got, clean))
    # the output kernel: a non-finite sym + pm, nothing else
    pm, _, sym = clean
    for bad in (float('nan'), float('inf'), float('-inf')):
        p = pm.clone()
        p[0, 2, 11] = bad
        flag = _flag()
        out = _output(L, sym, p, status=flag)
        assert int(flag) == IMAGE, (bad, int(flag))
        keep = torch.ones_like(p, dtype=torch.bool)
        keep[0, 2, 11] = False
        assert torch.equal(out[keep], ec.ref_lossless_output(sym, pm)[keep])
        _output(L, sym, p, status=None)
    flag = _flag()
    _output(L, sym, pm, status=flag)
    assert int(flag) == 0


# ------------------------------------------------------------------------------------------------ B. scale indexes
def _prior_index(L, prm, tab, bound, B, HW, z, status=None):
    prm_d, tab_d = prm.cuda(), tab.cuda()
    pm = torch.full((B * HW, z), float('nan'), device='cuda')
    idx = torch.full((B, z, HW), 255 if tab.numel() < 256 else 7, dtype=torch.uint8, device='cuda')
    rc = L.lvae_prior_index_f32(prm_d.data_ptr(), pm.data_ptr(), idx.data_ptr(), tab_d.data_ptr(), tab.numel(), float(bound), B, HW, z, _ptr(status), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return pm.cpu(), idx.cpu()


@pytest.mark.parametrize('n_scales', ec.INDEX_NS)
@pytest.mark.parametrize('B,HW,z', ec.INDEX_SHAPES)
def test_prior_index_grid(L, B, HW, z, n_scales):
    """Log-scales over [-100, 100] -- both sides of the softplus cut-over, expf underflowing, expf overflowing -- on ragged pixel tiles
    and channel chunks, for tables of 2 .. 256 entries (the kernel keeps the table in 256 words of LDS)."""
    prm = ec.index_inputs(B, HW, z)
    tab = ec.table(n_scales)
    bound = float(tab[0])
    rpm, ridx, near = ec.ref_prior_index(prm, tab, bound, B, HW, z)
    flag = _flag()
    pm, idx = _prior_index(L, prm, tab, bound, B, HW, z, status=flag)
    assert int(flag) == 0
    assert torch.equal(pm, rpm)
    assert float(near.float().mean()) <= ec.NEAR_CAP
    bad = (idx.long() != ridx) & ~near
    assert not bool(bad.any()), (int(bad.sum()), idx[bad][:8].tolist(), ridx[bad][:8].tolist())


@pytest.mark.parametrize('n_scales', ec.INDEX_NS)
def test_prior_index_boundaries(L, n_scales):
    """The bound trick of test_lossless_index_boundaries for every j: log-scales of -100, -90 and -30 give exp(-2.3), below every
    table, so s == bound; +100 gives inf."""
    tab = ec.table(n_scales)
    tab_d = tab.cuda()
    n, z = n_scales, len(ec.BOUND_LVS)
    prm = torch.tensor([[0.5, -1.5, 2.5, -3.5] + list(ec.BOUND_LVS)])
    prm_d = prm.cuda()
    pm = torch.full((n, 2, z), float('nan'), device='cuda')
    idx = torch.full((n, 2, z), 255 if n < 256 else 7, dtype=torch.uint8, device='cuda')
    for j in range(n):
        for up in (0, 1):
            bound = ec.next_up(tab[j]) if up else float(tab[j])
            assert L.lvae_prior_index_f32(prm_d.data_ptr(), pm[j, up].data_ptr(), idx[j, up].data_ptr(), tab_d.data_ptr(), n, bound, 1, 1, z,
                                          None, _st()) == 0
    torch.cuda.synchronize()
    idx, j = idx.cpu().long(), torch.arange(n)
    for up in (0, 1):
        want = (j + up).clamp(max=n - 1)
        for c in range(z - 1):
            assert torch.equal(idx[:, up, c], want), (up, c)
        assert bool((idx[:, up, z - 1] == n - 1).all())
    assert bool((pm.cpu() == prm[0, :z]).all())


def test_prior_index_behind_split_k_same_bits(L):
    """The _sk_ form with S = 3 on the grid: the parameters it forms, the means and every index equal the plain form's on the sum done
    by torch in slice order."""
    B, HW, z, S = 2, 129, 33, 3
    tab = ec.table(64)
    bound = float(tab[0])
    ws, bias, prm = ec.index_sk_inputs(B, HW, z, S)
    pm0, idx0 = _prior_index(L, prm, tab, bound, B, HW, z)
    rpm, ridx, near = ec.ref_prior_index(prm, tab, bound, B, HW, z)
    assert torch.equal(pm0, rpm) and float(near.float().mean()) <= ec.NEAR_CAP and torch.equal(idx0.long()[~near], ridx[~near])
    ws_d, bias_d, tab_d = ws.cuda(), bias.cuda(), tab.cuda()
    prm1 = torch.full((B * HW, 2 * z), float('nan'), device='cuda')
    pm1 = torch.full((B * HW, z), float('nan'), device='cuda')
    idx1 = torch.full((B, z, HW), 255, dtype=torch.uint8, device='cuda')
    flag = _flag()
    assert L.lvae_prior_index_sk_f32(ws_d.data_ptr(), S, bias_d.data_ptr(), prm1.data_ptr(), pm1.data_ptr(), idx1.data_ptr(), tab_d.data_ptr(), 64,
                                     bound, B, HW, z, flag.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert int(flag) == 0
    assert torch.equal(prm1.cpu(), prm) and torch.equal(pm1.cpu(), pm0) and torch.equal(idx1.cpu(), idx0)


# ------------------------------------------------------------------------------------------------ C. rate term
@pytest.fixture(scope='module')
def rate_refs():
    return {form: ec.rate_reference(form) for form in (0, 1)}


def _nll_map(L, prm, sym, form):
    B, z, HW = sym.shape
    prm_d, sym_d = prm.cuda(), sym.cuda()
    out = torch.full((B, z, HW), float('nan'), device='cuda')
    assert L.lvae_gaussian_nll_map_f32(prm_d.data_ptr(), sym_d.data_ptr(), out.data_ptr(), ec.BOUND, B, HW, z, form, _st()) == 0
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('form', (0, 1))
def test_rate_term_against_fp64(L, rate_refs, form):
    """lv in [-30, 30] x sym in -40 .. 40, both CDF forms (0: the hand-written lvae_erff of csrc/device_math.h, 1: erfcf): exp(-out)
    against the fp64 P of the same formula, absolute -- the fp32 difference up - lo carries ~1e-7 whatever P is.  The allowance is
    RATE_TOL_FACTOR times what the same formula in fp32 torch loses on this grid; and since an absolute bound in P cannot see the
    max(P, 1e-9) clamp, every output is finite and at most -logf(1e-9f), attained bit for bit at |sym| = 40 with s at the bound."""
    prm, sym, p64, err32 = rate_refs[form]
    out = _nll_map(L, prm, sym, form)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    err = float((torch.exp(-out.double()) - p64).abs().max())
    print(f'rate term, cdf_form {form}: max |P - P64| kernel {err:.3e}, fp32 torch {err32:.3e}')
    assert err <= ec.RATE_TOL_FACTOR * err32, f'cdf_form {form}: kernel {err:.3e} > {ec.RATE_TOL_FACTOR} x fp32 torch {err32:.3e}'
    cap = float(ec.RATE_CAP)
    assert float(out.max()) <= cap, (float(out.max()), cap)
    at_bound = (prm[:, ec.RATE_Z:].view(ec.RATE_B, -1, ec.RATE_Z).permute(0, 2, 1) <= -25.0) & (sym.abs() == 40)
    assert int(at_bound.sum()) > 300
    assert bool((out[at_bound] == ec.RATE_CAP).all()), (sorted(set(out[at_bound].tolist())), cap)
    assert float(out.min()) >= 0.0 and float(out.min()) < 1e-3                    # P <= 1, and P reaches 1 where s is small


@pytest.mark.parametrize('form', (0, 1))
def test_rate_sum_is_the_sum_of_the_map(L, form):
    """lvae_gaussian_nll_f32 on every fifth pixel of the grid: its per-image fp64 sum is the fp64 sum of the map's fp32 terms."""
    prm, sym = ec.rate_inputs(5)
    B, z, HW = sym.shape
    out = _nll_map(L, prm, sym, form)
    prm_d, sym_d = prm.cuda(), sym.cuda()
    nats = torch.zeros(B, dtype=torch.float64, device='cuda')
    assert L.lvae_gaussian_nll_f32(prm_d.data_ptr(), sym_d.data_ptr(), nats.data_ptr(), ec.BOUND, B, HW, z, form, _st()) == 0
    torch.cuda.synchronize()
    sums = out.double().sum(dim=(1, 2))
    assert torch.allclose(nats.cpu(), sums, rtol=1e-9, atol=0), (nats.cpu().tolist(), sums.tolist())
