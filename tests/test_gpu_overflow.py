"""-m gpu: the default GEMM arithmetic ('f16x2': every fp32 operand split into two fp16 terms, csrc/gemm_h2.hip) has fp16's exponent
range, the reference's fp32 MLPs / 1x1 convs (lvae/models/common.py:154, qarv/model.py:36-39) do not overflow at 65504.  An
activation of 65520 or more turns into inf in its hi term and stays NaN / inf until it reaches one of the codec's sinks -- a prior
parameter (qarv/model.py:51-53), a posterior mean (:56-70, :107-108) or the reconstruction (:224-232) -- where the kernels OR a bit into
the plan's status word (include/lvae_hip.h "status word") and the host raises `lvae.NonFiniteError` naming
`set_gemm_precision('bf16x3')` BEFORE any byte string / image is returned.  These tests pin that, kernel by kernel and end to end.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import seeded_init
from conftest import load_seeded_into

pytestmark = pytest.mark.gpu

PRIOR, LATENT, IMAGE = 2, 4, 8      # LVAE_STATUS_NONFINITE_*


def _lib():
    from lvae import _native
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _img(h, w, seed):
    u8 = seeded_init.synthetic_image_u8(h, w, seed, 'natural')
    return torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


# ----------------------------------------------------------------------------------------------- the three sinks, kernel by kernel
@pytest.mark.parametrize('bad,where', [(float('nan'), 'mean'), (float('inf'), 'mean'), (float('-inf'), 'lv'), (float('nan'), 'lv'), (None, None)])
def test_prior_index_reports_nonfinite_parameters(bad, where):
    L = _lib()
    B, HW, z = 2, 96, 32
    g = torch.Generator().manual_seed(0)
    prm = torch.randn(B * HW, 2 * z, generator=g).cuda()
    if bad is not None:
        prm[77, (5 if where == 'mean' else z + 5)] = bad
    pm = torch.empty(B * HW * z, device='cuda')
    idx = torch.empty(B * HW * z, dtype=torch.uint8, device='cuda')
    table = torch.exp(torch.linspace(np.log(0.11), np.log(20.0), 64)).cuda()
    flag = _flag()
    assert L.lvae_prior_index_f32(prm.data_ptr(), pm.data_ptr(), idx.data_ptr(), table.data_ptr(), 64, 0.11, B, HW, z, flag.data_ptr(), _st()) == 0
    assert int(flag.item()) == (0 if bad is None else PRIOR)
    assert int(idx.max()) <= 63                       # whatever the parameters: always a valid table row (the coder cannot be hurt)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), 3.0e9, None])
def test_quantize_reports_nonfinite_and_out_of_int32_latents(bad):
    L = _lib()
    B, HW, z = 1, 64, 8
    g = torch.Generator().manual_seed(1)
    qm, pm = (torch.randn(B * HW, z, generator=g) * 5).cuda(), torch.randn(B * HW, z, generator=g).cuda()
    if bad is not None:
        qm[13, 3] = bad
    sym = torch.empty(B * HW * z, dtype=torch.int32, device='cuda')
    zh = torch.empty(B * HW * z, device='cuda')
    flag = _flag()
    assert L.lvae_quantize_f32(qm.data_ptr(), pm.data_ptr(), sym.data_ptr(), zh.data_ptr(), B, HW, z, z, flag.data_ptr(), _st()) == 0
    assert int(flag.item()) == (0 if bad is None else LATENT)


def _gemm(A, W, bias, prec, store=0, r=0, H=0, Wd=0, status=None):
    """out = A W^T + bias through lvae_gemm_f32 in the given arithmetic (4 = f16x2 on csrc/gemm_h2.hip, 2 = bf16x3)."""
    from lvae import _native
    from lvae.models.base import pack_bf16x3, pack_f16x2
    L = _lib()
    M, K = A.shape
    N = W.shape[0]
    d = _native.GemmDesc()
    w16 = pack_f16x2(W) if prec == 4 else pack_bf16x3(W)
    out = torch.full((M * N,), 7.0, device='cuda')
    d.A0, d.lda0, d.K0, d.K1, d.Wt, d.ldw, d.bias = A.data_ptr(), K, K, 0, W.data_ptr(), K, bias.data_ptr()
    d.out, d.ldo, d.M, d.N, d.K = out.data_ptr(), N, M, N, K
    d.a_mode, d.epi, d.store, d.r, d.H, d.W = _native.A_PLAIN, _native.EPI_BIAS, store, r, H, Wd
    d.prec, d.Wt16 = prec, w16.data_ptr()
    d.status = status.data_ptr() if status is not None else None
    assert L.lvae_gemm_f32(ctypes.byref(d), _st()) == 0
    torch.cuda.synchronize()
    return out


def test_gemm_with_one_activation_beyond_fp16_poisons_its_row_and_the_sink_reports_it():
    """One 7e4 activation: under f16x2 its hi term is inf, so its whole output row is NaN / inf (never a wrong FINITE number), and the
    prior-parameter sink fed with that output raises the flag; the same GEMM under bf16x3 is finite and close to fp64."""
    L = _lib()
    g = torch.Generator().manual_seed(2)
    M, K, N = 256, 128, 64
    A = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    b = torch.randn(N, generator=g).cuda()
    A[100, 17] = 7.0e4
    ref = (A.double() @ W.double().t() + b.double())
    o4 = _gemm(A, W, b, 4).view(M, N)
    assert not torch.isfinite(o4[100]).any(), 'an operand beyond 65520 must poison every output of its row'
    rows = torch.ones(M, dtype=torch.bool); rows[100] = False
    assert torch.isfinite(o4[rows]).all() and (o4[rows].double() - ref[rows]).abs().max() < 1e-4
    o2 = _gemm(A, W, b, 2).view(M, N)
    assert torch.isfinite(o2).all() and ((o2.double() - ref).abs() / (1 + ref.abs())).max() < 1e-5
    # the GEMM's output as prior parameters [M][2z]: the sink reports it
    z = N // 2
    pm = torch.empty(M * z, device='cuda'); idx = torch.empty(M * z, dtype=torch.uint8, device='cuda')
    table = torch.exp(torch.linspace(np.log(0.11), np.log(20.0), 64)).cuda()
    for out, want in ((o4, PRIOR), (o2, 0)):
        flag = _flag()
        assert L.lvae_prior_index_f32(out.data_ptr(), pm.data_ptr(), idx.data_ptr(), table.data_ptr(), 64, 0.11, 1, M, z, flag.data_ptr(), _st()) == 0
        assert int(flag.item()) == want
    # 65504 (largest finite fp16) .. just below 65520 still splits exactly: no overflow, no flag
    A[100, 17] = 65519.0
    o4 = _gemm(A, W, b, 4).view(M, N)
    ref = (A.double() @ W.double().t() + b.double())
    assert torch.isfinite(o4).all() and ((o4.double() - ref).abs() / (1 + ref.abs())).max() < 1e-5


def test_image_store_reports_nonfinite_before_the_clamp():
    """The final layer's store clamps to [-1, 1] (qarv/model.py:224-232): fminf / fmaxf would turn a NaN into a valid-looking pixel."""
    from lvae import _native
    g = torch.Generator().manual_seed(3)
    Hh, Ww, K, r = 8, 12, 128, 4
    M, N = Hh * Ww, 3 * r * r
    A = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    b = torch.zeros(N).cuda()
    for prec in (4, 2):
        flag = _flag()
        out = _gemm(A, W, b, prec, store=_native.ST_IMAGE, r=r, H=Hh, Wd=Ww, status=flag)
        assert int(flag.item()) == 0 and torch.isfinite(out).all() and 0.0 <= float(out.min()) and float(out.max()) <= 1.0
        A2 = A.clone(); A2[5, 9] = float('nan')
        flag = _flag()
        out = _gemm(A2, W, b, prec, store=_native.ST_IMAGE, r=r, H=Hh, Wd=Ww, status=flag)
        assert int(flag.item()) == IMAGE
    A2 = A.clone(); A2[5, 9] = 7.0e4                 # f16x2 only: overflow of the operand split
    flag = _flag()
    _gemm(A2, W, b, 4, store=_native.ST_IMAGE, r=r, H=Hh, Wd=Ww, status=flag)
    assert int(flag.item()) == IMAGE
    flag = _flag()
    _gemm(A2, W, b, 2, store=_native.ST_IMAGE, r=r, H=Hh, Wd=Ww, status=flag)
    assert int(flag.item()) == 0


# ----------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def fresh_model(qarv_seeded_sd):
    """A private qarv_base (the session's product_model must not see scaled weights)."""
    import lvae
    m = lvae.get_model('qarv_base')
    load_seeded_into(m, qarv_seeded_sd)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    return m


def _latent_blocks(m):
    return [b for b in m.dec_blocks if getattr(b, 'is_latent_block', False)]


@pytest.mark.parametrize('native_loops', [True, False])
def test_encoder_overflow_raises_under_f16x2_and_passes_under_bf16x3(fresh_model, native_loops):
    """post_merge of the last latent block scaled until its output (the residual stream of posterior2 and the A operand of the 3x3
    posterior head, qarv/model.py:56-70) passes 65504: compress() must raise under the default arithmetic -- from the native group
    loop and from the Python loop alike -- and code + round-trip under bf16x3, whose terms have fp32's range."""
    import lvae
    m = fresh_model
    im = _img(128, 192, 5).cuda()
    blk = _latent_blocks(m)[-1]
    w0, b0 = blk.post_merge.weight.data.clone(), blk.post_merge.bias.data.clone()
    loops0 = m.native_group_loops
    try:
        m.native_group_loops = native_loops
        m.set_gemm_precision('bf16x3')
        m.compress(im)
        pl = m._plan('enc', 1, 128, 192, 0)
        mg = float(pl.bufs['post_m'].abs().max())          # last writer: the last latent block's posterior2 output (in place)
        s = 4.0e5 / mg
        blk.post_merge.weight.data.mul_(s); blk.post_merge.bias.data.mul_(s)
        m._invalidate()
        m.set_gemm_precision('f16x2')
        with pytest.raises(lvae.NonFiniteError, match="set_gemm_precision\\('bf16x3'\\)"):
            m.compress(im)
        with pytest.raises(lvae.NonFiniteError):          # the status word was re-armed: the second call fails the same way
            m.compress(im)
        m.set_gemm_precision('bf16x3')
        s1 = m.compress(im)
        x1 = m.decompress(s1)
        assert torch.isfinite(x1).all()
        assert m.compress(im) == s1
        # good weights again: the same plans' status words are clean and the default arithmetic codes
        blk.post_merge.weight.data.copy_(w0); blk.post_merge.bias.data.copy_(b0)
        m._invalidate()
        m.set_gemm_precision('f16x2')
        s2 = m.compress(im)
        assert torch.isfinite(m.decompress(s2)).all()
    finally:
        blk.post_merge.weight.data.copy_(w0); blk.post_merge.bias.data.copy_(b0)
        m._invalidate()
        m.set_gemm_precision('f16x2')
        m.native_group_loops = loops0


@pytest.mark.parametrize('native_loops', [True, False])
def test_decoder_overflow_raises_under_f16x2_and_passes_under_bf16x3(fresh_model, native_loops):
    """z_proj of the LAST latent block feeds only layers the encoder never runs (it stops at CompresionStopFlag, qarv/model.py:310-312):
    scaled up, the top-down state passes 65504 inside the decoder's tail, the upsampling GEMMs overflow and the reconstruction is NaN --
    which the final clamp would hide.  decompress() must raise under f16x2 and return a finite image under bf16x3; a batch and
    conditional_sample() raise as well."""
    import lvae
    m = fresh_model
    im = _img(128, 192, 6).cuda()
    blk = _latent_blocks(m)[-1]
    w0, b0 = blk.z_proj.weight.data.clone(), blk.z_proj.bias.data.clone()
    loops0 = m.native_group_loops
    try:
        m.native_group_loops = native_loops
        m.set_gemm_precision('f16x2')
        s_ok = m.compress(im)
        x_ok = m.decompress(s_ok)
        blk.z_proj.weight.data.mul_(3.0e6)
        m._invalidate()
        s_f16 = m.compress(im)                              # the encoder does not reach the scaled layer
        assert s_f16 == s_ok
        with pytest.raises(lvae.NonFiniteError, match='reconstruction'):
            m.decompress(s_f16)
        with pytest.raises(lvae.NonFiniteError):
            m.decompress_batch([s_f16] * 4)
        m.set_gemm_precision('bf16x3')
        s_x3 = m.compress(im)
        x = m.decompress(s_x3)
        assert torch.isfinite(x).all() and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        blk.z_proj.weight.data.copy_(w0); blk.z_proj.bias.data.copy_(b0)
        m._invalidate()
        m.set_gemm_precision('f16x2')
        assert torch.equal(m.decompress(s_ok), x_ok)        # clean again
    finally:
        blk.z_proj.weight.data.copy_(w0); blk.z_proj.bias.data.copy_(b0)
        m._invalidate()
        m.set_gemm_precision('f16x2')
        m.native_group_loops = loops0


def test_prior_overflow_is_reported_on_both_sides(fresh_model):
    """A top-down state beyond fp16 BEFORE a latent block (z_proj of block 0 scaled): the next block's prior parameters are NaN on the
    encoder and on the decoder -- both must raise, not code / decode against index 0 and a NaN mean (VERDICT r03 'Missing 1')."""
    import lvae
    m = fresh_model
    im = _img(64, 64, 7).cuda()
    blk = _latent_blocks(m)[0]
    w0 = blk.z_proj.weight.data.clone()
    try:
        m.set_gemm_precision('f16x2')
        s_ok = m.compress(im)
        blk.z_proj.weight.data.mul_(3.0e6)
        m._invalidate()
        with pytest.raises(lvae.NonFiniteError, match='prior parameters'):
            m.compress(im)
        with pytest.raises(lvae.NonFiniteError):
            m.decompress(s_ok)
        with pytest.raises(lvae.NonFiniteError):
            m.estimate(im)
        m.set_gemm_precision('bf16x3')
        assert torch.isfinite(m.decompress(m.compress(im))).all()
    finally:
        blk.z_proj.weight.data.copy_(w0)
        m._invalidate()
        m.set_gemm_precision('f16x2')


def test_qres_overflow_raises():
    """qres34m shares the sinks (lvae_prior_index_f32 / lvae_quantize_f32 / the image store): with z_proj of its first latent block
    scaled up the top-down state overflows fp16 and both compress() and decompress() raise; bf16x3 codes."""
    import lvae
    from oracle import qres_oracle
    sd = seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(qres_oracle.qres34m_arch()), seed=0)
    m = lvae.get_model('qres34m')
    load_seeded_into(m, sd)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    im = _img(64, 64, 8).cuda()
    obj = m.compress(im)
    assert torch.isfinite(m.decompress(obj)).all()
    qlb = [b for b in m.decoder.dec_blocks if getattr(b, 'kind', '') == 'qlb'][0]
    w0 = qlb.z_proj[2].weight.data.clone()
    for scale in (1e5, 1e6, 1e7, 1e8):                  # the first scale that pushes the top-down state past fp16's range
        qlb.z_proj[2].weight.data.copy_(w0 * scale)
        m._invalidate()
        try:
            m.compress(im)
        except lvae.NonFiniteError:
            break
    else:
        pytest.fail('no scale of z_proj overflowed the f16x2 arithmetic')
    with pytest.raises(lvae.NonFiniteError):
        m.compress(im)
    with pytest.raises(lvae.NonFiniteError):
        m.decompress(obj)
    m.set_gemm_precision('bf16x3')
    m._invalidate()
    assert torch.isfinite(m.decompress(m.compress(im))).all()
