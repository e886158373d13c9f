"""Eval-mode forward pass (`model(im)`, forward_eval, image_self_evaluate) of the four models: the host helpers and the C ABI (not-gpu),
the three statistics kernels (lvae_gaussian_nll_chan_f32, lvae_rd_image_f32, lvae_pixel_nll_f32), the models against the reference's
goldens (tests/golden/make_golden_eval_forward.py) and the invariants that tie forward() to the codec (gpu)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import seeded_init
from oracle import qarv_oracle, qres_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('lvae_gaussian_nll_chan_f32', 'lvae_rd_image_f32', 'lvae_pixel_nll_f32')


# ----------------------------------------------------------------------------------------------- not-gpu: ABI and host helpers
def test_new_symbols_exported_and_declared():
    from lvae import _native
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'lvae_hip.h')).read(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _native.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', src), name
        assert name in exported and name in _native.SIGNATURES and name in _native.OP_KINDS, name
    assert _native.ABI_VERSION == 27 and _native.lib().lvae_abi_version() == 27


def test_new_kernels_reject_bad_arguments_without_gpu():
    L = __import__('lvae')._native.lib()
    assert L.lvae_gaussian_nll_chan_f32(None, None, None, 0.11, 1, 4, 4, 1, None) == -22
    assert L.lvae_rd_image_f32(None, None, None, None, None, 1, 4, 4, None, None) == -22
    assert L.lvae_pixel_nll_f32(None, None, None, None, None, 1, 4, 4, None, None) == -22
    from lvae import _native
    assert _native.EVAL_CHUNKS == int(re.search(r'#define LVAE_EVAL_CHUNKS (\d+)', open(os.path.join(REPO, 'include', 'lvae_hip.h')).read()).group(1))


@pytest.mark.parametrize('h,w,top,left', [(67, 131, 2, 2), (65, 193, 0, 0), (64, 199, 0, 4), (127, 64, 32, 0), (130, 135, 1, 4),
                                          (64, 128, 0, 0)])
def test_crop_divisible_by_center_offsets(h, w, top, left):
    """torchvision's center_crop offsets, int(round((h - h_new) / 2)) -- Python's round, ties to even: 1.5 -> 2, 0.5 -> 0, 3.5 -> 4."""
    from PIL import Image
    from lvae.utils.coding import crop_divisible_by
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    a = np.stack([yy % 256, xx % 256, (yy // 256) * 16 + xx // 256], -1).astype(np.uint8)
    out = np.asarray(crop_divisible_by(Image.fromarray(a), div=64))
    hn, wn = 64 * (h // 64), 64 * (w // 64)
    assert (top, left) == (int(round((h - hn) / 2.0)), int(round((w - wn) / 2.0)))
    assert out.shape == (hn, wn, 3)
    assert np.array_equal(out, a[top:top + hn, left:left + wn])


class _StubModel(torch.nn.Module):
    """CPU stand-in with the forward() contract: a dict of per-image statistics (one of them a tensor, as `loss`)."""
    max_stride = 64

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, im):
        self.seen.append((tuple(im.shape), float(im[0, 0, 0, 0])))
        return {'loss': im.mean() + self.w[0], 'h': float(im.shape[2]), 'first': float(im[0, 0, 0, 0])}


def test_image_self_evaluate_on_a_stub(tmp_path):
    from PIL import Image
    from lvae.evaluation import image_self_evaluate
    (tmp_path / 'sub').mkdir()
    specs = {'b.png': (130, 70, 10), 'a.png': (64, 64, 20), 'sub/c.png': (200, 128, 30)}
    for name, (h, w, v) in specs.items():
        a = np.full((h, w, 3), v, np.uint8)
        y0, x0 = int(round((h - 64 * (h // 64)) / 2.0)), int(round((w - 64 * (w // 64)) / 2.0))
        a[y0, x0, 0] = v + 1                                  # the crop's first pixel
        Image.fromarray(a).save(tmp_path / name)
    m = _StubModel()
    res = image_self_evaluate(m, str(tmp_path), progress=False)
    order = sorted(specs, key=lambda n: str(tmp_path / n))
    assert [s[0] for s in m.seen] == [(1, 3, 64 * (specs[n][0] // 64), 64 * (specs[n][1] // 64)) for n in order]
    assert [round(s[1] * 255) for s in m.seen] == [specs[n][2] + 1 for n in order]
    assert set(res) == {'loss', 'h', 'first'}
    assert res['h'] == pytest.approx(np.mean([64 * (specs[n][0] // 64) for n in order]))
    assert res['first'] == pytest.approx(np.mean([(specs[n][2] + 1) / 255 for n in order]))
    assert isinstance(res['loss'], torch.Tensor)


# ----------------------------------------------------------------------------------------------- gpu: kernels
def _lib():
    from lvae import _native
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('cdf_form', [0, 1])
def test_nll_chan_equals_fp64_sums_of_nll_map(cdf_form):
    L = _lib()
    gen = torch.Generator().manual_seed(11 + cdf_form)
    for B, HW, z in ((3, 517, 10), (2, 1536, 40), (1, 2, 16), (4, 64, 17)):
        M = B * HW
        prm = torch.cat([torch.randn(M, z, generator=gen) * 2, torch.rand(M, z, generator=gen) * 8 - 5], 1).contiguous().cuda()
        sym = torch.randint(-6, 7, (B, z, HW), generator=gen, dtype=torch.int32).cuda()
        kl = torch.empty(B, z, HW, device='cuda')
        out = torch.full((B, z), float('nan'), dtype=torch.float64, device='cuda')
        assert L.lvae_gaussian_nll_map_f32(prm.data_ptr(), sym.data_ptr(), kl.data_ptr(), 0.11, B, HW, z, cdf_form, _st()) == 0
        assert L.lvae_gaussian_nll_chan_f32(prm.data_ptr(), sym.data_ptr(), out.data_ptr(), 0.11, B, HW, z, cdf_form, _st()) == 0
        torch.cuda.synchronize()
        ref = kl.double().sum(dim=2)
        assert torch.allclose(out, ref, rtol=1e-12, atol=0), float(((out - ref) / ref).abs().max())
        again = torch.empty_like(out)
        assert L.lvae_gaussian_nll_chan_f32(prm.data_ptr(), sym.data_ptr(), again.data_ptr(), 0.11, B, HW, z, cdf_form, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(again), _bits(out))


@pytest.mark.gpu
def test_rd_image_equals_fp64_restatement():
    from lvae import _native
    L = _lib()
    gen = torch.Generator().manual_seed(4)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    for B, H, W in ((2, 64, 128), (1, 37, 1030), (3, 8, 8)):
        raw = (torch.randn(B * H * W, 3, generator=gen) * 0.8).cuda()
        im = torch.rand(B, 3, H, W, generator=gen).cuda()
        im_hat = torch.empty(B, 3, H, W, device='cuda')
        sums = torch.empty(B, 2, dtype=torch.float64, device='cuda')
        ws = torch.empty(B, 256, 2, dtype=torch.float64, device='cuda')
        assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        v = raw.view(B, H, W, 3).permute(0, 3, 1, 2)
        want = v.clamp(-1.0, 1.0).mul(0.5).add(0.5)
        assert torch.equal(im_hat, want)
        d = (v - (im - 0.5) * 2.0).double()
        e = (want - im).double()
        ref = torch.stack([d.square().sum(dim=(1, 2, 3)), e.square().sum(dim=(1, 2, 3))], 1)
        assert torch.allclose(sums, ref, rtol=1e-12, atol=0)
        again = torch.empty_like(sums)
        assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), again.data_ptr(), ws.data_ptr(), B, H, W, None, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(again), _bits(sums))
        # the chunk map depends on H*W alone: one image of the batch on its own gives its row of the batched call, bit for bit
        one = torch.empty(1, 2, dtype=torch.float64, device='cuda')
        hat1 = torch.empty(1, 3, H, W, device='cuda')
        assert L.lvae_rd_image_f32(raw[(B - 1) * H * W:].data_ptr(), im[B - 1:].data_ptr(), hat1.data_ptr(), one.data_ptr(), ws.data_ptr(), 1, H, W,
                                   None, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(one[0]), _bits(sums[B - 1])) and torch.equal(hat1[0], im_hat[B - 1])
    assert int(status) == 0
    raw[5, 1] = float('inf')
    assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert int(status) == _native.STATUS_NONFINITE_IMAGE
    assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), B, H, W, None, _st()) == -22
    assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), 0, H, W, None, _st()) == -22
    assert L.lvae_rd_image_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), None, B, H, W, None, _st()) == -22


def _pixel_nll_torch(raw6, im, B, H, W):
    """forward_loss of GaussianNLLOutputNet in torch fp32 on the same device (the reference's expression, entropy_coding.py:18-49)."""
    r = raw6.view(B, H, W, 6).permute(0, 3, 1, 2)
    mean, l = r[:, :3], r[:, 3:]
    logscale = torch.nn.functional.softplus(l + 16) - 16
    x = (im - 0.5) * 2.0
    dist = torch.distributions.Normal(mean, torch.exp(logscale), validate_args=False)
    b = 1 / 127.5
    pm = dist.cdf(x + 0.5 * b) - dist.cdf(x - 0.5 * b)
    lp = torch.where(pm > 1e-6, torch.log(pm.clamp(min=1e-8)), dist.log_prob(x) + math.log(b))
    return -lp, pm, mean


@pytest.mark.gpu
def test_pixel_nll_agrees_with_torch_restatement():
    L = _lib()
    gen = torch.Generator().manual_seed(8)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    for B, H, W in ((2, 48, 80), (1, 33, 1100)):
        n = B * H * W
        # log-scales from -24 (the softplus bound: logscale -> -16) to 8 (softplus' identity branch, l + 16 > 20); means from well inside
        # the bin to far outside it: P on both sides of 1e-6
        mean = (torch.randn(n, 3, generator=gen) * 1.5).clamp(-3, 3)
        ls = torch.rand(n, 3, generator=gen) * 32 - 24
        raw = torch.cat([mean, ls], 1).contiguous().cuda()
        im = torch.randint(0, 256, (B, 3, H, W), generator=gen).float().div(255).cuda()
        im_hat = torch.empty(B, 3, H, W, device='cuda')
        sums = torch.empty(B, 2, dtype=torch.float64, device='cuda')
        ws = torch.empty(B, 256, 2, dtype=torch.float64, device='cuda')
        assert L.lvae_pixel_nll_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        nll, pm, m = _pixel_nll_torch(raw, im, B, H, W)
        frac_tail = float((pm <= 1e-6).float().mean())
        assert 0.05 < frac_tail < 0.95, frac_tail                          # both branches are exercised
        assert bool(((ls + 16) > 20).any()) and bool((ls < -20).any())
        want_hat = m.clamp(-1.0, 1.0).mul(0.5).add(0.5)
        assert torch.equal(im_hat, want_hat)
        ref = nll.double().sum(dim=(1, 2, 3))
        assert torch.allclose(sums[:, 0], ref, rtol=2e-6, atol=0), (sums[:, 0], ref)
        sq = (want_hat - im).double().square().sum(dim=(1, 2, 3))
        assert torch.allclose(sums[:, 1], sq, rtol=1e-12, atol=0)
        again = torch.empty_like(sums)
        assert L.lvae_pixel_nll_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), again.data_ptr(), ws.data_ptr(), B, H, W, None, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(again), _bits(sums))
    assert int(status) == 0
    assert L.lvae_pixel_nll_f32(raw.data_ptr(), None, im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, None, _st()) == -22
    assert L.lvae_pixel_nll_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, 0, W, None, _st()) == -22
    assert L.lvae_gaussian_nll_chan_f32(raw.data_ptr(), raw.data_ptr(), sums.data_ptr(), 0.11, B, 4, 4, 2, _st()) == -22


# ----------------------------------------------------------------------------------------------- gpu: models against the goldens
def _load(m, sd):
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    return m


_ARCH = {'qres34m': qres_oracle.qres34m_arch, 'qres17m': qres_oracle.qres17m_arch, 'qres34m_lossless': qres_oracle.qres34m_lossless_arch}


@pytest.fixture(scope='module')
def models():
    import lvae
    out = {}
    for name, arch in _ARCH.items():
        m = _load(lvae.get_model(name), seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(arch()), seed=0))
        m.compress_mode()
        out[name] = m.to('cuda:0').eval()
    m = lvae.get_model('qarv_base')
    _load(m, seeded_init.seeded_state_dict(qarv_oracle.qarv_param_shapes(qarv_oracle.qarv_base_arch()), seed=0))
    m = m.to('cuda:0').eval()
    m.compress_mode()
    out['qarv_base'] = m
    return out


def _img(h, w, seed):
    u8 = seeded_init.synthetic_image_u8(h, w, seed)
    return torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0)


def _check_stats(stats, g, keys):
    for k in keys:
        if k == 'psnr':
            assert abs(stats[k] - float(g['stat.psnr'])) <= 0.01, (stats[k], float(g['stat.psnr']))
        else:
            v = float(stats[k]) if not isinstance(stats[k], torch.Tensor) else float(stats[k].cpu())
            assert v == pytest.approx(float(g[f'stat.{k}']), rel=2e-3), k


def _syms(pl, B):
    return [pl.sym_all[o:o + B * z * hw].view(B, z, hw).cpu().numpy() for o, (z, hw) in zip(pl.sym_off, pl.lat_shapes)]


def _x_raw(pl, B, H, W):
    return pl.x_raw[:B * H * W * 3].view(B, H, W, 3).permute(0, 3, 1, 2).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres34m', 'qres17m', 'qres34m_lossless'])
def test_qres_forward_matches_reference(golden_dir, models, name):
    m = models[name]
    g = np.load(os.path.join(golden_dir, f'{name}_64x128_eval_forward.npz'))
    H, W = g['hw'].tolist()
    im = _img(H, W, int(g['img_seed'])).cuda()
    stats = m(im, return_rec=True)
    lossless = name.endswith('lossless')
    assert list(stats) == ['loss', 'kl', 'nll' if lossless else 'mse', 'bppix', 'psnr', 'im_hat']
    assert stats['loss'].dim() == 0 and stats['loss'].device == im.device
    pl = m._plan('eval', 1, H, W)
    L = len(pl.lat_shapes)
    flips = sum(int((s.reshape(g[f'sym{i}'].shape) != g[f'sym{i}']).sum()) for i, s in enumerate(_syms(pl, 1)))
    assert flips == 0, flips
    kl_chan = pl.kl_chan.cpu()
    kl = np.array([[float(kl_chan[o:o + z].sum())] for o, (z, _) in zip(pl.chan_off, pl.lat_shapes)])
    np.testing.assert_allclose(kl, g['kl_sums'], rtol=2e-3)
    chans = m._stats_log['eval_channels']
    assert len(chans) == L
    for i in range(L):
        np.testing.assert_allclose(np.array(chans[i]), g[f'chan{i}'], rtol=2e-3, atol=1e-9)
    np.testing.assert_allclose(np.array(m._stats_log['eval_bppix']), np.array(m._stats_log['eval_bpdim']) * 3, rtol=1e-12)
    assert float((stats['im_hat'].cpu() - torch.from_numpy(g['im_hat'])).abs().max()) <= 1e-4
    if lossless:
        x_hat = pl.px_raw[:H * W * 6].view(1, H, W, 6)[..., :3].permute(0, 3, 1, 2).cpu()
    else:
        x_hat = _x_raw(pl, 1, H, W)
    assert float((x_hat - torch.from_numpy(g['x_hat'])).abs().max()) <= 1e-4
    _check_stats(stats, g, ['loss', 'kl', 'nll' if lossless else 'mse', 'bppix', 'psnr'])
    m.train()
    try:
        m(im)
        assert m._stats_log['train_bpdim'] == m._stats_log['eval_bpdim']
    finally:
        m.eval()


@pytest.mark.gpu
def test_qarv_forward_matches_reference(golden_dir, models):
    m = models['qarv_base']
    g = np.load(os.path.join(golden_dir, 'qarv_base_64x128_eval_forward.npz'))
    H, W = g['hw'].tolist()
    seeds, lmbs = g['img_seeds'].tolist(), g['lmbs'].tolist()
    im = torch.cat([_img(H, W, s) for s in seeds]).cuda()
    stats = m(im, lmb=torch.tensor(lmbs, device='cuda'), return_rec=True)
    assert list(stats) == ['loss', 'bppix', 'mse', 'psnr', 'im_hat']
    flips, kl = 0, np.zeros((m.num_latents, 2))
    x_hat = torch.empty(2, 3, H, W)
    for b, lmb in enumerate(lmbs):          # one sub-batch per lambda: the B = 1 plans, re-run on this image alone
        m(im[b:b + 1], lmb=lmb)
        enc, dec = m._plan('ence', 1, H, W), m._plan('evald', 1, H // 64, W // 64)
        for i, s in enumerate(_syms(enc, 1)):
            flips += int((s.reshape(g[f'sym{i}'][b:b + 1].shape) != g[f'sym{i}'][b:b + 1]).sum())
        kc = enc.kl_chan.cpu()
        kl[:, b] = [float(kc[o:o + z].sum()) for o, (z, _) in zip(enc.chan_off, enc.lat_shapes)]
        x_hat[b] = _x_raw(dec, 1, H, W)[0]
    assert flips == 0, flips
    # qarv's erf-form fp32 CDF saturates in the far tails (see test_gpu_model.py::test_estimated_rate_path): there P is 0 (clamped to
    # 1e-9) or one fp32 quantum 2^-25 depending on the last ulp of the platform's erff, so a single far-tail element moves a block's sum
    # by ln(2^-25 / 1e-9) = 3.39 nats; rtol 2e-3 plus two such elements per block, and the total within rtol 2e-3
    ref = g['kl_sums']
    assert np.all(np.abs(kl - ref) <= 2e-3 * np.abs(ref) + 2 * 3.4), (kl, ref)
    np.testing.assert_allclose(kl.sum(0), ref.sum(0), rtol=2e-3)
    assert float((x_hat - torch.from_numpy(g['x_hat'])).abs().max()) <= 1e-4
    assert float((stats['im_hat'].cpu() - torch.from_numpy(g['im_hat'])).abs().max()) <= 1e-4
    _check_stats(stats, g, ['loss', 'mse', 'bppix', 'psnr'])


# ----------------------------------------------------------------------------------------------- gpu: invariants
@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['f16x2', 'bf16x3'])
@pytest.mark.parametrize('name', ['qres34m', 'qres17m', 'qarv_base'])
def test_forward_im_hat_equals_the_codec(models, name, prec):
    """model(im, return_rec=True)['im_hat'] is decompress(compress(im)) bit for bit: the raw final store runs the ST_IMAGE launch's
    GEMM, and lvae_rd_image_f32 applies its clamp expression."""
    m = models[name]
    base = m._prec
    m.set_gemm_precision(prec)
    try:
        im = _img(128, 192, 3).cuda()
        kw = {'lmb': m.default_lmb} if name == 'qarv_base' else {}
        x = m(im, return_rec=True, **kw)['im_hat']
        y = m.decompress(m.compress(im))
        assert torch.equal(_bits(x), _bits(y))
    finally:
        m.set_gemm_precision(base)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres34m', 'qres34m_lossless'])
def test_qres_forward_kl_equals_forward_get_latents(models, name):
    m = models[name]
    im = torch.cat([_img(128, 128, 5), _img(128, 128, 6)]).cuda()
    stats = m(im, return_rec=True)
    pl = m._plan('eval', 2, 128, 128)
    kc = pl.kl_chan.cpu()
    lat = m.forward_get_latents(im)
    for (o, (z, _)), st in zip(zip(pl.chan_off, pl.lat_shapes), lat):
        ref = st['kl'].double().sum(dim=(2, 3)).cpu()
        assert torch.allclose(kc[o:o + 2 * z].view(2, z), ref, rtol=1e-12, atol=0)
    again = m(im, return_rec=True)
    assert torch.equal(_bits(again['im_hat']), _bits(stats['im_hat']))
    for k in stats:
        if k != 'im_hat':
            a, b = stats[k], again[k]
            assert (torch.equal(_bits(a), _bits(b)) if isinstance(a, torch.Tensor) else a == b), k


@pytest.mark.gpu
def test_qarv_distinct_lambdas_equal_single_image_calls(models):
    m = models['qarv_base']
    im = torch.cat([_img(64, 128, 1), _img(64, 128, 2), _img(64, 128, 3)]).cuda()
    lmbs = [256.0, 32.0, 256.0]
    both = m(im, lmb=torch.tensor(lmbs, device='cuda'), return_rec=True)
    singles = [m(im[i:i + 1], lmb=lmbs[i], return_rec=True) for i in range(3)]
    pair = m(im[0::2], lmb=256.0, return_rec=True)
    assert torch.equal(_bits(both['im_hat'][0::2]), _bits(pair['im_hat']))
    assert torch.equal(_bits(both['im_hat'][1]), _bits(singles[1]['im_hat'][0]))
    mse = np.mean([s['mse'] for s in singles])
    assert both['mse'] == pytest.approx(mse, rel=1e-12)
    assert both['bppix'] == pytest.approx(np.mean([s['bppix'] for s in singles]), rel=1e-12)
    loss = np.mean([float(s['loss']) for s in singles])
    assert float(both['loss']) == pytest.approx(loss, rel=1e-6)
    again = m(im, lmb=torch.tensor(lmbs, device='cuda'), return_rec=True)
    assert torch.equal(_bits(again['im_hat']), _bits(both['im_hat'])) and again['mse'] == both['mse'] and again['bppix'] == both['bppix']
    torch.manual_seed(0)
    r = m((im, None))                                   # (im, label) pair, lambda drawn by sample_lmb
    assert set(r) == {'loss', 'bppix', 'mse', 'psnr'} and math.isfinite(r['psnr'])
    lo, hi = m.lmb_range
    s = m.sample_lmb(1000)
    assert s.device == im.device and float(s.min()) >= lo * (1 - 1e-5) and float(s.max()) <= hi * (1 + 1e-5)


@pytest.mark.gpu
def test_forward_input_checks(models):
    m = models['qres34m']
    with pytest.raises(AssertionError):
        m(torch.rand(1, 3, 64, 96, device='cuda'))                   # not a multiple of max_stride
    with pytest.raises(AssertionError):
        m(torch.rand(1, 3, 64, 64, device='cuda') * 1.5)             # outside [0, 1]
    assert math.isfinite(m(_img(64, 64, 0).cuda())['psnr'])          # the status word was cleared
    q = models['qarv_base']
    with pytest.raises(AssertionError):
        q(torch.rand(1, 3, 64, 64, device='cuda') - 0.5, lmb=64.0)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres34m', 'qarv_base'])
def test_image_self_evaluate_runs(models, tmp_path, name):
    from PIL import Image
    from lvae.evaluation import image_self_evaluate
    for i, (h, w) in enumerate([(70, 130), (64, 64), (129, 200)]):
        Image.fromarray(seeded_init.synthetic_image_u8(h, w, 10 + i)).save(tmp_path / f'im{i}.png')
    torch.manual_seed(1)
    res = image_self_evaluate(models[name], str(tmp_path), progress=False)
    want = {'loss', 'kl', 'mse', 'bppix', 'psnr'} if name == 'qres34m' else {'loss', 'bppix', 'mse', 'psnr'}
    assert set(res) == want
    assert all(math.isfinite(float(v)) for v in res.values())
    if name == 'qres34m':                                           # the average of the per-image calls on the cropped images
        from lvae.utils.coding import crop_divisible_by, pil_to_tensor01
        per = [models[name](pil_to_tensor01(crop_divisible_by(Image.open(tmp_path / f'im{i}.png'))).unsqueeze(0).cuda()) for i in range(3)]
        for k in want:
            assert float(res[k]) == pytest.approx(np.mean([float(p[k]) for p in per]), rel=1e-6), k
