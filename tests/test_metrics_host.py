"""not-gpu: lvae.metrics (MS-SSIM, PSNR) on CPU tensors, the argument checks of the C-ABI entry, and the `metrics` option of the
evaluation harness with a CPU stub codec.  `ms_ssim_fp64` below is the yardstick of every MS-SSIM test (tests/test_gpu_msssim.py imports
it): an fp64 restatement of the published definition, independent of the package's own code paths."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seeded_init

W5 = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss(n=11, s=1.5):
    c = torch.arange(n, dtype=torch.float64) - n // 2
    g = torch.exp(-(c ** 2) / (2 * s * s)); return g / g.sum()


def _filt(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def _ssim(x, y, g, C1=1e-4, C2=9e-4):
    mx, my = _filt(x, g), _filt(y, g)
    sxx = _filt(x * x, g) - mx * mx; syy = _filt(y * y, g) - my * my; sxy = _filt(x * y, g) - mx * my
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    ss = ((2 * mx * my + C1) / (mx * mx + my * my + C1)) * cs
    return ss.flatten(2).mean(-1), cs.flatten(2).mean(-1)          # (B, C)


def ms_ssim_fp64(x, y, return_scales=False):                       # (B, C, h, w) in [0, 1] -> (B,) float64
    x, y, g, mcs, raw = x.double(), y.double(), gauss(), [], []
    assert min(x.shape[-2:]) > 160
    for i in range(5):
        ss, cs = _ssim(x, y, g)
        raw.append(cs if i < 4 else ss)
        if i < 4:
            mcs.append(torch.relu(cs))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    st = torch.stack(mcs + [torch.relu(ss)], 0)
    out = torch.prod(st ** torch.tensor(W5, dtype=torch.float64).view(-1, 1, 1), 0).mean(1)
    return (out, torch.stack(raw, 1)) if return_scales else out   # scales: (B, 5, C), cs of scales 0..3 and ssim of scale 4, before the relu


def image01(h, w, seed=0, kind='natural'):
    return torch.from_numpy(seeded_init.synthetic_image_u8(h, w, seed, kind)).permute(2, 0, 1).float().div(255).unsqueeze(0)


def noisy(x, sigma, seed):
    """x + N(0, sigma^2), clipped and re-quantised to 8 bits."""
    g = torch.Generator().manual_seed(seed)
    return (x + sigma * torch.randn(x.shape, generator=g)).clamp(0, 1).mul(255).round().div(255)


# ----------------------------------------------------------------------------------------------- lvae.metrics on the CPU
@pytest.mark.parametrize('h,w', [(161, 161), (181, 203), (256, 384)])
def test_cpu_path_equals_yardstick(h, w):
    from lvae.metrics import ms_ssim
    x = torch.cat([image01(h, w, 1), image01(h, w, 2, 'noise')], 0)
    for sigma in (0.01, 0.05, 0.2):
        y = noisy(x, sigma, 7)
        got, ref = ms_ssim(x, y), ms_ssim_fp64(x, y)
        assert got.dtype == torch.float64 and got.shape == (2,)
        assert float((got - ref).abs().max()) <= 1e-12, (sigma, got, ref)
        assert 0.0 < float(ref.min()) and float(ref.max()) < 1.0


def test_yardstick_orders_the_noise_levels_and_knows_black_against_white():
    """The yardstick is not flat: more noise, lower value, in steps of at least 1e-3 -- a thousand times the 1e-6 the GPU tests allow, so
    that bound tells the noise levels apart; black against white is 0.2872 (only C1 keeps it off zero)."""
    x = image01(200, 200, 3)
    v = [float(ms_ssim_fp64(x, noisy(x, s, 5))) for s in (0.01, 0.05, 0.2)]
    assert v[0] > v[1] + 1e-3 and v[1] > v[2] + 1e-3, v
    bw = float(ms_ssim_fp64(torch.zeros(1, 3, 200, 200), torch.ones(1, 3, 200, 200)))
    assert abs(bw - 0.2872) < 5e-5, bw


def test_identical_inverted_and_black_white_on_cpu():
    from lvae.metrics import ms_ssim
    for kind in ('natural', 'noise'):
        x = image01(192, 224, 4, kind)
        assert ms_ssim(x, x).tolist() == [1.0]
        inv = ms_ssim(x, 1 - x)
        assert inv.tolist() == [0.0] and not torch.isnan(inv).any()          # negative cs means: the relu, not a NaN from a fractional power
    bw = ms_ssim(torch.zeros(1, 3, 200, 200), torch.ones(1, 3, 200, 200))
    assert abs(float(bw) - float(ms_ssim_fp64(torch.zeros(1, 3, 200, 200), torch.ones(1, 3, 200, 200)))) <= 1e-12


def test_lists_views_sizes_and_per_scale_means():
    from lvae.metrics import ms_ssim
    big = torch.zeros(2, 3, 256, 320)
    hw = [(181, 203), (256, 300)]
    xs = [image01(h, w, 10 + i) for i, (h, w) in enumerate(hw)]
    ys = [noisy(x, 0.05, i) for i, x in enumerate(xs)]
    for i, (h, w) in enumerate(hw):
        big[i, :, :h, :w] = ys[i][0]
    ref = torch.cat([ms_ssim_fp64(x, y) for x, y in zip(xs, ys)])
    views = [big[i:i + 1, :, :h, :w] for i, (h, w) in enumerate(hw)]
    assert float((ms_ssim(xs, views) - ref).abs().max()) <= 1e-12
    assert float((ms_ssim([x[0] for x in xs], [v[0] for v in views]) - ref).abs().max()) <= 1e-12
    pad_x = torch.zeros_like(big)
    for i, (h, w) in enumerate(hw):
        pad_x[i, :, :h, :w] = xs[i][0]
    assert float((ms_ssim(pad_x, big, sizes=hw) - ref).abs().max()) <= 1e-12
    v, m = ms_ssim(xs[:1], ys[:1], return_scales=True)
    rv, rm = ms_ssim_fp64(xs[0], ys[0], return_scales=True)
    assert m.shape == (1, 5, 3) and float((m - rm).abs().max()) <= 1e-12 and float((v - rv).abs().max()) <= 1e-12


def test_errors_name_the_problem():
    from lvae.metrics import ms_ssim
    x = torch.rand(1, 3, 160, 400)
    with pytest.raises(ValueError, match='160x400'):
        ms_ssim(x, x)
    with pytest.raises(ValueError, match='160x400'):
        ms_ssim(torch.rand(1, 3, 200, 400), torch.rand(1, 3, 200, 400), sizes=[(160, 400)])
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 200, 200), torch.rand(1, 3, 200, 201))
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(1, 3, 200, 200), torch.rand(1, 1, 200, 200))
    with pytest.raises(ValueError):
        ms_ssim([torch.rand(3, 200, 200)], [torch.rand(3, 200, 200), torch.rand(3, 200, 200)])
    with pytest.raises(ValueError):
        ms_ssim(torch.rand(3, 200, 200), torch.rand(3, 200, 200))


def test_psnr_and_db_helpers():
    import lvae
    from lvae.metrics import ms_ssim_db, psnr
    assert lvae.metrics.ms_ssim is not None
    x = image01(64, 64, 0)
    y = noisy(x, 0.05, 1)
    assert psnr(x, y) == pytest.approx(-10 * math.log10(float((x.double() - y.double()).square().mean())), abs=1e-12)
    assert ms_ssim_db(0.99) == pytest.approx(20.0, abs=1e-9)
    assert float(ms_ssim_db(torch.tensor([0.9], dtype=torch.float64))) == pytest.approx(10.0, abs=1e-9)


# ----------------------------------------------------------------------------------------------- the C-ABI entry without a GPU
def _call(L, x, y, hw, B, C, Hmax, Wmax, strides, out, means, ws, ws_bytes):
    flat = [v for p in hw for v in p] if hw is not None else None
    arr = (ctypes.c_int * len(flat))(*flat) if flat is not None else None
    return L.lvae_msssim_f32(x, *strides, y, *strides, arr, B, C, Hmax, Wmax, out, means, ws, ws_bytes, None)


def test_native_entry_rejects_bad_arguments_without_gpu():
    """-22 before any HIP call: safe on a GPU-less host.  The 'device' pointers are host buffers nothing dereferences."""
    from lvae import _native
    L = _native.lib()
    need = L.lvae_msssim_workspace_bytes(1, 3, 200, 400)
    assert need > 0 and need % 8 == 0
    assert L.lvae_msssim_workspace_bytes(2, 3, 200, 400) > need
    assert L.lvae_msssim_workspace_bytes(1, 3, 160, 400) == 0 and L.lvae_msssim_workspace_bytes(0, 3, 200, 400) == 0
    assert L.lvae_msssim_workspace_bytes(1, 0, 200, 400) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    full = (3 * 200 * 400, 200 * 400, 400)
    good = dict(x=p, y=p, hw=[(200, 400)], B=1, C=3, Hmax=200, Wmax=400, strides=full, out=p, means=p, ws=p, ws_bytes=need)
    for k in ('x', 'y', 'hw', 'out', 'means', 'ws'):
        assert _call(L, **{**good, k: None}) == -22, k
    assert _call(L, **{**good, 'B': 0}) == -22
    assert _call(L, **{**good, 'C': 0}) == -22
    assert _call(L, **{**good, 'hw': [(160, 400)]}) == -22                       # a 160-pixel side
    assert _call(L, **{**good, 'hw': [(200, 160)]}) == -22
    assert _call(L, **{**good, 'hw': [(201, 400)]}) == -22                       # beyond Hmax
    assert _call(L, **{**good, 'strides': (3 * 200 * 400, 200 * 400, 399)}) == -22          # a row longer than the row stride
    assert _call(L, **{**good, 'strides': (3 * 200 * 400, 199 * 400, 400)}) == -22          # planes that overlap
    assert _call(L, **{**good, 'B': 2, 'hw': [(200, 400)] * 2, 'strides': (2 * 200 * 400, 200 * 400, 400),
                       'ws_bytes': L.lvae_msssim_workspace_bytes(2, 3, 200, 400)}) == -22  # images that overlap
    assert _call(L, **{**good, 'ws_bytes': need - 1}) == -22


# ----------------------------------------------------------------------------------------------- the evaluation harness, CPU stub codec
class _StubCodec(torch.nn.Module):
    """Deterministic stand-in with the model file API (the real model needs a GPU): keeps the upper 4 bits of every sample."""
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def compress_file(self, img_path, output_path, lmb=None):
        from PIL import Image
        a = np.asarray(Image.open(img_path))
        q = (a >> 4).astype(np.uint8).reshape(-1)
        with open(output_path, 'wb') as f:
            f.write(struct.pack('2H', a.shape[0], a.shape[1]) + ((q[0::2] << 4) | q[1::2]).tobytes())

    def decompress_file(self, bits_path):
        with open(bits_path, 'rb') as f:
            h, w = struct.unpack('2H', f.read(4))
            b = np.frombuffer(f.read(), dtype=np.uint8)
        q = np.stack([b >> 4, b & 15], 1).reshape(h, w, 3).astype(np.float32)
        return torch.from_numpy((q * 16 + 8) / 255).permute(2, 0, 1).unsqueeze(0).contiguous()


def _make_images(d, n=4):
    from PIL import Image
    for i in range(n):
        Image.fromarray(seeded_init.synthetic_image_u8(168 + 8 * i, 200 - 6 * i, seed=20 + i)).save(os.path.join(d, f'im{i:02d}.png'))


def test_imcoding_evaluate_metrics_option(tmp_path):
    from PIL import Image
    from lvae.evaluation import imcoding_evaluate
    from lvae.utils.coding import pil_to_tensor01
    d = str(tmp_path)
    _make_images(d)
    m = _StubCodec()
    base = imcoding_evaluate(m, d)
    assert set(base) == {'bpp', 'mse', 'psnr'}
    assert imcoding_evaluate(m, d, metrics=('psnr',)) == base
    both = imcoding_evaluate(m, d, metrics=('psnr', 'ms-ssim'))
    assert set(both) == {'bpp', 'mse', 'psnr', 'ms-ssim'}
    for k in base:
        assert both[k] == base[k], k
    vals = []
    for name in sorted(os.listdir(d)):
        p = os.path.join(d, name)
        bits = str(tmp_path / 'one.bits')
        m.compress_file(p, bits)
        vals.append(float(ms_ssim_fp64(pil_to_tensor01(Image.open(p)).unsqueeze(0), m.decompress_file(bits))))
        os.unlink(bits)
    assert abs(both['ms-ssim'] - sum(vals) / len(vals)) <= 1e-12 and 0.5 < both['ms-ssim'] < 1.0
    with pytest.raises(ValueError, match='unknown metrics'):
        imcoding_evaluate(m, d, metrics=('psnr', 'lpips'))


def test_gather_stats_default_stays_four_columns():
    import inspect
    from lvae.evaluation import gather_stats, imcoding_evaluate, imcoding_evaluate_sharded
    assert inspect.signature(gather_stats).parameters['columns'].default == 4
    for fn in (imcoding_evaluate, imcoding_evaluate_sharded):
        assert inspect.signature(fn).parameters['metrics'].default == ('psnr',)


def test_sharded_world_one_equals_single_with_the_option(tmp_path):
    import torch.distributed as dist
    from lvae.evaluation import imcoding_evaluate, imcoding_evaluate_sharded
    d = str(tmp_path)
    _make_images(d)
    m = _StubCodec()
    single = imcoding_evaluate(m, d, metrics=('psnr', 'ms-ssim'))
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "rdzv"}', rank=0, world_size=1)
    try:
        assert imcoding_evaluate_sharded(m, d, metrics=('psnr', 'ms-ssim')) == single
        assert imcoding_evaluate_sharded(m, d) == imcoding_evaluate(m, d)
    finally:
        dist.destroy_process_group()
