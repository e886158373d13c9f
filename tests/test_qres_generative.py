"""QRes-VAE generative API (cond_sample with missing latents / paint_box, uncond_sample, forward_get_latents, inpaint): the host
box arithmetic (not-gpu), the three sampling / likelihood kernels, the model paths against the reference's t = 0 goldens
(tests/golden/make_golden_qres_generative.py) and the invariants that tie them to the codec (gpu)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
from oracle import qres_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- host: the paint box
BOXES = [(0.25, 0.25, 0.75, 0.75), (0.4, 0.4, 0.8, 0.8), (0.0, 0.0, 1.0, 1.0), (0.5, 0.5, 0.5, 0.5), (0.125, 0.375, 0.625, 0.875),
         (0.1, 0.3, 0.3, 0.1), (-0.2, -0.1, 0.3, 1.4), (0.75, 0.25, 0.25, 0.75)]
MAPS = [(1, 2), (1, 1), (2, 1), (2, 3), (2, 4), (4, 8), (8, 12), (5, 7), (6, 10), (16, 32), (64, 128)]


@pytest.mark.parametrize('box', BOXES)
def test_box_indices_match_reference_slicing(box):
    """The host helper gives the rows / columns the reference's `z[:, :, round(y1*h):round(y2*h), round(x1*w):round(x2*w)]` touches
    (Python's round: ties to even, e.g. 0.5*2 -> 1 but 0.25*2 = 0.5 -> 0 and 0.75*2 = 1.5 -> 2), including 1-wide maps."""
    from lvae.models.qresvae.model import box_slices, latent_box
    x1, y1, x2, y2 = box
    for h, w in MAPS:
        ref = np.zeros((h, w), bool)
        ref[round(y1 * h):round(y2 * h), round(x1 * w):round(x2 * w)] = True
        r0, r1, c0, c1 = box_slices(box, h, w)
        got = np.zeros((h, w), bool)
        got[r0:r1, c0:c1] = True
        assert np.array_equal(got, ref), (box, h, w, (r0, r1, c0, c1))
        assert 0 <= r0 <= r1 <= h and 0 <= c0 <= c1 <= w
        lb = latent_box(box, h, w)
        assert (lb is None) == (min(h, w) == 1)
        if lb is not None:
            assert lb == (r0, r1, c0, c1)


def test_box_ties_go_to_even():
    from lvae.models.qresvae.model import box_slices
    assert box_slices((0.25, 0.25, 0.75, 0.75), 2, 2) == (0, 2, 0, 2)            # round(0.5) = 0, round(1.5) = 2
    assert box_slices((0.25, 0.25, 0.75, 0.75), 6, 6) == (2, 4, 2, 4)            # round(1.5) = 2, round(4.5) = 4
    assert box_slices((0.5, 0.5, 0.5, 0.5), 4, 4) == (0, 0, 0, 0)                # empty


# ----------------------------------------------------------------------------------------------- gpu: kernels
def _lib():
    from lvae import _native
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prm(M, z, gen, lv_lo=-3.0, lv_hi=3.0):
    pm = torch.randn(M, z, generator=gen) * 2
    lv = torch.rand(M, z, generator=gen) * (lv_hi - lv_lo) + lv_lo
    return torch.cat([pm, lv], 1).contiguous().cuda()


def _box(L, prm, lat, out, B, h, w, z, ld, box, t, seed, off):
    rc = L.lvae_latent_sample_box_f32(prm.data_ptr(), None if lat is None else lat.data_ptr(), out.data_ptr(), B, h, w, z, ld, *box,
                                      t, seed, off, _st())
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_latent_box_kernel_branches():
    L = _lib()
    gen = torch.Generator().manual_seed(5)
    B, h, w, z, ld = 2, 9, 70, 14, 16                  # 630 pixels per image: 10 pixel tiles, the last one partial; 14 + 2 pad lanes
    M = B * h * w
    prm = _prm(M, z, gen)
    lat = torch.randn(B, z, h, w, generator=gen).cuda()
    t, seed, off = 0.7, 1234567, 3 << 40
    full = torch.full((M, ld), float('nan'), device='cuda')
    assert L.lvae_prior_sample_f32(prm.data_ptr(), full.data_ptr(), M, z, ld, t, seed, off, _st()) == 0
    # no latent given, and a full box: the draw of lvae_prior_sample_f32, bit for bit (pad lanes 0)
    for lt, box in ((None, (0, 0, 0, 0)), (lat, (0, h, 0, w))):
        out = torch.full((M, ld), float('nan'), device='cuda')
        _box(L, prm, lt, out, B, h, w, z, ld, box, t, seed, off)
        assert torch.equal(out.view(torch.int32), full.view(torch.int32))
    # empty box: the NHWC transpose of the given latent, zero pad lanes
    want = torch.zeros(M, ld, device='cuda')
    want[:, :z] = lat.permute(0, 2, 3, 1).reshape(M, z)
    for box in ((0, 0, 0, 0), (3, 3, 0, w), (0, h, 5, 5)):
        out = torch.full((M, ld), float('nan'), device='cuda')
        _box(L, prm, lat, out, B, h, w, z, ld, box, t, seed, off)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), box
    # a partial box: cells on its first / last row and column are drawn, the ones just outside are copied
    r0, r1, c0, c1 = 2, 6, 17, 65
    out = torch.full((M, ld), float('nan'), device='cuda')
    _box(L, prm, lat, out, B, h, w, z, ld, (r0, r1, c0, c1), t, seed, off)
    inside = torch.zeros(B, h, w, dtype=torch.bool)
    inside[:, r0:r1, c0:c1] = True
    inside = inside.reshape(M).cuda()
    exp = torch.where(inside[:, None], full, want)
    assert torch.equal(out.view(torch.int32), exp.view(torch.int32))
    o4, f4, w4 = out.view(B, h, w, ld), full.view(B, h, w, ld), want.view(B, h, w, ld)
    for y, x in ((r0, c0), (r1 - 1, c1 - 1), (r0, c1 - 1), (r1 - 1, c0)):
        assert torch.equal(o4[:, y, x], f4[:, y, x])
    for y, x in ((r0 - 1, c0), (r1, c0), (r0, c0 - 1), (r0, c1)):
        assert torch.equal(o4[:, y, x], w4[:, y, x])


@pytest.mark.gpu
def test_latent_box_kernel_in_box_moments():
    L = _lib()
    B, h, w, z = 1, 300, 300, 8
    M, lv = B * h * w, 0.7
    pv = math.exp(math.log1p(math.exp(lv + 2.3)) - 2.3)
    prm = torch.cat([torch.full((M, z), 0.25), torch.full((M, z), lv)], 1).contiguous().cuda()
    lat = torch.full((B, z, h, w), -7.0, device='cuda')
    r0, r1, c0, c1 = 40, 260, 30, 280
    for t in (1.0, 0.5):
        out = torch.empty(M, z, device='cuda')
        _box(L, prm, lat, out, B, h, w, z, z, (r0, r1, c0, c1), t, 99, 0)
        o = out.view(h, w, z)
        assert torch.all(o[:r0] == -7.0) and torch.all(o[r1:] == -7.0) and torch.all(o[:, :c0] == -7.0) and torch.all(o[:, c1:] == -7.0)
        d = o[r0:r1, c0:c1].double() - 0.25
        n = d.numel()
        var = (pv * t) ** 2 + t * t / 12.0
        assert abs(float(d.mean())) < 4 * math.sqrt(var / n)
        assert abs(float(d.var()) / var - 1) < 0.02
        s2, u2, u4 = (pv * t) ** 2, t * t / 12.0, t ** 4 / 80.0
        assert abs(float((d ** 4).mean()) / (3 * s2 * s2 + 6 * s2 * u2 + u4) - 1) < 0.05


@pytest.mark.gpu
def test_pixel_sampler():
    L = _lib()
    gen = torch.Generator().manual_seed(3)
    B, H, W = 2, 24, 40
    raw = torch.cat([torch.randn(B * H * W, 3, generator=gen) * 0.8, torch.randn(B * H * W, 3, generator=gen)], 1).contiguous().cuda()
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = torch.empty(B, 3, H, W, device='cuda')
    assert L.lvae_pixel_sample_f32(raw.data_ptr(), out.data_ptr(), B, H, W, 0.0, 7, 0, status.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    mean = raw[:, :3].reshape(B, H, W, 3).permute(0, 3, 1, 2)
    assert torch.equal(out, mean.clamp(-1.0, 1.0).mul(0.5).add(0.5)) and int(status) == 0
    # moments where the clamp cannot bite: mean 0.1, scale 0.05 * t
    B, H, W = 1, 256, 384
    n = B * H * W
    raw = torch.cat([torch.full((n, 3), 0.1), torch.full((n, 3), math.log(0.05))], 1).contiguous().cuda()
    for t in (1.0, 0.5):
        out = torch.empty(B, 3, H, W, device='cuda')
        assert L.lvae_pixel_sample_f32(raw.data_ptr(), out.data_ptr(), B, H, W, t, 11, 5 << 40, status.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        d = (out.double() - 0.5) * 2 - 0.1
        s2 = (0.05 * t) ** 2
        assert abs(float(d.mean())) < 4 * math.sqrt(s2 / d.numel())
        assert abs(float(d.var()) / s2 - 1) < 0.02
        assert abs(float((d ** 4).mean()) / (3 * s2 * s2) - 1) < 0.05
    assert int(status) == 0
    raw[0, 0] = float('nan')
    assert L.lvae_pixel_sample_f32(raw.data_ptr(), out.data_ptr(), B, H, W, 1.0, 11, 0, status.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    from lvae import _native
    assert int(status) == _native.STATUS_NONFINITE_IMAGE


@pytest.mark.gpu
def test_nll_map_matches_sum_and_fp64():
    L = _lib()
    gen = torch.Generator().manual_seed(9)
    B, HW, z = 3, 517, 10
    prm = _prm(B * HW, z, gen)
    sym = torch.randint(-4, 5, (B, z, HW), generator=gen, dtype=torch.int32).cuda()
    kl = torch.empty(B, z, HW, device='cuda')
    nats = torch.zeros(B, dtype=torch.float64, device='cuda')
    assert L.lvae_gaussian_nll_map_f32(prm.data_ptr(), sym.data_ptr(), kl.data_ptr(), 0.11, B, HW, z, 1, _st()) == 0
    assert L.lvae_gaussian_nll_f32(prm.data_ptr(), sym.data_ptr(), nats.data_ptr(), 0.11, B, HW, z, 1, _st()) == 0
    torch.cuda.synchronize()
    sums = kl.double().sum(dim=(1, 2))
    assert torch.allclose(sums, nats, rtol=1e-9, atol=0), (sums, nats)
    lv = prm[:, z:].double().view(B, HW, z).permute(0, 2, 1)
    s = torch.exp(torch.nn.functional.softplus(lv + 2.3) - 2.3).clamp(min=0.11)
    v = sym.double().abs()
    up = 0.5 * torch.special.erfc(-((0.5 - v) / s) / math.sqrt(2))
    lo = 0.5 * torch.special.erfc(-((-0.5 - v) / s) / math.sqrt(2))
    ref = -torch.log((up - lo).clamp(min=1e-9))
    assert torch.allclose(kl.double(), ref, rtol=1e-3, atol=1e-4), float((kl.double() - ref).abs().max())


# ----------------------------------------------------------------------------------------------- gpu: models against the goldens
def _model(name, arch):
    import lvae
    sd = seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(arch), seed=0)
    m = lvae.get_model(name)
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.compress_mode()
    return m.to('cuda:0').eval()


@pytest.fixture(scope='module')
def q34():
    return _model('qres34m', qres_oracle.qres34m_arch())


@pytest.fixture(scope='module')
def q34l():
    return _model('qres34m_lossless', qres_oracle.qres34m_lossless_arch())


@pytest.fixture(scope='module')
def q17():
    return _model('qres17m', qres_oracle.qres17m_arch())


def _img(h, w, seed):
    u8 = seeded_init.synthetic_image_u8(h, w, seed)
    return torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0)


def _maxdiff(x, g):
    return float((x.cpu() - torch.from_numpy(g)).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres34m', 'qres34m_lossless'])
def test_generative_api_matches_reference(golden_dir, q34, q34l, name):
    """forward_get_latents, progressive anchors, uncond_sample, the paint_box case and inpaint, all at t = 0, against the reference.
    inpaint re-encodes a composite of its own output: like any encode, one latent there may sit within arithmetic noise of a rounding
    boundary and flip (z moves by one, the sample by ~0.1); the golden image is one whose encodes keep clear of that."""
    m = {'qres34m': q34, 'qres34m_lossless': q34l}[name]
    g = np.load(os.path.join(golden_dir, f'{name}_64x128_generative.npz'))
    h, w = g['hw'].tolist()
    im = _img(h, w, int(g['img_seed'])).cuda()
    stats = m.forward_get_latents(im)
    assert len(stats) == 12
    flips = 0
    for i, st in enumerate(stats):
        gz = g[f'z{i}']
        assert tuple(st['z'].shape) == gz.shape and st['kl'].shape == st['z'].shape
        dz = (st['z'].cpu() - torch.from_numpy(gz)).abs()
        flips += int((dz > 0.5).sum())                                   # a flipped symbol moves z by one
        assert float(dz[dz <= 0.5].max()) <= 1e-3, i
    assert flips == 0, flips
    kl = np.array([float(st['kl'].double().sum()) for st in stats])
    np.testing.assert_allclose(kl, g['kl_sums'], rtol=2e-3)
    zs = [torch.from_numpy(g[f'z{i}']).cuda() for i in range(12)]
    for k in g['keeps'].tolist():
        x = m.cond_sample([z if i < k else None for i, z in enumerate(zs)], nhw_repeat=(1, h // 64, w // 64), temprature=0.0)
        assert _maxdiff(x, g[f'x_keep{k}']) <= 1e-4, k
    assert _maxdiff(m.uncond_sample((1, h // 64, w // 64), temprature=0.0), g['x_uncond_t0']) <= 1e-4
    assert _maxdiff(m.cond_sample(zs, temprature=0.0, paint_box=tuple(g['paint_box'].tolist())), g['x_paint_t0']) <= 1e-4
    box = tuple(g['inpaint_box'].tolist())
    masked = im.clone()
    masked[:, :, round(box[1] * h):round(box[3] * h), round(box[0] * w):round(box[2] * w)] = 0.0
    assert _maxdiff(m.inpaint(masked, box, steps=2, temprature=0.0), g['x_inpaint_t0']) <= 1e-4


# ----------------------------------------------------------------------------------------------- gpu: invariants
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres34m', 'qres17m'])
def test_decompress_equals_cond_sample_of_latents(q34, q17, name):
    m = {'qres34m': q34, 'qres17m': q17}[name]
    im = _img(128, 192, 4).cuda()
    x_dec = m.decompress(m.compress(im))
    zs = [st['z'] for st in m.forward_get_latents(im)]
    assert torch.equal(m.cond_sample(zs), x_dec)
    assert torch.equal(m.cond_sample(zs, temprature=0.3, seed=5), x_dec)       # given latents, no box: nothing is drawn


@pytest.mark.gpu
def test_seeds_batch_rows_and_inpaint_reproducible(q34):
    m = q34
    a, za = m.uncond_sample((2, 1, 2), temprature=0.5, seed=1234, return_latents=True)
    b, zb = m.uncond_sample((2, 1, 2), temprature=0.5, seed=1234, return_latents=True)
    c, zc = m.uncond_sample((2, 1, 2), temprature=0.5, seed=1235, return_latents=True)
    bits = lambda x: x.view(torch.int32)                                         # noqa: E731  (NaN-safe bit comparison)
    assert a.shape == (2, 3, 64, 128) and len(za) == 12 and za[0].shape == (2, 16, 1, 2)
    assert torch.equal(bits(a), bits(b)) and all(torch.equal(bits(p), bits(q)) for p, q in zip(za, zb))
    assert not torch.equal(za[0], zc[0])
    assert not torch.equal(za[0][0], za[0][1])
    torch.manual_seed(3)
    d = m.uncond_sample((1, 1, 2), temprature=0.5, return_latents=True)[1]
    torch.manual_seed(3)
    e = m.uncond_sample((1, 1, 2), temprature=0.5, return_latents=True)[1]
    assert torch.equal(d[0], e[0])
    # a paint box draws inside and keeps the given latent outside; 1-wide maps keep it whole
    im = _img(64, 128, 2).cuda()
    zs = [st['z'] for st in m.forward_get_latents(im)]
    _, used = m.cond_sample(zs, temprature=0.5, paint_box=(0.25, 0.25, 0.75, 0.75), seed=9, return_latents=True)
    for z, u in zip(zs, used):
        hh, ww = z.shape[2:]
        if min(hh, ww) == 1:
            assert torch.equal(u, z)
            continue
        r0, r1, c0, c1 = round(0.25 * hh), round(0.75 * hh), round(0.25 * ww), round(0.75 * ww)
        keep = torch.ones(hh, ww, dtype=torch.bool)
        keep[r0:r1, c0:c1] = False
        assert torch.equal(u[:, :, keep], z[:, :, keep])
        assert not torch.equal(u[:, :, r0:r1, c0:c1], z[:, :, r0:r1, c0:c1])
    box = (0.4, 0.4, 0.8, 0.8)
    p = m.inpaint(im, box, steps=2, temprature=0.5, seed=7)
    q = m.inpaint(im, box, steps=2, temprature=0.5, seed=7)
    r = m.inpaint(im, box, steps=2, temprature=0.5, seed=8)
    assert p.shape == im.shape and torch.equal(bits(p), bits(q)) and not torch.equal(bits(p), bits(r))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qres17m', 'qres34m_lossless'])
def test_uncond_sample_is_finite(q17, q34l, name):
    m = {'qres17m': q17, 'qres34m_lossless': q34l}[name]
    x = m.uncond_sample((2, 1, 2), temprature=0.5, seed=21)
    assert x.shape == (2, 3, 64, 128) and bool(torch.isfinite(x).all())
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('demo', ['progressive', 'sample', 'interpolate', 'inpaint'])
def test_demo_script(tmp_path, demo):
    script = os.path.join(REPO, 'scripts', 'qresvae', 'generative-demos.py')
    r = subprocess.run([sys.executable, script, demo, '-m', 'qres34m', '--synthetic', '64', '128', '-n', '2', '--out', str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pngs = [f for f in os.listdir(tmp_path) if f.endswith('.png')]
    assert len(pngs) == 1
    if demo == 'progressive':
        import json
        rows = json.load(open(os.path.join(tmp_path, 'qres34m-progressive.json')))
        assert [r['keep'] for r in rows] == list(range(13)) and rows[0]['bpp'] == 0.0
        assert all(a['bpp'] <= b['bpp'] for a, b in zip(rows, rows[1:]))
