"""Rate maps on the GPU: the position kernels against their definitions (bit for bit, torch fp64 in the definition's order), the
composition kernel against the fp64 torch expression, model.rate_map of the four models against the plans' own buffers, forward() and
the per-channel rate, and scripts/lvae-codec.py ratemap against lvae.evaluation.rate_map_evaluate."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
LOG2E = 1.4426950408889634
BOUND = 0.11


def _lib():
    from lvae import _native
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32)


# ----------------------------------------------------------------------------------------------- the position kernel
def _latent_case(B, HW, z, seed):
    """prm NHWC [B*HW][2z] with log-scales from the floor of the table (scale_bound) to far above it, symbols in +-12 and a few at
    +-200 (there P underflows and the 1e-9 floor holds)."""
    gen = torch.Generator().manual_seed(seed)
    M = B * HW
    prm = torch.cat([torch.randn(M, z, generator=gen) * 2, torch.rand(M, z, generator=gen) * 9 - 5.5], 1).contiguous()
    sym = torch.randint(-12, 13, (B, z, HW), generator=gen, dtype=torch.int32)
    flat = sym.view(-1)
    far = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 50)]
    flat[far] = torch.where(torch.arange(far.numel()) % 2 == 0, 200, -200).to(torch.int32)
    return prm.cuda(), sym.cuda()


def _pos_definition(prm, sym, B, HW, z, cdf_form, bound=BOUND):
    """out[b, p] = the floats lvae_gaussian_nll_map_f32 stores at (b, c, p), widened to fp64 and added channel by channel, c ascending."""
    kl = torch.empty(B, z, HW, device=prm.device)
    assert _lib().lvae_gaussian_nll_map_f32(prm.data_ptr(), sym.data_ptr(), kl.data_ptr(), bound, B, HW, z, cdf_form, _st()) == 0
    acc = torch.zeros(B, HW, dtype=torch.float64, device=prm.device)
    for c in range(z):
        acc = acc + kl[:, c].double()
    return acc, kl


SHAPES = [(1, 1, 8), (3, 15, 8), (2, 96, 32), (1, 231, 96), (2, 1536, 14)]


@pytest.mark.parametrize('cdf_form', [0, 1])
@pytest.mark.parametrize('B,HW,z', SHAPES)
def test_position_kernel_equals_its_definition(B, HW, z, cdf_form):
    L = _lib()
    prm, sym = _latent_case(B, HW, z, 100 * cdf_form + z + HW)
    out = torch.full((B, HW), float('nan'), dtype=torch.float64, device=DEV)
    assert L.lvae_gaussian_nll_pos_f32(prm.data_ptr(), sym.data_ptr(), out.data_ptr(), BOUND, B, HW, z, cdf_form, _st()) == 0
    want, kl = _pos_definition(prm, sym, B, HW, z, cdf_form)
    torch.cuda.synchronize()
    far = kl[sym.abs() == 200]
    assert far.numel() >= 2 and bool((far == far[0]).all()) and abs(float(far[0]) + math.log(1e-9)) < 1e-4       # the 1e-9 floor is hit
    assert torch.equal(_bits(out), _bits(want)), float((out - want).abs().max())
    again = torch.empty_like(out)
    assert L.lvae_gaussian_nll_pos_f32(prm.data_ptr(), sym.data_ptr(), again.data_ptr(), BOUND, B, HW, z, cdf_form, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(out))


@pytest.mark.parametrize('cdf_form', [0, 1])
@pytest.mark.parametrize('B,HW,z', SHAPES)
def test_position_kernel_agrees_with_the_per_channel_kernel(B, HW, z, cdf_form):
    """Per image: sum over positions of the position kernel against sum over channels of lvae_gaussian_nll_chan_f32 -- fp64 sums of the
    same n = HW * z non-negative fp32 terms in two orders.  Each order's sum is within (n - 1) * 2^-53 (relative) of the exact one, so the
    two differ by at most n * 2^-52 relative."""
    L = _lib()
    prm, sym = _latent_case(B, HW, z, 100 * cdf_form + z + HW)
    pos = torch.empty(B, HW, dtype=torch.float64, device=DEV)
    chan = torch.empty(B, z, dtype=torch.float64, device=DEV)
    assert L.lvae_gaussian_nll_pos_f32(prm.data_ptr(), sym.data_ptr(), pos.data_ptr(), BOUND, B, HW, z, cdf_form, _st()) == 0
    assert L.lvae_gaussian_nll_chan_f32(prm.data_ptr(), sym.data_ptr(), chan.data_ptr(), BOUND, B, HW, z, cdf_form, _st()) == 0
    torch.cuda.synchronize()
    a, b = pos.sum(1).cpu(), chan.sum(1).cpu()
    bound = HW * z * 2.0 ** -52
    rel = ((a - b).abs() / b).max().item()
    print(f'pos vs chan {B=} {HW=} {z=} form {cdf_form}: relative difference {rel:.3e}, bound {bound:.3e}')
    assert (b > 0).all() and rel <= bound


# ----------------------------------------------------------------------------------------------- the composition kernel
def _compose(blocks, pix, H, W):
    """The definition of lvae_rate_map_f32 in torch fp64 (every operation rounded on its own), then .float()."""
    B = blocks[0].shape[0] if blocks else pix.shape[0]
    dev = blocks[0].device if blocks else pix.device
    acc = torch.zeros(B, H, W, dtype=torch.float64, device=dev)
    for blk in blocks:
        s = H // blk.shape[1]
        assert blk.shape[1] * s == H and blk.shape[2] * s == W and s & (s - 1) == 0
        up = blk.repeat_interleave(s, 1).repeat_interleave(s, 2)
        acc = acc + up * LOG2E * 2.0 ** (-2 * int(math.log2(s)))
    if pix is not None:
        acc = acc + pix * LOG2E
    return acc.float()


def _rate_map_call(blocks, pix, B, H, W, out, out_img, out_row, ch, cw):
    n = len(blocks)
    pos = (ctypes.c_void_p * max(1, n))(*[t.data_ptr() for t in blocks])
    lh = (ctypes.c_int * max(1, n))(*[t.shape[1] for t in blocks])
    lw = (ctypes.c_int * max(1, n))(*[t.shape[2] for t in blocks])
    return _lib().lvae_rate_map_f32(pos, lh, lw, n, None if pix is None else pix.data_ptr(), B, H, W, out.data_ptr(), out_img, out_row, ch, cw, _st())


@functools.lru_cache(maxsize=None)
def _synthetic_blocks():
    gen = torch.Generator().manual_seed(5)
    B, H, W = 2, 64, 128
    blocks = [(torch.rand(B, H // s, W // s, generator=gen, dtype=torch.float64) * s * s * 3.7).cuda() for s in (64, 32, 32, 16, 4)]
    pix = (torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 11).cuda()
    return B, H, W, blocks, pix


@pytest.mark.parametrize('with_pix', [False, True])
def test_composition_kernel_equals_the_fp64_expression(with_pix):
    B, H, W, blocks, pix = _synthetic_blocks()
    pix = pix if with_pix else None
    out = torch.full((B, 1, H, W), float('nan'), device=DEV)
    assert _rate_map_call(blocks, pix, B, H, W, out, H * W, W, H, W) == 0
    torch.cuda.synchronize()
    want = _compose(blocks, pix, H, W)
    assert torch.equal(_bits(out[:, 0]), _bits(want))
    # over an uncropped map the sum is the size in bits: the blocks' nats times log2 e
    total = sum(float(b.sum()) for b in blocks) + (float(pix.sum()) if with_pix else 0.0)
    assert float(out.double().sum()) == pytest.approx(total * LOG2E, rel=2.0 ** -23)


def test_composition_kernel_cropped_into_a_strided_view():
    B, H, W, blocks, pix = _synthetic_blocks()
    canvas = torch.full((B, 70, 140), -7.0, device=DEV)
    view = canvas[:, 3:53, 9:110]                                      # (B, 50, 101) with strides (70 * 140, 140, 1)
    assert _rate_map_call(blocks, pix, B, H, W, view, view.stride(0), view.stride(1), 50, 101) == 0
    torch.cuda.synchronize()
    want = _compose(blocks, pix, H, W)[:, :50, :101]
    assert torch.equal(_bits(view.contiguous()), _bits(want.contiguous()))
    rest = canvas.clone()
    rest[:, 3:53, 9:110] = -7.0
    assert bool((rest == -7.0).all())                                  # nothing outside the crop is written


def test_composition_kernel_rejects_bad_geometry():
    B, H, W, blocks, pix = _synthetic_blocks()
    out = torch.empty(B, 1, H, W, device=DEV)
    three = torch.zeros(B, 64, 128, dtype=torch.float64, device=DEV)
    assert _rate_map_call([three], None, B, 192, 384, out, H * W, W, H, W) == -22             # ratio 3: no power of two
    narrow = torch.zeros(B, 2, 2, dtype=torch.float64, device=DEV)
    assert _rate_map_call([blocks[0], narrow], None, B, H, W, out, H * W, W, H, W) == -22      # lat_w does not go with lat_h
    assert _rate_map_call(blocks, None, B, H, W, out, H * W, W, H, W) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- the pixel stage
def _lcg01(n, seed):
    """n floats in [0, 1) from a 64-bit LCG in integer arithmetic: the same values on every host, whatever torch's generator does."""
    a, c = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
    x = np.empty(n, np.uint64)
    s = np.uint64(seed)
    with np.errstate(over='ignore'):
        for i in range(n):
            s = s * a + c
            x[i] = s
    return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 24)).astype(np.float32)


PIXEL_CASES = [(2, 9, 13), (1, 16, 40)]


def _pixel_case(B, H, W):
    u = _lcg01(B * H * W * 9, 17 + H)
    n = B * H * W
    mean = (u[:3 * n] * 2.4 - 1.2).reshape(n, 3)
    logs = (u[3 * n:6 * n] * 9 - 8).reshape(n, 3)                      # scales from e^-8 (the Gaussian-density branch) to e
    raw = torch.from_numpy(np.concatenate([mean, logs], 1).astype(np.float32)).contiguous()
    im = torch.from_numpy(np.round(u[6 * n:] * 255).astype(np.float32) / np.float32(255)).view(B, 3, H, W).contiguous()
    return raw.cuda(), im.cuda()


def test_pixel_stage_by_position_and_unchanged_image_sums():
    """lvae_pixel_nll_pos_f32 summed over an image against lvae_pixel_nll_f32's sums[2b] (the same terms in two orders: the bound of the
    latent test with n = 3 * H * W), and lvae_pixel_nll_f32's own outputs == the values the formula gave before its term became a shared
    device function (tests/golden/pixel_nll_sums.json: fp64 bit patterns recorded from the previous build on these inputs)."""
    from lvae import _native
    L = _lib()
    golden = json.load(open(os.path.join(REPO, 'tests', 'golden', 'pixel_nll_sums.json')))
    for B, H, W in PIXEL_CASES:
        raw, im = _pixel_case(B, H, W)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        pos = torch.full((B, H * W), float('nan'), dtype=torch.float64, device=DEV)
        im_hat = torch.empty(B, 3, H, W, device=DEV)
        sums = torch.empty(B, 2, dtype=torch.float64, device=DEV)
        ws = torch.empty(B * _native.EVAL_CHUNKS * 2, dtype=torch.float64, device=DEV)
        assert L.lvae_pixel_nll_pos_f32(raw.data_ptr(), im.data_ptr(), pos.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
        assert L.lvae_pixel_nll_f32(raw.data_ptr(), im.data_ptr(), im_hat.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        a, b = pos.sum(1).cpu(), sums[:, 0].cpu()
        bound = 3 * H * W * 2.0 ** -52
        rel = ((a - b).abs() / b).max().item()
        print(f'pixel pos vs image sums {B=} {H=} {W=}: relative difference {rel:.3e}, bound {bound:.3e}')
        assert (pos >= 0).all() and rel <= bound
        assert _bits(sums.cpu()).view(-1).tolist() == golden[f'{B}x{H}x{W}']
        # position by position: every pixel as a 1 x 1 image of its own through lvae_pixel_nll_f32, whose sums[2b] is then that pixel's
        # three terms added in channel order from 0 -- the definition.  raw6 is one row per pixel already; im becomes [B*H*W][3][1][1].
        n = B * H * W
        im1 = im.view(B, 3, H * W).permute(0, 2, 1).contiguous().view(n, 3, 1, 1)
        hat1, sums1 = torch.empty(n, 3, 1, 1, device=DEV), torch.empty(n, 2, dtype=torch.float64, device=DEV)
        ws1 = torch.empty(n * _native.EVAL_CHUNKS * 2, dtype=torch.float64, device=DEV)
        assert L.lvae_pixel_nll_f32(raw.data_ptr(), im1.data_ptr(), hat1.data_ptr(), sums1.data_ptr(), ws1.data_ptr(), n, 1, 1, None, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(pos.view(-1), sums1[:, 0])
        assert len(set(pos.view(-1).tolist())) > n // 2                      # the positions differ, so a permutation would show
    # a NaN mean is flagged as by lvae_pixel_nll_f32
    raw[5, 1] = float('nan')
    assert L.lvae_pixel_nll_pos_f32(raw.data_ptr(), im.data_ptr(), pos.data_ptr(), B, H, W, status.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == _native.STATUS_NONFINITE_IMAGE


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _seeded(name):
    return _build_seeded(name)


def _build_seeded(name):
    """A new model object with seeded weights as scripts/lvae-codec.py --synthetic loads them."""
    import lvae
    m = lvae.get_model(name, pretrained=False)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m.compress_mode()
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _images(H, W):
    return torch.stack([torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 300 + i)).permute(2, 0, 1).float().div(255) for i in range(2)]).to(DEV)


LMBS = (16.0, 2048.0)
MODEL_CASES = [('qarv_base', 64, 64), ('qarv_base', 128, 192), ('qres34m', 64, 64), ('qres17m', 64, 64), ('qres34m_lossless', 64, 64)]


def _blocks_from_the_plan(m, name, B, H, W):
    """Replay the position plan rate_map just ran (its input and lambdas are still loaded) range by range and take every block's
    definition from the plan's own prm / sym buffers right behind its quantize launch, where `prm` still holds that block."""
    qarv = name == 'qarv_base'
    pl = m._plan('encp', B, H, W, vec=True) if qarv else m._plan('evalp', B, H, W)
    want, lo = [], 0
    with torch.cuda.device(pl.device):
        for li, cut in enumerate(pl.qcuts):
            pl.run(lo, cut)
            lo = cut
            z, hw = pl.lat_shapes[li]
            o = pl.sym_off[li]
            sym = pl.sym_all[o:o + B * z * hw]
            acc, _ = _pos_definition(pl.prm_bufs[li], sym, B, hw, z, 0 if qarv else 1, bound=pl.pk.scale_bound)
            want.append(acc.view(B, *pl.lat_hw[li]))
        torch.cuda.synchronize()
    return want


@pytest.mark.parametrize('name,H,W', MODEL_CASES)
def test_model_rate_map(name, H, W, product_model):
    qarv = name == 'qarv_base'
    m = product_model if qarv else _seeded(name)
    im = _images(H, W)
    B = im.shape[0]
    kw = {'lmb': list(LMBS)} if qarv else {}
    rmap, blocks, im_hat = m.rate_map(im, blocks=True, return_rec=True, **kw)
    assert rmap.shape == (B, 1, H, W) and rmap.dtype == torch.float32 and rmap.device == im.device
    lossless = name == 'qres34m_lossless'
    n_lat = len(blocks) - (1 if lossless else 0)
    # (a) every block tensor is the position kernel's definition on the plan's own buffers
    want = _blocks_from_the_plan(m, name, B, H, W)
    assert len(want) == n_lat
    for li, (got, ref) in enumerate(zip(blocks, want)):
        assert got.dtype == torch.float64 and got.shape == ref.shape and torch.equal(_bits(got), _bits(ref)), li
    if lossless:
        assert blocks[-1].shape == (B, H, W) and blocks[-1].dtype == torch.float64
    # (b) the map is the fp64 composition of the block tensors
    assert torch.equal(_bits(rmap[:, 0]), _bits(_compose(blocks[:n_lat], blocks[-1] if lossless else None, H, W)))
    # (c) the map's mean is the rate forward() / the per-channel kernel report: every entry is an fp64 value rounded to fp32 once
    # (relative 2^-24), so a sum of non-negative entries is within 2^-23 relative of the fp64 sum
    bpp = rmap.double().sum((1, 2, 3)).cpu() / (H * W)
    assert bool((rmap >= 0).all())
    for i in range(B):
        if qarv:
            ref = float(m._estimate_chan(im[i:i + 1], LMBS[i])[1][0]) * LOG2E / (H * W)
        else:
            st = m.forward(im[i:i + 1])
            ref = st['bppix'] + (st['nll'] * 3 * LOG2E if lossless else 0.0)
        rel = abs(float(bpp[i]) - ref) / ref
        print(f'{name} {H}x{W} image {i}: map {float(bpp[i]):.9f} bpp, reference {ref:.9f} bpp, relative difference {rel:.3e}')
        assert rel <= 2.0 ** -23
    # (d) the reconstruction is forward()'s
    fw = m.forward(im, lmb=torch.tensor(LMBS), return_rec=True) if qarv else m.forward(im, return_rec=True)
    assert torch.equal(im_hat, fw['im_hat'])
    # (e) two calls give the same bits
    again = m.rate_map(im, **kw)
    assert torch.equal(_bits(again), _bits(rmap))
    # (f) a batch row with its own lambda is the single call
    if qarv:
        for i in range(B):
            one = m.rate_map(im[i:i + 1], lmb=LMBS[i])
            assert torch.equal(_bits(one[0]), _bits(rmap[i])), i
    # (h), (i)
    if not qarv:
        with pytest.raises(TypeError):
            m.rate_map(im, lmb=3)
    with pytest.raises(AssertionError):
        m.rate_map(im * 1.5, **kw)
    assert torch.equal(_bits(m.rate_map(im, **kw)), _bits(rmap))        # the raise left the plan usable


@pytest.mark.parametrize('name', ['qarv_base', 'qres34m', 'qres17m', 'qres34m_lossless'])
def test_rate_map_of_u8_images(name):
    """(g) the list form: maps at the images' own sizes, equal to the crop of the tensor form on the padded images, and compress_images
    returns the bytes it returned before any rate_map call: the model object is built here, and `before` is its first call."""
    from lvae.utils.image import to_float01
    qarv = name == 'qarv_base'
    m = _build_seeded(name)
    kw = {'lmb': 64.0} if qarv else {}
    imgs = [torch.from_numpy(seeded_init.synthetic_image_u8(50, 101, 310 + i)) for i in range(2)]
    before = m.compress_images(imgs, **kw)
    maps, im_hat = m.rate_map(imgs, return_rec=True, **kw)
    assert [tuple(t.shape) for t in maps] == [(1, 50, 101)] * 2 and [tuple(t.shape) for t in im_hat] == [(3, 50, 101)] * 2
    padded, sizes = to_float01(imgs, div=m.max_stride, device=DEV)
    assert sizes == [(50, 101)] * 2 and padded.shape == (2, 3, 64, 128)
    full, rec = m.rate_map(padded, return_rec=True, **kw)
    for i in range(2):
        assert torch.equal(_bits(maps[i].contiguous()), _bits(full[i, :, :50, :101].contiguous())), i
        assert torch.equal(im_hat[i], rec[i, :, :50, :101])
    assert m.compress_images(imgs, **kw) == before
    with pytest.raises(AssertionError):
        m.rate_map([imgs[0], torch.zeros(70, 101, 3, dtype=torch.uint8)], **kw)       # padded sizes differ


# ----------------------------------------------------------------------------------------------- evaluation and the script
def test_ratemap_script_against_rate_map_evaluate(tmp_path):
    """scripts/lvae-codec.py ratemap --synthetic 2 as its own process; the .npy files it leaves sum to the bits rate_map_evaluate returns
    in this process for the PNGs it wrote."""
    from lvae.evaluation import rate_map_evaluate
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, out = tmp_path / 'src', tmp_path / 'maps'
    r = subprocess.run([sys.executable, script, 'ratemap', str(src), str(out), '-m', 'qres17m', '--synthetic', '2'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert sorted(p.name for p in out.iterdir()) == ['im00.npy', 'im00.png', 'im01.npy', 'im01.png']
    m = _seeded('qres17m')
    rows = rate_map_evaluate(m, str(src))
    assert [r_['name'] for r_ in rows] == ['im00', 'im01']
    for row, (h, w) in zip(rows, [(120, 180), (128, 192)]):
        arr = np.load(out / f"{row['name']}.npy")
        assert arr.dtype == np.float32 and arr.shape == (h, w)
        # the same fp32 map, summed in fp64 in another order: n non-negative terms, at most n * 2^-52 apart (relative)
        assert abs(float(arr.astype(np.float64).sum()) - row['bits']) <= arr.size * 2.0 ** -52 * row['bits']
        assert len(row['shares']) == len(m._latent_blocks()) and sum(row['shares']) == pytest.approx(1.0, abs=1e-9)
        assert f"{row['name']}: " in r.stdout
    from PIL import Image
    png = np.asarray(Image.open(out / 'im00.png'))
    assert png.shape == (120, 180) and png.dtype == np.uint8 and png.max() == 255
