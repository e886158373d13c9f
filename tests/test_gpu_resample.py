"""-m gpu: reduced-resolution coding.  The kernels of csrc/resample.hip against the fp64 definition (lvae/utils/resample.py) within a
bound derived from the tables, their 8-bit output against the rounded definition, the bit equalities between the three entry points,
then compress_scaled / decompress_scaled against the calls they are made of (every comparison == or torch.equal), the evaluation
harness and scripts/lvae-codec.py."""
import ctypes
import functools
import io
import os
import pickle
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
from lvae.utils import resample
from lvae.utils.image import ScaledU8Batch, _resample_f32, _tables, load_u8, resize, save_u8, to_float01, to_u8

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# name: (source (h, w), resized (h, w), images, canvas of the fp32 destination or None, misaligned source)
GEOMETRIES = {
    'exact_2to1': ((150, 200), (75, 100), 1, None, False),
    'non_integer': ((150, 200), (61, 77), 1, None, False),
    'upscale': ((61, 77), (150, 200), 1, None, False),
    'down_and_up': ((130, 70), (33, 210), 1, None, False),
    'one_axis': ((150, 200), (150, 100), 1, None, False),
    'truncated_windows': ((9, 13), (3, 5), 1, None, False),         # every window is cut at both borders
    'canvas': ((150, 200), (61, 77), 1, (64, 128), False),
    'misaligned': ((150, 200), (61, 77), 1, None, True),
    'batch_of_3': ((150, 200), (61, 77), 3, None, False),
    'batch_of_17': ((9, 13), (3, 5), 17, None, False),              # 16 images per launch: the chunk loop
    'one_eighth': ((256, 64), (32, 40), 2, None, False),            # 49 taps, 169 input rows per tile: the narrower tile of the 8-bit input
}
ALL_FILTERS = ('exact_2to1', 'non_integer', 'upscale')
CASES = [(g, f) for g in GEOMETRIES for f in (resample.FILTERS if g in ALL_FILTERS else ('lanczos3',))]
# (one_eighth: its derived bound times 255 is 2e-3, beyond the tie band of the 8-bit comparison, so it stays out of that test)
CASES_U8 = [c for c in CASES if c[0] != 'one_eighth']
TIE_BAND, TIE_CAP, TIE_PICK = 1e-3, 0.0025, 0.0022


def _bound(src, dst, filt):
    """(taps_h + taps_v + 4) * 2^-24 * L_h * L_v from the tables the call uses: every tap is one fused multiply-add (one rounding of a
    partial sum bounded by the row's sum of |w|, inputs in [0, 1]), the fp32 weights are the reference's own, and 4 covers the roundings of
    the two results.  An axis that is skipped has no taps and L = 1."""
    taps, L = [], []
    for n_in, n_out in ((src[1], dst[1]), (src[0], dst[0])):
        if n_in == n_out:
            taps.append(0); L.append(1.0)
        else:
            _, w = resample.axis_table(n_in, n_out, filt)
            taps.append(w.shape[1]); L.append(float(np.abs(w.astype(np.float64)).sum(1).max()))
    return (taps[0] + taps[1] + 4) * 2.0 ** -24 * L[0] * L[1]


def _tie_share(ref):
    v = 255.0 * np.clip(ref, 0.0, 1.0)
    near = np.abs(v - np.floor(v) - 0.5) < TIE_BAND
    return near, float(near.mean())


@functools.lru_cache(maxsize=None)
def _case(name, filt):
    """Per case, computed once and left unchanged: seeded torch.rand inputs (the first seed 1, 2, ... whose share of reference values
    within TIE_BAND of a rounding tie is under TIE_PICK -- a property of the inputs, found on the CPU), the fp64 reference, the device views."""
    src, dst, B, canvas, misaligned = GEOMETRIES[name]
    for seed in range(1, 200):
        x = torch.rand(B, 3, *src, generator=torch.Generator().manual_seed(seed))
        ref = resample.resize_reference(x.numpy(), dst[0], dst[1], filt)
        if _tie_share(ref)[1] < TIE_PICK:
            break
    else:
        raise AssertionError('no seed under the tie share')
    if misaligned:                                       # base 4 bytes past a 16-byte boundary, rows of 203 floats, planes 3 floats apart
        row, plane = src[1] + 3, src[0] * (src[1] + 3) + 3
        buf = torch.zeros(1 + 3 * plane, dtype=torch.float32, device=DEV)
        v = buf[1:].as_strided((3, *src), (plane, row, 1))
        v.copy_(x[0])
        assert v.data_ptr() % 16 == 4 and row % 2 == 1
        views = [v]
    else:
        xd = x.to(DEV)
        views = [xd[i] for i in range(B)]
    return dict(src=src, dst=dst, B=B, canvas=canvas, x=x, ref=ref, views=views, seed=seed, bound=_bound(src, dst, filt))


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('name,filt', CASES)
def test_f32_against_the_fp64_definition(name, filt):
    C = _case(name, filt)
    (h, w), canvas = C['dst'], C['canvas']
    out = _resample_f32(C['views'], C['dst'], filt, False, 'f32', canvas=canvas)
    H, W = canvas or (h, w)
    assert tuple(out.shape) == (C['B'], 3, H, W) and out.dtype == torch.float32
    got = out.cpu().numpy()
    err = np.abs(got[:, :, :h, :w].astype(np.float64) - C['ref']).max()
    print(f'{name} {filt}: seed {C["seed"]}, max|d| = {err:.3e}, bound {C["bound"]:.3e}')
    assert err <= C['bound']
    if canvas:                                           # replicate padding: the last row and column again, bit for bit
        assert np.array_equal(got[:, :, h:, :w], np.broadcast_to(got[:, :, h - 1:h, :w], (C['B'], 3, H - h, w)))
        assert np.array_equal(got[:, :, :, w:], np.broadcast_to(got[:, :, :, w - 1:w], (C['B'], 3, H, W - w)))
    if C['src'][0] == h:                                 # the skipped axis is a copy: the rows of the horizontal pass alone
        one = _resample_f32([v[:, 7:8] for v in C['views']], (1, w), filt, False, 'f32')
        assert torch.equal(out[:, :, 7:8], one)
    again = _resample_f32(C['views'], C['dst'], filt, False, 'f32', canvas=canvas)
    assert torch.equal(out, again)                       # no atomics: two calls, the same bits
    if C['B'] > 1:                                       # a batch row is the single call
        for i in (0, C['B'] - 1):
            assert torch.equal(out[i:i + 1], _resample_f32(C['views'][i:i + 1], C['dst'], filt, False, 'f32')), i
    clamped = _resample_f32(C['views'], C['dst'], filt, True, 'f32', canvas=canvas)
    assert torch.equal(clamped, out.clamp(0, 1))


@pytest.mark.parametrize('name,filt', CASES_U8)
def test_u8_against_the_rounded_definition(name, filt):
    """rint(255 * clamp(ref)) except where 255 * ref lies within 1e-3 of a half-integer (the size of the f32 bound times 255: 3e-4 to
    1.1e-3 over these cases): those values, at most 0.25 %, are left out."""
    C = _case(name, filt)
    near, share = _tie_share(C['ref'])
    print(f'{name} {filt}: seed {C["seed"]}, {share:.4%} of the values within {TIE_BAND} of a tie')
    assert share <= TIE_CAP
    out = _resample_f32(C['views'], C['dst'], filt, False, 'u8')
    assert len(out) == C['B'] and all(tuple(o.shape) == (*C['dst'], 3) and o.dtype == torch.uint8 for o in out)
    got = torch.stack(out).cpu().numpy().transpose(0, 3, 1, 2)
    want = np.rint(255.0 * np.clip(C['ref'], 0.0, 1.0)).astype(np.uint8)
    assert np.array_equal(got[~near], want[~near])
    again = _resample_f32(C['views'], C['dst'], filt, False, 'u8')
    assert all(torch.equal(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize('name,filt', [('non_integer', 'lanczos3'), ('non_integer', 'bicubic'), ('upscale', 'lanczos3'), ('one_axis', 'lanczos3'),
                                       ('canvas', 'lanczos3'), ('batch_of_17', 'lanczos3'), ('one_eighth', 'lanczos3')])
def test_entry_points_agree_bit_for_bit(name, filt):
    """u8 in == f32-with-clamp applied to lvae_image_u8_to_f32's output; u8 out == lvae_image_f32_to_u8 applied to f32 out."""
    C = _case(name, filt)
    imgs = [torch.from_numpy(seeded_init.synthetic_image_u8(*C['src'], 90 + i)).to(DEV) for i in range(C['B'])]
    canvas = C['canvas'] or C['dst']
    batch = ScaledU8Batch(imgs, C['dst'], filt, 1, DEV)
    batch.shape = (C['B'], 3, *canvas)
    direct = torch.empty(batch.shape, dtype=torch.float32, device=DEV)
    batch.fill(direct)
    x01 = to_float01(imgs, device=DEV)[0]
    assert torch.equal(direct, _resample_f32([x01[i] for i in range(C['B'])], C['dst'], filt, True, 'f32', canvas=C['canvas']))
    assert float(direct.min()) >= 0.0 and float(direct.max()) <= 1.0
    if C['canvas'] is None:
        assert torch.equal(direct, resize(imgs, C['dst'], filter=filt, clamp=True))
    f32 = _resample_f32(C['views'], C['dst'], filt, False, 'f32')
    u8 = _resample_f32(C['views'], C['dst'], filt, False, 'u8')
    for a, b in zip(u8, to_u8(f32)):
        assert torch.equal(a, b)


def test_same_size_is_the_conversion_alone():
    """Both axes skipped: u8 in is lvae_image_u8_to_f32 (replicate padding included), f32 out a copy, u8 out lvae_image_f32_to_u8."""
    imgs = [torch.from_numpy(seeded_init.synthetic_image_u8(50, 70, 95 + i)) for i in range(2)]
    batch = ScaledU8Batch(imgs, (50, 70), 'lanczos3', 64, DEV)
    assert batch.shape == (2, 3, 64, 128)
    got = torch.empty(batch.shape, dtype=torch.float32, device=DEV)
    batch.fill(got)
    assert torch.equal(got, to_float01(imgs, div=64, device=DEV)[0])
    x = torch.rand(2, 3, 50, 70, generator=torch.Generator().manual_seed(3)).to(DEV) * 1.2 - 0.1
    assert torch.equal(resize(x, (50, 70)), x)
    for a, b in zip(resize(x, (50, 70), out='u8'), to_u8(x)):
        assert torch.equal(a, b)


def test_only_the_destination_is_written():
    """The C entries themselves: an fp32 destination whose images lie 3 * H * W + 41 elements apart, and 8-bit outputs with rows
    3 * w + 5 bytes apart starting 1 byte past an aligned address; every element around the pixels keeps its sentinel."""
    from lvae import _native
    L = _native.lib()
    C = _case('batch_of_3', 'lanczos3')
    (h_in, w_in), (h, w) = C['src'], C['dst']
    tabs = _tables(h_in, w_in, h, w, 'lanczos3', torch.device(DEV))
    xd = torch.stack(C['views'])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W = 64, 80
    big = torch.full((3, 3 * H * W + 41), -7.0, dtype=torch.float32, device=DEV)
    assert L.lvae_resample_f32(xd.data_ptr(), 3 * h_in * w_in, h_in * w_in, w_in, 3, h_in, w_in, h, w, *tabs, 0, big.data_ptr(), big.stride(0),
                               H, W, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:, :3 * H * W].reshape(3, 3, H, W), _resample_f32(C['views'], C['dst'], 'lanczos3', False, 'f32', canvas=(H, W)))
    assert bool((big[:, 3 * H * W:] == -7.0).all())
    row = 3 * w + 5
    bufs = [torch.full((1 + h * row,), 7, dtype=torch.uint8, device=DEV) for _ in range(3)]
    views = [b[1:].as_strided((h, w, 3), (row, 3, 1)) for b in bufs]
    dst = (ctypes.c_void_p * 3)(*[v.data_ptr() for v in views])
    rows = (ctypes.c_long * 3)(row, row, row)
    assert L.lvae_resample_f32_to_u8(xd.data_ptr(), 3 * h_in * w_in, h_in * w_in, w_in, 3, h_in, w_in, h, w, *tabs, dst, rows, st) == 0
    torch.cuda.synchronize()
    want = _resample_f32(C['views'], C['dst'], 'lanczos3', False, 'u8')
    for i in range(3):
        assert torch.equal(views[i], want[i]), i
        mask = torch.ones(bufs[i].numel(), dtype=torch.bool, device=DEV)
        mask[1:].as_strided((h, w, 3), (row, 3, 1)).fill_(False)
        assert bool((bufs[i][mask] == 7).all()), i
    # an 8-bit source read where it lies: rows 3 * w + 5 bytes apart, 1 byte past an aligned address
    u8 = torch.from_numpy(seeded_init.synthetic_image_u8(h_in, w_in, 99))
    srow = 3 * w_in + 5
    sbuf = torch.zeros(1 + h_in * srow, dtype=torch.uint8, device=DEV)
    sview = sbuf[1:].as_strided((h_in, w_in, 3), (srow, 3, 1))
    sview.copy_(u8)
    assert sview.data_ptr() % 4 == 1
    assert torch.equal(resize([sview], (h, w), clamp=True), resize([u8.to(DEV)], (h, w), clamp=True))


def test_a_geometry_that_does_not_fit_is_refused():
    """yspan beyond what the narrowest tile holds in 64 KiB of LDS: -22, nothing is launched.  A yspan above the table's own only
    narrows the tile (400 rows: 8 columns instead of 32): the same bits."""
    from lvae import _native
    x = torch.rand(1, 3, 800, 16, generator=torch.Generator().manual_seed(4)).to(DEV)
    out = torch.full((1, 3, 100, 16), -7.0, device=DEV)
    tabs = list(_tables(800, 16, 100, 16, 'lanczos3', torch.device(DEV)))
    args = lambda span: _native.lib().lvae_resample_f32(x.data_ptr(), 3 * 800 * 16, 800 * 16, 16, 1, 800, 16, 100, 16, tabs[0], tabs[1], tabs[2], span,
                                                        *tabs[4:], 0, out.data_ptr(), 3 * 100 * 16, 100, 16, None)
    assert tabs[3] <= 15 * 8 + 2 * 24 + 2 and args(800) == -22
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert args(tabs[3]) == 0
    torch.cuda.synchronize()
    want = _resample_f32([x[0]], (100, 16), 'lanczos3', False, 'f32')
    assert torch.equal(out, want)
    out.fill_(-7.0)
    assert args(400) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _seeded(name):
    """Seeded weights as scripts/lvae-codec.py --synthetic loads them."""
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


@pytest.fixture(scope='module', params=['qarv_base', 'qres34m'])
def model(request, product_model):
    return (request.param, product_model if request.param == 'qarv_base' else _seeded(request.param))


SIZES = [(128, 192), (120, 180)]


@functools.lru_cache(maxsize=None)
def _image(i):
    return torch.from_numpy(seeded_init.synthetic_image_u8(*SIZES[i], 300 + i))


def _float_path_blob(m, name, im, size, **kw):
    """The model's float-tensor API on a padded (1, 3, H, W) image and the container around it, spelled out."""
    if name == 'qarv_base':
        return struct.pack('2H', *size) + m.compress(im, **kw)
    obj = m.compress(im)
    obj.append(tuple(size))
    buf = io.BytesIO()
    pickle.dump(obj, file=buf)
    return buf.getvalue()


def _decoded_crop(m, payload):
    """The fp32 reconstruction of a payload, cropped to the size in its header: (1, 3, ch, cw)."""
    body, (ch, cw), _ = m._unpack_blob(payload)
    return m.decompress_batch([body])[:, :, :ch, :cw]


@pytest.mark.parametrize('i', [0, 1])
def test_scale_one_is_compress_images(model, i):
    name, m = model
    img = _image(i)
    blob = m.compress_scaled([img], scale=1.0)[0]
    info, payload = resample.unpack_scaled(blob)
    assert info['size'] == info['coded'] == SIZES[i] and info['filter'] == 'lanczos3'
    assert payload == m.compress_images([img])[0]
    got = m.decompress_scaled([blob])[0]
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, m.decompress_images([payload])[0])


@pytest.mark.parametrize('i', [0, 1])
def test_scale_half_is_the_float_path_on_the_resized_image(model, i):
    name, m = model
    img, (h, w) = _image(i), SIZES[i]
    ch, cw = h // 2, w // 2
    blob = m.compress_scaled([img], scale=0.5)[0]
    info, payload = resample.unpack_scaled(blob)
    assert info == dict(filter='lanczos3', size=(h, w), coded=(ch, cw), payload_bytes=len(payload), offset=resample.HEAD_BYTES)
    assert m.compress_scaled([img], size=(ch, cw))[0] == blob
    # the reference: v / 255, the resampler with the clamp, replicate padding to multiples of 64, the float-tensor API, the container
    small = resize(to_float01([img], device=DEV)[0], (ch, cw), clamp=True)
    padded = torch.nn.functional.pad(small, (0, 128 - cw, 0, 64 - ch), mode='replicate')
    assert payload == _float_path_blob(m, name, padded, (ch, cw))
    crop = _decoded_crop(m, payload)
    got = m.decompress_scaled([blob])[0]
    assert tuple(got.shape) == (h, w, 3) and torch.equal(got, to_u8(resize(crop, (h, w)))[0])
    f32 = m.decompress_scaled([blob], out='f32')[0]
    assert tuple(f32.shape) == (1, 3, h, w) and torch.equal(f32, resize(crop, (h, w)))
    assert torch.equal(m.decompress_scaled([blob], size='coded')[0], m.decompress_images([payload])[0])
    assert torch.equal(m.decompress_scaled([blob], out='f32', size='coded')[0], crop)
    preview = m.decompress_scaled([blob], size=(32, 48))[0]
    assert tuple(preview.shape) == (32, 48, 3) and torch.equal(preview, to_u8(resize(crop, (32, 48)))[0])
    assert m.scaled_info(blob)['lmb'] == (float(m.default_lmb) if name == 'qarv_base' else None)


def test_batches_and_filters(model):
    """A batch is the single calls; blobs of two coded sizes and filters in one decompress_scaled call come back in order."""
    name, m = model
    a, b = _image(0), torch.from_numpy(seeded_init.synthetic_image_u8(*SIZES[0], 310))
    pair = m.compress_scaled([a, b], scale=0.5, filter='bicubic')
    assert pair == [m.compress_scaled([a], scale=0.5, filter='bicubic')[0], m.compress_scaled([b], scale=0.5, filter='bicubic')[0]]
    other = m.compress_scaled([_image(1)], scale=0.5)[0]
    assert resample.scaled_info(pair[0])['filter'] == 'bicubic' and pair[0] != m.compress_scaled([a], scale=0.5)[0]
    mixed = [pair[0], other, pair[1]]
    rec = m.decompress_scaled(mixed)
    assert [tuple(r.shape) for r in rec] == [(128, 192, 3), (120, 180, 3), (128, 192, 3)]
    for r, blob in zip(rec, mixed):
        assert torch.equal(r, m.decompress_scaled([blob])[0])
    for kw in ({}, dict(scale=0.5, size=(64, 96)), dict(scale=0.05), dict(size=(8, 96))):
        with pytest.raises(ValueError):
            m.compress_scaled([a], **kw)
    with pytest.raises(ValueError):
        m.compress_scaled([a, _image(1)], scale=0.5)                # one size per call
    with pytest.raises(ValueError):
        m.decompress_scaled([m.compress_images([a])[0]])            # not a scaled container
    with pytest.raises(ValueError):
        m.decompress_scaled([pair[0][:-1]])
    if name != 'qarv_base':
        with pytest.raises(ValueError):
            m.compress_scaled([a], scale=0.5, lmb=64)


def test_per_image_lambdas(product_model):
    m = product_model
    a, b = _image(0), torch.from_numpy(seeded_init.synthetic_image_u8(*SIZES[0], 310))
    pair = m.compress_scaled([a, b], scale=0.5, lmb=[16, 2048])
    assert pair == [m.compress_scaled([a], scale=0.5, lmb=16)[0], m.compress_scaled([b], scale=0.5, lmb=2048)[0]]
    assert [m.scaled_info(p)['lmb'] for p in pair] == [16.0, 2048.0]
    small = resize(to_float01([b], device=DEV)[0], (64, 96), clamp=True)
    padded = torch.nn.functional.pad(small, (0, 32, 0, 0), mode='replicate')
    assert resample.unpack_scaled(pair[1])[1] == _float_path_blob(m, 'qarv_base', padded, (64, 96), lmb=2048)


# ----------------------------------------------------------------------------------------------- callers
def test_evaluation_at_reduced_resolution(product_model, tmp_path):
    import math
    from lvae.evaluation import _mse, imcoding_evaluate
    m = product_model
    folder = tmp_path / 'set'
    folder.mkdir()
    imgs = [_image(0), _image(1), torch.from_numpy(seeded_init.synthetic_image_u8(*SIZES[0], 310))]
    for k, t in enumerate(imgs):
        save_u8(t, folder / f'im{k}.png')
    got = imcoding_evaluate(m, str(folder), scale=0.5)
    assert set(got) == {'bpp', 'mse', 'psnr'} and all(math.isfinite(v) for v in got.values())
    rows = []
    for t in imgs:
        blob = m.compress_scaled([t], scale=0.5)[0]
        real = to_float01([t], device=DEV)[0][0]
        mse = _mse(real, m.decompress_scaled([blob], out='f32')[0])
        rows.append((8 * len(blob) / (t.shape[0] * t.shape[1]), mse, -10 * math.log10(mse)))
    assert got['bpp'] == sum(r[0] for r in rows) / 3
    assert got['mse'] == sum(r[1] for r in rows) / 3 and got['psnr'] == sum(r[2] for r in rows) / 3
    fake = m.decompress_scaled([m.compress_scaled([imgs[1]], scale=0.5)[0]], out='f32')[0].cpu()
    assert tuple(fake.shape) == (1, 3, 120, 180)                    # the errors are taken at the original resolution
    assert rows[1][1] == pytest.approx(float((imgs[1].permute(2, 0, 1).float().div(255) - fake[0]).double().square().mean()), rel=1e-6)
    assert imcoding_evaluate(m, str(folder), scale=0.5, resample='bilinear')['bpp'] != got['bpp']
    with pytest.raises(ValueError):
        imcoding_evaluate(m, str(folder), scale=0.5, tile=(64, 128))


def test_codec_script_at_reduced_resolution(tmp_path):
    """encode --scale and decode as two runs of the script; decode --preview through the script's own decode(), in this process."""
    import importlib.util
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, rec, pre = tmp_path / 'src', tmp_path / 'bits', tmp_path / 'rec', tmp_path / 'pre'
    common = ['-m', 'qarv_base', '--synthetic', '2']
    for cmd in (['encode', str(src), str(bits), '--lmb', '256', '--scale', '0.5'], ['decode', str(bits), str(rec)]):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(bits.glob('*.bits'))
    assert [f.stem for f in files] == ['im00', 'im01']
    m = _seeded('qarv_base')
    spec = importlib.util.spec_from_file_location('lvae_codec_script', script)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    pre.mkdir()
    cli.decode(m, str(bits), str(pre), 8, preview=(32, 48))
    for f in files:
        blob = f.read_bytes()
        orig = load_u8(src / (f.stem + '.png'))
        assert blob[:4] == b'LVRS' and blob == m.compress_scaled([orig], scale=0.5, lmb=256)[0]
        assert m.scaled_info(blob)['lmb'] == 256.0 and m.scaled_info(blob)['size'] == tuple(orig.shape[:2])
        png = load_u8(rec / (f.stem + '.png'))
        assert png.shape == orig.shape and torch.equal(png, m.decompress_scaled([blob])[0].cpu())
        assert torch.equal(load_u8(pre / (f.stem + '.png')), m.decompress_scaled([blob], size=(32, 48))[0].cpu())
