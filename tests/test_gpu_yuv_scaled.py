"""-m gpu: YUV frames at reduced resolution.  The fused kernels of csrc/resample_yuv.hip against the composition of the existing entries
they replace -- lvae_image_yuv*_to_f32 then lvae_resample_f32(clamp=1, canvas) on the way in, lvae_resample_f32(clamp=0) then
lvae_image_f32_to_yuv* on the way out -- and compress_yuv_scaled / decompress_yuv_scaled, the sequence container, the evaluation harness and
scripts/lvae-codec.py against the calls they are made of.  Every comparison is == or torch.equal: no tolerance anywhere."""
import functools
import io
import math
import os
import pickle
import struct
import subprocess
import sys

import pytest
import torch

import seeded_init
from lvae.utils import resample, yuvseq
from lvae.utils.image import _resample_f32, resize
from lvae.utils.yuv import (FrameFormat, ScaledYuvBatch, from_rgb01_any, from_rgb01_scaled, to_rgb01_any, to_rgb01_scaled, write_frames)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# name: (layout, depth, subsampling, siting, matrix, range)
KINDS = {
    'i420': ('i420', 8, '420', 'center', 'bt601', 'limited'),
    'nv12': ('nv12', 8, '420', 'center', 'bt709', 'full'),
    '420p10_left': ('planar', 10, '420', 'left', 'bt2020', 'limited'),
    'p010': ('semiplanar', 10, '420', 'center', 'bt709', 'limited'),
    '422p12_left': ('planar', 12, '422', 'left', 'bt709', 'full'),
    'p210': ('semiplanar', 10, '422', 'left', 'bt2020', 'limited'),
    '444p8': ('planar', 8, '444', 'center', 'bt709', 'limited'),
}
# name: (frame (h, w), resized (h, w), frames, canvas of the fp32 destination or None, filter) -- the way out runs them backwards
GEOMETRIES = {
    'non_integer': ((70, 98), (37, 53), 2, (64, 64), 'lanczos3'),   # width % 4 == 2, more than one tile each way, remainders, a padded canvas
    'odd_444': ((45, 67), (23, 34), 1, None, 'bicubic'),
    'upscale': ((48, 64), (72, 96), 1, None, 'bilinear'),
    'copy_rows': ((64, 96), (64, 48), 1, None, 'lanczos3'),
    'copy_columns': ((64, 96), (32, 96), 1, None, 'bicubic'),
    'same_size': ((64, 96), (64, 96), 2, None, 'lanczos3'),
    'one_eighth': ((256, 40), (32, 16), 1, None, 'lanczos3'),       # 49 taps, 169 input rows per tile: the narrower tile
    'batch_of_17': ((16, 16), (8, 8), 17, None, 'bicubic'),         # 16 frames per launch: the chunk loop
}
CASES = [(k, g) for g in GEOMETRIES for k in KINDS if (g != 'odd_444' or k == '444p8')]
SENTINEL = 77


def _fits(size, sub):
    return yuvseq._extent_ok(size[0], size[1], sub)


def _fmt(kind):
    layout, depth, sub, siting, matrix, _ = KINDS[kind]
    return FrameFormat(layout, depth, sub, siting, matrix)


def _colour(kind):
    _, _, _, siting, matrix, rng = KINDS[kind]
    return dict(siting=siting, matrix=matrix, range=rng)


def _guarded_frame(fmt, h, w, fill=None):
    """A frame of `fmt` whose planes are views, with row strides above their widths, cut from sentinel-filled tensors on the device (the
    base 2 samples in: misaligned for every vector width) -> (frame, the backing tensors)."""
    backs, planes = [], []
    for shape in ((h, w),) + fmt._chroma_shapes(h, w):
        cols = shape[1] * (2 if len(shape) == 3 else 1)
        back = torch.full((shape[0] + 2, cols + 5), SENTINEL, dtype=fmt.dtype, device=DEV)
        view = back[1:1 + shape[0], 2:2 + cols]
        if fill is not None:
            view.copy_(fill(shape[0], cols))
        backs.append(back)
        planes.append(view.unflatten(1, (shape[1], 2)) if len(shape) == 3 and fmt.layout == 'nv12' else view)
    return fmt.frame(*planes, scan=False), backs


def _sentinels_intact(backs):
    for back in backs:
        inner = torch.zeros_like(back, dtype=torch.bool)
        inner[1:-1, 2:-3] = True
        if not bool((back[~inner] == SENTINEL).all()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _frames(kind, geom):
    """Seeded frames of the case, computed once and left unchanged: random codes in every bit of the container (low bits of a semi-planar
    word, high bits of a planar one: the kernels mask them)."""
    fmt, ((h, w), _, B, _, _) = _fmt(kind), GEOMETRIES[geom]
    g = torch.Generator().manual_seed(11 + len(kind) + len(geom))

    def fill(rows, cols):
        hi = 256 if fmt.depth == 8 else 65536
        t = torch.randint(0, hi, (rows, cols), generator=g)
        return (t.to(torch.uint8) if fmt.depth == 8 else (t - 65536 * (t >= 32768)).to(torch.int16)).to(DEV)
    return [_guarded_frame(fmt, h, w, fill) for _ in range(B)]


# ----------------------------------------------------------------------------------------------- kernels: the way in
@pytest.mark.parametrize('chroma', ['nearest', 'bilinear'])
@pytest.mark.parametrize('kind,geom', CASES)
def test_in_is_the_conversion_then_the_resampler(kind, geom, chroma):
    (h, w), size, B, canvas, filt = GEOMETRIES[geom]
    guarded, kw = _frames(kind, geom), dict(_colour(kind), chroma=chroma)
    frames = [f for f, _ in guarded]
    rgb = to_rgb01_any(frames, 1, DEV, kw['matrix'], kw['range'], chroma, kw['siting'])[0]            # lvae_image_yuv*_to_f32
    want = _resample_f32([rgb[i] for i in range(B)], size, filt, True, 'f32', canvas)                # lvae_resample_f32(clamp=1)
    H, W = canvas or size
    big = torch.full((B + 2, 3, H, W), -7.0, device=DEV)
    batch = ScaledYuvBatch(_fmt(kind), frames, size, filt, 1, DEV, kw['matrix'], kw['range'], chroma, kw['siting'], canvas=canvas)
    assert batch.shape == (B, 3, H, W) and batch.sizes == [size] * B
    batch.fill(big[1:B + 1])
    torch.cuda.synchronize()
    assert torch.equal(big[1:B + 1], want)
    assert bool((big[0] == -7.0).all()) and bool((big[-1] == -7.0).all())
    assert all(_sentinels_intact(backs) for _, backs in guarded)
    assert torch.equal(to_rgb01_scaled(frames, size, filt, canvas, **kw), want)
    if geom == 'same_size':                                  # the plain conversion's bits
        assert torch.equal(want, rgb)


def test_in_batch_rows_are_single_calls():
    frames = [f for f, _ in _frames('420p10_left', 'non_integer')]
    both = to_rgb01_scaled(frames, (37, 53), 'bicubic', (64, 64), **_colour('420p10_left'))
    for i, f in enumerate(frames):
        assert torch.equal(both[i:i + 1], to_rgb01_scaled([f], (37, 53), 'bicubic', (64, 64), **_colour('420p10_left')))


# ----------------------------------------------------------------------------------------------- kernels: the way out
@functools.lru_cache(maxsize=None)
def _rgb(geom):
    """The decoder's side of a case: views of a padded batch, values beyond [0, 1] and a few NaNs."""
    _, (h, w), B, _, _ = GEOMETRIES[geom]
    x = torch.rand(B, 3, h + 5, w + 7, generator=torch.Generator().manual_seed(5 + len(geom))) * 1.4 - 0.2
    x[0, 0, 1, 2] = x[0, 1, h - 1, w - 1] = x[B - 1, 2, h // 2, 0] = float('nan')
    x[0, :, 0, 0] = torch.tensor([-3.0, 9.0, 0.5])
    x = x.to(DEV)
    return x, [x[i, :, :h, :w] for i in range(B)]


@pytest.mark.parametrize('kind,geom', [(k, g) for k, g in CASES if _fits(GEOMETRIES[g][0], KINDS[k][2])])
def test_out_is_the_resampler_then_the_conversion(kind, geom):
    size, _, B, _, filt = GEOMETRIES[geom]                   # backwards: the frame's size is the target
    layout, depth, sub, siting, matrix, rng = KINDS[kind]
    how = dict(depth=depth, subsampling=sub, siting=siting, matrix=matrix, range=rng, layout=layout)
    x, views = _rgb(geom)
    before = x.clone()
    mid = _resample_f32(views, size, filt, False, 'f32')                                             # lvae_resample_f32(clamp=0)
    want = from_rgb01_any(mid, None, **how)                                                          # lvae_image_f32_to_yuv*
    fmt = _fmt(kind)
    guarded = [_guarded_frame(fmt, *size) for _ in range(B)]
    got = from_rgb01_scaled(views, size, filt, outs=[f for f, _ in guarded], **how)
    torch.cuda.synchronize()
    fresh = from_rgb01_scaled(views, size, filt, **how)
    for g, f, wnt, (_, backs) in zip(got, fresh, want, guarded):
        assert FrameFormat.of(g) == FrameFormat.of(wnt) == fmt and g.size == size
        for pg, pf, pw in zip(g.planes(), f.planes(), wnt.planes()):                                 # plane by plane
            assert torch.equal(pg, pw) and torch.equal(pf, pw)
        assert _sentinels_intact(backs)
    assert torch.equal(x.isnan(), before.isnan()) and torch.equal(x.nan_to_num(), before.nan_to_num())


def test_out_halo_column_comes_from_the_neighbouring_tile():
    """37x53 -> 70x98 with left-sited chroma: tiles 1 .. 3 of a row start at columns 32, 64, 96 and their first chroma sample reads the
    resized column before; a tile that took its own first column instead would differ in chroma column 16 | 32 | 48."""
    x, views = _rgb('non_integer')
    how = dict(depth=10, subsampling='420', siting='left', matrix='bt709', range='limited')
    got = from_rgb01_scaled(views, (70, 98), 'lanczos3', **how)
    want = from_rgb01_any(_resample_f32(views, (70, 98), 'lanczos3', False, 'f32'), None, **how)
    centre = from_rgb01_scaled(views, (70, 98), 'lanczos3', **dict(how, siting='center'))
    for g, wnt, c in zip(got, want, centre):
        assert torch.equal(g.u[:, [16, 32, 48]], wnt.u[:, [16, 32, 48]]) and torch.equal(g.v, wnt.v) and torch.equal(g.u, wnt.u)
        assert not torch.equal(g.u, c.u)                     # the siting is not ignored


def test_a_geometry_that_does_not_fit_is_refused():
    """A yspan beyond what the narrowest tile holds in 64 KiB of LDS: -22 from both entries, nothing is launched, nothing is written."""
    fmt = FrameFormat('planar', 8, '420')
    frame, _ = _guarded_frame(fmt, 800, 16, lambda r, c: torch.randint(0, 256, (r, c), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(DEV))
    batch = ScaledYuvBatch(fmt, [frame], (100, 16), 'lanczos3', 1, DEV)
    out = torch.full((1, 3, 100, 16), -7.0, device=DEV)
    want = to_rgb01_scaled([frame], (100, 16))
    tabs = batch._tabs
    batch._tabs = tabs[:3] + (800,) + tabs[4:]
    with pytest.raises(RuntimeError, match='-22'):
        batch.fill(out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    batch._tabs = tabs[:3] + (400,) + tabs[4:]               # a yspan above the table's own only narrows the tile: the same bits
    batch.fill(out)
    assert torch.equal(out, want)
    # the way out, 800 x 16 -> 100 x 16, with the same forged yspan
    from lvae import _native
    from lvae.utils import yuv as Y
    x = torch.rand(1, 3, 800, 16, generator=torch.Generator().manual_seed(2)).to(DEV)
    dst, backs = _guarded_frame(fmt, 100, 16)
    codes, names, lay = Y._kind_codes(fmt, 'center', 'bt709', 'limited')
    tabs, _ = Y._scaled_tables((800, 16), (100, 16), 'lanczos3', torch.device(DEV))
    ptrs, rows, hw, _ = Y._plane_args([dst], names)
    call = lambda span: _native.lib().lvae_resample_f32_to_yuv(x.data_ptr(), 3 * 800 * 16, 800 * 16, 16, hw, 1, *codes, lay, 800, 16, 100, 16, tabs[0],
                                                               tabs[1], tabs[2], span, *tabs[4:], *ptrs, *rows, None)
    assert call(800) == -22
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in backs)
    assert call(tabs[3]) == 0
    torch.cuda.synchronize()
    ref = from_rgb01_scaled(x, (100, 16))[0]
    assert torch.equal(dst.y, ref.y) and torch.equal(dst.u, ref.u) and torch.equal(dst.v, ref.v)


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


H, W = 128, 192
HOW = dict(depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited')
ENC = dict(siting='left', matrix='bt2020', range='limited', chroma='bilinear')


@functools.lru_cache(maxsize=None)
def _frame(i):
    """Frame i of the model tests: a seeded image as a 10-bit 4:2:0 left-sited frame on the device."""
    rgb = torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 300 + i)).permute(2, 0, 1).float().div(255)
    return from_rgb01_any([rgb], **HOW)[0].to(DEV)


def _float_path_blob(m, name, im, size, **kw):
    """The model's float-tensor API on a padded (1, 3, H, W) image and the container around it, spelled out."""
    if name == 'qarv_base':
        return struct.pack('2H', *size) + m.compress(im, **kw)
    obj = m.compress(im)
    obj.append(tuple(size))
    buf = io.BytesIO()
    pickle.dump(obj, file=buf)
    return buf.getvalue()


def _same_frames(a, b):
    return FrameFormat.of(a) == FrameFormat.of(b) and a.size == b.size and all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))


def test_scale_half_is_the_float_path_on_the_resized_frame(model):
    name, m = model
    f = _frame(0)
    blob = m.compress_yuv_scaled([f], scale=0.5, **ENC)[0]
    info, payload = resample.unpack_scaled(blob)
    assert info == dict(filter='lanczos3', size=(H, W), coded=(64, 96), payload_bytes=len(payload), offset=resample.HEAD_BYTES)
    assert m.compress_yuv_scaled([f], size=(64, 96), **ENC)[0] == blob
    small = resize(to_rgb01_any([f], 1, DEV, 'bt2020', 'limited', 'bilinear', 'left')[0], (64, 96), clamp=True)
    padded = torch.nn.functional.pad(small, (0, 32, 0, 0), mode='replicate')
    assert payload == _float_path_blob(m, name, padded, (64, 96))
    assert m.compress_yuv_scaled([f.to_semiplanar()], scale=0.5, **ENC)[0] == blob                   # the P010 twin
    assert m.scaled_info(blob)['lmb'] == (float(m.default_lmb) if name == 'qarv_base' else None)
    # the way back
    got = m.decompress_yuv_scaled([blob], **HOW)[0]
    want = from_rgb01_any(m.decompress_scaled([blob], out='f32'), **HOW)[0]
    assert got.size == (H, W) and _same_frames(got, want)
    assert _same_frames(m.decompress_yuv_scaled([blob], layout='semiplanar', **HOW)[0], want.to_semiplanar())
    assert _same_frames(m.decompress_yuv_scaled([blob], size='coded', **HOW)[0], m.decompress_yuv([payload], **HOW)[0])
    pre = m.decompress_yuv_scaled([blob], size=(32, 48), **HOW)[0]
    assert pre.size == (32, 48) and _same_frames(pre, from_rgb01_any(m.decompress_scaled([blob], out='f32', size=(32, 48)), **HOW)[0])
    with pytest.raises(ValueError, match='420'):
        m.decompress_yuv_scaled([blob], size=(33, 48), **HOW)


def test_scale_one_is_compress_yuv(model):
    name, m = model
    f = _frame(1)
    blob = m.compress_yuv_scaled([f], scale=1.0, **ENC)[0]
    info, payload = resample.unpack_scaled(blob)
    assert info['size'] == info['coded'] == (H, W) and payload == m.compress_yuv([f], **ENC)[0]


def test_batches_lambdas_and_argument_checks(model):
    name, m = model
    fs = [_frame(0), _frame(1), _frame(2)]
    trio = m.compress_yuv_scaled(fs, scale=0.5, filter='bicubic', **ENC)
    assert trio == [m.compress_yuv_scaled([f], scale=0.5, filter='bicubic', **ENC)[0] for f in fs]
    rec = m.decompress_yuv_scaled(trio, **HOW)
    for r, b in zip(rec, trio):
        assert _same_frames(r, m.decompress_yuv_scaled([b], **HOW)[0])
    if name == 'qarv_base':
        pair = m.compress_yuv_scaled(fs[:2], scale=0.5, lmb=[16, 2048], **ENC)
        assert pair == [m.compress_yuv_scaled([fs[0]], scale=0.5, lmb=16, **ENC)[0], m.compress_yuv_scaled([fs[1]], scale=0.5, lmb=2048, **ENC)[0]]
        assert [m.scaled_info(p)['lmb'] for p in pair] == [16.0, 2048.0]
    else:
        with pytest.raises(ValueError):
            m.compress_yuv_scaled(fs[:1], scale=0.5, lmb=64, **ENC)
    for kw in ({}, dict(scale=0.5, size=(64, 96)), dict(scale=0.05)):
        with pytest.raises(ValueError):
            m.compress_yuv_scaled(fs[:1], **kw, **ENC)
    with pytest.raises(ValueError):
        m.compress_yuv_scaled([fs[0], fs[1].to_semiplanar()], scale=0.5, **ENC)


def test_sequences_at_reduced_resolution(product_model):
    m = product_model
    fs = [_frame(0), _frame(1), _frame(2)]
    seq = m.compress_yuv_sequence(fs, scale=0.5, lmb=[16, 256, 2048], max_batch=2, **ENC)
    info, entries = yuvseq.unpack_sequence(seq)
    assert (info['height'], info['width'], info['depth'], info['siting'], info['matrix']) == (H, W, 10, 'left', 'bt2020')
    assert entries == [m.compress_yuv_scaled([f], scale=0.5, lmb=v, **ENC)[0] for f, v in zip(fs, (16, 256, 2048))]
    assert m.yuv_sequence_info(seq)['lmb'] == [16.0, 256.0, 2048.0]
    for mb in (1, 3):                                        # the container does not depend on the batching
        assert m.compress_yuv_sequence(fs, scale=0.5, lmb=[16, 256, 2048], max_batch=mb, **ENC) == seq
    rec = m.decompress_yuv_sequence(seq)                     # no colour parameter
    for r, b in zip(rec, entries):
        assert r.size == (H, W) and _same_frames(r, m.decompress_yuv_scaled([b], **HOW)[0])
    assert _same_frames(m.decompress_yuv_sequence(seq, frames=[2])[0], rec[2])
    plain = m.compress_yuv_sequence(fs, **ENC)               # scale=None: the entries are compress_yuv's
    assert yuvseq.unpack_sequence(plain)[1] == m.compress_yuv(fs, **ENC)
    with pytest.raises(ValueError):
        m.compress_yuv_sequence(fs, scale=0.5, tile=(64, 128), **ENC)


def test_evaluation_at_reduced_resolution(product_model, tmp_path):
    from lvae.evaluation import yuv_evaluate
    from lvae.metrics import psnr_yuv
    m = product_model
    fs = [_frame(0), _frame(1)]
    path = str(tmp_path / 'in.yuv')
    write_frames(fs, path)
    kw = dict(depth=10, siting='left', matrix='bt2020', range='limited')
    plain = yuv_evaluate(m, path, W, H, **kw)
    got = yuv_evaluate(m, path, W, H, scale=0.5, **kw)
    assert set(got) == set(plain) and all(math.isfinite(v) for v in got.values())
    blobs = m.compress_yuv_scaled(fs, scale=0.5, **ENC)
    assert got['bpp'] == sum(8 * len(b) / (H * W) for b in blobs) / 2                                # against the ORIGINAL pixel count
    rows = psnr_yuv(fs, m.decompress_yuv_scaled(blobs, **HOW))
    assert got['psnr-y'] == sum(r['psnr-y'] for r in rows) / 2
    assert yuv_evaluate(m, path, W, H, scale=0.5, resample='bilinear', **kw)['bpp'] != got['bpp']
    with pytest.raises(ValueError):
        yuv_evaluate(m, path, W, H, scale=0.5, tile=(64, 128), **kw)


def test_codec_script_at_reduced_resolution(tmp_path):
    """encode-yuv --scale and decode-yuv as two runs of the script, folder mode; --container and --preview through the script's own
    functions, in this process."""
    import importlib.util
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, rec = tmp_path / 'in.yuv', tmp_path / 'bits', tmp_path / 'rec.yuv'
    common = ['-m', 'qarv_base', '--synthetic', '2', '--depth', '10', '--siting', 'left', '--lmb', '256']
    for cmd in (['encode-yuv', str(src), str(bits), '--size', str(W), str(H), '--scale', '0.5', '--filter', 'bicubic'],
                ['decode-yuv', str(bits), str(rec)]):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = _seeded('qarv_base')
    fmt = FrameFormat('planar', 10, '420', 'left')
    frames = fmt.read(str(src), W, H)
    files = sorted(bits.glob('*.bits'))
    assert len(files) == len(frames) == 2
    colour = dict(siting='left', matrix='bt709', range='limited', chroma='bilinear')
    how = dict(depth=10, subsampling='420', siting='left', matrix='bt709', range='limited')
    blobs = [f.read_bytes() for f in files]
    assert blobs == m.compress_yuv_scaled(frames, scale=0.5, filter='bicubic', lmb=256, **colour)
    assert all(m.scaled_info(b)['filter'] == 'bicubic' and b[:4] == b'LVRS' for b in blobs)
    for got, want in zip(fmt.read(str(rec), W, H), m.decompress_yuv_scaled(blobs, **how)):
        assert _same_frames(got, want.cpu())
    spec = importlib.util.spec_from_file_location('lvae_codec_script', script)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    pre = tmp_path / 'pre.yuv'
    cli.decode_yuv(m, str(bits), str(pre), fmt, 8, colour, preview=(32, 48))
    for got, want in zip(fmt.read(str(pre), 48, 32), m.decompress_yuv_scaled(blobs, size=(32, 48), **how)):
        assert _same_frames(got, want.cpu())
    box, out = tmp_path / 'seq.lvys', tmp_path / 'seq.yuv'
    cli.encode_yuv_container(m, str(src), str(box), (W, H), fmt, None, 256, 8, colour, scale=0.5, filt='bicubic')
    assert yuvseq.unpack_sequence(box.read_bytes())[1] == blobs
    cli.decode_yuv_container(m, str(box), str(out), 8)
    assert out.read_bytes() == rec.read_bytes()
    cli.decode_yuv_container(m, str(box), str(out), 8, preview=(32, 48))
    assert out.read_bytes() == pre.read_bytes()
