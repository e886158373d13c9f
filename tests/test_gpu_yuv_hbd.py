"""-m gpu: planar YUV frames of 8 / 10 / 12 bits at 4:2:0 / 4:2:2 / 4:4:4 with centre- or left-sited chroma, end to end.  The three kernels of
csrc/yuv_io.hip against the CPU expressions that define them (lvae/utils/yuv.py; torch.equal / ==: every bit), then the model-level API
against the float path spelled out here, yuv_evaluate against its per-frame loop, and scripts/lvae-codec.py encode-yuv / decode-yuv with
--depth 10 against decompress_yuv."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
import yuv_hbd_ref as ref
from conftest import load_seeded_into
from lvae.metrics import psnr_yuv, psnr_yuv420, sse_u16
from lvae.utils.yuv import (YuvBatch, YuvFrame, from_rgb01, from_rgb01_any, read_yuv, read_yuv420, to_rgb01_any, write_yuv, write_yuv420)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
EXTENTS = [(2, 2), (6, 10), (62, 70), (64, 128)]             # widths that are no multiple of 4, the right-edge path, rows / columns beyond


def _extents(sub):
    return EXTENTS + ([(5, 7)] if sub == '444' else [])


def _frame(planes, depth, sub, device='cpu'):
    return YuvFrame(*planes, depth=depth, subsampling=sub).to(device)


def _planes_equal(a, b):
    return (a.depth, a.subsampling, a.size) == (b.depth, b.subsampling, b.size) and all(torch.equal(p.cpu(), q.cpu()) for p, q in zip(a.planes(), b.planes()))


# ----------------------------------------------------------------------------------------------- lvae_image_yuv_to_f32
@pytest.mark.parametrize('sub,siting', ref.LAYOUTS)
def test_yuv_to_f32_extent_to_canvas(sub, siting):
    for extent in _extents(sub):
        fr = _frame(ref.noise_planes(*extent, 10, sub, 11), 10, sub)
        for chroma in ('bilinear', 'nearest'):
            want, _ = to_rgb01_any([fr], div=64, siting=siting, chroma=chroma)          # the CPU expression, replicate-padded
            assert tuple(want.shape) == (1, 3, 64, 128 if extent[1] > 64 else 64)
            x, sizes = to_rgb01_any([fr], div=64, device=DEV, siting=siting, chroma=chroma)
            assert sizes == [extent] and x.is_cuda and x.dtype == torch.float32
            assert torch.equal(x.cpu(), want), (extent, chroma)


@pytest.mark.parametrize('sub,siting', ref.LAYOUTS)
def test_yuv_to_f32_batch_of_three_extents(sub, siting):
    sizes = [(6, 10), (62, 70), (64, 128)]
    frames = [_frame(ref.noise_planes(h, w, 10, sub, 20 + i), 10, sub) for i, (h, w) in enumerate(sizes)]
    want, _ = to_rgb01_any(frames, div=64, siting=siting)
    x, got = to_rgb01_any([f.to(DEV) for f in frames], div=64, siting=siting)
    assert got == sizes and tuple(x.shape) == (3, 3, 64, 128) and x.is_cuda
    assert torch.equal(x.cpu(), want)


@pytest.mark.parametrize('sub', ['420', '422', '444'])
@pytest.mark.parametrize('depth', [8, 10])
def test_yuv_to_f32_strided_misaligned_planes(depth, sub):
    """Planes that are views of a larger buffer: rows 5 samples longer than the plane, bases one sample past an aligned address (the
    scalar-load fallback of the 4-sample luma load); read in place."""
    h, w = 6, 12
    planes = ref.noise_planes(h, w, depth, sub, 31)

    def view(p):
        p = torch.from_numpy(p.view(np.int16) if depth > 8 else p)
        row = p.shape[1] + 5
        buf = torch.zeros(1 + p.shape[0] * row, dtype=p.dtype, device=DEV)
        v = buf[1:].as_strided(tuple(p.shape), (row, 1))
        v.copy_(p)
        assert v.data_ptr() % 8 == p.element_size()
        return v
    fr = YuvFrame(*(view(p) for p in planes), depth=depth, subsampling=sub)
    for siting in ('center', 'left'):
        b = YuvBatch([fr], 64, DEV, siting=siting)
        out = torch.empty(b.shape, dtype=torch.float32, device=DEV)
        b.fill(out)
        assert b.frames[0].y.data_ptr() == fr.y.data_ptr()
        assert torch.equal(out.cpu(), to_rgb01_any([_frame(planes, depth, sub)], div=64, siting=siting)[0])


@pytest.mark.parametrize('gap', [40, 41])
def test_yuv_to_f32_writes_only_its_planes(gap):
    """A destination whose image stride exceeds 3 * H * W (gap 41: also off the 16-byte grid, the scalar-store path), guard words around it."""
    H = W = 8
    for sub, siting in (('420', 'left'), ('444', 'center')):
        frames = [_frame(ref.noise_planes(h, w, 10, sub, 40 + i), 10, sub) for i, (h, w) in enumerate([(6, 4), (8, 8)])]
        big = torch.full((4 + 2 * (3 * H * W + gap),), -7.0, dtype=torch.float32, device=DEV)
        body = big[4:].view(2, 3 * H * W + gap)
        YuvBatch(frames, 8, DEV, siting=siting).fill(body[:, :3 * H * W].view(2, 3, H, W))
        got = big.cpu()
        inner = got[4:].view(2, 3 * H * W + gap)
        assert torch.equal(inner[:, :3 * H * W].reshape(2, 3, H, W), to_rgb01_any(frames, div=8, siting=siting)[0])
        assert bool((inner[:, 3 * H * W:] == -7.0).all()) and bool((got[:4] == -7.0).all())


@pytest.mark.parametrize('sub,siting', [('420', 'center'), ('420', 'left'), ('422', 'left'), ('444', 'center')])
@pytest.mark.parametrize('depth', ref.DEPTHS)
def test_yuv_to_f32_every_code_and_colour_parameters(depth, sub, siting):
    """Ramps in which every code of Y, U and V occurs, next to noise: nearest and bilinear, both ranges, the three matrices."""
    frames = [_frame(ref.ramp_planes(depth, sub), depth, sub), _frame(ref.noise_planes(128, 128, depth, sub, 12), depth, sub)]
    for p in frames[0].planes():
        assert len(torch.unique(p)) == 1 << depth
    dev = [f.to(DEV) for f in frames]
    for matrix in ref.MATRICES:
        for rng in ref.RANGES:
            for chroma in ('nearest', 'bilinear'):
                kw = dict(matrix=matrix, range=rng, chroma=chroma, siting=siting)
                assert torch.equal(to_rgb01_any(dev, **kw)[0].cpu(), to_rgb01_any(frames, **kw)[0]), kw


def test_8_bit_420_centre_equals_the_yuv420_entry():
    import yuv_ref
    from lvae.utils.yuv import Yuv420Frame, to_rgb01
    planes = yuv_ref.noise_planes(62, 70, 13)
    old = Yuv420Frame('i420', *(torch.from_numpy(p) for p in planes)).to(DEV)
    new = _frame(planes, 8, '420', DEV)
    for chroma in ('nearest', 'bilinear'):
        assert torch.equal(to_rgb01_any([new], div=64, matrix='bt601', range='full', chroma=chroma)[0],
                           to_rgb01([old], div=64, matrix='bt601', range='full', chroma=chroma)[0])


# ----------------------------------------------------------------------------------------------- lvae_image_f32_to_yuv
@pytest.fixture(scope='module')
def f32_batch():
    """(3, 3, 128, 128) fp32 in [-0.1, 1.1] with exact 0 / 1 / out-of-range values, a NaN and infinities in every image's corner."""
    g = torch.Generator().manual_seed(6)
    x = torch.rand(3, 3, 128, 128, generator=g) * 1.2 - 0.1
    x[:, :, 0, :6] = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5, 0.25])
    x[:, 0, 1, 0] = float('nan')
    x[:, 1, 1, 1] = float('inf')
    x[:, 2, 0, 1] = float('-inf')
    return x, x.to(DEV)


def _cpu_frames(views, **kw):
    """The CPU expression on the same crops, once on the values themselves (NaN included) and once with what its clamp makes of them."""
    raw = from_rgb01_any(list(views), **kw)
    clean = from_rgb01_any([torch.nan_to_num(v, nan=0.0, posinf=1.0, neginf=0.0) for v in views], **kw)
    assert all(_planes_equal(a, b) for a, b in zip(raw, clean))
    return raw


@pytest.mark.parametrize('sub,siting', ref.LAYOUTS)
@pytest.mark.parametrize('depth', ref.DEPTHS)
def test_f32_to_yuv_crops_of_one_padded_batch(f32_batch, depth, sub, siting):
    x, xd = f32_batch
    kw = dict(depth=depth, subsampling=sub, siting=siting)
    ext = _extents(sub)
    for sizes in (ext[:3], ext[3:]):                                               # crops of the batch, read in place, several per call
        out = from_rgb01_any(xd[:len(sizes)], sizes, **kw)
        want = _cpu_frames([x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], **kw)
        for i, (o, r) in enumerate(zip(out, want)):
            assert o.y.is_cuda and o.size == sizes[i] and _planes_equal(o, r), (i, sizes[i])
    h, w = ext[2]
    assert _planes_equal(from_rgb01_any([xd[2:3, :, :h, :w]], **kw)[0], _cpu_frames([x[2, :, :h, :w]], **kw)[0])      # a single-image call


@pytest.mark.parametrize('matrix', ref.MATRICES)
@pytest.mark.parametrize('rng', ref.RANGES)
def test_f32_to_yuv_colour_parameters_and_offset_views(f32_batch, matrix, rng):
    x, xd = f32_batch
    for depth, sub, siting in ((10, '420', 'left'), (12, '422', 'center'), (10, '444', 'center'), (8, '422', 'left')):
        kw = dict(depth=depth, subsampling=sub, siting=siting, matrix=matrix, range=rng)
        out = from_rgb01_any([xd[i, :, 1:67, 1:71] for i in range(2)], **kw)       # views off the 16-byte grid: scalar loads
        assert all(_planes_equal(o, r) for o, r in zip(out, _cpu_frames([x[i, :, 1:67, 1:71] for i in range(2)], **kw)))
        out = from_rgb01_any(xd[:2], **kw)                                         # whole planes: the 16-byte loads
        assert all(_planes_equal(o, r) for o, r in zip(out, _cpu_frames([x[0], x[1]], **kw)))


@pytest.mark.parametrize('depth,sub,siting', [(10, '420', 'left'), (10, '422', 'center'), (12, '444', 'center'), (8, '420', 'left'), (8, '444', 'center')])
def test_f32_to_yuv_strided_misaligned_output(f32_batch, depth, sub, siting):
    """The C entry itself: planes with rows 5 samples longer than their width starting 1 sample past an aligned address; only they are
    written -- the guard samples before, between the rows of and after every plane keep their value."""
    from lvae import _native
    x, xd = f32_batch
    sizes = [(62, 70), (6, 10)] if sub != '444' else [(62, 70), (5, 7)]
    want = _cpu_frames([x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], depth=depth, subsampling=sub, siting=siting)
    dt = torch.uint8 if depth == 8 else torch.int16
    bufs, views = [], []
    for h, w in sizes:
        for ph, pw in ((h, w),) + (ref.chroma_shape(h, w, sub),) * 2:
            buf = torch.full((1 + ph * (pw + 5),), 7, dtype=dt, device=DEV)
            bufs.append(buf)
            views.append(buf[1:].as_strided((ph, pw), (pw + 5, 1)))
    arr = lambda k: (ctypes.c_void_p * 2)(*[views[3 * i + k].data_ptr() for i in range(2)])
    row = lambda k: (ctypes.c_long * 2)(*[views[3 * i + k].stride(0) for i in range(2)])
    hw = (ctypes.c_int * 4)(*[v for s in sizes for v in s])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _native.lib().lvae_image_f32_to_yuv(xd.data_ptr(), 3 * 128 * 128, 128 * 128, 128, 128, 128, hw, 2, depth, _native.YUV_SUBSAMPLINGS.index(sub),
                                             _native.YUV_SITINGS.index(siting), 1, 0, arr(0), arr(1), arr(2), row(0), row(1), row(2), st)
    assert rc == 0
    torch.cuda.synchronize()
    for i in range(2):
        for k, p in enumerate(want[i].planes()):
            v, buf = views[3 * i + k], bufs[3 * i + k]
            assert torch.equal(v.cpu(), p), (i, k)
            mask = torch.ones(buf.numel(), dtype=torch.bool)
            mask[1:].as_strided(tuple(v.shape), v.stride()).fill_(False)
            assert bool((buf.cpu()[mask] == 7).all()), (i, k)


@pytest.mark.parametrize('sub', ['420', '422'])
def test_f32_to_yuv_left_siting_at_the_first_and_last_chroma_column(sub):
    """Column 0 has no left neighbour (it repeats itself); the last chroma column's right tap is the last luma column.  Widths 2 (one lane
    owns both), 6 (the last block holds two columns) and 8, each alone in its call and against the formula written out."""
    for w in (2, 6, 8):
        g = torch.Generator().manual_seed(w)
        x = torch.rand(3, 4, w, generator=g)
        fr = from_rgb01_any([x.to(DEV)], depth=10, subsampling=sub, siting='left')[0]
        want = from_rgb01_any([x], depth=10, subsampling=sub, siting='left')[0]
        assert _planes_equal(fr, want), w
        r, gg, b = x[0], x[1], x[2]                            # BT.709, limited range, spelled out in fp32
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        yn = (f(0.2126) * r + f(0.7152) * gg) + f(0.0722) * b
        cb = (b - yn) / f(1.8556)
        first = ((cb[:, 0] + cb[:, 1]) + (cb[:, 0] + cb[:, 0])) * 0.25
        last = ((cb[:, max(w - 3, 0)] + cb[:, w - 1]) + (cb[:, w - 2] + cb[:, w - 2])) * 0.25
        if sub == '420':
            first, last = (first[0::2] + first[1::2]) * 0.5, (last[0::2] + last[1::2]) * 0.5
        code = lambda t: torch.round(t * f(896.0) + f(512.0)).clamp(0, 1023).to(torch.int16)
        assert torch.equal(fr.u[:, 0].cpu(), code(first)) and torch.equal(fr.u[:, -1].cpu(), code(last)), w


# ----------------------------------------------------------------------------------------------- lvae_sse_u16, psnr_yuv
def test_sse_u16_against_numpy():
    g = np.random.default_rng(50)
    shapes = [(1, 1), (3, 17), (64, 64), (70, 130), (70, 130), (64, 64)]
    pairs, want = [], []
    for k, (h, w) in enumerate(shapes):
        a, b = g.integers(0, 65536, (h, w)).astype(np.uint16), g.integers(0, 65536, (h, w)).astype(np.uint16)
        if k == 5:
            a[:], b[:] = 0, 65535                                                  # the largest per-sample term everywhere
        want.append(int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()))
        ta, tb = torch.from_numpy(a.view(np.int16)).to(DEV), torch.from_numpy(b.view(np.int16)).to(DEV)
        if k == 4:                                                                 # strided, misaligned views of larger buffers
            big_a, big_b = torch.zeros(h + 2, w + 7, dtype=torch.int16, device=DEV), torch.zeros(h, w + 8, dtype=torch.int16, device=DEV)
            big_a[1:h + 1, 3:w + 3] = ta
            big_b[:, 8:] = tb
            ta, tb = big_a[1:h + 1, 3:w + 3], big_b[:, 8:]
            assert not ta.is_contiguous() and ta.data_ptr() % 16
        pairs.append((ta, tb))
    assert want[5] == 64 * 64 * 65535 * 65535 and want[5] > 2 ** 43
    assert sse_u16(pairs) == want                                                  # six pairs in one call
    assert sse_u16(pairs[1:2]) == want[1:2]
    assert sse_u16([(pairs[3][0], pairs[3][1].cpu())]) == want[3:4]                # a CPU plane is uploaded
    assert sse_u16(pairs) == want                                                  # `out` is zeroed by every call
    assert sse_u16([(p.cpu(), q.cpu()) for p, q in pairs]) == want


def test_psnr_yuv_device_equals_cpu():
    cases = [(10, '420', (6, 10)), (10, '444', (5, 7)), (12, '422', (62, 70)), (8, '422', (6, 10))]
    for depth, sub, (h, w) in cases:
        a = [_frame(ref.noise_planes(h, w, depth, sub, 60 + i), depth, sub) for i in range(2)]
        b = [_frame(ref.noise_planes(h, w, depth, sub, 70 + i), depth, sub) for i in range(2)]
        assert psnr_yuv([f.to(DEV) for f in a], [f.to(DEV) for f in b]) == psnr_yuv(a, b)
        assert psnr_yuv(a[0].to(DEV), a[0].to(DEV))['psnr-avg'] == float('inf')


# ----------------------------------------------------------------------------------------------- the models
def _seeded(name):
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
def _qres34m():
    return _seeded('qres34m')


@pytest.fixture(scope='module')
def qarv(qarv_seeded_sd):
    import lvae
    m = load_seeded_into(lvae.get_model('qarv_base'), qarv_seeded_sd).to(DEV).eval()
    m.compress_mode()
    return m


SIZES = [(62, 126), (64, 128), (60, 120)]                    # all pad to 64 x 128


def _natural_rgb(h, w, seed):
    return torch.from_numpy(seeded_init.synthetic_image_u8(h, w, seed)).permute(2, 0, 1).float().div(255)


def _natural_frames(depth, sub, siting):
    return from_rgb01_any([_natural_rgb(h, w, 80 + i) for i, (h, w) in enumerate(SIZES)], depth=depth, subsampling=sub, siting=siting)


@pytest.fixture(scope='module', params=[('qarv_base', '420', 'left'), ('qarv_base', '444', 'center'), ('qres34m', '420', 'left'), ('qres34m', '444', 'center')],
                ids=lambda p: '-'.join(p))
def coded(request, qarv):
    """Per model and layout, computed once: three 10-bit frames, compress_yuv's bytes and decompress_yuv's frames."""
    name, sub, siting = request.param
    m = qarv if name == 'qarv_base' else _qres34m()
    frames = _natural_frames(10, sub, siting)
    blobs = m.compress_yuv(frames, siting=siting)
    recs = m.decompress_yuv(blobs, depth=10, subsampling=sub, siting=siting)
    return dict(name=name, model=m, sub=sub, siting=siting, frames=frames, blobs=blobs, recs=recs)


def test_streams_are_the_float_path_bytes(coded):
    m, siting = coded['model'], coded['siting']
    for i, fr in enumerate(coded['frames']):
        x, sizes = to_rgb01_any([fr], div=64, siting=siting)                       # the host conversion, then the float-tensor API
        assert tuple(x.shape) == (1, 3, 64, 128) and sizes == [SIZES[i]]
        assert isinstance(coded['blobs'][i], bytes) and coded['blobs'][i] == m._pack_blob(m.compress(x.to(DEV)), sizes[0]), i
    assert m.compress_yuv(coded['frames'][1:2], siting=siting)[0] == coded['blobs'][1]      # alone as in a batch
    assert m.compress_yuv([f.to(DEV) for f in coded['frames']], siting=siting) == coded['blobs']
    if coded['name'] != 'qarv_base':
        with pytest.raises(ValueError):
            m.compress_yuv(coded['frames'], lmb=64)
    with pytest.raises(ValueError):
        m.compress_yuv(coded['frames'][:1] + _natural_frames(12, coded['sub'], siting)[1:2])            # depths differ


def test_reconstructions_are_the_converted_decompress(coded):
    m, sub, siting = coded['model'], coded['sub'], coded['siting']
    for i, blob in enumerate(coded['blobs']):
        body, size, _ = m._unpack_blob(blob)
        assert size == SIZES[i]
        x = m.decompress(body)[:, :, :size[0], :size[1]].cpu()
        want = from_rgb01_any(x, depth=10, subsampling=sub, siting=siting)[0]
        rec = coded['recs'][i]
        assert rec.y.is_cuda and rec.y.dtype == torch.int16 and _planes_equal(rec, want), i
    x = m.decompress(m._unpack_blob(coded['blobs'][0])[0])[:, :, :62, :126].cpu()     # another depth, subsampling, matrix and range on the way out
    other = m.decompress_yuv(coded['blobs'][:1], depth=12, subsampling='422', siting='left', matrix='bt2020', range='full')[0]
    assert _planes_equal(other, from_rgb01_any(x, depth=12, subsampling='422', siting='left', matrix='bt2020', range='full')[0])


def test_decompress_yuv_rejects_sizes_that_do_not_fit(qarv):
    blob = qarv.compress_yuv(from_rgb01_any([_natural_rgb(5, 7, 1)], depth=10, subsampling='444'))[0]
    assert qarv.decompress_yuv([blob], depth=10, subsampling='444')[0].size == (5, 7)
    for sub in ('420', '422'):
        with pytest.raises(ValueError, match='does not fit'):
            qarv.decompress_yuv([blob], depth=10, subsampling=sub)


def test_per_frame_lambdas(qarv):
    import struct
    frames = _natural_frames(10, '420', 'left')
    lmbs = [16, 256, 2048]
    blobs = qarv.compress_yuv(frames, lmb=lmbs, siting='left')
    for i, lmb in enumerate(lmbs):
        assert blobs[i] == qarv.compress_yuv([frames[i]], lmb=lmb, siting='left')[0], i
        assert struct.unpack('f', blobs[i][4:8])[0] == lmb


def test_8_bit_420_centre_streams_are_compress_yuv420s(qarv):
    from lvae.utils.yuv import Yuv420Frame
    old = from_rgb01([_natural_rgb(h, w, 80 + i) for i, (h, w) in enumerate(SIZES)])
    new = [YuvFrame(f.y, f.u, f.v) for f in old]
    for m in (qarv, _qres34m()):
        blobs = m.compress_yuv(new)
        assert blobs == m.compress_yuv420(old)
        for a, b in zip(m.decompress_yuv(blobs), m.decompress_yuv420(blobs)):
            assert isinstance(b, Yuv420Frame) and all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))


# ----------------------------------------------------------------------------------------------- yuv_evaluate
def test_yuv_evaluate_is_the_per_frame_loop(qarv, tmp_path):
    from lvae.evaluation import yuv_evaluate
    frames = from_rgb01_any([_natural_rgb(62, 66, 90 + i) for i in range(3)], depth=10, siting='left')
    path = tmp_path / 'clip10.yuv'
    write_yuv(frames, path)
    rows = []
    for fr in read_yuv(path, 66, 62, depth=10):
        blob = qarv.compress_yuv([fr], lmb=256, matrix='bt2020', siting='left')[0]
        rec = qarv.decompress_yuv([blob], depth=10, siting='left', matrix='bt2020')[0]
        rows.append(dict(psnr_yuv(fr, rec.cpu()), bpp=8 * len(blob) / (62 * 66)))
    want = {}
    for k in rows[0]:
        acc = 0.0
        for r in rows:
            acc += r[k]
        want[k] = acc / 3
    got = yuv_evaluate(qarv, path, 66, 62, batch=2, lmb=256, matrix='bt2020', depth=10, siting='left')
    assert got == want and set(got) == {'bpp', 'mse-y', 'mse-u', 'mse-v', 'psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv', 'psnr-avg'}


def test_yuv_evaluate_defaults_are_unchanged(qarv, tmp_path):
    from lvae.evaluation import yuv_evaluate
    frames = from_rgb01([_natural_rgb(62, 66, 90 + i) for i in range(3)])
    path = tmp_path / 'clip8.yuv'
    write_yuv420(frames, path)
    rows = []
    for fr in read_yuv420(path, 66, 62):
        blob = qarv.compress_yuv420([fr], lmb=256)[0]
        rec = qarv.decompress_yuv420([blob])[0]
        rows.append(dict(psnr_yuv420(fr, rec.cpu()), bpp=8 * len(blob) / (62 * 66)))
    want = {}
    for k in rows[0]:
        acc = 0.0
        for r in rows:
            acc += r[k]
        want[k] = acc / 3
    got = yuv_evaluate(qarv, path, 66, 62, batch=2, lmb=256)
    assert got == want and 'psnr-avg' not in got
    assert yuv_evaluate(qarv, path, 66, 62, batch=2, lmb=256, depth=8, subsampling='420', siting='center') == want


# ----------------------------------------------------------------------------------------------- the script
def test_codec_script_yuv_round_trip_at_10_bits(tmp_path):
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, out = tmp_path / 'in.yuv', tmp_path / 'bits', tmp_path / 'out.yuv'
    common = ['-m', 'qarv_base', '--synthetic', '3', '--batch', '2', '--depth', '10', '--siting', 'left']
    for cmd in (['encode-yuv', str(src), str(bits), '--size', '66', '62', '--lmb', '256'], ['decode-yuv', str(bits), str(out)]):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(bits.glob('*.bits'))
    assert [f.name for f in files] == ['frame00000.bits', 'frame00001.bits', 'frame00002.bits']
    assert src.stat().st_size == out.stat().st_size == 3 * (62 * 66 * 3 // 2) * 2
    m = _seeded('qarv_base')
    frames = read_yuv(src, 66, 62, depth=10)
    assert len(frames) == 3 and [f.read_bytes() for f in files] == m.compress_yuv(frames, lmb=256, siting='left')
    recs = m.decompress_yuv([f.read_bytes() for f in files], depth=10, siting='left')
    for a, b in zip(read_yuv(out, 66, 62, depth=10), recs):
        assert _planes_equal(a, b)
