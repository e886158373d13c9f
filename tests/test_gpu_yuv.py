"""-m gpu: 8-bit YUV 4:2:0 frames end to end.  The three kernels of csrc/yuv_io.hip against the CPU expressions that define them
(lvae/utils/yuv.py; torch.equal / ==: every bit), then the model-level API against the float path spelled out here, yuv_evaluate against
its per-frame loop, and scripts/lvae-codec.py encode-yuv / decode-yuv against decompress_yuv420."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
import yuv_ref
from conftest import load_seeded_into
from lvae.metrics import psnr_yuv420, sse_u8
from lvae.utils.yuv import Yuv420Batch, Yuv420Frame, from_rgb01, read_yuv420, to_rgb01, write_yuv420

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
EXTENTS = [((2, 2), 64, (64, 64)), ((6, 10), 64, (64, 64)), ((64, 64), 64, (64, 64)), ((66, 130), 64, (128, 192)), ((10, 6), 1, (10, 6))]


def _frame(planes, fmt='i420', device='cpu'):
    y, u, v = (torch.from_numpy(p) for p in planes)
    return Yuv420Frame('i420', y, u, v).as_format(fmt).to(device)


def _planes_equal(a, b):
    return a.fmt == b.fmt and all(torch.equal(p.cpu(), q.cpu()) for p, q in zip(a.planes(), b.planes()))


# ----------------------------------------------------------------------------------------------- lvae_image_yuv420_to_f32
@pytest.mark.parametrize('extent,div,canvas', EXTENTS)
def test_yuv420_to_f32_extent_to_canvas(extent, div, canvas):
    planes = yuv_ref.noise_planes(*extent, 11)
    ref, _ = to_rgb01([_frame(planes)], div=div)                                  # the CPU expression, replicate-padded
    assert tuple(ref.shape) == (1, 3) + canvas
    outs = {}
    for fmt in ('i420', 'nv12'):
        x, sizes = to_rgb01([_frame(planes, fmt)], div=div, device=DEV)
        assert sizes == [extent] and x.is_cuda and x.dtype == torch.float32
        assert torch.equal(x.cpu(), ref), fmt
        outs[fmt] = x
    assert torch.equal(outs['i420'], outs['nv12'])
    x, _ = to_rgb01([_frame(planes)], div=div, device=DEV, chroma='nearest')
    assert torch.equal(x.cpu(), to_rgb01([_frame(planes)], div=div, chroma='nearest')[0])


@pytest.mark.parametrize('matrix,rng,chroma', yuv_ref.COMBOS)
def test_yuv420_to_f32_colour_parameters(matrix, rng, chroma):
    planes = yuv_ref.noise_planes(6, 10, 12)
    kw = dict(matrix=matrix, range=rng, chroma=chroma)
    ref, _ = to_rgb01([_frame(planes)], div=64, **kw)
    for fmt in ('i420', 'nv12'):
        assert torch.equal(to_rgb01([_frame(planes, fmt)], div=64, device=DEV, **kw)[0].cpu(), ref), fmt


def test_yuv420_to_f32_batch_of_three_extents():
    sizes = [(6, 10), (62, 66), (64, 128)]
    frames = [_frame(yuv_ref.noise_planes(h, w, 20 + i)) for i, (h, w) in enumerate(sizes)]
    ref, _ = to_rgb01(frames, div=64)
    x, got = to_rgb01([f.to(DEV) for f in frames], div=64)
    assert got == sizes and tuple(x.shape) == (3, 3, 64, 128) and x.is_cuda
    assert torch.equal(x.cpu(), ref)


@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_yuv420_to_f32_strided_misaligned_planes(fmt):
    """Planes that are views of a larger buffer: rows 5 bytes longer than the plane, bases 1 byte past an aligned address; read in place."""
    h, w = 6, 12
    planes = yuv_ref.noise_planes(h, w, 31)

    def view(p):
        p = torch.from_numpy(p)
        row = p.shape[1] * (p.shape[2] if p.dim() == 3 else 1) + 5
        buf = torch.zeros(1 + p.shape[0] * row, dtype=torch.uint8, device=DEV)
        v = buf[1:].as_strided(tuple(p.shape), (row,) + ((2, 1) if p.dim() == 3 else (1,)))
        v.copy_(p)
        assert v.data_ptr() % 4 == 1
        return v
    if fmt == 'i420':
        fr = Yuv420Frame('i420', view(planes[0]), view(planes[1]), view(planes[2]))
    else:
        fr = Yuv420Frame('nv12', view(planes[0]), uv=view(yuv_ref.nv12_uv(planes[1], planes[2])))
    b = Yuv420Batch([fr], 64, DEV)
    out = torch.empty(b.shape, dtype=torch.float32, device=DEV)
    b.fill(out)
    assert b.frames[0].y.data_ptr() == fr.y.data_ptr()
    assert torch.equal(out.cpu(), to_rgb01([_frame(planes)], div=64)[0])


@pytest.mark.parametrize('gap', [40, 41])
def test_yuv420_to_f32_writes_only_its_planes(gap):
    """A destination whose image stride exceeds 3 * H * W (gap 41: also off the 16-byte grid, the scalar-store path)."""
    frames = [_frame(yuv_ref.noise_planes(h, w, 40 + i)) for i, (h, w) in enumerate([(6, 4), (8, 8)])]
    H = W = 8
    big = torch.full((2, 3 * H * W + gap), -7.0, dtype=torch.float32, device=DEV)
    Yuv420Batch(frames, 8, DEV).fill(big[:, :3 * H * W].view(2, 3, H, W))
    got = big.cpu()
    assert torch.equal(got[:, :3 * H * W].reshape(2, 3, H, W), to_rgb01(frames, div=8)[0])
    assert bool((got[:, 3 * H * W:] == -7.0).all())


def test_yuv420_to_f32_all_values():
    planes = yuv_ref.all_values_planes()
    for kw in (dict(chroma='nearest'), dict(chroma='bilinear'), dict(chroma='nearest', matrix='bt601', range='full')):
        assert torch.equal(to_rgb01([_frame(planes)], device=DEV, **kw)[0].cpu(), to_rgb01([_frame(planes)], **kw)[0]), kw


# ----------------------------------------------------------------------------------------------- lvae_image_f32_to_yuv420
@pytest.fixture(scope='module')
def f32_batch():
    """(5, 3, 128, 192) fp32 in [-0.1, 1.1] with exact 0 / 1 / out-of-range values, a NaN and infinities in every image's corner."""
    x = yuv_ref.rgb_batch()
    return x, x.to(DEV)


def _cpu_frames(x, sizes, fmt, **kw):
    z = torch.nan_to_num(x, nan=0.0, posinf=1.0, neginf=0.0)       # what the clamp of the definition makes of them, spelled out
    return from_rgb01([z[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], fmt=fmt, **kw)


@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_f32_to_yuv420_crops_of_one_padded_batch(f32_batch, fmt):
    x, xd = f32_batch
    sizes = [e for e, _, _ in EXTENTS]
    out = from_rgb01(xd, sizes, fmt=fmt)                                           # crops of the batch, read in place
    ref = _cpu_frames(x, sizes, fmt)
    raw = from_rgb01([x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], fmt=fmt)   # the CPU expression on the NaN itself
    for i, (o, r, q) in enumerate(zip(out, ref, raw)):
        assert o.y.is_cuda and o.size == sizes[i] and _planes_equal(o, r) and _planes_equal(o, q), (i, sizes[i])
    for i, (h, w) in enumerate(sizes):                                             # single-image calls: the same bytes
        assert _planes_equal(from_rgb01([xd[i:i + 1, :, :h, :w]], fmt=fmt)[0], ref[i]), i


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
@pytest.mark.parametrize('rng', ['limited', 'full'])
def test_f32_to_yuv420_colour_parameters_and_offset_views(f32_batch, matrix, rng):
    x, xd = f32_batch
    kw = dict(matrix=matrix, range=rng)
    out = from_rgb01([xd[i, :, 1:67, 1:131] for i in range(2)], fmt='nv12', **kw)  # views off the 16-byte grid: scalar loads
    ref = from_rgb01([torch.nan_to_num(x[i, :, 1:67, 1:131], nan=0.0, posinf=1.0, neginf=0.0) for i in range(2)], fmt='nv12', **kw)
    assert all(_planes_equal(o, r) for o, r in zip(out, ref))
    out = from_rgb01(xd[:2], fmt='i420', **kw)                                     # whole planes: the 16-byte loads
    assert all(_planes_equal(o, r) for o, r in zip(out, _cpu_frames(x, [(128, 192)] * 2, 'i420', **kw)))


def test_f32_to_yuv420_strided_misaligned_output(f32_batch):
    """The C entry itself: planes with rows 5 bytes longer than their width starting 1 byte past an aligned address; only they are written."""
    from lvae import _native
    x, xd = f32_batch
    sizes = [(66, 130), (6, 10)]
    ref = _cpu_frames(x, sizes, 'i420')
    bufs, views = [], []
    for h, w in sizes:
        for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
            buf = torch.full((1 + ph * (pw + 5),), 7, dtype=torch.uint8, device=DEV)
            bufs.append(buf)
            views.append(buf[1:].as_strided((ph, pw), (pw + 5, 1)))
    arr = lambda k: (ctypes.c_void_p * 2)(*[views[3 * i + k].data_ptr() for i in range(2)])
    row = lambda k: (ctypes.c_long * 2)(*[views[3 * i + k].stride(0) for i in range(2)])
    hw = (ctypes.c_int * 4)(*[v for s in sizes for v in s])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _native.lib().lvae_image_f32_to_yuv420(xd.data_ptr(), 3 * 128 * 192, 128 * 192, 192, 128, 192, hw, 2, 0, 1, 0, arr(0), arr(1), arr(2),
                                                row(0), row(1), row(2), st)
    assert rc == 0
    torch.cuda.synchronize()
    for i in range(2):
        for k, p in enumerate(ref[i].planes()):
            v, buf = views[3 * i + k], bufs[3 * i + k]
            assert torch.equal(v.cpu(), p), (i, k)
            mask = torch.ones(buf.numel(), dtype=torch.bool)
            mask[1:].as_strided(tuple(v.shape), v.stride()).fill_(False)
            assert bool((buf.cpu()[mask] == 7).all()), (i, k)


def test_f32_to_yuv420_nv12_every_store_path(f32_batch):
    """The C entry with fmt NV12: planes that start 0, 1, 2 and 3 bytes past a 4-byte-aligned address, Y rows of w + 5 and UV rows of
    w + 4 bytes.  Widths 2 and 6 end in a block with two valid columns; a UV block leaves as one dword, as two half-dwords or byte by
    byte, as its address allows.  Every path writes the definition's bytes, and only the planes are written."""
    from lvae import _native
    x, xd = f32_batch
    sizes = [(2, 2), (2, 6), (4, 8), (6, 10), (66, 130)]
    n = len(sizes)
    ref = _cpu_frames(x, sizes, 'nv12')
    hw = (ctypes.c_int * (2 * n))(*[v for s in sizes for v in s])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in range(4):
        bufs, views = [], []
        for h, w in sizes:
            for ph, row in ((h, w + 5), (h // 2, w + 4)):
                buf = torch.full((4 + ph * row,), 7, dtype=torch.uint8, device=DEV)
                bufs.append(buf)
                views.append(buf[off:].as_strided((ph, w), (row, 1)))
                assert views[-1].data_ptr() % 4 == off
        arr = lambda k: (ctypes.c_void_p * n)(*[views[2 * i + k].data_ptr() for i in range(n)])
        row = lambda k: (ctypes.c_long * n)(*[views[2 * i + k].stride(0) for i in range(n)])
        rc = _native.lib().lvae_image_f32_to_yuv420(xd.data_ptr(), 3 * 128 * 192, 128 * 192, 192, 128, 192, hw, n, 1, 1, 0, arr(0), arr(1), None,
                                                    row(0), row(1), None, st)
        assert rc == 0
        torch.cuda.synchronize()
        for i in range(n):
            for k, p in enumerate((ref[i].y, ref[i].uv.flatten(1))):
                v, buf = views[2 * i + k], bufs[2 * i + k]
                assert torch.equal(v.cpu(), p), (off, i, k)
                mask = torch.ones(buf.numel(), dtype=torch.bool)
                mask[off:].as_strided(tuple(v.shape), v.stride()).fill_(False)
                assert bool((buf.cpu()[mask] == 7).all()), (off, i, k)


@pytest.mark.parametrize('chroma', ['nearest', 'bilinear'])
@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_yuv420_to_f32_edges_and_alignments(fmt, chroma):
    """Frames narrower and lower than their 16 x 16 canvas -- widths 2 and 6 end in the right-edge path, 8 and 12 in whole quads, and the
    rows below the extent repeat its last row -- read in place from planes 0, 1, 2 and 3 bytes past a 4-byte-aligned address."""
    sizes = [(h, w) for h in (2, 6) for w in (2, 6, 8, 12)]
    planes = [yuv_ref.noise_planes(h, w, 100 + i) for i, (h, w) in enumerate(sizes)]
    ref, _ = to_rgb01([_frame(p) for p in planes], div=16, chroma=chroma)
    assert tuple(ref.shape) == (8, 3, 16, 16)
    for off in range(4):
        def view(p):
            p = torch.from_numpy(p)
            row = p[0].numel() + 5
            buf = torch.zeros(4 + p.shape[0] * row, dtype=torch.uint8, device=DEV)
            v = buf[off:].as_strided(tuple(p.shape), (row,) + ((2, 1) if p.dim() == 3 else (1,)))
            v.copy_(p)
            assert v.data_ptr() % 4 == off
            return v
        if fmt == 'i420':
            frames = [Yuv420Frame('i420', view(y), view(u), view(v)) for y, u, v in planes]
        else:
            frames = [Yuv420Frame('nv12', view(y), uv=view(yuv_ref.nv12_uv(u, v))) for y, u, v in planes]
        b = Yuv420Batch(frames, 16, DEV, chroma=chroma)
        out = torch.empty(b.shape, dtype=torch.float32, device=DEV)
        b.fill(out)
        assert torch.equal(out.cpu(), ref), off


@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_yuv420_seventeen_frames_cross_the_launch_chunk(fmt):
    """B = 17 is one frame more than a launch takes: in and out, frames of 4 x 4, 6 x 8 and 8 x 12 mixed."""
    sizes = [(4 + 2 * (i % 3), 4 + 4 * (i % 3)) for i in range(17)]
    planes = [yuv_ref.noise_planes(h, w, 200 + i) for i, (h, w) in enumerate(sizes)]
    ref, _ = to_rgb01([_frame(p) for p in planes])
    x, got = to_rgb01([_frame(p, fmt) for p in planes], device=DEV)
    assert got == sizes and tuple(x.shape) == (17, 3, 8, 12) and torch.equal(x.cpu(), ref)
    out, want = from_rgb01(x, sizes, fmt=fmt), from_rgb01(ref, sizes, fmt=fmt)
    assert len(out) == 17 and all(o.y.is_cuda and _planes_equal(o, w) for o, w in zip(out, want))


# ----------------------------------------------------------------------------------------------- lvae_sse_u8
def test_sse_u8_against_numpy():
    g = np.random.default_rng(50)
    shapes = [(1, 1), (3, 5), (64, 64), (33, 130), (33, 130), (64, 64)]
    pairs, want = [], []
    for k, (h, w) in enumerate(shapes):
        a, b = g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h, w), dtype=np.uint8)
        if k == 5:
            a[:], b[:] = 0, 255                                                    # the largest per-sample term everywhere
        want.append(int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()))
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        if k == 4:                                                                 # strided, misaligned views of larger buffers
            big_a, big_b = torch.zeros(h + 2, w + 7, dtype=torch.uint8, device=DEV), torch.zeros(h, w + 16, dtype=torch.uint8, device=DEV)
            big_a[1:h + 1, 3:w + 3] = ta
            big_b[:, 16:] = tb
            ta, tb = big_a[1:h + 1, 3:w + 3], big_b[:, 16:]
            assert not ta.is_contiguous() and ta.data_ptr() % 16
        pairs.append((ta, tb))
    assert want[5] == 64 * 64 * 255 * 255
    assert sse_u8(pairs) == want                                                   # six pairs in one call
    assert sse_u8(pairs[1:2]) == want[1:2]
    assert sse_u8([(pairs[3][0], pairs[3][1].cpu())]) == want[3:4]                 # a CPU plane is uploaded
    assert sse_u8(pairs) == want                                                   # `out` is zeroed by every call


def test_psnr_yuv420_device_equals_cpu():
    a = [_frame(yuv_ref.noise_planes(h, w, 60 + i), fmt) for i, ((h, w), fmt) in enumerate([((6, 10), 'i420'), ((62, 66), 'nv12')])]
    b = [_frame(yuv_ref.noise_planes(h, w, 70 + i), fmt) for i, ((h, w), fmt) in enumerate([((6, 10), 'nv12'), ((62, 66), 'nv12')])]
    assert psnr_yuv420([f.to(DEV) for f in a], [f.to(DEV) for f in b]) == psnr_yuv420(a, b)
    assert psnr_yuv420(a[0].to(DEV), a[0].to(DEV))['psnr-yuv'] == float('inf')


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _qres34m():
    import lvae
    m = lvae.get_model('qres34m', pretrained=False)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m.compress_mode()
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def qarv(qarv_seeded_sd):
    import lvae
    m = load_seeded_into(lvae.get_model('qarv_base'), qarv_seeded_sd).to(DEV).eval()
    m.compress_mode()
    return m


@pytest.fixture(scope='module', params=['qarv_base', 'qres34m'])
def coded(request, qarv):
    """Per model, computed once: three 62 x 66 frames (canvas 64 x 128), compress_yuv420's bytes and decompress_yuv420's frames."""
    m = qarv if request.param == 'qarv_base' else _qres34m()
    frames = [_natural_frame(62, 66, 80 + i) for i in range(3)]
    blobs = m.compress_yuv420(frames)
    return dict(name=request.param, model=m, frames=frames, blobs=blobs, recs=m.decompress_yuv420(blobs))


def _natural_frame(h, w, seed, fmt='i420'):
    rgb = torch.from_numpy(seeded_init.synthetic_image_u8(h, w, seed)).permute(2, 0, 1).float().div(255)
    return from_rgb01([rgb], fmt=fmt)[0]


def test_streams_are_the_float_path_bytes(coded):
    m = coded['model']
    for i, fr in enumerate(coded['frames']):
        x, sizes = to_rgb01([fr], div=64)                                          # the host conversion, then the float-tensor API
        assert tuple(x.shape) == (1, 3, 64, 128)
        assert isinstance(coded['blobs'][i], bytes) and coded['blobs'][i] == m._pack_blob(m.compress(x.to(DEV)), sizes[0]), i
    assert m.compress_yuv420(coded['frames'][1:2])[0] == coded['blobs'][1]         # alone as in a batch
    assert m.compress_yuv420([f.as_format('nv12').to(DEV) for f in coded['frames']]) == coded['blobs']
    if coded['name'] != 'qarv_base':
        with pytest.raises(ValueError):
            m.compress_yuv420(coded['frames'], lmb=64)


def test_reconstructions_are_the_converted_decompress(coded):
    m = coded['model']
    nv = m.decompress_yuv420(coded['blobs'], fmt='nv12')
    for i, blob in enumerate(coded['blobs']):
        body, size, _ = m._unpack_blob(blob)
        assert size == (62, 66)
        x = m.decompress(body)[:, :, :62, :66].cpu()
        ref = from_rgb01(x)[0]
        rec = coded['recs'][i]
        assert rec.y.is_cuda and rec.fmt == 'i420' and _planes_equal(rec, ref), i
        assert _planes_equal(nv[i], ref.as_format('nv12')), i
    full = m.decompress_yuv420(coded['blobs'][:1], matrix='bt601', range='full')[0]
    assert _planes_equal(full, from_rgb01(m.decompress(m._unpack_blob(coded['blobs'][0])[0])[:, :, :62, :66].cpu(), matrix='bt601', range='full')[0])


def test_per_frame_lambdas(qarv):
    import struct
    frames = [_natural_frame(62, 66, 80 + i) for i in range(3)]
    lmbs = [16, 256, 2048]
    blobs = qarv.compress_yuv420(frames, lmb=lmbs)
    for i, lmb in enumerate(lmbs):
        assert blobs[i] == qarv.compress_yuv420([frames[i]], lmb=lmb)[0], i
        assert struct.unpack('f', blobs[i][4:8])[0] == lmb


def test_the_general_entry_points_take_yuv420_frames(qarv):
    """compress_yuv / decompress_yuv on Yuv420Frames are compress_yuv420 / decompress_yuv420: two 66 x 70 frames on one 128 x 128 canvas."""
    for fmt in ('i420', 'nv12'):
        frames = [_natural_frame(66, 70, 70 + i, fmt) for i in range(2)]
        blobs = qarv.compress_yuv(frames)
        assert all(isinstance(b, bytes) for b in blobs) and blobs == qarv.compress_yuv420(frames)
        got, want = qarv.decompress_yuv(blobs, layout=fmt), qarv.decompress_yuv420(blobs, fmt=fmt)
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert type(g) is Yuv420Frame and g.fmt == fmt and g.size == (66, 70) and g.y.is_cuda
            assert len(g.planes()) == len(w.planes()) and all(torch.equal(p, q) for p, q in zip(g.planes(), w.planes()))
        with pytest.raises(ValueError, match='siting'):
            qarv.compress_yuv(frames, siting='left')


# ----------------------------------------------------------------------------------------------- yuv_evaluate
@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_yuv_evaluate_is_the_per_frame_loop(qarv, tmp_path, fmt):
    from lvae.evaluation import yuv_evaluate
    frames = [_natural_frame(62, 66, 90 + i, fmt) for i in range(4)]
    path = tmp_path / 'clip.yuv'
    write_yuv420(frames, path)
    rows = []
    for fr in read_yuv420(path, 66, 62, fmt):
        blob = qarv.compress_yuv420([fr], lmb=256, matrix='bt601')[0]
        rec = qarv.decompress_yuv420([blob], fmt=fmt, matrix='bt601')[0]
        rows.append(dict(psnr_yuv420(fr, rec.cpu()), bpp=8 * len(blob) / (62 * 66)))
    want = {}
    for k in rows[0]:
        acc = 0.0
        for r in rows:
            acc += r[k]
        want[k] = acc / 4
    got = yuv_evaluate(qarv, path, 66, 62, fmt=fmt, batch=3, lmb=256, matrix='bt601')
    assert got == want and set(got) == {'bpp', 'mse-y', 'mse-u', 'mse-v', 'psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv'}
    assert yuv_evaluate(qarv, path, 66, 62, fmt=fmt, max_frames=2, batch=8, lmb=256, matrix='bt601')['bpp'] == (rows[0]['bpp'] + rows[1]['bpp']) / 2


# ----------------------------------------------------------------------------------------------- the script
def test_codec_script_yuv_round_trip(tmp_path):
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, out = tmp_path / 'in.yuv', tmp_path / 'bits', tmp_path / 'out.yuv'
    common = ['-m', 'qarv_base', '--synthetic', '3', '--batch', '2', '--format', 'nv12']
    for cmd in (['encode-yuv', str(src), str(bits), '--size', '66', '62', '--lmb', '256'], ['decode-yuv', str(bits), str(out)]):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(bits.glob('*.bits'))
    assert [f.name for f in files] == ['frame00000.bits', 'frame00001.bits', 'frame00002.bits']
    import lvae
    m = lvae.get_model('qarv_base', pretrained=False)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m.compress_mode()
    m = m.to(DEV).eval()
    frames = read_yuv420(src, 66, 62, 'nv12')
    assert len(frames) == 3 and [f.read_bytes() for f in files] == m.compress_yuv420(frames, lmb=256)
    recs = m.decompress_yuv420([f.read_bytes() for f in files], fmt='nv12')
    for a, b in zip(read_yuv420(out, 66, 62, 'nv12'), recs):
        assert _planes_equal(a, b)
