"""-m gpu: semi-planar 10 / 12-bit frames (P010 / P012 / P210 / P212) and self-describing YUV sequences, end to end.  The contract of
lvae_image_yuvsp_to_f32 / lvae_image_f32_to_yuvsp is bit equality with the planar entries on the deinterleaved, shifted planes, so every
comparison here is torch.equal / ==: the two kernels against the planar kernels and the CPU expressions, compress_yuv / decompress_yuv on
YuvSpFrames against the planar frames' bytes and frames, the LVYS container against single calls, and scripts/lvae-codec.py with --container."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
from lvae import _native
from lvae.metrics import psnr_yuv
from lvae.utils import yuvseq
from lvae.utils.yuv import (YuvBatch, YuvFrame, YuvSpBatch, YuvSpFrame, Yuv420Frame, from_rgb01, from_rgb01_any, read_yuv_sp, to_rgb01_any,
                            write_yuv_sp)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
CASES = [(10, '420'), (12, '420'), (10, '422'), (12, '422')]
SMALL = [(18, 22), (2, 2)]                                   # chroma width 11 (odd), a 22-column row tail, the smallest frame; canvas 64 x 64


def _sp_frame(h, w, depth, sub, seed):
    """Random 16-bit words: every code occurs, and the low 16 - depth bits are garbage."""
    g = np.random.default_rng(seed)
    return YuvSpFrame(g.integers(0, 65536, (h, w)).astype(np.uint16), g.integers(0, 65536, (h >> (sub == '420'), w)).astype(np.uint16), depth, sub)


def _strided(p, off, pad=5, fill=0):
    """A device copy of plane p as a view of a larger buffer: rows `pad` samples longer than the plane, starting `off` samples into the
    allocation (off 1: 2-byte but not 4-byte aligned).  -> (view, buffer)"""
    row = p.shape[1] + pad
    buf = torch.full((off + p.shape[0] * row,), fill, dtype=torch.int16, device=DEV)
    v = buf[off:].as_strided(tuple(p.shape), (row, 1))
    v.copy_(p)
    assert v.data_ptr() % 4 == 2 * (off % 2)
    return v, buf


def _sp_equal(a, b):
    return (type(a), a.depth, a.subsampling, a.size) == (type(b), b.depth, b.subsampling, b.size) and \
        all(torch.equal(p.cpu(), q.cpu()) for p, q in zip(a.planes(), b.planes()))


def _fill(batch):
    out = torch.empty(batch.shape, dtype=torch.float32, device=DEV)
    batch.fill(out)
    return out


# ----------------------------------------------------------------------------------------------- lvae_image_yuvsp_to_f32
@pytest.mark.parametrize('chroma', ['nearest', 'bilinear'])
@pytest.mark.parametrize('siting', ['center', 'left'])
@pytest.mark.parametrize('depth,sub', CASES)
def test_yuvsp_to_f32_is_the_planar_kernel_and_the_expression(depth, sub, siting, chroma):
    frames = [_sp_frame(h, w, depth, sub, 100 + i) for i, (h, w) in enumerate(SMALL)]
    planar = [f.to_planar() for f in frames]
    kw = dict(siting=siting, chroma=chroma)
    want, sizes = to_rgb01_any(planar, div=64, **kw)         # yuv_to_rgb_expr2 on the CPU, replicate-padded to the canvas
    assert tuple(want.shape) == (2, 3, 64, 64) and sizes == SMALL
    ref = _fill(YuvBatch(planar, 64, DEV, **kw))             # lvae_image_yuv_to_f32 on the deinterleaved, shifted planes
    assert torch.equal(ref.cpu(), want)
    got, got_sizes = to_rgb01_any([f.to(DEV) for f in frames], div=64, **kw)
    assert got_sizes == SMALL and got.is_cuda and torch.equal(got, ref) and torch.equal(got.cpu(), want)
    # a row stride larger than the row; Y and UV, each alone and both, starting one sample into their allocation
    for oy, ouv in ((0, 0), (1, 0), (0, 1), (1, 1)):
        views = [YuvSpFrame(_strided(f.y, oy)[0], _strided(f.uv, ouv)[0], depth, sub) for f in frames]
        b = YuvSpBatch(views, 64, DEV, **kw)
        assert b.frames[0].y.data_ptr() == views[0].y.data_ptr() and b.frames[1].uv.data_ptr() == views[1].uv.data_ptr()      # read in place
        assert torch.equal(_fill(b), ref), (oy, ouv)
    # the low 16 - depth bits: all clear, all set
    low = (1 << (16 - depth)) - 1
    for op in (lambda p: p & ~low, lambda p: p | low):
        masked = [YuvSpFrame(op(f.y.to(DEV)), op(f.uv.to(DEV)), depth, sub) for f in frames]
        assert torch.equal(_fill(YuvSpBatch(masked, 64, DEV, **kw)), ref)


@pytest.mark.parametrize('B', [3, 17])
def test_yuvsp_to_f32_batches_across_the_launch_boundary(B):
    """Mixed sizes on one canvas; 17 frames are two launches (16 per launch)."""
    sizes = [[(18, 22), (2, 2), (64, 64), (6, 10)][i % 4] for i in range(B)]
    for depth, sub, siting in ((10, '420', 'left'), (12, '422', 'center')):
        frames = [_sp_frame(h, w, depth, sub, 200 + i) for i, (h, w) in enumerate(sizes)]
        want, _ = to_rgb01_any([f.to_planar() for f in frames], div=64, siting=siting)
        got, got_sizes = to_rgb01_any([f.to(DEV) for f in frames], div=64, siting=siting)
        assert got_sizes == sizes and tuple(got.shape) == (B, 3, 64, 64) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize('matrix,rng', [('bt601', 'full'), ('bt2020', 'limited')])
def test_yuvsp_to_f32_matrix_and_range(matrix, rng):
    frames = [_sp_frame(18, 22, 10, '420', 300), _sp_frame(18, 22, 10, '420', 301)]
    kw = dict(div=64, matrix=matrix, range=rng, siting='left')
    assert torch.equal(to_rgb01_any([f.to(DEV) for f in frames], **kw)[0].cpu(), to_rgb01_any([f.to_planar() for f in frames], **kw)[0])


# ----------------------------------------------------------------------------------------------- lvae_image_f32_to_yuvsp
@pytest.fixture(scope='module')
def f32_batch():
    """(17, 3, 72, 80) fp32 in [-0.1, 1.1] -- a padded batch whose crops the tests read in place -- with exact 0 / 1, out-of-range values, a
    NaN and infinities in every image's corner."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(17, 3, 72, 80, generator=g) * 1.2 - 0.1
    x[:, :, 0, :6] = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5, 0.25])
    x[:, 0, 1, 0] = float('nan')
    x[:, 1, 1, 1] = float('inf')
    x[:, 2, 0, 1] = float('-inf')
    return x, x.to(DEV)


def _low_bits_zero(fr):
    low = (1 << (16 - fr.depth)) - 1
    return all(int((p.to(torch.int32) & low).abs().max()) == 0 for p in fr.planes())


@pytest.mark.parametrize('siting', ['center', 'left'])
@pytest.mark.parametrize('depth,sub', CASES)
def test_f32_to_yuvsp_is_the_planar_kernel_interleaved_and_shifted(f32_batch, depth, sub, siting):
    x, xd = f32_batch
    kw = dict(depth=depth, subsampling=sub, siting=siting)
    sizes = SMALL + [(64, 64), (6, 10)]
    planar = from_rgb01_any(xd[:4], sizes, **kw)             # lvae_image_f32_to_yuv on crops of the padded batch
    cpu = from_rgb01_any([x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], **kw)          # rgb_to_yuv_expr2
    got = from_rgb01_any(xd[:4], sizes, layout='semiplanar', **kw)
    for i, (g, p, c) in enumerate(zip(got, planar, cpu)):
        assert isinstance(g, YuvSpFrame) and g.y.is_cuda and g.size == sizes[i]
        assert _sp_equal(g, p.to_semiplanar()) and _sp_equal(g, c.to_semiplanar()) and _low_bits_zero(g), i
    one = from_rgb01_any([xd[3:4, :, 1:19, 1:23]], layout='semiplanar', **kw)[0]      # a single image, its view off the 16-byte grid
    assert _sp_equal(one, from_rgb01_any([x[3, :, 1:19, 1:23]], **kw)[0].to_semiplanar())


def test_f32_to_yuvsp_across_the_launch_boundary(f32_batch):
    x, xd = f32_batch
    sizes = [[(18, 22), (2, 2), (64, 64), (6, 10)][i % 4] for i in range(17)]
    kw = dict(depth=10, subsampling='420', siting='left', matrix='bt2020', range='full')
    got = from_rgb01_any(xd, sizes, layout='semiplanar', **kw)
    want = from_rgb01_any([x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)], **kw)
    assert len(got) == 17 and all(_sp_equal(g, w.to_semiplanar()) for g, w in zip(got, want))


@pytest.mark.parametrize('depth,sub,siting', [(10, '420', 'left'), (12, '420', 'center'), (10, '422', 'center'), (12, '422', 'left')])
def test_f32_to_yuvsp_strided_misaligned_output_writes_only_its_planes(f32_batch, depth, sub, siting):
    """The C entry itself: planes whose rows are 5 samples longer than the row, Y and UV each alone and both starting one sample into their
    allocation; the guard samples in front of, between the rows of and behind every plane keep their value."""
    x, xd = f32_batch
    want = [f.to_semiplanar() for f in from_rgb01_any([x[i, :, :h, :w] for i, (h, w) in enumerate(SMALL)], depth=depth, subsampling=sub, siting=siting)]
    hw = (ctypes.c_int * 4)(*[v for s in SMALL for v in s])
    for oy, ouv in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ys = [_strided(torch.full(tuple(f.y.shape), 7, dtype=torch.int16), oy, fill=7) for f in want]
        uvs = [_strided(torch.full(tuple(f.uv.shape), 7, dtype=torch.int16), ouv, fill=7) for f in want]
        arr = lambda ps: (ctypes.c_void_p * 2)(*[v.data_ptr() for v, _ in ps])
        row = lambda ps: (ctypes.c_long * 2)(*[v.stride(0) for v, _ in ps])
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = _native.lib().lvae_image_f32_to_yuvsp(xd.data_ptr(), xd.stride(0), xd.stride(1), xd.stride(2), 72, 80, hw, 2, depth,
                                                   _native.YUV_SUBSAMPLINGS.index(sub), _native.YUV_SITINGS.index(siting), 1, 0, arr(ys), arr(uvs),
                                                   row(ys), row(uvs), st)
        assert rc == 0
        torch.cuda.synchronize()
        for i, f in enumerate(want):
            for (v, buf), p, off in ((ys[i], f.y, oy), (uvs[i], f.uv, ouv)):
                assert torch.equal(v.cpu(), p), (oy, ouv, i)
                mask = torch.ones(buf.numel(), dtype=torch.bool)
                mask[off:].as_strided(tuple(v.shape), v.stride()).fill_(False)
                assert int(mask.sum()) > 0 and bool((buf.cpu()[mask] == 7).all()), (oy, ouv, i)


def test_psnr_yuv_takes_semiplanar_frames():
    a = [_sp_frame(18, 22, 10, '420', 400 + i) for i in range(2)]
    b = [_sp_frame(18, 22, 10, '420', 410 + i) for i in range(2)]
    want = psnr_yuv([f.to_planar() for f in a], [f.to_planar() for f in b])
    assert psnr_yuv([f.to(DEV) for f in a], [f.to(DEV) for f in b]) == want == psnr_yuv(a, b)
    assert psnr_yuv(a[0].to(DEV), a[0])['psnr-avg'] == float('inf')


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
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


def _rgb(h, w, seed):
    return torch.from_numpy(seeded_init.synthetic_image_u8(h, w, seed)).permute(2, 0, 1).float().div(255)


def _frames(size, n, seed=80, **kw):
    return from_rgb01_any([_rgb(size[0], size[1], seed + i) for i in range(n)], **kw)


@pytest.mark.parametrize('name', ['qarv_base', 'qres34m'])
def test_compress_and_decompress_semiplanar_equal_planar(name):
    m = _seeded(name)
    for size, depth, sub, siting in (((64, 64), 10, '420', 'left'), ((48, 80), 12, '422', 'center')):
        planar = _frames(size, 2, depth=depth, subsampling=sub, siting=siting)
        sp = [f.to_semiplanar() for f in planar]
        blobs = m.compress_yuv(planar, siting=siting)
        assert m.compress_yuv(sp, siting=siting) == blobs                                   # CPU frames: uploaded as the file holds them
        assert m.compress_yuv([f.to(DEV) for f in sp], siting=siting) == blobs
        assert m.compress_yuv(sp[1:], siting=siting)[0] == blobs[1]
        kw = dict(depth=depth, subsampling=sub, siting=siting)
        recs = m.decompress_yuv(blobs, layout='semiplanar', **kw)
        want = m.decompress_yuv(blobs, **kw)
        for r, w in zip(recs, want):
            assert isinstance(r, YuvSpFrame) and r.y.is_cuda and r.size == size and _sp_equal(r, w.to_semiplanar())
        with pytest.raises(ValueError, match='mixed'):
            m.compress_yuv([planar[0], sp[1]], siting=siting)
    with pytest.raises(ValueError):
        m.decompress_yuv(blobs, depth=8, layout='semiplanar')


def test_per_frame_lambdas_on_semiplanar_frames():
    import struct
    m = _seeded('qarv_base')
    sp = [f.to_semiplanar() for f in _frames((64, 64), 3, depth=10, siting='left')]
    lmbs = [16, 256, 2048]
    blobs = m.compress_yuv(sp, lmb=lmbs, siting='left')
    for i, lmb in enumerate(lmbs):
        assert blobs[i] == m.compress_yuv([sp[i].to_planar()], lmb=lmb, siting='left')[0], i
        assert struct.unpack('f', blobs[i][4:8])[0] == lmb
    with pytest.raises(ValueError):
        _seeded('qres34m').compress_yuv(sp, lmb=64)


# ----------------------------------------------------------------------------------------------- sequences
P010 = dict(siting='left', matrix='bt2020', range='limited', chroma='bilinear')


@pytest.fixture(scope='module')
def p010_sequence():
    """5 left-sited bt2020 P010 frames of 48 x 80 coded by qarv_base with max_batch 2, and the single calls they must equal."""
    m = _seeded('qarv_base')
    frames = [f.to_semiplanar() for f in _frames((48, 80), 5, seed=500, depth=10, siting='left', matrix='bt2020')]
    single = [m.compress_yuv([f], **P010)[0] for f in frames]
    return m, frames, single, m.compress_yuv_sequence(frames, max_batch=2, **P010)


def test_sequence_frames_are_single_calls_whatever_max_batch(p010_sequence):
    m, frames, single, blob = p010_sequence
    info, blobs = yuvseq.unpack_sequence(blob)
    assert blobs == single
    want = dict(width=80, height=48, depth=10, subsampling='420', layout='semiplanar', model='qarv_base', gemm=m._prec, **P010)
    assert {k: info[k] for k in yuvseq.FIELDS} == want and info['frames'] == 5 and m._prec == 'f16x2'
    for mb in (1, 8):
        assert m.compress_yuv_sequence(frames, max_batch=mb, **P010) == blob
    assert m.yuv_sequence_info(blob)['lmb'] == [m._blob_lmb(b) for b in single]
    lmbs = [16, 64, 256, 1024, 2048]
    per_frame = m.compress_yuv_sequence(frames, lmb=lmbs, max_batch=2, **P010)
    assert m.yuv_sequence_info(per_frame)['lmb'] == lmbs
    assert yuvseq.unpack_sequence(per_frame)[1][3] == m.compress_yuv([frames[3]], lmb=1024, **P010)[0]


def test_sequence_from_a_raw_file(p010_sequence, tmp_path):
    m, frames, _, blob = p010_sequence
    path = tmp_path / 'clip.p010'
    write_yuv_sp(frames, path)
    kw = dict(depth=10, subsampling='420', layout='semiplanar', max_batch=2, **P010)
    assert m.compress_yuv_sequence(path, 80, 48, **kw) == blob
    assert yuvseq.unpack_sequence(m.compress_yuv_sequence(str(path), 80, 48, frames=3, **kw))[1] == yuvseq.unpack_sequence(blob)[1][:3]
    out = tmp_path / 'out.p010'
    assert m.decompress_yuv_sequence(blob, out_path=out, max_batch=2) == 5
    recs = m.decompress_yuv_sequence(blob)
    assert all(_sp_equal(a, b) for a, b in zip(read_yuv_sp(out, 80, 48), recs))


def test_sequence_decodes_with_no_parameters(p010_sequence):
    m, frames, single, blob = p010_sequence
    recs = m.decompress_yuv_sequence(blob)
    want = m.decompress_yuv(single, depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited', layout='semiplanar')
    assert len(recs) == 5 and all(isinstance(r, YuvSpFrame) and r.y.is_cuda and _sp_equal(r, w) for r, w in zip(recs, want))
    planar = m.decompress_yuv_sequence(blob, layout='planar', frames=range(1, 3))
    assert len(planar) == 2 and all(isinstance(p, YuvFrame) and _sp_equal(p.to_semiplanar(), w) for p, w in zip(planar, want[1:3]))
    with pytest.raises(ValueError):
        m.decompress_yuv_sequence(blob, layout='nv12')       # no such layout at 10 bits
    with pytest.raises(ValueError):
        m.decompress_yuv_sequence(blob[:-3])
    # random access: frames=[3] reads and decodes one blob
    seen = []
    orig = m._unpack_blob
    m._unpack_blob = lambda b: (seen.append(bytes(b)), orig(b))[1]
    try:
        one = m.decompress_yuv_sequence(blob, frames=[3])
    finally:
        del m._unpack_blob
    assert len(one) == 1 and _sp_equal(one[0], want[3]) and set(seen) == {single[3]}


def test_sequence_of_8_bit_i420_frames():
    m = _seeded('qarv_base')
    frames = from_rgb01([_rgb(48, 80, 600 + i) for i in range(5)], matrix='bt601', range='full')
    blob = m.compress_yuv_sequence(frames, matrix='bt601', range='full', max_batch=2)
    info, blobs = yuvseq.unpack_sequence(blob)
    assert (info['layout'], info['depth'], info['subsampling'], info['siting'], info['matrix'], info['range']) == ('i420', 8, '420', 'center', 'bt601', 'full')
    assert blobs == [m.compress_yuv420([f], matrix='bt601', range='full')[0] for f in frames]
    assert m.compress_yuv_sequence([YuvFrame(f.y, f.u, f.v) for f in frames], matrix='bt601', range='full', max_batch=8)[-sum(info['lengths']):] == b''.join(blobs)
    recs = m.decompress_yuv_sequence(blob)
    want = m.decompress_yuv(blobs, depth=8, subsampling='420', siting='center', matrix='bt601', range='full')
    for r, w in zip(recs, want):
        assert isinstance(r, Yuv420Frame) and r.fmt == 'i420' and all(torch.equal(p, q) for p, q in zip(r.planes(), w.planes()))
    nv12 = m.decompress_yuv_sequence(blob, frames=[4], layout='nv12')[0]
    assert nv12.fmt == 'nv12' and torch.equal(nv12.u, want[4].u) and torch.equal(nv12.v, want[4].v)


def test_sequence_refuses_another_model_or_arithmetic(p010_sequence):
    m, _, _, blob = p010_sequence
    with pytest.raises(ValueError, match='qarv_base.*qres34m'):
        _seeded('qres34m').decompress_yuv_sequence(blob)
    try:
        m.set_gemm_precision('bf16x3')
        with pytest.raises(ValueError, match="'f16x2'.*'bf16x3'"):
            m.decompress_yuv_sequence(blob)
    finally:
        m.set_gemm_precision('f16x2')
    assert len(m.decompress_yuv_sequence(blob, frames=[0])) == 1


def test_yuv_evaluate_reads_semiplanar_files(tmp_path):
    from lvae.evaluation import yuv_evaluate
    m = _seeded('qarv_base')
    frames = [f.to_semiplanar() for f in _frames((48, 80), 3, seed=700, depth=10, siting='left')]
    sp_path, pl_path = tmp_path / 'clip.p010', tmp_path / 'clip.yuv'
    write_yuv_sp(frames, sp_path)
    from lvae.utils.yuv import write_yuv
    write_yuv([f.to_planar() for f in frames], pl_path)
    kw = dict(batch=2, lmb=256, depth=10, siting='left')
    assert yuv_evaluate(m, sp_path, 80, 48, layout='semiplanar', **kw) == yuv_evaluate(m, pl_path, 80, 48, **kw)


# ----------------------------------------------------------------------------------------------- the script
def test_codec_script_container_round_trip(tmp_path):
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, box, out = tmp_path / 'in.p010', tmp_path / 'clip.lvys', tmp_path / 'out.p010'
    common = ['-m', 'qarv_base', '--synthetic', '3', '--batch', '2']
    enc = ['encode-yuv', str(src), str(box), '--size', '80', '48', '--container', '--layout', 'p010', '--siting', 'left', '--matrix', 'bt2020', '--lmb', '256']
    for cmd in (enc, ['decode-yuv', str(box), str(out)]):    # decoding takes no colour flag
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = _seeded('qarv_base')
    frames = read_yuv_sp(src, 80, 48)
    blob = box.read_bytes()
    assert len(frames) == 3 and blob == m.compress_yuv_sequence(frames, lmb=256, siting='left', matrix='bt2020', max_batch=8)
    assert src.stat().st_size == out.stat().st_size == 3 * 48 * 80 * 3
    recs = m.decompress_yuv([yuvseq.frame_blob(blob, yuvseq.yuv_sequence_info(blob), k) for k in range(3)], depth=10, siting='left', matrix='bt2020',
                            layout='semiplanar')
    assert all(_sp_equal(a, b) for a, b in zip(read_yuv_sp(out, 80, 48), recs))
