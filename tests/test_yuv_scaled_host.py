"""not-gpu: YUV frames at reduced resolution, host side -- the argument checks of the Python surface (before anything touches a device), the
`LVYS` container around scaled entries, the CPU compositions of the tensor-level pair, and, through the C ABI without a GPU, the argument
checks of lvae_resample_yuv_to_f32 / lvae_resample_f32_to_yuv."""
import ctypes
import struct

import pytest
import torch

from lvae import _native
from lvae.utils import resample, yuvseq
from lvae.utils.image import resize
from lvae.utils.yuv import (FrameFormat, ScaledYuvBatch, YuvFrame, from_rgb01_any, from_rgb01_scaled, to_rgb01_any, to_rgb01_scaled)

META = dict(width=192, height=128, depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited', chroma='bilinear',
            layout='planar', model='qarv_base', gemm='f16x2')


def _frame(h=32, w=48, depth=10, sub='420', seed=0):
    g = torch.Generator().manual_seed(seed)
    sx, sy = (0, 0) if sub == '444' else (1, 1) if sub == '420' else (1, 0)
    mk = lambda r, c: torch.randint(0, 1 << depth, (r, c), generator=g).to(torch.uint8 if depth == 8 else torch.int16)
    return YuvFrame(mk(h, w), mk(h >> sy, w >> sx), mk(h >> sy, w >> sx), depth, sub)


class _Stub:
    """The argument checks of the model methods run before any model state is read: a bare CodecBase will do."""

    def __new__(cls):
        from lvae.models.base import CodecBase
        m = CodecBase.__new__(CodecBase)
        torch.nn.Module.__init__(m)
        m.variable_rate = True
        m.max_stride = 64
        return m


# ----------------------------------------------------------------------------------------------- argument checks
def test_scale_and_size_exclude_each_other():
    m, f = _Stub(), _frame()
    for kw in ({}, dict(scale=0.5, size=(16, 24))):
        with pytest.raises(ValueError, match='exactly one of scale and size'):
            m.compress_yuv_scaled([f], **kw)
    with pytest.raises(ValueError, match='ratios'):
        m.compress_yuv_scaled([f], scale=0.05)
    with pytest.raises(ValueError, match='filter'):
        m.compress_yuv_scaled([f], scale=0.5, filter='nearest')
    with pytest.raises(ValueError, match='not both'):
        m.compress_yuv_sequence([f], scale=0.5, size=(16, 24))


def test_scale_and_tile_exclude_each_other(tmp_path):
    from lvae.evaluation import yuv_evaluate
    m, f = _Stub(), _frame()
    with pytest.raises(ValueError, match='tile'):
        m.compress_yuv_sequence([f], scale=0.5, tile=(64, 128))
    with pytest.raises(ValueError, match='tile'):
        m.compress_yuv_sequence([f], size=(16, 24), tile=(64, 128))
    path = tmp_path / 'in.yuv'
    path.write_bytes(bytes(48 * 32 * 3 // 2))
    model = torch.nn.Linear(1, 1)                            # (yuv_evaluate asks it for a device only before the check)
    with pytest.raises(ValueError, match='scale and tile'):
        yuv_evaluate(model, str(path), 48, 32, scale=0.5, tile=(64, 128))


def test_mixed_frame_kinds_are_refused():
    m = _Stub()
    a, b = _frame(), _frame(depth=8)
    with pytest.raises(ValueError, match='mixed'):
        m.compress_yuv_scaled([a, b], scale=0.5)
    with pytest.raises(ValueError, match='mixed'):
        m.compress_yuv_scaled([a, a.to_semiplanar()], scale=0.5)
    with pytest.raises(ValueError, match='one size'):
        to_rgb01_scaled([a, _frame(16, 48)], (8, 24))
    with pytest.raises(ValueError, match='one size'):
        ScaledYuvBatch(FrameFormat.of(a), [a, _frame(16, 48)], (8, 24), 'bicubic', 1, 'cpu')
    with pytest.raises(ValueError, match='no frames'):
        m.compress_yuv_scaled([], scale=0.5)


def test_a_preview_off_the_chroma_grid_is_refused():
    m = _Stub()
    blob = resample.pack_scaled('bicubic', (128, 192), (64, 96), b'payload')
    m._unpack_blob = lambda payload: (payload, (64, 96), 'key')
    for size, sub in (((33, 48), '420'), ((32, 47), '422'), ((32, 47), '420')):
        with pytest.raises(ValueError, match=f'{size[0]} x {size[1]}.*subsampling {sub}'):
            m.decompress_yuv_scaled([blob], depth=10, subsampling=sub, size=size)
    with pytest.raises(ValueError, match='subsampling 420'):          # the original size itself, for a container of an odd image
        m.decompress_yuv_scaled([resample.pack_scaled('bicubic', (127, 192), (64, 96), b'payload')], subsampling='420')
    with pytest.raises(ValueError, match='semi-planar'):
        m.decompress_yuv_scaled([blob], depth=8, layout='semiplanar')
    with pytest.raises(ValueError, match='bad magic'):
        m.decompress_yuv_scaled([b'LVTL' + blob[4:]])
    with pytest.raises(ValueError, match='payload'):
        m.decompress_yuv_scaled([blob[:-1]])
    with pytest.raises(ValueError, match='does not fit subsampling'):
        from_rgb01_scaled(torch.zeros(1, 3, 16, 24), (9, 12))


# ----------------------------------------------------------------------------------------------- the sequence container
def test_the_sequence_header_does_not_change_with_scaled_entries():
    plain = [b'blob-of-frame-%d' % k for k in range(3)]
    scaled = [resample.pack_scaled('bicubic', (128, 192), (64, 96), b) for b in plain]
    a, b = yuvseq.pack_sequence(META, plain), yuvseq.pack_sequence(META, scaled)
    n = yuvseq.HEAD_BYTES + len(META['model']) + len(META['gemm'])
    assert a[:n] == b[:n]                                    # magic, version, every parameter, the names, the frame count
    info, entries = yuvseq.unpack_sequence(b)
    assert entries == scaled and all(resample.is_scaled(e) for e in entries) and not any(resample.is_scaled(e) for e in plain)
    assert {k: info[k] for k in META} == META and info['lengths'] == [len(e) for e in scaled]
    for e, p in zip(entries, plain):
        assert resample.unpack_scaled(e) == (dict(filter='bicubic', size=(128, 192), coded=(64, 96), payload_bytes=len(p),
                                                  offset=resample.HEAD_BYTES), p)
    for bad in (b[:-1], b + b'\0', b'LVRS' + b[4:]):
        with pytest.raises(ValueError):
            yuvseq.yuv_sequence_info(bad)
    with pytest.raises(ValueError):
        resample.scaled_info(scaled[0][:resample.HEAD_BYTES + 3])


def test_sequence_info_reads_lambdas_through_scaled_entries():
    m = _Stub()
    m._blob_lmb = lambda blob: float(struct.unpack('<f', blob[:4])[0])
    plain = [struct.pack('<f', v) + b'rest' for v in (16.0, 2048.0)]
    scaled = [resample.pack_scaled('lanczos3', (128, 192), (64, 96), b) for b in plain]
    assert m.yuv_sequence_info(yuvseq.pack_sequence(META, [scaled[0], plain[1]]))['lmb'] == [16.0, 2048.0]
    assert m.scaled_info(scaled[1])['lmb'] == 2048.0


def test_without_scale_the_sequence_is_the_parents(monkeypatch):
    """compress_yuv_sequence(scale=None) hands the frames to compress_yuv in the same chunks and packs what it returns: the bytes
    pack_sequence gives for the stub's blobs.  With scale= the chunks go to compress_yuv_scaled instead."""
    m = _Stub()
    m._prec, m.model_name = 'f16x2', 'qarv_base'
    fs = [_frame(128, 192, seed=k) for k in range(3)]
    calls = []

    def stub(chunk, **kw):
        calls.append(('plain', len(chunk), kw))
        return [b'P%d' % f.y[0, 0] for f in chunk]

    def stub_scaled(chunk, **kw):
        calls.append(('scaled', len(chunk), kw))
        return [resample.pack_scaled(kw['filter'], (128, 192), (64, 96), b'S%d' % f.y[0, 0]) for f in chunk]
    monkeypatch.setattr(m, 'compress_yuv', stub, raising=False)
    monkeypatch.setattr(m, 'compress_yuv_scaled', stub_scaled, raising=False)
    colour = dict(siting='left', matrix='bt2020', range='limited', chroma='bilinear')
    got = m.compress_yuv_sequence(fs, max_batch=2, lmb=[1, 2, 3], **colour)
    assert got == yuvseq.pack_sequence(META, [b'P%d' % f.y[0, 0] for f in fs])
    assert calls == [('plain', 2, dict(colour, lmb=[1.0, 2.0])), ('plain', 1, dict(colour, lmb=[3.0]))]
    calls.clear()
    got = m.compress_yuv_sequence(fs, max_batch=2, scale=0.5, filter='bicubic', **colour)
    assert [c[:2] for c in calls] == [('scaled', 2), ('scaled', 1)] and calls[0][2] == dict(colour, scale=0.5, size=None, filter='bicubic')
    assert yuvseq.unpack_sequence(got)[1] == [resample.pack_scaled('bicubic', (128, 192), (64, 96), b'S%d' % f.y[0, 0]) for f in fs]


# ----------------------------------------------------------------------------------------------- CPU frames: the composition
def test_cpu_frames_take_the_composition_of_the_cpu_paths():
    fs = [_frame(seed=1), _frame(seed=2)]
    kw = dict(matrix='bt2020', range='limited', chroma='bilinear', siting='left')
    want = resize(to_rgb01_any(fs, **kw)[0], (16, 24), 'bicubic', clamp=True)
    got = to_rgb01_scaled(fs, (16, 24), 'bicubic', **kw)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    padded = to_rgb01_scaled(fs, (16, 24), 'bicubic', (64, 64), **kw)
    assert tuple(padded.shape) == (2, 3, 64, 64) and torch.equal(padded[:, :, :16, :24], want)
    assert torch.equal(padded[:, :, 16:, :24], want[:, :, 15:16].expand(-1, -1, 48, -1)) and torch.equal(padded[:, :, :, 24:], padded[:, :, :, 23:24].expand(-1, -1, -1, 40))
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    how = dict(depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited')
    back = from_rgb01_scaled(x, (32, 48), 'bicubic', **how)
    for g, w in zip(back, from_rgb01_any(resize(x, (32, 48), 'bicubic'), **how)):
        assert g.size == (32, 48) and all(torch.equal(p, q) for p, q in zip(g.planes(), w.planes()))
    with pytest.raises(ValueError, match='canvas'):
        to_rgb01_scaled(fs, (16, 24), canvas=(8, 64))


# ----------------------------------------------------------------------------------------------- the C ABI without a GPU
def _in_call(**over):
    """lvae_resample_yuv_to_f32 on fake device addresses (nothing is launched: every case returns -22 first), one argument changed."""
    B = over.pop('B', 2)
    arr = lambda typ, vals: (typ * len(vals))(*vals)
    a = dict(y=arr(ctypes.c_void_p, [4096] * B), u=arr(ctypes.c_void_p, [8192] * B), v=arr(ctypes.c_void_p, [12288] * B),
             y_row=arr(ctypes.c_long, [96] * B), u_row=arr(ctypes.c_long, [48] * B), v_row=arr(ctypes.c_long, [48] * B),
             hw=arr(ctypes.c_int, [64, 96] * B), B=B, depth=10, sub=0, siting=0, matrix=1, range=0, chroma=1, layout=0, h_in=64, w_in=96,
             h_out=32, w_out=48, ystart=ctypes.c_void_p(256), ywgt=ctypes.c_void_p(512), ytaps=6, yspan=40, xstart=ctypes.c_void_p(768),
             xwgt=ctypes.c_void_p(1024), xtaps=6, xspan=24, dst=ctypes.c_void_p(65536), dst_img=3 * 64 * 64, H=64, W=64)
    a.update(over)
    return _native.lib().lvae_resample_yuv_to_f32(*a.values(), None)


def _out_call(**over):
    B = over.pop('B', 2)
    arr = lambda typ, vals: (typ * len(vals))(*vals)
    a = dict(src=ctypes.c_void_p(65536), src_img=3 * 64 * 128, src_plane=64 * 128, src_row=128, hw=arr(ctypes.c_int, [64, 96] * B), B=B, depth=10,
             sub=0, siting=1, matrix=1, range=0, layout=0, h_in=32, w_in=48, h_out=64, w_out=96, ystart=ctypes.c_void_p(256),
             ywgt=ctypes.c_void_p(512), ytaps=6, yspan=12, xstart=ctypes.c_void_p(768), xwgt=ctypes.c_void_p(1024), xtaps=6,
             y=arr(ctypes.c_void_p, [4096] * B), u=arr(ctypes.c_void_p, [8192] * B), v=arr(ctypes.c_void_p, [12288] * B),
             y_row=arr(ctypes.c_long, [96] * B), u_row=arr(ctypes.c_long, [48] * B), v_row=arr(ctypes.c_long, [48] * B))
    a.update(over)
    return _native.lib().lvae_resample_f32_to_yuv(*a.values(), None)


BAD_COMMON = [dict(B=0), dict(depth=9), dict(depth=16), dict(sub=3), dict(siting=2), dict(matrix=3), dict(range=2), dict(layout=2),
              dict(layout=1, depth=8, matrix=2), dict(layout=1, depth=8, siting=1), dict(layout=1, sub=2), dict(y=None), dict(u=None),
              dict(v=None), dict(y_row=None), dict(hw=None), dict(ytaps=65), dict(ytaps=-1), dict(xtaps=65), dict(yspan=0), dict(ystart=None),
              dict(xwgt=None), dict(ytaps=0), dict(xtaps=0), dict(h_out=0), dict(w_out=-1)]


@pytest.mark.parametrize('over', BAD_COMMON + [dict(dst=None), dict(chroma=2), dict(xspan=0), dict(H=31), dict(W=47), dict(dst_img=3 * 64 * 64 - 1),
                                               dict(h_out=7), dict(w_in=400, w_out=48), dict(hw=(ctypes.c_int * 4)(64, 96, 64, 94)),
                                               dict(hw=(ctypes.c_int * 4)(62, 96, 62, 96)), dict(h_in=63, hw=(ctypes.c_int * 4)(63, 96, 63, 96)),
                                               dict(y_row=(ctypes.c_long * 2)(96, 95)), dict(u_row=(ctypes.c_long * 2)(48, 47)),
                                               dict(y=(ctypes.c_void_p * 2)(4096, None)), dict(yspan=1024, h_in=1024, h_out=128, H=128, dst_img=3 * 128 * 64, hw=(ctypes.c_int * 4)(1024, 96, 1024, 96))],
                         ids=repr)
def test_the_in_entry_refuses_bad_arguments_without_a_gpu(over):
    assert _in_call(**over) == -22


@pytest.mark.parametrize('over', BAD_COMMON + [dict(src=None), dict(src_row=47), dict(src_plane=31 * 128 + 47), dict(src_img=2 * 64 * 128),
                                               dict(hw=(ctypes.c_int * 4)(64, 96, 64, 94)), dict(h_out=63, hw=(ctypes.c_int * 4)(63, 96, 63, 96)),
                                               dict(w_out=95, hw=(ctypes.c_int * 4)(64, 95, 64, 95)), dict(v_row=(ctypes.c_long * 2)(48, 47)),
                                               dict(h_out=2, hw=(ctypes.c_int * 4)(2, 96, 2, 96)),
                                               dict(h_in=1024, h_out=128, src_plane=1024 * 128, src_img=3 * 1024 * 128, yspan=1024, hw=(ctypes.c_int * 4)(128, 96, 128, 96))],
                         ids=repr)
def test_the_out_entry_refuses_bad_arguments_without_a_gpu(over):
    assert _out_call(**over) == -22


def test_the_entries_are_part_of_the_abi():
    assert {'lvae_resample_yuv_to_f32', 'lvae_resample_f32_to_yuv'} <= set(_native.SIGNATURES)
    assert len(_native.SIGNATURES['lvae_resample_yuv_to_f32'][1]) == 32 and len(_native.SIGNATURES['lvae_resample_f32_to_yuv'][1]) == 30
    assert not any('resample' in name for name in _native.OP_KINDS)      # no launch-plan kind
