"""not-gpu: semi-planar high-bit-depth frames (P010 / P012 / P210 / P212) and the LVYS sequence container on the host -- the layout as torch
ops (YuvSpFrame.to_planar / YuvFrame.to_semiplanar, which the GPU tests use as their reference), the raw files, the container's header and
its refusals, the rule of which layouts exist (utils.yuvseq.check_layout) with utils.yuv.FrameFormat for every frame kind, and the argument
checks of the two native entries (they return before any HIP call)."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from lvae import _native
from lvae.utils import yuvseq
from lvae.utils.yuv import (SP_LAYOUTS, FrameFormat, Yuv420Frame, YuvFrame, YuvSpFrame, from_rgb01_any, frame_bytes2, read_yuv, read_yuv_sp,
                            to_rgb01, to_rgb01_any, write_frames, write_yuv, write_yuv_sp)

CASES = [(10, '420'), (12, '420'), (10, '422'), (12, '422')]


def _words(shape, seed):
    return np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)


def _sp_frame(h, w, depth, sub, seed):
    """Random 16-bit words: the low 16 - depth bits are garbage."""
    return YuvSpFrame(_words((h, w), seed), _words((h >> (sub == '420'), w), seed + 1), depth, sub)


def _equal(a, b):
    return (type(a), a.depth, a.subsampling, a.size) == (type(b), b.depth, b.subsampling, b.size) and \
        all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))


@pytest.mark.parametrize('depth,sub', CASES)
def test_to_planar_and_to_semiplanar_are_inverses(depth, sub):
    h, w = 6, 22                                             # chroma width 11: odd
    sp = _sp_frame(h, w, depth, sub, 1)
    pl = sp.to_planar()
    assert isinstance(pl, YuvFrame) and (pl.depth, pl.subsampling, pl.size) == (depth, sub, (h, w))
    assert tuple(pl.u.shape) == (h >> (sub == '420'), w // 2)
    y, uv = sp.y.numpy().view(np.uint16), sp.uv.numpy().view(np.uint16)
    assert np.array_equal(pl.y.numpy(), (y >> (16 - depth)).astype(np.int16))
    assert np.array_equal(pl.u.numpy(), (uv[:, 0::2] >> (16 - depth)).astype(np.int16))
    assert np.array_equal(pl.v.numpy(), (uv[:, 1::2] >> (16 - depth)).astype(np.int16))
    back = pl.to_semiplanar()                                # the words with their low bits cleared
    low = (1 << (16 - depth)) - 1
    assert np.array_equal(back.y.numpy().view(np.uint16), y & ~np.uint16(low)) and np.array_equal(back.uv.numpy().view(np.uint16), uv & ~np.uint16(low))
    assert _equal(back.to_planar(), pl) and _equal(back.to_planar().to_semiplanar(), back)
    # planar -> semi-planar -> planar on codes that did not come from words
    g = np.random.default_rng(2)
    cs = (h >> (sub == '420'), w // 2)
    fr = YuvFrame(*(g.integers(0, 1 << depth, s).astype(np.uint16) for s in ((h, w), cs, cs)), depth=depth, subsampling=sub)
    assert _equal(fr.to_semiplanar().to_planar(), fr)


@pytest.mark.parametrize('depth,sub', CASES)
def test_low_bits_do_not_change_to_planar(depth, sub):
    sp = _sp_frame(6, 22, depth, sub, 3)
    low = (1 << (16 - depth)) - 1
    clean = YuvSpFrame((sp.y.numpy().view(np.uint16) & ~np.uint16(low)), (sp.uv.numpy().view(np.uint16) & ~np.uint16(low)), depth, sub)
    ones = YuvSpFrame((sp.y.numpy().view(np.uint16) | np.uint16(low)), (sp.uv.numpy().view(np.uint16) | np.uint16(low)), depth, sub)
    assert not torch.equal(clean.y, ones.y)
    assert _equal(clean.to_planar(), sp.to_planar()) and _equal(ones.to_planar(), sp.to_planar())
    assert torch.equal(to_rgb01_any([sp])[0], to_rgb01_any([sp.to_planar()])[0]) and torch.equal(to_rgb01_any([ones])[0], to_rgb01_any([clean])[0])


def test_frame_accepts_both_uv_shapes_and_rejects_the_rest():
    y, uv = _words((4, 6), 4), _words((2, 6), 5)
    a, b = YuvSpFrame(y, uv), YuvSpFrame(y, uv.reshape(2, 3, 2))
    assert _equal(a, b) and tuple(b.uv.shape) == (2, 6) and a.size == (4, 6) and len(a.planes()) == 2 and a.cpu() is a and a.to('cpu') is a
    for bad in (dict(depth=8), dict(depth=16), dict(subsampling='444')):
        with pytest.raises(ValueError):
            YuvSpFrame(y, uv, **bad)
    with pytest.raises(ValueError):
        YuvSpFrame(y, _words((4, 6), 6))                     # a 4:2:0 chroma plane has h / 2 rows
    with pytest.raises(ValueError):
        YuvSpFrame(_words((4, 5), 7), _words((2, 5), 8))     # odd width
    with pytest.raises(ValueError):
        YuvSpFrame(y.astype(np.uint8), uv)
    with pytest.raises(ValueError):
        YuvFrame(_words((4, 6), 1).astype(np.uint8), *[_words((2, 3), 2).astype(np.uint8)] * 2).to_semiplanar()     # 8-bit: no such layout
    with pytest.raises(ValueError):
        from_rgb01_any(torch.rand(1, 3, 4, 6), depth=8, layout='semiplanar')


@pytest.mark.parametrize('name', sorted(SP_LAYOUTS))
def test_raw_file_round_trip_and_size(tmp_path, name):
    depth, sub = SP_LAYOUTS[name]
    h, w = 6, 22
    frames = [_sp_frame(h, w, depth, sub, 10 + 2 * i) for i in range(3)]
    path = tmp_path / f'clip.{name}'
    write_yuv_sp(frames[:2], path)
    write_yuv_sp(frames[2:], path, append=True)
    per = 2 * (h * w + 2 * (w // 2) * (h >> (sub == '420')))
    assert path.stat().st_size == 3 * per == 3 * frame_bytes2(w, h, sub, depth)
    back = read_yuv_sp(path, w, h, depth, sub)
    assert len(back) == 3 and all(_equal(a, b) for a, b in zip(back, frames))
    assert _equal(read_yuv_sp(path, w, h, depth, sub, frames=1, start=2)[0], frames[2]) and len(read_yuv_sp(path, w, h, depth, sub, frames=2)) == 2
    raw = np.fromfile(path, dtype='<u2')                     # the Y plane, then the UV plane, little-endian words
    assert np.array_equal(raw[:h * w].reshape(h, w), frames[0].y.numpy().view(np.uint16))
    assert np.array_equal(raw[h * w:per // 2].reshape(-1, w), frames[0].uv.numpy().view(np.uint16))
    with pytest.raises(ValueError):
        read_yuv_sp(path, w + 2, h, depth, sub)              # not a whole number of frames
    with pytest.raises(ValueError):
        read_yuv_sp(path, w, h, 8, sub)
    # the planar file of the same codes holds as many bytes
    write_yuv([f.to_planar() for f in frames], tmp_path / 'planar.yuv')
    assert (tmp_path / 'planar.yuv').stat().st_size == 3 * per
    assert _equal(read_yuv(tmp_path / 'planar.yuv', w, h, sub, depth)[1], frames[1].to_planar())


# ----------------------------------------------------------------------------------------------- the LVYS container
META = dict(width=22, height=6, depth=10, subsampling='420', siting='left', matrix='bt2020', range='full', chroma='nearest', layout='semiplanar',
            model='qarv_base', gemm='bf16x3')
BLOBS = [b'first', b'', b'\x00\x01\x02' * 100]


def test_container_round_trip_and_info():
    blob = yuvseq.pack_sequence(META, BLOBS)
    assert blob[:4] == b'LVYS' and yuvseq.is_yuv_sequence(blob) and not yuvseq.is_yuv_sequence(b'LVTL....')
    info, frames = yuvseq.unpack_sequence(blob)
    assert frames == BLOBS and info == yuvseq.yuv_sequence_info(blob)
    assert {k: info[k] for k in yuvseq.FIELDS} == META and info['frames'] == 3 and info['lengths'] == [5, 0, 300] and info['version'] == 1
    table = yuvseq.HEAD_BYTES + len('qarv_base') + len('bf16x3')
    assert info['offsets'] == [table + 12, table + 17, table + 17] and len(blob) == table + 12 + 305
    assert struct.unpack_from('<3I', blob, table) == (5, 0, 300)
    assert yuvseq.frame_blob(blob, info, 2) == BLOBS[2]
    assert yuvseq.frame_indexes(info) == [0, 1, 2] and yuvseq.frame_indexes(info, range(1, 3)) == [1, 2] and yuvseq.frame_indexes(info, [-1, 0]) == [2, 0]
    with pytest.raises(IndexError):
        yuvseq.frame_indexes(info, [3])
    assert yuvseq.unpack_sequence(yuvseq.pack_sequence(META, []))[1] == []


FIELD_VALUES = dict(width=[2, 4096], height=[2, 2160], depth=[12], subsampling=['422'], siting=['center'], matrix=['bt601', 'bt709'], range=['limited'],
                    chroma=['bilinear'], layout=['planar'], model=['qres34m_lossless'], gemm=['fp32', 'f16x2'])


@pytest.mark.parametrize('field', yuvseq.FIELDS)
def test_every_header_field_survives(field):
    for value in FIELD_VALUES[field]:
        meta = dict(META, **{field: value})
        info = yuvseq.yuv_sequence_info(yuvseq.pack_sequence(meta, BLOBS))
        assert {k: info[k] for k in yuvseq.FIELDS} == meta, (field, value)
    for meta in (dict(META, depth=8, subsampling='420', siting='center', matrix='bt601', layout='nv12'),
                 dict(META, depth=8, subsampling='444', layout='planar', width=7, height=5)):
        info = yuvseq.yuv_sequence_info(yuvseq.pack_sequence(meta, BLOBS))
        assert {k: info[k] for k in yuvseq.FIELDS} == meta


def test_malformed_containers_raise():
    blob = yuvseq.pack_sequence(META, BLOBS)
    table = yuvseq.HEAD_BYTES + len('qarv_base') + len('bf16x3')
    bad = {'magic': b'LVYT' + blob[4:], 'version': blob[:4] + b'\x02' + blob[5:], 'short': blob[:10], 'empty': b'',
           'truncated blobs': blob[:-1], 'trailing bytes': blob + b'\x00', 'truncated table': blob[:table + 5], 'truncated names': blob[:yuvseq.HEAD_BYTES + 3],
           'count beyond the blob': blob[:yuvseq.HEAD_BYTES - 4] + struct.pack('<I', 1 << 30) + blob[yuvseq.HEAD_BYTES:],
           'length beyond the blob': blob[:table] + struct.pack('<I', 1 << 31) + blob[table + 4:]}
    for k, code in enumerate((3, 3, 2, 3, 2, 2, 4)):         # depth, subsampling, siting, matrix, range, chroma, layout: one past the last code
        o = 14 + k
        bad[f'enum {k}'] = blob[:o] + bytes([code]) + blob[o + 1:]
    bad['layout that the depth does not have'] = blob[:14] + b'\x00' + blob[15:]                 # depth 8, semi-planar
    bad['odd width'] = blob[:6] + struct.pack('<I', 21) + blob[10:]
    bad['zero height'] = blob[:10] + struct.pack('<I', 0) + blob[14:]
    for what, b in bad.items():
        with pytest.raises(ValueError):
            yuvseq.yuv_sequence_info(b)
        with pytest.raises(ValueError):
            yuvseq.unpack_sequence(b)
    assert yuvseq.yuv_sequence_info(blob)['depth'] == 10     # (the offsets patched above are the header's)
    for meta in (dict(META, depth=9), dict(META, layout='p010'), dict(META, width=21), dict(META, depth=8), dict(META, model=''),
                 dict(META, layout='i420'), {k: v for k, v in META.items() if k != 'gemm'}):
        with pytest.raises(ValueError):
            yuvseq.pack_sequence(meta, BLOBS)


def test_container_does_not_depend_on_max_batch():
    """A CPU stub codec whose blob depends on the frame and its lambda only, as the models' batch rows do."""
    frames = [_sp_frame(6, 22, 10, '420', 30 + i) for i in range(5)]
    calls = []

    def compress(chunk, lmb=None):
        calls.append(len(chunk))
        lm = [lmb] * len(chunk) if lmb is None or isinstance(lmb, (int, float)) else lmb
        return [struct.pack('<f', -1.0 if v is None else v) + f.uv.numpy().tobytes()[:7 + int(f.y[0, 0]) % 2] for f, v in zip(chunk, lm)]
    out = {}
    for mb in (1, 3, 8):
        calls.clear()
        out[mb] = yuvseq.pack_sequence(META, yuvseq.code_sequence(compress, frames, mb))
        assert calls == {1: [1] * 5, 3: [3, 2], 8: [5]}[mb]
    assert out[1] == out[3] == out[8]
    lmbs = [16, 32, 64, 128, 256]
    per_frame = [yuvseq.code_sequence(compress, frames, mb, lmbs) for mb in (1, 3)]
    assert per_frame[0] == per_frame[1] and [struct.unpack('<f', b[:4])[0] for b in per_frame[0]] == lmbs
    assert yuvseq.code_sequence(compress, frames, 2, 64.0) == yuvseq.code_sequence(compress, frames, 5, [64.0] * 5)
    reader = lambda start, n: frames[start:start + n]        # a file read max_batch frames at a time
    assert yuvseq.code_sequence(compress, reader, 2) == yuvseq.code_sequence(compress, frames, 8)
    with pytest.raises(ValueError):
        yuvseq.code_sequence(compress, frames, 2, lmbs[:4])
    with pytest.raises(ValueError):
        yuvseq.code_sequence(compress, reader, 2, lmbs + [1])


# ----------------------------------------------------------------------------------------------- which layouts exist, and FrameFormat
def _layout_exists(layout, depth, sub, siting, matrix):
    """The rule, written out: planar frames at any depth and subsampling; semi-planar ones at 10 or 12 bits and '420' or '422'; 'i420' /
    'nv12' at 8 bits, '420', 'center' and bt601 or bt709."""
    if layout == 'planar':
        return True
    if layout == 'semiplanar':
        return depth in (10, 12) and sub in ('420', '422')
    return depth == 8 and sub == '420' and siting == 'center' and matrix in ('bt601', 'bt709')


def test_check_layout_is_the_rule_at_all_216_combinations():
    import itertools
    combos = list(itertools.product(('planar', 'semiplanar', 'i420', 'nv12'), (8, 10, 12), ('420', '422', '444'), ('center', 'left'),
                                    ('bt601', 'bt709', 'bt2020')))
    assert len(combos) == 216
    for c in combos:
        if _layout_exists(*c):
            yuvseq.check_layout(*c)
            assert tuple(FrameFormat(*c)) == c[:3]           # the constructor asks the same rule; siting and matrix are not kept
        else:
            with pytest.raises(ValueError):
                yuvseq.check_layout(*c)
            with pytest.raises(ValueError):
                FrameFormat(*c)
    assert sum(_layout_exists(*c) for c in combos) == 54 + 24 + 2 + 2
    ok = ('planar', 10, '420', 'left', 'bt2020')
    for k, bad in ((0, 'p010'), (0, None), (1, 9), (1, 16), (1, '10'), (2, '440'), (2, 420), (3, 'top'), (4, 'bt470')):   # outside the enumerations
        with pytest.raises(ValueError):
            yuvseq.check_layout(*ok[:k], bad, *ok[k + 1:])


def test_the_one_byte_codes_of_the_container_keep_their_values():
    """The header stores indexes into these tuples: their values and their order ARE the file format."""
    assert yuvseq.DEPTHS == (8, 10, 12) and yuvseq.SUBSAMPLINGS == ('420', '422', '444') and yuvseq.SITINGS == ('center', 'left')
    assert yuvseq.MATRICES == ('bt601', 'bt709', 'bt2020') and yuvseq.RANGES == ('limited', 'full') and yuvseq.CHROMA == ('nearest', 'bilinear')
    assert yuvseq.LAYOUTS == ('planar', 'semiplanar', 'i420', 'nv12')
    blob = yuvseq.pack_sequence(META, [])
    assert tuple(blob[14:21]) == (1, 0, 1, 2, 1, 0, 1)       # META's depth 10, '420', 'left', 'bt2020', 'full', 'nearest', 'semiplanar'


FORMAT_CASES = [('planar', 8, '444'), ('planar', 10, '422'), ('planar', 12, '420'), ('semiplanar', 10, '420'), ('semiplanar', 12, '422'),
                ('i420', 8, '420'), ('nv12', 8, '420')]
FRAME_KIND = {'planar': YuvFrame, 'semiplanar': YuvSpFrame, 'i420': Yuv420Frame, 'nv12': Yuv420Frame}


def _seeded_frame(fmt, h, w, seed):
    """fmt.new(...) with seeded codes in its planes: bytes, codes of `depth` bits, or -- semi-planar -- 16-bit words, low bits and all."""
    fr, g = fmt.new(h, w, 'cpu'), np.random.default_rng(seed)
    for p in fr.planes():
        hi = 65536 if fmt.layout == 'semiplanar' else 1 << fmt.depth
        p.copy_(torch.from_numpy(g.integers(0, hi, tuple(p.shape)).astype(np.uint8 if fmt.depth == 8 else np.uint16).view(np.uint8 if fmt.depth == 8 else np.int16)))
    return fr


def _same_planes(a, b):
    return type(a) is type(b) and a.size == b.size and len(a.planes()) == len(b.planes()) and \
        all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))


@pytest.mark.parametrize('case', FORMAT_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_frame_format_new_files_and_crop(tmp_path, case):
    h, w = 12, 16
    fmt = FrameFormat(*case)
    assert fmt == case and (fmt.layout, fmt.depth, fmt.subsampling) == case and hash(fmt) == hash(FrameFormat(*case))
    with pytest.raises(AttributeError):
        fmt.depth = 8                                        # a value, not a record
    new = fmt.new(h, w, 'cpu')
    assert type(new) is FRAME_KIND[fmt.layout] and new.size == (h, w) and FrameFormat.of(new) == fmt
    assert all(p.dtype == (torch.uint8 if fmt.depth == 8 else torch.int16) for p in new.planes())
    frames = [_seeded_frame(fmt, h, w, 40 + i) for i in range(3)]
    assert all(FrameFormat.of(f) == fmt for f in frames)
    # files: write_frames then read
    path = tmp_path / 'clip.yuv'
    write_frames(frames[:2], path)
    write_frames(frames[2:], path, append=True)
    sx, sy = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}[fmt.subsampling]
    per = (h * w + 2 * (h >> sy) * (w >> sx)) * (1 if fmt.depth == 8 else 2)
    assert fmt.frame_bytes(w, h) == per and path.stat().st_size == 3 * per
    back = fmt.read(path, w, h)
    assert len(back) == 3 and all(_same_planes(a, b) for a, b in zip(back, frames))
    assert _same_planes(fmt.read(path, w, h, frames=1, start=2)[0], frames[2]) and len(fmt.read(path, w, h, frames=2)) == 2
    with pytest.raises(ValueError, match='whole number'):
        fmt.read(path, w + 2, h)
    if fmt.subsampling != '444':
        with pytest.raises(ValueError, match='does not fit'):
            fmt.read(path, w + 1, h)
    # crop: views of the frame's planes, and the window of the frame's conversion
    fr = frames[0]
    win = fmt.crop(fr, 4, 8, 8, 8)
    assert type(win) is type(fr) and win.size == (8, 8) and FrameFormat.of(win) == fmt
    assert all(p.untyped_storage().data_ptr() == q.untyped_storage().data_ptr() for p, q in zip(win.planes(), fr.planes()))
    assert torch.equal(win.y, fr.y[4:12, 8:16])
    convert = to_rgb01 if fmt.layout in ('i420', 'nv12') else to_rgb01_any
    whole, part = convert([fr], chroma='nearest')[0], convert([win], chroma='nearest')[0]
    assert tuple(part.shape) == (1, 3, 8, 8) and torch.equal(part, whole[:, :, 4:12, 8:16])
    assert not torch.equal(part, whole[:, :, 4:12, 6:14])    # (the window is told apart from its neighbour)


# ----------------------------------------------------------------------------------------------- the native entries' argument checks
def test_argument_validation_without_gpu():
    """-22 before any HIP call: null pointers and entries, B <= 0, odd extents, short strides, unsupported depth / subsampling.  The plane
    addresses are never dereferenced on this path."""
    L = _native.lib()
    one = lambda v, t=ctypes.c_void_p: (t * 1)(v)
    ok = dict(y=one(4096), uv=one(8192), y_row=one(8, ctypes.c_long), uv_row=one(8, ctypes.c_long), hw=(ctypes.c_int * 2)(4, 8), B=1, depth=10, sub=0,
              siting=0, matrix=1, range=0, chroma=1, f32=ctypes.c_void_p(1 << 20))
    cases = [dict(y=None), dict(uv=None), dict(y_row=None), dict(uv_row=None), dict(hw=None), dict(f32=None), dict(y=one(None)), dict(uv=one(None)),
             dict(B=0), dict(B=-1), dict(depth=8), dict(depth=16), dict(sub=2), dict(sub=3), dict(siting=2), dict(matrix=3), dict(range=2),
             dict(hw=(ctypes.c_int * 2)(3, 8)), dict(hw=(ctypes.c_int * 2)(4, 7)), dict(hw=(ctypes.c_int * 2)(0, 8)), dict(hw=(ctypes.c_int * 2)(4, 10)),
             dict(y_row=one(7, ctypes.c_long)), dict(uv_row=one(7, ctypes.c_long))]
    for change in cases:
        a = dict(ok, **change)
        assert L.lvae_image_yuvsp_to_f32(a['y'], a['uv'], a['y_row'], a['uv_row'], a['hw'], a['B'], a['depth'], a['sub'], a['siting'], a['matrix'],
                                         a['range'], a['chroma'], a['f32'], 3 * 64, 8, 8, None) == -22, change
        assert L.lvae_image_f32_to_yuvsp(a['f32'], 3 * 64, 64, 8, 8, 8, a['hw'], a['B'], a['depth'], a['sub'], a['siting'], a['matrix'], a['range'],
                                         a['y'], a['uv'], a['y_row'], a['uv_row'], None) == -22, change
    a = dict(ok, chroma=2)
    assert L.lvae_image_yuvsp_to_f32(a['y'], a['uv'], a['y_row'], a['uv_row'], a['hw'], 1, 10, 0, 0, 1, 0, 2, a['f32'], 3 * 64, 8, 8, None) == -22
    # a 4:2:2 frame may have an odd height: the same odd-height frame that 4:2:0 refused is only refused for its stride here
    assert L.lvae_image_f32_to_yuvsp(ok['f32'], 3 * 64, 64, 8, 8, 8, (ctypes.c_int * 2)(3, 8), 1, 10, 1, 0, 1, 0, ok['y'], ok['uv'], ok['y_row'],
                                     one(6, ctypes.c_long), None) == -22
    assert L.lvae_image_f32_to_yuvsp(ok['f32'], 3 * 64, 64, 7, 8, 8, ok['hw'], 1, 10, 0, 0, 1, 0, ok['y'], ok['uv'], ok['y_row'], ok['uv_row'], None) == -22
