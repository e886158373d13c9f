"""not-gpu: the host side of the 8 / 10 / 12-bit, 4:2:0 / 4:2:2 / 4:4:4 YUV path.  The defining CPU expressions of lvae/utils/yuv.py
(yuv_to_rgb_expr2 / rgb_to_yuv_expr2) against the ITU-R definition in fp64 (tests/yuv_hbd_ref.py, separate code) and against the 8-bit
4:2:0 expressions they generalise, psnr_yuv's CPU path against numpy int64, raw files, and the argument checks of lvae_image_yuv_to_f32 /
lvae_image_f32_to_yuv / lvae_sse_u16, which come before any HIP call and so run without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import yuv_hbd_ref as ref
import yuv_ref
from lvae.metrics import PSNR_YUV_KEYS2, psnr_yuv, sse_u16
from lvae.utils.yuv import (YuvFrame, from_rgb01_any, read_yuv, rgb_to_yuv_expr, rgb_to_yuv_expr2, to_rgb01_any, write_yuv, yuv_to_rgb_expr,
                            yuv_to_rgb_expr2)

# extents of the noise planes: 34 x 38 (36 x 38 where the height must be even, 35 x 37 where nothing must)
EXTENT = {'420': (36, 38), '422': (34, 38), '444': (35, 37)}
# Bound 2e-6 on RGB values, as tests/test_yuv_host.py derives it for the 8-bit expression: values stay in [0, 1.2], the numerators of the
# two divisions are exact (the chroma filter is exact on integers up to 16 * 4095), the rest is at most three multiply-adds of fp32 constants.
BOUND = 2e-6


def _frame(planes, depth, sub):
    return YuvFrame(*planes, depth=depth, subsampling=sub)


# ----------------------------------------------------------------------------------------------- to RGB against the definition
@pytest.mark.parametrize('sub,siting', ref.LAYOUTS)
@pytest.mark.parametrize('depth', ref.DEPTHS)
def test_to_rgb_cpu_against_the_fp64_definition(depth, sub, siting):
    h, w = EXTENT[sub]
    for planes in (ref.noise_planes(h, w, depth, sub, 1), ref.ramp_planes(depth, sub)):
        for matrix in ref.MATRICES:
            for rng in ref.RANGES:
                for chroma in ('nearest', 'bilinear'):
                    x, sizes = to_rgb01_any([_frame(planes, depth, sub)], matrix=matrix, range=rng, chroma=chroma, siting=siting)
                    assert x.dtype == torch.float32 and sizes == [planes[0].shape] and tuple(x.shape) == (1, 3) + planes[0].shape
                    want = ref.yuv_to_rgb64(*planes, depth, sub, siting, matrix, rng, chroma)
                    err = float(np.abs(x[0].numpy().astype(np.float64) - want).max())
                    assert err <= BOUND, (matrix, rng, chroma, err)
                    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_left_sited_taps():
    """One chroma sample set: left siting puts it ON column 2k with halves on the odd columns beside it; vertically the centre filter."""
    from lvae.utils.yuv import _upsample2
    c = torch.zeros(3, 4, dtype=torch.int16)
    c[1, 2] = 16
    up = _upsample2(c, 10, '420', 'left', 'bilinear')
    want = torch.zeros(6, 8)
    want[1:5, 3:6] = 16 * torch.tensor([0.25, 0.75, 0.75, 0.25])[:, None] * torch.tensor([0.5, 1.0, 0.5])[None]
    assert torch.equal(up, want)
    up = _upsample2(c, 10, '422', 'left', 'bilinear')
    want = torch.zeros(3, 8)
    want[1, 3:6] = torch.tensor([8.0, 16.0, 8.0])
    assert torch.equal(up, want)
    c = torch.zeros(3, 4, dtype=torch.int16)
    c[0, 3] = 16                                            # the last chroma column: the odd column after it repeats it
    assert _upsample2(c, 10, '422', 'left', 'bilinear')[0].tolist() == [0, 0, 0, 0, 0, 8, 16, 16]
    assert torch.equal(_upsample2(c, 10, '444', 'left', 'bilinear'), c.float())           # no subsampled axis: siting has no effect
    assert torch.equal(_upsample2(c, 10, '420', 'left', 'nearest'), _upsample2(c, 10, '420', 'center', 'nearest'))


def test_canvas_padding_and_batches():
    sizes = [(6, 10), (62, 66), (64, 128)]
    planes = [ref.noise_planes(h, w, 10, '422', 10 + i) for i, (h, w) in enumerate(sizes)]
    x, got = to_rgb01_any([_frame(p, 10, '422') for p in planes], div=64, matrix='bt2020', range='full', siting='left')
    assert got == sizes and tuple(x.shape) == (3, 3, 64, 128)
    for i, p in enumerate(planes):
        want = ref.yuv_to_rgb64(*p, 10, '422', 'left', 'bt2020', 'full', 'bilinear', canvas=(64, 128))
        assert float(np.abs(x[i].numpy().astype(np.float64) - want).max()) <= BOUND, i
    with pytest.raises(ValueError):
        to_rgb01_any([_frame(planes[0], 10, '422'), _frame(ref.noise_planes(6, 10, 12, '422', 1), 12, '422')])


# ----------------------------------------------------------------------------------------------- from RGB against the definition
def _rgb_inputs(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3, h, w, generator=g) * 1.2 - 0.1        # values outside [0, 1] included
    x[:, :2, :2] = torch.tensor([0.0, 1.0, 2.0, -1.0]).view(1, 2, 2)
    return x


@pytest.mark.parametrize('sub,siting', ref.LAYOUTS)
@pytest.mark.parametrize('depth', ref.DEPTHS)
def test_from_rgb_cpu_against_the_fp64_definition(depth, sub, siting):
    h, w = EXTENT[sub]
    for matrix in ref.MATRICES:
        for rng in ref.RANGES:
            inside = total = 0
            for seed in (3, 4):
                x = _rgb_inputs(seed, h, w)
                want = ref.rgb_to_yuv64(x.numpy(), depth, sub, siting, matrix, rng)
                fr = from_rgb01_any(x.unsqueeze(0), depth=depth, subsampling=sub, siting=siting, matrix=matrix, range=rng)[0]
                assert (fr.size, fr.depth, fr.subsampling) == ((h, w), depth, sub) and tuple(fr.u.shape) == ref.chroma_shape(h, w, sub)
                assert fr.y.dtype == (torch.uint8 if depth == 8 else torch.int16)
                for got, w64 in zip(fr.planes(), want):
                    n, t = ref.check_codes(got.numpy(), w64, depth)
                    inside, total = inside + n, total + t
            # a condition, not a measurement: uniform values put 2 * guard of the samples there (0.02 / 0.08 / 0.32 % at 8 / 10 / 12 bits)
            assert inside <= 0.01 * total, (matrix, rng, inside, total)


def test_identity_with_the_8_bit_420_expressions():
    y, u, v = (torch.from_numpy(p) for p in yuv_ref.noise_planes(36, 38, 5))
    x = _rgb_inputs(6, 36, 38)
    x[0, 5, 5] = float('nan')
    for matrix in ('bt601', 'bt709'):
        for rng in ref.RANGES:
            for chroma in ('nearest', 'bilinear'):
                assert torch.equal(yuv_to_rgb_expr2(y, u, v, 8, '420', 'center', matrix, rng, chroma), yuv_to_rgb_expr(y, u, v, matrix, rng, chroma))
            for a, b in zip(rgb_to_yuv_expr2(x, 8, '420', 'center', matrix, rng), rgb_to_yuv_expr(x, matrix, rng)):
                assert a.dtype == torch.uint8 and torch.equal(a, b)


def test_from_rgb_cpu_codes_of_white_black_and_nan():
    white = from_rgb01_any([torch.ones(3, 2, 2)], depth=10)[0]
    assert white.y.tolist() == [[940, 940], [940, 940]] and white.u.item() == 512 and white.v.item() == 512
    black = from_rgb01_any([torch.zeros(3, 2, 2)], depth=12, subsampling='444')[0]
    assert black.y.tolist() == [[256, 256], [256, 256]] and black.u.tolist() == [[2048, 2048], [2048, 2048]]
    assert from_rgb01_any([torch.ones(3, 2, 2)], depth=10, range='full')[0].y.tolist() == [[1023, 1023], [1023, 1023]]
    red = from_rgb01_any([torch.tensor([1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2)], depth=10, range='full', siting='left')[0]
    assert red.v.item() == 1023                             # 512 + 511.5 rounds to 1024 and is clamped
    x = _rgb_inputs(7, 6, 10)
    z, w = x.clone(), x.clone()
    z[0, 0, 0], w[0, 0, 0] = float('nan'), 0.0              # NaN counts as 0
    for sub, siting in ref.LAYOUTS:
        kw = dict(depth=10, subsampling=sub, siting=siting)
        assert all(torch.equal(p, q) for p, q in zip(from_rgb01_any([z], **kw)[0].planes(), from_rgb01_any([w], **kw)[0].planes()))
    a = from_rgb01_any(x.unsqueeze(0), sizes=[(4, 6)], depth=10, subsampling='422')[0]
    b = from_rgb01_any([x[:, :4, :6]], depth=10, subsampling='422')[0]
    assert a.size == (4, 6) and all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))
    with pytest.raises(ValueError):
        from_rgb01_any([torch.zeros(3, 5, 6)], subsampling='420')
    with pytest.raises(ValueError):
        from_rgb01_any([torch.zeros(3, 6, 5)], subsampling='422')
    with pytest.raises(ValueError):
        from_rgb01_any([torch.zeros(3, 6, 6)], depth=16)
    with pytest.raises(ValueError):
        from_rgb01_any([torch.zeros(3, 6, 6)], siting='top')
    assert from_rgb01_any([torch.zeros(3, 5, 7)], subsampling='444')[0].size == (5, 7)


# ----------------------------------------------------------------------------------------------- the frame type and files
def test_frame_type():
    z16, z8 = (lambda *s: torch.zeros(*s, dtype=torch.int16)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    fr = YuvFrame(z16(6, 8), z16(3, 4), z16(3, 4), depth=10)
    assert fr.size == (6, 8) and fr.device.type == 'cpu' and len(fr.planes()) == 3 and fr.cpu() is fr and fr.to('cpu') is fr
    assert YuvFrame(z8(5, 7), z8(5, 7), z8(5, 7), subsampling='444').size == (5, 7)
    assert YuvFrame(z16(5, 8), z16(5, 4), z16(5, 4), depth=12, subsampling='422').size == (5, 8)
    a = np.full((6, 8), 1023, dtype=np.uint16)              # numpy uint16 is reinterpreted, not copied
    fr = YuvFrame(a, a[:3, :4].copy(), a[:3, :4].copy(), depth=10)
    assert fr.y.dtype == torch.int16 and int(fr.y[0, 0]) == 1023
    a[0, 0] = 7
    assert int(fr.y[0, 0]) == 7
    for bad in (1024, 65535):                               # beyond 10 bits; the high bit of the container
        b = np.zeros((6, 8), dtype=np.uint16)
        b[2, 3] = bad
        with pytest.raises(ValueError, match='codes outside'):
            YuvFrame(b, a[:3, :4].copy(), a[:3, :4].copy(), depth=10)
        with pytest.raises(ValueError, match='codes outside'):
            YuvFrame(a, a[:3, :4].copy(), b[:3, :4].copy(), depth=10)
    assert YuvFrame(np.full((6, 8), 4095, dtype=np.uint16), a[:3, :4].copy(), a[:3, :4].copy(), depth=12).depth == 12
    for args, kw in (((z16(5, 8), z16(2, 4), z16(2, 4)), dict(depth=10)),                      # odd height at 4:2:0
                     ((z16(6, 7), z16(6, 3), z16(6, 3)), dict(depth=10, subsampling='422')),   # odd width at 4:2:2
                     ((z16(6, 8), z16(3, 4), z16(3, 3)), dict(depth=10)),                      # a chroma plane of the wrong size
                     ((z16(6, 8), z16(3, 4), z16(3, 4)), dict(depth=8)),                       # 16-bit planes at depth 8
                     ((z8(6, 8), z8(3, 4), z8(3, 4)), dict(depth=10)),                         # bytes at depth 10
                     ((z16(6, 8), z16(3, 4), z16(3, 4)), dict(depth=16)),
                     ((z16(6, 8), z16(3, 4), z16(3, 4)), dict(depth=10, subsampling='411')),
                     ((z16(0, 8), z16(0, 8), z16(0, 8)), dict(depth=10, subsampling='444'))):
        with pytest.raises(ValueError):
            YuvFrame(*args, **kw)


@pytest.mark.parametrize('depth,sub', [(8, '420'), (10, '420'), (10, '422'), (12, '444'), (8, '444')])
def test_yuv_file_round_trip(tmp_path, depth, sub):
    h, w = (6, 10) if sub != '444' else (5, 7)
    frames = [_frame(ref.noise_planes(h, w, depth, sub, 30 + i), depth, sub) for i in range(3)]
    path = tmp_path / 'a.yuv'
    write_yuv(frames, path)
    ch, cw = ref.chroma_shape(h, w, sub)
    per = (h * w + 2 * ch * cw) * (1 if depth == 8 else 2)
    assert path.stat().st_size == 3 * per
    raw = path.read_bytes()
    if depth > 8:                                           # int16 tensors hold the container's bits: little-endian, value in the low bits
        want = b''.join(p.numpy().view(np.uint16).astype('<u2').tobytes() for f in frames for p in f.planes())
        assert raw[0] + 256 * raw[1] == int(frames[0].y[0, 0]) < (1 << depth)
    else:
        want = b''.join(p.numpy().tobytes() for f in frames for p in f.planes())
    assert raw == want
    back = read_yuv(path, w, h, sub, depth)
    assert len(back) == 3 and all((b.size, b.depth, b.subsampling) == ((h, w), depth, sub) for b in back)
    for a, b in zip(frames, back):
        assert all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))
    assert len(read_yuv(path, w, h, sub, depth, frames=2)) == 2
    write_yuv(back[:1], path, append=True)
    assert path.read_bytes() == raw + raw[:per]
    assert len(read_yuv(path, w, h, sub, depth)) == 4


def test_yuv_file_argument_errors(tmp_path):
    path = tmp_path / 'bad.yuv'
    path.write_bytes(bytes(181))
    with pytest.raises(ValueError, match='whole number'):
        read_yuv(path, 10, 6, depth=10)
    path.write_bytes(bytes(180))
    assert len(read_yuv(path, 10, 6, depth=10)) == 1 and len(read_yuv(path, 10, 6)) == 2
    with pytest.raises(ValueError, match='whole number'):
        read_yuv(path, 10, 6, '422', 10)
    for w, h, sub in ((9, 6, '420'), (10, 5, '420'), (9, 6, '422'), (0, 6, '444')):
        with pytest.raises(ValueError):
            read_yuv(path, w, h, sub, 10)
    with pytest.raises(ValueError):
        read_yuv(path, 10, 6, depth=9)
    with pytest.raises(ValueError):
        read_yuv(path, 10, 6, '440')
    path.write_bytes(b'\x00\x04' * 90)                      # 1024: beyond 10 bits
    with pytest.raises(ValueError, match='codes outside'):
        read_yuv(path, 10, 6, depth=10)
    assert read_yuv(path, 10, 6, depth=12)[0].y[0, 0].item() == 1024


# ----------------------------------------------------------------------------------------------- psnr_yuv
def test_psnr_yuv_cpu_against_numpy():
    cases = [(10, '420', (6, 10)), (10, '444', (5, 7)), (12, '422', (6, 10)), (8, '422', (6, 10))]
    for depth, sub, (h, w) in cases:
        a, b = ref.noise_planes(h, w, depth, sub, 20), ref.noise_planes(h, w, depth, sub, 21)
        row = psnr_yuv(_frame(a, depth, sub), _frame(b, depth, sub))
        assert tuple(row) == PSNR_YUV_KEYS2 and PSNR_YUV_KEYS2[-1] == 'psnr-avg'
        peak = 255.0 * 2 ** (depth - 8)                     # 1020 at 10 bits, HM / VTM's convention
        ps, tot, cnt = [], 0, 0
        for k, pa, pb in zip('yuv', a, b):
            sse = int(((pa.astype(np.int64) - pb.astype(np.int64)) ** 2).sum())
            mse = sse / float(pa.size)
            assert row['mse-' + k] == mse and row['psnr-' + k] == 10 * math.log10(peak ** 2 / mse)
            ps.append(row['psnr-' + k])
            tot, cnt = tot + sse, cnt + pa.size
        assert row['psnr-yuv'] == (6 * ps[0] + ps[1] + ps[2]) / 8
        assert row['psnr-avg'] == 10 * math.log10(peak ** 2 / (tot / float(cnt)))
    one = np.zeros((2, 2), dtype=np.uint16)
    off = one + 1                                           # every sample off by one: mse 1, psnr 20 log10(1020)
    row = psnr_yuv(_frame((one, one, one), 10, '444'), _frame((off, off, off), 10, '444'))
    assert row['mse-y'] == 1.0 and row['psnr-y'] == 10 * math.log10(1020.0 ** 2) and row['psnr-avg'] == row['psnr-y'] == row['psnr-yuv']
    fa = _frame(ref.noise_planes(6, 10, 10, '420', 20), 10, '420')
    same = psnr_yuv([fa], [fa])[0]
    assert all(same[k] == 0.0 for k in ('mse-y', 'mse-u', 'mse-v'))
    assert all(same[k] == math.inf for k in ('psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv', 'psnr-avg'))
    lo, hi = torch.zeros(3, 5, dtype=torch.int16), torch.full((3, 5), -1, dtype=torch.int16)          # 0 against 65535
    assert sse_u16([(lo, hi), (hi, lo), (hi, hi)]) == [15 * 65535 * 65535, 15 * 65535 * 65535, 0]
    with pytest.raises(ValueError):
        psnr_yuv([fa], [_frame(ref.noise_planes(6, 10, 10, '422', 1), 10, '422')])
    with pytest.raises(ValueError):
        psnr_yuv([fa], [_frame(ref.noise_planes(6, 10, 12, '420', 1), 12, '420')])
    with pytest.raises(ValueError):
        sse_u16([(torch.zeros(0, 5, dtype=torch.int16), torch.zeros(0, 5, dtype=torch.int16))])
    with pytest.raises(ValueError):
        sse_u16([(torch.zeros(2, 5, dtype=torch.uint8), torch.zeros(2, 5, dtype=torch.uint8))])


# ----------------------------------------------------------------------------------------------- the C entries without a GPU
def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _to_f32(L, y=1 << 20, u=1 << 21, v=1 << 22, rows=(64, 32, 32), hw=((8, 8),), B=1, depth=10, sub=0, siting=0, matrix=1, rng=0, chroma=1,
            dst=1 << 23, dst_img=3 * 64 * 64, H=64, W=64, null=()):
    n = max(B, 1)
    ptr = lambda name, val: None if name in null else _arr(ctypes.c_void_p, [val] * n)
    row = lambda name, val: None if name in null else _arr(ctypes.c_long, [val] * n)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * n)[:n] for x in p])
    return L.lvae_image_yuv_to_f32(ptr('y', y), ptr('u', u), ptr('v', v), row('y_row', rows[0]), row('u_row', rows[1]), row('v_row', rows[2]),
                                   hp, B, depth, sub, siting, matrix, rng, chroma, None if 'dst' in null else dst, dst_img, H, W, None)


def _to_yuv(L, src=1 << 20, strides=(3 * 64 * 64, 64 * 64, 64), H=64, W=64, y=1 << 21, u=1 << 22, v=1 << 23, rows=(64, 32, 32), hw=((8, 8),),
            B=1, depth=10, sub=0, siting=0, matrix=1, rng=0, null=()):
    n = max(B, 1)
    ptr = lambda name, val: None if name in null else _arr(ctypes.c_void_p, [val] * n)
    row = lambda name, val: None if name in null else _arr(ctypes.c_long, [val] * n)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * n)[:n] for x in p])
    return L.lvae_image_f32_to_yuv(None if 'src' in null else src, *strides, H, W, hp, B, depth, sub, siting, matrix, rng, ptr('y', y), ptr('u', u),
                                   ptr('v', v), row('y_row', rows[0]), row('u_row', rows[1]), row('v_row', rows[2]), None)


def _sse(L, a=1 << 20, b=1 << 21, rows=(8, 8), hw=((8, 8),), n=1, out=1 << 22, null=()):
    m = max(n, 1)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * m)[:m] for x in p])
    return L.lvae_sse_u16(None if 'a' in null else _arr(ctypes.c_void_p, [a] * m), None if 'a_row' in null else _arr(ctypes.c_long, [rows[0]] * m),
                          None if 'b' in null else _arr(ctypes.c_void_p, [b] * m), None if 'b_row' in null else _arr(ctypes.c_long, [rows[1]] * m),
                          hp, n, None if 'out' in null else out, None)


def test_hbd_kernels_reject_bad_arguments_without_gpu():
    """Every case returns -22 from the host-side checks: no pointer here is real, so reaching a launch would not go unnoticed."""
    from lvae import _native
    L = _native.lib()
    for call, side in ((_to_f32, 'dst'), (_to_yuv, 'src')):
        for null in ('y', 'u', 'v', 'y_row', 'u_row', 'v_row', 'hw', side):
            assert call(L, null=(null,)) == -22, (call.__name__, null)
        assert call(L, B=0) == -22 and call(L, B=-1) == -22
        assert call(L, H=0) == -22 and call(L, W=0) == -22
        for bad in ((0, 8), (8, 0), (7, 8), (8, 7), (66, 8), (8, 66)):                      # 4:2:0: empty, odd, beyond the canvas
            assert call(L, hw=(bad,)) == -22, (call.__name__, bad)
        for bad in ((0, 8), (8, 7), (66, 8), (8, 66)):                                      # 4:2:2: an odd height is fine, an odd width is not
            assert call(L, sub=1, hw=(bad,)) == -22, (call.__name__, bad)
        for bad in ((0, 7), (7, 0), (65, 7), (7, 65)):                                      # 4:4:4: any extent inside the canvas
            assert call(L, sub=2, hw=(bad,), rows=(64, 64, 64)) == -22, (call.__name__, bad)
        assert call(L, hw=((8, 8), (8, 7)), B=2) == -22                                     # ... in a later frame of the batch
        assert call(L, rows=(7, 32, 32)) == -22 and call(L, rows=(64, 3, 32)) == -22 and call(L, rows=(64, 32, 3)) == -22
        assert call(L, sub=2, rows=(64, 7, 64)) == -22 and call(L, sub=2, rows=(64, 64, 7)) == -22     # 4:4:4: chroma rows hold w samples
        for depth in (0, 7, 9, 11, 14, 16):
            assert call(L, depth=depth) == -22, (call.__name__, depth)
        assert call(L, sub=3) == -22 and call(L, sub=-1) == -22 and call(L, siting=2) == -22 and call(L, siting=-1) == -22
        assert call(L, matrix=3) == -22 and call(L, matrix=-1) == -22 and call(L, rng=2) == -22 and call(L, rng=-1) == -22
        assert call(L, y=0) == -22 and call(L, u=0) == -22 and call(L, v=0) == -22          # a null entry of a plane array
    assert _to_f32(L, chroma=2) == -22
    assert _to_f32(L, B=2, hw=((8, 8), (8, 8)), dst_img=3 * 64 * 64 - 1) == -22             # images that overlap
    assert _to_yuv(L, strides=(3 * 64 * 64, 64 * 64, 63)) == -22                            # strides that do not hold the canvas
    assert _to_yuv(L, strides=(3 * 64 * 64, 64 * 63, 64)) == -22
    for null in ('a', 'a_row', 'b', 'b_row', 'hw', 'out'):
        assert _sse(L, null=(null,)) == -22, null
    assert _sse(L, n=0) == -22 and _sse(L, a=0) == -22 and _sse(L, b=0) == -22
    assert _sse(L, hw=((0, 8),)) == -22 and _sse(L, hw=((8, 0),)) == -22                    # planes of 0 rows / columns
    assert _sse(L, rows=(7, 8)) == -22 and _sse(L, rows=(8, 7)) == -22
    assert _sse(L, hw=((8, 8), (0, 8)), n=2) == -22


def test_abi_declares_the_hbd_entries():
    import os
    import re
    from lvae import _native
    assert {'lvae_image_yuv_to_f32', 'lvae_image_f32_to_yuv', 'lvae_sse_u16'} <= set(_native.SIGNATURES)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lvae_hip.h')).read()
    for group, prefix, names in (('SUBSAMPLINGS', 'SUB_', ('420', '422', '444')), ('SITINGS', 'SITING_', ('CENTER', 'LEFT')),
                                 ('MATRICES2', '', ('BT601', 'BT709', 'BT2020'))):
        for code, name in enumerate(names):                 # a name's code on the Python side is its index
            assert re.search(rf'LVAE_YUV_{prefix}{name}\s*=\s*{code}\b', hdr), name
            assert getattr(_native, 'YUV_' + group)[code] == name.lower()
    assert _native.YUV_MATRICES == ('bt601', 'bt709')       # the 8-bit 4:2:0 entries keep their two matrices
