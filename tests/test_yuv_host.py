"""not-gpu: the host side of the YUV 4:2:0 path.  The defining CPU expressions of lvae/utils/yuv.py against the ITU-R definition in fp64
(tests/yuv_ref.py, separate code), psnr_yuv420's CPU path against numpy int64, raw .yuv files, and the argument checks of
lvae_image_yuv420_to_f32 / lvae_image_f32_to_yuv420 / lvae_sse_u8, which come before any HIP call and so run without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import yuv_ref
from lvae.metrics import PSNR_YUV_KEYS, psnr_yuv420, sse_u8
from lvae.utils.yuv import Yuv420Frame, from_rgb01, read_yuv420, to_rgb01, write_yuv420


def _frame(planes, fmt='i420'):
    y, u, v = (torch.from_numpy(p) for p in planes)
    return Yuv420Frame('i420', y, u, v).as_format(fmt)


# ----------------------------------------------------------------------------------------------- to_rgb01 against the definition
# Bound 2e-6: |values| <= ~1.2; a result is one IEEE division ((Y - 16) / 219 and (C - 128) / 224 have exact numerators: the chroma
# filter is exact on bytes) and at most three multiply-adds, each operation rounded to 2^-24 relative: <= ~8 * 1.2 * 6e-8 = 6e-7,
# plus the fp32 rounding of the four constants (<= 6e-8 relative each).
BOUND = 2e-6


@pytest.mark.parametrize('matrix,rng,chroma', yuv_ref.COMBOS)
def test_to_rgb01_cpu_against_the_fp64_definition(matrix, rng, chroma):
    for planes in (yuv_ref.all_values_planes(), yuv_ref.noise_planes(6, 10, 1), yuv_ref.noise_planes(62, 66, 2)):
        for fmt in ('i420', 'nv12'):
            x, sizes = to_rgb01([_frame(planes, fmt)], matrix=matrix, range=rng, chroma=chroma)
            assert x.dtype == torch.float32 and sizes == [planes[0].shape] and tuple(x.shape) == (1, 3) + planes[0].shape
            ref = yuv_ref.yuv_to_rgb64(*planes, matrix, rng, chroma)
            err = float(np.abs(x[0].numpy().astype(np.float64) - ref).max())
            assert err <= BOUND, (fmt, err)
            assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_to_rgb01_cpu_pads_a_batch_to_one_canvas():
    sizes = [(6, 10), (62, 66), (64, 128)]
    planes = [yuv_ref.noise_planes(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    x, got = to_rgb01([_frame(p) for p in planes], div=64, matrix='bt601', range='full')
    assert got == sizes and tuple(x.shape) == (3, 3, 64, 128)
    for i, p in enumerate(planes):
        ref = yuv_ref.yuv_to_rgb64(*p, 'bt601', 'full', 'bilinear', canvas=(64, 128))
        assert float(np.abs(x[i].numpy().astype(np.float64) - ref).max()) <= BOUND, i


def test_bilinear_taps_are_the_3_4_1_4_filter():
    """A chroma plane with one sample set: the separable (1/4, 3/4 | 3/4, 1/4) footprint around its 2x2 block, clamped at the edges."""
    from lvae.utils.yuv import _upsample2
    _upsample = lambda c, chroma: _upsample2(c, 8, '420', 'center', chroma)      # the 8-bit 4:2:0 expressions' upsampling
    c = torch.zeros(3, 4, dtype=torch.uint8)
    c[1, 2] = 16
    up = _upsample(c, 'bilinear')
    k = torch.tensor([0.25, 0.75, 0.75, 0.25])
    want = torch.zeros(6, 8)
    want[1:5, 3:7] = 16 * k[:, None] * k[None]
    assert torch.equal(up, want)
    c = torch.zeros(3, 4, dtype=torch.uint8)
    c[0, 0] = 16                                            # a corner: the clamped neighbour is the sample itself
    want = torch.zeros(6, 8)
    w = torch.tensor([1.0, 0.75, 0.25])
    want[:3, :3] = 16 * w[:, None] * w[None]
    assert torch.equal(_upsample(c, 'bilinear'), want)
    assert torch.equal(_upsample(c, 'nearest')[:2, :2], torch.full((2, 2), 16.0))


# ----------------------------------------------------------------------------------------------- the bits of the two expressions
def _expr_digests():
    """SHA-256 of the raw result bytes of yuv_to_rgb_expr (every colour combination, three inputs) and of the three planes of
    rgb_to_yuv_expr (every matrix / range pair, the five images of yuv_ref.rgb_batch with NaN / +-inf replaced as the clamp does)."""
    import hashlib
    from lvae.utils.yuv import rgb_to_yuv_expr, yuv_to_rgb_expr
    sha = lambda *ts: hashlib.sha256(b''.join(t.contiguous().numpy().tobytes() for t in ts)).hexdigest()
    inputs = {'all_values': yuv_ref.all_values_planes(), 'noise_6x10': yuv_ref.noise_planes(6, 10, 1), 'noise_62x66': yuv_ref.noise_planes(62, 66, 2)}
    out = {}
    for name, planes in inputs.items():
        y, u, v = (torch.from_numpy(p) for p in planes)
        for matrix, rng, chroma in yuv_ref.COMBOS:
            out[f'yuv_to_rgb/{name}/{matrix}/{rng}/{chroma}'] = sha(yuv_to_rgb_expr(y, u, v, matrix, rng, chroma))
    z = torch.nan_to_num(yuv_ref.rgb_batch(), nan=0.0, posinf=1.0, neginf=0.0)
    for matrix in ('bt601', 'bt709'):
        for rng in ('limited', 'full'):
            planes = [rgb_to_yuv_expr(img, matrix, rng) for img in z]
            for k, p in enumerate('yuv'):
                out[f'rgb_to_yuv/{matrix}/{rng}/{p}'] = sha(*[q[k] for q in planes])
    return out


def test_8_bit_420_expressions_keep_their_bits():
    """tests/golden/yuv420_expr_sha256.json was written by _expr_digests when yuv_to_rgb_expr / rgb_to_yuv_expr were expressions of
    their own, before they became the general ones at depth 8, '420', 'center': every result byte is still the same."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'yuv420_expr_sha256.json')) as f:
        want = json.load(f)
    assert len(want) == 3 * 8 + 4 * 3
    assert _expr_digests() == want


# ----------------------------------------------------------------------------------------------- from_rgb01 against the definition
def _rgb_inputs(seed, h=62, w=66):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3, h, w, generator=g) * 1.2 - 0.1        # values outside [0, 1] included
    x[:, :2, :2] = torch.tensor([0.0, 1.0, 2.0, -1.0]).view(1, 2, 2)
    return x


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
@pytest.mark.parametrize('rng', ['limited', 'full'])
def test_from_rgb01_cpu_against_the_fp64_definition(matrix, rng):
    inside = total = 0
    for seed in (3, 4):
        x = _rgb_inputs(seed)
        want = yuv_ref.rgb_to_yuv64(x.numpy(), matrix, rng)
        for fmt in ('i420', 'nv12'):
            fr = from_rgb01(x.unsqueeze(0), fmt=fmt, matrix=matrix, range=rng)[0]
            assert fr.fmt == fmt and fr.size == (62, 66)
            for got, w64 in zip((fr.y, fr.u, fr.v), want):
                n, t = yuv_ref.check_bytes(got.numpy(), w64)
                inside, total = inside + n, total + t
    assert inside <= 0.01 * total, (inside, total)          # the guard band must not swallow the comparison


def test_from_rgb01_cpu_sizes_nan_and_range():
    x = _rgb_inputs(5)
    a = from_rgb01(x.unsqueeze(0), sizes=[(6, 10)])[0]
    b = from_rgb01([x[:, :6, :10]])[0]
    assert a.size == (6, 10) and all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))
    z = x.clone()
    z[0, 0, 0] = float('nan')                               # NaN counts as 0
    w = x.clone()
    w[0, 0, 0] = 0.0
    assert all(torch.equal(p, q) for p, q in zip(from_rgb01([z])[0].planes(), from_rgb01([w])[0].planes()))
    white, black = from_rgb01([torch.ones(3, 2, 2)])[0], from_rgb01([torch.zeros(3, 2, 2)])[0]
    assert white.y.tolist() == [[235, 235], [235, 235]] and white.u.item() == 128 and white.v.item() == 128
    assert black.y.tolist() == [[16, 16], [16, 16]] and black.u.item() == 128
    assert from_rgb01([torch.ones(3, 2, 2)], range='full')[0].y.tolist() == [[255, 255], [255, 255]]
    red = from_rgb01([torch.tensor([1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2)], range='full')[0]
    assert red.v.item() == 255                              # 128 + 127.5 rounds to 256 and is clamped
    with pytest.raises(ValueError):
        from_rgb01([torch.zeros(3, 5, 6)])
    with pytest.raises(ValueError):
        from_rgb01([torch.zeros(3, 6, 6)], matrix='bt2020')


def test_round_trip_of_bytes_is_close():
    """yuv -> rgb -> yuv returns the luma within 1 and -- for a frame whose chroma is constant per 2x2 block's neighbourhood (nearest
    upsampling) -- the chroma within 1, wherever the RGB values did not clip."""
    y, u, v = yuv_ref.noise_planes(8, 8, 7)
    y = (y.astype(np.int64) % 100 + 80).astype(np.uint8)
    u, v = (u.astype(np.int64) % 40 + 108).astype(np.uint8), (v.astype(np.int64) % 40 + 108).astype(np.uint8)
    x, _ = to_rgb01([_frame((y, u, v))], chroma='nearest')
    assert float(x.min()) > 0 and float(x.max()) < 1
    fr = from_rgb01(x)[0]
    for got, want in zip((fr.y, fr.u, fr.v), (y, u, v)):
        assert int((got.numpy().astype(np.int64) - want.astype(np.int64)).__abs__().max()) <= 1


# ----------------------------------------------------------------------------------------------- psnr_yuv420
def test_psnr_yuv420_cpu_against_numpy():
    a, b = yuv_ref.noise_planes(6, 10, 20), yuv_ref.noise_planes(6, 10, 21)
    c = yuv_ref.noise_planes(62, 66, 22)
    d = tuple(np.clip(p.astype(np.int64) + 1, 0, 255).astype(np.uint8) for p in c)
    rows = psnr_yuv420([_frame(a), _frame(c, 'nv12')], [_frame(b, 'nv12'), _frame(d)])
    for row, (p, q) in zip(rows, [(a, b), (c, d)]):
        assert tuple(row) == PSNR_YUV_KEYS
        ps = []
        for k, pa, pb in zip('yuv', p, q):
            sse = int(((pa.astype(np.int64) - pb.astype(np.int64)) ** 2).sum())
            mse = sse / float(pa.size)
            assert row['mse-' + k] == mse and row['psnr-' + k] == 10 * math.log10(255.0 ** 2 / mse)
            ps.append(row['psnr-' + k])
        assert row['psnr-yuv'] == (6 * ps[0] + ps[1] + ps[2]) / 8
    same = psnr_yuv420(_frame(a), _frame(a))
    assert all(same[k] == 0.0 for k in ('mse-y', 'mse-u', 'mse-v')) and all(same[k] == math.inf for k in ('psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv'))
    assert sse_u8([(torch.zeros(3, 5, dtype=torch.uint8), torch.full((3, 5), 255, dtype=torch.uint8))]) == [15 * 255 * 255]
    with pytest.raises(ValueError):
        psnr_yuv420([_frame(a)], [_frame(c)])
    with pytest.raises(ValueError):
        sse_u8([(torch.zeros(0, 5, dtype=torch.uint8), torch.zeros(0, 5, dtype=torch.uint8))])


# ----------------------------------------------------------------------------------------------- files and argument errors
@pytest.mark.parametrize('fmt', ['i420', 'nv12'])
def test_yuv_file_round_trip(tmp_path, fmt):
    frames = [_frame(yuv_ref.noise_planes(6, 10, 30 + i), fmt) for i in range(3)]
    path = tmp_path / 'a.yuv'
    write_yuv420(frames, path)
    assert path.stat().st_size == 3 * 6 * 10 * 3 // 2
    raw = path.read_bytes()
    f0 = frames[0]
    assert raw[:60] == f0.y.numpy().tobytes()
    if fmt == 'i420':
        assert raw[60:75] == f0.u.numpy().tobytes() and raw[75:90] == f0.v.numpy().tobytes()
    else:
        assert raw[60:90:2] == f0.u.contiguous().numpy().tobytes() and raw[61:90:2] == f0.v.contiguous().numpy().tobytes()
    back = read_yuv420(path, 10, 6, fmt)
    assert len(back) == 3 and all(b.fmt == fmt and b.size == (6, 10) for b in back)
    for a, b in zip(frames, back):
        assert all(torch.equal(p, q) for p, q in zip(a.planes(), b.planes()))
        assert torch.equal(a.u, b.u) and torch.equal(a.v, b.v)
    assert len(read_yuv420(path, 10, 6, fmt, frames=2)) == 2
    other = read_yuv420(path, 10, 6, 'nv12' if fmt == 'i420' else 'i420')          # the same bytes read as the other layout differ
    assert not torch.equal(other[0].u, frames[0].u)
    write_yuv420(frames[:1], path, append=True)
    assert len(read_yuv420(path, 10, 6, fmt)) == 4


def test_yuv_argument_errors(tmp_path):
    path = tmp_path / 'bad.yuv'
    path.write_bytes(bytes(91))
    with pytest.raises(ValueError, match='whole number'):
        read_yuv420(path, 10, 6)
    path.write_bytes(bytes(90))
    for w, h in ((9, 6), (10, 5), (0, 6)):
        with pytest.raises(ValueError):
            read_yuv420(path, w, h)
    with pytest.raises(ValueError):
        read_yuv420(path, 10, 6, fmt='yv12')
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError):
        Yuv420Frame('i420', z(5, 6), z(2, 3), z(2, 3))                              # odd height
    with pytest.raises(ValueError):
        Yuv420Frame('i420', z(6, 7), z(3, 3), z(3, 3))                              # odd width
    with pytest.raises(ValueError):
        Yuv420Frame('i420', z(6, 8), z(3, 4), z(3, 3))                              # a chroma plane of the wrong size
    with pytest.raises(ValueError):
        Yuv420Frame('nv12', z(6, 8), uv=z(3, 8))
    with pytest.raises(ValueError):
        to_rgb01([Yuv420Frame('i420', z(6, 8), z(3, 4), z(3, 4))], chroma='bicubic')
    with pytest.raises(ValueError):
        to_rgb01([])


# ----------------------------------------------------------------------------------------------- the C entries without a GPU
def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _to_f32(L, y=1 << 20, u=1 << 21, v=1 << 22, rows=(64, 32, 32), hw=((8, 8),), B=1, fmt=0, matrix=1, rng=0, chroma=1, dst=1 << 23,
            dst_img=3 * 64 * 64, H=64, W=64, null=()):
    n = max(B, 1)
    ptr = lambda name, val: None if name in null else _arr(ctypes.c_void_p, [val] * n)
    row = lambda name, val: None if name in null else _arr(ctypes.c_long, [val] * n)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * n)[:n] for x in p])
    return L.lvae_image_yuv420_to_f32(ptr('y', y), ptr('u', u), ptr('v', v), row('y_row', rows[0]), row('u_row', rows[1]), row('v_row', rows[2]),
                                      hp, B, fmt, matrix, rng, chroma, None if 'dst' in null else dst, dst_img, H, W, None)


def _to_yuv(L, src=1 << 20, strides=(3 * 64 * 64, 64 * 64, 64), H=64, W=64, y=1 << 21, u=1 << 22, v=1 << 23, rows=(64, 32, 32), hw=((8, 8),),
            B=1, fmt=0, matrix=1, rng=0, null=()):
    n = max(B, 1)
    ptr = lambda name, val: None if name in null else _arr(ctypes.c_void_p, [val] * n)
    row = lambda name, val: None if name in null else _arr(ctypes.c_long, [val] * n)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * n)[:n] for x in p])
    return L.lvae_image_f32_to_yuv420(None if 'src' in null else src, *strides, H, W, hp, B, fmt, matrix, rng, ptr('y', y), ptr('u', u), ptr('v', v),
                                      row('y_row', rows[0]), row('u_row', rows[1]), row('v_row', rows[2]), None)


def _sse(L, a=1 << 20, b=1 << 21, rows=(8, 8), hw=((8, 8),), n=1, out=1 << 22, null=()):
    m = max(n, 1)
    hp = None if 'hw' in null else _arr(ctypes.c_int, [x for p in (list(hw) * m)[:m] for x in p])
    return L.lvae_sse_u8(None if 'a' in null else _arr(ctypes.c_void_p, [a] * m), None if 'a_row' in null else _arr(ctypes.c_long, [rows[0]] * m),
                         None if 'b' in null else _arr(ctypes.c_void_p, [b] * m), None if 'b_row' in null else _arr(ctypes.c_long, [rows[1]] * m),
                         hp, n, None if 'out' in null else out, None)


def test_yuv_kernels_reject_bad_arguments_without_gpu():
    """Every case returns -22 from the host-side checks: no pointer here is real, so reaching a launch would not go unnoticed."""
    from lvae import _native
    L = _native.lib()
    for call, side in ((_to_f32, 'dst'), (_to_yuv, 'src')):
        for null in ('y', 'u', 'v', 'y_row', 'u_row', 'v_row', 'hw', side):
            assert call(L, null=(null,)) == -22, (call.__name__, null)
        assert call(L, B=0) == -22 and call(L, B=-1) == -22
        assert call(L, H=0) == -22 and call(L, W=0) == -22
        for bad in ((0, 8), (8, 0), (7, 8), (8, 7), (66, 8), (8, 66)):                      # empty, odd, beyond the canvas
            assert call(L, hw=(bad,)) == -22, (call.__name__, bad)
        assert call(L, hw=((8, 8), (8, 7)), B=2) == -22                                     # ... in a later frame of the batch
        assert call(L, rows=(7, 32, 32)) == -22 and call(L, rows=(64, 3, 32)) == -22 and call(L, rows=(64, 32, 3)) == -22
        assert call(L, fmt=1, rows=(64, 7, 32)) == -22                                      # NV12: the UV rows hold w bytes
        assert call(L, fmt=2) == -22 and call(L, matrix=2) == -22 and call(L, rng=-1) == -22
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


def test_abi_declares_the_yuv_entries():
    from lvae import _native
    assert {'lvae_image_yuv420_to_f32', 'lvae_image_f32_to_yuv420', 'lvae_sse_u8'} <= set(_native.SIGNATURES)
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lvae_hip.h')).read()
    for group, names in (('FORMATS', ('I420', 'NV12')), ('MATRICES', ('BT601', 'BT709')), ('RANGES', ('LIMITED', 'FULL')), ('CHROMA', ('NEAREST', 'BILINEAR'))):
        for code, name in enumerate(names):                 # a name's code on the Python side is its index
            assert re.search(rf'LVAE_YUV_{name}\s*=\s*{code}\b', hdr), name
            assert getattr(_native, 'YUV_' + group)[code] == name.lower()
