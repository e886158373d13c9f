"""not-gpu: reduced-resolution coding, host side (lvae/utils/resample.py).  The tap tables against the window rule, resize_reference
against two independent implementations of the same rule (PIL's Image.resize on mode-'F' planes, torch's antialiased F.interpolate),
the scaled container, and the argument checks -- Python's and, through the C ABI without a GPU, those of the three lvae_resample_*
entry points."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

from lvae.utils import resample

GEOMETRIES = [((150, 200), (75, 100)), ((150, 200), (61, 77)), ((61, 77), (150, 200)), ((64, 64), (64, 64)), ((130, 70), (33, 210))]
IDS = ['{}x{}-{}x{}'.format(*a, *b) for a, b in GEOMETRIES]


@functools.lru_cache(maxsize=None)
def _plane(h, w):
    return np.random.default_rng(h * 1000 + w).random((h, w), dtype=np.float32)


# ----------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize('filt', resample.FILTERS)
@pytest.mark.parametrize('n_in,n_out', [(200, 100), (200, 77), (77, 200), (13, 5), (9, 3), (70, 210), (130, 33), (64, 8), (8, 64), (5, 5)])
def test_axis_table_follows_the_window_rule(filt, n_in, n_out):
    start, wgt = resample.axis_table(n_in, n_out, filt)
    assert start.dtype == np.int32 and wgt.dtype == np.float32 and start.shape == (n_out,) and wgt.shape[0] == n_out
    if n_in == n_out:                                    # the identity: callers skip the axis
        assert np.array_equal(start, np.arange(n_out)) and np.array_equal(wgt, np.ones((n_out, 1), np.float32))
        return
    a = resample.HALF_WIDTH[filt]
    s = n_in / n_out
    support = a * max(s, 1.0)
    counts = []
    for i in range(n_out):
        c = (i + 0.5) * s
        lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        assert start[i] == lo and 0 <= lo < hi <= n_in
        counts.append(hi - lo)
        assert not wgt[i, hi - lo:].any()                # zero padding behind the window
        assert abs(float(wgt[i].astype(np.float64).sum()) - 1.0) <= (hi - lo) * 2.0 ** -24
    assert wgt.shape[1] == max(counts)
    assert np.all(np.diff(start) >= 0)
    lo_w, hi_w = resample.axis_windows(n_in, n_out, filt)
    assert np.array_equal(lo_w, start) and np.array_equal(hi_w - lo_w, counts)
    # the span the kernel's tile is sized from covers every run of 16 output rows
    span = resample.tile_span(start, wgt.shape[1], n_in)
    for i in range(n_out):
        last = min(i + 15, n_out - 1)
        assert min(start[last] + wgt.shape[1], n_in) - start[i] <= span <= n_in


def test_weights_are_the_filters():
    """Spot values: bilinear 2:1 is the 4-tap triangle (1, 3, 3, 1) / 8; a Lanczos row is symmetric about its centre."""
    start, wgt = resample.axis_table(8, 4, 'bilinear')
    assert start[1] == 1 and np.allclose(wgt[1], np.array([1, 3, 3, 1]) / 8.0, atol=1e-7)
    start, wgt = resample.axis_table(200, 100, 'lanczos3')
    assert wgt.shape[1] == 12 and np.allclose(wgt[50], wgt[50][::-1], atol=1e-7) and wgt[50].min() < 0
    x = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5])
    assert np.allclose(resample._kernel('bicubic', x), [1.0, 0.5625, 0.0, -0.0625, 0.0, 0.0])


def test_same_size_axis_is_a_bit_copy():
    x = _plane(64, 64).astype(np.float64)
    for filt in resample.FILTERS:
        assert np.array_equal(resample.resize_reference(x, 64, 64, filt), x)
    y = resample.resize_reference(_plane(150, 200), 150, 100)          # the rows pass untouched: the horizontal pass alone
    start, wgt = resample.axis_table(200, 100)
    row = sum(_plane(150, 200).astype(np.float64)[7, np.minimum(start + j, 199)] * wgt[:, j].astype(np.float64) for j in range(wgt.shape[1]))
    assert np.allclose(y[7], row, rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------------------------- independent implementations
@pytest.mark.parametrize('filt', resample.FILTERS)
@pytest.mark.parametrize('src,dst', GEOMETRIES, ids=IDS)
def test_reference_against_pil(src, dst, filt):
    """PIL resamples mode-'F' planes with fp64 weights of the same window rule: within 1e-6 (fp32 weights and PIL's fp32 intermediate
    plane account for a few 1e-7)."""
    from PIL import Image
    x = _plane(*src)
    mode = {'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'lanczos3': Image.LANCZOS}[filt]
    want = np.asarray(Image.fromarray(x).resize((dst[1], dst[0]), mode), dtype=np.float64)
    got = resample.resize_reference(x, dst[0], dst[1], filt)
    err = np.abs(got - want).max()
    print(f'{src} -> {dst} {filt}: max|d| vs PIL = {err:.2e}')
    assert got.shape == tuple(dst) and err <= 1e-6


@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('src,dst', GEOMETRIES, ids=IDS)
def test_reference_against_torch_antialias(src, dst, filt):
    """torch's antialiased interpolate, align_corners=False: the same rule with the scale formed in fp32: within 2e-5."""
    x = torch.from_numpy(_plane(*src))[None, None]
    want = torch.nn.functional.interpolate(x, size=dst, mode=filt, antialias=True, align_corners=False)[0, 0].numpy().astype(np.float64)
    got = resample.resize_reference(_plane(*src), dst[0], dst[1], filt)
    err = np.abs(got - want).max()
    print(f'{src} -> {dst} {filt}: max|d| vs torch = {err:.2e}')
    assert err <= 2e-5


def test_clamp_and_leading_axes():
    x = (np.indices((3, 40, 60)).sum(0) % 2).astype(np.float64)            # a checkerboard: Lanczos overshoots on the way up
    y = resample.resize_reference(x, 90, 130, 'lanczos3')
    assert y.shape == (3, 90, 130) and (y.min() < 0 or y.max() > 1)
    yc = resample.resize_reference(x, 90, 130, 'lanczos3', clamp=True)
    assert yc.min() >= 0 and yc.max() <= 1 and np.array_equal(yc, np.clip(y, 0, 1))
    assert np.array_equal(y[1], resample.resize_reference(x[1], 90, 130, 'lanczos3'))


def test_resize_on_cpu_is_the_reference():
    from lvae.utils.image import resize, to_u8
    x = torch.rand(2, 3, 20, 30, generator=torch.Generator().manual_seed(0))
    want = resample.resize_reference(x.numpy(), 9, 41, 'bicubic', clamp=True).astype(np.float32)
    got = resize(x, (9, 41), filter='bicubic', clamp=True)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    u8 = resize(x, (9, 41), filter='bicubic', out='u8')
    assert len(u8) == 2 and torch.equal(u8[0], to_u8(got)[0])
    imgs = [(x[i].permute(1, 2, 0) * 255).to(torch.uint8) for i in range(2)]
    got8 = resize(imgs, (10, 15))
    want8 = resample.resize_reference(torch.stack(imgs).permute(0, 3, 1, 2).float().div(255).numpy(), 10, 15).astype(np.float32)
    assert np.array_equal(got8.numpy(), want8)
    with pytest.raises(ValueError):
        resize(x, (9, 41), filter='nearest')
    with pytest.raises(ValueError):
        resize(x, (9, 41), out='f16')
    with pytest.raises(ValueError):
        resize(x, (2, 41))                               # 20 -> 2 rows: beyond 1/8


# ----------------------------------------------------------------------------------------------- container
def test_container_round_trip():
    payload = bytes(range(200)) * 3
    blob = resample.pack_scaled('bicubic', (120, 180), (60, 90), payload)
    assert blob[:4] == b'LVRS' and len(blob) == resample.HEAD_BYTES + len(payload) and blob[resample.HEAD_BYTES:] == payload
    assert resample.is_scaled(blob) and not resample.is_scaled(payload) and not resample.is_scaled(b'')
    info, got = resample.unpack_scaled(blob)
    assert got == payload
    assert info == dict(filter='bicubic', size=(120, 180), coded=(60, 90), payload_bytes=len(payload), offset=resample.HEAD_BYTES)
    assert resample.scaled_info(blob) == info
    assert struct.unpack_from('<4sBB', blob) == (b'LVRS', 1, 1)
    assert resample.unpack_scaled(memoryview(blob))[1] == payload


def test_container_rejects_malformed_blobs():
    blob = bytearray(resample.pack_scaled('lanczos3', (120, 180), (60, 90), b'x' * 50))
    bad = {
        'magic': bytes(b'LVTL') + bytes(blob[4:]),
        'version': bytes(blob[:4]) + b'\x02' + bytes(blob[5:]),
        'filter': bytes(blob[:5]) + b'\x03' + bytes(blob[6:]),
        'length': bytes(blob[:-1]),
        'short': bytes(blob[:10]),
        'zero size': bytes(blob[:8]) + struct.pack('<I', 0) + bytes(blob[12:]),
        'ratio': bytes(blob[:16]) + struct.pack('<I', 7) + bytes(blob[20:]),          # 120 rows coded as 7
    }
    for name, b in bad.items():
        with pytest.raises(ValueError):
            resample.scaled_info(b)
        with pytest.raises(ValueError):
            resample.unpack_scaled(b)
    with pytest.raises(ValueError):
        resample.pack_scaled('nearest', (120, 180), (60, 90), b'')
    with pytest.raises(ValueError):
        resample.pack_scaled('bilinear', (120, 180), (6, 90), b'')


# ----------------------------------------------------------------------------------------------- argument checks
def test_scale_or_size_and_the_ratio_limit():
    assert resample.scaled_size(120, 180, scale=0.5) == (60, 90)
    assert resample.scaled_size(125, 75, scale=0.5) == (62, 38)                     # Python's round: ties to even
    assert resample.scaled_size(3, 5, scale=0.125) == (1, 1)                          # max(1, round(.)): 0.375 and 0.625 both reach 1
    assert resample.scaled_size(120, 180, size=(64, 100)) == (64, 100)
    assert resample.scaled_size(120, 180, scale=1.0) == (120, 180)
    for kw in ({}, dict(scale=0.5, size=(60, 90)), dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=0.1),
               dict(scale=9.0), dict(size=(14, 180)), dict(size=(120, 1441))):
        with pytest.raises(ValueError):
            resample.scaled_size(120, 180, **kw)
    resample.axis_table(64, 8)
    resample.axis_table(8, 64)
    for n_in, n_out in ((65, 8), (8, 65), (0, 4), (4, 0)):
        with pytest.raises(ValueError):
            resample.axis_table(n_in, n_out)
    with pytest.raises(ValueError):
        resample.resize_reference(np.zeros((3, 65, 20)), 8, 20)


def test_entry_points_check_their_arguments_without_a_gpu():
    """-22 before any HIP call: the addresses below are never dereferenced."""
    from lvae import _native
    L = _native.lib()
    assert {'lvae_resample_u8_to_f32', 'lvae_resample_f32_to_u8', 'lvae_resample_f32'} <= set(_native.SIGNATURES)
    P = 0x10000                                          # a non-null address
    ptrs = (ctypes.c_void_p * 2)(P, P)
    rows = (ctypes.c_long * 2)(3 * 200, 3 * 200)
    geom = dict(B=2, h_in=150, w_in=200, h_out=75, w_out=100)
    tabs = dict(ystart=P, ywgt=P, ytaps=12, yspan=42, xstart=P, xwgt=P, xtaps=12)

    def u8_in(src=ptrs, src_row=rows, dst=P, dst_img=3 * 128 * 128, H=128, W=128, **kw):
        a = {**geom, **tabs, **kw}
        return L.lvae_resample_u8_to_f32(src, src_row, a['B'], a['h_in'], a['w_in'], a['h_out'], a['w_out'], a['ystart'], a['ywgt'], a['ytaps'],
                                         a['yspan'], a['xstart'], a['xwgt'], a['xtaps'], dst, dst_img, H, W, None)

    def u8_out(src=P, strides=(3 * 150 * 200, 150 * 200, 200), dst=ptrs, dst_row=(ctypes.c_long * 2)(300, 300), **kw):
        a = {**geom, **tabs, **kw}
        return L.lvae_resample_f32_to_u8(src, *strides, a['B'], a['h_in'], a['w_in'], a['h_out'], a['w_out'], a['ystart'], a['ywgt'], a['ytaps'],
                                         a['yspan'], a['xstart'], a['xwgt'], a['xtaps'], dst, dst_row, None)

    def f32(src=P, strides=(3 * 150 * 200, 150 * 200, 200), dst=P, dst_img=3 * 128 * 128, H=128, W=128, clamp=0, **kw):
        a = {**geom, **tabs, **kw}
        return L.lvae_resample_f32(src, *strides, a['B'], a['h_in'], a['w_in'], a['h_out'], a['w_out'], a['ystart'], a['ywgt'], a['ytaps'],
                                   a['yspan'], a['xstart'], a['xwgt'], a['xtaps'], clamp, dst, dst_img, H, W, None)

    shared = [dict(B=0), dict(h_in=0), dict(w_out=-1), dict(ystart=None), dict(xwgt=None), dict(ytaps=0), dict(xtaps=65), dict(ytaps=-1),
              dict(yspan=0), dict(h_in=601), dict(w_in=12), dict(yspan=800, h_in=800, h_out=100)]
    for fn in (u8_in, u8_out, f32):
        for kw in shared:
            assert fn(**kw) == -22, (fn.__name__, kw)
        # a skipped axis takes no table, and only when the size stays
        assert fn(h_in=75, ytaps=0, ystart=P, ywgt=None) == -22
    for fn in (u8_in, f32):
        assert fn(dst=None) == -22 and fn(H=74) == -22 and fn(W=99) == -22 and fn(dst_img=3 * 128 * 128 - 1) == -22
    for fn in (u8_out, f32):
        assert fn(src=None) == -22
        assert fn(strides=(3 * 150 * 200, 150 * 200, 199)) == -22 and fn(strides=(3 * 150 * 200, 150 * 200 - 1, 200)) == -22
        assert fn(strides=(3 * 150 * 200 - 1, 150 * 200, 200)) == -22
    assert u8_in(src=None) == -22 and u8_in(src_row=None) == -22
    assert u8_in(src=(ctypes.c_void_p * 2)(P, None)) == -22 and u8_in(src_row=(ctypes.c_long * 2)(600, 599)) == -22
    assert u8_out(dst=None) == -22 and u8_out(dst_row=None) == -22
    assert u8_out(dst=(ctypes.c_void_p * 2)(None, P)) == -22 and u8_out(dst_row=(ctypes.c_long * 2)(300, 299)) == -22
