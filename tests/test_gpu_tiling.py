"""-m gpu: tiled coding.  The stitch kernel (csrc/tile_stitch.hip) against the fp64 restatement of its definition in
tests/test_tiling_host.py, then the models' compress_tiled / decompress_tiled / decompress_region against the per-tile calls they are
made of (every comparison == or torch.equal), the evaluation harness and scripts/lvae-codec.py."""
import ctypes
import functools
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
from lvae.utils import tiling
from lvae.utils.image import load_u8, save_u8, stitch_tiles
from test_tiling_host import blend_fp64

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
TH, TW = 64, 128

# (h, w, overlap, misaligned tile addresses, window, seed of the tiles).  The seeds: the u8 test leaves out values of 255 * out within 1e-3
# of a half-integer and caps their share at 0.2 %.  That band is 2e-3 of every unit interval, so for uniform values the expected share
# is 0.2 % itself, not below it; each seed is the first of 1, 2, ... whose share, computed on the CPU from the fp64 reference, is under
# 0.18 % (the test asserts the cap again, from the same reference).
GEOMETRIES = {
    'seams': (150, 200, 16, False, None, 13),
    'triple': (120, 200, 16, False, None, 2),
    'triple_both_axes': (120, 250, 16, False, None, 3),   # columns at 0, 112, 122: up to 9 covering tiles
    'no_overlap': (150, 200, 0, False, None, 4),
    'one_padded_tile': (50, 70, 16, False, None, 1),
    'misaligned_window': (150, 200, 16, True, (3, 5, 101, 77), 2),
}


# ----------------------------------------------------------------------------------------------- the kernel
@functools.lru_cache(maxsize=None)
def _geometry(name):
    """Per geometry, computed once: random fp32 tiles in [0, 1] on the host and on the device, the fp64 reference of the whole image
    and the cover count."""
    h, w, ov, misaligned, box, seed = GEOMETRIES[name]
    ys, xs = tiling.tile_grid(h, w, TH, TW, ov)
    g = torch.Generator().manual_seed(seed)
    host = [torch.rand(3, TH, TW, generator=g) for _ in range(len(ys) * len(xs))]
    dev = []
    for t in host:
        if misaligned:                                  # base 4 bytes past a 16-byte boundary, rows of 131 floats, planes 3 floats apart
            row, plane = TW + 3, TH * (TW + 3) + 3
            buf = torch.zeros(1 + 3 * plane, dtype=torch.float32, device=DEV)
            v = buf[1:].as_strided((3, TH, TW), (plane, row, 1))
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
        else:
            v = t.to(DEV)
        dev.append(v)
    ref, count = blend_fp64([t.numpy() for t in host], h, w, TH, TW, ov)
    return dict(h=h, w=w, ov=ov, box=box or (0, 0, h, w), host=host, dev=dev, ref=ref, count=count, ys=ys, xs=xs)


def _crop(a, box):
    y0, x0, hh, ww = box
    return a[..., y0:y0 + hh, x0:x0 + ww]


@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_stitch_f32_against_fp64(name):
    """|d| <= 1e-6: at most 9 products of weights and values in [0, 1], one sum and one division: about 11 * 2^-24 = 6.6e-7."""
    G = _geometry(name)
    out = stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=G['box'], out='f32')
    y0, x0, hh, ww = G['box']
    assert tuple(out.shape) == (1, 3, hh, ww) and out.dtype == torch.float32
    got = out[0].cpu().numpy()
    ref, count = _crop(G['ref'], G['box']), _crop(G['count'], G['box'])
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f'{name}: max|d| = {err:.3e}, covers up to {count.max()}')
    assert err <= 1e-6
    assert G['count'].max() == {'triple': 6, 'triple_both_axes': 9, 'no_overlap': 4, 'one_padded_tile': 1}.get(name, 4)
    # single-cover pixels: the tile's value, bit for bit
    single = count == 1
    assert single.any()
    assert np.array_equal(got[:, single], ref[:, single].astype(np.float32))
    assert np.array_equal(got[:, single].astype(np.float64), ref[:, single])
    # determinism: two calls, the same bits
    again = stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=G['box'], out='f32')
    assert torch.equal(out, again)


@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_stitch_u8_against_fp64(name):
    """rint of the fp64 value except where 255 * out lies within 1e-3 of a half-integer: those pixels (at most 0.2 %, see GEOMETRIES)
    are left out."""
    G = _geometry(name)
    out = stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=G['box'], out='u8')
    y0, x0, hh, ww = G['box']
    assert tuple(out.shape) == (hh, ww, 3) and out.dtype == torch.uint8
    v = 255.0 * np.clip(_crop(G['ref'], G['box']), 0.0, 1.0)
    near_tie = np.abs(v - np.floor(v) - 0.5) < 1e-3
    share = near_tie.mean()
    print(f'{name}: {share:.4%} of the values within 1e-3 of a tie')
    assert share <= 0.002                                # the seed stays under the cap (a property of the inputs, checked on the CPU)
    got = out.cpu().numpy().transpose(2, 0, 1)
    want = np.rint(v).astype(np.uint8)
    assert np.array_equal(got[~near_tie], want[~near_tie])
    assert torch.equal(out, stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=G['box'], out='u8'))


def _raw(G, tiles, box, dst_ptr, d_plane, d_row, u8):
    from lvae import _native
    lib = _native.lib()
    ys, xs = G['ys'], G['xs']
    t0 = next(t for t in tiles if t is not None)
    addr = (ctypes.c_void_p * len(tiles))(*[None if t is None else t.data_ptr() for t in tiles])
    oy, ox = (ctypes.c_int * len(ys))(*ys), (ctypes.c_int * len(xs))(*xs)
    nbytes = lib.lvae_tile_stitch_workspace_bytes(len(ys), len(xs))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.lvae_tile_stitch(addr, t0.stride(0), t0.stride(1), oy, ox, len(ys), len(xs), TH, TW, G['ov'], G['h'], G['w'], *box,
                              dst_ptr, d_plane, d_row, int(u8), ws.data_ptr(), nbytes, st)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('name', ['seams', 'misaligned_window'])
def test_stitch_writes_only_the_window(name):
    """A window in a larger destination (fp32: 2 rows / 3 columns in, u8: rows 3 * ww + 11 bytes apart from an odd address): the window
    is what the wrapper returns, every byte around it keeps the sentinel."""
    G = _geometry(name)
    box = (3, 5, 101, 77)
    y0, x0, hh, ww = box
    want32 = stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=box, out='f32')[0]
    want8 = stitch_tiles(G['dev'], G['h'], G['w'], TH, TW, G['ov'], box=box, out='u8')
    big = torch.full((3, hh + 4, ww + 7), -7.0, dtype=torch.float32, device=DEV)
    view = big[:, 2:2 + hh, 3:3 + ww]
    assert _raw(G, G['dev'], box, view.data_ptr(), big.stride(0), big.stride(1), False) == 0
    assert torch.equal(view, want32)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 2:2 + hh, 3:3 + ww] = False
    assert bool((big[mask] == -7.0).all())
    row = 3 * ww + 11
    buf = torch.full((1 + hh * row,), 7, dtype=torch.uint8, device=DEV)
    v8 = buf[1:].as_strided((hh, ww, 3), (row, 3, 1))
    assert _raw(G, G['dev'], box, v8.data_ptr(), 0, row, True) == 0
    assert torch.equal(v8, want8)
    m8 = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    m8[1:].as_strided((hh, ww, 3), (row, 3, 1)).fill_(False)
    assert bool((buf[m8] == 7).all())


def test_stitch_null_tiles_and_argument_errors():
    G = _geometry('seams')                               # rows at 0, 48, 86; columns at 0, 72
    box = (2, 3, 40, 60)                                 # inside tile 0 alone
    only0 = [G['dev'][0]] + [None] * 5
    out = torch.empty(3, 40, 60, dtype=torch.float32, device=DEV)
    assert _raw(G, only0, box, out.data_ptr(), 40 * 60, 60, False) == 0
    assert torch.equal(out, G['dev'][0][:, 2:42, 3:63])
    assert torch.equal(stitch_tiles(only0, G['h'], G['w'], TH, TW, G['ov'], box=box, out='f32')[0], out)
    across = (2, 3, 40, 80)                              # reaches column 72: tile 1 is needed and null
    big = torch.empty(3, 40, 80, dtype=torch.float32, device=DEV)
    assert _raw(G, only0, across, big.data_ptr(), 40 * 80, 80, False) == -22
    full = G['dev']
    assert _raw(G, full, (100, 3, 51, 60), big.data_ptr(), 51 * 60, 60, False) == -22        # a window below the image
    assert _raw(G, full, (0, 150, 10, 51), big.data_ptr(), 10 * 51, 51, False) == -22         # ... right of it
    assert _raw(G, full, (0, 0, 0, 10), big.data_ptr(), 10, 10, False) == -22                 # ... empty
    assert _raw(G, full, across, big.data_ptr(), 40 * 80, 79, False) == -22                   # destination rows too short
    narrow = [t[:, :, :100] for t in full]               # tiles whose strides are fine but whose claimed row stride is not
    from lvae import _native
    lib = _native.lib()
    addr = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in narrow])
    oy, ox = (ctypes.c_int * 3)(*G['ys']), (ctypes.c_int * 2)(*G['xs'])
    ws = torch.empty(16, dtype=torch.int64, device=DEV)
    args = lambda plane, row: lib.lvae_tile_stitch(addr, plane, row, oy, ox, 3, 2, TH, TW, 16, 150, 200, 2, 3, 40, 80, big.data_ptr(), 3200, 80,
                                                   0, ws.data_ptr(), 128, None)
    assert args(TH * TW, TW - 1) == -22 and args(TH * TW - 1, TW) == -22                      # strides that do not hold (th, tw)


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _model(name):
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


H, W, OV = 120, 200, 16                                  # rows at 0, 48, 56 (rows 56 .. 63 are covered three times), columns at 0, 72


@functools.lru_cache(maxsize=None)
def _coded(name):
    """Per model, computed once and left unchanged: the image, its container (max_batch 8) and the stitched reconstruction."""
    m = _model(name)
    img = torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 70))
    blob = m.compress_tiled(img, tile=(TH, TW), overlap=OV, max_batch=8)
    return dict(model=m, img=img, blob=blob, parts=tiling.unpack_tiled(blob), full=m.decompress_tiled(blob, max_batch=8))


MAIN = ['qarv_base', 'qres34m']


@pytest.mark.parametrize('name', MAIN)
def test_tiles_are_compress_images_of_the_crops(name):
    C = _coded(name)
    m, p = C['model'], C['parts']
    assert (p['ys'], p['xs']) == ([0, 48, 56], [0, 72]) and (p['h'], p['w'], p['th'], p['tw'], p['overlap']) == (H, W, TH, TW, OV)
    k = 0
    for y in p['ys']:
        for x in p['xs']:
            assert p['tiles'][k] == m.compress_images([C['img'][y:y + TH, x:x + TW]])[0], k
            k += 1
    info = m.tiled_info(C['blob'])
    assert info['lengths'] == [len(t) for t in p['tiles']] and (info['rows'], info['cols'], info['tile']) == (3, 2, (TH, TW))


@pytest.mark.parametrize('name', MAIN)
def test_container_and_pixels_do_not_depend_on_max_batch(name):
    C = _coded(name)
    m = C['model']
    for mb in (1, 3):
        assert m.compress_tiled(C['img'], tile=(TH, TW), overlap=OV, max_batch=mb) == C['blob'], mb
    assert torch.equal(m.decompress_tiled(C['blob'], max_batch=1), C['full'])
    assert tuple(C['full'].shape) == (H, W, 3) and C['full'].dtype == torch.uint8 and C['full'].is_cuda
    f8, f1 = m.decompress_tiled(C['blob'], out='f32', max_batch=8), m.decompress_tiled(C['blob'], out='f32', max_batch=1)
    assert tuple(f8.shape) == (1, 3, H, W) and torch.equal(f8, f1)
    assert torch.equal(torch.round(f8[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0), C['full'])


BOXES = {'one_tile': ((2, 3, 30, 40), 1), 'seam': ((10, 60, 20, 40), 2), 'triple_band': ((50, 10, 12, 30), 3), 'whole': ((0, 0, H, W), 6)}


@pytest.mark.parametrize('name', MAIN)
@pytest.mark.parametrize('box_name', list(BOXES))
def test_region_equals_the_crop_and_decodes_only_its_tiles(name, box_name, monkeypatch):
    C = _coded(name)
    m = C['model']
    box, n_tiles = BOXES[box_name]
    y0, x0, hh, ww = box
    assert len(tiling.tiles_in_box(C['parts']['ys'], C['parts']['xs'], TH, TW, box)) == n_tiles
    handed = []
    inner = m.decompress_batch
    monkeypatch.setattr(m, 'decompress_batch', lambda blobs: (handed.append(len(blobs)), inner(blobs))[1])
    got = m.decompress_region(C['blob'], box)
    assert sum(handed) == n_tiles
    assert torch.equal(got, C['full'][y0:y0 + hh, x0:x0 + ww])
    assert torch.equal(m.decompress_region(C['blob'], box, out='f32', max_batch=2)[0],
                       m.decompress_tiled(C['blob'], out='f32')[0][:, y0:y0 + hh, x0:x0 + ww])


@pytest.mark.parametrize('name', MAIN)
def test_interior_of_a_tile_is_its_own_decode(name):
    C = _coded(name)
    m, p = C['model'], C['parts']
    alone = m.decompress_images([p['tiles'][0], p['tiles'][5]])
    assert torch.equal(C['full'][:48, :72], alone[0][:48, :72])                     # tile 0 is alone above row 48, left of column 72
    assert torch.equal(C['full'][112:, 128:], alone[1][112 - 56:, 128 - 72:])       # tile 5 below row 111, right of column 127


@pytest.mark.parametrize('name', MAIN)
def test_image_smaller_than_a_tile(name):
    m = _model(name)
    img = torch.from_numpy(seeded_init.synthetic_image_u8(50, 70, 71))
    blob = m.compress_tiled(img, tile=(128, 256), overlap=OV)
    p = tiling.unpack_tiled(blob)
    assert (p['rows'], p['cols']) == (1, 1) and p['tiles'][0] == m.compress_images([img])[0]
    want = m.decompress_images([m.compress_images([img])[0]])[0]
    assert torch.equal(m.decompress_tiled(blob), want)
    assert torch.equal(m.decompress_region(blob, (7, 9, 30, 41)), want[7:37, 9:50])


def test_lambda_map_gives_per_tile_lambdas():
    C = _coded('qarv_base')
    m = C['model']
    lmbs = [[16, 64], [256, 1024], [2048, 32]]
    blob = m.compress_tiled(C['img'], tile=(TH, TW), overlap=OV, lmb=np.array(lmbs), max_batch=4)
    p = tiling.unpack_tiled(blob)
    for r, y in enumerate(p['ys']):
        for c, x in enumerate(p['xs']):
            assert p['tiles'][r * 2 + c] == m.compress_images([C['img'][y:y + TH, x:x + TW]], lmb=lmbs[r][c])[0], (r, c)
    assert m.tiled_info(blob)['lmb'] == [[float(v) for v in row] for row in lmbs]
    assert m.tiled_info(C['blob'])['lmb'] == [[float(m.default_lmb)] * 2] * 3
    assert m.compress_tiled(C['img'], tile=(TH, TW), overlap=OV, lmb=64) == m.compress_tiled(C['img'], tile=(TH, TW), overlap=OV,
                                                                                               lmb=np.full((3, 2), 64.0))
    assert tuple(m.decompress_tiled(blob).shape) == (H, W, 3)
    with pytest.raises(ValueError):
        m.compress_tiled(C['img'], tile=(TH, TW), overlap=OV, lmb=np.ones((2, 3)))
    with pytest.raises(ValueError):
        m.compress_tiled(C['img'], tile=(TH, 100))                                   # not a multiple of max_stride
    with pytest.raises(ValueError):
        m.decompress_region(C['blob'], (100, 0, 21, 10))


@pytest.mark.parametrize('name', ['qres34m_lossless', 'qres17m'])
def test_round_trip_without_overlap(name):
    m = _model(name)
    img = torch.from_numpy(seeded_init.synthetic_image_u8(100, 150, 72))
    blob = m.compress_tiled(img, tile=(TH, TW), overlap=0, max_batch=2)
    p = tiling.unpack_tiled(blob)
    assert (p['ys'], p['xs']) == ([0, 36], [0, 22])
    rec = m.decompress_tiled(blob)
    assert tuple(rec.shape) == (100, 150, 3) and rec.dtype == torch.uint8
    assert torch.equal(m.decompress_region(blob, (30, 20, 40, 50)), rec[30:70, 20:70])
    assert torch.equal(rec[:36, :22], m.decompress_images([p['tiles'][0]])[0][:36, :22])
    assert m.tiled_info(blob)['lmb'] is None
    if name == 'qres34m_lossless':
        assert torch.equal(rec.cpu(), img)
    with pytest.raises(ValueError):
        m.compress_tiled(img, tile=(TH, TW), lmb=64)


# ----------------------------------------------------------------------------------------------- callers
def test_evaluation_in_tiles(tmp_path):
    from lvae.evaluation import imcoding_evaluate
    m = _model('qarv_base')
    folder = tmp_path / 'set'
    folder.mkdir()
    img = torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 70))
    save_u8(img, folder / 'im0.png')
    got = imcoding_evaluate(m, str(folder), tile=(TH, TW), overlap=OV)
    assert set(got) == {'bpp', 'mse', 'psnr'} and all(math.isfinite(v) for v in got.values())
    assert got['bpp'] == 8 * len(_coded('qarv_base')['blob']) / (H * W)
    real = img.permute(2, 0, 1).float().div(255)
    fake = m.decompress_tiled(_coded('qarv_base')['blob'], out='f32')[0].cpu()
    assert got['mse'] == pytest.approx(float((real - fake).double().square().mean()), rel=1e-6)


def test_codec_script_in_tiles(tmp_path):
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, rec, crops = tmp_path / 'src', tmp_path / 'bits', tmp_path / 'rec', tmp_path / 'crops'
    common = ['-m', 'qarv_base', '--synthetic', '1', '--batch', '4']
    for cmd in (['encode', str(src), str(bits), '--lmb', '256', '--tile', '64', '128', '--overlap', '16'], ['decode', str(bits), str(rec)],
                ['region', str(bits), str(crops), '--box', '40', '50', '60', '100']):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(bits.glob('*.bits'))
    assert [f.stem for f in files] == ['im00']
    m = _model('qarv_base')
    for f in files:
        blob = f.read_bytes()
        assert blob[:4] == b'LVTL' and blob == m.compress_tiled(src / (f.stem + '.png'), tile=(64, 128), overlap=16, lmb=256)
        full = m.decompress_tiled(blob).cpu()
        assert torch.equal(load_u8(rec / (f.stem + '.png')), full)
        assert torch.equal(load_u8(crops / (f.stem + '.png')), full[40:100, 50:150])
        assert struct.unpack('f', tiling.unpack_tiled(blob)['tiles'][0][4:8])[0] == 256.0
