"""-m gpu: tiled coding of YUV frames.  The fused kernel (csrc/tile_stitch_yuv.hip) against the composition it replaces -- stitch_tiles to
fp32, then from_rgb01 / from_rgb01_any -- and, where the stitch is a copy, against the CPU expression that defines the conversion; then
the models' compress_yuv_tiled / decompress_yuv_tiled / decompress_yuv_region, tiled sequences, the evaluation harness and
scripts/lvae-codec.py against the per-tile calls they are made of.  Every comparison is == or torch.equal."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init
from lvae.utils import tiling, yuv, yuvseq
from lvae.utils.image import stitch_tiles
from lvae.utils.yuv import Yuv420Frame, YuvFrame, YuvSpFrame, from_rgb01, from_rgb01_any, rgb_to_yuv_expr2, stitch_tiles_yuv

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
TH, TW = 32, 48

# (h, w, overlap): the smallest geometries with each behaviour
GEOMETRIES = {
    'exact_grid': (64, 96, 0),                           # 2 x 2, no pixel has two covers: the stitch is a copy
    'seams': (70, 118, 8),                               # 3 x 3, the last tiles moved in: rows at 0, 24, 38, columns at 0, 40, 70
    'triple_both_axes': (58, 90, 8),                     # rows at 0, 24, 26, columns at 0, 40, 42: up to 9 covers; a 2-wide last quad
    'one_padded_tile': (20, 30, 8),                      # the tile is larger than the image
}
FORMATS = {
    'i420': dict(layout='i420', matrix='bt601'),
    'nv12': dict(layout='nv12', matrix='bt601'),
    'yuv420p10_left': dict(depth=10, siting='left', matrix='bt2020'),
    'p010': dict(depth=10, layout='semiplanar'),
    'yuv422p12_left': dict(depth=12, subsampling='422', siting='left', range='full'),
    'p210': dict(depth=10, subsampling='422', layout='semiplanar'),
    'yuv444p8': dict(subsampling='444', range='full'),
}


def _params(fmt):
    return dict(dict(depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar'), **FORMATS[fmt])


def _misaligned(t):
    """The tile at an address 4 bytes past a 16-byte boundary, rows of TW + 3 floats, planes 3 floats apart (tests/test_gpu_tiling.py)."""
    row, plane = TW + 3, TH * (TW + 3) + 3
    buf = torch.zeros(1 + 3 * plane, dtype=torch.float32, device=DEV)
    v = buf[1:].as_strided((3, TH, TW), (plane, row, 1))
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """Per geometry, once: random fp32 tiles in [-0.1, 1.1] (the clamp works on both sides) with a few NaNs, on the host and the device."""
    h, w, ov = GEOMETRIES[name]
    ys, xs = tiling.tile_grid(h, w, TH, TW, ov)
    g = torch.Generator().manual_seed(1 + list(GEOMETRIES).index(name))
    host = []
    for _ in range(len(ys) * len(xs)):
        t = torch.rand(3, TH, TW, generator=g) * 1.2 - 0.1
        t.view(-1)[torch.randint(0, t.numel(), (6,), generator=g)] = float('nan')
        host.append(t)
    return dict(h=h, w=w, ov=ov, ys=ys, xs=xs, host=host, dev=[t.to(DEV) for t in host])


def _grid(G):
    return G['h'], G['w'], TH, TW, G['ov']


def _crop(fr, box, sub):
    """The planes of the window `box` of a frame, as lists of tensors (whatever the frame's kind)."""
    y0, x0, hh, ww = box
    sx, sy = yuv.SHIFTS[sub]
    rows = slice(y0 >> sy, (y0 + hh) >> sy)
    out = [fr.y[y0:y0 + hh, x0:x0 + ww]]
    if isinstance(fr, YuvSpFrame):
        return out + [fr.uv[rows, x0:x0 + ww]]
    if isinstance(fr, Yuv420Frame) and fr.fmt == 'nv12':
        return out + [fr.uv[rows, x0 >> 1:(x0 + ww) >> 1]]
    return out + [fr.u[rows, x0 >> sx:(x0 + ww) >> sx], fr.v[rows, x0 >> sx:(x0 + ww) >> sx]]


def _whole(fr, sub):
    return _crop(fr, (0, 0, fr.h, fr.w), sub)


def _same(a, b):
    return len(a) == len(b) and all(p.dtype == q.dtype and p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


def _convert(x, p):
    """The second half of the composition: an fp32 image -> the frame, by the entry the layout names."""
    if p['layout'] in ('i420', 'nv12'):
        return from_rgb01(x, fmt=p['layout'], matrix=p['matrix'], range=p['range'])[0]
    return from_rgb01_any(x, **p)[0]


def _composition(tiles, G, box, p):
    """lvae_tile_stitch to an fp32 image, then the matching lvae_image_f32_to_yuv* entry, as the planes of the window.  The conversion runs
    on the window itself -- except with left-sited chroma and x0 > 0: a window is defined as the crop of the whole frame, whose first
    chroma column reads the image's column x0 - 1, so the fp32 window starts one chroma pixel (two columns) earlier and that pixel is
    cropped away afterwards."""
    y0, x0, hh, ww = box
    pad = 2 if p['siting'] == 'left' and p['subsampling'] != '444' and x0 > 0 else 0
    f32 = stitch_tiles(tiles, *_grid(G), box=(y0, x0 - pad, hh, ww + pad), out='f32')
    return _crop(_convert(f32, p), (0, pad, hh, ww), p['subsampling'])


WINDOW = (2, 6, 40, 50)                                  # even on both axes
ODD_WINDOW = (3, 5, 41, 37)                              # 4:4:4 only


# ----------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('fmt', list(FORMATS))
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_fused_equals_the_composition(name, fmt):
    G, p = _geometry(name), _params(fmt)
    full_box = (0, 0, G['h'], G['w'])
    full = stitch_tiles_yuv(G['dev'], *_grid(G), **p)
    kind = Yuv420Frame if p['layout'] in ('i420', 'nv12') else YuvSpFrame if p['layout'] == 'semiplanar' else YuvFrame
    assert type(full) is kind and full.size == (G['h'], G['w']) and full.y.is_cuda
    assert _same(_whole(full, p['subsampling']), _composition(G['dev'], G, full_box, p))
    assert _same(_whole(full, p['subsampling']), _whole(stitch_tiles_yuv(G['dev'], *_grid(G), **p), p['subsampling']))     # two calls, the same bits
    if name == 'one_padded_tile':
        return
    boxes = [WINDOW] + ([ODD_WINDOW] if p['subsampling'] == '444' else [])
    if name == 'exact_grid':
        boxes += [(0, 48, 64, 48), (2, 48, 40, 30)]      # column x0 - 1 = 47 lies in tile column 0, the window in tile column 1
    for box in boxes:
        win = stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **p)
        assert win.size == box[2:]
        assert _same(_whole(win, p['subsampling']), _composition(G['dev'], G, box, p)), box
        assert _same(_whole(win, p['subsampling']), _crop(full, box, p['subsampling'])), box


@pytest.mark.parametrize('fmt', list(FORMATS))
def test_exact_grid_equals_the_cpu_expression(fmt):
    """No pixel of the exact grid has two covers, so the stitched image is the tiles side by side: the kernel's output is
    rgb_to_yuv_expr2 of that image, evaluated on the CPU -- a reference that rests on no device code."""
    G, p = _geometry('exact_grid'), _params(fmt)
    img = torch.empty(3, G['h'], G['w'])
    for k, t in enumerate(G['host']):
        oy, ox = G['ys'][k // 2], G['xs'][k % 2]
        img[:, oy:oy + TH, ox:ox + TW] = t
    want = YuvFrame(*rgb_to_yuv_expr2(img, p['depth'], p['subsampling'], p['siting'], p['matrix'], p['range']), p['depth'], p['subsampling'])
    if p['layout'] == 'semiplanar':
        want = want.to_semiplanar()
    elif p['layout'] in ('i420', 'nv12'):
        want = Yuv420Frame('i420', want.y, want.u, want.v).as_format(p['layout'])
    got = stitch_tiles_yuv(G['dev'], *_grid(G), **p)
    assert _same([t.cpu() for t in _whole(got, p['subsampling'])], _whole(want, p['subsampling']))
    box = (2, 48, 40, 30)
    win = stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **p)
    assert _same([t.cpu() for t in _whole(win, p['subsampling'])], _crop(want, box, p['subsampling']))


@pytest.mark.parametrize('name', ['seams', 'triple_both_axes'])
def test_semiplanar_outputs_are_the_planar_ones_interleaved(name):
    G = _geometry(name)
    for fmt in ('p010', 'p210'):
        p = _params(fmt)
        for box in (None, WINDOW):
            planar = stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **dict(p, layout='planar'))
            assert _same(_whole(stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **p), p['subsampling']), _whole(planar.to_semiplanar(), p['subsampling']))
    for box in (None, WINDOW):
        i420 = stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **_params('i420'))
        assert _same(_whole(stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **_params('nv12')), '420'), _whole(i420.as_format('nv12'), '420'))


@pytest.mark.parametrize('fmt', ['yuv420p10_left', 'nv12', 'yuv444p8'])
def test_misaligned_tile_addresses_and_strides(fmt):
    G, p = _geometry('seams'), _params(fmt)
    tiles = [_misaligned(t) for t in G['host']]
    for box in (None, WINDOW):
        got = _whole(stitch_tiles_yuv(tiles, *_grid(G), box=box, **p), p['subsampling'])
        assert _same(got, _whole(stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **p), p['subsampling']))
        assert _same(got, _composition(tiles, G, box or (0, 0, G['h'], G['w']), p))


@pytest.mark.parametrize('fmt', ['yuv420p10_left', 'p010', 'i420', 'nv12', 'yuv444p8'])
def test_only_the_windows_planes_are_written(fmt):
    """Destination planes that are views inside larger tensors, at odd offsets: the views hold the window, every sample around them keeps
    the sentinel."""
    G, p = _geometry('seams'), _params(fmt)
    box = ODD_WINDOW if p['subsampling'] == '444' else WINDOW
    hh, ww = box[2:]
    sx, sy = yuv.SHIFTS[p['subsampling']]
    dtype, sentinel = (torch.uint8, 0x5a) if p['depth'] == 8 else (torch.int16, 0x5a5a)
    bigs, views = [], []

    def plane(rows, cols, trailing=()):
        big = torch.full((rows + 3, cols + 8) + trailing, sentinel, dtype=dtype, device=DEV)
        bigs.append(big)
        views.append(big[1:1 + rows, 3:3 + cols])
        return views[-1]
    if p['layout'] == 'nv12':
        out = Yuv420Frame('nv12', plane(hh, ww), uv=plane(hh // 2, ww // 2, (2,)))
    elif p['layout'] == 'i420':
        out = Yuv420Frame('i420', plane(hh, ww), plane(hh // 2, ww // 2), plane(hh // 2, ww // 2))
    elif p['layout'] == 'semiplanar':
        out = YuvSpFrame(plane(hh, ww), plane(hh >> sy, ww), p['depth'], p['subsampling'])
    else:
        out = YuvFrame(plane(hh, ww), plane(hh >> sy, ww >> sx), plane(hh >> sy, ww >> sx), p['depth'], p['subsampling'])
    assert stitch_tiles_yuv(G['dev'], *_grid(G), box=box, out=out, **p) is out
    assert _same(_whole(out, p['subsampling']), _whole(stitch_tiles_yuv(G['dev'], *_grid(G), box=box, **p), p['subsampling']))
    for big, view in zip(bigs, views):
        outside = torch.ones_like(big, dtype=torch.bool)
        outside[1:1 + view.shape[0], 3:3 + view.shape[1]] = False
        assert bool((big[outside] == sentinel).all())


def test_null_tiles():
    """A tile the window needs -- counting the column before it where the chroma is left-sited -- must be there; any other may be None."""
    G = _geometry('exact_grid')
    t = G['dev']
    right = [None, t[1], None, t[3]]                     # tile column 1 alone: columns 48 .. 95
    box = (0, 48, 64, 48)
    centre, left = _params('p010'), _params('yuv420p10_left')
    got = stitch_tiles_yuv(right, *_grid(G), box=box, **centre)
    assert _same(_whole(got, '420'), _crop(stitch_tiles_yuv(t, *_grid(G), **centre), box, '420'))
    with pytest.raises(ValueError, match='column before'):
        stitch_tiles_yuv(right, *_grid(G), box=box, **left)
    with pytest.raises(ValueError, match='not decoded'):
        stitch_tiles_yuv(right, *_grid(G), box=(0, 46, 64, 50), **centre)
    top_right = [None, t[1], None, None]                 # left siting, x0 = 50: column 49 is tile column 1's own
    got = stitch_tiles_yuv(top_right, *_grid(G), box=(0, 50, 32, 40), **left)
    assert _same(_whole(got, '420'), _crop(stitch_tiles_yuv(t, *_grid(G), **left), (0, 50, 32, 40), '420'))
    # the native entry agrees: -22 for the same two calls
    import ctypes
    from lvae import _native
    lib = _native.lib()
    addr = (ctypes.c_void_p * 4)(*[None if x is None else x.data_ptr() for x in right])
    oy, ox = (ctypes.c_int * 2)(*G['ys']), (ctypes.c_int * 2)(*G['xs'])
    ws = torch.empty(8, dtype=torch.int64, device=DEV)
    fr = yuv.new_frame(64, 50, DEV, 10, '420', 'planar')

    def raw(x0, ww, siting):
        return lib.lvae_tile_stitch_yuv(addr, TH * TW, TW, oy, ox, 2, 2, TH, TW, 0, 64, 96, 0, x0, 64, ww, 10, 0, siting, 1, 0, 0, fr.y.data_ptr(),
                                        fr.u.data_ptr(), fr.v.data_ptr(), 50, 25, 25, ws.data_ptr(), 64, None)
    assert raw(48, 48, 1) == -22 and raw(46, 50, 0) == -22
    assert raw(48, 48, 0) == 0
    torch.cuda.synchronize()


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


def _rgb(h, w, seed):
    return torch.from_numpy(seeded_init.synthetic_image_u8(h, w, seed)).permute(2, 0, 1).float().div(255)


H, W, TILE, OV = 128, 192, (64, 64), 16                  # rows at 0, 48, 64, columns at 0, 48, 96, 128
KW = dict(depth=10, subsampling='420', siting='left')    # what the decoder has to be told
MAIN = ['qarv_base', 'qres34m']


@functools.lru_cache(maxsize=None)
def _frame(seed=90, h=H, w=W):
    return from_rgb01_any([_rgb(h, w, seed)], **KW)[0]   # a CPU frame: 10-bit 4:2:0, left-sited


@functools.lru_cache(maxsize=None)
def _coded(name):
    """Per model, once and left unchanged: the frame's container (max_batch 8), its parts and the decoded frame."""
    m = _model(name)
    blob = m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, siting='left', max_batch=8)
    return dict(model=m, blob=blob, parts=tiling.unpack_tiled(blob), full=m.decompress_yuv_tiled(blob, **KW))


def _tile_frame(fr, y, x, th, tw):
    """The crop of a planar 4:2:0 frame as a frame of its own, planes copied."""
    c = lambda p, y, x, th, tw: p[y:y + th, x:x + tw].clone()
    return YuvFrame(c(fr.y, y, x, th, tw), c(fr.u, y // 2, x // 2, th // 2, tw // 2), c(fr.v, y // 2, x // 2, th // 2, tw // 2), fr.depth, fr.subsampling)


@pytest.mark.parametrize('name', MAIN)
def test_tile_blobs_are_compress_yuv_of_the_crops(name):
    C = _coded(name)
    m, p = C['model'], C['parts']
    assert (p['ys'], p['xs']) == ([0, 48, 64], [0, 48, 96, 128]) and (p['h'], p['w'], p['th'], p['tw'], p['overlap']) == (H, W, 64, 64, OV)
    k = 0
    for y in p['ys']:
        for x in p['xs']:
            assert p['tiles'][k] == m.compress_yuv([_tile_frame(_frame(), y, x, 64, 64)], siting='left')[0], k
            k += 1
    info = m.tiled_info(C['blob'])
    assert info['lengths'] == [len(t) for t in p['tiles']] and (info['rows'], info['cols'], info['tile'], info['overlap']) == (3, 4, (64, 64), OV)


def test_tiles_are_views_of_the_planes():
    """The frame classes and the native entries' argument builder take crops of planes as they lie: no plane is copied."""
    fr = _frame().to(DEV)
    views = [YuvFrame(fr.y[48:112, 96:160], fr.u[24:56, 48:80], fr.v[24:56, 48:80], 10, '420'),
             YuvFrame(fr.y[64:128, 128:192], fr.u[32:64, 64:96], fr.v[32:64, 64:96], 10, '420')]
    _, rows, _, kept = yuv._plane_args(views, ('y', 'u', 'v'))
    for q, name in zip(kept, 'yuv'):
        assert [t.data_ptr() for t in q] == [getattr(v, name).data_ptr() for v in views]
    assert list(rows[0]) == [W, W] and list(rows[1]) == [W // 2, W // 2]
    sp = fr.to_semiplanar()
    spv = [YuvSpFrame(sp.y[48:112, 96:160], sp.uv[24:56, 96:160], 10, '420')]
    _, rows, _, kept = yuv._plane_args(spv, ('y', 'uv'))
    assert kept[1][0].data_ptr() == sp.uv[24:56, 96:160].data_ptr() and list(rows[1]) == [W]


@pytest.mark.parametrize('name', MAIN)
def test_container_does_not_depend_on_max_batch(name):
    C = _coded(name)
    m = C['model']
    for mb in (1, 3):
        assert m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, siting='left', max_batch=mb) == C['blob'], mb
    assert m.compress_yuv_tiled(_frame().to(DEV), tile=TILE, overlap=OV, siting='left') == C['blob']
    assert _same(_whole(m.decompress_yuv_tiled(C['blob'], max_batch=1, **KW), '420'), _whole(C['full'], '420'))


@pytest.mark.parametrize('name', MAIN)
def test_decode_equals_the_conversion_of_the_stitched_fp32_image(name):
    C = _coded(name)
    m = C['model']
    assert type(C['full']) is YuvFrame and C['full'].size == (H, W) and C['full'].y.is_cuda and C['full'].depth == 10
    want = from_rgb01_any(m.decompress_tiled(C['blob'], out='f32'), **KW)[0]
    assert _same(_whole(C['full'], '420'), _whole(want, '420'))
    other = dict(depth=8, subsampling='444', matrix='bt601', range='full')              # the decoder may ask for any format
    assert _same(_whole(m.decompress_yuv_tiled(C['blob'], **other), '444'), _whole(from_rgb01_any(m.decompress_tiled(C['blob'], out='f32'), **other)[0], '444'))


# box -> tiles decoded with left-sited chroma.  'left_neighbour': columns 64 .. 93 lie in tile column 1 alone, column 63 also in column 0
BOXES = {'one_tile': ((2, 4, 30, 40), 1), 'left_neighbour': ((0, 64, 40, 30), 2), 'seam': ((10, 40, 20, 40), 2), 'whole': ((0, 0, H, W), 12)}


@pytest.mark.parametrize('name', MAIN)
@pytest.mark.parametrize('box_name', list(BOXES))
def test_region_equals_the_crop_and_decodes_only_its_tiles(name, box_name, monkeypatch):
    C = _coded(name)
    m = C['model']
    box, n_tiles = BOXES[box_name]
    handed = []
    inner = m.decompress_batch
    monkeypatch.setattr(m, 'decompress_batch', lambda blobs: (handed.append(len(blobs)), inner(blobs))[1])
    got = m.decompress_yuv_region(C['blob'], box, max_batch=5, **KW)
    assert sum(handed) == n_tiles
    assert got.size == box[2:] and _same(_whole(got, '420'), _crop(C['full'], box, '420'))
    if box_name == 'left_neighbour':                     # centre-sited chroma reads nothing outside the box: one tile
        del handed[:]
        m.decompress_yuv_region(C['blob'], box, depth=10)
        assert sum(handed) == 1
    with pytest.raises(ValueError, match='chroma grid'):
        m.decompress_yuv_region(C['blob'], (1, 4, 30, 40), **KW)
    with pytest.raises(ValueError, match='not inside'):
        m.decompress_yuv_region(C['blob'], (100, 0, 30, 40), **KW)


@pytest.mark.parametrize('name', MAIN)
def test_frame_smaller_than_a_tile(name):
    m = _model(name)
    fr = _frame(91, 52, 70)
    blob = m.compress_yuv_tiled(fr, tile=(128, 256), overlap=OV, siting='left')
    p = tiling.unpack_tiled(blob)
    one = m.compress_yuv([fr], siting='left')[0]
    assert (p['rows'], p['cols']) == (1, 1) and p['tiles'][0] == one
    want = m.decompress_yuv([one], **KW)[0]
    assert _same(_whole(m.decompress_yuv_tiled(blob, **KW), '420'), _whole(want, '420'))
    assert _same(_whole(m.decompress_yuv_region(blob, (6, 8, 30, 40), **KW), '420'), _crop(want, (6, 8, 30, 40), '420'))


def test_lambda_map_gives_per_tile_lambdas():
    C = _coded('qarv_base')
    m = C['model']
    lmbs = [[16, 64, 256, 1024], [2048, 32, 128, 512], [24, 48, 96, 192]]
    blob = m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, siting='left', lmb=np.array(lmbs), max_batch=5)
    p = tiling.unpack_tiled(blob)
    for r, y in enumerate(p['ys']):
        for c, x in enumerate(p['xs']):
            assert p['tiles'][r * 4 + c] == m.compress_yuv([_tile_frame(_frame(), y, x, 64, 64)], siting='left', lmb=lmbs[r][c])[0], (r, c)
    assert m.tiled_info(blob)['lmb'] == [[float(v) for v in row] for row in lmbs]
    assert m.tiled_info(C['blob'])['lmb'] == [[float(m.default_lmb)] * 4] * 3
    assert m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, siting='left', lmb=64) == \
        m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, siting='left', lmb=np.full((3, 4), 64.0))
    assert m.decompress_yuv_tiled(blob, **KW).size == (H, W)
    with pytest.raises(ValueError):
        m.compress_yuv_tiled(_frame(), tile=TILE, overlap=OV, lmb=np.ones((4, 3)))
    with pytest.raises(ValueError):
        _model('qres34m').compress_yuv_tiled(_frame(), tile=TILE, lmb=64)


@pytest.mark.parametrize('name', MAIN)
def test_p010_frames_give_the_planar_frames_bytes_and_codes(name):
    C = _coded(name)
    m = C['model']
    sp = _frame().to_semiplanar()
    assert m.compress_yuv_tiled(sp, tile=TILE, overlap=OV, siting='left', max_batch=3) == C['blob']
    got = m.decompress_yuv_tiled(C['blob'], layout='semiplanar', **KW)
    assert type(got) is YuvSpFrame and _same(_whole(got, '420'), _whole(C['full'].to_semiplanar(), '420'))
    box = (16, 64, 48, 64)
    assert _same(_whole(m.decompress_yuv_region(C['blob'], box, layout='semiplanar', **KW), '420'), _crop(got, box, '420'))


def test_eight_bit_frames_in_both_layouts():
    m = _model('qarv_base')
    i420 = from_rgb01([_rgb(H, W, 92)])[0]
    blob = m.compress_yuv_tiled(i420, tile=TILE, overlap=OV)
    assert m.compress_yuv_tiled(i420.as_format('nv12'), tile=TILE, overlap=OV) == blob
    p = tiling.unpack_tiled(blob)
    crop = Yuv420Frame('i420', i420.y[48:112, 96:160].clone(), i420.u[24:56, 48:80].clone(), i420.v[24:56, 48:80].clone())
    assert p['tiles'][1 * 4 + 2] == m.compress_yuv420([crop])[0]
    want = from_rgb01(m.decompress_tiled(blob, out='f32'))[0]
    for fmt in ('i420', 'nv12'):
        got = m.decompress_yuv_tiled(blob, layout=fmt)
        assert type(got) is Yuv420Frame and got.fmt == fmt and _same(_whole(got, '420'), _whole(want.as_format(fmt), '420'))


# ----------------------------------------------------------------------------------------------- sequences
SEQ = dict(siting='left', matrix='bt2020', range='limited', chroma='bilinear')


def test_sequence_of_tiled_frames():
    m = _model('qarv_base')
    frames = from_rgb01_any([_rgb(H, W, 300 + i) for i in range(3)], depth=10, siting='left', matrix='bt2020')
    blob = m.compress_yuv_sequence(frames, tile=TILE, overlap=OV, max_batch=5, **SEQ)
    info, entries = yuvseq.unpack_sequence(blob)
    enc = {k: v for k, v in SEQ.items()}
    assert entries == [m.compress_yuv_tiled(f, tile=TILE, overlap=OV, **enc) for f in frames]
    assert all(tiling.is_tiled(e) for e in entries) and info['version'] == 1 and (info['width'], info['height'], info['depth']) == (W, H, 10)
    dec = dict(depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited')
    want = [m.decompress_yuv_tiled(e, **dec) for e in entries]
    got = m.decompress_yuv_sequence(blob)                # no colour parameter
    assert len(got) == 3 and all(type(g) is YuvFrame and _same(_whole(g, '420'), _whole(w, '420')) for g, w in zip(got, want))
    one = m.decompress_yuv_sequence(blob, frames=[2], layout='semiplanar')
    assert len(one) == 1 and _same(_whole(one[0], '420'), _whole(want[2].to_semiplanar(), '420'))
    assert m.yuv_sequence_info(blob)['lmb'] == [[[float(m.default_lmb)] * 4] * 3] * 3
    per_frame = m.compress_yuv_sequence(frames, tile=TILE, overlap=OV, lmb=[16, 256, 2048], **SEQ)
    assert m.yuv_sequence_info(per_frame)['lmb'] == [[[float(v)] * 4] * 3 for v in (16, 256, 2048)]
    # tile=None: the bytes of the path that was there before
    plain = m.compress_yuv_sequence(frames, max_batch=2, **SEQ)
    assert yuvseq.unpack_sequence(plain)[1] == [m.compress_yuv([f], **SEQ)[0] for f in frames]
    assert plain == m.compress_yuv_sequence(frames, max_batch=2, tile=None, overlap=0, **SEQ)
    assert m.yuv_sequence_info(plain)['lmb'] == [float(m.default_lmb)] * 3
    with pytest.raises(ValueError, match='overlap'):
        m.compress_yuv_sequence(frames, tile=TILE, overlap=15, **SEQ)


# ----------------------------------------------------------------------------------------------- callers
def test_evaluation_in_tiles(tmp_path):
    from lvae.evaluation import yuv_evaluate
    from lvae.metrics import psnr_yuv
    m = _model('qarv_base')
    frames = from_rgb01_any([_rgb(H, W, 400 + i) for i in range(2)], **KW)
    path = tmp_path / 'clip.yuv'
    yuv.write_yuv(frames, path)
    got = yuv_evaluate(m, path, W, H, depth=10, siting='left', tile=TILE, overlap=OV, batch=4)
    blobs = [m.compress_yuv_tiled(f, tile=TILE, overlap=OV, siting='left') for f in frames]
    assert got['bpp'] == sum(8 * len(b) / (H * W) for b in blobs) / 2           # the whole container counts
    recs = [m.decompress_yuv_tiled(b, **KW) for b in blobs]
    want = psnr_yuv([f.to(DEV) for f in frames], recs)
    assert got['psnr-y'] == pytest.approx(sum(r['psnr-y'] for r in want) / 2, rel=1e-12)
    assert set(yuv_evaluate(m, path, W, H, depth=10, siting='left', batch=4)) == set(got)       # tile=None: the same keys
    with pytest.raises(ValueError, match='psnr'):
        yuv_evaluate(m, path, W, H, depth=10, siting='left', tile=TILE, metrics=('psnr', 'ssim'))


def test_codec_script_in_tiles(tmp_path):
    """encode-yuv --tile and decode-yuv once each, on a 2-frame synthetic file: one tiled container per frame, recognised by its magic."""
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, out = tmp_path / 'in.yuv', tmp_path / 'bits', tmp_path / 'out.yuv'
    common = ['-m', 'qarv_base', '--synthetic', '2', '--batch', '4', '--depth', '10', '--siting', 'left']
    enc = ['encode-yuv', str(src), str(bits), '--size', str(W), str(H), '--tile', '64', '64', '--overlap', '16', '--lmb', '256']
    for cmd in (enc, ['decode-yuv', str(bits), str(out)]):
        r = subprocess.run([sys.executable, script] + cmd + common, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = _model('qarv_base')
    frames = yuv.read_yuv(src, W, H, '420', 10)
    files = sorted(bits.glob('*.bits'))
    assert len(frames) == 2 and [f.name for f in files] == ['frame00000.bits', 'frame00001.bits']
    blobs = [f.read_bytes() for f in files]
    assert blobs == [m.compress_yuv_tiled(f, tile=TILE, overlap=OV, lmb=256, siting='left') for f in frames] and blobs[0][:4] == b'LVTL'
    want = [m.decompress_yuv_tiled(b, **KW) for b in blobs]
    assert all(_same(_whole(a, '420'), [t.cpu() for t in _whole(b, '420')]) for a, b in zip(yuv.read_yuv(out, W, H, '420', 10), want))
