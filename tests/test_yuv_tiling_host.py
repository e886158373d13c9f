"""Tiled coding of YUV frames, host side (no GPU): the argument errors of compress_yuv_tiled / stitch_tiles_yuv / lvae_tile_stitch_yuv that
are decided before any device work, the chroma-grid property of the tile grid they rest on, and tiled frame entries in the LVYS container."""
import ctypes
import functools
import itertools

import pytest
import torch

from lvae import _native
from lvae.utils import tiling, yuvseq
from lvae.utils.yuv import Yuv420Frame, YuvFrame, stitch_tiles_yuv


@functools.lru_cache(maxsize=None)
def _model():
    import lvae
    return lvae.get_model('qarv_base', pretrained=False)


def _frame(h, w, depth=8, sub='420'):
    sx, sy = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}[sub]
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8 if depth == 8 else torch.int16)
    return YuvFrame(z(h, w), z(h >> sy, w >> sx), z(h >> sy, w >> sx), depth, sub)


# ----------------------------------------------------------------------------------------------- compress_yuv_tiled
@pytest.mark.parametrize('sub', ['420', '422'])
def test_odd_overlap_is_refused_where_the_chroma_is_subsampled(sub):
    m = _model()
    with pytest.raises(ValueError, match='overlap'):
        m.compress_yuv_tiled(_frame(128, 192, 10, sub), tile=(64, 64), overlap=15)
    with pytest.raises(ValueError, match='overlap'):
        m.compress_yuv_tiled(_frame(128, 192, 10, sub).to_semiplanar(), tile=(64, 64), overlap=1)
    if sub == '420':
        f = _frame(128, 192)
        with pytest.raises(ValueError, match='overlap'):
            m.compress_yuv_tiled(Yuv420Frame('i420', f.y, f.u, f.v), tile=(64, 64), overlap=7)


def test_other_argument_errors_of_compress_yuv_tiled():
    m = _model()
    f = _frame(128, 192)
    with pytest.raises(ValueError, match='max_stride'):
        m.compress_yuv_tiled(f, tile=(64, 100))
    with pytest.raises(ValueError, match='frame'):
        m.compress_yuv_tiled(torch.zeros(128, 192, 3, dtype=torch.uint8), tile=(64, 64))
    with pytest.raises(ValueError, match='frame'):
        m.compress_yuv_tiled([f], tile=(64, 64))
    with pytest.raises(ValueError, match='siting'):
        m.compress_yuv_tiled(Yuv420Frame('i420', f.y, f.u, f.v), tile=(64, 64), siting='left')


@pytest.mark.parametrize('h,w,tile,overlap', [(128, 192, (64, 64), 16), (2160, 3840, (512, 768), 32), (70, 118, (32, 48), 8), (58, 90, (32, 48), 8),
                                              (1080, 1920, (256, 256), 0), (20, 30, (32, 48), 6), (4320, 7680, (512, 768), 64), (130, 66, (64, 64), 2)])
def test_tile_origins_lie_on_the_chroma_grid(h, w, tile, overlap):
    """Even frame sides, even tile sides (multiples of max_stride) and an even overlap: every origin is even, the last one (size - T) too."""
    ys, xs = tiling.tile_grid(h, w, tile[0], tile[1], overlap)
    assert all(y % 2 == 0 for y in ys) and all(x % 2 == 0 for x in xs)
    assert ys[-1] + min(tile[0], h) == h and xs[-1] + min(tile[1], w) == w


# ----------------------------------------------------------------------------------------------- stitch_tiles_yuv
TILES = [torch.zeros(3, 32, 48) for _ in range(4)]          # the 2 x 2 grid of a 64 x 96 image; never read: every call below raises first
GRID = (64, 96, 32, 48, 0)


@pytest.mark.parametrize('sub,box', [('420', (1, 0, 32, 48)), ('420', (0, 0, 31, 48)), ('420', (0, 3, 32, 48)), ('420', (0, 0, 32, 47)),
                                     ('422', (0, 3, 32, 48)), ('422', (0, 0, 32, 47))])
def test_box_off_the_chroma_grid(sub, box):
    with pytest.raises(ValueError, match='chroma grid'):
        stitch_tiles_yuv(TILES, *GRID, box=box, subsampling=sub)


def test_box_parity_that_the_subsampling_allows_is_not_refused_for_it():
    """4:2:2 takes odd rows and 4:4:4 any box: these get past the grid check and fail on the next one, the box outside the image."""
    for sub, box in (('422', (1, 0, 64, 48)), ('444', (1, 3, 64, 47))):
        with pytest.raises(ValueError, match='not inside'):
            stitch_tiles_yuv(TILES, *GRID, box=box, subsampling=sub)


@pytest.mark.parametrize('kw', [dict(layout='semiplanar'), dict(layout='semiplanar', depth=10, subsampling='444'), dict(layout='nv12', depth=10),
                                dict(layout='nv12', subsampling='422'), dict(layout='i420', siting='left'), dict(layout='nv12', matrix='bt2020'),
                                dict(layout='p010', depth=10), dict(depth=9), dict(subsampling='440'), dict(siting='top'), dict(matrix='bt470'),
                                dict(range='studio')])
def test_layout_and_depth_combinations(kw):
    with pytest.raises(ValueError):
        stitch_tiles_yuv(TILES, *GRID, **kw)


def test_tile_list_errors_are_those_of_stitch_tiles():
    with pytest.raises(ValueError, match='3 tiles'):
        stitch_tiles_yuv(TILES[:3], *GRID)
    with pytest.raises(ValueError, match='no decoded tile'):
        stitch_tiles_yuv([None] * 4, *GRID)
    with pytest.raises(ValueError, match='overlap'):
        stitch_tiles_yuv(TILES, 64, 96, 32, 48, 17)
    with pytest.raises(ValueError, match='not decoded'):
        stitch_tiles_yuv([TILES[0], None, TILES[2], TILES[3]], *GRID)
    with pytest.raises(ValueError, match='not decoded.*column before'):        # left siting: column 47 belongs to tile column 0
        stitch_tiles_yuv([None, TILES[1], None, TILES[3]], *GRID, box=(0, 48, 64, 48), depth=10, siting='left')


# ----------------------------------------------------------------------------------------------- the native entry
def test_native_argument_checks_without_gpu():
    """-22 before any HIP call; the addresses are never dereferenced on this path."""
    L = _native.lib()
    addr = (ctypes.c_void_p * 4)(4096, 8192, 12288, 16384)
    oy, ox = (ctypes.c_int * 2)(0, 32), (ctypes.c_int * 2)(0, 48)
    ok = dict(tiles=addr, plane=32 * 48, row=48, oy=oy, ox=ox, rows=2, cols=2, th=32, tw=48, ov=0, h=64, w=96, y0=0, x0=0, hh=64, ww=96, depth=10,
              sub=0, siting=0, matrix=1, range=0, layout=0, y=1 << 20, u=1 << 21, v=1 << 22, y_row=96, u_row=48, v_row=48, ws=1 << 23, ws_bytes=64)

    def call(**change):
        a = dict(ok, **change)
        return L.lvae_tile_stitch_yuv(*[a[k] for k in ok], None)
    gaps, left_gaps = (ctypes.c_void_p * 4)(4096, None, 12288, 16384), (ctypes.c_void_p * 4)(None, 8192, None, 16384)
    cases = [dict(tiles=None), dict(oy=None), dict(ws=None), dict(y=None), dict(u=None), dict(v=None), dict(rows=0), dict(ov=-1), dict(ov=17),
             dict(y0=1), dict(hh=63), dict(x0=1, ww=95), dict(ww=95), dict(hh=66), dict(ww=98), dict(hh=0), dict(row=47), dict(plane=32 * 48 - 1),
             dict(ws_bytes=47), dict(ws=(1 << 23) + 4), dict(oy=(ctypes.c_int * 2)(0, 30)), dict(depth=9), dict(sub=3), dict(siting=2), dict(matrix=3),
             dict(range=2), dict(layout=2), dict(layout=-1), dict(y_row=95), dict(u_row=47), dict(v_row=47), dict(layout=1, u_row=95),
             dict(layout=1, sub=2), dict(layout=1, depth=8, sub=1), dict(layout=1, depth=8, siting=1), dict(layout=1, depth=8, matrix=2),
             dict(tiles=gaps), dict(tiles=left_gaps, x0=48, ww=48, siting=1),                  # column 47, which the first chroma column reads, is null
             dict(sub=1, x0=1, ww=94), dict(sub=1, ww=95)]
    for change in cases:
        assert call(**change) == -22, change
    assert L.lvae_tile_stitch_workspace_bytes(2, 2) == 4 * 8 + 4 * 4


# ----------------------------------------------------------------------------------------------- tiled frames inside LVYS
META = dict(width=192, height=128, depth=10, subsampling='420', siting='left', matrix='bt2020', range='limited', chroma='bilinear',
            layout='planar', model='qarv_base', gemm='f16x2')


def test_tiled_frame_entries_round_trip_through_the_sequence_container():
    ys, xs = tiling.tile_grid(128, 192, 64, 64, 16)
    entries = [tiling.pack_tiled(128, 192, 64, 64, 16, [bytes([f, k]) * (k + 1) for k in range(len(ys) * len(xs))]) for f in range(3)]
    blob = yuvseq.pack_sequence(META, entries)
    info, frames = yuvseq.unpack_sequence(blob)
    assert frames == entries and info['frames'] == 3 and info['version'] == yuvseq.VERSION == 1
    assert info['lengths'] == [len(e) for e in entries] and {k: info[k] for k in yuvseq.FIELDS} == META
    for k, e in enumerate(entries):
        fb = yuvseq.frame_blob(blob, info, k)
        assert tiling.is_tiled(fb) and fb == e
        c = tiling.unpack_tiled(fb)
        assert (c['h'], c['w'], c['th'], c['tw'], c['overlap'], c['ys'], c['xs']) == (128, 192, 64, 64, 16, ys, xs)
        assert c['tiles'] == [bytes([k, t]) * (t + 1) for t in range(len(ys) * len(xs))]
    mixed = yuvseq.pack_sequence(META, [entries[0], b'\x00' * 9])                       # entries are opaque: kinds may differ
    info = yuvseq.yuv_sequence_info(mixed)
    assert [tiling.is_tiled(yuvseq.frame_blob(mixed, info, k)) for k in range(2)] == [True, False]
    assert not tiling.is_tiled(blob) and not yuvseq.is_yuv_sequence(entries[0])
    assert list(itertools.accumulate([info['offsets'][0]] + info['lengths']))[:-1] == info['offsets']
