"""not-gpu: lvae/utils/tiling.py -- the tile grid, the blend weights and the tiled container -- and `blend_fp64`, the fp64 restatement of
the weight / blend definition that tests/test_gpu_tiling.py holds the stitch kernel against."""
import itertools
import struct

import numpy as np
import pytest

from lvae.utils import tiling


# ----------------------------------------------------------------------------------------------- the definition, restated in fp64
def axis_weight_fp64(x, o, T, size, overlap):
    """Weight of coordinate x (inside the tile at origin o) along one axis."""
    u, r = float(x - o), float(max(overlap, 1))
    wl = min(1.0, (u + 0.5) / r) if o > 0 else 1.0
    wr = min(1.0, (T - u - 0.5) / r) if o + T < size else 1.0
    return min(wl, wr)


def grid_rule(size, T, overlap):
    """The issue's grid rule for one axis, written out on its own."""
    if size <= T:
        return [0]
    n = int(np.ceil((size - overlap) / (T - overlap)))
    return [k * (T - overlap) for k in range(n - 1)] + [size - T]


def blend_fp64(tiles, h, w, th, tw, overlap):
    """tiles[k]: (3, >= th', >= tw') array of tile k (row-major).  -> ((3, h, w) fp64 blend, (h, w) cover count).  Per pixel: one
    covering tile -> its value; else sum(wy * wx * v) / sum(wy * wx) over the covering tiles."""
    ys, xs = grid_rule(h, th, overlap), grid_rule(w, tw, overlap)
    wy = np.zeros((len(ys), h))
    wx = np.zeros((len(xs), w))
    for r, o in enumerate(ys):
        for y in range(o, min(o + th, h)):
            wy[r, y] = axis_weight_fp64(y, o, th, h, overlap)
    for c, o in enumerate(xs):
        for x in range(o, min(o + tw, w)):
            wx[c, x] = axis_weight_fp64(x, o, tw, w, overlap)
    num, den = np.zeros((3, h, w)), np.zeros((h, w))
    count, last = np.zeros((h, w), np.int64), np.zeros((3, h, w))
    for r, oy in enumerate(ys):
        for c, ox in enumerate(xs):
            eh, ew = min(th, h - oy), min(tw, w - ox)
            v = np.asarray(tiles[r * len(xs) + c], dtype=np.float64)[:, :eh, :ew]
            wgt = wy[r, oy:oy + eh, None] * wx[c, None, ox:ox + ew]
            num[:, oy:oy + eh, ox:ox + ew] += wgt * v
            den[oy:oy + eh, ox:ox + ew] += wgt
            count[oy:oy + eh, ox:ox + ew] += 1
            last[:, oy:oy + eh, ox:ox + ew] = v
    return np.where(count[None] == 1, last, num / den), count


# ----------------------------------------------------------------------------------------------- grid
AXIS_CASES = [(size, T, ov) for T in (64, 128) for ov in (0, 1, 16, 31, T // 2)
              for size in (1, 50, T - 1, T, T + 1, T + ov, 2 * T - ov - 1, 2 * T - ov, 2 * T - ov + 1, 120, 150, 200, 333)]


@pytest.mark.parametrize('size,T,ov', AXIS_CASES)
def test_axis_grid_covers_and_weights_are_positive(size, T, ov):
    org = tiling.axis_origins(size, T, ov)
    assert org == grid_rule(size, T, ov)
    if size <= T:
        assert org == [0]                                   # the single padded tile
    else:
        assert all(0 <= o and o + T <= size for o in org)   # every tile lies inside the image
        assert org == sorted(set(org)) and org[0] == 0 and org[-1] == size - T
    cover = np.zeros(size, np.int64)
    wsum = np.zeros(size)
    for o in org:
        w32 = tiling.axis_weights(size, T, ov, o)
        assert w32.dtype == np.float32
        for x in range(size):
            inside = o <= x < o + T
            cover[x] += inside
            want = axis_weight_fp64(x, o, T, size, ov) if inside else 0.0
            assert abs(float(w32[x]) - want) <= 2.0 ** -23, (x, o)
            wsum[x] += want
    assert cover.min() >= 1 and cover.max() <= 3
    assert wsum.min() > 0


def test_triple_cover_case():
    assert tiling.axis_origins(120, 64, 16) == [0, 48, 56]
    ys, xs = tiling.tile_grid(120, 200, 64, 128, 16)
    assert (ys, xs) == ([0, 48, 56], [0, 72])
    cover = sum(((np.arange(120) >= o) & (np.arange(120) < o + 64)).astype(int) for o in ys)
    assert cover.max() == 3 and set(np.nonzero(cover == 3)[0]) == set(range(56, 64))


def test_grid_two_axes_and_boxes():
    for h, w, ov in itertools.product((50, 64, 65, 120, 150), (70, 128, 129, 200), (0, 16)):
        ys, xs = tiling.tile_grid(h, w, 64, 128, ov)
        assert ys == grid_rule(h, 64, ov) and xs == grid_rule(w, 128, ov)
        assert tiling.tiles_in_box(ys, xs, 64, 128, (0, 0, h, w)) == list(range(len(ys) * len(xs)))
    ys, xs = tiling.tile_grid(150, 200, 64, 128, 16)
    assert (ys, xs) == ([0, 48, 86], [0, 72])
    assert tiling.tiles_in_box(ys, xs, 64, 128, (0, 0, 48, 72)) == [0]
    assert tiling.tiles_in_box(ys, xs, 64, 128, (40, 60, 20, 20)) == [0, 1, 2, 3]
    assert tiling.tiles_in_box(ys, xs, 64, 128, (120, 130, 30, 70)) == [5]


@pytest.mark.parametrize('args', [(0, 10, 64, 64, 0), (10, 10, 0, 64, 0), (100, 100, 64, 64, 33), (100, 100, 64, 128, -1)])
def test_grid_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        tiling.tile_grid(*args)


def test_blend_reference_matches_the_fp64_restatement():
    rng = np.random.default_rng(3)
    for h, w, ov in [(150, 200, 16), (120, 200, 16), (150, 200, 0), (50, 70, 16)]:
        ys, xs = tiling.tile_grid(h, w, 64, 128, ov)
        tiles = [rng.random((3, 64, 128), dtype=np.float32) for _ in range(len(ys) * len(xs))]
        got, count = tiling.blend_reference(tiles, h, w, 64, 128, ov)
        want, count2 = blend_fp64(tiles, h, w, 64, 128, ov)
        assert np.array_equal(count, count2)
        assert np.abs(got - want).max() <= 1e-6                        # (the module forms wy * wx in fp32)
        assert np.array_equal(got[:, count == 1], want[:, count == 1])


# ----------------------------------------------------------------------------------------------- container
def _container(h=150, w=200, th=64, tw=128, ov=16, seed=0):
    rng = np.random.default_rng(seed)
    ys, xs = tiling.tile_grid(h, w, th, tw, ov)
    blobs = [rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes() for _ in range(len(ys) * len(xs))]
    return blobs, tiling.pack_tiled(h, w, th, tw, ov, blobs)


def test_container_round_trip_and_layout():
    blobs, c = _container()
    assert tiling.is_tiled(c) and not tiling.is_tiled(b'\x00' * 32)
    assert struct.unpack_from('<4sBBHIIHHHH', c, 0) == (b'LVTL', 1, 0, 16, 150, 200, 64, 128, 3, 2)
    n = 6
    assert struct.unpack_from(f'<{n}I', c, 24) == tuple(len(b) for b in blobs)
    assert c[24 + 4 * n:] == b''.join(blobs)
    u = tiling.unpack_tiled(c)
    assert u['tiles'] == blobs and u['lengths'] == [len(b) for b in blobs]
    assert (u['h'], u['w'], u['th'], u['tw'], u['overlap'], u['rows'], u['cols']) == (150, 200, 64, 128, 16, 3, 2)
    assert (u['ys'], u['xs']) == ([0, 48, 86], [0, 72])
    blobs1, c1 = _container(50, 70)                                      # a single padded tile
    assert tiling.unpack_tiled(c1)['tiles'] == blobs1 and len(blobs1) == 1
    with pytest.raises(ValueError):
        tiling.pack_tiled(150, 200, 64, 128, 16, blobs[:-1])


def test_container_corruptions_raise():
    _, c = _container()
    bad_magic = b'LVTX' + c[4:]
    bad_version = c[:4] + b'\x02' + c[5:]
    bad_grid = c[:20] + struct.pack('<HH', 2, 3) + c[24:]               # rows, cols swapped: not tile_grid's answer
    bad_grid2 = c[:8] + struct.pack('<I', 151 + 64) + c[12:]            # an h that needs a fourth tile row
    longer, shorter = c + b'\x00', c[:-1]
    bad_len = c[:24] + struct.pack('<I', struct.unpack_from('<I', c, 24)[0] + 1) + c[28:]
    for name, blob in dict(magic=bad_magic, version=bad_version, grid=bad_grid, grid2=bad_grid2, longer=longer, shorter=shorter,
                           length=bad_len, header=c[:10], table=c[:30]).items():
        with pytest.raises(ValueError):
            tiling.unpack_tiled(blob)
        assert name


# ----------------------------------------------------------------------------------------------- the native entry's argument checks
def test_stitch_entry_rejects_bad_arguments_without_gpu():
    """lvae_tile_stitch returns -22 before any HIP call (the addresses below are never dereferenced)."""
    import ctypes
    from lvae import _native
    lib = _native.lib()
    assert lib.lvae_tile_stitch_workspace_bytes(3, 2) == 6 * 8 + 5 * 4 and lib.lvae_tile_stitch_workspace_bytes(0, 2) == 0
    ys, xs = tiling.tile_grid(150, 200, 64, 128, 16)
    fake = 0x1000

    def call(tiles=None, plane=64 * 128, row=128, oy=ys, ox=xs, th=64, tw=128, ov=16, h=150, w=200, box=(0, 0, 150, 200), dst=fake,
             d_plane=150 * 200, d_row=200, u8=0, ws=fake, ws_bytes=1024):
        tiles = [fake] * (len(oy) * len(ox)) if tiles is None else tiles
        addr = (ctypes.c_void_p * len(tiles))(*tiles)
        return lib.lvae_tile_stitch(addr, plane, row, (ctypes.c_int * len(oy))(*oy), (ctypes.c_int * len(ox))(*ox), len(oy), len(ox), th, tw,
                                    ov, h, w, *box, dst, d_plane, d_row, u8, ws, ws_bytes, None)

    assert call(tiles=[fake, fake, None, fake, fake, fake]) == -22                  # a null tile inside the window
    assert call(tiles=[None] + [fake] * 5, box=(0, 0, 10, 10)) == -22
    for box in [(0, 0, 151, 200), (0, 1, 150, 200), (-1, 0, 10, 10), (0, 0, 0, 10), (149, 199, 2, 1)]:
        assert call(box=box) == -22, box                                             # a window outside the image, or empty
    assert call(row=127) == -22 and call(plane=64 * 128 - 1) == -22                  # strides that do not hold (th, tw)
    assert call(d_row=199) == -22 and call(d_plane=150 * 200 - 1) == -22 and call(u8=1, d_row=599) == -22
    assert call(oy=[0, 48, 85]) == -22 and call(ox=[0, 71]) == -22 and call(oy=[0, 48]) == -22       # not the grid rule's origins
    assert call(ov=33) == -22 and call(ov=-1) == -22
    assert call(ws_bytes=67) == -22 and call(ws=fake + 4) == -22 and call(ws=None) == -22 and call(dst=None) == -22
