"""Tiled coding of large images, host side: the tile grid, the blend weights of overlapping tiles and the container that holds the
tiles' bytes.  Pure Python / numpy, no GPU: the models' compress_tiled / decompress_tiled / decompress_region (lvae/models/base.py)
code each tile through compress_images / decompress_batch and put the reconstructions together with lvae_tile_stitch
(csrc/tile_stitch.hip), whose arithmetic `axis_weights` and `blend_reference` state.

Grid (per axis, here for the width): w <= tw gives one column with origin 0 and valid extent w (the tile is replicate-padded by the
existing path).  Otherwise n = ceil((w - overlap) / (tw - overlap)) columns with origins k * (tw - overlap) for k < n - 1 and w - tw for
the last: every tile is full size, nothing is padded, all tiles of an image share one shape.  The last tile may overlap its neighbour by
more than `overlap`, so a pixel is covered by up to 3 tiles per axis.  Tiles are numbered row-major.
"""
import struct

import numpy as np

MAGIC = b'LVTL'
VERSION = 1
_HEAD = '<4sBBHIIHHHH'          # magic, version, reserved, overlap, h, w, th, tw, rows, cols
HEAD_BYTES = struct.calcsize(_HEAD)


def axis_origins(size, T, overlap):
    """Tile origins of one axis."""
    if size <= T:
        return [0]
    step = T - overlap
    n = -(-(size - overlap) // step)
    return [k * step for k in range(n - 1)] + [size - T]


def tile_grid(h, w, th, tw, overlap):
    """(ys, xs): the row and column origins of the tiles of an (h, w) image; tile k (row-major) starts at (ys[k // len(xs)],
    xs[k % len(xs)]) and holds min(h, th) x min(w, tw) pixels of the image."""
    h, w, th, tw, overlap = int(h), int(w), int(th), int(tw), int(overlap)
    if h <= 0 or w <= 0 or th <= 0 or tw <= 0:
        raise ValueError(f'tile_grid: sizes must be positive, got image {(h, w)}, tile {(th, tw)}')
    if not 0 <= overlap <= min(th, tw) // 2:
        raise ValueError(f'tile_grid: overlap {overlap} outside [0, min(th, tw) // 2 = {min(th, tw) // 2}]')
    return axis_origins(h, th, overlap), axis_origins(w, tw, overlap)


def tiles_in_box(ys, xs, th, tw, box):
    """Row-major numbers of the tiles that intersect box = (y0, x0, hh, ww)."""
    y0, x0, hh, ww = box
    rows = [r for r, o in enumerate(ys) if o < y0 + hh and o + th > y0]
    cols = [c for c, o in enumerate(xs) if o < x0 + ww and o + tw > x0]
    return [r * len(xs) + c for r in rows for c in cols]


def axis_weights(size, T, overlap, origin, dtype=np.float32):
    """The ramp weight of every coordinate of one axis for the tile at `origin` (0 outside the tile): min(wl, wr) with
    wl = min(1, (u + 0.5) / r) if origin > 0 else 1, wr = min(1, (T - u - 0.5) / r) if origin + T < size else 1, u = x - origin,
    r = max(overlap, 1)."""
    x = np.arange(size)
    u = (x - origin).astype(dtype)
    r = dtype(max(overlap, 1))
    one = dtype(1)
    wl = np.minimum(one, (u + dtype(0.5)) / r) if origin > 0 else np.ones(size, dtype)
    wr = np.minimum(one, (dtype(T) - u - dtype(0.5)) / r) if origin + T < size else np.ones(size, dtype)
    wgt = np.minimum(wl, wr).astype(dtype)
    wgt[(x < origin) | (x >= origin + T)] = 0
    return wgt


def blend_reference(tiles, h, w, th, tw, overlap, dtype=np.float64):
    """The definition of the stitched image in numpy: tiles[k] is tile k's (3, th, tw) array (row-major numbering; a single padded tile
    may be larger than the image).  -> ((3, h, w) blended values, (h, w) number of covering tiles).  A pixel with one covering tile
    takes that tile's value unchanged; otherwise sum(w v) / sum(w), w = wy * wx formed in fp32, accumulated in ascending tile number in
    `dtype`."""
    ys, xs = tile_grid(h, w, th, tw, overlap)
    acc, wsum = np.zeros((3, h, w), dtype), np.zeros((h, w), dtype)
    count, single = np.zeros((h, w), np.int32), np.zeros((3, h, w), dtype)
    for k, (oy, ox) in enumerate((oy, ox) for oy in ys for ox in xs):
        eh, ew = min(h - oy, th), min(w - ox, tw)
        wgt = (axis_weights(h, th, overlap, oy)[oy:oy + eh, None] * axis_weights(w, tw, overlap, ox)[None, ox:ox + ew]).astype(np.float32)
        v = np.asarray(tiles[k])[:, :eh, :ew].astype(dtype)
        acc[:, oy:oy + eh, ox:ox + ew] += wgt.astype(dtype) * v
        wsum[oy:oy + eh, ox:ox + ew] += wgt.astype(dtype)
        count[oy:oy + eh, ox:ox + ew] += 1
        single[:, oy:oy + eh, ox:ox + ew] = v
    assert count.min() >= 1 and wsum.min() > 0
    return np.where(count[None] == 1, single, acc / wsum), count


def pack_tiled(h, w, th, tw, overlap, blobs):
    """The container: header, one uint32 byte length per tile, the tiles' blobs row-major (little-endian)."""
    ys, xs = tile_grid(h, w, th, tw, overlap)
    if len(blobs) != len(ys) * len(xs):
        raise ValueError(f'pack_tiled: {len(blobs)} blobs for a {len(ys)} x {len(xs)} grid')
    if max(th, tw, len(ys), len(xs)) > 0xffff:
        raise ValueError('pack_tiled: tile or grid size beyond 65535')
    head = struct.pack(_HEAD, MAGIC, VERSION, 0, overlap, h, w, th, tw, len(ys), len(xs))
    return head + struct.pack(f'<{len(blobs)}I', *[len(b) for b in blobs]) + b''.join(bytes(b) for b in blobs)


def unpack_tiled(blob):
    """Inverse of pack_tiled -> dict(h, w, th, tw, overlap, rows, cols, ys, xs, lengths, tiles) with tiles a list of bytes.  ValueError:
    bad magic, bad version, a grid that is not tile_grid's for the header's values, lengths that do not add up to the blob."""
    blob = bytes(blob)
    if len(blob) < HEAD_BYTES or blob[:4] != MAGIC:
        raise ValueError('not a tiled container (bad magic)')
    _, version, _reserved, overlap, h, w, th, tw, rows, cols = struct.unpack_from(_HEAD, blob, 0)
    if version != VERSION:
        raise ValueError(f'tiled container version {version}, expected {VERSION}')
    try:
        ys, xs = tile_grid(h, w, th, tw, overlap)
    except ValueError as e:
        raise ValueError(f'tiled container: bad header ({e})') from None
    if (rows, cols) != (len(ys), len(xs)):
        raise ValueError(f'tiled container: grid {rows} x {cols}, but {len(ys)} x {len(xs)} tiles cover {(h, w)}')
    n = rows * cols
    if len(blob) < HEAD_BYTES + 4 * n:
        raise ValueError('tiled container: truncated length table')
    lengths = list(struct.unpack_from(f'<{n}I', blob, HEAD_BYTES))
    o = HEAD_BYTES + 4 * n
    if o + sum(lengths) != len(blob):
        raise ValueError(f'tiled container: tile lengths add up to {o + sum(lengths)} bytes, the blob has {len(blob)}')
    tiles = []
    for ln in lengths:
        tiles.append(blob[o:o + ln])
        o += ln
    return dict(h=h, w=w, th=th, tw=tw, overlap=overlap, rows=rows, cols=cols, ys=ys, xs=xs, lengths=lengths, tiles=tiles)


def is_tiled(blob):
    return bytes(blob[:4]) == MAGIC
