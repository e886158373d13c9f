"""Reduced-resolution coding, host side: the definition of the resampler and the container of a scaled image.  Pure Python / numpy,
no GPU: csrc/resample.hip (lvae_resample_u8_to_f32 / lvae_resample_f32_to_u8 / lvae_resample_f32) is held to `axis_table` and
`resize_reference`, and the models' compress_scaled / decompress_scaled (lvae/models/base.py) wrap their own blobs in `pack_scaled`.

The resampler is separable and antialiased, with pixel-centre alignment and the window rule of PIL's Image.resize and of torch's
F.interpolate(antialias=True, align_corners=False).  One axis n_in -> n_out with a filter f of half-width a, all in fp64:
s = n_in / n_out, fs = max(s, 1), support = a * fs; output i has its centre at c = (i + 0.5) * s and the taps j = lo .. hi - 1 with
lo = max(0, int(c - support + 0.5)), hi = min(n_in, int(c + support + 0.5)) and w_j = f((j - c + 0.5) / fs): the window is truncated
at the border, not padded.  The weights are normalised to sum 1 in fp64 and then rounded to fp32.  A resized image is the horizontal
pass followed by the vertical pass with these fp32 weights; an axis with n_out == n_in is not filtered at all (a bit copy: the Lanczos
weights at integers are not exactly 0).
"""
import math
import struct

import numpy as np

FILTERS = ('bilinear', 'bicubic', 'lanczos3')          # a name's code in the container is its index
HALF_WIDTH = {'bilinear': 1.0, 'bicubic': 2.0, 'lanczos3': 3.0}
MAX_RATIO = 8                                          # n_in / n_out and n_out / n_in per axis
TILE_ROWS = 16                                         # output rows of a workgroup's tile (csrc/resample.hip: RS_TY)

MAGIC = b'LVRS'
VERSION = 1
_HEAD = '<4sBBHIIIII'           # magic, version, filter, reserved, h, w, coded h, coded w, payload bytes
HEAD_BYTES = struct.calcsize(_HEAD)


def _filter(name):
    if name not in FILTERS:
        raise ValueError(f'resample filter is one of {FILTERS}, got {name!r}')
    return name


def _kernel(name, x):
    """f(x) of a filter on an fp64 array."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    if name == 'bilinear':
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if name == 'bicubic':                              # Keys, a = -0.5
        a = -0.5
        near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    px = np.pi * np.where(x == 0.0, 1.0, x)
    lz = np.sin(px) / px * np.sin(px / 3.0) / (px / 3.0)
    return np.where(x == 0.0, 1.0, np.where(x < 3.0, lz, 0.0))


def check_ratio(n_in, n_out):
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f'resample: sizes must be positive, got {n_in} -> {n_out}')
    if n_in > MAX_RATIO * n_out or n_out > MAX_RATIO * n_in:
        raise ValueError(f'resample: {n_in} -> {n_out} is outside the supported ratios [1/{MAX_RATIO}, {MAX_RATIO}]')
    return n_in, n_out


def axis_windows(n_in, n_out, filter='lanczos3'):
    """(lo, hi) int arrays of the window rule: output i takes the taps lo[i] .. hi[i] - 1."""
    n_in, n_out = check_ratio(n_in, n_out)
    a = HALF_WIDTH[_filter(filter)]
    s = n_in / n_out
    support = a * max(s, 1.0)
    lo, hi = np.empty(n_out, np.int64), np.empty(n_out, np.int64)
    for i in range(n_out):
        c = (i + 0.5) * s
        lo[i] = max(0, int(c - support + 0.5))
        hi[i] = min(n_in, int(c + support + 0.5))
    return lo, hi


def axis_table(n_in, n_out, filter='lanczos3'):
    """The definition of one axis: (start int32[n_out], weights float32[n_out, taps]); output i = sum_j weights[i, j] * x[start[i] + j],
    rows zero-padded to the axis's largest tap count (a padded tap may lie beyond n_in - 1: it has weight 0 and is never read as such --
    readers clamp its index).  n_out == n_in gives the identity as one tap of weight 1; callers skip such an axis instead."""
    n_in, n_out = check_ratio(n_in, n_out)
    _filter(filter)
    if n_in == n_out:
        return np.arange(n_out, dtype=np.int32), np.ones((n_out, 1), np.float32)
    lo, hi = axis_windows(n_in, n_out, filter)
    s = n_in / n_out
    fs = max(s, 1.0)
    taps = int((hi - lo).max())
    wgt = np.zeros((n_out, taps), np.float32)
    for i in range(n_out):
        c = (i + 0.5) * s
        j = np.arange(lo[i], hi[i], dtype=np.float64)
        w = _kernel(filter, (j - c + 0.5) / fs)
        wgt[i, :hi[i] - lo[i]] = (w / w.sum()).astype(np.float32)
    return lo.astype(np.int32), wgt


def tile_span(start, taps, n_in, rows=TILE_ROWS):
    """The largest number of input rows that `rows` consecutive output rows read (what lvae_resample_* take as `yspan`: a workgroup's
    LDS tile is sized from it)."""
    start = np.asarray(start, dtype=np.int64)
    last = np.minimum(np.arange(len(start)) + rows - 1, len(start) - 1)
    return int((np.minimum(start[last] + taps, n_in) - start).max())


def _apply_axis(x, axis, n_out, filter):
    """One pass in fp64 along `axis` with the fp32 weights of axis_table."""
    n_in = x.shape[axis]
    if n_out == n_in:
        return x
    start, wgt = axis_table(n_in, n_out, filter)
    idx = np.minimum(start[:, None].astype(np.int64) + np.arange(wgt.shape[1])[None, :], n_in - 1)       # (n_out, taps)
    x = np.moveaxis(x, axis, -1)
    out = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    w64 = wgt.astype(np.float64)
    for j in range(wgt.shape[1]):                      # taps ascending
        out += x[..., idx[:, j]] * w64[:, j]
    return np.moveaxis(out, -1, axis)


def resize_reference(x, h, w, filter='lanczos3', clamp=False):
    """The definition of a resized image in numpy fp64: x is (..., h_in, w_in); the horizontal pass, then the vertical pass, each with
    axis_table's fp32 weights and exact (fp64) arithmetic; an axis whose size does not change is skipped.  clamp: the result is clamped
    to [0, 1] (bicubic and Lanczos overshoot).  -> (..., h, w) float64."""
    x = np.asarray(x, dtype=np.float64)
    check_ratio(x.shape[-2], h)
    check_ratio(x.shape[-1], w)
    y = _apply_axis(_apply_axis(x, -1, int(w), filter), -2, int(h), filter)
    return np.clip(y, 0.0, 1.0) if clamp else y


def scaled_size(h, w, scale=None, size=None):
    """The coded size of an (h, w) image: exactly one of `scale` (-> max(1, round(h * scale)), max(1, round(w * scale))) and `size`
    (-> itself); ValueError otherwise, or when an axis leaves the supported ratios."""
    if (scale is None) == (size is None):
        raise ValueError('give exactly one of scale and size')
    if scale is not None:
        scale = float(scale)
        if not (math.isfinite(scale) and scale > 0):
            raise ValueError(f'scale must be a positive number, got {scale}')
        ch, cw = max(1, round(h * scale)), max(1, round(w * scale))
    else:
        ch, cw = (int(v) for v in size)
    check_ratio(h, ch)
    check_ratio(w, cw)
    return ch, cw


def pack_scaled(filter, size, coded, payload):
    """The container of a scaled image: header (little-endian), then the model's own blob for the coded-resolution image,
    unchanged.  size: the original (h, w); coded: the (h, w) the payload holds."""
    payload = bytes(payload)
    (h, w), (ch, cw) = (int(v) for v in size), (int(v) for v in coded)
    check_ratio(h, ch)
    check_ratio(w, cw)
    return struct.pack(_HEAD, MAGIC, VERSION, FILTERS.index(_filter(filter)), 0, h, w, ch, cw, len(payload)) + payload


def scaled_info(blob):
    """Header parsing only -> dict(filter, size, coded, payload_bytes, offset).  ValueError: bad magic, version or filter code, sizes that are
    zero or outside the supported ratios, a payload length beyond the blob."""
    if len(blob) < HEAD_BYTES or bytes(blob[:4]) != MAGIC:
        raise ValueError('not a scaled container (bad magic)')
    _, version, fcode, _reserved, h, w, ch, cw, n = struct.unpack_from(_HEAD, bytes(blob[:HEAD_BYTES]), 0)
    if version != VERSION:
        raise ValueError(f'scaled container version {version}, expected {VERSION}')
    if fcode >= len(FILTERS):
        raise ValueError(f'scaled container: unknown filter code {fcode}')
    try:
        check_ratio(h, ch)
        check_ratio(w, cw)
    except ValueError as e:
        raise ValueError(f'scaled container: bad header ({e})') from None
    if HEAD_BYTES + n > len(blob):
        raise ValueError(f'scaled container: payload of {n} bytes, the blob holds {len(blob) - HEAD_BYTES} behind the header')
    return dict(filter=FILTERS[fcode], size=(h, w), coded=(ch, cw), payload_bytes=n, offset=HEAD_BYTES)


def unpack_scaled(blob):
    """Inverse of pack_scaled -> (info dict of scaled_info, payload bytes)."""
    info = scaled_info(blob)
    return info, bytes(blob[HEAD_BYTES:HEAD_BYTES + info['payload_bytes']])


def is_scaled(blob):
    return bytes(blob[:4]) == MAGIC
