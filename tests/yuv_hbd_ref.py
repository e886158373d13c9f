"""The ITU-R definition of the YUV <-> RGB conversions for any depth, subsampling and chroma siting in fp64 numpy, written for the tests and
independent of lvae/utils/yuv.py, and the planes the high-bit-depth YUV tests share."""
import numpy as np

KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020': (0.2627, 0.0593)}
MATRICES, RANGES, DEPTHS = ('bt601', 'bt709', 'bt2020'), ('limited', 'full'), (8, 10, 12)
LAYOUTS = [('420', 'center'), ('420', 'left'), ('422', 'center'), ('422', 'left'), ('444', 'center'), ('444', 'left')]
SHIFTS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}       # (horizontal, vertical)


def scales(depth, rng):
    """luma offset, luma scale, chroma offset, chroma scale"""
    s, peak = 2.0 ** (depth - 8), 2.0 ** depth - 1
    return (16 * s, 219 * s, 128 * s, 224 * s) if rng == 'limited' else (0.0, peak, 128 * s, peak)


def _taps(n, left):
    """Output positions 0 .. 2n - 1 in the coordinates of the n chroma samples -> clamped tap indices and the fraction.  Centre siting:
    sample k lies at luma position 2k + 0.5; left siting: at 2k."""
    x = np.arange(2 * n)
    pos = x / 2.0 if left else (x + 0.5) / 2 - 0.5
    i0 = np.floor(pos).astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), pos - i0


def upsample64(c, sub, siting, chroma):
    sx, sy = SHIFTS[sub]
    c = c.astype(np.float64)
    if sy:
        if chroma == 'nearest':
            c = np.repeat(c, 2, 0)
        else:
            a, b, f = _taps(c.shape[0], False)               # vertically the chroma is centred for both sitings
            c = c[a] * (1 - f)[:, None] + c[b] * f[:, None]
    if sx:
        if chroma == 'nearest':
            c = np.repeat(c, 2, 1)
        else:
            a, b, f = _taps(c.shape[1], siting == 'left')
            c = c[:, a] * (1 - f)[None] + c[:, b] * f[None]
    return c


def yuv_to_rgb64(y, u, v, depth, sub, siting, matrix, rng, chroma, canvas=None):
    """integer planes -> (3, H, W) float64 RGB in [0, 1], edge-padded to `canvas`."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    yo, ys, co, cs = scales(depth, rng)
    yn = (y.astype(np.float64) - yo) / ys
    cb, cr = (upsample64(u, sub, siting, chroma) - co) / cs, (upsample64(v, sub, siting, chroma) - co) / cs
    rgb = np.stack([yn + 2 * (1 - kr) * cr,
                    yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr,
                    yn + 2 * (1 - kb) * cb]).clip(0, 1)
    if canvas is not None:
        rgb = np.pad(rgb, ((0, 0), (0, canvas[0] - y.shape[0]), (0, canvas[1] - y.shape[1])), mode='edge')
    return rgb


def downsample64(c, sub, siting):
    sx, sy = SHIFTS[sub]
    if sx:
        if siting == 'left':                                 # the (1, 2, 1) / 4 filter centred on the even column, the edge repeated
            p = np.pad(c, ((0, 0), (1, 0)), mode='edge')
            c = (p[:, 0:-1:2] + 2 * c[:, 0::2] + c[:, 1::2]) / 4
        else:
            c = (c[:, 0::2] + c[:, 1::2]) / 2
    if sy:
        c = (c[0::2] + c[1::2]) / 2
    return c


def rgb_to_yuv64(x, depth, sub, siting, matrix, rng):
    """(3, h, w) floats -> the float64 values (y, u, v) BEFORE rounding, on the code scale; NaN counts as 0."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    yo, ys, co, cs = scales(depth, rng)
    x = np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0).clip(0, 1)
    r, g, b = x
    yn = kr * r + kg * g + kb * b
    cb, cr = (b - yn) / (2 * (1 - kb)), (r - yn) / (2 * (1 - kr))
    return yo + ys * yn, co + cs * downsample64(cb, sub, siting), co + cs * downsample64(cr, sub, siting)


def check_codes(got, want64, depth, guard=1e-4):
    """got (integer codes) against the float64 values before rounding: equal to their rounding clamped to 0 .. 2^depth - 1, except that a
    code may differ by 1 where the float64 value lies within guard * 2^(depth - 8) of a half-integer (fp32 error is relative, so the band
    grows with the code range).  -> (samples inside the guard band, samples)."""
    want = np.clip(np.rint(want64), 0, 2 ** depth - 1).astype(np.int64)
    near = np.abs(want64 - np.floor(want64) - 0.5) < guard * 2 ** (depth - 8)
    diff = got.astype(np.int64) - want
    assert np.all(diff[~near] == 0), f'{int((diff[~near] != 0).sum())} codes differ outside the guard band'
    assert np.all(np.abs(diff) <= 1), 'a code differs by more than 1'
    return int(near.sum()), int(near.size)


def chroma_shape(h, w, sub):
    sx, sy = SHIFTS[sub]
    return (h >> sy, w >> sx)


def noise_planes(h, w, depth, sub, seed):
    """Uniform codes of `depth` bits: uint8 planes at depth 8, uint16 above."""
    g = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    cs = chroma_shape(h, w, sub)
    return tuple(g.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), cs, cs))


def ramp_planes(depth, sub):
    """128 x 128: every code of `depth` bits occurs in Y, in U and in V (Y and U rising, V falling, at different rates)."""
    n = 1 << depth
    dt = np.uint8 if depth == 8 else np.uint16
    cs = chroma_shape(128, 128, sub)
    i = np.arange(cs[0] * cs[1])
    assert i.size >= n
    return ((np.arange(128 * 128) % n).astype(dt).reshape(128, 128), (i % n).astype(dt).reshape(cs), ((n - 1 - i * 3) % n).astype(dt).reshape(cs))
