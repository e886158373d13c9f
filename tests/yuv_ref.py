"""The ITU-R definition of the YUV 4:2:0 <-> RGB conversions in fp64 numpy, written for the tests and independent of lvae/utils/yuv.py,
and the frames the YUV tests share."""
import numpy as np

KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
COMBOS = [(m, r, c) for m in ('bt601', 'bt709') for r in ('limited', 'full') for c in ('nearest', 'bilinear')]


def _taps(n):
    """Luma positions 0 .. 2n - 1 in chroma coordinates (centre siting: (x + 0.5) / 2 - 0.5) -> clamped tap indices and the fraction."""
    pos = (np.arange(2 * n) + 0.5) / 2 - 0.5
    i0 = np.floor(pos).astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), pos - i0


def upsample64(c, chroma):
    c = c.astype(np.float64)
    if chroma == 'nearest':
        return np.repeat(np.repeat(c, 2, 0), 2, 1)
    a, b, f = _taps(c.shape[0])
    c = c[a] * (1 - f)[:, None] + c[b] * f[:, None]
    a, b, f = _taps(c.shape[1])
    return c[:, a] * (1 - f)[None] + c[:, b] * f[None]


def yuv_to_rgb64(y, u, v, matrix, rng, chroma, canvas=None):
    """uint8 planes -> (3, H, W) float64 RGB in [0, 1], edge-padded to `canvas`."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    cb, cr = upsample64(u, chroma) - 128, upsample64(v, chroma) - 128
    if rng == 'limited':
        yn, cb, cr = (y.astype(np.float64) - 16) / 219, cb / 224, cr / 224
    else:
        yn, cb, cr = y.astype(np.float64) / 255, cb / 255, cr / 255
    rgb = np.stack([yn + 2 * (1 - kr) * cr,
                    yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr,
                    yn + 2 * (1 - kb) * cb]).clip(0, 1)
    if canvas is not None:
        rgb = np.pad(rgb, ((0, 0), (0, canvas[0] - y.shape[0]), (0, canvas[1] - y.shape[1])), mode='edge')
    return rgb


def rgb_to_yuv64(x, matrix, rng):
    """(3, h, w) floats -> the float64 values (y, u, v) BEFORE rounding (already on the byte scale); NaN counts as 0."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    x = np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0).clip(0, 1)
    r, g, b = x
    yn = kr * r + kg * g + kb * b
    cb, cr = (b - yn) / (2 * (1 - kb)), (r - yn) / (2 * (1 - kr))
    mean4 = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) / 4
    if rng == 'limited':
        return 16 + 219 * yn, 128 + 224 * mean4(cb), 128 + 224 * mean4(cr)
    return 255 * yn, 128 + 255 * mean4(cb), 128 + 255 * mean4(cr)


def bytes_of(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def check_bytes(got, want64, guard=1e-4):
    """got (uint8) against the float64 values before rounding: equal to their rounding, except that a byte may differ by 1 where the
    float64 value lies within `guard` of a half-integer.  -> (samples inside the guard band, samples)."""
    want = bytes_of(want64)
    near = np.abs(want64 - np.floor(want64) - 0.5) < guard
    diff = got.astype(np.int64) - want.astype(np.int64)
    assert np.all(diff[~near] == 0), f'{int((diff[~near] != 0).sum())} bytes differ outside the guard band'
    assert np.all(np.abs(diff) <= 1), 'a byte differs by more than 1'
    return int(near.sum()), int(near.size)


def all_values_planes():
    """512 x 512: (U, V) runs over every pair of byte values, and every U and every V meets every Y."""
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    u, v = i.astype(np.uint8), j.astype(np.uint8)
    y = np.empty((512, 512), dtype=np.uint8)
    for a in range(2):
        for b in range(2):
            y[a::2, b::2] = (i + j + 64 * (2 * a + b)) % 256
    return y, u, v


def noise_planes(h, w, seed):
    g = np.random.default_rng(seed)
    return (g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            g.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def rgb_batch():
    """(5, 3, 128, 192) fp32 torch tensor in [-0.1, 1.1] with exact 0 / 1 / out-of-range values, a NaN and infinities in every image's corner."""
    import torch
    g = torch.Generator().manual_seed(6)
    x = torch.rand(5, 3, 128, 192, generator=g) * 1.2 - 0.1
    x[:, :, 0, :6] = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5, 0.25])
    x[:, 0, 1, 0] = float('nan')
    x[:, 1, 1, 1] = float('inf')
    x[:, 2, 0, 1] = float('-inf')
    return x


def nv12_uv(u, v):
    return np.ascontiguousarray(np.stack([u, v], -1))
