"""8-bit images in and out of the codec: interleaved RGB bytes (HWC uint8 tensors) <-> the fp32 NCHW tensors in [0, 1] the models code.

On the GPU the two conversions are the HIP kernels of csrc/image_io.hip (`lvae_image_u8_to_f32`, `lvae_image_f32_to_u8`): an image is
uploaded as the 3 bytes per pixel its PNG held, replicate-padded and converted where the encoder reads it, and a reconstruction is rounded
to bytes on the device before it is copied back.  CPU tensors take the expressions of lvae/utils/coding.py -- the same bits.
`stitch_tiles` puts the decoded tiles of a tiled image (lvae/utils/tiling.py) together on the GPU (csrc/tile_stitch.hip).
"""
import ctypes
import math

import numpy as np
import torch

from . import coding


def load_u8(path_or_pil):
    """An image file (or an opened PIL image) as an (h, w, 3) uint8 CPU tensor, in pinned memory when a GPU is there (its upload is then
    one asynchronous copy).  8-bit RGB only: any other PIL mode raises ValueError."""
    from PIL import Image
    img = path_or_pil if isinstance(path_or_pil, Image.Image) else Image.open(path_or_pil)
    if img.mode != 'RGB':
        raise ValueError(f'load_u8: expected an 8-bit RGB image, got PIL mode {img.mode!r}')
    a = torch.from_numpy(np.array(img, copy=True))
    if torch.cuda.is_available():
        t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
        t.copy_(a)
        return t
    return a


def save_u8(tensor, path):
    """Write an (h, w, 3) uint8 tensor (any device) as a PNG."""
    from PIL import Image
    t = _as_u8(tensor).cpu().contiguous()
    Image.fromarray(t.numpy()).save(path, format='PNG')


def _as_u8(im):
    """A list item of the u8 interfaces -> an (h, w, 3) uint8 tensor (PIL images and numpy arrays become CPU tensors)."""
    if isinstance(im, torch.Tensor):
        t = im
    elif isinstance(im, np.ndarray):
        t = torch.from_numpy(im)
    else:
        t = load_u8(im)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f'expected an (h, w, 3) uint8 image, got {t.dtype} {tuple(t.shape)}')
    return t


def _canvas(sizes, div):
    return (div * max(math.ceil(h / div) for h, _ in sizes), div * max(math.ceil(w / div) for _, w in sizes))


class U8Batch:
    """B uint8 images on one device that share a canvas (H, W) >= their own sizes: what CodecBase.compress_images hands to
    compress_batch as `u8=`, instead of a (B, 3, H, W) fp32 tensor.  `shape` is that tensor's shape; `fill(dst, start, n)` converts
    images start .. start + n straight into `dst` -- an (n, 3, H, W) fp32 view of an encode plan's input -- with one launch on the
    current stream."""

    def __init__(self, images, div, device):
        ts = [_as_u8(im) for im in images]
        if not ts:
            raise ValueError('no images')
        self.sizes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
        H, W = _canvas(self.sizes, div)
        self.shape = (len(ts), 3, H, W)
        self.device = torch.device(device)
        # 3 bytes per pixel cross the bus, unpadded; rows of a view may be strided, pixels are interleaved
        self.images = [t.to(self.device, non_blocking=True) if t.device != self.device else t for t in ts]
        self.images = [t if (t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * t.shape[1]) else t.contiguous() for t in self.images]

    def fill(self, dst, start=0, n=None):
        from .. import _native
        n = len(self.images) - start if n is None else n
        _, _, H, W = self.shape
        assert dst.dtype == torch.float32 and dst.device == self.device and tuple(dst.shape) == (n, 3, H, W) and dst[0].is_contiguous()
        ims, hw = self.images[start:start + n], self.sizes[start:start + n]
        src = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ims])
        rows = (ctypes.c_long * n)(*[t.stride(0) for t in ims])
        hw_arr = (ctypes.c_int * (2 * n))(*[v for p in hw for v in p])
        with torch.cuda.device(self.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _native.check(_native.lib().lvae_image_u8_to_f32(src, rows, hw_arr, n, dst.data_ptr(), dst.stride(0) if n > 1 else 3 * H * W, H, W, st),
                          'image_u8_to_f32')


def to_float01(u8_images, div=1, device=None):
    """A list of (h, w, 3) uint8 images (tensors on any device, numpy arrays, PIL images) -> ((B, 3, H, W) fp32 in [0, 1], [(h, w)]):
    v / 255, every image replicate-padded on the right / bottom to the common canvas, the smallest (H, W) of multiples of `div` that
    holds them all.  CPU inputs with device=None: `pil_to_tensor01(pad_divisible_by(img, div))` on the host.  Otherwise: one upload of
    each image's bytes (none for device tensors) and one kernel launch for the batch, on `device` (default: the images' device)."""
    ts = [_as_u8(im) for im in u8_images]
    if device is None and all(t.device.type == 'cpu' for t in ts):
        from PIL import Image
        sizes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
        H, W = _canvas(sizes, div)
        out = []
        for t, (h, w) in zip(ts, sizes):
            a = np.pad(t.numpy(), ((0, H - h), (0, W - w), (0, 0)), mode='edge') if (h, w) != (H, W) else t.numpy()
            out.append(coding.pil_to_tensor01(Image.fromarray(np.ascontiguousarray(a))))
        return torch.stack(out), sizes
    if device is None:
        device = next(t.device for t in ts if t.device.type != 'cpu')
    batch = U8Batch(ts, div, device)
    out = torch.empty(batch.shape, dtype=torch.float32, device=batch.device)
    batch.fill(out)
    return out, batch.sizes


def to_u8(x, sizes=None):
    """The inverse: fp32 images in [0, 1] -> a list of (h, w, 3) uint8 tensors on the same device, round(clamp(x, 0, 1) * 255) with ties
    to even (`torch.round(x * 255)` for x in [0, 1]); NaN -> 0 on the GPU.  x: a (B, 3, H, W) tensor or a list of (1, 3, h, w) / (3, h, w)
    tensors (crops of a decoder's padded batch are read in place); sizes: per-image valid extents [(h, w)] (default: every item whole).
    Device tensors: one kernel launch for the batch on the current stream; CPU tensors: the torch expression."""
    from .views import items, strided_batch
    xs = items(x, 'x')
    if sizes is not None:
        if len(sizes) != len(xs):
            raise ValueError(f'to_u8: {len(sizes)} sizes for {len(xs)} images')
        xs = [v[:, :h, :w] for v, (h, w) in zip(xs, sizes)]
    if not xs or any(v.shape[0] != 3 or v.shape[1] == 0 or v.shape[2] == 0 for v in xs):
        raise ValueError('to_u8: expected 3-channel, non-empty images')
    device = xs[0].device
    if device.type == 'cpu':
        return [torch.round(v.float().clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous() for v in xs]
    from .. import _native
    B = len(xs)
    hw = [(int(v.shape[1]), int(v.shape[2])) for v in xs]
    hmax, wmax = max(h for h, _ in hw), max(w for _, w in hw)
    with torch.cuda.device(device):
        keep, px, (s_img, s_plane, s_row) = strided_batch(xs, hmax, wmax, device)
        span = (hmax - 1) * s_row + wmax             # views whose common strides do not hold the largest extent are packed instead
        if s_row < wmax or s_plane < span or (B > 1 and s_img < 2 * s_plane + span):
            keep, px, (s_img, s_plane, s_row) = strided_batch([v.clone() for v in xs], hmax, wmax, device)
        outs = [torch.empty(h, w, 3, dtype=torch.uint8, device=device) for h, w in hw]
        dst = (ctypes.c_void_p * B)(*[t.data_ptr() for t in outs])
        rows = (ctypes.c_long * B)(*[3 * w for _, w in hw])
        hw_arr = (ctypes.c_int * (2 * B))(*[v for p in hw for v in p])
        # the canvas the strides are known to hold: the largest extent of the call
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _native.check(_native.lib().lvae_image_f32_to_u8(px, s_img if B > 1 else 3 * s_plane, s_plane, s_row, hmax, wmax, hw_arr, B, dst, rows, st),
                      'image_f32_to_u8')
    del keep
    return outs


def stitch_tiles(tiles, h, w, th, tw, overlap, box=None, out='u8', strides=None):
    """A window of an (h, w) image from the fp32 reconstructions of its tiles (grid and weights: lvae/utils/tiling.py), on the GPU
    (lvae_tile_stitch: one small copy and one launch on the current stream).  tiles: row-major list with one entry per tile of
    the grid (utils.tiling.axis_origins per axis) -- a (3, >= th', >= tw') fp32 device tensor with unit column stride, th' = min(th, rows the tile
    holds), all with the same plane and row strides (crops of a decoder's padded batch are read in place), or None for a tile that was
    not decoded (allowed where it does not meet the box).  box = (y0, x0, hh, ww), default the whole image.  -> (hh, ww, 3) uint8
    (out='u8': rint(clamp(v, 0, 1) * 255), ties to even) or (1, 3, hh, ww) fp32 (out='f32').  (th, tw) is the extent the tiles' buffers
    hold: for an image smaller than a tile along an axis, its padded size there."""
    from .. import _native
    from .tiling import axis_origins
    if out not in ('u8', 'f32'):
        raise ValueError(f"stitch_tiles: out is 'u8' or 'f32', got {out!r}")
    if min(h, w, th, tw) <= 0 or overlap < 0 or (h > th and overlap > th // 2) or (w > tw and overlap > tw // 2):
        raise ValueError(f'stitch_tiles: image {(h, w)}, tiles {(th, tw)}, overlap {overlap}')
    ys, xs = axis_origins(h, th, overlap), axis_origins(w, tw, overlap)
    if len(tiles) != len(ys) * len(xs):
        raise ValueError(f'stitch_tiles: {len(tiles)} tiles for a {len(ys)} x {len(xs)} grid')
    y0, x0, hh, ww = (0, 0, h, w) if box is None else (int(v) for v in box)
    have = [t for t in tiles if t is not None]
    if not have:
        raise ValueError('stitch_tiles: no decoded tile')
    t0 = have[0]
    device = t0.device
    for t in have:
        if (t.dtype != torch.float32 or t.device != device or t.dim() != 3 or t.shape[0] != 3 or t.stride(2) != 1
                or t.stride()[:2] != t0.stride()[:2]):
            raise ValueError('stitch_tiles: tiles are (3, th, tw) fp32 tensors on one device with unit column stride and common strides')
    lib = _native.lib()
    n = len(tiles)
    addr = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tiles])
    oy, ox = (ctypes.c_int * len(ys))(*ys), (ctypes.c_int * len(xs))(*xs)
    with torch.cuda.device(device):
        if out == 'u8':
            dst = torch.empty(hh, ww, 3, dtype=torch.uint8, device=device)
            d_plane, d_row = 0, 3 * ww
        else:
            dst = torch.empty(1, 3, hh, ww, dtype=torch.float32, device=device)
            d_plane, d_row = hh * ww, ww
        nbytes = lib.lvae_tile_stitch_workspace_bytes(len(ys), len(xs))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _native.check(lib.lvae_tile_stitch(addr, t0.stride(0), t0.stride(1), oy, ox, len(ys), len(xs), th, tw, overlap, h, w, y0, x0, hh, ww,
                                           dst.data_ptr(), d_plane, d_row, 1 if out == 'u8' else 0, ws.data_ptr(), nbytes, st), 'tile_stitch')
    return dst
