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


# ---- the resampler of reduced-resolution coding (lvae/utils/resample.py: the definition; csrc/resample.hip: the kernels)
_AXIS_TABLES = {}


def _axis_on_device(n_in, n_out, filter, device):
    """One axis of a resampling call as the native entries take it: (start pointer, weights pointer, taps, span of a 16-row tile),
    all 0 / None for an axis that keeps its size.  The device tables are built once per (n_in, n_out, filter, device) and kept."""
    from . import resample
    resample.check_ratio(n_in, n_out)
    if n_in == n_out:
        resample._filter(filter)
        return None, None, 0, 0
    key = (int(n_in), int(n_out), filter, str(device))
    hit = _AXIS_TABLES.get(key)
    if hit is None:
        start, wgt = resample.axis_table(n_in, n_out, filter)
        span = resample.tile_span(start, wgt.shape[1], n_in)
        hit = _AXIS_TABLES[key] = (torch.from_numpy(start).to(device), torch.from_numpy(wgt).contiguous().to(device), int(wgt.shape[1]), span)
    return hit[0].data_ptr(), hit[1].data_ptr(), hit[2], hit[3]


def _tables(h_in, w_in, h_out, w_out, filter, device):
    """The seven table arguments of lvae_resample_*: ystart, ywgt, ytaps, yspan, xstart, xwgt, xtaps."""
    return _axis_on_device(h_in, h_out, filter, device) + _axis_on_device(w_in, w_out, filter, device)[:3]


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _u8_descriptors(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), (ctypes.c_long * len(ts))(*[t.stride(0) for t in ts])


def _resample_f32(xs, size, filter, clamp, out, canvas=None):
    """A list of (3, h, w) fp32 device views of ONE size -> resized to `size`: out='f32': a (B, 3, H, W) tensor (canvas (H, W) >= size,
    replicate-padded; default: size itself); out='u8': a list of (h, w, 3) uint8 tensors.  Views cut from one tensor with common
    strides (crops of a decoder's padded batch) are read in place."""
    from .. import _native
    from .views import strided_batch
    device = xs[0].device
    B, (h_in, w_in), (h_out, w_out) = len(xs), (int(xs[0].shape[1]), int(xs[0].shape[2])), (int(size[0]), int(size[1]))
    tabs = _tables(h_in, w_in, h_out, w_out, filter, device)
    lib = _native.lib()
    with torch.cuda.device(device):
        keep, px, (s_img, s_plane, s_row) = strided_batch(xs, h_in, w_in, device)
        span = (h_in - 1) * s_row + w_in
        if B > 1 and s_img < 2 * s_plane + span:         # views that overlap as a batch are packed instead
            keep, px, (s_img, s_plane, s_row) = strided_batch([v.clone() for v in xs], h_in, w_in, device)
        s_img = s_img if B > 1 else 3 * s_plane
        if out == 'u8':
            outs = [torch.empty(h_out, w_out, 3, dtype=torch.uint8, device=device) for _ in range(B)]
            dst, rows = _u8_descriptors(outs)
            _native.check(lib.lvae_resample_f32_to_u8(px, s_img, s_plane, s_row, B, h_in, w_in, h_out, w_out, *tabs, dst, rows, _stream(device)),
                          'resample_f32_to_u8')
        else:
            H, W = (h_out, w_out) if canvas is None else canvas
            outs = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
            _native.check(lib.lvae_resample_f32(px, s_img, s_plane, s_row, B, h_in, w_in, h_out, w_out, *tabs, int(bool(clamp)), outs.data_ptr(),
                                                3 * H * W, H, W, _stream(device)), 'resample_f32')
    del keep
    return outs


class ScaledU8Batch(U8Batch):
    """B uint8 images of ONE size on one device, coded at `coded` = (h, w): what CodecBase.compress_scaled hands to compress_batch as `u8=`.
    `sizes` are the coded sizes (what the models' containers record), `shape` the coded canvas; `fill` resamples images start .. start + n
    straight into an encode plan's input -- v / 255, `filter`, clamped to [0, 1], replicate-padded -- with one launch
    (lvae_resample_u8_to_f32).  With coded == the images' size that is lvae_image_u8_to_f32's result, bit for bit."""

    def __init__(self, images, coded, filter, div, device):
        ts = [_as_u8(im) for im in images]
        if not ts:
            raise ValueError('no images')
        self.src_size = (int(ts[0].shape[0]), int(ts[0].shape[1]))
        if any((int(t.shape[0]), int(t.shape[1])) != self.src_size for t in ts):
            raise ValueError('the images of one scaled call share one size')
        super().__init__(ts, 1, device)
        self.filter = filter
        self.sizes = [(int(coded[0]), int(coded[1]))] * len(ts)
        self.shape = (len(ts), 3) + _canvas(self.sizes, div)
        self._tabs = _tables(*self.src_size, *self.sizes[0], filter, self.device)

    def fill(self, dst, start=0, n=None):
        from .. import _native
        n = len(self.images) - start if n is None else n
        _, _, H, W = self.shape
        assert dst.dtype == torch.float32 and dst.device == self.device and tuple(dst.shape) == (n, 3, H, W) and dst[0].is_contiguous()
        src, rows = _u8_descriptors(self.images[start:start + n])
        with torch.cuda.device(self.device):
            _native.check(_native.lib().lvae_resample_u8_to_f32(src, rows, n, *self.src_size, *self.sizes[0], *self._tabs, dst.data_ptr(),
                                                                dst.stride(0) if n > 1 else 3 * H * W, H, W, _stream(self.device)),
                          'resample_u8_to_f32')


def resize(x, size, filter='lanczos3', clamp=False, out='f32', device=None):
    """Resize images to size = (h, w) with the separable, antialiased resampler lvae/utils/resample.py defines (filter: 'bilinear' |
    'bicubic' | 'lanczos3'; pixel-centre alignment; an axis that keeps its size is copied, not filtered).  x: a (B, 3, h, w) fp32 tensor,
    or a list of (h, w, 3) uint8 images of ONE size (v / 255 first).  clamp: clamp the result to [0, 1] (bicubic and Lanczos overshoot).
    -> out='f32': a (B, 3, H, W) fp32 tensor; out='u8': a list of (H, W, 3) uint8 tensors, rint(clamp(v, 0, 1) * 255), ties to even.
    Inputs on a GPU (or `device`) run the kernels of csrc/resample.hip, one launch per 16 images on the current stream; CPU inputs take
    resample.resize_reference (fp64) cast to fp32.  ValueError: an unknown filter or out, a ratio outside [1/8, 8] on an axis."""
    from . import resample
    if out not in ('u8', 'f32'):
        raise ValueError(f"resize: out is 'u8' or 'f32', got {out!r}")
    resample._filter(filter)
    h, w = (int(v) for v in size)
    u8_in = not torch.is_tensor(x)
    if u8_in:
        ts = [_as_u8(im) for im in x]
        if not ts or any(t.shape != ts[0].shape for t in ts):
            raise ValueError('resize: a list holds (h, w, 3) uint8 images of one size')
        h_in, w_in = int(ts[0].shape[0]), int(ts[0].shape[1])
        if device is None:
            device = next((t.device for t in ts if t.device.type != 'cpu'), torch.device('cpu'))
    else:
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or x.shape[0] == 0:
            raise ValueError(f'resize: expected a (B, 3, h, w) fp32 tensor, got {x.dtype} {tuple(x.shape)}')
        h_in, w_in = int(x.shape[2]), int(x.shape[3])
        device = x.device if device is None else device
    device = torch.device(device)
    resample.check_ratio(h_in, h)
    resample.check_ratio(w_in, w)
    if device.type == 'cpu':
        x01 = to_float01(ts)[0] if u8_in else x
        y = torch.from_numpy(resample.resize_reference(x01.numpy(), h, w, filter, clamp=clamp).astype(np.float32))
        return y if out == 'f32' else to_u8(y)
    if u8_in and out == 'f32' and clamp:                 # the encoder's path: bytes in, one launch
        batch = ScaledU8Batch(ts, (h, w), filter, 1, device)
        y = torch.empty(batch.shape, dtype=torch.float32, device=device)
        batch.fill(y)
        return y
    x01 = to_float01(ts, device=device)[0] if u8_in else x.to(device)
    if x01.stride(3) != 1:
        x01 = x01.contiguous()
    return _resample_f32([x01[i] for i in range(x01.shape[0])], (h, w), filter, clamp, out)


def _stitch_args(tiles, h, w, th, tw, overlap, box, who):
    """The tile side of a stitch call, checked: -> (ys, xs, box as ints, the first decoded tile, and the host arrays of the native entries:
    tile addresses, row origins, column origins)."""
    from .tiling import axis_origins
    if min(h, w, th, tw) <= 0 or overlap < 0 or (h > th and overlap > th // 2) or (w > tw and overlap > tw // 2):
        raise ValueError(f'{who}: image {(h, w)}, tiles {(th, tw)}, overlap {overlap}')
    ys, xs = axis_origins(h, th, overlap), axis_origins(w, tw, overlap)
    if len(tiles) != len(ys) * len(xs):
        raise ValueError(f'{who}: {len(tiles)} tiles for a {len(ys)} x {len(xs)} grid')
    box = (0, 0, h, w) if box is None else tuple(int(v) for v in box)
    have = [t for t in tiles if t is not None]
    if not have:
        raise ValueError(f'{who}: no decoded tile')
    t0 = have[0]
    for t in have:
        if (t.dtype != torch.float32 or t.device != t0.device or t.dim() != 3 or t.shape[0] != 3 or t.stride(2) != 1
                or t.stride()[:2] != t0.stride()[:2]):
            raise ValueError(f'{who}: tiles are (3, th, tw) fp32 tensors on one device with unit column stride and common strides')
    addr = (ctypes.c_void_p * len(tiles))(*[None if t is None else t.data_ptr() for t in tiles])
    return ys, xs, box, t0, addr, (ctypes.c_int * len(ys))(*ys), (ctypes.c_int * len(xs))(*xs)


def stitch_tiles(tiles, h, w, th, tw, overlap, box=None, out='u8', strides=None):
    """A window of an (h, w) image from the fp32 reconstructions of its tiles (grid and weights: lvae/utils/tiling.py), on the GPU
    (lvae_tile_stitch: one small copy and one launch on the current stream).  tiles: row-major list with one entry per tile of
    the grid (utils.tiling.axis_origins per axis) -- a (3, >= th', >= tw') fp32 device tensor with unit column stride, th' = min(th, rows the tile
    holds), all with the same plane and row strides (crops of a decoder's padded batch are read in place), or None for a tile that was
    not decoded (allowed where it does not meet the box).  box = (y0, x0, hh, ww), default the whole image.  -> (hh, ww, 3) uint8
    (out='u8': rint(clamp(v, 0, 1) * 255), ties to even) or (1, 3, hh, ww) fp32 (out='f32').  (th, tw) is the extent the tiles' buffers
    hold: for an image smaller than a tile along an axis, its padded size there."""
    from .. import _native
    if out not in ('u8', 'f32'):
        raise ValueError(f"stitch_tiles: out is 'u8' or 'f32', got {out!r}")
    ys, xs, (y0, x0, hh, ww), t0, addr, oy, ox = _stitch_args(tiles, h, w, th, tw, overlap, box, 'stitch_tiles')
    device = t0.device
    lib = _native.lib()
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
