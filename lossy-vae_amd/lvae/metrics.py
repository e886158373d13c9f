"""Image-quality metrics: PSNR and MS-SSIM.

MS-SSIM is the form learned-compression evaluations use (Wang, Simoncelli, Bovik 2003): data range 1, K1 = 0.01, K2 = 0.03, an 11-tap
Gaussian window (sigma 1.5) as a valid correlation, 5 scales with weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), a 2x2 mean pool with
zero padding of size % 2 between them (avg_pool2d's defaults), per channel prod relu(cs_i)^w_i * relu(ssim_4)^w_4, mean over channels.
Defined for min(h, w) > 160 only.

CUDA tensors go through the HIP kernels (`lvae_msssim_f32`, csrc/metrics.hip: one fixed launch sequence for the whole batch, images of
different sizes included, read where they lie); CPU tensors through an fp64 torch evaluation of the same definition.
"""
import ctypes
import math

import torch
import torch.nn.functional as F

from .utils.views import items as _items, strided_batch as _strided_batch

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIDE = 161


def psnr(real, fake):
    """-10 log10(mean((real - fake)^2)) of one image pair in [0, 1], as a float."""
    mse = (real.double() - fake.double().to(real.device)).square().mean().item()
    return float(-10 * math.log10(mse))


PSNR_YUV_KEYS = ('mse-y', 'mse-u', 'mse-v', 'psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv')
PSNR_YUV_KEYS2 = PSNR_YUV_KEYS + ('psnr-avg',)


def _sse(pairs, dtype, entry, who):
    """sse_u8 / sse_u16: planes of `dtype` (torch.int16 is read as UNSIGNED 16-bit words); on a GPU ONE launch of `entry` for all pairs."""
    name = str(dtype).split('.')[-1]
    for a, b in pairs:
        if a.dtype != dtype or b.dtype != dtype or a.dim() != 2 or a.shape != b.shape or a.numel() == 0:
            raise ValueError(f'{who}: expected two equally shaped, non-empty 2-D {name} planes, got {tuple(a.shape)} and {tuple(b.shape)}')
    devs = {p.device for ab in pairs for p in ab if p.is_cuda}
    if len(devs) > 1:
        raise ValueError(f'{who}: planes on several GPUs {sorted(map(str, devs))}')
    if not devs:
        codes = lambda p: p.contiguous().numpy().view('uint8' if dtype == torch.uint8 else 'uint16').astype('int64')
        out = []
        for a, b in pairs:
            d = codes(a) - codes(b)
            out.append(int((d * d).sum()))
        return out
    from . import _native
    device, n = devs.pop(), len(pairs)
    plane = lambda p: (p if p.stride(1) == 1 and p.stride(0) >= p.shape[1] else p.contiguous())
    a = [plane(p.to(device, non_blocking=True)) for p, _ in pairs]
    b = [plane(p.to(device, non_blocking=True)) for _, p in pairs]
    ptr = lambda ps: (ctypes.c_void_p * n)(*[p.data_ptr() for p in ps])
    row = lambda ps: (ctypes.c_long * n)(*[p.stride(0) for p in ps])          # in samples
    hw = (ctypes.c_int * (2 * n))(*[int(v) for p in a for v in p.shape])
    out = torch.empty(n, dtype=torch.int64, device=device)            # (the sums stay far below 2^63: 65535^2 per sample at the most)
    with torch.cuda.device(device):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _native.check(getattr(_native.lib(), 'lvae_' + entry)(ptr(a), row(a), ptr(b), row(b), hw, n, out.data_ptr(), st), entry)
    return [int(v) for v in out.cpu().tolist()]


def sse_u8(pairs):
    """[(a, b)] pairs of equally shaped 2-D uint8 planes -> their sums of squared differences as Python ints, exact.  If a plane is on a
    GPU: ONE lvae_sse_u8 launch for all pairs on that device's current stream (integer arithmetic on the device, one 64-bit word per pair
    comes back; planes with unit column stride are read where they lie); CPU planes: numpy int64."""
    return _sse(pairs, torch.uint8, 'sse_u8', 'sse_u8')


def sse_u16(pairs):
    """sse_u8 for planes of 16-bit codes: [(a, b)] pairs of equally shaped 2-D torch.int16 planes, read as UNSIGNED 16-bit words -> their
    sums of squared differences as Python ints, exact for any 16-bit values.  If a plane is on a GPU: ONE lvae_sse_u16 launch for all pairs
    (64-bit integer sums on the device, one word per pair comes back); CPU planes: numpy int64."""
    return _sse(pairs, torch.int16, 'sse_u16', 'sse_u16')


def _psnr_rows(ref, rec, depth, keys):
    """Per frame pair the dict of `keys`; peak = 255 * 2^(depth - 8)."""
    sse = (sse_u8 if depth == 8 else sse_u16)([(getattr(a, p), getattr(b, p)) for a, b in zip(ref, rec) for p in 'yuv'])
    peak2 = (255.0 * (1 << (depth - 8))) ** 2
    db = lambda mse: float(10 * math.log10(peak2 / mse)) if mse > 0 else math.inf
    out = []
    for i, a in enumerate(ref):
        row, total, count = {}, 0, 0
        for j, p in enumerate('yuv'):
            mse = sse[3 * i + j] / float(getattr(a, p).numel())
            row['mse-' + p] = mse
            row['psnr-' + p] = db(mse)
            total, count = total + sse[3 * i + j], count + getattr(a, p).numel()
        row['psnr-yuv'] = (6 * row['psnr-y'] + row['psnr-u'] + row['psnr-v']) / 8
        row['psnr-avg'] = db(total / float(count))
        out.append({k: row[k] for k in keys})
    return out


def psnr_yuv420(ref_frames, rec_frames):
    """PSNR of 8-bit 4:2:0 frames (lists of utils.yuv.Yuv420Frame, or two frames) as video-side comparisons report it: per frame a dict
    {'mse-y', 'mse-u', 'mse-v', 'psnr-y', 'psnr-u', 'psnr-v', 'psnr-yuv'} of floats.  mse = the plane's exact sum of squared byte
    differences (sse_u8) / its sample count, in float64; psnr = 10 log10(255^2 / mse), inf for identical planes;
    psnr-yuv = (6 psnr-y + psnr-u + psnr-v) / 8, the weighting of the HM / VTM reference software for 4:2:0."""
    from .utils.yuv import Yuv420Frame
    if isinstance(ref_frames, Yuv420Frame):
        return psnr_yuv420([ref_frames], [rec_frames])[0]
    ref, rec = list(ref_frames), list(rec_frames)
    if len(ref) != len(rec) or not ref:
        raise ValueError(f'psnr_yuv420: {len(ref)} reference and {len(rec)} reconstructed frames')
    for i, (a, b) in enumerate(zip(ref, rec)):
        if a.size != b.size:
            raise ValueError(f'psnr_yuv420: frame {i} is {a.size} against {b.size}')
    return _psnr_rows(ref, rec, 8, PSNR_YUV_KEYS)


def psnr_yuv(ref_frames, rec_frames):
    """PSNR of utils.yuv.YuvFrame / YuvSpFrame lists (or two frames) of any depth and subsampling: per frame a dict {'mse-y', 'mse-u', 'mse-v', 'psnr-y',
    'psnr-u', 'psnr-v', 'psnr-yuv', 'psnr-avg'} of floats.  mse = the plane's exact sum of squared code differences (sse_u8 / sse_u16) / its
    sample count, in float64; psnr = 10 log10(peak^2 / mse), inf for identical planes, with peak = 255 * 2^(depth - 8) -- 1020 at 10 bits,
    4080 at 12: the convention of the HM / VTM reference software, NOT 2^depth - 1.  psnr-yuv = (6 psnr-y + psnr-u + psnr-v) / 8, HM's
    weighting for 4:2:0; psnr-avg is the PSNR of the pooled error, (sse-y + sse-u + sse-v) / (all three sample counts): the meaningful single
    number for 4:2:2 and 4:4:4, where 6:1:1 does not reflect the sample counts."""
    from .utils.yuv import YuvFrame, YuvSpFrame
    if isinstance(ref_frames, (YuvFrame, YuvSpFrame)):
        return psnr_yuv([ref_frames], [rec_frames])[0]
    planar = lambda f: f.to_planar() if isinstance(f, YuvSpFrame) else f       # semi-planar (P010 ...) frames: compared as their codes
    ref, rec = [planar(f) for f in ref_frames], [planar(f) for f in rec_frames]
    if len(ref) != len(rec) or not ref:
        raise ValueError(f'psnr_yuv: {len(ref)} reference and {len(rec)} reconstructed frames')
    for i, (a, b) in enumerate(zip(ref, rec)):
        if (a.size, a.depth, a.subsampling) != (b.size, b.depth, b.subsampling):
            raise ValueError(f'psnr_yuv: frame {i} is {a.size} {a.depth}-bit {a.subsampling} against {b.size} {b.depth}-bit {b.subsampling}')
    if any(a.depth != ref[0].depth for a in ref):
        raise ValueError('psnr_yuv: the frames of one call share a depth')
    return _psnr_rows(ref, rec, ref[0].depth, PSNR_YUV_KEYS2)


def ms_ssim_db(v):
    """MS-SSIM on the decibel scale result tables use: -10 log10(1 - v)."""
    if torch.is_tensor(v):
        return -10 * torch.log10(1 - v)
    return float(-10 * math.log10(1 - v))


def _gauss():
    c = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 * 1.5))
    return g / g.sum()


def _filt(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def _ms_ssim_cpu(x, y):
    """(B, C, h, w) pairs, everything in fp64 -> ((B,) values, (B, 5, C) per-scale means before the relu)."""
    x, y, g = x.double(), y.double(), _gauss()
    C1, C2 = 1e-4, 9e-4
    raw = []
    for i in range(5):
        mx, my = _filt(x, g), _filt(y, g)
        sxx, syy, sxy = _filt(x * x, g) - mx * mx, _filt(y * y, g) - my * my, _filt(x * y, g) - mx * my
        cs = (2 * sxy + C2) / (sxx + syy + C2)
        if i < 4:
            raw.append(cs.flatten(2).mean(-1))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
        else:
            raw.append((((2 * mx * my + C1) / (mx * mx + my * my + C1)) * cs).flatten(2).mean(-1))
    m = torch.stack(raw, 1)                                                              # (B, 5, C)
    w = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64).view(1, -1, 1)
    return torch.prod(torch.relu(m) ** w, 1).mean(1), m


def _ms_ssim_hip(xs, ys, device):
    from . import _native
    B, C = len(xs), xs[0].shape[0]
    hw = [(int(v.shape[1]), int(v.shape[2])) for v in xs]
    hmax, wmax = max(h for h, _ in hw), max(w for _, w in hw)
    L = _native.lib()
    with torch.cuda.device(device):                  # the launches go to the current stream of the tensors' device
        keep_x, px, sx = _strided_batch(xs, hmax, wmax, device)
        keep_y, py, sy = _strided_batch(ys, hmax, wmax, device)
        nbytes = int(L.lvae_msssim_workspace_bytes(B, C, hmax, wmax))
        if nbytes == 0:
            raise ValueError(f'ms_ssim: unsupported batch B={B} C={C} {hmax}x{wmax}')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        out = torch.empty(B, dtype=torch.float64, device=device)
        means = torch.empty(B, 5, C, dtype=torch.float64, device=device)
        hw_arr = (ctypes.c_int * (2 * B))(*[v for p in hw for v in p])
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _native.check(L.lvae_msssim_f32(px, *sx, py, *sy, hw_arr, B, C, hmax, wmax, out.data_ptr(), means.data_ptr(), ws.data_ptr(), nbytes, st),
                      'msssim')
    del keep_x, keep_y
    return out, means


def ms_ssim(real, fake, sizes=None, return_scales=False):
    """MS-SSIM of B image pairs in [0, 1]: a float64 tensor of B values (on the inputs' device).

    real, fake: (B, C, H, W) float tensors, or lists of (1, C, h, w) / (C, h, w) tensors whose sizes may differ from image to image; list
    items may be views (crops of a padded batch are read in place).  sizes: per-image valid extents [(h, w), ...] inside padded tensors
    (default: every item whole).  If either side is on a GPU the HIP kernels run there, on that device's current stream; two CPU inputs
    take the fp64 torch path.  return_scales: also return the (B, 5, C) per-scale means (cs of scales 0..3, ssim of scale 4, before
    the relu).  ValueError for mismatched shapes and for an image with min(h, w) <= 160."""
    xs, ys = _items(real, 'real'), _items(fake, 'fake')
    if len(xs) != len(ys) or not xs:
        raise ValueError(f'ms_ssim: {len(xs)} real and {len(ys)} fake images')
    if sizes is not None:
        if len(sizes) != len(xs):
            raise ValueError(f'ms_ssim: {len(sizes)} sizes for {len(xs)} images')
        for i, (h, w) in enumerate(sizes):
            if h > min(xs[i].shape[1], ys[i].shape[1]) or w > min(xs[i].shape[2], ys[i].shape[2]) or h <= 0 or w <= 0:
                raise ValueError(f'ms_ssim: size {h}x{w} of image {i} exceeds its tensors {tuple(xs[i].shape)} / {tuple(ys[i].shape)}')
        xs = [v[:, :h, :w] for v, (h, w) in zip(xs, sizes)]
        ys = [v[:, :h, :w] for v, (h, w) in zip(ys, sizes)]
    C = xs[0].shape[0]
    for i, (a, b) in enumerate(zip(xs, ys)):
        if a.shape != b.shape or a.shape[0] != C:
            raise ValueError(f'ms_ssim: image {i} has shapes {tuple(a.shape)} and {tuple(b.shape)} (channels of image 0: {C})')
        if not (a.is_floating_point() and b.is_floating_point()):
            raise ValueError(f'ms_ssim: image {i} is not a float tensor in [0, 1]')
        if min(a.shape[1:]) < MS_SSIM_MIN_SIDE:
            raise ValueError(f'ms_ssim: image {i} is {a.shape[1]}x{a.shape[2]}; MS-SSIM needs min(h, w) > 160 (5 scales of an 11-tap window)')
    devs = {v.device for v in xs + ys if v.is_cuda}
    if len(devs) > 1:
        raise ValueError(f'ms_ssim: inputs on several GPUs {sorted(map(str, devs))}')
    if devs:
        out, means = _ms_ssim_hip(xs, ys, devs.pop())
        return (out, means) if return_scales else out
    vals, means = [], []
    for a, b in zip(xs, ys):                       # per image: sizes may differ, and a value does not depend on the rest of the batch
        v, m = _ms_ssim_cpu(a.unsqueeze(0), b.unsqueeze(0))
        vals.append(v)
        means.append(m)
    out = torch.cat(vals)
    return (out, torch.cat(means)) if return_scales else out
