"""Image-quality metrics: PSNR, SSIM and MS-SSIM, on RGB tensors and on the planes of YUV frames.

MS-SSIM is the form learned-compression evaluations use (Wang, Simoncelli, Bovik 2003): data range 1, K1 = 0.01, K2 = 0.03, an 11-tap
Gaussian window (sigma 1.5) as a valid correlation, 5 scales with weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), a 2x2 mean pool with
zero padding of size % 2 between them (avg_pool2d's defaults), per channel prod relu(cs_i)^w_i * relu(ssim_4)^w_4, mean over channels.
Defined for min(h, w) > 160 only.

CUDA tensors go through the HIP kernels (`lvae_msssim_f32`, csrc/metrics.hip: one fixed launch sequence for the whole batch, images of
different sizes included, read where they lie); CPU tensors through an fp64 torch evaluation of the same definition.

`ssim` is scale 0 of that definition on its own (min(h, w) >= 11).  `ssim_yuv` / `ms_ssim_yuv` evaluate both on the integer planes of video
frames (utils.yuv) in code units, through `lvae_msssim_planes`: the same kernels behind loaders for bytes and 16-bit words.
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


def _ssim_maps(x, y, g, C1, C2):
    """(ssim map, cs map) of (B, C, h, w) fp64 pairs: the valid (h - 10, w - 10) pixels of the 11-tap window."""
    mx, my = _filt(x, g), _filt(y, g)
    sxx, syy, sxy = _filt(x * x, g) - mx * mx, _filt(y * y, g) - my * my, _filt(x * y, g) - mx * my
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    return ((2 * mx * my + C1) / (mx * mx + my * my + C1)) * cs, cs


def _ms_ssim_cpu(x, y, C1=1e-4, C2=9e-4):
    """(B, C, h, w) pairs, everything in fp64 -> ((B,) values, (B, 5, C) per-scale means before the relu).  C1, C2: (0.01 L)^2 and
    (0.03 L)^2 for samples of data range L."""
    x, y, g = x.double(), y.double(), _gauss()
    raw = []
    for i in range(5):
        ss, cs = _ssim_maps(x, y, g, C1, C2)
        if i < 4:
            raw.append(cs.flatten(2).mean(-1))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
        else:
            raw.append(ss.flatten(2).mean(-1))
    m = torch.stack(raw, 1)                                                              # (B, 5, C)
    w = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64).view(1, -1, 1)
    return torch.prod(torch.relu(m) ** w, 1).mean(1), m


def _ssim_cpu(x, y, C1=1e-4, C2=9e-4):
    """(B, C, h, w) pairs in fp64 -> (B, C) means of the SSIM map."""
    return _ssim_maps(x.double(), y.double(), _gauss(), C1, C2)[0].flatten(2).mean(-1)


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


def _image_pairs(real, fake, sizes, who, min_side, why):
    """The prelude of ms_ssim / ssim: the two inputs as lists of (C, h, w) views cut to `sizes`, checked."""
    xs, ys = _items(real, 'real'), _items(fake, 'fake')
    if len(xs) != len(ys) or not xs:
        raise ValueError(f'{who}: {len(xs)} real and {len(ys)} fake images')
    if sizes is not None:
        if len(sizes) != len(xs):
            raise ValueError(f'{who}: {len(sizes)} sizes for {len(xs)} images')
        for i, (h, w) in enumerate(sizes):
            if h > min(xs[i].shape[1], ys[i].shape[1]) or w > min(xs[i].shape[2], ys[i].shape[2]) or h <= 0 or w <= 0:
                raise ValueError(f'{who}: size {h}x{w} of image {i} exceeds its tensors {tuple(xs[i].shape)} / {tuple(ys[i].shape)}')
        xs = [v[:, :h, :w] for v, (h, w) in zip(xs, sizes)]
        ys = [v[:, :h, :w] for v, (h, w) in zip(ys, sizes)]
    C = xs[0].shape[0]
    for i, (a, b) in enumerate(zip(xs, ys)):
        if a.shape != b.shape or a.shape[0] != C:
            raise ValueError(f'{who}: image {i} has shapes {tuple(a.shape)} and {tuple(b.shape)} (channels of image 0: {C})')
        if not (a.is_floating_point() and b.is_floating_point()):
            raise ValueError(f'{who}: image {i} is not a float tensor in [0, 1]')
        if min(a.shape[1:]) < min_side:
            raise ValueError(f'{who}: image {i} is {a.shape[1]}x{a.shape[2]}; {why}')
    devs = {v.device for v in xs + ys if v.is_cuda}
    if len(devs) > 1:
        raise ValueError(f'{who}: inputs on several GPUs {sorted(map(str, devs))}')
    return xs, ys, (devs.pop() if devs else None)


def ms_ssim(real, fake, sizes=None, return_scales=False):
    """MS-SSIM of B image pairs in [0, 1]: a float64 tensor of B values (on the inputs' device).

    real, fake: (B, C, H, W) float tensors, or lists of (1, C, h, w) / (C, h, w) tensors whose sizes may differ from image to image; list
    items may be views (crops of a padded batch are read in place).  sizes: per-image valid extents [(h, w), ...] inside padded tensors
    (default: every item whole).  If either side is on a GPU the HIP kernels run there, on that device's current stream; two CPU inputs
    take the fp64 torch path.  return_scales: also return the (B, 5, C) per-scale means (cs of scales 0..3, ssim of scale 4, before
    the relu).  ValueError for mismatched shapes and for an image with min(h, w) <= 160."""
    xs, ys, device = _image_pairs(real, fake, sizes, 'ms_ssim', MS_SSIM_MIN_SIDE, 'MS-SSIM needs min(h, w) > 160 (5 scales of an 11-tap window)')
    if device is not None:
        out, means = _ms_ssim_hip(xs, ys, device)
        return (out, means) if return_scales else out
    vals, means = [], []
    for a, b in zip(xs, ys):                       # per image: sizes may differ, and a value does not depend on the rest of the batch
        v, m = _ms_ssim_cpu(a.unsqueeze(0), b.unsqueeze(0))
        vals.append(v)
        means.append(m)
    out = torch.cat(vals)
    return (out, torch.cat(means)) if return_scales else out


# ----------------------------------------------------------------------------------------------- planes: SSIM, and YUV frames
SSIM_MIN_SIDE = 11


def _planes_hip(xs, ys, kind, depth, data_range, scales, device):
    """lvae_msssim_planes: n pairs of 2-D planes of one sample kind -> ((n,) values, (n, scales) per-scale means), float64 on `device`.
    ONE call for all pairs, on the device's current stream.  A plane is read where it lies if its pixels are 1 or 2 samples apart and its
    rows do not overlap (any row stride: views into larger tensors, one half of an interleaved chroma plane); anything else is copied."""
    from . import _native
    n = len(xs)
    lies = lambda p: p.stride(1) in (1, 2) and p.stride(0) >= p.shape[1] * p.stride(1)
    dense = lambda p: p if lies(p) and p.stride(1) == 1 else p.contiguous()
    with torch.cuda.device(device):
        xs = [p.to(device, non_blocking=True) for p in xs]
        ys = [p.to(device, non_blocking=True) for p in ys]
        for k, (a, b) in enumerate(zip(xs, ys)):              # a pair shares its pixel stride
            if not (lies(a) and lies(b) and a.stride(1) == b.stride(1)):
                xs[k], ys[k] = dense(a), dense(b)
        hw = [(int(p.shape[0]), int(p.shape[1])) for p in xs]
        hmax, wmax = max(h for h, _ in hw), max(w for _, w in hw)
        L = _native.lib()
        nbytes = int(L.lvae_msssim_planes_workspace_bytes(n, hmax, wmax, scales))
        if nbytes == 0:
            raise ValueError(f'unsupported planes: n={n}, {hmax}x{wmax}, {scales} scales')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        out = torch.empty(n, dtype=torch.float64, device=device)
        means = torch.empty(n, scales, dtype=torch.float64, device=device)
        ptr = lambda ps: (ctypes.c_void_p * n)(*[p.data_ptr() for p in ps])
        row = lambda ps: (ctypes.c_long * n)(*[p.stride(0) for p in ps])
        hw_arr = (ctypes.c_int * (2 * n))(*[v for p in hw for v in p])
        pix = (ctypes.c_int * n)(*[p.stride(1) for p in xs])
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _native.check(L.lvae_msssim_planes(ptr(xs), row(xs), ptr(ys), row(ys), hw_arr, pix, n, _native.SAMPLE_KINDS.index(kind), depth,
                                           float(data_range), scales, out.data_ptr(), means.data_ptr(), ws.data_ptr(), nbytes, st), 'msssim_planes')
    del xs, ys
    return out, means


def ssim(real, fake, sizes=None):
    """Single-scale SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) of B image pairs in [0, 1]: a float64 tensor of B values (on the inputs'
    device), per image the channel mean of the mean SSIM map -- data range 1, K1 = 0.01, K2 = 0.03, the 11-tap Gaussian window (sigma 1.5)
    as a valid correlation: scale 0 of ms_ssim, with the luminance term.  real, fake, sizes: as in ms_ssim.  Defined for min(h, w) >= 11.
    If either side is on a GPU: ONE lvae_msssim_planes call (fp32 samples, one scale) for all channels of all images, read where they lie;
    two CPU inputs take the fp64 torch path."""
    xs, ys, device = _image_pairs(real, fake, sizes, 'ssim', SSIM_MIN_SIDE, 'SSIM needs min(h, w) >= 11 (one 11-tap window)')
    if device is not None:
        C = xs[0].shape[0]
        f32 = lambda v: v if v.dtype == torch.float32 else v.float()
        out, _ = _planes_hip([c for v in xs for c in f32(v)], [c for v in ys for c in f32(v)], 'f32', 8, 1.0, 1, device)
        return out.view(len(xs), C).mean(1)
    return torch.cat([_ssim_cpu(a.unsqueeze(0), b.unsqueeze(0)).mean(1) for a, b in zip(xs, ys)])


def _frame_planes(f):
    """A video frame's sample kind, depth and planes {'y', 'u', 'v'} as 2-D views (the chroma of NV12 / P010 frames: every other sample of
    the interleaved plane)."""
    from .utils.yuv import Yuv420Frame, YuvFrame, YuvSpFrame
    if isinstance(f, Yuv420Frame):
        return 'u8', 8, {'y': f.y, 'u': f.u, 'v': f.v}
    if isinstance(f, YuvFrame):
        return ('u8' if f.depth == 8 else 'u16_low'), f.depth, {'y': f.y, 'u': f.u, 'v': f.v}
    if isinstance(f, YuvSpFrame):
        return 'u16_high', f.depth, {'y': f.y, 'u': f.uv[:, 0::2], 'v': f.uv[:, 1::2]}
    raise ValueError(f'expected a Yuv420Frame, YuvFrame or YuvSpFrame, got {type(f).__name__}')


def _codes_f64(p, kind, depth):
    """A plane's codes as fp64, as the kernels read them: low-bit words masked to `depth` bits, high-bit words shifted down."""
    if kind == 'u8':
        return p.double()
    w = p.to(torch.int32) & 0xffff
    return ((w & ((1 << depth) - 1)) if kind == 'u16_low' else (w >> (16 - depth))).double()


def _yuv_structural(who, key, scales, ref, rec, planes, data_range, return_scales=False):
    """ssim_yuv / ms_ssim_yuv: per frame {key-<plane>: float} for the planes asked for."""
    single = not isinstance(ref, (list, tuple))
    ref, rec = ([ref], [rec]) if single else (list(ref), list(rec))
    if planes not in ('y', 'yuv'):
        raise ValueError(f"{who}: planes is 'y' or 'yuv', got {planes!r}")
    if len(ref) != len(rec) or not ref:
        raise ValueError(f'{who}: {len(ref)} reference and {len(rec)} reconstructed frames')
    min_side = SSIM_MIN_SIDE if scales == 1 else MS_SSIM_MIN_SIDE
    xs, ys, kinds = [], [], set()
    for i, (a, b) in enumerate(zip(ref, rec)):
        (ka, da, pa), (kb, db, pb) = _frame_planes(a), _frame_planes(b)
        if (ka, da) != (kb, db):
            raise ValueError(f'{who}: frame {i} holds {da}-bit {ka} samples against {db}-bit {kb} samples')
        kinds.add((ka, da))
        for name in planes:
            if pa[name].shape != pb[name].shape:
                raise ValueError(f'{who}: plane {name} of frame {i} is {tuple(pa[name].shape)} against {tuple(pb[name].shape)}')
            h, w = (int(v) for v in pa[name].shape)
            if min(h, w) < min_side:
                raise ValueError(f'{who}: plane {name} of frame {i} is {h}x{w}; ' + ('SSIM needs min(h, w) >= 11 (one 11-tap window)' if scales == 1 else
                                 'MS-SSIM needs min(h, w) > 160 (5 scales of an 11-tap window)'))
            xs.append(pa[name])
            ys.append(pb[name])
    if len(kinds) > 1:
        raise ValueError(f'{who}: the frames of one call share sample kind and depth, got {sorted(kinds)}')
    kind, depth = kinds.pop()
    L = float((1 << depth) - 1) if data_range is None else float(data_range)
    if not L > 0:
        raise ValueError(f'{who}: data_range is positive, got {data_range!r}')
    devs = {p.device for p in xs + ys if p.is_cuda}
    if len(devs) > 1:
        raise ValueError(f'{who}: frames on several GPUs {sorted(map(str, devs))}')
    if devs:
        out, means = _planes_hip(xs, ys, kind, depth, L, scales, devs.pop())
        out, means = out.cpu(), means.cpu()
    else:
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        vals, ms = [], []
        for a, b in zip(xs, ys):
            a, b = _codes_f64(a, kind, depth)[None, None], _codes_f64(b, kind, depth)[None, None]
            if scales == 1:
                v = _ssim_cpu(a, b, C1, C2).view(1)
                m = v.view(1, 1)
            else:
                v, m = _ms_ssim_cpu(a, b, C1, C2)
                m = m.view(1, 5)
            vals.append(v)
            ms.append(m)
        out, means = torch.cat(vals), torch.cat(ms)
    k, flat = len(planes), out.tolist()
    rows = [{f'{key}-{name}': float(flat[i * k + j]) for j, name in enumerate(planes)} for i in range(len(ref))]
    res = rows[0] if single else rows
    if return_scales:
        means = means.view(len(ref), k, scales)
        return res, (means[0] if single else means)
    return res


def ssim_yuv(ref_frames, rec_frames, planes='yuv', data_range=None):
    """Single-scale SSIM (the definition of `ssim`) on the planes of video frames: lists (or two frames) of utils.yuv.Yuv420Frame,
    YuvFrame or YuvSpFrame -> per frame a dict {'ssim-y', 'ssim-u', 'ssim-v'} of floats ('ssim-y' alone with planes='y'), computed on the
    CODES: no plane is converted or divided by anything, C1 = (0.01 L)^2 and C2 = (0.03 L)^2 carry the data range L.
    data_range=None: L = 2^depth - 1, the dynamic range of the codes -- SSIM's definition of L.  psnr_yuv uses the HM / VTM peak
    255 * 2^(depth - 8) instead (1020, not 1023, at 10 bits); data_range=255 * 2**(depth - 8) selects that convention here.  At depth 8
    they coincide; above it the choice moves a value by up to ~2e-4.
    The frames of one call share sample kind and depth (ref and rec frame by frame too); sizes may differ from frame to frame.  Every plane
    has min(h, w) >= 11.  Frames on a GPU: ONE lvae_msssim_planes call for all planes of all frames, read where they lie -- any row stride,
    the chroma of NV12 / P010 frames inside the interleaved plane, no to_planar(), no float copy; one small tensor comes back.  CPU
    frames: the fp64 torch path on the codes."""
    return _yuv_structural('ssim_yuv', 'ssim', 1, ref_frames, rec_frames, planes, data_range)


def ms_ssim_yuv(ref_frames, rec_frames, planes='y', data_range=None, return_scales=False):
    """MS-SSIM (the definition of `ms_ssim`) on the planes of video frames, with the inputs, the data range and the paths of ssim_yuv ->
    per frame {'ms-ssim-y'}, and 'ms-ssim-u' / 'ms-ssim-v' with planes='yuv'.  A plane with min(h, w) <= 160 raises ValueError naming the
    plane and its size -- the 4:2:0 chroma of every frame up to 320x320 is such a plane, which is why luma alone is the default.
    return_scales: also return the per-scale means, a float64 tensor (frames, planes, 5) ((planes, 5) for two single frames)."""
    return _yuv_structural('ms_ssim_yuv', 'ms-ssim', 5, ref_frames, rec_frames, planes, data_range, return_scales)
