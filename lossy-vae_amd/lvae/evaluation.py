"""Evaluation harness: drop-in for the reference's `imcoding_evaluate` (lvae/evaluation.py:15-67).

Same contract: sorted rglob('*.*') over the dataset folder; per image compress_file -> file size*8 ->
decompress_file; PSNR on the un-rounded float reconstruction; bpp over the ORIGINAL pixel count; mean of per-image
values.  `imcoding_evaluate_sharded` is the multi-GPU form (one process per GPU, images rank::world, one tiny
all_gather of per-image stats over RCCL/xGMI) -- the only collective on this path.
"""
import math
from collections import defaultdict
from pathlib import Path
from tempfile import gettempdir

import torch

from .paths import known_datasets
from .utils.coding import crop_divisible_by, pil_to_tensor01


def _list_images(dataset):
    root = known_datasets.get(dataset, Path(dataset))
    img_paths = list(Path(root).rglob('*.*'))
    img_paths.sort()
    return img_paths


def _mse(real, fake):
    """mean((real - fake)^2) of one image (evaluation.py:47-49).  On the GPU: the native fp64-accumulating reduction
    (lvae_sqerr_partials_f32: deterministic) on the decoder's output where it lies -- no 12 B/pixel device-to-host copy and CPU pass per image;
    CPU tensors (stub codecs in tests): the reference's expression.  Every caller goes through here, so the sharded and the
    single-process evaluations agree bit for bit."""
    fake = fake.squeeze(0)
    if fake.is_cuda:
        import ctypes
        from . import _native
        a = fake.contiguous()
        b = real.to(a.device, non_blocking=True).contiguous()
        nblk = 512
        out = torch.empty(nblk, dtype=torch.float64, device=a.device)
        with torch.cuda.device(a.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
            _native.check(_native.lib().lvae_sqerr_partials_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), nblk, a.numel(), st), 'sqerr')
        total = 0.0
        for v in out.cpu().tolist():          # fixed order: deterministic across runs and processes
            total += v
        return total / a.numel()
    return (real - fake.cpu()).square().mean().item()


METRICS = ('psnr', 'ms-ssim')


def _want_ms_ssim(metrics):
    """Validate the `metrics` option of the evaluation functions; 'psnr' (bpp, mse, psnr) is always reported."""
    unknown = [m for m in metrics if m not in METRICS]
    if unknown:
        raise ValueError(f'unknown metrics {unknown}; known: {METRICS}')
    return 'ms-ssim' in metrics


def _ms_ssim(reals, fakes):
    """Per-image MS-SSIM of a batch as floats: ONE lvae.metrics.ms_ssim call on the reconstructions where they lie (cropped views of the
    decoder's padded batch on the GPU; CPU tensors of stub codecs take the fp64 path)."""
    from .metrics import ms_ssim
    return [float(v) for v in ms_ssim(reals, fakes).tolist()]


def _u8_codec(model):
    """True for the package's codecs on a GPU: the evaluation then uploads each original ONCE, as the bytes its PNG held, codes it from
    there (compress_images: the bytes compress_file writes) and makes the fp32 `real` of the metrics on the device (to_float01).
    Anything else with compress_file / decompress_file (CPU stub codecs in the tests) keeps the host float path."""
    if not hasattr(model, 'compress_images'):
        return None
    dev = next(model.parameters()).device
    return dev if dev.type == 'cuda' else None


def _stats(num_bits, real, mse):
    return {'bpp': float(num_bits / float(real.shape[1] * real.shape[2])), 'mse': float(mse), 'psnr': float(-10 * math.log10(mse))}


def _eval_one_tiled(model, impath, tile, overlap, ms=False):
    """_eval_one through the tiled path: compress_tiled / decompress_tiled(out='f32'); the bits are the whole container's."""
    from .utils.image import load_u8, to_float01
    dev = _u8_codec(model)
    if dev is None or not hasattr(model, 'compress_tiled'):
        raise ValueError('tile=...: the model has no tiled coding (compress_tiled) or is not on a GPU')
    u8 = load_u8(impath).to(dev, non_blocking=True)
    blob = model.compress_tiled(u8, tile=tile, overlap=overlap)
    fake = model.decompress_tiled(blob, out='f32')
    real = to_float01([u8], device=dev)[0][0]
    out = _stats(len(blob) * 8, real, _mse(real, fake))
    if ms:
        out['ms-ssim'] = _ms_ssim([real], [fake])[0]
    return out


def _eval_one_scaled(model, impath, scale, resample, ms=False):
    """_eval_one through reduced-resolution coding: compress_scaled / decompress_scaled(out='f32'); the bits are the whole container's,
    counted against the ORIGINAL pixel count, and the errors are taken at the original resolution."""
    from .utils.image import load_u8, to_float01
    dev = _u8_codec(model)
    if dev is None or not hasattr(model, 'compress_scaled'):
        raise ValueError('scale=...: the model has no reduced-resolution coding (compress_scaled) or is not on a GPU')
    u8 = load_u8(impath).to(dev, non_blocking=True)
    blob = model.compress_scaled([u8], scale=scale, filter=resample)[0]
    fake = model.decompress_scaled([blob], out='f32')[0]
    real = to_float01([u8], device=dev)[0][0]
    out = _stats(len(blob) * 8, real, _mse(real, fake))
    if ms:
        out['ms-ssim'] = _ms_ssim([real], [fake])[0]
    return out


def _eval_one(model, impath, tmp_bits_dir, tag='', ms=False):
    from PIL import Image
    tmp_bits_path = tmp_bits_dir / f'{impath.stem}{tag}.bits'
    dev = _u8_codec(model)
    if dev is not None:
        from .utils.image import load_u8, to_float01
        u8 = load_u8(impath).to(dev, non_blocking=True)
        with open(tmp_bits_path, 'wb') as f:
            f.write(model.compress_images([u8])[0])
    else:
        model.compress_file(impath, tmp_bits_path)
    num_bits = tmp_bits_path.stat().st_size * 8
    fake = model.decompress_file(tmp_bits_path)
    tmp_bits_path.unlink()
    real = to_float01([u8], device=dev)[0][0] if dev is not None else pil_to_tensor01(Image.open(impath))
    out = _stats(num_bits, real, _mse(real, fake))
    if ms:
        out['ms-ssim'] = _ms_ssim([real], [fake])[0]
    return out


@torch.no_grad()
def imcoding_evaluate(model, dataset, progress=False, metrics=('psnr',), tile=None, overlap=0, scale=None, resample='lanczos3'):
    """dict {bpp, mse, psnr}: dataset means of per-image values (evaluation.py:59-66).  metrics=('psnr', 'ms-ssim') adds the key
    'ms-ssim' (lvae.metrics.ms_ssim, mean over images); the other keys are the same floats either way.  tile=(th, tw): every image is
    coded in tiles (compress_tiled / decompress_tiled(out='f32') with `overlap`) and bpp counts the whole tiled container; tile=None
    is the whole-image path, float for float.  scale=S: every image is coded at reduced resolution (compress_scaled(scale=S, filter=resample)
    / decompress_scaled(out='f32')): bpp counts the whole scaled container against the ORIGINAL pixel count, mse and psnr are taken at the
    original resolution; scale=None changes nothing.  scale together with tile raises ValueError."""
    ms = _want_ms_ssim(metrics)
    if scale is not None and tile is not None:
        raise ValueError('imcoding_evaluate: scale and tile exclude each other (scaled and tiled containers are not combined)')
    assert hasattr(model, 'compress_file') and hasattr(model, 'decompress_file')
    img_paths = _list_images(dataset)
    tmp_bits_dir = Path(gettempdir())
    sums, n = defaultdict(float), 0
    it = img_paths
    if progress:
        from tqdm import tqdm
        it = tqdm(img_paths, ascii=True)
    for impath in it:
        if scale is not None:
            stats = _eval_one_scaled(model, impath, scale, resample, ms=ms)
        else:
            stats = _eval_one(model, impath, tmp_bits_dir, ms=ms) if tile is None else _eval_one_tiled(model, impath, tile, overlap, ms=ms)
        n += 1
        for k, v in stats.items():      # timm AverageMeter: running sum / count
            sums[k] += v
    return {k: v / n for k, v in sums.items()}


def _cropped_block_bits(pos, size, canvas, log2e):
    """Bits of one (h_i, w_i) fp64 block map (nats per position) that fall on the top-left (h, w) pixels of an (H, W) canvas: a position
    at stride s gives pos * log2e / s^2 to each of its s x s pixels, so it counts with the number of its pixels inside the crop."""
    (h, w), (H, W) = size, canvas
    s = H // pos.shape[0]
    ny = (h - torch.arange(pos.shape[0], dtype=torch.float64, device=pos.device) * s).clamp(0, s)
    nx = (w - torch.arange(pos.shape[1], dtype=torch.float64, device=pos.device) * s).clamp(0, s)
    return float((pos * ny[:, None] * nx[None, :]).sum() * log2e / (s * s))


@torch.no_grad()
def rate_map_evaluate(model, dataset, out_dir=None, lmb=None):
    """Where the bits of every image of `dataset` (a known name or a folder, as imcoding_evaluate) go: model.rate_map on the image's
    bytes (the u8 path of compress_images), one image per call.  -> a list, in sorted path order, of
      {'name': the file's stem, 'bits': the fp64 sum of the image's map, 'shares': [the fraction of those bits each latent block -- and,
       last, the lossless model's pixel stage -- gives inside the image's own (h, w)]}.
    out_dir: also write <stem>.npy (the (h, w) fp32 map, bits per pixel at each pixel) and <stem>.png (grey, to_u8(map / map.max()),
    rounded where the map lies) there; the folder is created.  lmb: variable-rate models only (model.rate_map raises TypeError otherwise).
    ValueError: a model without rate_map, a dataset without files, two files of one stem with out_dir."""
    import numpy as np
    from .utils.image import load_u8, to_u8
    if not callable(getattr(model, 'rate_map', None)):
        raise ValueError(f'rate_map_evaluate: {type(model).__name__} has no rate_map')
    img_paths = [p for p in _list_images(dataset) if p.is_file()]
    if not img_paths:
        raise ValueError(f'rate_map_evaluate: no images in {dataset}')
    if out_dir is not None:
        stems = [p.stem for p in img_paths]
        if len(set(stems)) != len(stems):
            raise ValueError('rate_map_evaluate: two images share a stem; their maps would share a file name')
        out_dir = Path(out_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
    log2e = getattr(model, 'LOG2E', 1.4426950408889634)
    d = int(getattr(model, 'max_stride', 1))
    rows = []
    for impath in img_paths:
        u8 = load_u8(impath)
        h, w = int(u8.shape[0]), int(u8.shape[1])
        maps, blocks = model.rate_map([u8], blocks=True, **({} if lmb is None else {'lmb': lmb}))
        m = maps[0]
        assert tuple(m.shape) == (1, h, w), f'{impath}: map {tuple(m.shape)} for a {h} x {w} image'
        canvas = (d * math.ceil(h / d), d * math.ceil(w / d))
        per_block = [_cropped_block_bits(b[0], (h, w), canvas, log2e) for b in blocks]
        total = sum(per_block)
        rows.append({'name': impath.stem, 'bits': float(m.double().sum()), 'shares': [v / total if total > 0 else 0.0 for v in per_block]})
        if out_dir is not None:
            top = m.max()
            grey = to_u8([(m / top if float(top) > 0 else m).expand(3, h, w)])[0][:, :, 0]
            np.save(out_dir / f'{impath.stem}.npy', m[0].cpu().numpy())
            from PIL import Image
            Image.fromarray(grey.cpu().contiguous().numpy()).save(out_dir / f'{impath.stem}.png', format='PNG')
    return rows


YUV_METRICS = ('psnr', 'ssim', 'ms-ssim')


@torch.no_grad()
def yuv_evaluate(model, yuv_path, width, height, fmt='i420', max_frames=None, batch=8, lmb=None, depth=8, subsampling='420', siting='center',
                 layout='planar', metrics=('psnr',), tile=None, overlap=0, scale=None, resample='lanczos3', **colour):
    """A raw 8-bit 4:2:0 file coded frame by frame (an image codec as an intra-frame coder) -> dict of means over its frames: 'bpp'
    (8 * len(blob) / (h * w)) and the keys of lvae.metrics.psnr_yuv420 ('mse-y' ... 'psnr-yuv'), computed between the file's bytes and
    decompress_yuv420's.  colour: matrix / range / chroma of compress_yuv420 (matrix and range also go to decompress_yuv420).  Every frame
    is uploaded once, as the 1.5 bytes per pixel the file holds; conversion, coding, reconstruction and the squared errors stay on the
    device, and three integers per frame come back.  Frames are coded `batch` at a time; lmb: as in compress_yuv420.
    depth / subsampling / siting: with any value other than the defaults (8, '420', 'center') the file is a planar one of that depth and
    subsampling (utils.yuv.read_yuv; fmt must stay 'i420'), coded by compress_yuv / decompress_yuv with that siting and measured by
    lvae.metrics.psnr_yuv, whose key 'psnr-avg' joins the result; matrix may then be 'bt2020'.  layout 'semiplanar': a P010 / P012 / P210 /
    P212 file (utils.yuv.read_yuv_sp; depth 10 | 12, subsampling '420' | '422'), coded and reconstructed in that layout and measured on its
    codes.  fmt, depth, subsampling and layout are resolved ONCE, to a utils.yuv.FrameFormat that reads the file and names what
    compress_yuv / decompress_yuv code (they take every frame kind); a caller that holds a FrameFormat may pass it as `fmt`.
    metrics: 'psnr' (always reported: the keys above), 'ssim' adds 'ssim-y', 'ssim-u', 'ssim-v' (lvae.metrics.ssim_yuv) and 'ms-ssim' adds
    'ms-ssim-y' (lvae.metrics.ms_ssim_yuv on the luma plane; ValueError for frames with min(h, w) <= 160), both on the codes of the file's
    and the reconstruction's planes where they lie on the device, with data range 2^depth - 1; one more launch sequence per batch.  The
    other keys keep their values.
    tile = (th, tw), overlap: every frame is coded in tiles (compress_yuv_tiled / decompress_yuv_tiled, `batch` tiles at a time); 'bpp'
    then counts the whole tiled container.  Only 'psnr' is measured on frames coded in tiles.
    scale=S: every frame is coded at reduced resolution (compress_yuv_scaled(scale=S, filter=resample) / decompress_yuv_scaled); 'bpp'
    counts the whole scaled container against the ORIGINAL pixel count, and every metric is taken on the original-size frames.  ValueError
    for scale together with tile."""
    from .metrics import PSNR_YUV_KEYS, PSNR_YUV_KEYS2, ms_ssim_yuv, psnr_yuv, psnr_yuv420, ssim_yuv
    from .utils.yuv import FORMATS, FrameFormat
    if layout not in ('planar', 'semiplanar'):
        raise ValueError(f"yuv_evaluate: layout is 'planar' or 'semiplanar', got {layout!r}")
    unknown = set(colour) - {'matrix', 'range', 'chroma'}
    if unknown:
        raise TypeError(f'yuv_evaluate: unexpected arguments {sorted(unknown)}')
    bad = [m for m in metrics if m not in YUV_METRICS]
    if bad:
        raise ValueError(f'unknown metrics {bad}; known: {YUV_METRICS}')
    if 'ms-ssim' in metrics and min(height, width) <= 160:
        raise ValueError(f'yuv_evaluate: frames of {height}x{width}; MS-SSIM needs min(h, w) > 160 (5 scales of an 11-tap window)')
    dev = next(model.parameters()).device
    dec = {k: v for k, v in colour.items() if k != 'chroma'}
    if isinstance(fmt, FrameFormat):
        layout, depth, subsampling = fmt
    elif (depth, subsampling, siting, layout) == (8, '420', 'center', 'planar'):
        layout = fmt                                          # the 8-bit 4:2:0 file of `fmt`, as Yuv420Frames
    elif fmt != 'i420':
        raise ValueError(f'yuv_evaluate: depth / subsampling / siting apply to planar files, got fmt={fmt!r}')
    fmt = FrameFormat(layout, depth, subsampling, siting, colour.get('matrix', 'bt709'))
    frames = fmt.read(yuv_path, width, height, frames=max_frames, who='yuv_evaluate')
    how = dict(fmt._asdict(), siting=siting, **dec)
    compress = lambda chunk, **enc: model.compress_yuv(chunk, siting=siting, **enc)
    decompress = lambda blobs: model.decompress_yuv(blobs, **how)
    measure, keys = (psnr_yuv420, PSNR_YUV_KEYS) if fmt.layout in FORMATS else (psnr_yuv, PSNR_YUV_KEYS2)      # their keys differ
    if scale is not None:
        if tile is not None:
            raise ValueError('yuv_evaluate: scale and tile may not be combined (scaled and tiled coding are separate)')
        compress = lambda chunk, **enc: model.compress_yuv_scaled(chunk, scale=scale, filter=resample, siting=siting, **enc)
        decompress = lambda blobs: model.decompress_yuv_scaled(blobs, **how)
    if tile is not None:
        if set(metrics) - {'psnr'}:
            raise ValueError(f"yuv_evaluate: frames coded in tiles are measured by 'psnr' only, got metrics={tuple(metrics)}")

        def compress(chunk, lmb=None, **enc):
            per = lmb if isinstance(lmb, list) else [lmb] * len(chunk)
            return [model.compress_yuv_tiled(f, tile=tile, overlap=overlap, lmb=v, max_batch=batch, siting=siting, **enc) for f, v in zip(chunk, per)]
        decompress = lambda blobs: [model.decompress_yuv_tiled(b, max_batch=batch, **how) for b in blobs]
    frames = [f.to(dev, non_blocking=True) for f in frames]
    rows, step = [], max(1, int(batch))
    for o in range(0, len(frames), step):
        chunk = frames[o:o + step]
        enc = dict(colour)
        if lmb is not None:                    # a number, or one lambda per frame of the file
            enc['lmb'] = lmb if isinstance(lmb, (int, float)) else list(lmb)[o:o + step]
        blobs = compress(chunk, **enc)
        recs = decompress(blobs)
        stats = [dict(r) for r in measure(chunk, recs)]
        if 'ssim' in metrics:
            for r, extra in zip(stats, ssim_yuv(chunk, recs)):
                r.update(extra)
        if 'ms-ssim' in metrics:
            for r, extra in zip(stats, ms_ssim_yuv(chunk, recs)):
                r.update(extra)
        for blob, r in zip(blobs, stats):
            rows.append(dict(r, bpp=float(8 * len(blob) / float(height * width))))
    if 'ssim' in metrics:
        keys = keys + ('ssim-y', 'ssim-u', 'ssim-v')
    if 'ms-ssim' in metrics:
        keys = keys + ('ms-ssim-y',)
    out = {}
    for k in ('bpp',) + keys:
        acc = 0.0
        for r in rows:                         # frame order: the means do not depend on `batch`
            acc += r[k]
        out[k] = acc / len(rows)
    return out


class AverageMeter:
    """timm.utils.AverageMeter: running sum / count of the values it is updated with (tensors stay tensors)."""

    def __init__(self):
        self.val, self.sum, self.count, self.avg = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


@torch.no_grad()
def image_self_evaluate(model, dataset, progress=True):
    """The reference's validation loop (evaluation.py:70-107): for every image of sorted(rglob('*.*')) -- center-cropped to multiples of
    model.max_stride when the model has one (crop_divisible_by) -- call model(im) and average each returned statistic over the
    images (AverageMeter).  No entropy coding: the statistics are the model's forward() ones."""
    from PIL import Image
    device = next(model.parameters()).device
    img_paths = _list_images(dataset)
    pbar = img_paths
    if progress:
        from tqdm import tqdm
        pbar = tqdm(img_paths, ascii=True)
    all_image_stats = defaultdict(AverageMeter)
    for impath in pbar:
        img = Image.open(impath)
        if hasattr(model, 'max_stride'):
            img = crop_divisible_by(img, div=model.max_stride)
        im = pil_to_tensor01(img).unsqueeze_(0).to(device=device)
        stats = model(im)
        assert isinstance(stats, dict), f'{type(stats)=}. expected a dict.'
        for k, v in stats.items():
            all_image_stats[k].update(v)
        if progress:
            msg = ', '.join([f'{k}={v:.3f}' for k, v in stats.items()])
            pbar.set_description(f'image {impath.stem}: {msg}')
    return {k: meter.avg for k, meter in all_image_stats.items()}


def shard_paths(img_paths, rank, world):
    """Rank r of W codes sorted(img_paths)[r::W] -- the partition for same-size sets."""
    return img_paths[rank::world]


def padded_pixels(path, div=64):
    """Pixel count of an image after padding to multiples of `div` (what the codec actually processes); header read only."""
    from PIL import Image
    with Image.open(path) as img:
        h, w = img.height, img.width
    return (div * math.ceil(h / div)) * (div * math.ceil(w / div)), (div * math.ceil(h / div), div * math.ceil(w / div))


def lpt_partition(costs, world):
    """Longest-processing-time-first partition of items with the given costs over `world` ranks (mixed-size sets
    such as CLIC-2022, where rank::world leaves the ranks with the portrait/landscape 2048-wide images late).  Deterministic on
    every rank: items sorted by (-cost, index), each given to the least-loaded rank (ties -> lowest rank).  Returns a list of
    `world` index lists, each in ascending index order."""
    order = sorted(range(len(costs)), key=lambda i: (-costs[i], i))
    loads, parts = [0] * world, [[] for _ in range(world)]
    for i in order:
        r = min(range(world), key=lambda k: (loads[k], k))
        parts[r].append(i)
        loads[r] += costs[i]
    return [sorted(p) for p in parts]


def batch_same_size(indices, shapes, max_batch=8, max_pixels=8 * 512 * 768 * 4):
    """Group a rank's images by padded size into batches (<= max_batch images, <= max_pixels padded pixels in total): the GPU part
    of a batch runs batched and its rANS streams are coded by parallel host threads, instead of one image at a time."""
    groups, out = {}, []
    for i in indices:
        groups.setdefault(shapes[i], []).append(i)
    for shape, idxs in groups.items():
        per = max(1, min(max_batch, max_pixels // (shape[0] * shape[1])))
        for o in range(0, len(idxs), per):
            out.append(idxs[o:o + per])
    out.sort(key=lambda b: b[0])
    return out


def _decode_images(paths):
    """PIL images of `paths`, fully decoded (run on a helper thread: PNG decoding releases the GIL)."""
    from PIL import Image
    imgs = []
    for p in paths:
        img = Image.open(p)
        img.load()
        imgs.append(img)
    return imgs


def _eval_batch(model, paths, tmp_bits_dir, tag='', images=None, ms=False):
    """_eval_one for a batch of same-padded-size images through the model's batched file API (bit-identical per image); every
    PNG is decoded once (`images`: already decoded by the prefetch thread)."""
    if not hasattr(model, 'compress_files'):
        return [_eval_one(model, p, tmp_bits_dir, tag, ms) for p in paths]
    imgs = images if images is not None else _decode_images(paths)
    bits = [tmp_bits_dir / f'{p.stem}{tag}.{k}.bits' for k, p in enumerate(paths)]
    dev = _u8_codec(model)
    if dev is not None:
        from .utils.image import load_u8, to_float01
        u8 = [load_u8(img).to(dev, non_blocking=True) for img in imgs]
        for blob, b in zip(model.compress_images(u8), bits):
            with open(b, 'wb') as f:
                f.write(blob)
        x, sizes = to_float01(u8, device=dev)             # one launch: the batch's originals as fp32, cropped views below
        reals = [x[i, :, :h, :w] for i, (h, w) in enumerate(sizes)]
    else:
        model.compress_files(paths, bits, images=imgs)
        reals = [pil_to_tensor01(img) for img in imgs]
    fakes = model.decompress_files(bits)
    out = []
    for real, b, fake in zip(reals, bits, fakes):
        num_bits = b.stat().st_size * 8
        b.unlink()
        out.append(_stats(num_bits, real, _mse(real, fake)))
    if ms:
        for o, v in zip(out, _ms_ssim(reals, fakes)):
            o['ms-ssim'] = v
    return out


def gather_stats(local, world, device=None, columns=4):
    """all_gather of per-image (index, bpp, mse, psnr) rows as float64 (`columns=5`: with ms-ssim behind them); returns rows sorted
    by image index so that the mean is computed in exactly the single-process order."""
    import torch.distributed as dist
    t = torch.tensor(local, dtype=torch.float64).reshape(-1, columns)
    if device is not None:
        t = t.to(device)
    counts = [torch.zeros(1, dtype=torch.int64, device=t.device) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device))
    mx = max(int(c.item()) for c in counts)
    pad = torch.zeros(mx, columns, dtype=torch.float64, device=t.device)
    pad[:t.shape[0]] = t
    bufs = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad)
    rows = torch.cat([b[:int(c.item())] for b, c in zip(bufs, counts)], 0).cpu()
    return rows[torch.argsort(rows[:, 0])]


@torch.no_grad()
def imcoding_evaluate_sharded(model, dataset, partition='lpt', max_batch=8, metrics=('psnr',)):
    """Same result as imcoding_evaluate (to the last bit: per-image values do not depend on batching, means are formed in image
    order), with the image list sharded over torch.distributed ranks: LPT by padded pixel count (`partition='stride'`:
    rank::world), and inside a rank same-size images coded as batches of up to `max_batch`.  `metrics` as for imcoding_evaluate."""
    import torch.distributed as dist
    ms = _want_ms_ssim(metrics)
    keys = ('bpp', 'mse', 'psnr') + (('ms-ssim',) if ms else ())
    rank, world = dist.get_rank(), dist.get_world_size()
    img_paths = _list_images(dataset)
    tmp_bits_dir = Path(gettempdir())
    meta = [padded_pixels(p, getattr(model, 'max_stride', 64)) for p in img_paths]
    if partition == 'lpt':
        mine = lpt_partition([m[0] for m in meta], world)[rank]
    else:
        mine = list(range(rank, len(img_paths), world))
    local = []
    batches = batch_same_size(mine, [m[1] for m in meta], max_batch=max_batch)
    # the next batch's PNGs are decoded on a helper thread while the GPU and the coder threads work on the current one
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(_decode_images, [img_paths[i] for i in batches[0]]) if batches else None
        for bi, batch in enumerate(batches):
            imgs = nxt.result()
            nxt = pool.submit(_decode_images, [img_paths[i] for i in batches[bi + 1]]) if bi + 1 < len(batches) else None
            stats = _eval_batch(model, [img_paths[i] for i in batch], tmp_bits_dir, tag=f'.r{rank}',
                                images=imgs if hasattr(model, 'compress_files') else None, ms=ms)
            for idx, s in zip(batch, stats):
                local.append([float(idx)] + [s[k] for k in keys])
    dev = next(model.parameters()).device
    rows = gather_stats(local, world, dev if dist.get_backend() == 'nccl' else None, columns=1 + len(keys))
    assert rows.shape[0] == len(img_paths)
    out = {}
    for j, k in enumerate(keys):
        acc = 0.0
        for v in rows[:, j + 1].tolist():
            acc += v
        out[k] = acc / rows.shape[0]
    return out
