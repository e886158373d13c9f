"""SSIM / MS-SSIM on YUV frames on the HIP kernels (lvae.metrics.ssim_yuv / ms_ssim_yuv -> lvae_msssim_planes: the integer planes read where
they lie, one call for all planes of all frames) against what a user had before them on the same GPU: the planes converted to fp32 / L
with torch ops -- P010 frames through to_planar() first -- and lvae.metrics.ms_ssim once per plane size.  Frames are device-resident.
  (a) ms_ssim_yuv(planes='yuv') on 2 x 1080x1920 10-bit 4:2:0 planar frames,
  (b) the same on P010 frames,
  (c) ssim_yuv on 8 x 512x768 8-bit 4:2:0 frames; there was no single-scale SSIM, so the comparison is the definition in fp32 torch
      (F.conv2d) on the converted planes,
  (d) one yuv_evaluate step of 8 x 512x768 8-bit 4:2:0 with qarv_base (bench.py's seeded model) without and with metrics=('psnr', 'ssim').
The variants of a row are timed alternately in one process, after warm-up steps of all, the device synchronised after every call; medians
in ms.  These are call times with a host clock around a synchronised call, not kernel times.  Prints one JSON line.
    python tools/ssim_yuv_bench.py [--steps 20] [--warmup 3] [--no-codec]"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def torch_ssim_fp32(x, y):
    """Single-scale SSIM of (B, 1, h, w) fp32 planes in [0, 1] with F.conv2d -> (B,)."""
    c = torch.arange(11, dtype=x.dtype, device=x.device) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 * 1.5))
    g = g / g.sum()
    filt = lambda t: F.conv2d(F.conv2d(t, g.view(1, 1, -1, 1)), g.view(1, 1, 1, -1))
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    return (((2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)) * ((2 * sxy + 9e-4) / (sxx + syy + 9e-4))).flatten(1).mean(1)


def main():
    import bench
    import seeded_init
    from lvae.evaluation import yuv_evaluate
    from lvae.metrics import ms_ssim, ms_ssim_yuv, ssim_yuv
    from lvae.utils.yuv import from_rgb01, from_rgb01_any, write_yuv420
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-codec', action='store_true', help='skip the yuv_evaluate row (no model is built)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')

    def once(fn):
        t0 = time.perf_counter()
        fn(); torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def alternate(fns):
        """-> {name: (median, min, max) ms}: the functions timed in turn, step by step, so that drift of the host hits all alike."""
        for _ in range(args.warmup):
            for fn in fns.values():
                once(fn)
        ts = {k: [] for k in fns}
        for _ in range(args.steps):
            for k, fn in fns.items():
                ts[k].append(once(fn))
        return {k: dict(zip(('median', 'min', 'max'), (round(float(np.median(v)) * 1e3, 4), round(min(v) * 1e3, 4), round(max(v) * 1e3, 4))))
                for k, v in ts.items()}

    def pair(B, H, W, **layout):
        """B reference frames and noisy reconstructions of them on the device."""
        rgb = [torch.from_numpy(seeded_init.synthetic_image_u8(H, W, seed=1000 + i)).permute(2, 0, 1).float().div(255) for i in range(B)]
        g = torch.Generator().manual_seed(0)
        rec = [(x + 0.03 * torch.randn(x.shape, generator=g)).clamp(0, 1) for x in rgb]
        make = (lambda xs: from_rgb01_any(xs, **layout)) if layout else from_rgb01
        return [f.to(dev) for f in make(rgb)], [f.to(dev) for f in make(rec)]

    def composed(frames, recs, depth, fn):
        """What a user writes without the plane entry: planar frames, planes as fp32 / L, `fn` once per plane size -> [luma values, chroma values]."""
        L = float((1 << depth) - 1)
        planar = lambda f: f.to_planar() if hasattr(f, 'to_planar') else f
        a, b = [planar(f) for f in frames], [planar(f) for f in recs]
        f32 = lambda ps: torch.stack([p.float() for p in ps]).unsqueeze(1) / L
        return [fn(f32([f.y for f in a]), f32([f.y for f in b])),
                fn(f32([p for f in a for p in (f.u, f.v)]), f32([p for f in b for p in (f.u, f.v)]))]

    res = {'metric': 'ssim_yuv_ms', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup}
    for name, layout in {'ms_ssim_yuv_b2_1080x1920_10bit_420': dict(depth=10), 'ms_ssim_yuv_b2_1080x1920_p010': dict(depth=10, layout='semiplanar')}.items():
        ref, rec = pair(2, 1080, 1920, **layout)
        box = {}

        def planes():
            box['a'] = ms_ssim_yuv(ref, rec, planes='yuv')

        def today():
            box['b'] = [v.cpu() for v in composed(ref, rec, 10, ms_ssim)]
        row = alternate({'planes': planes, 'convert_then_ms_ssim': today})
        row['convert_then_ms_ssim_over_planes'] = round(row['convert_then_ms_ssim']['median'] / row['planes']['median'], 2)
        luma, chroma = box['b']
        row['max_abs_diff'] = max(max(abs(r['ms-ssim-y'] - float(luma[i])), abs(r['ms-ssim-u'] - float(chroma[2 * i])),
                                      abs(r['ms-ssim-v'] - float(chroma[2 * i + 1]))) for i, r in enumerate(box['a']))
        res[name] = row
    ref, rec = pair(8, 512, 768)
    box = {}

    def planes8():
        box['a'] = ssim_yuv(ref, rec)

    def torch8():
        box['b'] = [v.cpu() for v in composed(ref, rec, 8, torch_ssim_fp32)]
    row = alternate({'planes': planes8, 'convert_then_torch_fp32': torch8})
    row['convert_then_torch_fp32_over_planes'] = round(row['convert_then_torch_fp32']['median'] / row['planes']['median'], 2)
    row['max_abs_diff'] = max(abs(r['ssim-y'] - float(box['b'][0][i])) for i, r in enumerate(box['a']))
    res['ssim_yuv_b8_512x768_8bit_420'] = row
    if not args.no_codec:
        model = bench.build_model(dev)[0]
        path = Path(tempfile.mkdtemp()) / 'clip.yuv'
        write_yuv420([f.cpu() for f in ref], path)
        row = alternate({'psnr': lambda: yuv_evaluate(model, path, 768, 512, batch=8),
                         'psnr_ssim': lambda: yuv_evaluate(model, path, 768, 512, batch=8, metrics=('psnr', 'ssim')),
                         'psnr_ssim_ms_ssim': lambda: yuv_evaluate(model, path, 768, 512, batch=8, metrics=('psnr', 'ssim', 'ms-ssim'))})
        row['ssim_share_of_step'] = round(1 - row['psnr']['median'] / row['psnr_ssim']['median'], 4)
        row['ssim_and_ms_ssim_share_of_step'] = round(1 - row['psnr']['median'] / row['psnr_ssim_ms_ssim']['median'], 4)
        res['yuv_evaluate_step_b8_512x768'] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
