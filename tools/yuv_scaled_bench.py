"""YUV frames at reduced resolution: the fused kernels of csrc/resample_yuv.hip against the compositions of existing entries they replace,
on the same GPU in one run.
  in :  fused    = utils.yuv.to_rgb01_scaled                                  (lvae_resample_yuv_to_f32, one launch)
        composed = utils.yuv.to_rgb01_any, then utils.image._resample_f32     (lvae_image_yuv*_to_f32, then lvae_resample_f32(clamp=1)):
                   a full-resolution fp32 RGB image, 12 bytes per pixel, is written and read back
  out:  fused    = utils.yuv.from_rgb01_scaled                                (lvae_resample_f32_to_yuv, one launch)
        composed = utils.image._resample_f32, then utils.yuv.from_rgb01_any   (lvae_resample_f32(clamp=0), then lvae_image_f32_to_yuv*)
Cases, scale 0.5 each way, bicubic:
  (a) 2 frames of 2160x3840, 10-bit 4:2:0 planar  <->  1080x1920,
  (b) the same as P010,
  (c) 8 frames of 512x768, 8-bit 4:2:0 (I420)  <->  256x384.
Frames and fp32 images are device-resident (random codes; random fp32 in [-0.1, 1.1]).  The outputs of the two forms are asserted
bit-equal first.  The variants of a row are then timed alternately in one process, after warm-up steps of all, the device synchronised
after every call; medians, minima and maxima in ms.  These are call times with a host clock around a synchronised call, not kernel times.
peak_mib: the most device memory a call holds above what was allocated before it (torch.cuda.max_memory_allocated), outputs included.
Prints one JSON line.
    python tools/yuv_scaled_bench.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from lvae.utils.image import _resample_f32
    from lvae.utils.yuv import FrameFormat, from_rgb01_any, from_rgb01_scaled, to_rgb01_any, to_rgb01_scaled
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    filt = 'bicubic'

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

    def peak_mib(fn):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base
        del out
        return round(peak / 2 ** 20, 2)

    def compare(fused, composed, same):
        assert same(fused(), composed()), 'the two forms differ'
        r = alternate({'fused': fused, 'composed': composed})
        r['composed_over_fused'] = round(r['composed']['median'] / r['fused']['median'], 3)
        r['peak_mib'] = {'fused': peak_mib(fused), 'composed': peak_mib(composed)}
        return r

    def row(n, h, w, layout, depth, seed):
        fmt = FrameFormat(layout, depth, '420')
        g = torch.Generator(device=dev).manual_seed(seed)
        frames = []
        for _ in range(n):
            f = fmt.new(h, w, dev)
            for p in f.planes():
                codes = torch.randint(0, 1 << depth, tuple(p.shape), generator=g, device=dev)
                p.copy_(codes << (16 - depth) if layout == 'semiplanar' else codes)
            frames.append(f)
        small = (h // 2, w // 2)
        how = dict(depth=depth, subsampling='420', layout=layout)
        x = torch.rand(n, 3, *small, generator=g, device=dev) * 1.2 - 0.1
        views = [x[i] for i in range(n)]
        same_frames = lambda a, b: all(torch.equal(p, q) for fa, fb in zip(a, b) for p, q in zip(fa.planes(), fb.planes()))
        return {
            'in': compare(lambda: to_rgb01_scaled(frames, small, filt),
                          lambda: _resample_f32(list(to_rgb01_any(frames, 1, dev)[0]), small, filt, True, 'f32'), torch.equal),
            'out': compare(lambda: from_rgb01_scaled(views, (h, w), filt, **how),
                           lambda: from_rgb01_any(_resample_f32(views, (h, w), filt, False, 'f32'), **how), same_frames),
        }

    res = {'metric': 'yuv_scaled_ms', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'filter': filt}
    res['2x_2160x3840_10bit_420_planar'] = row(2, 2160, 3840, 'planar', 10, 1)
    res['2x_2160x3840_p010'] = row(2, 2160, 3840, 'semiplanar', 10, 2)
    res['8x_512x768_8bit_i420'] = row(8, 512, 768, 'i420', 8, 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
