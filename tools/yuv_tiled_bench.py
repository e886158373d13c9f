"""Decoded tiles -> YUV planes: the fused kernel (lvae.utils.yuv.stitch_tiles_yuv -> lvae_tile_stitch_yuv) against the composition it
replaces on the same GPU, stitch_tiles(out='f32') followed by from_rgb01_any / from_rgb01, which writes and reads back an fp32 image of
12 bytes per pixel.  Tiles are device-resident random fp32 in [-0.1, 1.1].
  (a) one 2160x3840 frame, 10-bit 4:2:0 planar, from 5 x 6 tiles of 512x768 with overlap 32,
  (b) the same as P010,
  (c) 8 frames of 512x768, 8-bit 4:2:0 (I420), each a single tile: 8 calls of either form per step,
  (d) unless --no-codec: qarv_base (bench.py's seeded model) decoding that 4K frame once from its tiled container (decompress_yuv_tiled)
      and once from the frame coded whole (decompress_yuv), after one warm-up call of each, with the containers' bytes.
The outputs of the two forms are asserted bit-equal first.  The variants of a row are then timed alternately in one process, after warm-up
steps of all, the device synchronised after every call; medians, minima and maxima in ms.  These are call times with a host clock around a
synchronised call, not kernel times.  peak_mib: the most device memory a call holds above what was allocated before it
(torch.cuda.max_memory_allocated), outputs and scratch included; in row (d) the launch plans recorded by the warm-up call are allocated
before it, and plan_mib is what that first call left allocated: the plans' weights-independent buffers, activations among them.  Prints
one JSON line.
    python tools/yuv_tiled_bench.py [--steps 20] [--warmup 3] [--no-codec]"""
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
    from lvae.utils import tiling
    from lvae.utils.image import stitch_tiles
    from lvae.utils.yuv import from_rgb01, from_rgb01_any, stitch_tiles_yuv
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-codec', action='store_true', help='skip row (d) (no model is built)')
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

    def peak_mib(fn):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base
        del out
        return round(peak / 2 ** 20, 2)

    def planes(fr):
        return fr.planes()

    def tiles_of(h, w, th, tw, ov, seed):
        ys, xs = tiling.tile_grid(h, w, th, tw, ov)
        g = torch.Generator(device=dev).manual_seed(seed)
        return [torch.rand(3, th, tw, generator=g, device=dev) * 1.2 - 0.1 for _ in range(len(ys) * len(xs))]

    def row(images, grid, fmt):
        """images: a list of tile lists, one call of either form per image and step."""
        i420 = fmt.get('layout') == 'i420'
        convert = (lambda x: from_rgb01(x)[0]) if i420 else (lambda x: from_rgb01_any(x, **fmt)[0])
        fused = lambda: [stitch_tiles_yuv(t, *grid, **fmt) for t in images]
        composed = lambda: [convert(stitch_tiles(t, *grid, out='f32')) for t in images]
        for a, b in zip(fused(), composed()):
            assert all(torch.equal(p, q) for p, q in zip(planes(a), planes(b))), 'the two forms differ'
        r = alternate({'fused': fused, 'stitch_f32_then_convert': composed})
        r['composition_over_fused'] = round(r['stitch_f32_then_convert']['median'] / r['fused']['median'], 3)
        r['peak_mib'] = {'fused': peak_mib(fused), 'stitch_f32_then_convert': peak_mib(composed)}
        return r

    res = {'metric': 'yuv_tiled_ms', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup}
    H, W, TH, TW, OV = 2160, 3840, 512, 768, 32
    big = tiles_of(H, W, TH, TW, OV, 1)
    res['stitch_2160x3840_10bit_420_planar'] = row([big], (H, W, TH, TW, OV), dict(depth=10))
    res['stitch_2160x3840_p010'] = row([big], (H, W, TH, TW, OV), dict(depth=10, layout='semiplanar'))
    del big
    small = [tiles_of(512, 768, 512, 768, 0, 10 + i) for i in range(8)]
    res['stitch_8x_512x768_8bit_420_single_tile'] = row(small, (512, 768, 512, 768, 0), dict(layout='i420'))
    del small
    if not args.no_codec:
        import bench
        import seeded_init
        model = bench.build_model(dev)[0]
        kw = dict(depth=10, subsampling='420', siting='center')
        rgb = torch.from_numpy(seeded_init.synthetic_image_u8(H, W, seed=2000)).permute(2, 0, 1).float().div(255)
        frame = from_rgb01_any([rgb], **kw)[0]
        tiled = model.compress_yuv_tiled(frame, tile=(TH, TW), overlap=OV)
        whole = model.compress_yuv([frame])[0]
        forms = {'decompress_yuv_tiled': lambda: model.decompress_yuv_tiled(tiled, **kw), 'decompress_yuv_whole_frame': lambda: model.decompress_yuv([whole], **kw)}
        r = {'bytes': {'tiled_container': len(tiled), 'whole_frame': len(whole)}}
        for k, fn in forms.items():
            torch.cuda.synchronize(dev)
            base = torch.cuda.memory_allocated(dev)
            once(fn)                                     # the launch plans of the shape are recorded here, with the activation buffers they keep
            kept = round((torch.cuda.memory_allocated(dev) - base) / 2 ** 20, 2)
            r[k] = {'ms': round(once(fn) * 1e3, 3), 'plan_mib': kept, 'peak_mib': peak_mib(fn)}
        res['decode_2160x3840_10bit_420_qarv_base'] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
