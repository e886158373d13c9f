"""The resampler of reduced-resolution coding (csrc/resample.hip) against what a user had before it on the same GPU: torch's antialiased
bicubic F.interpolate on fp32 NCHW, with lvae.utils.image.to_float01 in front of it on the way in and to_u8 behind it on the way out (an
fp32 round trip through HBM on each side of the resize).  Both sides run the bicubic filter at scale 0.5; the images are on the device
before the clock starts.  Workloads: 8 images of 512 x 768 and 2 of 1365 x 2048, seeded synthetic.
  in : torch_in     : to_float01(images) -> F.interpolate(size=half, mode='bicubic', antialias=True).clamp(0, 1) -> replicate padding to 64
       resample_in  : resize(images, half, 'bicubic', clamp=True) into the padded canvas (lvae_resample_u8_to_f32, one launch)
  out: torch_out    : F.interpolate(x, size=full, mode='bicubic', antialias=True) -> to_u8
       resample_out : resize(x, full, 'bicubic', out='u8') (lvae_resample_f32_to_u8, one launch)
The variants of a row alternate step by step in one process, the device synchronised after every call; medians, min, max in ms.  torch
forms its scale in fp32, so the two sides agree within 2e-5 / one byte, not bit for bit (asserted).  One JSON line.
    python tools/resample_bench.py [--steps 20] [--warmup 3] [--tag NAME]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WORKLOADS = {'b8_512x768': (8, 512, 768), 'b2_1365x2048': (2, 1365, 2048)}


def main():
    import seeded_init
    from lvae.utils.image import ScaledU8Batch, resize, to_float01, to_u8
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--tag', type=str, default='')
    args = ap.parse_args()
    dev = torch.device('cuda:0')

    def once(fn):
        t0 = time.perf_counter()
        fn(); torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def alternate(fns):
        for _ in range(args.warmup):
            for fn in fns.values():
                once(fn)
        ts = {k: [] for k in fns}
        for _ in range(args.steps):
            for k, fn in fns.items():
                ts[k].append(once(fn))
        return {k: dict(zip(('median', 'min', 'max'), (round(float(np.median(v)) * 1e3, 4), round(min(v) * 1e3, 4), round(max(v) * 1e3, 4))))
                for k, v in ts.items()}

    res = {'metric': 'resample_ms', 'tag': args.tag, 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
           'filter': 'bicubic', 'scale': 0.5}
    for name, (B, H, W) in WORKLOADS.items():
        imgs = [torch.from_numpy(seeded_init.synthetic_image_u8(H, W, seed=1000 + i)).to(dev) for i in range(B)]
        h, w = max(1, round(H * 0.5)), max(1, round(W * 0.5))
        batch = ScaledU8Batch(imgs, (h, w), 'bicubic', 64, dev)
        _, _, Hc, Wc = batch.shape
        box, row = {}, {'coded': [h, w], 'canvas': [Hc, Wc]}

        def torch_in():
            x = F.interpolate(to_float01(imgs, device=dev)[0], size=(h, w), mode='bicubic', antialias=True, align_corners=False).clamp_(0, 1)
            box['a'] = F.pad(x, (0, Wc - w, 0, Hc - h), mode='replicate')

        def resample_in():
            out = torch.empty(batch.shape, dtype=torch.float32, device=dev)
            batch.fill(out)
            box['b'] = out
        row.update(alternate({'torch_in': torch_in, 'resample_in': resample_in}))
        row['in_max_abs_diff'] = float((box['a'] - box['b']).abs().max())
        assert row['in_max_abs_diff'] <= 2e-5
        row['torch_in_over_resample_in'] = round(row['torch_in']['median'] / row['resample_in']['median'], 2)
        x = box['b'][:, :, :h, :w]                     # a crop of the padded batch, read in place by the kernel

        def torch_out():
            box['c'] = to_u8(F.interpolate(x, size=(H, W), mode='bicubic', antialias=True, align_corners=False))

        def resample_out():
            box['d'] = resize(x, (H, W), filter='bicubic', out='u8')
        row.update(alternate({'torch_out': torch_out, 'resample_out': resample_out}))
        row['out_max_byte_diff'] = max(int((c.int() - d.int()).abs().max()) for c, d in zip(box['c'], box['d']))
        assert row['out_max_byte_diff'] <= 1
        row['torch_out_over_resample_out'] = round(row['torch_out']['median'] / row['resample_out']['median'], 2)
        res[name] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
