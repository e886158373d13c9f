"""How an image gets into and out of the codec: the host float path (pad on the host, divide on the host, upload 12 bytes per padded
pixel) against the u8 path (upload 3 bytes per pixel, lvae_image_u8_to_f32 / lvae_image_f32_to_u8 on the device), and one evaluation
step (lvae.evaluation._eval_batch: compress, decompress, MSE) around them.  Workloads: 8 images of 512 x 768, and 2 of 1365 x 2048 (which
pad to 1408 x 2048); seeded synthetic images, decoded to PIL before anything is timed.
  (a) float_in : torch.stack([pil_to_tensor01(pad_divisible_by(img))]).to(device)
  (b) u8_in    : to_float01(u8 images, div=64, device)        -- inputs as load_u8 leaves them (pinned host tensors)
      u8_in_from_pil: to_float01([load_u8(img) ...])           -- from the same PIL images as (a): the copy out of PIL and the pinning included
  (c) u8_out   : to_u8(x) + one device-to-host copy per image, against torch_out: (x * 255).round().to(uint8).cpu() on the device
  (d) eval_step: _eval_batch(model, paths, images=PIL images) with qarv_base (bench.py's seeded model)
(a) / (b) and the two forms of (c) alternate step by step in one process, the device synchronised after every call; medians, min, max in
ms.  --eval-only times (d) alone and imports nothing the parent commit lacks, so the same file run from an earlier tree gives the other
side of an A/B on one box (LVAE_TREE names that tree; tools/ab_image_io.sh alternates the two, as tools/ab_bench.sh does for bench.py).
One JSON line.
    python tools/image_io_bench.py [--steps 20] [--warmup 3] [--eval-only] [--tag NAME]"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.environ.get('LVAE_TREE') or os.path.dirname(HERE)          # LVAE_TREE: time another checkout with this file
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

WORKLOADS = {'b8_512x768': (8, 512, 768), 'b2_1365x2048': (2, 1365, 2048)}


def main():
    import bench
    import seeded_init
    from PIL import Image
    from lvae.evaluation import _eval_batch
    from lvae.utils.coding import pad_divisible_by, pil_to_tensor01
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--eval-only', action='store_true')
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

    res = {'metric': 'image_io_ms', 'tag': args.tag, 'tree': 'LVAE_TREE' if os.environ.get('LVAE_TREE') else 'own', 'steps': args.steps, 'warmup': args.warmup}
    model, _ = bench.build_model(dev)
    tmp = Path(tempfile.mkdtemp())
    for name, (B, H, W) in WORKLOADS.items():
        paths = []
        for i in range(B):
            paths.append(tmp / f'{name}_{i}.png')
            Image.fromarray(seeded_init.synthetic_image_u8(H, W, seed=1000 + i)).save(paths[-1])
        pil = []
        for p in paths:
            img = Image.open(p)
            img.load()
            pil.append(img)
        row = {}
        if not args.eval_only:
            from lvae.utils.image import load_u8, to_float01, to_u8
            u8 = [load_u8(img) for img in pil]
            box = {}

            def float_in():
                box['a'] = torch.stack([pil_to_tensor01(pad_divisible_by(img, 64)) for img in pil]).to(dev)

            def u8_in():
                box['b'] = to_float01(u8, div=64, device=dev)[0]

            def u8_in_from_pil():
                box['b2'] = to_float01([load_u8(img) for img in pil], div=64, device=dev)[0]
            row.update(alternate({'float_in': float_in, 'u8_in': u8_in, 'u8_in_from_pil': u8_in_from_pil}))
            assert torch.equal(box['a'], box['b']) and torch.equal(box['a'], box['b2'])
            row['float_in_over_u8_in'] = round(row['float_in']['median'] / row['u8_in']['median'], 2)
            row['float_in_over_u8_in_from_pil'] = round(row['float_in']['median'] / row['u8_in_from_pil']['median'], 2)
            x = box['a']

            def u8_out():
                box['c'] = [t.cpu() for t in to_u8(x)]

            def torch_out():
                box['d'] = (x * 255).round().to(torch.uint8).cpu()
            row.update(alternate({'u8_out': u8_out, 'torch_out': torch_out}))
            assert all(torch.equal(c, d.permute(1, 2, 0)) for c, d in zip(box['c'], box['d']))
            row['torch_out_over_u8_out'] = round(row['torch_out']['median'] / row['u8_out']['median'], 2)
        row.update(alternate({'eval_step': lambda: _eval_batch(model, paths, tmp, images=pil)}))
        res[name] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
