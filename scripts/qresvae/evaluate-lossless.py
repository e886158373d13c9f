#!/usr/bin/env python
"""Lossless compression rate of qres34m_lossless over an image folder (the reference's scripts/qresvae/evaluate-lossless.py:14-62 on
this package): compress_file -> file size -> decompress_images (8-bit on the device), asserting that every image is reproduced bit-exactly.

    python scripts/qresvae/evaluate-lossless.py --root /path/to/kodak [--weights qres34m-lossless.pt]
    python scripts/qresvae/evaluate-lossless.py --synthetic 4            # seeded weights + seeded images (no network here)
"""
import argparse
import os
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import lvae  # noqa: E402


@torch.inference_mode()
def evaluate_model(model, img_paths):
    tmp_bit_path = Path(tempfile.mkdtemp()) / 'tmp.bits'
    accumulated_bpp = 0.0
    for impath in img_paths:
        model.compress_file(impath, tmp_bit_path)
        num_bits = tmp_bit_path.stat().st_size * 8
        fake = model.decompress_images([tmp_bit_path.read_bytes()])[0].cpu()                         # (h, w, 3) uint8, rounded on the device
        tmp_bit_path.unlink()
        real = torch.from_numpy(np.asarray(Image.open(impath).convert('RGB')))                       # uint8
        assert torch.equal(real, fake), f'{impath}: not lossless'
        bpp = num_bits / float(real.shape[0] * real.shape[1])
        accumulated_bpp += float(bpp)
        print(f'image {Path(impath).stem}: bpp={bpp:.4f}')
    return accumulated_bpp / len(img_paths)


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', type=str, default=None)
    ap.add_argument('--weights', type=str, default=None)
    ap.add_argument('--synthetic', type=int, default=0, help='use N seeded 256x384 images and seeded random-init weights')
    args = ap.parse_args()
    model = lvae.get_model('qres34m_lossless', pretrained=(args.weights or (not args.synthetic)))
    if args.synthetic and not args.weights:
        import seeded_init
        sd = model.state_dict()
        for k in list(sd.keys()):
            a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
            if a is not None and 'discrete_gaussian' not in k:
                sd[k] = torch.from_numpy(a)
        model.load_state_dict(sd)
    model.compress_mode()
    model = model.cuda()
    model.eval()
    if args.synthetic:
        import seeded_init
        d = Path(tempfile.mkdtemp())
        paths = []
        for i in range(args.synthetic):
            Image.fromarray(seeded_init.synthetic_image_u8(256, 384, 500 + i)).save(d / f'im{i}.png')
            paths.append(d / f'im{i}.png')
    else:
        paths = sorted(Path(args.root).rglob('*.*'))
    print(f'Average bpp: {evaluate_model(model, paths)} \n')


if __name__ == '__main__':
    main()
