#!/usr/bin/env python
"""Folder-to-folder codec: PNGs -> .bits files and back, 8-bit end to end on the GPU (CodecBase.compress_images /
decompress_to_files: the bytes of an image are uploaded as they are, a reconstruction is rounded to bytes before it is copied back).

    python scripts/lvae-codec.py encode IMAGES/ BITS/ -m qarv_base --lmb 256 [--batch 8]
    python scripts/lvae-codec.py decode BITS/ RECON/ -m qarv_base
    python scripts/lvae-codec.py encode --synthetic 3 IMAGES/ BITS/ -m qres34m     # seeded weights; writes N seeded PNGs to IMAGES/ first

Images whose sizes padded to the model's stride agree are coded as batches of up to --batch (lvae.evaluation.batch_same_size).  A .bits
file is what compress_file writes; decode names every PNG after its .bits file.  --synthetic (on decode: seeded weights only) needs no
checkpoint on disk."""
import argparse
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lossy-vae_amd'))
import torch  # noqa: E402
from lvae.evaluation import batch_same_size, padded_pixels  # noqa: E402
from lvae.models.registry import get_model  # noqa: E402


def load_model(name, synthetic, device):
    model = get_model(name, pretrained=not synthetic)
    if synthetic:
        import seeded_init
        sd = model.state_dict()
        for k in list(sd):
            a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
            if a is not None and 'discrete_gaussian' not in k:
                sd[k] = torch.from_numpy(a)
        model.load_state_dict(sd)
    model.compress_mode()
    return model.to(device).eval()


def encode(model, src, dst, lmb, batch):
    paths = sorted(p for p in Path(src).iterdir() if p.is_file())
    shapes = [padded_pixels(p, model.max_stride)[1] for p in paths]
    total = 0
    for idxs in batch_same_size(list(range(len(paths))), shapes, max_batch=batch):
        blobs = model.compress_images([paths[i] for i in idxs], **({'lmb': lmb} if lmb is not None else {}))
        for i, blob in zip(idxs, blobs):
            (Path(dst) / (paths[i].stem + '.bits')).write_bytes(blob)
            total += len(blob)
    print(f'encoded {len(paths)} images -> {total} bytes')


def decode(model, src, dst, batch):
    paths = sorted(Path(src).glob('*.bits'))
    for o in range(0, len(paths), batch):                  # decompress_images batches the files of a slice by latent shape itself
        model.decompress_to_files(paths[o:o + batch], [Path(dst) / (p.stem + '.png') for p in paths[o:o + batch]])
    print(f'decoded {len(paths)} files')


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('command', choices=['encode', 'decode'])
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('-m', '--model', type=str, default='qarv_base')
    ap.add_argument('--lmb', type=float, default=None, help='variable-rate models: the lambda to code at (default: the model\'s)')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('-d', '--device', type=str, default='cuda:0')
    ap.add_argument('--synthetic', type=int, default=0, help='seeded weights; on encode also write N seeded 120x180 / 128x192 PNGs to SRC')
    args = ap.parse_args()
    os.makedirs(args.dst, exist_ok=True)
    if args.synthetic and args.command == 'encode':
        import seeded_init
        from lvae.utils.image import save_u8
        os.makedirs(args.src, exist_ok=True)
        for i in range(args.synthetic):
            h, w = ((120, 180), (128, 192))[i % 2]
            save_u8(torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 300 + i)), Path(args.src) / f'im{i:02d}.png')
    model = load_model(args.model, args.synthetic, torch.device(args.device))
    if args.command == 'encode':
        encode(model, args.src, args.dst, args.lmb, args.batch)
    else:
        decode(model, args.src, args.dst, args.batch)


if __name__ == '__main__':
    main()
