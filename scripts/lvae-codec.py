#!/usr/bin/env python
"""Folder-to-folder codec: PNGs -> .bits files and back, 8-bit end to end on the GPU (CodecBase.compress_images /
decompress_to_files: the bytes of an image are uploaded as they are, a reconstruction is rounded to bytes before it is copied back).

    python scripts/lvae-codec.py encode IMAGES/ BITS/ -m qarv_base --lmb 256 [--batch 8]
    python scripts/lvae-codec.py decode BITS/ RECON/ -m qarv_base
    python scripts/lvae-codec.py encode --synthetic 3 IMAGES/ BITS/ -m qres34m     # seeded weights; writes N seeded PNGs to IMAGES/ first
    python scripts/lvae-codec.py encode IMAGES/ BITS/ --tile 512 768 --overlap 32   # large images: one tiled container per image
    python scripts/lvae-codec.py region BITS/ CROPS/ --box 100 200 512 512          # y0 x0 h w of every tiled file, nothing else decoded

Images whose sizes padded to the model's stride agree are coded as batches of up to --batch (lvae.evaluation.batch_same_size).  A .bits
file is what compress_file writes; decode names every PNG after its .bits file.  --synthetic (on decode: seeded weights only) needs no
checkpoint on disk.  With --tile every image is coded on its own as a tiled container (CodecBase.compress_tiled: tiles of one shape, coded
--batch at a time, whatever the image's size); decode recognises such files by their magic, region decodes only the tiles a box touches."""
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


def encode(model, src, dst, lmb, batch, tile=None, overlap=0):
    paths = sorted(p for p in Path(src).iterdir() if p.is_file())
    if tile is not None:
        total = sum(model.compress_file_tiled(p, Path(dst) / (p.stem + '.bits'), tile=tile, overlap=overlap, lmb=lmb, max_batch=batch)
                    for p in paths)
        print(f'encoded {len(paths)} images in tiles of {tile[0]}x{tile[1]} -> {total} bytes')
        return
    shapes = [padded_pixels(p, model.max_stride)[1] for p in paths]
    total = 0
    for idxs in batch_same_size(list(range(len(paths))), shapes, max_batch=batch):
        blobs = model.compress_images([paths[i] for i in idxs], **({'lmb': lmb} if lmb is not None else {}))
        for i, blob in zip(idxs, blobs):
            (Path(dst) / (paths[i].stem + '.bits')).write_bytes(blob)
            total += len(blob)
    print(f'encoded {len(paths)} images -> {total} bytes')


def _is_tiled(path):
    from lvae.utils.tiling import MAGIC
    with open(path, 'rb') as f:
        return f.read(4) == MAGIC


def decode(model, src, dst, batch, box=None):
    paths = sorted(Path(src).glob('*.bits'))
    tiled = [p for p in paths if _is_tiled(p)]
    if box is not None and len(tiled) != len(paths):
        raise SystemExit('region: ' + ', '.join(p.name for p in paths if p not in tiled) + ' not coded with --tile')
    for p in tiled:
        model.decompress_file_tiled(p, Path(dst) / (p.stem + '.png'), box=box, max_batch=batch)
    paths = [p for p in paths if p not in tiled]
    for o in range(0, len(paths), batch):                  # decompress_images batches the files of a slice by latent shape itself
        model.decompress_to_files(paths[o:o + batch], [Path(dst) / (p.stem + '.png') for p in paths[o:o + batch]])
    print(f'decoded {len(paths) + len(tiled)} files')


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('command', choices=['encode', 'decode', 'region'])
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('-m', '--model', type=str, default='qarv_base')
    ap.add_argument('--lmb', type=float, default=None, help='variable-rate models: the lambda to code at (default: the model\'s)')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('-d', '--device', type=str, default='cuda:0')
    ap.add_argument('--tile', type=int, nargs=2, default=None, metavar=('TH', 'TW'), help='encode: code every image in tiles of this size')
    ap.add_argument('--overlap', type=int, default=0, help='encode with --tile: pixels neighbouring tiles share')
    ap.add_argument('--box', type=int, nargs=4, default=None, metavar=('Y0', 'X0', 'H', 'W'), help='region: the window to decode')
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
    if args.command == 'region' and args.box is None:
        ap.error('region needs --box y0 x0 h w')
    if args.command == 'encode':
        encode(model, args.src, args.dst, args.lmb, args.batch, tuple(args.tile) if args.tile else None, args.overlap)
    else:
        decode(model, args.src, args.dst, args.batch, tuple(args.box) if args.command == 'region' else None)


if __name__ == '__main__':
    main()
