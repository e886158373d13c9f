#!/usr/bin/env python
"""The QRes-VAE generative demos (the reference's scripts/qresvae/{progressive-decoding,uncond-sampling,latent-interpolation,
inpainting}.ipynb) as one command line on this package.  Each writes a PNG grid; `progressive` also writes the bpp of every prefix
of latent blocks as JSON.

    python scripts/qresvae/generative-demos.py {progressive,sample,interpolate,inpaint} -m qres34m
        [--image PATH | --synthetic [H W]] [--weights CKPT] [-t TEMPERATURE] [--seed N] [--out DIR]

progressive  encode one image, decode it from its first k latent blocks (the rest at their prior means, t = 0)
sample       uncond_sample: a grid of new images at temperature t
interpolate  linear interpolation between the latents of two images (the second: the first one mirrored)
inpaint      mask a box of the image and fill it in (inpaint, 2 steps)
--synthetic: seeded random-init weights and a seeded synthetic image (no checkpoint needed).
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import lvae  # noqa: E402
import seeded_init  # noqa: E402
from lvae.utils import coding  # noqa: E402


def load_model(name, weights, device):
    model = lvae.get_model(name, pretrained=weights if weights else False)
    if not weights:                                              # no network for checkpoints: seeded random init
        sd = model.state_dict()
        for k in list(sd.keys()):
            a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
            if a is not None:
                sd[k] = torch.from_numpy(a)
        model.load_state_dict(sd)
    return model.to(device).eval()


def load_image(args, model, device):
    if args.image:
        img = coding.pad_divisible_by(Image.open(args.image).convert('RGB'), div=model.max_stride)
        return coding.pil_to_tensor01(img).unsqueeze(0).to(device)
    h, w = args.synthetic
    u8 = seeded_init.synthetic_image_u8(h, w, 0)
    return torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0).to(device)


def save_grid(images, path, ncol):
    """images: list of (3, H, W) tensors in [0, 1] -> one PNG, ncol per row."""
    ims = [x.clamp(0, 1).cpu() for x in images]
    while len(ims) % ncol:
        ims.append(torch.ones_like(ims[0]))
    rows = [torch.cat(ims[r:r + ncol], dim=2) for r in range(0, len(ims), ncol)]
    arr = (torch.cat(rows, dim=1).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
    Image.fromarray(arr).save(path)
    print(path)


@torch.no_grad()
def progressive(model, args, device, out):
    im = load_image(args, model, device)
    nB, _, H, W = im.shape
    stats = model.forward_get_latents(im)
    zs, L = [st['z'] for st in stats], len(stats)
    kl = [float(st['kl'].double().sum()) for st in stats]
    outs, rows = [], []
    for keep in range(L + 1):
        latents = [z if i < keep else None for i, z in enumerate(zs)]
        x = model.cond_sample(latents, nhw_repeat=(nB, H // 64, W // 64), temprature=0.0)
        bpp = sum(kl[:keep]) / (H * W) * math.log2(math.e)
        psnr = -10 * math.log10(max(float((x - im).square().mean()), 1e-12))
        rows.append(dict(keep=keep, bpp=bpp, psnr=psnr))
        outs.append(x[0])
        print(f'keep={keep:2d}  bpp={bpp:.4f}  psnr={psnr:.2f} dB')
    save_grid([im[0]] + outs, os.path.join(out, f'{args.model}-progressive.png'), ncol=min(len(outs) + 1, 7))
    path = os.path.join(out, f'{args.model}-progressive.json')
    with open(path, 'w') as f:
        json.dump(rows, f, indent=1)
    print(path)


@torch.no_grad()
def sample(model, args, device, out):
    n, (h, w) = args.n, args.latent_hw
    x = model.uncond_sample((n, h, w), temprature=args.t, seed=args.seed)
    save_grid(list(x), os.path.join(out, f'{args.model}-samples-t{args.t:g}.png'), ncol=min(n, 4))


@torch.no_grad()
def interpolate(model, args, device, out):
    im1 = load_image(args, model, device)
    im2 = im1.flip(3)
    z1 = [st['z'] for st in model.forward_get_latents(im1)]
    z2 = [st['z'] for st in model.forward_get_latents(im2)]
    outs = []
    for a in np.linspace(0, 1, args.n):
        latents = [(1 - a) * p + a * q for p, q in zip(z1, z2)]
        outs.append(model.cond_sample(latents, temprature=0.0)[0])
    save_grid(outs, os.path.join(out, f'{args.model}-interpolation.png'), ncol=len(outs))


@torch.no_grad()
def inpaint(model, args, device, out):
    im = load_image(args, model, device)
    _, _, H, W = im.shape
    box = tuple(args.box)
    x1, y1, x2, y2 = box
    masked = im.clone()
    masked[:, :, round(y1 * H):round(y2 * H), round(x1 * W):round(x2 * W)] = 0.0
    outs = [im[0], masked[0]]
    for k in range(args.n):
        outs.append(model.inpaint(masked, box, steps=2, temprature=args.t, seed=args.seed + k)[0])
    save_grid(outs, os.path.join(out, f'{args.model}-inpainting-t{args.t:g}.png'), ncol=len(outs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('demo', choices=['progressive', 'sample', 'interpolate', 'inpaint'])
    ap.add_argument('-m', '--model', type=str, default='qres34m', choices=['qres34m', 'qres17m', 'qres34m_lossless'])
    ap.add_argument('--image', type=str, default=None)
    ap.add_argument('--synthetic', type=int, nargs='*', default=None, metavar='H W',
                    help='seeded random-init weights and a seeded synthetic image of H x W (default 128 x 192)')
    ap.add_argument('--weights', type=str, default=None, help='checkpoint (state dict with the reference key names)')
    ap.add_argument('-t', type=float, default=0.5, help='temperature (sample, inpaint)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('-n', type=int, default=4, help='images per grid (sample, inpaint) / interpolation steps')
    ap.add_argument('--latent-hw', type=int, nargs=2, default=[2, 3], help='top latent map of a sample (images of 64h x 64w)')
    ap.add_argument('--box', type=float, nargs=4, default=[0.4, 0.4, 0.8, 0.8], metavar=('X1', 'Y1', 'X2', 'Y2'))
    ap.add_argument('--out', type=str, default='runs')
    args = ap.parse_args()
    if args.synthetic is not None and len(args.synthetic) not in (0, 2):
        ap.error('--synthetic takes no value or H W')
    if args.synthetic is None and not (args.image and args.weights):
        ap.error('give --weights and --image, or --synthetic for seeded weights and a synthetic image')
    args.synthetic = args.synthetic or [128, 192]
    torch.manual_seed(args.seed)
    device = torch.device('cuda:0')
    model = load_model(args.model, args.weights, device)
    os.makedirs(args.out, exist_ok=True)
    {'progressive': progressive, 'sample': sample, 'interpolate': interpolate, 'inpaint': inpaint}[args.demo](model, args, device, args.out)


if __name__ == '__main__':
    main()
