#!/usr/bin/env python
"""Measurements of tiled coding (README, "Tiled coding"): the stitch kernel against the same definition written with torch ops, tiled
against whole-image encode + decode, and region decode against a full decode -- all on qarv_base with SEEDED weights (byte counts say
nothing about trained models) and a 2048 x 3072 seeded image.

    python tools/tiled_bench.py [--reps 7] [--skip-codec]

Variants alternate inside every repetition (A B A B ...), each timed with HIP events after warm-up; the figures are medians with the
min .. max spread of the repetitions."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'lossy-vae_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lvae.utils import tiling  # noqa: E402
from lvae.utils.image import stitch_tiles  # noqa: E402

DEV = 'cuda:0'
H, W, TH, TW = 2048, 3072, 512, 768


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ts):
    return f'{statistics.median(ts):9.3f} ms  (min {min(ts):.3f} .. max {max(ts):.3f}, n={len(ts)})'


def torch_stitch(tiles, wts, ys, xs, h, w, u8):
    """The definition with torch ops: per-tile weighted accumulate into a canvas, divide, round."""
    acc = torch.zeros(3, h, w, device=DEV)
    den = torch.zeros(h, w, device=DEV)
    k = 0
    for oy in ys:
        for ox in xs:
            acc[:, oy:oy + TH, ox:ox + TW] += wts[k] * tiles[k]
            den[oy:oy + TH, ox:ox + TW] += wts[k]
            k += 1
    out = acc / den
    if u8:
        return torch.round(out.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    return out.unsqueeze(0)


def bench_stitch(reps):
    print(f'== stitch kernel vs torch ops, {H}x{W} from {TH}x{TW} tiles')
    g = torch.Generator().manual_seed(1)
    for ov in (0, 32):
        ys, xs = tiling.tile_grid(H, W, TH, TW, ov)
        n = len(ys) * len(xs)
        tiles = [torch.rand(3, TH, TW, generator=g).to(DEV) for _ in range(n)]
        wts = [torch.from_numpy(np.outer(tiling.axis_weights(H, TH, ov, oy)[oy:oy + TH], tiling.axis_weights(W, TW, ov, ox)[ox:ox + TW])).to(DEV)
               for oy in ys for ox in xs]
        for form in ('u8', 'f32'):
            k = lambda: stitch_tiles(tiles, H, W, TH, TW, ov, out=form)
            t = lambda: torch_stitch(tiles, wts, ys, xs, H, W, form == 'u8')
            a, b = k(), t()
            diff = (a.float() - b.float()).abs().max().item()
            for _ in range(3):
                k(); t()
            tk, tt = [], []
            for _ in range(reps):
                tk.append(timed(k)[0]); tt.append(timed(t)[0])
            moved = n * 3 * TH * TW * 4 + H * W * 3 * (1 if form == 'u8' else 4)      # tiles read once + the image written once
            print(f'ov={ov:2d} {form}: {n} tiles  max|kernel - torch| = {diff:g}')
            print(f'   kernel {summary(tk)}   {moved / statistics.median(tk) / 1e6:8.1f} GB/s effective')
            print(f'   torch  {summary(tt)}')


def load_model():
    import seeded_init
    from lvae.models.registry import get_model
    m = get_model('qarv_base', pretrained=False)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m.compress_mode()
    return m.to(DEV).eval()


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t, out = timed(fn)
    return t, out, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_codec(reps):
    import seeded_init
    print(f'== qarv_base (seeded weights: byte counts are NOT those of a trained model), {H}x{W}, encode + decode')
    m = load_model()
    img = torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 5)).to(DEV)
    variants = {
        'whole': (lambda: m.compress_images([img])[0], lambda b: m.decompress_images([b])[0]),
        'tiled ov=0': (lambda: m.compress_tiled(img, tile=(TH, TW), overlap=0, max_batch=8), lambda b: m.decompress_tiled(b, max_batch=8)),
        'tiled ov=32': (lambda: m.compress_tiled(img, tile=(TH, TW), overlap=32, max_batch=8), lambda b: m.decompress_tiled(b, max_batch=8)),
    }
    rows = {k: dict(enc=[], dec=[], mem_e=[], mem_d=[]) for k in variants}
    blobs = {}
    for name, (enc, dec) in variants.items():          # warm-up: plans recorded, allocator primed
        blobs[name] = enc()
        dec(blobs[name])
    for _ in range(reps):
        for name, (enc, dec) in variants.items():
            te, b, me = peak(enc)
            td, _, md = peak(lambda: dec(b))
            r = rows[name]
            r['enc'].append(te); r['dec'].append(td); r['mem_e'].append(me); r['mem_d'].append(md)
    for name, r in rows.items():
        print(f'{name:12s} {len(blobs[name]):9d} bytes ({len(blobs[name]) / len(blobs["whole"]):.4f} of whole)')
        print(f'   encode {summary(r["enc"])}   peak {max(r["mem_e"]):8.1f} MiB above the resident set')
        print(f'   decode {summary(r["dec"])}   peak {max(r["mem_d"]):8.1f} MiB above the resident set')
    print('== region decode, 512x512 box at (700, 1100), against the full decode')
    for name in ('tiled ov=0', 'tiled ov=32'):
        b = blobs[name]
        box = (700, 1100, 512, 512)
        info = tiling.unpack_tiled(b)
        touched = len(tiling.tiles_in_box(info['ys'], info['xs'], TH, TW, box))
        full, reg = lambda: m.decompress_tiled(b), lambda: m.decompress_region(b, box)
        assert torch.equal(reg(), full()[700:1212, 1100:1612])
        tf, tr = [], []
        for _ in range(reps):
            tf.append(timed(full)[0]); tr.append(timed(reg)[0])
        print(f'{name}: {touched} of {info["rows"] * info["cols"]} tiles touched')
        print(f'   full   {summary(tf)}')
        print(f'   region {summary(tr)}   ratio {statistics.median(tr) / statistics.median(tf):.3f} (tiles {touched / (info["rows"] * info["cols"]):.3f})')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-codec', action='store_true')
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    bench_stitch(args.reps)
    if not args.skip_codec:
        with torch.no_grad():
            bench_codec(args.reps)


if __name__ == '__main__':
    main()
