#!/usr/bin/env python
"""Folder-to-folder codec: PNGs -> .bits files and back, 8-bit end to end on the GPU (CodecBase.compress_images /
decompress_to_files: the bytes of an image are uploaded as they are, a reconstruction is rounded to bytes before it is copied back).

    python scripts/lvae-codec.py encode IMAGES/ BITS/ -m qarv_base --lmb 256 [--batch 8]
    python scripts/lvae-codec.py decode BITS/ RECON/ -m qarv_base
    python scripts/lvae-codec.py encode --synthetic 3 IMAGES/ BITS/ -m qres34m     # seeded weights; writes N seeded PNGs to IMAGES/ first
    python scripts/lvae-codec.py encode IMAGES/ BITS/ --tile 512 768 --overlap 32   # large images: one tiled container per image
    python scripts/lvae-codec.py region BITS/ CROPS/ --box 100 200 512 512          # y0 x0 h w of every tiled file, nothing else decoded
    python scripts/lvae-codec.py encode IMAGES/ BITS/ --scale 0.5 [--filter bicubic]   # reduced resolution: one scaled container per image
    python scripts/lvae-codec.py decode BITS/ PREVIEWS/ --preview 128 192              # scaled files at H x W instead of their original size
    python scripts/lvae-codec.py encode-yuv IN.yuv BITS/ --size 1920 1080 [--format nv12] [--frames N]   # raw 8-bit 4:2:0: one .bits per frame
    python scripts/lvae-codec.py decode-yuv BITS/ OUT.yuv [--format nv12]
    python scripts/lvae-codec.py encode-yuv IN.yuv BITS/ --size 1920 1080 --depth 10 [--subsampling 422] [--siting left] [--matrix bt2020]
    python scripts/lvae-codec.py decode-yuv BITS/ OUT.yuv --depth 10 [--subsampling 422] [--siting left] [--matrix bt2020]   # yuv420p10le ...
    python scripts/lvae-codec.py encode-yuv IN.yuv OUT.lvys --size 1920 1080 --container [--layout p010] [--siting left] [--matrix bt2020]
    python scripts/lvae-codec.py decode-yuv IN.lvys OUT.yuv [--layout p010]          # no colour flags: the container holds them
    python scripts/lvae-codec.py encode-yuv IN.yuv BITS/ --size 3840 2160 --depth 10 --tile 512 768 --overlap 32 [--container]   # frames in tiles
    python scripts/lvae-codec.py encode-yuv IN.yuv BITS/ --size 3840 2160 --depth 10 --scale 0.5 [--filter bicubic] [--container]   # frames at reduced resolution
    python scripts/lvae-codec.py decode-yuv BITS/ OUT.yuv --depth 10 [--preview 540 960]   # scaled frames: recognised by their magic
    python scripts/lvae-codec.py eval-yuv IN.yuv --size 1920 1080 [--depth 10 | --layout p010 ...] [--ssim] [--ms-ssim]   # bpp, PSNR-YUV, SSIM as JSON
    python scripts/lvae-codec.py ratemap IMAGES/ MAPS/ -m qarv_base [--lmb 256]      # where the bits go: <stem>.npy + <stem>.png per image

Images whose sizes padded to the model's stride agree are coded as batches of up to --batch (lvae.evaluation.batch_same_size).  A .bits
file is what compress_file writes; decode names every PNG after its .bits file.  --synthetic (on decode: seeded weights only) needs no
checkpoint on disk.  With --tile every image is coded on its own as a tiled container (CodecBase.compress_tiled: tiles of one shape, coded
--batch at a time, whatever the image's size); decode recognises such files by their magic, region decodes only the tiles a box touches.
With --scale every image is resampled on the device, coded at S times its size and wrapped in a scaled container
(CodecBase.compress_scaled, lvae/utils/resample.py); decode recognises these by their magic too and writes PNGs of the ORIGINAL size, or
of --preview H W.  --scale and --tile exclude each other.
encode-yuv / decode-yuv code the frames of a raw .yuv file as an intra-frame coder (CodecBase.compress_yuv420 / decompress_yuv420): frame
k becomes BITS/frame<k>.bits, a file compress_file could have written; --matrix / --range / --chroma are NOT stored, give decode-yuv the
same --matrix and --range.  With --synthetic N, encode-yuv first writes N seeded frames of --size to IN.yuv.  --depth 10 | 12,
--subsampling 422 | 444, --siting left or --matrix bt2020 select planar files with 16-bit little-endian samples above 8 bits
(CodecBase.compress_yuv / decompress_yuv); none of them is stored either: decode-yuv needs the encoder's --depth and --siting too (it may
ask for another depth or subsampling on purpose: the reconstruction is fp32).  --layout p010 | p012 | p210 | p212: the raw file is
semi-planar with the value in the high bits (what hardware decoders deliver); the name gives depth and subsampling.  --container:
encode-yuv writes ONE self-describing file (CodecBase.compress_yuv_sequence, the LVYS container of lvae/utils/yuvseq.py) instead of a
folder; decode-yuv recognises it by its magic, takes every parameter from its header and writes the source's layout unless --layout
/ --format asks for another.  encode-yuv --tile TH TW [--overlap OV] codes every frame in tiles (CodecBase.compress_yuv_tiled: one tiled
container per frame, as a .bits file or as the frame's entry of the --container file; the overlap is even where the chroma is
subsampled); decode-yuv recognises such frames by their magic and writes the planes straight from the blend of the tiles.
encode-yuv --scale S [--filter F] codes every frame at S times its size (CodecBase.compress_yuv_scaled: one scaled container per frame, as
a .bits file or as the frame's entry of the --container file; not together with --tile); decode-yuv recognises such frames by their magic
and writes them at their original size, or with --preview H W at that size.
eval-yuv codes the frames of a raw file as encode-yuv would (the same --size / --format / --depth / --subsampling / --siting / --layout /
colour flags, --frames, --batch, --lmb; --synthetic N writes seeded frames first), decodes them and prints lvae.evaluation.yuv_evaluate's
dict of means as one JSON line: bpp and the PSNR keys, with --ssim also ssim-y / ssim-u / ssim-v, with --ms-ssim also ms-ssim-y (frames
with min(h, w) > 160 only).  It takes no DST.
ratemap writes, for every image of IMAGES/, the per-pixel bit allocation of the model's rate estimate (lvae.evaluation.rate_map_evaluate:
CodecBase.rate_map on the image's bytes) as MAPS/<stem>.npy (fp32, bits per pixel at each pixel) and a grey MAPS/<stem>.png, and prints
each image's estimated bits and the share of every latent block; nothing is entropy-coded.  --synthetic N writes seeded PNGs first, as encode."""
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


def encode(model, src, dst, lmb, batch, tile=None, overlap=0, scale=None, filt='lanczos3'):
    paths = sorted(p for p in Path(src).iterdir() if p.is_file())
    if scale is not None:
        total = sum(model.compress_file_scaled(p, Path(dst) / (p.stem + '.bits'), scale=scale, filter=filt, lmb=lmb) for p in paths)
        print(f'encoded {len(paths)} images at scale {scale} ({filt}) -> {total} bytes')
        return
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


def _is_scaled(path):
    from lvae.utils.resample import MAGIC
    with open(path, 'rb') as f:
        return f.read(4) == MAGIC


def decode(model, src, dst, batch, box=None, preview=None):
    paths = sorted(Path(src).glob('*.bits'))
    scaled = [p for p in paths if _is_scaled(p)]
    if preview is not None and len(scaled) != len(paths):
        raise SystemExit('--preview: ' + ', '.join(p.name for p in paths if p not in scaled) + ' not coded with --scale')
    if box is not None and scaled:
        raise SystemExit('region: ' + ', '.join(p.name for p in scaled) + ' coded with --scale, not with --tile')
    for p in scaled:
        model.decompress_file_scaled(p, Path(dst) / (p.stem + '.png'), size=preview)
    n_scaled, paths = len(scaled), [p for p in paths if p not in scaled]
    tiled = [p for p in paths if _is_tiled(p)]
    if box is not None and len(tiled) != len(paths):
        raise SystemExit('region: ' + ', '.join(p.name for p in paths if p not in tiled) + ' not coded with --tile')
    for p in tiled:
        model.decompress_file_tiled(p, Path(dst) / (p.stem + '.png'), box=box, max_batch=batch)
    paths = [p for p in paths if p not in tiled]
    for o in range(0, len(paths), batch):                  # decompress_images batches the files of a slice by latent shape itself
        model.decompress_to_files(paths[o:o + batch], [Path(dst) / (p.stem + '.png') for p in paths[o:o + batch]])
    print(f'decoded {len(paths) + len(tiled) + n_scaled} files')


def _is_sequence(path):
    from lvae.utils.yuvseq import MAGIC
    if not os.path.isfile(path):
        return False
    with open(path, 'rb') as f:
        return f.read(4) == MAGIC


def _decode_kw(fmt, colour):
    """What decompress_yuv / decompress_yuv_tiled / from_rgb01_any take: the format and the colour parameters but the encoder's filter."""
    return dict(fmt._asdict(), **{k: v for k, v in colour.items() if k != 'chroma'})


def encode_yuv_container(model, src, dst, size, fmt, frames, lmb, batch, colour, tile=None, overlap=0, scale=None, filt='lanczos3'):
    blob = model.compress_yuv_sequence(src, size[0], size[1], frames=frames, lmb=lmb, max_batch=batch, tile=tile, overlap=overlap,
                                       scale=scale, filter=filt, **fmt._asdict(), **colour)
    Path(dst).write_bytes(blob)
    print(f'encoded {model.yuv_sequence_info(blob)["frames"]} frames -> {len(blob)} bytes')


def decode_yuv_container(model, src, dst, batch, layout=None, preview=None):
    blob = Path(src).read_bytes()
    if preview is not None:                                  # every frame at the preview size: the entries must be scaled containers
        from lvae.utils.resample import is_scaled
        from lvae.utils.yuv import write_frames
        from lvae.utils.yuvseq import unpack_sequence
        info, entries = unpack_sequence(blob)
        if not all(is_scaled(b) for b in entries):
            raise SystemExit('--preview: the sequence was not coded with --scale')
        how = {k: info[k] for k in ('depth', 'subsampling', 'siting', 'matrix', 'range')}
        how['layout'] = info['layout'] if layout is None else layout
        for o in range(0, len(entries), batch):
            write_frames(model.decompress_yuv_scaled(entries[o:o + batch], size=tuple(preview), **how), dst, append=o > 0)
        print(f'decoded {len(entries)} frames at {preview[0]}x{preview[1]}')
        return
    n = model.decompress_yuv_sequence(blob, layout=layout, out_path=dst, max_batch=batch)
    print(f'decoded {n} frames')


def encode_yuv(model, src, dst, size, fmt, frames, lmb, batch, colour, tile=None, overlap=0, scale=None, filt='lanczos3'):
    fs, compress = fmt.read(src, size[0], size[1], frames=frames), model.compress_yuv
    if scale is not None:                                    # a scaled container per frame
        if tile is not None:
            raise SystemExit('encode-yuv: --scale and --tile may not be combined')
        compress = lambda chunk, **kw: model.compress_yuv_scaled(chunk, scale=scale, filter=filt, **kw)
    if tile is not None:                                     # every frame on its own, as a tiled container, its tiles --batch at a time
        compress = lambda chunk, **kw: [model.compress_yuv_tiled(f, tile=tile, overlap=overlap, max_batch=batch, **kw) for f in chunk]
    total = 0
    for o in range(0, len(fs), batch):
        blobs = compress(fs[o:o + batch], **colour, **({'lmb': lmb} if lmb is not None else {}))
        for k, blob in enumerate(blobs, o):
            (Path(dst) / f'frame{k:05d}.bits').write_bytes(blob)
            total += len(blob)
    print(f'encoded {len(fs)} frames -> {total} bytes')


def decode_yuv(model, src, dst, fmt, batch, colour, preview=None):
    from lvae.utils.resample import MAGIC as SCALED_MAGIC
    from lvae.utils.tiling import MAGIC as TILED_MAGIC
    from lvae.utils.yuv import write_frames
    paths, how = sorted(Path(src).glob('*.bits')), _decode_kw(fmt, colour)
    for o in range(0, len(paths), batch):
        blobs = [p.read_bytes() for p in paths[o:o + batch]]
        if preview is not None and not all(b[:4] == SCALED_MAGIC for b in blobs):
            raise SystemExit('--preview: the frames were not coded with --scale')
        if all(b[:4] == SCALED_MAGIC for b in blobs):        # encode-yuv --scale wrote them: one scaled container per frame
            got = model.decompress_yuv_scaled(blobs, size=None if preview is None else tuple(preview), **how)
        elif all(b[:4] == TILED_MAGIC for b in blobs):       # encode-yuv --tile wrote them: one tiled container per frame
            got = [model.decompress_yuv_tiled(b, max_batch=batch, **how) for b in blobs]
        else:
            got = model.decompress_yuv(blobs, **how)
        write_frames(got, dst, append=o > 0)
    print(f'decoded {len(paths)} frames')


def eval_yuv(model, src, size, fmt, frames, lmb, batch, colour, metrics=('psnr',)):
    import json
    from lvae.evaluation import yuv_evaluate
    res = yuv_evaluate(model, src, size[0], size[1], fmt=fmt, max_frames=frames, batch=batch, lmb=lmb, metrics=metrics, **colour)
    print(json.dumps(res))
    return res


def synthetic_yuv(path, n, size, fmt, colour):
    """N seeded frames of size (w, h) as a raw .yuv file: seeded RGB images through the defining host conversion."""
    import seeded_init
    from lvae.utils.yuv import from_rgb01_any, write_frames
    w, h = size
    rgb = [torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 300 + i)).permute(2, 0, 1).float().div(255) for i in range(n)]
    write_frames(from_rgb01_any(rgb, **_decode_kw(fmt, colour)), path)


def ratemap(model, src, dst, lmb):
    from lvae.evaluation import rate_map_evaluate
    rows = rate_map_evaluate(model, src, out_dir=dst, lmb=lmb)
    for r in rows:
        print(f"{r['name']}: {r['bits']:.1f} bits; blocks " + ' '.join(f'{100 * v:.1f}%' for v in r['shares']))
    print(f"mapped {len(rows)} images -> {sum(r['bits'] for r in rows):.1f} estimated bits")
    return rows


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('command', choices=['encode', 'decode', 'region', 'encode-yuv', 'decode-yuv', 'eval-yuv', 'ratemap'])
    ap.add_argument('src')
    ap.add_argument('dst', nargs='?', default=None, help='every command but eval-yuv')
    ap.add_argument('-m', '--model', type=str, default='qarv_base')
    ap.add_argument('--lmb', type=float, default=None, help='variable-rate models: the lambda to code at (default: the model\'s)')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('-d', '--device', type=str, default='cuda:0')
    ap.add_argument('--tile', type=int, nargs=2, default=None, metavar=('TH', 'TW'), help='encode / encode-yuv: code every image (frame) in tiles of this size')
    ap.add_argument('--overlap', type=int, default=0, help='encode with --tile: pixels neighbouring tiles share')
    ap.add_argument('--scale', type=float, default=None, help='encode / encode-yuv: code every image (frame) at SCALE times its size (a scaled container each)')
    ap.add_argument('--filter', type=str, default='lanczos3', choices=['bilinear', 'bicubic', 'lanczos3'], help='encode with --scale: the resampling filter')
    ap.add_argument('--preview', type=int, nargs=2, default=None, metavar=('H', 'W'), help='decode / decode-yuv: write scaled files (frames) at this size')
    ap.add_argument('--box', type=int, nargs=4, default=None, metavar=('Y0', 'X0', 'H', 'W'), help='region: the window to decode')
    ap.add_argument('--synthetic', type=int, default=0, help='seeded weights; on encode / ratemap also write N seeded 120x180 / 128x192 PNGs to SRC')
    ap.add_argument('--size', type=int, nargs=2, default=None, metavar=('W', 'H'), help='encode-yuv: the frame size of the raw file')
    ap.add_argument('--format', type=str, default='i420', choices=['i420', 'nv12'], help='encode-yuv / decode-yuv: the plane layout of the raw file')
    ap.add_argument('--frames', type=int, default=None, help='encode-yuv: code only the first N frames')
    ap.add_argument('--matrix', type=str, default='bt709', choices=['bt601', 'bt709', 'bt2020'])
    ap.add_argument('--depth', type=int, default=8, choices=[8, 10, 12], help='encode-yuv / decode-yuv: bits per sample (above 8: 16-bit little-endian words)')
    ap.add_argument('--subsampling', type=str, default='420', choices=['420', '422', '444'], help='encode-yuv / decode-yuv: the chroma subsampling')
    ap.add_argument('--siting', type=str, default='center', choices=['center', 'left'], help="encode-yuv / decode-yuv: where the chroma samples lie; 'left' is H.264 / HEVC co-sited chroma")
    ap.add_argument('--range', type=str, default='limited', choices=['limited', 'full'])
    ap.add_argument('--chroma', type=str, default='bilinear', choices=['nearest', 'bilinear'], help='encode-yuv: the chroma upsampling filter')
    ap.add_argument('--layout', type=str, default=None, choices=['p010', 'p012', 'p210', 'p212'],
                    help='encode-yuv / decode-yuv: the raw file is semi-planar with the value in the high bits; sets --depth and --subsampling')
    ap.add_argument('--ssim', action='store_true', help='eval-yuv: also report ssim-y / ssim-u / ssim-v')
    ap.add_argument('--ms-ssim', action='store_true', help='eval-yuv: also report ms-ssim-y')
    ap.add_argument('--container', action='store_true', help='encode-yuv: write one self-describing .lvys file to DST instead of a folder of .bits files')
    return ap


@torch.no_grad()
def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if (args.dst is None) != (args.command == 'eval-yuv'):
        ap.error('eval-yuv takes IN.yuv alone' if args.dst is not None else f'{args.command} needs SRC and DST')
    if args.command in ('encode-yuv', 'decode-yuv', 'eval-yuv'):
        if args.command == 'decode-yuv' and _is_sequence(args.src):      # every parameter comes from the container's header
            model = load_model(args.model, args.synthetic, torch.device(args.device))
            decode_yuv_container(model, args.src, args.dst, args.batch,
                                 'semiplanar' if args.layout else args.format if args.format != 'i420' else None, args.preview)
            return
        from lvae.utils.yuv import SP_LAYOUTS, FrameFormat
        colour = dict(matrix=args.matrix, range=args.range, chroma=args.chroma, siting=args.siting)
        layout = args.format                                 # Yuv420Frames, the 8-bit 4:2:0 centre-sited path, unless one option asks for more
        if args.layout is not None:
            if args.format != 'i420':
                ap.error('--layout and --format nv12 exclude each other')
            layout, (args.depth, args.subsampling) = 'semiplanar', SP_LAYOUTS[args.layout]
        elif (args.depth, args.subsampling, args.siting) != (8, '420', 'center') or args.matrix == 'bt2020':
            if args.format != 'i420':
                ap.error('--depth / --subsampling / --siting / --matrix bt2020 apply to planar files (--format i420)')
            layout = 'planar'
        fmt = FrameFormat(layout, args.depth, args.subsampling, args.siting, args.matrix)
        if args.command == 'eval-yuv':
            if args.size is None:
                ap.error('eval-yuv needs --size W H')
            if args.synthetic:
                synthetic_yuv(args.src, args.synthetic, args.size, fmt, colour)
            model = load_model(args.model, args.synthetic, torch.device(args.device))
            eval_yuv(model, args.src, args.size, fmt, args.frames, args.lmb, args.batch, colour,
                     ('psnr',) + (('ssim',) if args.ssim else ()) + (('ms-ssim',) if args.ms_ssim else ()))
        elif args.command == 'encode-yuv':
            if args.size is None:
                ap.error('encode-yuv needs --size W H')
            if not args.container:
                os.makedirs(args.dst, exist_ok=True)
            if args.synthetic:
                synthetic_yuv(args.src, args.synthetic, args.size, fmt, colour)
            model = load_model(args.model, args.synthetic, torch.device(args.device))
            (encode_yuv_container if args.container else encode_yuv)(model, args.src, args.dst, args.size, fmt, args.frames, args.lmb, args.batch, colour,
                                                                     tuple(args.tile) if args.tile else None, args.overlap, args.scale,
                                                                     args.filter)
        else:
            model = load_model(args.model, args.synthetic, torch.device(args.device))
            decode_yuv(model, args.src, args.dst, fmt, args.batch, colour, args.preview)
        return
    os.makedirs(args.dst, exist_ok=True)
    if args.synthetic and args.command in ('encode', 'ratemap'):
        import seeded_init
        from lvae.utils.image import save_u8
        os.makedirs(args.src, exist_ok=True)
        for i in range(args.synthetic):
            h, w = ((120, 180), (128, 192))[i % 2]
            save_u8(torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 300 + i)), Path(args.src) / f'im{i:02d}.png')
    model = load_model(args.model, args.synthetic, torch.device(args.device))
    if args.command == 'ratemap':
        ratemap(model, args.src, args.dst, args.lmb)
        return
    if args.command == 'region' and args.box is None:
        ap.error('region needs --box y0 x0 h w')
    if args.scale is not None and args.tile:
        ap.error('--scale and --tile exclude each other')
    if args.command == 'encode':
        encode(model, args.src, args.dst, args.lmb, args.batch, tuple(args.tile) if args.tile else None, args.overlap, args.scale, args.filter)
    else:
        decode(model, args.src, args.dst, args.batch, tuple(args.box) if args.command == 'region' else None,
               tuple(args.preview) if args.preview and args.command == 'decode' else None)


if __name__ == '__main__':
    main()
