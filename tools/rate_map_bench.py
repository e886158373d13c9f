"""Time model.rate_map against the torch composition a user had before it: lvae_gaussian_nll_map_f32 per latent block into a
(B, z, h, w) tensor, .sum(1), repeat_interleave to the image size, scale, add.

    python tools/rate_map_bench.py [--calls 20] [--warmup 3] > profiles/<name>.txt        (on the GPU)

Both variants run the same position plan on the same GPU (the torch one launches the per-element kernel where rate_map launches the
position kernel; both stop behind the last block's) and end with one synchronisation; they alternate call by call; the figures are
medians of --calls synchronised calls after --warmup calls of each.  Before any timing the two maps are asserted torch.equal.  Cases: qarv_base at 8 x 512 x 768 and qres34m
at 2 x 1408 x 2048, seeded weights and seeded images.  One JSON line per case."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lossy-vae_amd'))
import torch  # noqa: E402

CASES = (('qarv_base', 8, 512, 768), ('qres34m', 2, 1408, 2048))


def load_model(name, device):
    import seeded_init
    from lvae.models.registry import get_model
    model = get_model(name, pretrained=False)
    sd = model.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    model.load_state_dict(sd)
    model.compress_mode()
    return model.to(device).eval()


@torch.no_grad()
def torch_rate_map(model, im):
    """rate_map(im) the old way: the plan's launches with the per-element kernel behind each quantize, the rest in torch (fp64, the
    definition's block order; the channel sum is torch's)."""
    from lvae import _native
    B, _, H, W = im.shape
    log2e = model.LOG2E
    if model.variable_rate:
        lmb = model._lmb_arg(None, B)
        model._prepare(); model._set_lmb(lmb)
        pl, cdf_form = model._plan('encp', B, H, W), 0
        model._use_lmb(pl)
    else:
        model._ensure_tables(); model._prepare()
        pl, cdf_form = model._plan('evalp', B, H, W), 1
        assert not pl.lossless
    pl.im.view(B, 3, H, W).copy_(im)
    st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
    acc = torch.zeros(B, H, W, dtype=torch.float64, device=pl.device)
    lo = 0
    for li, cut in enumerate(pl.qcuts):
        pl.run(lo, cut)
        lo = cut
        (z, hw), (h, w) = pl.lat_shapes[li], pl.lat_hw[li]
        kl = torch.empty(B, z, h, w, device=pl.device)
        _native.check(pl.lib.lvae_gaussian_nll_map_f32(pl.prm_bufs[li].data_ptr(), pl.sym_all.data_ptr() + 4 * pl.sym_off[li], kl.data_ptr(),
                                                       pl.pk.scale_bound, B, hw, z, cdf_form, st), 'lvae_gaussian_nll_map_f32')
        s = H // h
        acc = acc + kl.double().sum(1).repeat_interleave(s, 1).repeat_interleave(s, 2) * log2e * 2.0 ** (-2 * int(math.log2(s)))
    pl.fetch_status()
    torch.cuda.current_stream(pl.device).synchronize()
    pl.raise_if_flagged(where='in torch_rate_map()')
    return acc.float().unsqueeze(1)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    del out
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('-d', '--device', type=str, default='cuda:0')
    args = ap.parse_args()
    import seeded_init
    dev = torch.device(args.device)
    for name, B, H, W in CASES:
        model = load_model(name, dev)
        im = torch.stack([torch.from_numpy(seeded_init.synthetic_image_u8(H, W, 300 + i)).permute(2, 0, 1).float().div(255) for i in range(B)]).to(dev)
        variants = {'rate_map': lambda: model.rate_map(im), 'torch': lambda: torch_rate_map(model, im)}
        a, b = variants['rate_map'](), variants['torch']()
        torch.cuda.synchronize(dev)
        assert torch.equal(a, b), f'{name}: the two maps differ in {int((a != b).sum())} of {a.numel()} pixels, max |d| {float((a - b).abs().max()):.3e}'
        bits = a.double().sum((1, 2, 3)).tolist()
        del a, b
        for _ in range(args.warmup):
            for fn in variants.values():
                timed(fn, dev)
        ms = {k: [] for k in variants}
        for _ in range(args.calls):
            for k, fn in variants.items():                     # alternating: both see the same clocks and the same neighbours
                ms[k].append(timed(fn, dev))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({'model': name, 'batch': B, 'height': H, 'width': W, 'calls': args.calls, 'warmup': args.warmup, 'equal': True,
                          'rate_map_ms': round(med['rate_map'], 3), 'torch_ms': round(med['torch'], 3),
                          'rate_map_ms_min_max': [round(min(ms['rate_map']), 3), round(max(ms['rate_map']), 3)],
                          'torch_ms_min_max': [round(min(ms['torch']), 3), round(max(ms['torch']), 3)],
                          'torch_over_rate_map': round(med['torch'] / med['rate_map'], 3), 'bpp': [round(v / (H * W), 4) for v in bits]}), flush=True)
        del model, im, variants
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
