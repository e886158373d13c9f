"""MS-SSIM on the HIP kernels (lvae.metrics.ms_ssim) against what a user would otherwise write: the same definition in fp32 torch with
F.conv2d on the same GPU.  Two workloads, both device-resident: 8 x 3 x 512 x 768 pairs, and one 3 x 1408 x 2048 pair.  The two paths
are timed alternately in one process (kernel, torch, kernel, torch, ...), after warm-up steps of both, the device synchronised after
every call; medians.  The codec's own compress_batch + decompress_batch time for the 512 x 768 batch gives the share of an evaluation step.
Prints one JSON line.
    python tools/msssim_bench.py [--steps 20] [--warmup 3] [--no-codec]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

W5 = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_ms_ssim_fp32(x, y):
    """The definition (lvae/metrics.py) evaluated in the inputs' dtype on their device with grouped F.conv2d."""
    c = torch.arange(11, dtype=x.dtype, device=x.device) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 * 1.5))
    g = g / g.sum()
    C = x.shape[1]
    gv, gh = g.view(1, 1, -1, 1).expand(C, 1, -1, 1), g.view(1, 1, 1, -1).expand(C, 1, 1, -1)
    filt = lambda t: F.conv2d(F.conv2d(t, gv, groups=C), gh, groups=C)
    terms = []
    for i in range(5):
        mx, my = filt(x), filt(y)
        sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        cs = (2 * sxy + 9e-4) / (sxx + syy + 9e-4)
        if i < 4:
            terms.append(torch.relu(cs.flatten(2).mean(-1)))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
        else:
            terms.append(torch.relu((((2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)) * cs).flatten(2).mean(-1)))
    return torch.prod(torch.stack(terms, 0) ** torch.tensor(W5, dtype=x.dtype, device=x.device).view(-1, 1, 1), 0).mean(1)


def main():
    import bench
    from lvae.metrics import ms_ssim
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-codec', action='store_true', help='skip the encode + decode row (no model is built)')
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

    res = {'metric': 'ms_ssim_ms', 'steps': args.steps, 'warmup': args.warmup}
    for name, (B, H, W) in {'b8_512x768': (8, 512, 768), 'b1_1408x2048': (1, 1408, 2048)}.items():
        x = bench.synth_batch(B, H, W, 0).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=torch.Generator().manual_seed(0)).to(dev)).clamp(0, 1)
        row = alternate({'hip': lambda: ms_ssim(x, y), 'torch_fp32': lambda: torch_ms_ssim_fp32(x, y)})
        row['torch_over_hip'] = round(row['torch_fp32']['median'] / row['hip']['median'], 2)
        row['max_abs_diff_hip_vs_torch_fp32'] = float((ms_ssim(x, y) - torch_ms_ssim_fp32(x, y).double()).abs().max())
        res[name] = row
    if not args.no_codec:
        model, _ = bench.build_model(dev)
        x = bench.synth_batch(8, 512, 768, 0).to(dev)
        box = {}

        def codec():
            box['y'] = model.decompress_batch(model.compress_batch(x))
        row = alternate({'encode_decode': codec, 'hip': lambda: ms_ssim(x, box['y'])})
        res['eval_step_b8_512x768'] = {'encode_decode_ms': row['encode_decode'], 'ms_ssim_ms': row['hip'],
                                       'ms_ssim_share_of_step': round(row['hip']['median'] / (row['hip']['median'] + row['encode_decode']['median']), 4)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
