"""Mixed-lambda batches against the alternatives: 8 seeded 512x768 images, 8 distinct lambdas log-spaced over lmb_range, default arithmetic.
  (i)   sequential: 8 x (compress + decompress), one image and one lambda each
  (ii)  mixed:      one compress_batch + one decompress_batch with the lambda list
  (iii) shared:     the same batch at ONE lambda (what the batch path could do before)
and forward() with 8 sampled lambdas.  Protocol of bench.py's speed test: warm-up steps, the device synchronised after each phase,
median of the timed steps.  Prints one JSON line.
    python tools/lmb_batch_bench.py [--steps 20] [--warmup 3] [--forward-only]"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'lossy-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--forward-only', action='store_true', help='only the forward() row (also runs on trees without per-image lambdas)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    model, _ = bench.build_model(dev)
    B = args.batch
    x = bench.synth_batch(B, args.height, args.width, 0).to(dev)
    lo, hi = model.lmb_range
    lmbs = [float(np.float32(math.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * i / (B - 1)))) for i in range(B)]

    def timed(fn):
        for _ in range(args.warmup):
            fn(); torch.cuda.synchronize(dev)
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn(); torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3), round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)

    def phases(enc, dec):
        """-> (enc ms, dec ms): median / min / max each; the decode is timed on the strings of the last encode."""
        box = {}

        def e():
            box['s'] = enc()
        te = timed(e)
        td = timed(lambda: dec(box['s']))
        return te, td

    res = {'metric': 'mixed_lambda_batch_ms', 'batch': B, 'height': args.height, 'width': args.width, 'steps': args.steps, 'warmup': args.warmup,
           'precision': model._prec, 'lambdas': [round(v, 3) for v in lmbs]}
    torch.manual_seed(0)
    sampled = model.sample_lmb(B)
    res['forward_sampled_lmb_ms'] = dict(zip(('median', 'min', 'max'), timed(lambda: model(x, lmb=sampled))))
    if not args.forward_only:
        rows = {}
        rows['sequential'] = phases(lambda: [model.compress(x[i:i + 1], lmbs[i]) for i in range(B)], lambda ss: [model.decompress(s) for s in ss])
        rows['mixed'] = phases(lambda: model.compress_batch(x, lmbs), model.decompress_batch)
        rows['shared'] = phases(lambda: model.compress_batch(x, lmbs[-1]), model.decompress_batch)
        assert model.compress_batch(x, lmbs) == [model.compress(x[i:i + 1], lmbs[i]) for i in range(B)]
        for k, (te, td) in rows.items():
            res[k] = {'enc_ms': dict(zip(('median', 'min', 'max'), te)), 'dec_ms': dict(zip(('median', 'min', 'max'), td)),
                      'ms': round(te[0] + td[0], 3)}
        res['mixed_over_sequential'] = round(res['mixed']['ms'] / res['sequential']['ms'], 4)
        res['mixed_over_shared'] = round(res['mixed']['ms'] / res['shared']['ms'], 4)
        # the cost that is new in (ii): the three batched embedding launches for 8 lambdas (the cache is defeated by alternating two lists)
        alt = [lmbs, lmbs[::-1]]
        it = [0]

        def emb():
            it[0] += 1
            model._set_lmb(alt[it[0] % 2])
        res['set_lmb_8_ms'] = dict(zip(('median', 'min', 'max'), timed(emb)))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
