"""tests/golden/make_golden_eval_forward.py -- fixtures of the eval-mode forward pass, `model(im)` (build container only).

Runs the reference's models on the CPU with seeded weights (through make_golden's helpers) in eval mode and records, at 64x128:
for qres34m, qres17m and qres34m_lossless one image, for qarv_base a batch of two images at lambda = (64, 1024): the statistics
model(im, return_rec=True) returns, the per-block per-image kl sums (nats), the `_stats_log` channel bpps (QRes-VAE), the decoder's
output before the clamp (x_hat; the lossless model's pixel mean) and im_hat.  Eval mode quantises every latent, so the fixtures do not
depend on torch's RNG.  Run:  python tests/golden/make_golden_eval_forward.py
"""
import os

import numpy as np
import torch

import make_golden as mg

H, W = 64, 128
QRES_IMG_SEED = 4
QARV_IMG_SEEDS = (4, 7)
QARV_LMBS = (64.0, 1024.0)
STAT_KEYS = ('loss', 'kl', 'mse', 'nll', 'bppix', 'psnr')


def f32(x):
    return mg.npf(x).astype(np.float32)


def record_symbols(model):
    """Wrap every latent block's entropy model so that each eval-mode call records its symbols round(qm - pm) (CompressAI's
    'dequantize' quantisation) in call order, i.e. block order."""
    syms = []
    for blk in model.modules():
        dg = getattr(blk, 'discrete_gaussian', None)
        if dg is None or getattr(dg, '_recording', False):
            continue
        orig = dg.forward

        def fwd(inputs, scales, means=None, _orig=orig):
            syms.append(mg.npf(torch.round(inputs - means)).astype(np.int32))
            return _orig(inputs, scales, means=means)
        dg.forward, dg._recording = fwd, True
    return syms


@torch.no_grad()
def golden_qres(name):
    model = mg.lvae.get_model(name)
    mg.load_seeded(model, 0)
    model.eval()
    im, _ = mg.image_tensor(H, W, QRES_IMG_SEED)
    syms = record_symbols(model)
    stats = model(im, return_rec=True)
    out = {'hw': np.array([H, W]), 'img_seed': np.array(QRES_IMG_SEED)}
    for k in STAT_KEYS:
        if k in stats:
            out[f'stat.{k}'] = np.array(float(stats[k]))
    out['im_hat'] = f32(stats['im_hat'])
    for i, sy in enumerate(syms):
        assert np.abs(sy).max() < 128
        out[f'sym{i}'] = sy.astype(np.int8)
    del syms[:]
    chans = model._stats_log['eval_channels']
    for i, c in enumerate(chans):
        out[f'chan{i}'] = np.array(c, dtype=np.float64)
    # the pieces of forward() (qresvae/model.py:539-546): per-block kl sums and the out net's x_hat before the clamp
    x = model.preprocess_input(im)
    feature, stats_all = model.decoder(model.encoder(x))
    _, x_hat = model.out_net.forward_loss(feature, model.preprocess_target(im))
    out['kl_sums'] = np.array([mg.npf(st['kl'].double().sum(dim=(1, 2, 3))) for st in stats_all])          # [block][image]
    out['x_hat'] = f32(x_hat)
    assert np.array_equal(out['im_hat'], f32(model.process_output(x_hat)))
    print(name, {k: round(float(v), 5) for k, v in out.items() if k.startswith('stat.')})
    save(out, f'{name}_{H}x{W}_eval_forward.npz')


@torch.no_grad()
def golden_qarv():
    model = mg.lvae.get_model('qarv_base')
    mg.load_seeded(model, 0)
    model.eval()
    im = torch.cat([mg.image_tensor(H, W, s)[0] for s in QARV_IMG_SEEDS])
    lmb = torch.tensor(QARV_LMBS)
    syms = record_symbols(model)
    stats = model(im, lmb=lmb, return_rec=True)
    out = {'hw': np.array([H, W]), 'img_seeds': np.array(QARV_IMG_SEEDS), 'lmbs': np.array(QARV_LMBS)}
    for k in STAT_KEYS:
        if k in stats:
            out[f'stat.{k}'] = np.array(float(stats[k]))
    out['im_hat'] = f32(stats['im_hat'])
    for i, sy in enumerate(syms):
        assert np.abs(sy).max() < 128
        out[f'sym{i}'] = sy.astype(np.int8)
    del syms[:]
    x_hat, stats_all = model.forward_end2end(im, lmb)
    out['kl_sums'] = np.array([mg.npf(st['kl'].double().sum(dim=(1, 2, 3))) for st in stats_all])           # [block][image]
    out['x_hat'] = f32(x_hat)
    assert np.array_equal(out['im_hat'], f32(model.process_output(x_hat)))
    print('qarv_base', {k: round(float(v), 5) for k, v in out.items() if k.startswith('stat.')})
    save(out, f'qarv_base_{H}x{W}_eval_forward.npz')


def save(out, fname):
    path = os.path.join(mg.OUT, fname)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    for name in ('qres34m', 'qres17m', 'qres34m_lossless'):
        golden_qres(name)
    golden_qarv()
