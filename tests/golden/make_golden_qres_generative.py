"""tests/golden/make_golden_qres_generative.py -- fixtures of the QRes-VAE generative API (build container only).

Runs the reference's HierarchicalVAE on the CPU with seeded weights (through make_golden's helpers) and records, for qres34m
and qres34m_lossless at 64x128: forward_get_latents (z and per-block kl sums), cond_sample at t = 0 for a few progressive
anchors, uncond_sample((1, 1, 2), 0), cond_sample(all z, 0, paint_box) and inpaint(masked image, box, steps=2, 0).  Everything
is at temperature 0, so the fixtures do not depend on torch's RNG.  Run:  python tests/golden/make_golden_qres_generative.py
"""
import os

import numpy as np
import torch

import make_golden as mg

H, W, IMG_SEED = 64, 128, 4
KEEPS = (1, 3, 6, 12)                         # progressive anchors: the first `keep` latents given, the rest at the prior mean
PAINT_BOX = (0.25, 0.25, 0.75, 0.75)
INPAINT_BOX = (0.4, 0.4, 0.8, 0.8)


def masked(im, box):
    x1, y1, x2, y2 = box
    _, _, h, w = im.shape
    out = im.clone()
    out[:, :, round(y1 * h):round(y2 * h), round(x1 * w):round(x2 * w)] = 0.0
    return out


@torch.no_grad()
def golden_generative(name):
    model = mg.lvae.get_model(name)
    mg.load_seeded(model, 0)
    model.eval()
    im, _ = mg.image_tensor(H, W, IMG_SEED)
    stats = model.forward_get_latents(im)
    zs = [st['z'] for st in stats]
    out = {'hw': np.array([H, W]), 'img_seed': np.array(IMG_SEED), 'keeps': np.array(KEEPS),
           'paint_box': np.array(PAINT_BOX), 'inpaint_box': np.array(INPAINT_BOX),
           'kl_sums': np.array([float(st['kl'].double().sum()) for st in stats])}
    for i, z in enumerate(zs):
        out[f'z{i}'] = mg.npf(z).astype(np.float32)
    f32 = lambda x: mg.npf(x).astype(np.float32)  # noqa: E731
    for k in KEEPS:
        latents = [z if i < k else None for i, z in enumerate(zs)]
        out[f'x_keep{k}'] = f32(model.cond_sample(latents, nhw_repeat=(1, H // 64, W // 64), temprature=0.0))
    out['x_uncond_t0'] = f32(model.uncond_sample((1, H // 64, W // 64), temprature=0.0))
    out['x_paint_t0'] = f32(model.cond_sample(zs, temprature=0.0, paint_box=PAINT_BOX))
    out['x_inpaint_t0'] = f32(model.inpaint(masked(im, INPAINT_BOX), INPAINT_BOX, steps=2, temprature=0.0))
    diff = float((out['x_paint_t0'] - out[f'x_keep{len(zs)}']).__abs__().max())
    print(name, 'kl sums (nats)', np.round(out['kl_sums'], 2).tolist(), 'paint_box moves the sample by up to', diff)
    path = os.path.join(mg.OUT, f'{name}_{H}x{W}_generative.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    golden_generative('qres34m')
    golden_generative('qres34m_lossless')
