"""-m gpu: MS-SSIM on the HIP kernels (lvae.metrics.ms_ssim -> lvae_msssim_f32) against the fp64 yardstick of tests/test_metrics_host.py,
its independence of batching and padding, and the `metrics` option of the evaluation harness with the real qarv_base.

Bound: 1e-6 absolute on every value and every per-scale mean.  Results are quoted to 4-5 decimals and 1e-6 at 0.99 is 4e-4 dB; a plain fp32
evaluation of the yardstick stays within 1.5e-7 of it on the CPU, so the bound does not hide a wrong formula, and one step of the noise
levels used here moves the value by more than 1e-3 (test_metrics_host.py).  The measured errors are printed (pytest -s) and, when
LVAE_MSSSIM_REPORT names a file, appended to it (profiles/r08_msssim_parity.txt is such a file)."""
import os

import pytest
import torch

from test_metrics_host import image01, ms_ssim_fp64, noisy

pytestmark = pytest.mark.gpu

BOUND = 1e-6
LAMBDAS = (32.0, 1024.0)


def _report(line):
    print(line)
    path = os.environ.get('LVAE_MSSSIM_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _reconstructions(model, x, tmp_path):
    """qarv_base (seeded weights) reconstructions of the (1, 3, h, w) image x at LAMBDAS, through the file API (pads to 64, crops back)."""
    from PIL import Image
    png, bits = str(tmp_path / 'x.png'), str(tmp_path / 'x.bits')
    Image.fromarray(x[0].permute(1, 2, 0).mul(255).round().byte().numpy()).save(png)
    out = []
    for lmb in LAMBDAS:
        model.compress_file(png, bits, lmb=lmb)
        out.append(model.decompress_file(bits))          # a cropped VIEW of the decoder's padded output, on the GPU
    return out


@pytest.mark.parametrize('h,w', [(512, 768), (161, 161), (181, 203), (1408, 2048)])
def test_kernel_against_yardstick(product_model, tmp_path, h, w):
    from lvae.metrics import ms_ssim
    x = image01(h, w, 31)
    pairs = [('identical', x, x)]
    pairs += [(f'noise sigma {s}', x, noisy(x, s, 3)) for s in (0.01, 0.05, 0.2)]
    pairs += [('black / white', torch.zeros_like(x), torch.ones_like(x)), ('x / 1 - x', x, 1 - x)]
    pairs += [(f'qarv_base lambda {lmb:g}', x, r) for lmb, r in zip(LAMBDAS, _reconstructions(product_model, x, tmp_path))]
    reals = [a.cuda() for _, a, _ in pairs]
    fakes = [b if b.is_cuda else b.cuda() for _, _, b in pairs]
    got, got_m = ms_ssim(reals, fakes, return_scales=True)          # ONE call for the 8 pairs: packed reals, and fakes that are views
    torch.cuda.synchronize()
    got, got_m = got.cpu(), got_m.cpu()
    assert got.dtype == torch.float64 and got.shape == (len(pairs),) and got_m.shape == (len(pairs), 5, 3)
    worst = worst_m = 0.0
    for i, (name, a, b) in enumerate(pairs):
        ref, ref_m = ms_ssim_fp64(a.cpu(), b.cpu(), return_scales=True)
        err, err_m = abs(float(got[i]) - float(ref)), float((got_m[i] - ref_m[0]).abs().max())
        _report(f'{h}x{w} {name}: kernel {float(got[i]):.12f} yardstick {float(ref):.12f} |d| {err:.3e} per-scale means max|d| {err_m:.3e}')
        worst, worst_m = max(worst, err), max(worst_m, err_m)
    _report(f'{h}x{w} WORST |d| {worst:.3e}, per-scale means {worst_m:.3e} (bound {BOUND:g})')
    assert worst <= BOUND and worst_m <= BOUND, (worst, worst_m)
    assert float(got[0]) == 1.0 and float(got[5]) == 0.0 and not torch.isnan(got).any()
    # the single-pair call on a reconstruction view (read in place) and on a contiguous copy of it agree to the bit
    one = ms_ssim([reals[6]], [fakes[6]])
    assert torch.equal(one.cpu(), got[6:7]) and torch.equal(ms_ssim(reals[6], fakes[6].contiguous()).cpu(), got[6:7])


def test_extents_batching_and_determinism():
    """4 images of different sizes cropped from one padded (4, 3, 512, 768) batch: row i of the batched call (views, read in place)
    equals the single-image call on a contiguous copy of that crop bit for bit, and a repeated call returns the same bits."""
    from lvae.metrics import ms_ssim
    hw = [(512, 768), (161, 300), (333, 161), (470, 701)]
    real = torch.zeros(4, 3, 512, 768)
    fake = torch.rand(4, 3, 512, 768, generator=torch.Generator().manual_seed(1))          # garbage outside the extents must not matter
    for i, (h, w) in enumerate(hw):
        x = image01(h, w, 40 + i)
        real[i, :, :h, :w] = x[0]
        fake[i, :, :h, :w] = noisy(x, 0.03 * (i + 1), i)[0]
    real, fake = real.cuda(), fake.cuda()
    rv = [real[i:i + 1, :, :h, :w] for i, (h, w) in enumerate(hw)]
    fv = [fake[i:i + 1, :, :h, :w] for i, (h, w) in enumerate(hw)]
    a, am = ms_ssim(rv, fv, return_scales=True)
    b, bm = ms_ssim(rv, fv, return_scales=True)
    c = ms_ssim(real, fake, sizes=hw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(am, bm) and torch.equal(a, c)
    for i in range(4):
        s, sm = ms_ssim(rv[i].contiguous(), fv[i].contiguous(), return_scales=True)
        assert torch.equal(s, a[i:i + 1]) and torch.equal(sm, am[i:i + 1]), (i, s, a[i])
        ref = ms_ssim_fp64(rv[i].cpu(), fv[i].cpu())
        assert abs(float(a[i]) - float(ref)) <= BOUND, (i, float(a[i]), float(ref))
    with pytest.raises(ValueError, match='160x768'):
        ms_ssim(real, fake, sizes=[(160, 768)] * 4)


# ------------------------------------------------------------------------------------------------------------------ the harness
SET = [(192, 256), (200, 301), (192, 256), (200, 301), (192, 256)]          # two sizes; 200 x 301 is not a multiple of 64
BOTH = ('psnr', 'ms-ssim')


def _write_set(d):
    import seeded_init
    from PIL import Image
    for i, (h, w) in enumerate(SET):
        Image.fromarray(seeded_init.synthetic_image_u8(h, w, seed=70 + i)).save(os.path.join(d, f'im{i:02d}.png'))


def _seeded_model():
    import lvae
    import seeded_init
    from oracle import qarv_oracle
    sd = seeded_init.seeded_state_dict(qarv_oracle.qarv_param_shapes(qarv_oracle.qarv_base_arch()), seed=0)
    m = lvae.get_model('qarv_base')
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    return m


def _sharded_worker(rank, world, dataset, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from lvae.evaluation import imcoding_evaluate_sharded
    res = imcoding_evaluate_sharded(_seeded_model(), dataset, metrics=BOTH)
    if rank == 0:
        q.put(res)
    dist.barrier()
    dist.destroy_process_group()


def _run_sharded(world, dataset):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1500) + world          # the two runs of the test do not share a port
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, dataset, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def test_harness_option_real_model(product_model, tmp_path):
    from PIL import Image
    from lvae.evaluation import imcoding_evaluate
    from lvae.utils.coding import pil_to_tensor01
    d = tmp_path / 'set'
    d.mkdir()
    _write_set(str(d))
    m = product_model
    old = m.default_lmb
    m.default_lmb = 256.0
    try:
        base = imcoding_evaluate(m, str(d))
        both = imcoding_evaluate(m, str(d), metrics=BOTH)
        vals = []
        for p in sorted(d.iterdir()):
            bits = str(tmp_path / 'one.bits')
            m.compress_file(p, bits)
            vals.append(float(ms_ssim_fp64(pil_to_tensor01(Image.open(p)).unsqueeze(0), m.decompress_file(bits).cpu())))
    finally:
        m.default_lmb = old
    assert set(base) == {'bpp', 'mse', 'psnr'} and set(both) == {'bpp', 'mse', 'psnr', 'ms-ssim'}
    for k in base:
        assert both[k] == base[k], k
    ref = sum(vals) / len(vals)
    _report(f'harness, 5 images at lambda 256: ms-ssim {both["ms-ssim"]:.12f} yardstick mean {ref:.12f} |d| {abs(both["ms-ssim"] - ref):.3e}')
    assert abs(both['ms-ssim'] - ref) <= BOUND
    # sharded: world 1, then 2 ranks sharing cuda:0 over gloo (each rank builds the same seeded model) -> the same dictionary, to the bit
    assert _run_sharded(1, str(d)) == both
    assert _run_sharded(2, str(d)) == both
