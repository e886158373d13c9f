"""-m gpu: per-image lambda in the batched qarv_base paths -- the strided depthwise launches, the batched embedding GEMV, the three
public batch interfaces, forward() and compress_to_target -- each against the single-lambda / single-image path, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import seeded_init

pytestmark = pytest.mark.gpu

# 8 distinct-or-equal lambdas spanning lmb_range = (16, 2048): both ends, two equal ones, non-integer values
LMBS = [16.0, 2048.0, 100.5, 100.5, 37.25, 733.3, 1500.123, 64.0]


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _images(n, H, W, seed0=70):
    return torch.stack([torch.from_numpy(seeded_init.synthetic_image_u8(H, W, seed0 + i)).permute(2, 0, 1).float().div(255) for i in range(n)]).cuda()


# ---------------------------------------------------------------------------------------------------------------- kernels
def _dw_out_bytes(fmt, B, H, W, C):
    M = B * H * W
    return {'f32': M * C * 4, 'h2': M * C * 4, 'bf16': M * C * 2, 'q8': M * C + (C // 64) * M * 2}[fmt]


def _image_bytes(fmt, buf, b, B, H, W, C):
    """The bytes of image b inside the output of a launch over B images (Q8: the data rows, then each 64-channel block's scales)."""
    hw, M = H * W, B * H * W
    if fmt != 'q8':
        n = _dw_out_bytes(fmt, 1, H, W, C)
        return buf[b * n:(b + 1) * n]
    parts = [buf[b * hw * C:(b + 1) * hw * C]]
    for w in range(C // 64):
        o = M * C + (w * M + b * hw) * 2
        parts.append(buf[o:o + hw * 2])
    return torch.cat(parts)


def _tile_rows(L, fmt, C, k, B, H, W):
    """Output rows per tile (TH) of the csrc/dwconv_cl.hip instance a launch runs: lvae_dwconv_ln_choice, the function the launcher
    itself switches on (the same for the _v entry points).  The kernel-level test below uses it to assert that its two map sizes really
    reach the one-row and the 8-row instances (the k = 7, TH = 8 instance is the one at the register limit)."""
    import dwconv_cases
    picks = {dwconv_cases.choice(L, fmt, 1, per_image, B, H, W, C, k) for per_image in (0, 1)}
    (rc, family, th, _), = picks
    assert rc == 0 and family == 0
    return th


# every (C, k) of qarv_base's AdaLN blocks
QARV_CK = [(128, 7), (192, 7), (256, 7), (384, 5), (384, 7), (512, 1), (512, 3), (512, 5), (512, 7)]


@pytest.mark.parametrize('fmt', ['f32', 'h2', 'bf16', 'q8'])
@pytest.mark.parametrize('size', ['small', 'large'])        # few workgroups: the launcher's one-row tiles; many: its 8-row tiles (asserted below)
@pytest.mark.parametrize('C,k', QARV_CK)
def test_strided_dwconv_equals_single_image_launches(L, C, k, size, fmt):
    B = 3
    # which instance the launcher runs for this launch (see _tile_rows).  Small map: one-row tiles, for the batch of 3 and for a
    # single image alike.  Large map: the first of two sizes that reaches the 8-row tiles.  C = 512 with k = 5, and with k = 7 on bf16
    # maps, never get there on any map (one workgroup per CU at TH = 8 against two at TH = 4, so the 4-row tiles always win): there the
    # large map stands for the largest instance the launcher uses.  k = 1 has one-row tiles only.
    lowp_ = fmt in ('bf16', 'q8')
    if size == 'small':
        H, W = 8, 16
        assert _tile_rows(L, fmt, C, k, B, H, W) == 1 and _tile_rows(L, fmt, C, k, 1, H, W) == 1
    else:
        H, W = next((hw for hw in ((128, 192), (128, 128)) if _tile_rows(L, fmt, C, k, B, *hw) == 8), (128, 192))
        want = 1 if k == 1 else 4 if (C == 512 and (k == 5 or (k == 7 and lowp_))) else 8
        assert _tile_rows(L, fmt, C, k, B, H, W) == want, (C, k, fmt, H, W)
    g = torch.Generator(device='cpu').manual_seed(C * 31 + k * 7 + H)
    x = torch.randn(B, H, W, C, generator=g).cuda()
    wt = (torch.randn(k * k, C, generator=g) / k).cuda()
    bias = torch.randn(C, generator=g).cuda()
    stride = 2 * C + 64                                      # rows of a wider table, as in the model's [B][adaln_total] slab
    tab = torch.randn(B, stride, generator=g).cuda()         # row b: shift at 0, 1 + scale at C
    tab[:, C:2 * C] = 1 + 0.3 * tab[:, C:2 * C]
    lowp = fmt in ('bf16', 'q8')
    xi = x.to(torch.bfloat16) if lowp else x
    old = getattr(L, 'lvae_dwconv_ln_' + fmt)
    new = getattr(L, 'lvae_dwconv_ln_' + fmt + '_v')
    es = tab.element_size()

    def run_old(xs, row, nb):
        y = torch.full((_dw_out_bytes(fmt, nb, H, W, C),), 0xA5, dtype=torch.uint8, device='cuda')
        rc = old(xs.data_ptr(), wt.data_ptr(), bias.data_ptr(), None, None, tab.data_ptr() + row * stride * es, tab.data_ptr() + (row * stride + C) * es,
                 y.data_ptr(), nb, H, W, C, k, _st())
        assert rc == 0, rc
        return y

    def run_new(vstride):
        y = torch.full((_dw_out_bytes(fmt, B, H, W, C),), 0x5A, dtype=torch.uint8, device='cuda')
        rc = new(xi.data_ptr(), wt.data_ptr(), bias.data_ptr(), tab.data_ptr(), tab.data_ptr() + C * es, y.data_ptr(), B, H, W, C, k, vstride, _st())
        assert rc == 0, rc
        return y
    y_v = run_new(stride)
    singles = [run_old(xi[b:b + 1].contiguous(), b, 1) for b in range(B)]
    y_0, y_all = run_new(0), run_old(xi, 0, B)
    torch.cuda.synchronize()
    for b in range(B):
        assert torch.equal(_image_bytes(fmt, y_v, b, B, H, W, C), _image_bytes(fmt, singles[b], 0, 1, H, W, C)), (C, k, fmt, b)
    assert torch.equal(y_0, y_all)                           # stride 0 = the existing entry point on the whole batch
    assert not torch.equal(_image_bytes(fmt, y_v, 1, B, H, W, C), _image_bytes(fmt, y_all, 1, B, H, W, C))   # the vectors do matter


def test_strided_dwconv_rejects_other_shapes(L):
    x = torch.zeros(1, 8, 8, 144, device='cuda')
    v = torch.zeros(288, device='cuda')
    for fmt in ('f32', 'h2', 'bf16', 'q8'):
        rc = getattr(L, f'lvae_dwconv_ln_{fmt}_v')(x.data_ptr(), x.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), x.data_ptr(), 1, 8, 8, 144, 7, 0, _st())
        assert rc == -22


@pytest.mark.parametrize('n', [1, 2, 8, 11])
def test_batched_gemv_rows_equal_single_launches(L, product_model, n):
    """The three launches of _set_lmb (lambda-MLP layer 0 with GELU out, layer 2, all AdaLN embedding layers with GELU in) on the model's
    own weights: row i of the batched launch == lvae_gemv_f32 on input i."""
    pk = product_model._prepare()
    g = torch.Generator(device='cpu').manual_seed(n)
    for wn, bn, N, K, gin, gout in (('lmb.0.w', 'lmb.0.b', 256, 256, 0, 1), ('lmb.2.w', 'lmb.2.b', 256, 256, 0, 0),
                                    ('adaln.w', 'adaln.b', pk.adaln_total, 256, 1, 0)):
        x = torch.randn(n, K, generator=g).cuda()
        y = torch.full((n, N), float('nan'), device='cuda')
        assert L.lvae_gemv_batch_f32(pk.p(wn), pk.p(bn), x.data_ptr(), y.data_ptr(), N, K, n, gin, gout, _st()) == 0
        for i in range(n):
            y1 = torch.full((N,), float('nan'), device='cuda')
            assert L.lvae_gemv_f32(pk.p(wn), pk.p(bn), x[i].data_ptr(), y1.data_ptr(), N, K, gin, gout, _st()) == 0
            torch.cuda.synchronize()
            assert torch.equal(y[i].view(torch.int32), y1.view(torch.int32)), (wn, n, i)


@pytest.mark.parametrize('K', [1024, 1028, 2048])
def test_batched_gemv_long_rows(L, K):
    """Rows beyond the register-held form (K > 1024: the weight row is re-fetched once per 8 inputs) and the longest one inside it, on
    random weights, both GELU switches on, n = 11 (two passes): row i == lvae_gemv_f32 on input i."""
    n, N = 11, 37
    g = torch.Generator(device='cpu').manual_seed(K)
    Wt = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    x = torch.randn(n, K, generator=g).cuda()
    y = torch.full((n, N), float('nan'), device='cuda')
    assert L.lvae_gemv_batch_f32(Wt.data_ptr(), b.data_ptr(), x.data_ptr(), y.data_ptr(), N, K, n, 1, 1, _st()) == 0
    for i in range(n):
        y1 = torch.full((N,), float('nan'), device='cuda')
        assert L.lvae_gemv_f32(Wt.data_ptr(), b.data_ptr(), x[i].data_ptr(), y1.data_ptr(), N, K, 1, 1, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(y[i].view(torch.int32), y1.view(torch.int32)), (K, i)
    ref = torch.nn.functional.gelu(torch.nn.functional.gelu(x.double()) @ Wt.double().t() + b.double())
    assert float((y.double() - ref).abs().max()) < 2e-5


# ---------------------------------------------------------------------------------------------------------------- model
def _with_prec(m, prec):
    base = m._prec
    m.set_gemm_precision(prec)
    return base


@pytest.mark.parametrize('prec', ['f16x2', 'bf16x3', 'fp8'])
def test_mixed_lambda_batch_equals_single_image_calls(product_model, prec):
    m = product_model
    from lvae.models.base import DEFAULT_PRECISION
    assert DEFAULT_PRECISION == 'f16x2'
    base, groups, native = _with_prec(m, prec), m.pipeline_groups, m.native_group_loops
    try:
        ims = _images(8, 128, 192)
        singles = [m.compress(ims[i:i + 1], LMBS[i]) for i in range(8)]
        recs = [m.decompress(s) for s in singles]
        assert len({len(s) for s in singles}) > 1                          # the lambdas do change the streams
        for G in (1, 2):
            for nat in (True, False):
                m.pipeline_groups, m.native_group_loops = G, nat
                strings = m.compress_batch(ims, LMBS)
                assert strings == singles, (prec, G, nat, [a == b for a, b in zip(strings, singles)])
                out = m.decompress_batch(strings)
                for i in range(8):
                    assert torch.equal(out[i:i + 1], recs[i]), (prec, G, nat, i)
                # B = 5 on the same model object, after B = 8: other group sizes and group starts behind the same cached-plan keys
                sub = [7, 2, 3, 0, 5]
                s5 = m.compress_batch(ims[sub], [LMBS[i] for i in sub])
                assert s5 == [singles[i] for i in sub], (prec, G, nat)
                o5 = m.decompress_batch(s5)
                for j, i in enumerate(sub):
                    assert torch.equal(o5[j:j + 1], recs[i]), (prec, G, nat, i)
                # a tensor and a shared lambda as a list take the same route as before
                assert m.compress_batch(ims[:4], torch.tensor(LMBS[:4])) == singles[:4]
                assert m.compress_batch(ims[2:4], [100.5, 100.5]) == singles[2:4]
    finally:
        m.pipeline_groups, m.native_group_loops = groups, native
        m.set_gemm_precision(base)


def test_mixed_lambda_batch_512x768(product_model):
    m = product_model
    ims = _images(8, 512, 768, seed0=90)
    strings = m.compress_batch(ims, LMBS)
    out = m.decompress_batch(strings)
    for i in range(8):
        s = m.compress(ims[i:i + 1], LMBS[i])
        assert strings[i] == s, i
        assert torch.equal(out[i:i + 1], m.decompress(s)), i


def test_mixed_lambda_files(product_model, tmp_path):
    from PIL import Image
    m = product_model
    paths, bits1, bitsB = [], [], []
    for i in range(4):
        p = tmp_path / f'im{i}.png'
        Image.fromarray(seeded_init.synthetic_image_u8(120, 180, 50 + i)).save(p)
        paths.append(str(p)); bits1.append(str(tmp_path / f's{i}.bits')); bitsB.append(str(tmp_path / f'b{i}.bits'))
        m.compress_file(paths[-1], bits1[-1], lmb=LMBS[i])
    m.compress_files(paths, bitsB, lmb=LMBS[:4])
    for a, b in zip(bits1, bitsB):
        assert open(a, 'rb').read() == open(b, 'rb').read()
    outs = m.decompress_files(bitsB)
    for a, o in zip(bits1, outs):
        assert torch.equal(o, m.decompress_file(a))


def test_mixed_lambda_rows_against_oracle(product_model, qarv_seeded_sd):
    """Rows 1 and 6 of the mixed-lambda batch against the CPU oracle run at that row's lambda: the teacher-forced comparison and the bars
    of tests/test_gpu_configs.py::test_config2_qarv_base_b8_512x768_against_oracle (guard bands of parity_util, |dx| <= 1e-4, flips <= 1e-4 n)."""
    import parity_util
    from oracle import qarv_oracle
    m = product_model
    orc = qarv_oracle.QarvOracle(qarv_seeded_sd)
    orc.compress_mode()
    ims = _images(8, 128, 192)
    rows = [1, 6]
    otrs = [orc.encode_trace(ims[r:r + 1].cpu(), LMBS[r], code=False) for r in rows]
    oblocks = [{k: torch.cat([o['blocks'][bi][k] for o in otrs], 0) for k in ('pm', 'pv', 'qm', 'indexes', 'symbols', 'z')} for bi in range(9)]
    trf = m.encode_trace(ims, LMBS, full=True, force_z=[(rows, b['z']) for b in oblocks])
    guard = parity_util.check_blocks('qarv_base B=8 128x192 mixed lambda rows 1,6', trf, oblocks, m._dg().scale_table.cpu().numpy(),
                                     m._packed.scale_bound, rows=rows)
    print(parity_util.describe(guard))
    n = guard['n']
    assert n == 2 * sum(z * hw for z, hw in m._plan('enc', 8, 128, 192, vec=True).lat_shapes)
    assert guard['sym_flips'] + guard['idx_flips'] <= 1e-4 * n, guard
    zs = [b['z'] for b in oblocks]
    x_hip = m.conditional_sample([LMBS[r] for r in rows], [z.cuda() for z in zs]).cpu()
    x_orc = torch.cat([orc.decode_from_latents(LMBS[r], [z[i:i + 1] for z in zs]) for i, r in enumerate(rows)], 0)
    err = float((x_hip - x_orc).abs().max())
    print(f'max|dx| = {err:.3e}')
    assert err <= 1e-4, err


def test_forward_with_per_image_lambdas_is_one_plan_run_each(product_model, monkeypatch):
    from lvae.engine import Plan
    from lvae.models.qarv.model import _DecPlan, _EncPlan
    m = product_model
    ims = _images(8, 128, 192)
    lmb = torch.tensor(LMBS, device='cuda')
    per = [m(ims[i:i + 1], lmb=LMBS[i], return_rec=True) for i in range(8)]
    runs = []
    orig = Plan.run

    def spy(self, *a, **k):
        runs.append(type(self))
        return orig(self, *a, **k)
    monkeypatch.setattr(Plan, 'run', spy)
    st = m(ims, lmb=lmb, return_rec=True)
    monkeypatch.setattr(Plan, 'run', orig)
    assert runs.count(_EncPlan) == 1 and runs.count(_DecPlan) == 1 and len(runs) == 2, runs
    st2 = m(ims, lmb=lmb, return_rec=True)
    for i in range(8):
        assert torch.equal(st['im_hat'][i:i + 1], per[i]['im_hat']), i
    # mse_i is exactly image i's distortion (a batch of one), and the batch's mse the fp64 mean of those: the same floats
    assert st['mse'] == float(torch.tensor([p['mse'] for p in per], dtype=torch.float64).mean(0))
    # bppix_i = kl_i * log2(e) * 3 is rounded per image, so the mean of the eight only agrees to fp64 rounding
    assert st['bppix'] == pytest.approx(np.mean([p['bppix'] for p in per]), rel=1e-12)
    assert st['mse'] == st2['mse'] and st['bppix'] == st2['bppix'] and st['psnr'] == st2['psnr'] and torch.equal(st['loss'], st2['loss'])
    assert torch.equal(st['im_hat'], st2['im_hat'])
    est_im, est_nats = m.estimate(ims, LMBS)
    for i in (0, 3, 6):
        e1, n1 = m.estimate(ims[i:i + 1], LMBS[i])
        assert torch.equal(est_im[i:i + 1], e1)
        # (the per-block rate is summed with fp64 atomics, lvae_gaussian_nll_f32: the order of the partial sums is not fixed)
        assert torch.allclose(est_nats[:, i], n1[:, 0], rtol=1e-12, atol=0)


def test_compress_to_target(product_model):
    """The contract of compress_to_target on the seeded model: the returned stream is compress(im, returned lambda), its size obeys the
    return rule against every probe (each recomputed alone), rounds <= max_rounds.
    With the seeded (untrained) weights the size hardly depends on lambda -- measured on MI355X: 34591 bytes at lambda 16, 34579 at 2048,
    not even monotone -- so nothing here is about convergence; that rests on tests/test_rate_search.py (synthetic monotone size functions)."""
    m = product_model
    im = _images(1, 128, 192, seed0=5)
    lo, hi = (len(m.compress(im, v)) + 4 for v in m.lmb_range)
    print(f'sizes at the ends of lmb_range: {lo} .. {hi} bytes')
    target = (lo + hi) // 2
    probes = []
    orig = m.compress_batch

    def spy(batch, lmb=None):
        out = orig(batch, lmb)
        probes.extend(zip([float(np.float32(v)) for v in lmb], out))
        return out
    m.compress_batch = spy
    try:
        s, lmb, rounds = m.compress_to_target(im, target, n_probe=8, max_rounds=6)
    finally:
        del m.compress_batch
    assert 1 <= rounds <= 6 and len(probes) == 8 * rounds
    assert s == m.compress(im, lmb)
    assert m.lmb_range[0] < lmb < m.lmb_range[1]
    sizes = []
    for v, coded in probes:                                  # every probe, recomputed alone
        one = m.compress(im, v)
        assert one == coded
        sizes.append(len(one) + 4)
    fits = [n for n in sizes if n <= target]
    print(f'target {target}: returned {len(s) + 4} bytes at lmb={lmb:.4f} after {rounds} rounds')
    assert len(s) + 4 == (max(fits) if fits else min(sizes))


def _png_dir(tmp_path, sizes, seed0=40):
    from PIL import Image
    paths = []
    for i, (h, w) in enumerate(sizes):
        p = tmp_path / f'im{i:02d}.png'
        Image.fromarray(seeded_init.synthetic_image_u8(h, w, seed0 + i)).save(p)
        paths.append(p)
    return paths


def test_self_evaluate_batched_equals_the_per_image_loop(product_model, tmp_path):
    """self_evaluate runs each image once, as a batch of `steps` lambdas.  (a) Every returned float equals (`==`) the reference's loop
    -- `_self_evaluate(paths, lmb)` per lambda, one image and one lambda at a time -- and a second call.  (b) Against the loop as it was
    before (rate from estimate()): psnr `==` (the reconstruction is bit-equal); bpp and loss to 1e-10 relative only, because estimate()
    adds its per-workgroup partial sums with fp64 atomics in arrival order and is itself not reproducible to the last bit.  The bound:
    the rate is a sum of N < 1e5 non-negative fp64 terms per image here, any order of which is within (N - 1) 2^-53 < 1.2e-11 relative of
    the exact sum, so two orders differ by < 2.4e-11; the distortion term of the loss is identical and positive."""
    import math
    from lvae.utils import coding
    from PIL import Image
    m = product_model
    paths = _png_dir(tmp_path, [(120, 180), (64, 64), (200, 130)])
    stats = m.self_evaluate(str(tmp_path), steps=8)
    again = m.self_evaluate(str(tmp_path), steps=8)
    lambdas = torch.linspace(math.log(m.lmb_range[0]), math.log(m.lmb_range[1]), steps=8).exp().tolist()
    assert stats['lambda'] == lambdas and set(stats) == {'loss', 'bpp', 'psnr', 'lambda'}
    for j, lmb in enumerate(lambdas):
        one = m._self_evaluate(paths, lmb)
        for k in ('loss', 'bpp', 'psnr', 'lambda'):
            assert stats[k][j] == one[k] == again[k][j], (k, j, stats[k][j], one[k])
        tot = {'loss': 0.0, 'bpp': 0.0, 'psnr': 0.0}      # the loop as it was: estimate() on one image at one lambda
        for p in paths:
            img = Image.open(p)
            h, w = img.height, img.width
            im = coding.pil_to_tensor01(coding.pad_divisible_by(img, div=m.max_stride)).unsqueeze_(0).cuda()
            im_hat, nats = m.estimate(im, lmb)
            kl = float(nats.sum()) / (3 * h * w)
            mse = float((coding.pil_to_tensor01(img).cuda() - im_hat[0, :, :h, :w]).square().mean())
            tot['loss'] += kl + lmb * 4.0 * mse
            tot['bpp'] += kl * m.log2_e * 3
            tot['psnr'] += -10 * math.log10(mse)
        assert stats['psnr'][j] == tot['psnr'] / len(paths)
        print(f"lmb {lmb:.2f}: bpp {stats['bpp'][j]!r} vs {tot['bpp'] / len(paths)!r}")
        assert stats['bpp'][j] == pytest.approx(tot['bpp'] / len(paths), rel=1e-10, abs=0)
        assert stats['loss'][j] == pytest.approx(tot['loss'] / len(paths), rel=1e-10, abs=0)


def test_rate_targeting_script_with_probes(tmp_path):
    """scripts/qarv/test-at-target-bytes.py --probes 4: one 'round k:' line per round, and the file it leaves decodes."""
    import os
    import subprocess
    import sys
    import lvae
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = tmp_path / 'torch_home' / 'hub' / 'checkpoints'
    os.makedirs(ck)
    m = lvae.get_model('qarv_base')
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None:
            sd[k] = torch.from_numpy(a)
    torch.save({'model': sd}, str(ck / 'qarv_base-2022-dec-12.pt'))
    img, = _png_dir(tmp_path, [(120, 180)], seed0=60)
    bits = tmp_path / 'x.bits'
    env = dict(os.environ, TORCH_HOME=str(tmp_path / 'torch_home'),
               PYTHONPATH=os.pathsep.join([repo, os.path.join(repo, 'lossy-vae_amd'), os.environ.get('PYTHONPATH', '')]))
    r = subprocess.run([sys.executable, os.path.join(repo, 'scripts', 'qarv', 'test-at-target-bytes.py'), '-i', str(img), '-b', str(bits),
                        '-t', '30000', '--probes', '4'], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    rounds = [l for l in lines if l.startswith('round ')]
    assert [l.split(':')[0] for l in rounds] == [f'round {k}' for k in range(len(rounds))] and rounds
    assert all(l.count('lmb=') == 4 for l in rounds)
    summary = [l for l in lines if ' rounds of 4 probes: ' in l]
    assert len(summary) == 1 and int(summary[0].split()[0]) == len(rounds)
    assert lines[-1].startswith('lambda = ')
    n_bytes = int(summary[0].split('bytes=')[1].split('B')[0])
    assert os.path.getsize(bits) == n_bytes
    sizes = [int(x.split('B')[0]) for l in rounds for x in l.split('-> ')[1:]]
    fits = [n for n in sizes if n <= 30000]
    assert n_bytes == (max(fits) if fits else min(sizes))
    # the file is a compress_file stream: it decodes in this process, to the size of the image
    m.load_state_dict(sd)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    out = m.decompress_file(str(bits))
    assert tuple(out.shape) == (1, 3, 120, 180) and bool(torch.isfinite(out).all())
