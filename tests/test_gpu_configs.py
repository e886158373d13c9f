"""-m gpu: the BASELINE.json configurations the golden tests do not reach, and the reference's harness scripts executed as
scripts (subprocesses with the reference's own CLI defaults), so that they cannot rot silently.

  config 3  qres34m, eval-fix-rate.py call sequence over 24 synthetic 512x768 PNGs (`get_model(name, lmb=, pretrained=True)`,
            compress_mode() BEFORE .to(), imcoding_evaluate) + a golden-free oracle comparison of one 512x768 image;
  config 4  imcoding_evaluate_sharded with the REAL qarv_base: two ranks on cuda:0 (gloo) over mixed-size images == the
            single-process dict; scripts/eval-sharded.py and `bench.py --gpus 2` in their single-GPU rehearsal mode;
  H2 / f2   scripts/speedtest-lvae.py, eval-var-rate.py, scripts/qarv/test-at-target-bytes.py.

`pretrained=True` works offline because torch.hub's `load_state_dict_from_url` takes a file that is already in
$TORCH_HOME/hub/checkpoints: the tests put seeded-weight checkpoints there under the reference's file names.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeded_init

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seeded_checkpoint(name, path, profile='typical', **kw):
    import lvae
    m = lvae.get_model(name, **kw)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile=profile)
        if a is not None:
            sd[k] = torch.from_numpy(a)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({'model': sd}, path)
    return sd


def _write_pngs(folder, sizes, seed0):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(seeded_init.synthetic_image_u8(h, w, seed0 + i)).save(os.path.join(folder, f'im{i:02d}.png'))


@pytest.fixture(scope='module')
def offline_home(tmp_path_factory):
    """TORCH_HOME with the two checkpoints the scripts' `pretrained=True` resolve to + a datasets root (paths.py contract)."""
    root = tmp_path_factory.mktemp('offline')
    ck = root / 'torch_home' / 'hub' / 'checkpoints'
    _seeded_checkpoint('qarv_base', str(ck / 'qarv_base-2022-dec-12.pt'))
    _seeded_checkpoint('qres34m', str(ck / 'qres34m-lmb64.pt'), lmb=64)
    _write_pngs(str(root / 'datasets' / 'kodak'), [(512, 768)] * 24, 700)                       # config 3: "Kodak-24" stand-in
    _write_pngs(str(root / 'datasets' / 'clic' / 'test-2022'),
                [(300, 500), (512, 768), (768, 512), (1365, 2048), (640, 640), (200, 333), (512, 768)], 800)   # mixed sizes
    return root


def _env(root, **extra):
    e = dict(os.environ)
    e.update(TORCH_HOME=str(root / 'torch_home'), LVAE_DATASETS=str(root / 'datasets'), MASTER_ADDR='127.0.0.1',
             PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, 'lossy-vae_amd'), e.get('PYTHONPATH', '')]))
    e.update(extra)
    return e


def _run(cmd, root, cwd, timeout=900, **env):
    r = subprocess.run([sys.executable] + cmd, cwd=str(cwd), env=_env(root, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f'{cmd}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}'
    return r.stdout


# ------------------------------------------------------------------------------------------------------------------ config 3
def test_config3_eval_fix_rate_script_qres34m(offline_home, tmp_path):
    """eval-fix-rate.py (reference :25-35) as a script: qres34m, lambda 64, 24 x 512x768; the JSON it writes must hold exactly
    what the same call sequence gives in this process."""
    out = _run([os.path.join(REPO, 'eval-fix-rate.py'), '-m', 'qres34m', '-l', '64', '-n', 'kodak'], offline_home, tmp_path)
    assert 'lambda=64' in out
    res = json.load(open(tmp_path / 'runs' / 'results' / 'kodak-qres34m.json'))
    assert res['name'] == 'qres34m' and res['lambdas'] == [64] and set(res['results']) == {'bpp', 'mse', 'psnr'}
    import lvae
    from lvae.evaluation import imcoding_evaluate
    os.environ['TORCH_HOME'] = str(offline_home / 'torch_home')
    try:
        m = lvae.get_model('qres34m', lmb=64, pretrained=True)
    finally:
        os.environ.pop('TORCH_HOME')
    m.compress_mode()                                   # on the CPU, then .to(): eval-fix-rate.py:30-31
    m = m.to('cuda:0').eval()
    mine = imcoding_evaluate(m, str(offline_home / 'datasets' / 'kodak'))
    for k in ('bpp', 'mse', 'psnr'):
        assert res['results'][k] == [mine[k]], (k, res['results'][k], mine[k])
    assert 0.05 < mine['bpp'] < 24 and math.isfinite(mine['psnr'])
    # round trip / determinism / batch == single at the full size
    ims = torch.stack([torch.from_numpy(seeded_init.synthetic_image_u8(512, 768, 700 + i)).permute(2, 0, 1).float().div(255)
                       for i in range(4)]).cuda()
    objs = m.compress_batch(ims)
    assert objs[3] == m.compress(ims[3:4]) and objs == m.compress_batch(ims)
    xb = m.decompress_batch(objs)
    assert torch.equal(xb[1:2], m.decompress(objs[1])) and xb.shape == ims.shape


def _free_running_flips(tr, oblocks):
    """Symbol / index disagreements of the FREE-RUNNING encoder (each block conditioned on the GPU's own latents).  A symbol flip
    changes the latent every later block is conditioned on, so whatever follows it is a cascade, not independent rounding events:
    the count up to and including the first block with a symbol flip ("first-order") is returned next to the totals."""
    n = flips = iflips = n1 = f1 = 0
    clean = True
    for a, b in zip(tr, oblocks):
        sf = int((a['symbols'].reshape(-1) != b['symbols'].numpy().reshape(-1)).sum())
        xf = int((a['indexes'].reshape(-1) != b['indexes'].numpy().reshape(-1)).sum())
        n += a['symbols'].size; flips += sf; iflips += xf
        if clean:
            n1 += a['symbols'].size; f1 += sf + xf
            clean = sf == 0
    return n, flips, iflips, n1, f1


def test_config3_qres34m_512x768_against_oracle():
    """One full-size image, HIP path vs the live CPU oracle on the same seeded ('wide') weights -- no golden at this size.
    (1) TEACHER-FORCED comparison (parity_util.py): the HIP encoder is handed the oracle's latents block by block, every element
    of pm / qm / ln sigma must lie within rounding noise of the oracle's and every flipped index / symbol inside its guard band;
    (2) reconstruction: the HIP DECODER fed with the oracle's latents verbatim (cond_sample) against the oracle's decoder,
    |dx| <= 1e-4 -- independent of any encoder-side flip; (3) free-running flip counts, reported and sanity-bounded."""
    import parity_util
    from conftest import parity_record
    from oracle import qres_oracle
    import lvae
    sd = seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(qres_oracle.qres34m_arch()), seed=0)
    m = lvae.get_model('qres34m')
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.compress_mode()
    m = m.to('cuda:0').eval()
    orc = qres_oracle.QresOracle(sd)
    orc.compress_mode()
    im = torch.from_numpy(seeded_init.synthetic_image_u8(512, 768, 31)).permute(2, 0, 1).float().div(255).unsqueeze(0)
    otr = orc.encode_trace(im, code=False)
    zs = [b['z'] for b in otr['blocks']]
    case = 'qres34m 512x768 vs LIVE ORACLE'
    guard = parity_util.check_blocks(case, m.encode_trace(im.cuda(), full=True, force_z=zs), otr['blocks'],
                                     m._dg().scale_table.cpu().numpy(), m._packed.scale_bound)
    err = float((m.cond_sample([z.cuda() for z in zs]).cpu() - orc.decode_from_latents(zs)).abs().max())
    n, flips, iflips, n1, f1 = _free_running_flips(m.encode_trace(im.cuda()), otr['blocks'])
    parity_record(f'{case} (free-running: first-order flips {f1} in the {n1} symbols up to the first symbol flip, totals incl. its cascade:)',
                  flips, iflips, n, err, flips + iflips == 0, guard)
    assert n == guard['n'] == 1536 + 2 * 5376 + 3 * 18432 + 3 * 61440 + 3 * 196608       # symbols per block, 512x768
    assert err <= 1e-4, err
    assert guard['sym_flips'] + guard['idx_flips'] <= 1e-4 * n, guard
    # free-running: only the flips up to the first symbol flip are independent events; what follows is the cascade of a changed latent
    # (recorded, not bounded: one early flip legitimately changes every later prior)
    assert f1 <= 1e-4 * n1, (f1, n1, flips, iflips, n)
    obj = m.compress(im.cuda())
    assert torch.equal(m.decompress(obj), m.decompress(m.compress(im.cuda())))


def test_config2_qarv_base_b8_512x768_against_oracle():
    """BASELINE config 2 as stated -- `qarv_base`, a BATCH of 8 images of 512x768 -- against the live CPU oracle run on two images of
    the batch (rows 0 and 5); no golden at this size.  Same three parts as the qres34m test above: teacher-forced guard-band proof
    on the batched encode plan (only rows 0 and 5 are forced and compared), |dx| <= 1e-4 for the HIP decoder fed with the oracle's
    latents (conditional_sample), free-running flip counts of the batched encoder."""
    import parity_util
    from conftest import load_seeded_into, parity_record
    from oracle import qarv_oracle
    import lvae
    sd = seeded_init.seeded_state_dict(qarv_oracle.qarv_param_shapes(qarv_oracle.qarv_base_arch()), seed=0)
    m = lvae.get_model('qarv_base')
    load_seeded_into(m, sd)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    orc = qarv_oracle.QarvOracle(sd)
    orc.compress_mode()
    ims = torch.stack([torch.from_numpy(seeded_init.synthetic_image_u8(512, 768, 33 + i)).permute(2, 0, 1).float().div(255) for i in range(8)])
    lmb, rows = 2048.0, [0, 5]
    otrs = [orc.encode_trace(ims[r:r + 1], lmb, code=False) for r in rows]
    oblocks = [{k: torch.cat([o['blocks'][bi][k] for o in otrs], 0) for k in ('pm', 'pv', 'qm', 'indexes', 'symbols', 'z')} for bi in range(9)]
    case = 'qarv_base B=8 512x768 lmb=2048 rows 0,5 vs LIVE ORACLE'
    trf = m.encode_trace(ims.cuda(), lmb, full=True, force_z=[(rows, b['z']) for b in oblocks])
    guard = parity_util.check_blocks(case, trf, oblocks, m._dg().scale_table.cpu().numpy(), m._packed.scale_bound, rows=rows)
    zs = [b['z'] for b in oblocks]
    x_hip = m.conditional_sample(lmb, [z.cuda() for z in zs]).cpu()
    x_orc = torch.cat([orc.decode_from_latents(lmb, [z[i:i + 1] for z in zs]) for i in range(len(rows))], 0)
    err = float((x_hip - x_orc).abs().max())
    tr = m.encode_trace(ims.cuda(), lmb)
    n, flips, iflips, n1, f1 = _free_running_flips([{k: v[rows] for k, v in blk.items()} for blk in tr], oblocks)
    parity_record(f'{case} (free-running: first-order flips {f1} in the {n1} symbols up to the first symbol flip, totals incl. its cascade:)',
                  flips, iflips, n, err, flips + iflips == 0, guard)
    assert n == guard['n'] == 2 * 617472                 # symbols per 512x768 image
    assert err <= 1e-4, err
    assert guard['sym_flips'] + guard['idx_flips'] <= 1e-4 * n, guard
    assert f1 <= 1e-4 * n1, (f1, n1, flips, iflips, n)          # free-running: first-order flips only (see the qres34m test)
    # the batched strings are what single-image calls give, and the round trip is deterministic
    strings = m.compress_batch(ims.cuda(), lmb)
    assert strings[5] == m.compress(ims[5:6].cuda(), lmb)
    assert torch.equal(m.decompress_batch(strings)[5:6], m.decompress(strings[5]))


def _golden_blocks(g, prefix, n_blocks):
    """Per-block dicts (pm, pv, qm, indexes, symbols, z = symbols + pm) of a reference-generated golden (tests/golden/make_golden.py)."""
    out = []
    for bi in range(n_blocks):
        b = {k: g[f'{prefix}b{bi}.{k}'] for k in ('pm', 'pv', 'qm', 'indexes', 'symbols')}
        b['z'] = torch.from_numpy(b['symbols'].astype(np.float32) + b['pm'].astype(np.float32))
        out.append(b)
    return out


def test_config2_qarv_base_512x768_against_reference_golden(golden_dir):
    """The size BASELINE.json's metric is quoted on, held to a fixture the REFERENCE produced (tests/golden/make_golden.py full:
    `lvae.get_model('qarv_base')` of /root/reference, lambda = 2048, image seed 7): qarv/model.py:516-557 at 512x768.
    Image = batch row 3 of a batch of 8 (config 2 is a batch; the other rows are other images).  Teacher-forced guard-band proof for
    all 617 472 elements, |dx| <= 1e-4 for the HIP decoder on the reference's latents AND for decoding the reference's own bitstream
    when the free-running encoder has no flip on that image, byte-identical rANS strings block by block while symbols / indexes match."""
    import parity_util
    from conftest import load_seeded_into, parity_record
    from oracle import qarv_oracle
    from lvae.utils import coding
    import lvae
    g = np.load(os.path.join(golden_dir, 'qarv_base_512x768.npz'))
    sd = seeded_init.seeded_state_dict(qarv_oracle.qarv_param_shapes(qarv_oracle.qarv_base_arch()), seed=0)
    m = lvae.get_model('qarv_base')
    load_seeded_into(m, sd)
    m = m.to('cuda:0').eval()
    m.compress_mode()
    lmb, row, key = 2048.0, 3, 'lmb2048.'
    mk = lambda s: torch.from_numpy(seeded_init.synthetic_image_u8(512, 768, s)).permute(2, 0, 1).float().div(255)
    ims = torch.stack([mk(int(g['img_seed'])) if i == row else mk(50 + i) for i in range(8)])
    gb = _golden_blocks(g, key, 9)
    case = 'qarv_base B=8 512x768 lmb=2048 row 3 vs REFERENCE GOLDEN'
    trf = m.encode_trace(ims.cuda(), lmb, full=True, force_z=[([row], b['z']) for b in gb])
    guard = parity_util.check_blocks(case, trf, gb, m._dg().scale_table.cpu().numpy(), m._packed.scale_bound, rows=[row])
    x_ref = torch.from_numpy(g[key + 'xhat'])
    err = float((m.conditional_sample(lmb, [b['z'].cuda() for b in gb]).cpu() - x_ref).abs().max())
    # the reference's own container decodes here (same priors bit for bit unless an index sits on a threshold: then the stream is
    # undecodable on ANY other arithmetic -- the reference's CPU vs CUDA included -- and only the latent-fed check above applies)
    tr = m.encode_trace(ims.cuda(), lmb)
    n = flips = iflips = n1 = f1 = 0
    clean = True
    strings = coding.unpack_byte_string(m.compress_batch(ims.cuda(), lmb)[row][10:])
    same = True
    for bi, (a, b) in enumerate(zip(tr, gb)):
        sf = int((a['symbols'][row].reshape(-1) != b['symbols'].reshape(-1)).sum())
        xf = int((a['indexes'][row].reshape(-1) != b['indexes'].reshape(-1)).sum())
        n += b['symbols'].size; flips += sf; iflips += xf
        if clean:
            n1 += b['symbols'].size; f1 += sf + xf
            if sf == 0 and xf == 0:
                assert strings[bi] == g[f'{key}b{bi}.string'].tobytes(), f'{case}: block {bi} stream differs although symbols and indexes match'
            clean = sf == 0
        same = same and sf == 0 and xf == 0
    if same:
        err = max(err, float((m.decompress(g[key + 'bitstream'].tobytes()).cpu() - x_ref).abs().max()))
    parity_record(f'{case} (free-running: first-order flips {f1} in the {n1} symbols up to the first symbol flip, totals incl. its cascade:)',
                  flips, iflips, n, err, same, guard)
    assert n == guard['n'] == 617472
    assert err <= 1e-4, err
    assert guard['sym_flips'] + guard['idx_flips'] <= 1e-4 * n, guard
    assert f1 <= 1e-4 * n1, (f1, n1, flips, iflips, n)


def test_config3_qres34m_512x768_against_reference_golden(golden_dir):
    """qres34m at 512x768 against the reference-generated fixture (qresvae/model.py:649-725 run by make_golden.py full): the same
    three parts, plus the cross-decoder check -- the HIP encoder's strings decoded by the ORACLE's decoder (the container and the
    bitstream against the reference's semantics) give its reconstruction to 1e-4 when the free-running encode has no flip, and the
    total free-running flip count stays sane."""
    import parity_util
    from conftest import parity_record
    from oracle import qres_oracle
    import lvae
    g = np.load(os.path.join(golden_dir, 'qres34m_512x768.npz'))
    sd = seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(qres_oracle.qres34m_arch()), seed=0)
    m = lvae.get_model('qres34m')
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v)
    m.load_state_dict(full)
    m.compress_mode()
    m = m.to('cuda:0').eval()
    im = torch.from_numpy(seeded_init.synthetic_image_u8(512, 768, int(g['img_seed']))).permute(2, 0, 1).float().div(255).unsqueeze(0)
    gb = _golden_blocks(g, '', 12)
    zs = [b['z'] for b in gb]
    case = 'qres34m 512x768 vs REFERENCE GOLDEN'
    guard = parity_util.check_blocks(case, m.encode_trace(im.cuda(), full=True, force_z=zs), gb,
                                     m._dg().scale_table.cpu().numpy(), m._packed.scale_bound)
    x_ref = torch.from_numpy(g['xhat'])
    err = float((m.cond_sample([z.cuda() for z in zs]).cpu() - x_ref).abs().max())
    tr = m.encode_trace(im.cuda())
    obj = m.compress(im.cuda())
    n = flips = iflips = n1 = f1 = 0
    clean = True
    for bi, (a, b) in enumerate(zip(tr, gb)):
        sf = int((a['symbols'].reshape(-1) != b['symbols'].reshape(-1)).sum())
        xf = int((a['indexes'].reshape(-1) != b['indexes'].reshape(-1)).sum())
        n += b['symbols'].size; flips += sf; iflips += xf
        if clean:
            n1 += b['symbols'].size; f1 += sf + xf
            if sf == 0 and xf == 0:
                assert obj[bi][0] == g[f'b{bi}.string'].tobytes(), f'{case}: block {bi} stream differs although symbols and indexes match'
            clean = sf == 0
    parity_record(f'{case} (free-running: first-order flips {f1} in the {n1} symbols up to the first symbol flip, totals incl. its cascade:)',
                  flips, iflips, n, err, flips + iflips == 0, guard)
    assert n == guard['n'] == 841728 and tuple(obj[-1]) == tuple(g['smallest'].tolist())
    assert err <= 1e-4, err
    assert guard['sym_flips'] + guard['idx_flips'] <= 1e-4 * n, guard
    assert f1 <= 1e-4 * n1, (f1, n1, flips, iflips, n)
    assert flips + iflips <= 0.05 * n, (flips, iflips, n)              # loose sanity bound on the cascade
    # cross-decoder: the oracle decodes the HIP strings (its priors differ from the HIP decoder's by rounding noise only)
    orc = qres_oracle.QresOracle(sd)
    orc.compress_mode()
    if flips + iflips == 0:
        assert float((orc.decompress(obj) - x_ref).abs().max()) <= 1e-4
    assert torch.equal(m.decompress(obj), m.decompress(m.compress(im.cuda())))


# ------------------------------------------------------------------------------------------------------------------ config 4
def _sharded_worker(rank, world, dataset, ckpt, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import lvae
    from lvae.evaluation import imcoding_evaluate_sharded
    m = lvae.get_model('qarv_base', pretrained=ckpt).to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    res = imcoding_evaluate_sharded(m, dataset)
    if rank == 0:
        q.put(res)
    dist.barrier()
    dist.destroy_process_group()


def test_config4_sharded_eval_real_model_two_ranks(offline_home):
    """imcoding_evaluate_sharded with qarv_base itself (not a stub): 2 ranks sharing cuda:0, gloo, 7 mixed-size images ->
    the same dict, to the last bit, as the single-process imcoding_evaluate (reference loop: evaluation.py:31-66)."""
    import torch.multiprocessing as mp
    import lvae
    from lvae.evaluation import imcoding_evaluate
    ckpt = str(offline_home / 'torch_home' / 'hub' / 'checkpoints' / 'qarv_base-2022-dec-12.pt')
    dataset = str(offline_home / 'datasets' / 'clic' / 'test-2022')
    m = lvae.get_model('qarv_base', pretrained=ckpt).to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    single = imcoding_evaluate(m, dataset)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, dataset, ckpt, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res == single, (res, single)


# CLIC-2022-test shaped set (30 images drawn from {2048x1365, 1365x2048, 2048x1152, 1536x2048}; here 32, the
# sizes scaled by 1/4 so that eight ranks sharing ONE GPU finish in a minute): (h, w) per image
CLIC_SHAPES_FULL = [(1365, 2048)] * 14 + [(2048, 1365)] * 8 + [(1152, 2048)] * 6 + [(2048, 1536)] * 4


def test_config4_eight_ranks_clic_shaped_set_and_lpt_balance(offline_home, tmp_path_factory):
    """The 8-rank layout of BASELINE config 4, rehearsed on one GPU: 8 gloo ranks sharing cuda:0, the REAL qarv_base, a 32-image set
    with the CLIC-2022 size mix -> the same dict, to the last bit, as the single-process imcoding_evaluate; and the LPT partition of the
    FULL-size set is balanced: predicted makespan / mean load <= 1.1 (rank::world on the sorted file list: checked to be no better)."""
    import torch.multiprocessing as mp
    import lvae
    from lvae.evaluation import imcoding_evaluate, lpt_partition
    pad = lambda v: (v + 63) // 64 * 64
    costs = [pad(h) * pad(w) for h, w in CLIC_SHAPES_FULL]
    parts = lpt_partition(costs, 8)
    assert sorted(i for p_ in parts for i in p_) == list(range(32))
    loads = [sum(costs[i] for i in p_) for p_ in parts]
    imbalance = max(loads) / (sum(loads) / 8.0)
    naive = [sum(costs[i] for i in range(r, 32, 8)) for r in range(8)]
    print(f'LPT partition of the CLIC-shaped set over 8 ranks: predicted imbalance {imbalance:.3f} (rank::world: {max(naive) / (sum(naive) / 8.0):.3f})')
    assert imbalance <= 1.1 and imbalance <= max(naive) / (sum(naive) / 8.0) + 1e-9
    root = tmp_path_factory.mktemp('clic32')
    rng_sizes = [(h // 4, w // 4) for h, w in CLIC_SHAPES_FULL]
    order = [(i * 13) % 32 for i in range(32)]                      # file order != size order
    _write_pngs(str(root / 'clic32'), [rng_sizes[i] for i in order], 900)
    ckpt = str(offline_home / 'torch_home' / 'hub' / 'checkpoints' / 'qarv_base-2022-dec-12.pt')
    m = lvae.get_model('qarv_base', pretrained=ckpt).to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    single = imcoding_evaluate(m, str(root / 'clic32'))
    del m
    torch.cuda.empty_cache()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 27100 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 8, str(root / 'clic32'), ckpt, port, q)) for r in range(8)]
    for p_ in procs:
        p_.start()
    res = q.get(timeout=900)
    for p_ in procs:
        p_.join(timeout=300)
        assert p_.exitcode == 0
    assert res == single, (res, single)


def test_config4_eval_sharded_script_and_bench_two_ranks(offline_home, tmp_path):
    """scripts/eval-sharded.py and `bench.py --gpus 2` launched by torch.distributed.run exactly as the driver does, in their
    documented 1-GPU rehearsal mode (all ranks on cuda:0, gloo instead of RCCL)."""
    port = 29300 + (os.getpid() % 300)
    launch = ['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
              '--master-port', str(port)]
    out = _run(launch + [os.path.join(REPO, 'scripts', 'eval-sharded.py'), '-m', 'qarv_base', '-n', 'clic2022-test', '-l', '64', '1024',
                         '-s', '2', '--backend', 'gloo'], offline_home, tmp_path, LVAE_SINGLE_GPU_TEST='1')
    lines = [l for l in out.splitlines() if l.startswith('lambda=')]
    assert len(lines) == 2 and all("'bpp'" in l and "'psnr'" in l for l in lines), out
    out = _run(launch[:-1] + [str(port + 1), os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '4',
                              '--no-cpu-baseline', '--no-kernel-timing'], offline_home, tmp_path, LVAE_BENCH_SINGLE_GPU_TEST='1')
    js = [json.loads(l) for l in out.splitlines() if l.startswith('{')]
    assert len(js) == 1                                              # rank 0 only
    j = js[0]
    assert j['n_gpus'] == 2 and j['steps'] == 2 and j['scaling'] == 'weak' and j['config']['global_batch'] == 8
    assert j['unit'] == 'Mpixels/s' and j['value'] > 0 and abs(j['value'] - 8 * 512 * 768 / (j['ms_per_step'] * 1e3)) < 0.01 * j['value']


def test_bench_line_carries_a_measured_roofline(offline_home, tmp_path):
    """The single-GPU bench line with --full (short run): the roofline object is MEASURED in that run -- launches > 0, an average launch
    duration, 0 < frac < 1 -- also now that the product path runs a pipeline group's loop natively (no per-launch hook: the
    roofline pass replays launch by launch), and value = pixels / time."""
    out = _run([os.path.join(REPO, 'bench.py'), '--full', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--fp32-steps', '0',
                '--config5-steps', '0', '--roofline-steps', '1', '--coder-steps', '2', '--size-steps', '1', '--qres-steps', '0'], offline_home, tmp_path)
    j = [json.loads(l) for l in out.splitlines() if l.startswith('{')][0]
    r = j['roofline']
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and r['launches'] > 100 and r['avg_launch_us'] > 5
    assert 0.05 < r['frac'] < 1 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    # ... on the launch mix of the TIMED region: the pass replays the timed region's own plans (two groups of
    # four images, one after the other) -- as many launches of the family per step as those plans hold, none from other plans
    assert r['launches'] == r['launches_per_step'] * 1 == r['timed_plans_launches_per_step'], r
    assert 'groups of 4, 4 images' in r['measured_over'], r['measured_over']
    assert abs(j['value'] - 8 * 512 * 768 / (j['ms_per_step'] * 1e3)) < 0.01 * j['value']
    assert abs(j['ms_per_step'] - j['enc_ms_per_step'] - j['dec_ms_per_step']) < 0.05 * j['ms_per_step']
    # the family per kernel (round 6): the rows add up to the family
    bk = r['by_kernel']
    assert sum(v['launches_per_step'] for v in bk.values()) == r['launches_per_step'] and any(k.startswith('mlp_sk') for k in bk), bk
    # the coder workloads: typical / calibrated / worst case at the headline's batch and for one image; calibrated
    # streams obey their tables (coded size == table entropy) and are NOT mostly modes; the other image sizes of BASELINE.json
    cw = j['coder_workloads']
    for op in ('b8_512x768', 'b1_512x768'):
        for kind in ('typical', 'calibrated', 'worst_case'):
            row = cw[op][kind]
            assert 'error' not in row and row['value'] > 0 and row['dec_ms_per_step'] > 0 and row['dec_ns_per_symbol_single_stream'] > 0, (op, kind, row)
        assert abs(cw[op]['calibrated']['coded_over_table_entropy'] - 1) < 0.02 and cw[op]['calibrated']['mode_hit_rate'] < 0.6
        assert cw[op]['typical']['mode_hit_rate'] > 0.9 and cw[op]['worst_case']['escape_rate'] > 0.05
    assert 'error' not in cw and set(j['other_sizes']) == {'b4_1216x1216', 'b2_1408x2048'}
    assert all('error' not in v and v['value'] > 0 for v in j['other_sizes'].values()), j['other_sizes']
    sp = j['step_spread']            # the timed steps one by one beside the contract's mean: min <= median <= max, the mean inside [min, max]
    for k, mean in (('enc_ms', j['enc_ms_per_step']), ('dec_ms', j['dec_ms_per_step'])):
        assert 0 < sp[k]['min'] <= sp[k]['median'] <= sp[k]['max'] and sp[k]['min'] - 0.05 <= mean <= sp[k]['max'] + 0.05, (k, sp[k], mean)


def test_bench_plain_line_and_dumped_outputs(offline_home, tmp_path):
    """A plain bench run (no --full): exactly the timed steps, the headline keys and none of the side measurements; --dump-outputs
    writes the last timed step's strings and reconstruction, and a second run with the same arguments writes the same arrays."""
    dumps = []
    for i in range(2):
        d = tmp_path / f'dump{i}'
        out = _run([os.path.join(REPO, 'bench.py'), '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)], offline_home, tmp_path)
        j = [json.loads(l) for l in out.splitlines() if l.startswith('{')][0]
        assert j['steps'] == 3 and j['full'] is False and j['higher_is_better'] is True and j['unit'] == 'Mpixels/s'
        assert j['ms_per_step'] > 0 and abs(j['value'] - 8 * 512 * 768 / (j['ms_per_step'] * 1e3)) < 0.01 * j['value']
        assert not {'roofline', 'b1', 'qres34m', 'config5', 'other_sizes', 'coder_workloads', 'host_coder', 'cpu_baseline'} & set(j), sorted(j)
        dumps.append({n: np.load(str(d / f'{n}.npy')) for n in ('bitstream_lengths', 'bitstreams', 'reconstruction')})
    a, b = dumps
    assert a['reconstruction'].dtype == np.float32 and a['reconstruction'].shape == (8, 3, 512, 768)
    assert a['bitstreams'].dtype == np.float32 and a['bitstream_lengths'].dtype == np.float64
    assert a['bitstreams'].size == int(a['bitstream_lengths'].sum()) and a['bitstream_lengths'].shape == (8,)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    # the dumped strings are the path's own: decoding them gives the dumped reconstruction
    raw = a['bitstreams'].astype(np.uint8).tobytes()
    ends = np.cumsum(a['bitstream_lengths'].astype(np.int64))
    strings = [raw[e - n:e] for e, n in zip(ends, a['bitstream_lengths'].astype(np.int64))]
    import bench
    m, _ = bench.build_model(torch.device('cuda', 0))
    m.set_gemm_precision('f16x2')                    # the bench's default arithmetic
    x = m.decompress_batch(strings).cpu().numpy()
    assert np.array_equal(x, a['reconstruction'])


# ------------------------------------------------------------------------------------------------------------------ H2, f2
def test_speedtest_script(offline_home, tmp_path):
    """scripts/speedtest-lvae.py (reference :13-44,76-88)."""
    out = _run([os.path.join(REPO, 'scripts', 'speedtest-lvae.py'), '--synthetic', '5'], offline_home, tmp_path)
    last = out.strip().splitlines()[-1]
    assert last.startswith('encode time=') and 'decode time=' in last, out
    enc, dec = (float(t.split('=')[1].rstrip('s')) for t in last.split(', '))
    assert 0 < enc < 1.0 and 0 < dec < 1.0                        # 512x768 on an MI355X: milliseconds (printed with 3 decimals)
    assert 'Number of parameters: 93.4' in out


def test_eval_var_rate_script(offline_home, tmp_path):
    """eval-var-rate.py (reference :24-61): pretrained=True default, .to() BEFORE compress_mode(), lambda sweep via default_lmb."""
    _run([os.path.join(REPO, 'eval-var-rate.py'), '-m', 'qarv_base', '-n', 'clic2022-test', '-s', '3', '-l', '32', '1024'],
         offline_home, tmp_path)
    res = json.load(open(tmp_path / 'runs' / 'results' / 'clic2022-test-qarv_base.json'))
    assert len(res['lambdas']) == 3 and abs(res['lambdas'][0] - 32) < 1e-3 and abs(res['lambdas'][-1] - 1024) < 1e-2
    bpp, psnr = res['results']['bpp'], res['results']['psnr']
    assert len(bpp) == 3 and all(math.isfinite(v) and v > 0 for v in bpp + psnr)


def test_rate_targeting_script(offline_home, tmp_path):
    """scripts/qarv/test-at-target-bytes.py (reference :17-53): bisection over lambda through compress_file(..., lmb=)."""
    img = str(offline_home / 'datasets' / 'clic' / 'test-2022' / 'im00.png')
    out = _run([os.path.join(REPO, 'scripts', 'qarv', 'test-at-target-bytes.py'), '-i', img, '-b', str(tmp_path / 'x.bits'), '-t', '60000'],
               offline_home, tmp_path)
    its = [l for l in out.splitlines() if l.startswith('iter ')]
    assert its and out.strip().splitlines()[-1].startswith('lambda = ')
    sizes = [int(l.split('bytes=')[1].split('B')[0]) for l in its]
    lmbs = [float(l.split('lmb=')[1].split(',')[0]) for l in its]
    assert all(16 <= v <= 2048 for v in lmbs)
    # the search moves lambda towards the target: a larger-than-target file lowers lambda, a smaller one raises it
    for (s0, l0), l1 in zip(zip(sizes, lmbs), lmbs[1:]):
        assert (l1 < l0) == (s0 > 60000)
    assert os.path.getsize(tmp_path / 'x.bits') == sizes[-1]


def test_eval_theoretical_robust_decoding_and_lossless_scripts(offline_home, tmp_path):
    """The remaining CLIs of SURVEY.md 8(f): scripts/qarv/eval-theoretical.py (reference :8-31, `pretrained=True` default),
    scripts/qarv/robust-decoding.py in all four modes (reference :38-56) and scripts/qresvae/evaluate-lossless.py."""
    out = _run([os.path.join(REPO, 'scripts', 'qarv', 'eval-theoretical.py'), '-n', 'clic2022-test', '-s', '2', '-l', '64', '512'],
               offline_home, tmp_path)
    assert '================ clic2022-test ================' in out
    rows = {l.split('=')[0].strip(): l for l in out.splitlines() if '= [' in l}
    assert {'loss', 'bpp', 'psnr', 'lambda'} <= set(rows) and rows['bpp'].count(',') == 1
    for mode in ('progressive', 'exclude', 'reverse', 'single'):
        out = _run([os.path.join(REPO, 'scripts', 'qarv', 'robust-decoding.py'), '--synthetic', '128', '192', '--mode', mode,
                    '--out', str(tmp_path / f'{mode}.png')], offline_home, tmp_path)
        assert out.count(f'{mode}=') == 9, out                       # one line per latent block (anchor)
        assert os.path.getsize(tmp_path / f'{mode}.png') > 0
    out = _run([os.path.join(REPO, 'scripts', 'qresvae', 'evaluate-lossless.py'), '--synthetic', '3'], offline_home, tmp_path)
    assert 'Average bpp:' in out and float(out.split('Average bpp:')[1].split()[0]) > 0, out      # asserts bit-exact round trips inside


# ------------------------------------------------------------------------------------------------------------------ published numbers
@pytest.mark.parametrize('model,dataset', [('qarv_base', 'kodak'), ('qres34m', 'kodak')])
def test_published_numbers_acceptance_gate(model, dataset):
    """north_star: "identical bpp/PSNR on Kodak".  With the reference's TRAINED checkpoints in torch.hub's cache and the Kodak folder in
    place, scripts/accept-published.py must reproduce every published point (reference results/kodak/kodak-qarv_base.json:25-78,
    kodak-qres34m.json:15-44) within 0.5 % bpp / 0.02 dB.  This build is offline -- no weights, no Kodak -- so the test SKIPS here;
    it is the one command to run the day they are present."""
    sys.path.insert(0, os.path.join(REPO, 'scripts'))
    import importlib
    gate = importlib.import_module('accept-published')
    case = json.load(open(gate.FIXTURE))['cases'][model][dataset]
    miss = gate.missing_inputs(model, dataset, case)
    if miss:
        pytest.skip('trained weights / test images not available offline: ' + ', '.join(os.path.basename(m) for m in miss))
    r = subprocess.run([sys.executable, os.path.join(REPO, 'scripts', 'accept-published.py'), '-m', model, '-n', dataset],
                       capture_output=True, text=True, timeout=3600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def _nccl_world1_worker(dataset, ckpt, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))      # backend "nccl" IS RCCL on ROCm
    import lvae
    from lvae.evaluation import gather_stats, imcoding_evaluate_sharded
    m = lvae.get_model('qarv_base', pretrained=ckpt).to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    res = imcoding_evaluate_sharded(m, dataset)                    # its all_gather runs on device tensors over RCCL
    rows = gather_stats([[2.0, 0.5, 1e-3, 30.0], [0.0, 0.25, 2e-3, 27.0]], 1, torch.device('cuda', 0))
    # bench.py's collectives as well: max-over-ranks of the timing pair, all_gather of (bpp, mse)
    t = torch.tensor([1.5, 0.5], dtype=torch.float64, device='cuda:0')
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    q.put((res, rows.tolist(), t.tolist(), dist.get_backend()))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_branch_initialises_and_collates_world1(offline_home):
    """The RCCL ('nccl') branch of the multi-GPU path -- init_process_group with a device id, the device-tensor all_gather of
    imcoding_evaluate_sharded / gather_stats, bench.py's all_reduce(MAX) -- executed for real on the one GPU there is (world size 1):
    same dict as the single-process evaluation.  The 8-GPU curve itself is the driver's to take."""
    import torch.multiprocessing as mp
    import lvae
    from lvae.evaluation import imcoding_evaluate
    ckpt = str(offline_home / 'torch_home' / 'hub' / 'checkpoints' / 'qarv_base-2022-dec-12.pt')
    dataset = str(offline_home / 'datasets' / 'clic' / 'test-2022')
    m = lvae.get_model('qarv_base', pretrained=ckpt).to('cuda:0').eval()
    m.compress_mode()
    m.default_lmb = 256.0
    single = imcoding_evaluate(m, dataset)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_world1_worker, args=(dataset, ckpt, 29900 + (os.getpid() % 90), q))
    p.start()
    res, rows, t, backend = q.get(timeout=900)
    p.join(timeout=120)
    assert p.exitcode == 0 and backend == 'nccl'
    assert res == single, (res, single)
    assert rows == [[0.0, 0.25, 2e-3, 27.0], [2.0, 0.5, 1e-3, 30.0]] and t == [1.5, 0.5]
