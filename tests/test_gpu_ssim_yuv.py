"""-m gpu: SSIM / MS-SSIM on the planes of YUV frames on the HIP kernels (lvae.metrics.ssim_yuv / ms_ssim_yuv / ssim ->
lvae_msssim_planes) against the fp64 yardstick of tests/test_metrics_host.py on the codes (tests/test_ssim_yuv_host.py builds the frames
and states the yardsticks), the bit equalities between the sample loaders, and the `metrics` option of yuv_evaluate with the real qarv_base.

Shapes: the output tile is 28 x 32 and the halo 10, so 11 x 11 has one valid pixel, 12 x 43 a valid width of 33 that straddles a tile column,
39 x 12 a valid height of 29 that straddles a tile row; a 161 x 163 chroma plane is the smallest MS-SSIM input and odd at every pooling step.

Bound: 1e-6 absolute on every value and every per-scale mean -- the bound of tests/test_gpu_msssim.py for the reason its docstring gives:
the arithmetic is the same (fp64 moments of samples that are exact as floats), one step of the noise levels moves a value by far more
than 1e-3 and the two data-range conventions differ by more than 5e-7 on each side (tests/test_ssim_yuv_host.py).  The measured errors are
printed (pytest -s) and, when LVAE_SSIM_YUV_REPORT names a file, appended to it (profiles/r17_ssim_yuv_parity.txt is such a file)."""
import os

import numpy as np
import pytest
import torch

from test_metrics_host import _ssim, gauss, image01, noisy
from test_ssim_yuv_host import (SIGMAS, frame_codes, frame_pair, make_frame, ms_ssim_codes_fp64, noisy_codes, plane_sizes, ssim_codes_fp64)

pytestmark = pytest.mark.gpu

BOUND = 1e-6
DEV = 'cuda:0'


def _report(line):
    print(line)
    path = os.environ.get('LVAE_SSIM_YUV_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _cases(h, w, depth, sub, cls):
    """[(name, ref frame, rec frame, ref codes, rec codes)] on the CPU: identical, three noise levels, all-0 against all-L."""
    L = (1 << depth) - 1
    out = [('identical',) + frame_pair(h, w, depth, sub, 11, 0, cls)]
    out += [(f'noise sigma {s}',) + frame_pair(h, w, depth, sub, 11, s, cls) for s in SIGMAS]
    zero = [torch.zeros(s, dtype=torch.int64) for s in plane_sizes(h, w, sub)]
    full = [torch.full(s, L, dtype=torch.int64) for s in plane_sizes(h, w, sub)]
    return out + [('0 / L', make_frame(zero, depth, sub, cls), make_frame(full, depth, sub, cls), zero, full)]


def _check_ssim(tag, cases, depth, data_range=None):
    """ONE ssim_yuv call for all cases on the GPU against the yardstick; -> the per-frame dicts."""
    from lvae.metrics import ssim_yuv
    L = (1 << depth) - 1 if data_range is None else data_range
    got = ssim_yuv([c[1].to(DEV) for c in cases], [c[2].to(DEV) for c in cases], data_range=data_range)
    worst = 0.0
    for row, (name, _, _, ra, rb) in zip(got, cases):
        assert set(row) == {'ssim-y', 'ssim-u', 'ssim-v'}
        for p, x, y in zip('yuv', ra, rb):
            ref = ssim_codes_fp64(x, y, L)
            err = abs(row['ssim-' + p] - ref)
            _report(f'{tag} {name} {p} {tuple(x.shape)}: kernel {row["ssim-" + p]:.12f} yardstick {ref:.12f} |d| {err:.3e}')
            worst = max(worst, err)
    _report(f'{tag} WORST |d| {worst:.3e} (bound {BOUND:g})')
    assert worst <= BOUND, worst
    assert got[0] == {'ssim-y': 1.0, 'ssim-u': 1.0, 'ssim-v': 1.0}                      # identical frames: exactly 1
    return got


# ----------------------------------------------------------------------------------------------- single-scale SSIM
@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('h,w', [(11, 11), (12, 43), (39, 12)])
def test_ssim_single_planes(h, w, depth):
    _check_ssim(f'ssim {depth}-bit {h}x{w}', _cases(h, w, depth, '444', 'yuv'), depth)


@pytest.mark.parametrize('h,w,depth,sub,cls', [(78, 86, 8, '420', '420'), (78, 86, 10, '420', 'yuv'), (78, 86, 12, '420', 'yuv'),
                                               (40, 86, 10, '422', 'yuv'), (22, 22, 8, '444', 'yuv')])
def test_ssim_frames(h, w, depth, sub, cls):
    """Frames against the yardstick, and the other layouts of the same codes to the bit: NV12 for 8-bit 4:2:0, P010 / P210 / P012 (with
    garbage in the low bits of the words) for 10 / 12 bits at 4:2:0 / 4:2:2."""
    from lvae.metrics import ssim_yuv
    from lvae.utils.yuv import YuvSpFrame
    cases = _cases(h, w, depth, sub, cls)
    got = _check_ssim(f'ssim {depth}-bit {sub} {h}x{w}', cases, depth)
    ref, rec = [c[1].to(DEV) for c in cases], [c[2].to(DEV) for c in cases]
    again = ssim_yuv(ref, rec)
    assert again == got                                                                 # a repeated call: the same bits
    assert ssim_yuv(ref, rec, planes='y') == [{'ssim-y': r['ssim-y']} for r in got]
    if cls == '420':
        other = lambda fs: [f.as_format('nv12') for f in fs]
    elif sub in ('420', '422') and depth > 8:
        def other(fs):
            out = []
            for k, f in enumerate(fs):
                sp = f.to_semiplanar()
                g = torch.Generator().manual_seed(50 + k)
                junk = lambda p: (p.to(torch.int32) | torch.randint(0, 1 << (16 - depth), p.shape, generator=g).to(p.device)).to(torch.int16)
                out.append(YuvSpFrame(junk(sp.y), junk(sp.uv), depth, sub))
            return out
    else:
        return
    assert ssim_yuv(other(ref), other(rec)) == got


def test_ssim_convention_and_containers():
    """data_range: the HM-style peak 1020 at 10 bits differs from the default 1023 on the GPU as on the CPU, each side within the bound of
    its own yardstick.  8-bit codes held in 16-bit low-bit planes with data_range 255 give the bits of the uint8 planes."""
    from lvae.metrics import ssim_yuv
    from lvae.utils.yuv import YuvFrame
    cases = _cases(78, 86, 10, '420', 'yuv')
    d1023 = _check_ssim('ssim 10-bit 420 78x86 L=1023', cases, 10)
    d1020 = _check_ssim('ssim 10-bit 420 78x86 L=1020', cases, 10, data_range=1020)
    for i in (2, 3):                                                                    # sigma 8 and 32
        assert abs(d1023[i]['ssim-y'] - d1020[i]['ssim-y']) > 5e-7
    c8 = _cases(78, 86, 8, '420', 'yuv')
    wide = lambda f: YuvFrame(*[p.to(torch.int16) for p in f.planes()], depth=10, subsampling='420')
    ref8, rec8 = [c[1].to(DEV) for c in c8], [c[2].to(DEV) for c in c8]
    assert ssim_yuv([wide(f) for f in ref8], [wide(f) for f in rec8], data_range=255) == ssim_yuv(ref8, rec8)


@pytest.mark.parametrize('depth', [8, 10])
def test_views_batching_and_determinism(depth):
    """Planes that are views into larger tensors (row stride above w, odd offsets, seeded garbage around them) give the bits of contiguous
    copies; row i of a call with frames of two sizes equals the single-frame call."""
    from lvae.metrics import ssim_yuv
    from lvae.utils.yuv import YuvFrame
    dtype = torch.uint8 if depth == 8 else torch.int16
    g = torch.Generator().manual_seed(9)

    def embedded(f):
        planes = []
        for p in f.planes():
            h, w = p.shape
            big = torch.randint(0, 1 << depth, (h + 5, w + 9), generator=g).to(dtype).to(DEV)
            big[2:2 + h, 3:3 + w] = p.to(DEV)
            planes.append(big[2:2 + h, 3:3 + w])
        return YuvFrame(*planes, depth=depth, subsampling=f.subsampling)
    a1, b1, _, _ = frame_pair(78, 86, depth, '420', 21, 8)
    a2, b2, _, _ = frame_pair(22, 24, depth, '420', 22, 32)
    va, vb = [embedded(a1), embedded(a2)], [embedded(b1), embedded(b2)]
    assert va[0].y.stride(0) == 95 and not va[0].y.is_contiguous()
    both = ssim_yuv(va, vb)
    assert both == ssim_yuv([a1.to(DEV), a2.to(DEV)], [b1.to(DEV), b2.to(DEV)])
    assert both == ssim_yuv(va, vb)
    assert both[0] == ssim_yuv(a1.to(DEV), b1.to(DEV)) and both[1] == ssim_yuv(va[1], vb[1])
    assert both[1] == ssim_yuv(a2, b2.to(DEV))                                          # one side on the CPU: uploaded, the same bits


# ----------------------------------------------------------------------------------------------- MS-SSIM
@pytest.mark.parametrize('h,w,depth,planes,cls', [(322, 326, 10, 'yuv', 'yuv'), (162, 164, 8, 'y', '420')])
def test_ms_ssim_frames(h, w, depth, planes, cls):
    from lvae.metrics import ms_ssim_yuv
    from lvae.utils.yuv import YuvFrame
    L = (1 << depth) - 1
    cases = _cases(h, w, depth, '420', cls)
    ref, rec = [c[1].to(DEV) for c in cases], [c[2].to(DEV) for c in cases]
    got, means = ms_ssim_yuv(ref, rec, planes=planes, return_scales=True)
    assert means.shape == (len(cases), len(planes), 5) and means.dtype == torch.float64
    worst = worst_m = 0.0
    for i, (name, _, _, ra, rb) in enumerate(cases):
        assert set(got[i]) == {'ms-ssim-' + p for p in planes}
        for j, p in enumerate(planes):
            x, y = ra['yuv'.index(p)], rb['yuv'.index(p)]
            ref_v, ref_m = ms_ssim_codes_fp64(x, y, L)
            err, err_m = abs(got[i]['ms-ssim-' + p] - ref_v), float((means[i, j] - ref_m).abs().max())
            _report(f'ms-ssim {depth}-bit {h}x{w} {name} {p} {tuple(x.shape)}: kernel {got[i]["ms-ssim-" + p]:.12f} yardstick {ref_v:.12f} '
                    f'|d| {err:.3e} per-scale means max|d| {err_m:.3e}')
            worst, worst_m = max(worst, err), max(worst_m, err_m)
    _report(f'ms-ssim {depth}-bit {h}x{w} WORST |d| {worst:.3e}, per-scale means {worst_m:.3e} (bound {BOUND:g})')
    assert worst <= BOUND and worst_m <= BOUND, (worst, worst_m)
    assert all(v == 1.0 for v in got[0].values())
    again, means2 = ms_ssim_yuv(ref, rec, planes=planes, return_scales=True)
    assert again == got and torch.equal(means, means2)
    one, m1 = ms_ssim_yuv(ref[2], rec[2], planes=planes, return_scales=True)
    assert one == got[2] and torch.equal(m1, means[2])
    if depth > 8:                                                                       # P010, garbage-free: the bits of the planar frames
        sp, sm = ms_ssim_yuv([f.to_semiplanar() for f in ref], [f.to_semiplanar() for f in rec], planes=planes, return_scales=True)
        assert sp == got and torch.equal(sm, means)
    else:                                                                               # NV12 and the general 8-bit frame class
        assert ms_ssim_yuv([f.as_format('nv12') for f in ref], [f.as_format('nv12') for f in rec], planes=planes) == got
        assert ms_ssim_yuv([YuvFrame(*f.planes()) for f in ref], [YuvFrame(*f.planes()) for f in rec], planes=planes) == got
        with pytest.raises(ValueError, match='plane u of frame 0 is 81x82'):
            ms_ssim_yuv(ref, rec, planes='yuv')


# ----------------------------------------------------------------------------------------------- ssim on float RGB
def test_ssim_on_float_rgb():
    from lvae.metrics import ssim
    x = torch.cat([image01(40, 50, 1), image01(40, 50, 2, 'noise')], 0)
    y = noisy(x, 0.05, 7)
    got = ssim(x.to(DEV), y.to(DEV))
    ref = _ssim(x.double(), y.double(), gauss())[0].mean(1)
    err = float((got.cpu() - ref).abs().max())
    _report(f'ssim float RGB 2 x 3x40x50: max|d| {err:.3e} (bound {BOUND:g})')
    assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda and err <= BOUND
    assert torch.equal(ssim(x.to(DEV), x.to(DEV)).cpu(), torch.ones(2, dtype=torch.float64))
    pad = torch.rand(2, 3, 48, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    pad[:, :, :40, :50] = y.to(DEV)
    assert torch.equal(ssim(x.to(DEV), pad, sizes=[(40, 50)] * 2), got)                 # read in place inside a padded batch
    x = image01(161, 161, 31)                                                           # the smallest input of tests/test_gpu_msssim.py
    v = float(ssim(x.to(DEV), noisy(x, 0.05, 3).to(DEV)))
    assert np.isfinite(v) and 0.0 < v <= 1.0
    assert abs(v - float(_ssim(x.double(), noisy(x, 0.05, 3).double(), gauss())[0].mean())) <= BOUND


# ----------------------------------------------------------------------------------------------- the harness
def _yardstick_means(ref, rec, L):
    acc = {'ssim-' + p: 0.0 for p in 'yuv'}
    for a, b in zip(ref, rec):
        for p in 'yuv':
            acc['ssim-' + p] += ssim_codes_fp64(getattr(a, p).cpu().to(torch.int64), getattr(b, p).cpu().to(torch.int64), L)
    return {k: v / len(ref) for k, v in acc.items()}


@pytest.mark.parametrize('layout', ['i420', 'p010'])
def test_yuv_evaluate_metrics_option(product_model, tmp_path, layout):
    from lvae.evaluation import yuv_evaluate
    from lvae.utils.yuv import read_yuv420, read_yuv_sp, write_yuv420, write_yuv_sp
    m, path = product_model, str(tmp_path / 'clip.yuv')
    if layout == 'i420':
        write_yuv420([make_frame(frame_codes(128, 192, 8, '420', 80 + i), 8, '420', '420') for i in range(2)], path)
        kw, L = dict(lmb=256), 255
        frames = [f.to(DEV) for f in read_yuv420(path, 192, 128)]
        recs = m.decompress_yuv420(m.compress_yuv420(frames, lmb=256))
    else:
        write_yuv_sp([make_frame(frame_codes(128, 192, 10, '420', 90 + i), 10, '420', 'sp') for i in range(2)], path)
        kw, L = dict(lmb=256, depth=10, layout='semiplanar'), 1023
        frames = [f.to(DEV) for f in read_yuv_sp(path, 192, 128, 10, '420')]
        recs = m.decompress_yuv(m.compress_yuv(frames, siting='center', lmb=256), depth=10, subsampling='420', siting='center', layout='semiplanar')
        frames, recs = [f.to_planar() for f in frames], [f.to_planar() for f in recs]
    base = yuv_evaluate(m, path, 192, 128, batch=2, **kw)
    assert yuv_evaluate(m, path, 192, 128, batch=2, metrics=('psnr',), **kw) == base
    both = yuv_evaluate(m, path, 192, 128, batch=2, metrics=('psnr', 'ssim'), **kw)
    assert set(both) == set(base) | {'ssim-y', 'ssim-u', 'ssim-v'}
    for k in base:
        assert both[k] == base[k], k
    ref = _yardstick_means(frames, recs, L)
    for k, v in ref.items():
        _report(f'yuv_evaluate {layout} 2 x 128x192 {k}: {both[k]:.12f} yardstick mean {v:.12f} |d| {abs(both[k] - v):.3e}')
        assert abs(both[k] - v) <= BOUND and 0.0 < both[k] < 1.0
    assert yuv_evaluate(m, path, 192, 128, batch=1, metrics=('psnr', 'ssim'), **kw) == both
    with pytest.raises(ValueError, match='128x192'):
        yuv_evaluate(m, path, 192, 128, batch=2, metrics=('ms-ssim',), **kw)
