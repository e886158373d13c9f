"""not-gpu: SSIM / MS-SSIM on the planes of YUV frames (lvae.metrics.ssim, ssim_yuv, ms_ssim_yuv) on CPU frames against the fp64
yardstick of tests/test_metrics_host.py evaluated on the CODES with C1 = (0.01 L)^2, C2 = (0.03 L)^2, the properties of that
yardstick the GPU bound relies on, the argument errors, and the -22 cases of lvae_msssim_planes.  tests/test_gpu_ssim_yuv.py imports the
frame builders and the yardsticks below."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seeded_init
from test_metrics_host import W5, _ssim, gauss, image01, noisy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (2, 8, 32)                     # noise levels in 8-bit codes (scaled by 2^(depth - 8) above 8 bits)
SHIFT = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}          # subsampling -> (horizontal, vertical) shift of the chroma planes


# ----------------------------------------------------------------------------------------------- planes, frames, yardsticks
def codes(h, w, depth=8, seed=0, ch=0):
    """(h, w) int64 codes of `depth` bits: channel `ch` of a seeded synthetic image << (depth - 8), plus seeded low bits."""
    c = seeded_init.synthetic_image_u8(h, w, seed)[..., ch].astype(np.int64) << (depth - 8)
    if depth > 8:
        c = c + np.random.default_rng(1000 + seed).integers(0, 1 << (depth - 8), size=(h, w))
    return torch.from_numpy(np.ascontiguousarray(c))


def noisy_codes(c, sigma, depth, seed):
    """c + N(0, (sigma 2^(depth - 8))^2), rounded and clipped to the codes of `depth` bits."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(c.shape, generator=g, dtype=torch.float64) * (sigma * (1 << (depth - 8)))
    return (c.double() + n).round().clamp(0, (1 << depth) - 1).to(torch.int64)


def plane_sizes(h, w, sub):
    sx, sy = SHIFT[sub]
    return [(h, w), (h >> sy, w >> sx), (h >> sy, w >> sx)]


def frame_codes(h, w, depth, sub, seed):
    """[y, u, v] int64 code planes of one frame."""
    return [codes(ph, pw, depth, seed, ch) for ch, (ph, pw) in enumerate(plane_sizes(h, w, sub))]


def make_frame(planes, depth, sub, cls='yuv'):
    """int64 code planes -> a CPU frame: 'yuv' YuvFrame, '420' Yuv420Frame (I420), 'nv12' Yuv420Frame (NV12), 'sp' YuvSpFrame."""
    from lvae.utils.yuv import Yuv420Frame, YuvFrame
    t = [p.to(torch.uint8 if depth == 8 else torch.int16) for p in planes]
    if cls in ('420', 'nv12'):
        return Yuv420Frame('i420', *t).as_format('i420' if cls == '420' else 'nv12')
    fr = YuvFrame(*t, depth=depth, subsampling=sub)
    return fr.to_semiplanar() if cls == 'sp' else fr


def frame_pair(h, w, depth, sub, seed, sigma, cls='yuv'):
    """(ref frame, rec frame, ref code planes, rec code planes): rec = ref + noise of `sigma` 8-bit codes (0: identical)."""
    ref = frame_codes(h, w, depth, sub, seed)
    rec = [noisy_codes(p, sigma, depth, 7 + i) if sigma else p.clone() for i, p in enumerate(ref)]
    return make_frame(ref, depth, sub, cls), make_frame(rec, depth, sub, cls), ref, rec


def constants(L):
    return (0.01 * L) ** 2, (0.03 * L) ** 2


def ssim_codes_fp64(x, y, L):
    """The yardstick on one pair of (h, w) code planes: _ssim on the codes as fp64 with the constants of data range L -> float."""
    C1, C2 = constants(L)
    return float(_ssim(x.double()[None, None], y.double()[None, None], gauss(), C1, C2)[0])


def ms_ssim_codes_fp64(x, y, L):
    """ms_ssim_fp64 of tests/test_metrics_host.py with the constants of data range L on one pair of code planes (that function fixes
    L = 1): the same pieces in the same order -> (float, (5,) per-scale means before the relu)."""
    C1, C2 = constants(L)
    x, y, g, raw = x.double()[None, None], y.double()[None, None], gauss(), []
    assert min(x.shape[-2:]) > 160
    for i in range(5):
        ss, cs = _ssim(x, y, g, C1, C2)
        raw.append(cs if i < 4 else ss)
        if i < 4:
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    m = torch.stack(raw, 0).view(5)
    return float(torch.prod(torch.relu(m) ** torch.tensor(W5, dtype=torch.float64))), m


# ----------------------------------------------------------------------------------------------- the CPU paths
@pytest.mark.parametrize('depth,sub,cls', [(8, '420', '420'), (8, '420', 'nv12'), (8, '444', 'yuv'), (10, '420', 'yuv'), (12, '422', 'yuv'),
                                           (10, '420', 'sp'), (12, '422', 'sp')])
def test_cpu_ssim_yuv_equals_yardstick(depth, sub, cls):
    from lvae.metrics import ssim_yuv
    L = (1 << depth) - 1
    for sigma in SIGMAS:
        a, b, ra, rb = frame_pair(78, 86, depth, sub, 3, sigma, cls)
        got = ssim_yuv(a, b)
        assert set(got) == {'ssim-y', 'ssim-u', 'ssim-v'} and all(isinstance(v, float) for v in got.values())
        for name, x, y in zip('yuv', ra, rb):
            assert abs(got['ssim-' + name] - ssim_codes_fp64(x, y, L)) <= 1e-12, (name, sigma)
        assert ssim_yuv([a], [b], planes='y') == [{'ssim-y': got['ssim-y']}]


def test_cpu_ms_ssim_yuv_equals_yardstick():
    from lvae.metrics import ms_ssim_yuv
    a, b, ra, rb = frame_pair(322, 326, 10, '420', 5, 8)
    got, m = ms_ssim_yuv([a], [b], planes='yuv', return_scales=True)
    assert set(got[0]) == {'ms-ssim-y', 'ms-ssim-u', 'ms-ssim-v'} and m.shape == (1, 3, 5)
    for j, (name, x, y) in enumerate(zip('yuv', ra, rb)):
        ref, ref_m = ms_ssim_codes_fp64(x, y, 1023)
        assert abs(got[0]['ms-ssim-' + name] - ref) <= 1e-12 and float((m[0, j] - ref_m).abs().max()) <= 1e-12, name
    assert ms_ssim_yuv(a, b) == {'ms-ssim-y': got[0]['ms-ssim-y']}          # luma alone is the default


def test_cpu_ssim_on_float_images_equals_yardstick():
    from lvae.metrics import ssim
    x = torch.cat([image01(40, 50, 1), image01(40, 50, 2, 'noise')], 0)
    y = noisy(x, 0.05, 7)
    got = ssim(x, y)
    ref = _ssim(x.double(), y.double(), gauss())[0].mean(1)
    assert got.dtype == torch.float64 and got.shape == (2,) and float((got - ref).abs().max()) <= 1e-12
    assert ssim(x, x).tolist() == [1.0, 1.0]
    one = ssim([x[0, :, :11, :30]], [y[0, :, :11, :30]])                     # views; 11 rows: one valid row
    assert abs(float(one) - float(_ssim(x[:1, :, :11, :30].double(), y[:1, :, :11, :30].double(), gauss())[0].mean())) <= 1e-12
    with pytest.raises(ValueError, match='10x50'):
        ssim(x[:, :, :10], y[:, :, :10])


@pytest.mark.parametrize('depth', [8, 10, 12])
def test_identical_frames_and_black_against_white(depth):
    """Identical frames: exactly 1.  All-0 against all-L planes: the moments are exact, the covariance terms cancel, and what is left is
    C1 / (L^2 + C1) = 1e-4 / 1.0001 = 9.999e-5 at every depth."""
    from lvae.metrics import ssim_yuv
    L = (1 << depth) - 1
    a, _, _, _ = frame_pair(22, 22, depth, '444', 2, 0)
    assert ssim_yuv(a, a) == {'ssim-y': 1.0, 'ssim-u': 1.0, 'ssim-v': 1.0}
    zero = make_frame([torch.zeros(22, 22, dtype=torch.int64)] * 3, depth, '444')
    full = make_frame([torch.full((22, 22), L, dtype=torch.int64)] * 3, depth, '444')
    C1, _ = constants(L)
    for v in ssim_yuv(zero, full).values():
        assert abs(v - C1 / (L * L + C1)) <= 1e-12 and abs(v - 9.999e-5) < 1e-8


@pytest.mark.parametrize('h,w', [(11, 11), (78, 86)])
def test_yardstick_orders_the_noise_levels(h, w):
    """More noise, lower value, in steps of far more than 1e-3: the 1e-6 of the GPU tests tells the levels apart (0.997 / 0.936 / 0.533
    on the 11 x 11 plane, 0.992 / 0.889 / 0.388 at 78 x 86)."""
    x = codes(h, w, 8, 3)
    v = [ssim_codes_fp64(x, noisy_codes(x, s, 8, 7), 255) for s in SIGMAS]
    assert 1.0 > v[0] > v[1] + 1e-3 and v[1] > v[2] + 1e-3 and v[2] > 0.0, v


@pytest.mark.parametrize('h,w', [(11, 11), (78, 86)])
def test_scale_invariance_and_the_data_range_convention(h, w):
    """8-bit codes at data_range 255 and the same codes x 4 as a 10-bit frame at data_range 1020 give the same value; the default range
    of a 10-bit frame, 1023, gives another one -- by more than 5e-7 for sigma 8 and 32, so the GPU bound of 1e-6 on each side tells the
    two conventions apart."""
    from lvae.metrics import ssim_yuv
    from lvae.utils.yuv import YuvFrame
    for sigma in SIGMAS:
        x = codes(h, w, 8, 3)
        y = noisy_codes(x, sigma, 8, 7)
        f8 = lambda p: YuvFrame(*[p.to(torch.uint8)] * 3, depth=8, subsampling='444')
        f10 = lambda p: YuvFrame(*[(p * 4).to(torch.int16)] * 3, depth=10, subsampling='444')
        v8 = ssim_yuv(f8(x), f8(y), planes='y', data_range=255)['ssim-y']
        assert v8 == ssim_yuv(f8(x), f8(y), planes='y')['ssim-y']                       # the default at depth 8 IS 255
        v1020 = ssim_yuv(f10(x), f10(y), planes='y', data_range=1020)['ssim-y']
        v1023 = ssim_yuv(f10(x), f10(y), planes='y')['ssim-y']
        assert abs(v8 - v1020) <= 1e-15, (sigma, v8, v1020)
        assert abs(v1023 - ssim_codes_fp64(x * 4, y * 4, 1023)) <= 1e-12
        if sigma >= 8:
            assert 5e-7 < abs(v1023 - v1020) < 1e-3, (sigma, v1023, v1020)


def test_argument_errors():
    from lvae.metrics import ms_ssim_yuv, ssim_yuv
    a8, b8, _, _ = frame_pair(78, 86, 8, '420', 1, 8)
    a10, b10, _, _ = frame_pair(78, 86, 10, '420', 1, 8)
    sp10 = a10.to_semiplanar()
    small, _, _, _ = frame_pair(40, 44, 8, '420', 1, 8)
    with pytest.raises(ValueError):
        ssim_yuv(a8, b10)                                                    # depths
    with pytest.raises(ValueError):
        ssim_yuv(a10, sp10)                                                  # kinds: low-bit against high-bit words
    with pytest.raises(ValueError):
        ssim_yuv([a8, a10], [b8, b10])                                       # the frames of one call share kind and depth
    with pytest.raises(ValueError):
        ssim_yuv(a8, small)                                                  # sizes
    with pytest.raises(ValueError):
        ssim_yuv([a8, a8], [b8])
    with pytest.raises(ValueError):
        ssim_yuv(a8, torch.zeros(78, 86))
    for bad in ('uv', 'YUV', '', None):
        with pytest.raises(ValueError, match='planes'):
            ssim_yuv(a8, b8, planes=bad)
    with pytest.raises(ValueError, match='data_range'):
        ssim_yuv(a8, b8, data_range=0)
    tiny, _, _, _ = frame_pair(20, 24, 8, '420', 1, 0)                       # chroma 10 x 12
    assert set(ssim_yuv(tiny, tiny, planes='y')) == {'ssim-y'}
    with pytest.raises(ValueError, match='plane u of frame 0 is 10x12'):
        ssim_yuv(tiny, tiny)
    big, _, _, _ = frame_pair(320, 322, 8, '420', 1, 0)                      # chroma 160 x 161
    assert ms_ssim_yuv(big, big) == {'ms-ssim-y': 1.0}
    with pytest.raises(ValueError, match='plane u of frame 0 is 160x161'):
        ms_ssim_yuv(big, big, planes='yuv')
    with pytest.raises(ValueError, match='plane y of frame 1 is 78x86'):
        ms_ssim_yuv([big, a8], [big, b8])


# ----------------------------------------------------------------------------------------------- the C-ABI entry without a GPU
def _call(L, x, y, x_row, y_row, hw, pix, n, kind, depth, data_range, scales, out, means, ws, ws_bytes):
    arr = lambda t, v: None if v is None else (t * len(v))(*v)
    flat = None if hw is None else [v for p in hw for v in p]
    return L.lvae_msssim_planes(arr(ctypes.c_void_p, x), arr(ctypes.c_long, x_row), arr(ctypes.c_void_p, y), arr(ctypes.c_long, y_row),
                                arr(ctypes.c_int, flat), arr(ctypes.c_int, pix), n, kind, depth, data_range, scales, out, means, ws, ws_bytes, None)


def test_native_entry_rejects_bad_arguments_without_gpu():
    """-22 before any HIP call: safe on a GPU-less host.  The 'device' pointers are host buffers nothing dereferences."""
    from lvae import _native
    L = _native.lib()
    F32, U8, LOW, HIGH = (_native.SAMPLE_KINDS.index(k) for k in ('f32', 'u8', 'u16_low', 'u16_high'))
    size = L.lvae_msssim_planes_workspace_bytes
    need1, need5 = size(2, 200, 400, 1), size(2, 200, 400, 5)
    assert 0 < need1 < need5 and need1 % 8 == 0 and need5 % 8 == 0 and size(3, 200, 400, 5) > need5
    assert size(2, 160, 400, 5) == 0 and size(2, 160, 400, 1) > 0 and size(2, 10, 400, 1) == 0 and size(2, 11, 11, 1) > 0
    assert size(0, 200, 400, 1) == 0 and size(2, 200, 400, 2) == 0 and size(2, 200, 400, 0) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    good = dict(x=[p, p], y=[p, p], x_row=[400, 200], y_row=[400, 200], hw=[(200, 400), (100, 200)], pix=[1, 1], n=2, kind=LOW, depth=10,
                data_range=1023.0, scales=1, out=p, means=p, ws=p, ws_bytes=need1)
    for k in ('x', 'y', 'x_row', 'y_row', 'hw', 'pix', 'out', 'means', 'ws'):
        assert _call(L, **{**good, k: None}) == -22, k
    assert _call(L, **{**good, 'x': [p, None]}) == -22 and _call(L, **{**good, 'y': [None, p]}) == -22          # an entry of a table
    assert _call(L, **{**good, 'n': 0}) == -22
    assert _call(L, **{**good, 'hw': [(200, 400), (10, 200)]}) == -22                   # a side below 11 at one scale
    assert _call(L, **{**good, 'hw': [(200, 400), (100, 10)]}) == -22
    assert _call(L, **{**good, 'scales': 5, 'ws_bytes': need5}) == -22                  # 100 x 200 is below 161 at five scales
    assert _call(L, **{**good, 'x_row': [399, 200]}) == -22 and _call(L, **{**good, 'y_row': [400, 199]}) == -22
    assert _call(L, **{**good, 'pix': [1, 2]}) == -22                                   # w * pixstride beyond the row
    assert _call(L, **{**good, 'pix': [1, 3], 'x_row': [400, 600], 'y_row': [400, 600]}) == -22
    assert _call(L, **{**good, 'pix': [1, 0]}) == -22
    for depth in (0, 9, 11, 16):
        assert _call(L, **{**good, 'depth': depth}) == -22, depth
        assert _call(L, **{**good, 'depth': depth, 'kind': HIGH}) == -22, depth
    assert _call(L, **{**good, 'kind': U8, 'depth': 10}) == -22
    assert _call(L, **{**good, 'kind': -1}) == -22 and _call(L, **{**good, 'kind': 4}) == -22
    for scales in (0, 2, 4, 6):
        assert _call(L, **{**good, 'scales': scales}) == -22, scales
    for rng in (0.0, -1.0, float('nan'), float('inf'), 65536.0):
        assert _call(L, **{**good, 'data_range': rng}) == -22, rng
    assert _call(L, **{**good, 'ws_bytes': need1 - 1}) == -22
    big = dict(good, hw=[(200, 400), (161, 200)], scales=5)
    assert _call(L, **{**big, 'ws_bytes': need5 - 1}) == -22
    assert {'lvae_msssim_planes', 'lvae_msssim_planes_workspace_bytes'} <= set(_native.SIGNATURES)
    assert F32 == 0 and (U8, LOW, HIGH) == (1, 2, 3)


# ----------------------------------------------------------------------------------------------- the evaluation harness
def test_yuv_evaluate_validates_metrics_before_it_touches_the_model(tmp_path):
    """The host tests have no CPU stub with the YUV coding API (the key sets are checked on the GPU, tests/test_gpu_ssim_yuv.py); the
    option's own checks come first and need neither a model nor a file."""
    import inspect
    from lvae.evaluation import yuv_evaluate
    assert inspect.signature(yuv_evaluate).parameters['metrics'].default == ('psnr',)
    with pytest.raises(ValueError, match='unknown metrics'):
        yuv_evaluate(None, str(tmp_path / 'none.yuv'), 192, 128, metrics=('psnr', 'vmaf'))
    with pytest.raises(ValueError, match='128x192'):
        yuv_evaluate(None, str(tmp_path / 'none.yuv'), 192, 128, metrics=('ms-ssim',))


def test_codec_script_has_the_eval_yuv_subcommand(capsys):
    """eval-yuv takes the raw file alone (no DST) and the flags of encode-yuv plus --ssim / --ms-ssim; every other command still needs DST."""
    spec = importlib.util.spec_from_file_location('lvae_codec_script', os.path.join(REPO, 'scripts', 'lvae-codec.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args(['eval-yuv', 'IN.yuv', '--size', '192', '128', '--layout', 'p010', '--ssim', '--ms-ssim', '--frames', '2'])
    assert (a.command, a.src, a.dst, a.size, a.layout, a.ssim, a.ms_ssim, a.frames) == ('eval-yuv', 'IN.yuv', None, [192, 128], 'p010', True, True, 2)
    a = cli.build_parser().parse_args(['eval-yuv', 'IN.yuv', '--size', '192', '128'])
    assert not a.ssim and not a.ms_ssim
    for argv in (['encode-yuv', 'IN.yuv', '--size', '192', '128'], ['eval-yuv', 'IN.yuv', 'OUT', '--size', '192', '128'], ['eval-yuv', 'IN.yuv']):
        with pytest.raises(SystemExit):
            cli.main(argv)                                                    # argparse errors: before any model is built
    capsys.readouterr()
