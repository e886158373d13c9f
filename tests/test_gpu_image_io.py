"""-m gpu: 8-bit images end to end.  The two kernels of csrc/image_io.hip against the CPU expressions they stand for (torch.equal: every
bit), then the model-level u8 API of all four models against the float path it replaces: compress_images gives the bytes compress_file
writes -- and, spelled out here, the bytes the float-tensor API gives for the host-padded image -- decompress_images the rounded
decompress_file, the evaluation the floats of per-image host computations, and scripts/lvae-codec.py the same PNGs."""
import ctypes
import functools
import io
import os
import pickle
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import seeded_init
from lvae.utils.coding import pad_divisible_by, pil_to_tensor01
from lvae.utils.image import U8Batch, load_u8, save_u8, to_float01, to_u8

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
MODELS = ['qarv_base', 'qres34m', 'qres17m', 'qres34m_lossless']


# ----------------------------------------------------------------------------------------------- test 1: u8 -> f32
def _edge_ref(u8, H, W):
    """np.pad(mode='edge') to the canvas, then the host conversion: the definition of lvae_image_u8_to_f32."""
    h, w = u8.shape[:2]
    return pil_to_tensor01(Image.fromarray(np.ascontiguousarray(np.pad(u8, ((0, H - h), (0, W - w), (0, 0)), mode='edge'))))


def _all_values_image():
    v = np.arange(512, dtype=np.int64).reshape(2, 256)
    return np.stack([v % 256, (v + 85) % 256, (255 - v) % 256], -1).astype(np.uint8)


def test_u8_to_f32_all_256_values():
    u8 = _all_values_image()
    x, sizes = to_float01([torch.from_numpy(u8)], div=64, device=DEV)
    assert sizes == [(2, 256)] and tuple(x.shape) == (1, 3, 64, 256)
    ref = pil_to_tensor01(pad_divisible_by(Image.fromarray(u8), 64))
    assert torch.equal(x[0].cpu(), ref)
    assert torch.equal(x[0, 0, 0].cpu(), torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255))


@pytest.mark.parametrize('extent,div,canvas', [((1, 1), 4, (4, 4)), ((5, 7), 8, (8, 8)), ((3, 67), 64, (64, 128)), ((64, 64), 64, (64, 64)),
                                               ((5, 7), 1, (5, 7)), ((9, 130), 1, (9, 130))])
def test_u8_to_f32_extent_to_canvas(extent, div, canvas):
    """The issue's extent -> canvas pairs, and two canvases whose width is no multiple of 4 (scalar stores, a partial last quad)."""
    u8 = seeded_init.synthetic_image_u8(*extent, 11)
    x, _ = to_float01([torch.from_numpy(u8)], div=div, device=DEV)
    assert tuple(x.shape) == (1, 3) + canvas
    assert torch.equal(x[0].cpu(), _edge_ref(u8, *canvas))
    if div == 64:
        assert torch.equal(x[0].cpu(), pil_to_tensor01(pad_divisible_by(Image.fromarray(u8), 64)))


def test_u8_to_f32_batch_of_three_extents():
    ims = [seeded_init.synthetic_image_u8(h, w, 20 + i) for i, (h, w) in enumerate([(50, 70), (64, 100), (3, 67)])]
    x, sizes = to_float01([torch.from_numpy(a).to(DEV) for a in ims], div=64)
    assert sizes == [(50, 70), (64, 100), (3, 67)] and tuple(x.shape) == (3, 3, 64, 128) and x.device.type == 'cuda'
    for i, a in enumerate(ims):
        assert torch.equal(x[i].cpu(), pil_to_tensor01(pad_divisible_by(Image.fromarray(a), 64))), i


@pytest.mark.parametrize('w', [67, 64])
def test_u8_to_f32_strided_misaligned_source(w):
    """A view: rows 3 * w + 5 bytes apart, the base 1 byte past an aligned address (w = 64: rows of 192 bytes that still start off a
    dword boundary in three rows out of four)."""
    h, row = 6, 3 * w + 5
    u8 = seeded_init.synthetic_image_u8(h, w, 31)
    buf = torch.zeros(1 + h * row, dtype=torch.uint8, device=DEV)
    view = buf[1:].as_strided((h, w, 3), (row, 3, 1))
    view.copy_(torch.from_numpy(u8))
    assert view.data_ptr() % 4 == 1
    b = U8Batch([view], 64, DEV)
    assert b.images[0].data_ptr() == view.data_ptr()                       # read where it lies
    out = torch.empty(b.shape, dtype=torch.float32, device=DEV)
    b.fill(out)
    assert torch.equal(out[0].cpu(), _edge_ref(u8, 64, 128 if w == 67 else 64))


@pytest.mark.parametrize('gap', [40, 41])
def test_u8_to_f32_writes_only_its_planes(gap):
    """A destination whose image stride exceeds 3 * H * W (gap 41: also off the 16-byte grid, the scalar-store path): the planes are
    right and every element between them still holds the sentinel."""
    ims = [seeded_init.synthetic_image_u8(h, w, 40 + i) for i, (h, w) in enumerate([(5, 7), (8, 8)])]
    H = W = 8
    big = torch.full((2, 3 * H * W + gap), -7.0, dtype=torch.float32, device=DEV)
    dst = big[:, :3 * H * W].view(2, 3, H, W)
    U8Batch([torch.from_numpy(a) for a in ims], 8, DEV).fill(dst)
    got = big.cpu()
    for i, a in enumerate(ims):
        assert torch.equal(got[i, :3 * H * W].view(3, H, W), _edge_ref(a, H, W)), i
    assert bool((got[:, 3 * H * W:] == -7.0).all())


# ----------------------------------------------------------------------------------------------- test 2: f32 -> u8
def _f32_values():
    k = torch.arange(255, dtype=torch.float32)
    ties = (k + 0.5) / 255
    g = torch.Generator().manual_seed(5)
    return torch.cat([torch.arange(256, dtype=torch.float32) / 255, ties, torch.nextafter(ties, torch.tensor(2.0)),
                      torch.nextafter(ties, torch.tensor(-1.0)), torch.tensor([-0.0, -1e-3, 1 + 1e-3, 2.0]),
                      torch.rand(4096, generator=g)])


def _u8_ref(x):
    """(3, h, w) fp32 on the CPU -> (h, w, 3) uint8: the definition of lvae_image_f32_to_u8 for inputs without a NaN."""
    return torch.round(x.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.fixture(scope='module')
def f32_batch():
    """(3, 3, 64, 128) fp32: the test values fill the (63, 127) crop of every plane (rotated per plane), the rest is uniform noise."""
    vals = _f32_values()
    assert torch.equal(torch.round(vals[:256] * 255).to(torch.uint8), torch.arange(256, dtype=torch.uint8))      # v / 255 gives v back
    g = torch.Generator().manual_seed(6)
    x = torch.rand(3, 3, 64, 128, generator=g)
    n = 63 * 127
    fill = torch.cat([vals, torch.rand(n - vals.numel(), generator=g)])
    for b in range(3):
        for c in range(3):
            x[b, c, :63, :127] = torch.roll(fill, 1000 * (3 * b + c)).view(63, 127)
    return x, x.to(DEV)


def test_f32_to_u8_cropped_views_of_one_batch(f32_batch):
    x, xd = f32_batch
    sizes = [(63, 127), (5, 7), (3, 67)]
    out = to_u8([xd[i:i + 1, :, :h, :w] for i, (h, w) in enumerate(sizes)])
    for i, (h, w) in enumerate(sizes):
        assert out[i].dtype == torch.uint8 and out[i].is_cuda and torch.equal(out[i].cpu(), _u8_ref(x[i, :, :h, :w])), i
    out = to_u8(xd, sizes)                                                  # the same through `sizes`
    for i, (h, w) in enumerate(sizes):
        assert torch.equal(out[i].cpu(), _u8_ref(x[i, :, :h, :w])), i


def test_f32_to_u8_whole_and_offset_views(f32_batch):
    x, xd = f32_batch
    for o, r in zip(to_u8(xd), x):                                          # whole planes: the 16-byte loads
        assert torch.equal(o.cpu(), _u8_ref(r))
    out = to_u8([xd[i, :, 1:, 1:] for i in range(3)])                       # views that start off the 16-byte grid: scalar loads
    for o, r in zip(out, x):
        assert torch.equal(o.cpu(), _u8_ref(r[:, 1:, 1:]))


def test_f32_to_u8_strided_misaligned_output(f32_batch):
    """The C entry itself: outputs with rows 3 * w + 5 bytes apart starting 1 byte past an aligned address; only the pixels are written."""
    from lvae import _native
    x, xd = f32_batch
    sizes = [(63, 127), (5, 8), (3, 67)]
    bufs, views = [], []
    for h, w in sizes:
        buf = torch.full((1 + h * (3 * w + 5),), 7, dtype=torch.uint8, device=DEV)
        bufs.append(buf)
        views.append(buf[1:].as_strided((h, w, 3), (3 * w + 5, 3, 1)))
    dst = (ctypes.c_void_p * 3)(*[v.data_ptr() for v in views])
    rows = (ctypes.c_long * 3)(*[3 * w + 5 for _, w in sizes])
    hw = (ctypes.c_int * 6)(*[v for s in sizes for v in s])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _native.lib().lvae_image_f32_to_u8(xd.data_ptr(), 3 * 64 * 128, 64 * 128, 128, 64, 128, hw, 3, dst, rows, st)
    assert rc == 0
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(sizes):
        assert torch.equal(views[i].cpu(), _u8_ref(x[i, :, :h, :w])), i
        mask = torch.ones(bufs[i].numel(), dtype=torch.bool)
        mask[1:].as_strided((h, w, 3), (3 * w + 5, 3, 1)).fill_(False)
        assert bool((bufs[i].cpu()[mask] == 7).all()), i


def test_f32_to_u8_nan_gives_zero():
    g = torch.Generator().manual_seed(8)
    x = torch.rand(1, 3, 6, 9, generator=g)
    ref = _u8_ref(x[0])
    nan = [(0, 0, 0), (1, 2, 3), (2, 5, 8), (1, 5, 4)]
    for c, r, q in nan:
        x[0, c, r, q] = float('nan')
        ref[r, q, c] = 0
    x[0, 0, 1, 1] = float('inf'); ref[1, 1, 0] = 255
    x[0, 0, 1, 2] = float('-inf'); ref[1, 2, 0] = 0
    assert torch.equal(to_u8(x.to(DEV))[0].cpu(), ref)


# ----------------------------------------------------------------------------------------------- the models
@functools.lru_cache(maxsize=None)
def _model(name):
    """Seeded weights as scripts/lvae-codec.py --synthetic loads them."""
    import lvae
    m = lvae.get_model(name, pretrained=False)
    sd = m.state_dict()
    for k in list(sd):
        a = seeded_init.seeded_tensor(k, tuple(sd[k].shape), 0, profile='typical')
        if a is not None and 'discrete_gaussian' not in k:
            sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m.compress_mode()
    return m.to(DEV).eval()


SIZES = [(50, 70), (64, 100)]                       # both pad to 64 x 128


@pytest.fixture(scope='module', params=MODELS)
def coded(request, tmp_path_factory):
    """Per model, computed once: the two images as PNGs, the files compress_file writes for them, and compress_images' bytes."""
    name = request.param
    m = _model(name)
    d = tmp_path_factory.mktemp(name)
    u8 = [torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 60 + i)) for i, (h, w) in enumerate(SIZES)]
    pngs, bits = [d / f'im{i}.png' for i in range(2)], [d / f'im{i}.bits' for i in range(2)]
    for t, p, b in zip(u8, pngs, bits):
        save_u8(t, p)
        m.compress_file(p, b)
    return dict(name=name, model=m, dir=d, u8=u8, pngs=pngs, bits=bits, files=[b.read_bytes() for b in bits], blobs=m.compress_images(u8))


def _float_path_bytes(m, name, u8):
    """The parent's construction of a compress_file, spelled out: host padding, host division, the float-tensor API, the container."""
    img = Image.fromarray(u8.numpy())
    im = pil_to_tensor01(pad_divisible_by(img, 64)).unsqueeze(0).to(DEV)
    if name == 'qarv_base':
        return struct.pack('2H', img.height, img.width) + m.compress(im)
    obj = m.compress(im)
    obj.append((img.height, img.width))
    buf = io.BytesIO()
    pickle.dump(obj, file=buf)
    return buf.getvalue()


def test_streams_are_the_files_compress_file_writes(coded):
    m, name = coded['model'], coded['name']
    for i in range(2):
        assert isinstance(coded['blobs'][i], bytes) and coded['blobs'][i] == coded['files'][i], i
        assert coded['blobs'][i] == _float_path_bytes(m, name, coded['u8'][i]), i
    assert m.compress_images(coded['u8'][1:])[0] == coded['files'][1]              # alone as in a batch
    if name == 'qarv_base':
        with pytest.raises(AssertionError):
            m.compress_images([coded['u8'][0], torch.zeros(64, 64, 3, dtype=torch.uint8)])      # padded sizes differ
    else:
        with pytest.raises(ValueError):
            m.compress_images(coded['u8'], lmb=64)


def test_streams_with_per_image_lambdas():
    m = _model('qarv_base')
    u8 = [torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 60 + i)) for i, (h, w) in enumerate(SIZES)]
    blobs = m.compress_images(u8, lmb=[16, 2048])
    for i, lmb in enumerate([16, 2048]):
        img = Image.fromarray(u8[i].numpy())
        im = pil_to_tensor01(pad_divisible_by(img, 64)).unsqueeze(0).to(DEV)
        assert blobs[i] == struct.pack('2H', img.height, img.width) + m.compress(im, lmb=lmb), i
        assert struct.unpack('f', blobs[i][4:8])[0] == lmb
    assert blobs[0] != blobs[1][:len(blobs[0])]


def test_streams_do_not_depend_on_the_input_kind(coded):
    m, u8 = coded['model'], coded['u8']
    kinds = {'device': [t.to(DEV) for t in u8], 'numpy': [t.numpy() for t in u8], 'pil': [Image.open(p) for p in coded['pngs']],
             'pinned': [load_u8(p) for p in coded['pngs']], 'path': list(coded['pngs'])}
    for kind, ims in kinds.items():
        assert m.compress_images(ims) == coded['blobs'], kind


# ----------------------------------------------------------------------------------------------- test 4: reconstructions
def test_decompress_images_is_the_rounded_decompress_file(coded):
    m = coded['model']
    rec = m.decompress_images(coded['blobs'])
    for i, (h, w) in enumerate(SIZES):
        ref = torch.round(m.decompress_file(coded['bits'][i])[0] * 255).to(torch.uint8).permute(1, 2, 0)
        assert rec[i].is_cuda and rec[i].dtype == torch.uint8 and tuple(rec[i].shape) == (h, w, 3)
        assert torch.equal(rec[i], ref), i
    outs = [coded['dir'] / f'rec{i}.png' for i in range(2)]
    m.decompress_to_files(coded['bits'], outs)
    for i in range(2):
        assert torch.equal(load_u8(outs[i]), rec[i].cpu()), i
    if coded['name'] == 'qres34m_lossless':
        assert torch.equal(m.decompress_images(m.compress_images([coded['u8'][0]]))[0].cpu(), coded['u8'][0])
        assert torch.equal(rec[1].cpu(), coded['u8'][1])


def test_decompress_images_batches_by_latent_shape():
    """Blobs of two latent shapes in one call come back in the order they went in."""
    m = _model('qres17m')
    u8 = [torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 80 + i)) for i, (h, w) in enumerate([(50, 70), (64, 64), (64, 100)])]
    blobs = m.compress_images([u8[0], u8[2]])
    blobs = [blobs[0], m.compress_images([u8[1]])[0], blobs[1]]
    rec = m.decompress_images(blobs)
    assert [tuple(r.shape) for r in rec] == [(50, 70, 3), (64, 64, 3), (64, 100, 3)]
    for r, b in zip(rec, blobs):
        assert torch.equal(r, m.decompress_images([b])[0])


# ----------------------------------------------------------------------------------------------- test 5: evaluation
@pytest.mark.parametrize('name', ['qarv_base', 'qres34m', 'qres17m'])        # (qres34m_lossless: mse = 0, the harness has no PSNR for it)
def test_evaluation_keeps_its_floats(name, tmp_path):
    """The evaluation codes from device u8 tensors and takes its `real` from to_float01 on the device.  Its floats == the ones of the
    float path spelled out here: host padding and division, the float-tensor compress(), the container, decompress_file, the CPU
    pil_to_tensor01 as `real`, _mse."""
    import math
    from lvae.evaluation import _eval_batch, _eval_one, _mse, imcoding_evaluate
    m = _model(name)
    folder = tmp_path / 'set'
    folder.mkdir()
    for i, (h, w) in enumerate(SIZES + [(64, 64)]):
        save_u8(torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 60 + i)), folder / f'im{i}.png')
    paths = sorted(folder.iterdir())
    rows = []
    for p in paths:
        blob = _float_path_bytes(m, name, torch.from_numpy(np.array(Image.open(p))))
        (tmp_path / 'x.bits').write_bytes(blob)
        fake = m.decompress_file(tmp_path / 'x.bits')
        real = pil_to_tensor01(Image.open(p))
        mse = _mse(real, fake)
        rows.append({'bpp': float(len(blob) * 8 / float(real.shape[1] * real.shape[2])), 'mse': float(mse), 'psnr': float(-10 * math.log10(mse))})
    want = {k: sum(r[k] for r in rows) / 3 for k in ('bpp', 'mse', 'psnr')}
    assert imcoding_evaluate(m, str(folder)) == want
    one = [_eval_one(m, p, tmp_path, ms=False) for p in paths]
    assert one == rows
    assert _eval_batch(m, paths[:2], tmp_path) + _eval_batch(m, paths[2:], tmp_path) == one
    pil = [Image.open(p) for p in paths[:2]]
    assert _eval_batch(m, paths[:2], tmp_path, images=pil) == one[:2]                    # as the sharded evaluation calls it


# ----------------------------------------------------------------------------------------------- test 6: the script
def test_codec_script_round_trip(tmp_path):
    script = os.path.join(REPO, 'scripts', 'lvae-codec.py')
    src, bits, rec = tmp_path / 'src', tmp_path / 'bits', tmp_path / 'rec'
    for cmd in (['encode', str(src), str(bits)], ['decode', str(bits), str(rec)]):
        r = subprocess.run([sys.executable, script] + cmd + ['-m', 'qarv_base', '--lmb', '256', '--synthetic', '3', '--batch', '2'],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(bits.glob('*.bits'))
    assert [f.stem for f in files] == ['im00', 'im01', 'im02'] == sorted(p.stem for p in rec.glob('*.png'))
    m = _model('qarv_base')
    for f in files:
        assert struct.unpack('f', f.read_bytes()[4:8])[0] == 256.0
        assert torch.equal(load_u8(rec / (f.stem + '.png')), m.decompress_images([f.read_bytes()])[0].cpu()), f.name
        assert f.read_bytes() == m.compress_images([src / (f.stem + '.png')], lmb=256)[0]
