"""not-gpu: the host side of the 8-bit image path (lvae/utils/image.py) -- PNG round trip, the modes load_u8 refuses, the CPU forms of
to_float01 / to_u8 against the expressions they stand for -- and the argument checks of lvae_image_u8_to_f32 / lvae_image_f32_to_u8,
which come before any HIP call and so run without a GPU."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import seeded_init
from lvae.utils.coding import pad_divisible_by, pil_to_tensor01
from lvae.utils.image import load_u8, save_u8, to_float01, to_u8


def test_png_round_trip(tmp_path):
    a = torch.from_numpy(seeded_init.synthetic_image_u8(50, 70, 1))
    save_u8(a, tmp_path / 'a.png')
    b = load_u8(tmp_path / 'a.png')
    assert b.dtype == torch.uint8 and tuple(b.shape) == (50, 70, 3) and torch.equal(a, b)
    assert torch.equal(load_u8(Image.open(tmp_path / 'a.png')), a)
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'a.png')), a.numpy())


@pytest.mark.parametrize('mode', ['L', 'RGBA'])
def test_load_u8_refuses_other_modes(tmp_path, mode):
    Image.fromarray(seeded_init.synthetic_image_u8(8, 9, 2)).convert(mode).save(tmp_path / 'x.png')
    with pytest.raises(ValueError, match=mode):
        load_u8(tmp_path / 'x.png')


@pytest.mark.parametrize('h,w', [(50, 70), (64, 100), (64, 64)])
def test_to_float01_cpu_is_the_host_expression(h, w):
    u8 = seeded_init.synthetic_image_u8(h, w, 3)
    ref = pil_to_tensor01(pad_divisible_by(Image.fromarray(u8), 64))
    for im in (torch.from_numpy(u8), u8, Image.fromarray(u8)):
        x, sizes = to_float01([im], div=64)
        assert sizes == [(h, w)] and x.dtype == torch.float32 and torch.equal(x[0], ref)
    x, _ = to_float01([u8], div=1)
    assert torch.equal(x[0], pil_to_tensor01(Image.fromarray(u8)))


def test_to_float01_cpu_batch_of_different_sizes_on_one_canvas():
    a, b = seeded_init.synthetic_image_u8(50, 70, 4), seeded_init.synthetic_image_u8(64, 100, 5)
    x, sizes = to_float01([a, b], div=64)
    assert tuple(x.shape) == (2, 3, 64, 128) and sizes == [(50, 70), (64, 100)]
    for i, u8 in enumerate((a, b)):
        assert torch.equal(x[i], pil_to_tensor01(pad_divisible_by(Image.fromarray(u8), 64)))


def test_to_u8_cpu_is_the_torch_expression():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 9, 11, generator=g) * 1.2 - 0.1
    x[0, 0, 0, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255])      # near-ties
    ref = torch.round(x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)
    out = to_u8(x)
    assert all(o.dtype == torch.uint8 and torch.equal(o, r) for o, r in zip(out, ref))
    out = to_u8([x[0], x[1:2]], sizes=[(5, 7), (9, 3)])
    assert torch.equal(out[0], ref[0, :5, :7]) and torch.equal(out[1], ref[1, :9, :3])
    v = torch.arange(256, dtype=torch.float32).div(255).view(1, 1, 1, 256).expand(1, 3, 1, 256)
    assert torch.equal(to_u8(v)[0][0, :, 0], torch.arange(256, dtype=torch.uint8))       # v / 255 gives v back


def _u8_to_f32(L, src=1 << 20, rows=(64 * 3,), hw=((8, 8),), B=1, dst=1 << 21, dst_img=3 * 64 * 64, H=64, W=64, null=()):
    n = max(B, 1)
    sp = None if 'src' in null else (ctypes.c_void_p * n)(*([src] * n))
    rp = None if 'rows' in null else (ctypes.c_long * n)(*(list(rows) * n)[:n])
    hp = None if 'hw' in null else (ctypes.c_int * (2 * n))(*[v for p in (list(hw) * n)[:n] for v in p])
    return L.lvae_image_u8_to_f32(sp, rp, hp, B, None if 'dst' in null else dst, dst_img, H, W, None)


def _f32_to_u8(L, src=1 << 20, strides=(3 * 64 * 64, 64 * 64, 64), H=64, W=64, hw=((8, 8),), B=1, dst=1 << 21, rows=(24,), null=()):
    n = max(B, 1)
    dp = None if 'dst' in null else (ctypes.c_void_p * n)(*([dst] * n))
    rp = None if 'rows' in null else (ctypes.c_long * n)(*(list(rows) * n)[:n])
    hp = None if 'hw' in null else (ctypes.c_int * (2 * n))(*[v for p in (list(hw) * n)[:n] for v in p])
    return L.lvae_image_f32_to_u8(None if 'src' in null else src, *strides, H, W, hp, B, dp, rp, None)


def test_kernels_reject_bad_arguments_without_gpu():
    """Every case returns -22 from the host-side checks: no pointer here is real, so reaching a launch would not go unnoticed."""
    from lvae import _native
    L = _native.lib()
    for call in (_u8_to_f32, _f32_to_u8):
        for null in ('src', 'rows', 'hw', 'dst'):
            assert call(L, null=(null,)) == -22, (call.__name__, null)
        assert call(L, B=0) == -22 and call(L, B=-1) == -22
        assert call(L, hw=((0, 8),)) == -22 and call(L, hw=((8, 0),)) == -22                 # an empty extent
        assert call(L, hw=((65, 8),)) == -22 and call(L, hw=((8, 65),)) == -22               # beyond the canvas
        assert call(L, hw=((8, 8), (8, 65)), B=2) == -22                                      # ... in a later image of the batch
        assert call(L, rows=(23,)) == -22                                                     # rows shorter than 3 * w bytes
    assert _u8_to_f32(L, src=0) == -22                                                        # a null entry of the pointer array
    assert _f32_to_u8(L, dst=0) == -22
    assert _u8_to_f32(L, B=2, hw=((8, 8), (8, 8)), dst_img=3 * 64 * 64 - 1) == -22            # images that overlap
    assert _f32_to_u8(L, strides=(3 * 64 * 64, 64 * 64, 63)) == -22                           # strides that do not hold the canvas
    assert _f32_to_u8(L, strides=(3 * 64 * 64, 64 * 63, 64)) == -22


def test_abi_declares_the_two_entries():
    from lvae import _native
    assert {'lvae_image_u8_to_f32', 'lvae_image_f32_to_u8'} <= set(_native.SIGNATURES)
