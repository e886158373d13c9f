"""not-gpu: the rate-map entry points at the C boundary (header, library, ctypes table, argument checks), lvae.evaluation.rate_map_evaluate
on a CPU stub codec, and the `ratemap` sub-command of scripts/lvae-codec.py."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('lvae_gaussian_nll_pos_f32', 'lvae_pixel_nll_pos_f32', 'lvae_rate_map_f32')


def _prototypes():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'lvae_hip.h')).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\bint\s+(lvae_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


def _ctype_of(param):
    """The ctypes type _native.SIGNATURES must hold for one parameter of a prototype."""
    param = param.strip()
    if '*' in param:
        return ctypes.c_void_p
    base = param.rsplit(None, 1)[0].replace('const', '').strip()
    return {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double}[base]


def test_rate_map_symbols_declared_exported_and_bound():
    """The three names are in the header, exported by the library and in the ctypes table, argument for argument; the ABI number did not
    move.  They have no launch-plan kind: the table of kinds keeps its 26 rows and LVAE_OP_ORDER its value (tests/test_abi.py pins both)
    -- the callers launch them between the ranges of a plan."""
    from lvae import _native
    protos = _prototypes()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _native.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    for name in NEW_SYMBOLS:
        assert name in protos and name in exported and name in _native.SIGNATURES, name
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int
        assert args == [_ctype_of(p) for p in protos[name].split(',')], name
        assert protos[name].split(',')[-1].strip() == 'void* stream'
        assert name not in _native.OP_KINDS
    assert _native.ABI_VERSION == 27 and _native.lib().lvae_abi_version() == 27
    plan_ops = open(os.path.join(REPO, 'lossy-vae_amd', 'csrc', 'plan_ops.h')).read()
    assert plan_ops.count('LVAE_PLAN_ROW(LVAE_OP_') == len(_native.OP_KINDS) == 26


def test_rate_map_entries_reject_bad_arguments_without_gpu():
    """Every check comes before any HIP call; the addresses below are never read."""
    from lvae import _native
    L = _native.lib()
    fake = 0x1000
    assert L.lvae_gaussian_nll_pos_f32(None, None, None, 0.11, 1, 4, 4, 1, None) == -22
    assert L.lvae_gaussian_nll_pos_f32(fake, fake, fake, 0.11, 1, 4, 4, 2, None) == -22
    assert L.lvae_gaussian_nll_pos_f32(fake, fake, fake, 0.11, 1, 0, 4, 1, None) == -22
    assert L.lvae_pixel_nll_pos_f32(None, None, None, 1, 4, 4, None, None) == -22
    assert L.lvae_pixel_nll_pos_f32(fake, fake, fake, 1, 0, 4, None, None) == -22

    def rate_map(lat, H=64, W=128, n=None, pix=None, B=1, crop=None, row=None, out=fake):
        pos = (ctypes.c_void_p * max(1, len(lat)))(*[fake] * len(lat))
        lh = (ctypes.c_int * max(1, len(lat)))(*[h for h, _ in lat])
        lw = (ctypes.c_int * max(1, len(lat)))(*[w for _, w in lat])
        ch, cw = crop or (H, W)
        return L.lvae_rate_map_f32(pos, lh, lw, len(lat) if n is None else n, pix, B, H, W, out, ch * (row or cw), row or cw, ch, cw, None)

    assert rate_map([(1, 2)], out=None) == -22
    assert rate_map([(64, 128)], H=192, W=384) == -22                # ratio 3: no power of two
    assert rate_map([(1, 4)]) == -22                                 # 64 / 1 != 128 / 4
    assert rate_map([(5, 10)]) == -22                                # 64 % 5
    assert rate_map([(1, 2)], n=33) == -22
    assert rate_map([], n=0) == -22                                  # nothing to add
    assert rate_map([(1, 2)], crop=(65, 128)) == -22
    assert rate_map([(1, 2)], crop=(50, 101), row=100) == -22        # a row stride below the crop
    assert rate_map([(1, 2)], B=0) == -22


class _StubCodec:
    """CPU stand-in with the rate_map contract for lists: two latent blocks at strides 64 and 32 and a map that is their composition."""
    max_stride = 64
    LOG2E = 1.4426950408889634

    def __init__(self):
        self.calls = []

    def rate_map(self, images, blocks=False, **kw):
        assert blocks and len(images) == 1
        self.calls.append(kw)
        h, w = images[0].shape[:2]
        H, W = 64 * -(-h // 64), 64 * -(-w // 64)
        b0 = torch.full((1, H // 64, W // 64), 64.0 * 64.0, dtype=torch.float64)          # 1 nat per pixel
        b1 = torch.arange(1, 1 + (H // 32) * (W // 32), dtype=torch.float64).view(1, H // 32, W // 32) * 32.0 * 32.0
        full = (b0.repeat_interleave(64, 1).repeat_interleave(64, 2) / 4096 + b1.repeat_interleave(32, 1).repeat_interleave(32, 2) / 1024) * self.LOG2E
        return [full[:, :h, :w].float()], [b0, b1]


def _write_images(folder, specs):
    from PIL import Image
    for name, (h, w) in specs.items():
        (folder / name).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(folder / name)


def test_rate_map_evaluate_on_a_stub(tmp_path):
    from PIL import Image
    from lvae.evaluation import rate_map_evaluate
    src, out = tmp_path / 'src', tmp_path / 'out' / 'maps'
    _write_images(src, {'b.png': (50, 101), 'sub/a.png': (64, 64)})
    m = _StubCodec()
    rows = rate_map_evaluate(m, str(src), out_dir=out)
    assert [r['name'] for r in rows] == ['b', 'a']                   # sorted by path: src/b.png < src/sub/a.png
    assert m.calls == [{}, {}]
    assert sorted(p.name for p in out.iterdir()) == ['a.npy', 'a.png', 'b.npy', 'b.png']
    for r, (h, w) in zip(rows, [(50, 101), (64, 64)]):
        arr = np.load(out / f"{r['name']}.npy")
        assert arr.dtype == np.float32 and arr.shape == (h, w)
        assert r['bits'] == float(arr.astype(np.float64).sum())
        assert len(r['shares']) == 2 and sum(r['shares']) == pytest.approx(1.0, abs=1e-12)
        png = np.asarray(Image.open(out / f"{r['name']}.png"))
        assert png.dtype == np.uint8 and png.shape == (h, w) and png.max() == 255
        assert np.array_equal(png, np.round(arr / arr.max() * np.float32(255)).astype(np.uint8))
    # the shares count every position with the pixels it has inside the image: b.png is 50 x 101 of a 64 x 128 canvas
    b0 = 50 * 101 * 1.0
    b1 = sum((k + 1) * ny * nx for k, (ny, nx) in enumerate([(32, 32), (32, 32), (32, 32), (32, 5), (18, 32), (18, 32), (18, 32), (18, 5)]))
    assert rows[0]['shares'][0] == pytest.approx(b0 / (b0 + b1), rel=1e-12)
    assert rows[0]['bits'] == pytest.approx((b0 + b1) * _StubCodec.LOG2E, rel=1e-6)
    # lmb is handed on; no out_dir writes nothing
    rows2 = rate_map_evaluate(m, str(src), lmb=64)
    assert m.calls[2:] == [{'lmb': 64}, {'lmb': 64}] and [r['bits'] for r in rows2] == [r['bits'] for r in rows]


def test_rate_map_evaluate_argument_checks(tmp_path):
    from lvae.evaluation import rate_map_evaluate
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match='no images'):
        rate_map_evaluate(_StubCodec(), str(empty))
    with pytest.raises(ValueError, match='no rate_map'):
        rate_map_evaluate(object(), str(empty))
    twice = tmp_path / 'twice'
    _write_images(twice, {'x/a.png': (64, 64), 'y/a.png': (64, 64)})
    with pytest.raises(ValueError, match='share a stem'):
        rate_map_evaluate(_StubCodec(), str(twice), out_dir=tmp_path / 'o')
    assert len(rate_map_evaluate(_StubCodec(), str(twice))) == 2        # without files to write the stems may repeat


def test_ratemap_subcommand_parses():
    spec = importlib.util.spec_from_file_location('lvae_codec_script', os.path.join(REPO, 'scripts', 'lvae-codec.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args(['ratemap', 'IMAGES', 'OUT', '-m', 'qres34m', '--synthetic', '2'])
    assert (a.command, a.src, a.dst, a.model, a.synthetic, a.lmb) == ('ratemap', 'IMAGES', 'OUT', 'qres34m', 2, None)
    a = cli.build_parser().parse_args(['ratemap', 'IMAGES', 'OUT', '--lmb', '256'])
    assert a.model == 'qarv_base' and a.lmb == 256.0
    assert callable(cli.ratemap)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['ratemaps', 'IMAGES', 'OUT'])
