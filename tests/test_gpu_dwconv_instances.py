"""-m gpu: every depthwise + LayerNorm kernel instance a launch can reach (tests/dwconv_cases.py; the closure is asserted without a GPU
by tests/test_dwconv_choice_host.py) against an fp64 evaluation of the operator -- F.conv2d(groups=C) + F.layer_norm in double -- at
ragged shapes: tiles of 4 and 8 rows whose last tile is cut (at TH = 8 shorter than the halo), several tiles per workgroup with a
short last workgroup, strips cut by the right edge, two or three distinct images, the per-image (_v) entry points, every output format.

Bound, fp32 output against fp64: |err| <= 3e-5 max(1, |ref|), the bound of test_gpu_kernels.py::test_dwconv_ln (torch's own fp32
evaluation of these shapes is within 3.1e-6 absolute / 2.1e-6 relative of fp64).  The other formats are checked by their exact
relation to the fp32 kernel's result at the same shape, which the same case compares with fp64.  Every output sits inside a larger
buffer with one image row of sentinel bytes on either side and is prefilled with 0xFF bytes (NaN in fp32 / fp16 / bf16 / e4m3, and no
E8M0 scale the kernel writes): the sentinels must survive and the prefill must not -- ragged tiles rely on descriptor clipping."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import dwconv_cases as dc

pytestmark = pytest.mark.gpu

TOL = 3e-5
SENTINEL, PREFILL = 0xA5, 0xFF


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _native.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out_bytes(fmt, B, H, W, C):
    M = B * H * W
    return {'f32': M * C * 4, 'h2': M * C * 4, 'bf16': M * C * 2, 'q8': M * C + (C // 64) * M * 2}[fmt]


class Guarded:
    """An output buffer of `fmt` inside a larger allocation: one image row of sentinel bytes before and after (Q8: before the byte
    plane and after the scale plane, which the format lays out back to back), the output itself prefilled."""

    def __init__(self, fmt, B, H, W, C):
        self.fmt, self.n = fmt, _out_bytes(fmt, B, H, W, C)
        self.guard = W * C * {'f32': 4, 'h2': 4, 'bf16': 2, 'q8': 1}[fmt]
        self.buf = torch.full((self.guard + self.n + self.guard,), SENTINEL, dtype=torch.uint8, device='cuda')
        self.body = self.buf[self.guard:self.guard + self.n]
        self.body.fill_(PREFILL)
        assert self.body.data_ptr() % 16 == 0

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        """After the launch: both guards untouched, no prefill left in the output."""
        assert bool((self.buf[:self.guard] == SENTINEL).all()), f'{what}: wrote in front of its output'
        assert bool((self.buf[self.guard + self.n:] == SENTINEL).all()), f'{what}: wrote behind its output'
        if self.fmt == 'q8':
            left = int((self.body == PREFILL).sum())          # no e4m3 byte (saturating conversion) and no scale (clamped to 1 .. 254) is 0xFF
        else:
            dt = {'f32': torch.float32, 'h2': torch.float16, 'bf16': torch.bfloat16}[self.fmt]
            left = int(torch.isnan(self.body.view(dt)).sum())
        assert left == 0, f'{what}: {left} output elements never written'


def _ref64(x, wt, bias, k, affines):
    """The operator in fp64.  x: [B][H][W][C]; wt: [k * k][C] (tap-major); affines: (weight, bias) pairs applied in order after the
    normalisation, each [C] or [B][C] (per-image vectors)."""
    B, H, W, C = x.shape
    w = wt.double().t().reshape(C, 1, k, k)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w, bias.double(), padding=(k - 1) // 2, groups=C).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (C,), eps=1e-6)
    for aw, ab in affines:
        aw, ab = aw.double(), ab.double()
        if aw.dim() == 2:
            aw, ab = aw.view(B, 1, 1, C), ab.view(B, 1, 1, C)
        y = y * aw + ab
    return y


def _worst(out, ref):
    """max |err| / max(1, |ref|)"""
    return float(((out.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


class Params:
    """Weights, bias and the affine vectors of one case.  affine: 'adaln' (shift, 1 + scale), 'ln' (LayerNorm weight / bias), 'none',
    'both'; per_image: a [B][stride] table, stride = 2 C + 64 > 2 C, row b holding image b's shift at 0 and 1 + scale at C."""

    def __init__(self, g, B, C, k, affine, per_image):
        self.C, self.k, self.affine, self.per_image = C, k, affine, per_image
        self.wt = (torch.randn(k * k, C, generator=g) / k).cuda()
        self.bias = torch.randn(C, generator=g).cuda()
        self.stride = 2 * C + 64
        tab = torch.randn(B if per_image else 1, self.stride, generator=g)
        tab[:, C:2 * C] = 1 + 0.3 * tab[:, C:2 * C]
        self.tab = tab.cuda()
        self.ln_b, self.ln_w = torch.randn(C, generator=g).cuda(), (1 + 0.3 * torch.randn(C, generator=g)).cuda()
        assert not per_image or affine == 'adaln'

    def ada(self):
        return (self.tab[:, self.C:2 * self.C], self.tab[:, :self.C]) if self.per_image else (self.tab[0, self.C:2 * self.C], self.tab[0, :self.C])

    def affines(self):
        return {'adaln': [self.ada()], 'ln': [(self.ln_w, self.ln_b)], 'none': [], 'both': [(self.ln_w, self.ln_b), self.ada()]}[self.affine]

    def launch(self, L, fmt, x, y_ptr):
        (B, H, W, _), C = x.shape, self.C
        es = self.tab.element_size()
        shift, sc1p = self.tab.data_ptr(), self.tab.data_ptr() + C * es
        if self.per_image:
            return getattr(L, f'lvae_dwconv_ln_{fmt}_v')(x.data_ptr(), self.wt.data_ptr(), self.bias.data_ptr(), shift, sc1p, y_ptr,
                                                         B, H, W, C, self.k, self.stride, _st())
        ln = (self.ln_w.data_ptr(), self.ln_b.data_ptr()) if self.affine in ('ln', 'both') else (None, None)
        ada = (shift, sc1p) if self.affine in ('adaln', 'both') else (None, None)
        return getattr(L, f'lvae_dwconv_ln_{fmt}')(x.data_ptr(), self.wt.data_ptr(), self.bias.data_ptr(), *ln, *ada, y_ptr,
                                                   B, H, W, C, self.k, _st())


def _run(L, prm, fmt, x, what):
    """One guarded launch; returns the output bytes (a view into the guarded buffer)."""
    B, H, W, C = x.shape
    out = Guarded(fmt, B, H, W, C)
    rc = prm.launch(L, fmt, x, out.ptr())
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    out.check(what)
    return out.body


def _check_relation(fmt, got, y32, M, C, what):
    """The exact relation of a reduced format's bytes to the fp32 kernel's result y32 ([M][C]) for the same input."""
    if fmt == 'h2':                                              # test_gpu_f16x2.py::test_dwconv_ln_h2_is_the_split_of_the_fp32_result
        from lvae.models.base import split_f16x2, unpack_f16x2_k32
        hi, lo = unpack_f16x2_k32(got, M, C)
        want = split_f16x2(y32)
        assert torch.equal(hi, want[0]) and torch.equal(lo, want[1]), what
    elif fmt == 'bf16':                                          # test_gpu_fp8.py::test_dwconv_ln_bf16
        assert torch.equal(got.view(torch.bfloat16).view(M, C), y32.to(torch.bfloat16)), what
    else:                                                        # test_gpu_fp8.py::test_dwconv_ln_q8_quantises_the_fp32_result, both bounds
        from lvae.models.base import pack_mxfp8_q8, unpack_mxfp8_q8
        y = y32.cpu()
        q = unpack_mxfp8_q8(got.cpu(), M, C)
        want = unpack_mxfp8_q8(pack_mxfp8_q8(y), M, C)
        frac = float((q != want).float().mean())
        print(f'{what}: {frac:.2e} of the bytes differ from the host quantiser')
        assert frac <= 1e-3, (what, frac)
        blockmax = y.view(M, C // 32, 32).abs().amax(2, keepdim=True).expand(M, C // 32, 32).reshape(M, C)
        assert bool(((q - y).abs() <= blockmax * 2.0 ** -3 + 1e-30).all()), what


# ------------------------------------------------------------------------------------------------ channel-per-lane kernel
# f32 / h2 (and bf16 / q8) cases of one shape share the input, the fp64 reference and the fp32 kernel's result: the cases are ordered
# shape by shape and the last shape's base is kept.
_CL_ORDER = sorted(range(len(dc.CL_CASES)), key=lambda i: (dc.CL_CASES[i][0] in dc.LOWP, dc.CL_CASES[i][1:8], dc.FMTS.index(dc.CL_CASES[i][0])))
_base_cache = {}


def _cl_base(L, lowp, C, k, B, H, W, affine, per_image):
    """Input (bf16-valued for the bf16-map formats), parameters, and the fp32 kernel's guarded result with its error against fp64."""
    key = (lowp, C, k, B, H, W, affine, per_image)
    if key not in _base_cache:
        _base_cache.clear()
        g = torch.Generator().manual_seed(C * 1000 + k * 100 + H + 7 * W + B)
        x = torch.randn(B, H, W, C, generator=g)
        xin = x.to(torch.bfloat16).cuda() if lowp else x.cuda()
        xf = xin.float().contiguous()
        assert B < 2 or not torch.equal(xf[0], xf[1])
        prm = Params(g, B, C, k, affine, per_image)
        ref = _ref64(xf, prm.wt, prm.bias, k, prm.affines())
        y32 = _run(L, prm, 'f32', xf, f'f32 {key}').view(torch.float32).view(B * H * W, C)
        err = _worst(y32.view(B, H, W, C), ref)
        del ref
        _base_cache[key] = (xin, prm, y32, err)
    return _base_cache[key]


def _cl_id(i):
    fmt, C, k, th, tpw, B, H, W, affine, per_image = dc.CL_CASES[i]
    return f'{fmt}-C{C}-k{k}-TH{th}-tpw{tpw}-{B}x{H}x{W}-{affine}' + ('-v' if per_image else '')


@pytest.mark.parametrize('i', _CL_ORDER, ids=_cl_id)
def test_channel_per_lane_instance(L, i):
    fmt, C, k, th, tpw, B, H, W, affine, per_image = dc.CL_CASES[i]
    naff = 0 if affine == 'none' else 1
    assert dc.choice(L, fmt, naff, per_image, B, H, W, C, k) == (0, 0, th, tpw)            # the instance this case is listed for
    assert dc.choice(L, 'f32', naff, per_image, B, H, W, C, k)[:2] == (0, 0)
    xin, prm, y32, err = _cl_base(L, fmt in dc.LOWP, C, k, B, H, W, affine, per_image)
    print(f'{_cl_id(i)}: fp32 kernel against fp64: worst |err| / max(1, |ref|) = {err:.3e}')
    assert err <= TOL, err
    if fmt != 'f32':
        got = _run(L, prm, fmt, xin, _cl_id(i))
        _check_relation(fmt, got, y32, B * H * W, C, _cl_id(i))


def _image_bytes(fmt, buf, b, B, H, W, C):
    """The bytes of image b inside the output of a launch over B images (Q8: the data rows, then each 64-channel block's scales)."""
    hw, M = H * W, B * H * W
    if fmt != 'q8':
        n = _out_bytes(fmt, 1, H, W, C)
        return buf[b * n:(b + 1) * n]
    parts = [buf[b * hw * C:(b + 1) * hw * C]]
    for w in range(C // 64):
        o = M * C + (w * M + b * hw) * 2
        parts.append(buf[o:o + hw * 2])
    return torch.cat(parts)


@pytest.mark.parametrize('fmt', dc.FMTS)
@pytest.mark.parametrize('C,k', [(C, k) for C in dc.CL_WIDTHS for k in dc.KS if k > 1])
def test_same_bits_across_tile_heights(L, C, k, fmt):
    """One ragged map at batch sizes for which the launcher runs the 1-, 4- and 8-row tiles (where the 8-row instance is reachable):
    the batch cycles through three distinct images, and an image has the same bytes in every launch."""
    lowp = fmt in dc.LOWP
    H, W, batches = dc.CL_ACROSS_TH[(lowp, C, k)]
    ths = [dc.choice(L, fmt, 1, 0, B, H, W, C, k)[2] for B in batches]
    assert ths == [1, 4, 8][:len(batches)], ths
    g = torch.Generator().manual_seed(C + k + H + W)
    x3 = torch.randn(3, H, W, C, generator=g)
    x3 = x3.to(torch.bfloat16).cuda() if lowp else x3.cuda()
    prm = Params(g, 1, C, k, 'adaln', False)
    want = [_image_bytes(fmt, _run(L, prm, fmt, x3[j:j + 1].contiguous(), f'{fmt} single {j}'), 0, 1, H, W, C).clone() for j in range(3)]
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    for B in batches[1:]:
        x = x3.repeat((B + 2) // 3, 1, 1, 1)[:B].contiguous()
        out = _run(L, prm, fmt, x, f'{fmt} B={B}')
        for b in range(B):
            assert torch.equal(_image_bytes(fmt, out, b, B, H, W, C), want[b % 3]), (fmt, C, k, B, b)


# ------------------------------------------------------------------------------------------------ sliding-window kernel
_SW_LPP = {128: 16, 144: 4, 192: 16, 256: 32, 288: 8, 384: 32, 512: 32}     # lanes per pixel group (pointwise.hip::dispatch_dwln_c)


def _sw_geometry(C, B, H, W):
    """(pixel groups, groups per wave, blocks) of a one-row-per-group launch: 4 pixels per group, 4 waves per block."""
    groups, gpw = B * H * ((W + 3) // 4), 64 // _SW_LPP[C]
    waves = (groups + gpw - 1) // gpw
    return groups, gpw, (waves + 3) // 4


@pytest.mark.parametrize('fmt,C,k,affine', dc.SW_CASES)
def test_sliding_window(L, fmt, C, k, affine):
    """fp32 maps against fp64; bf16 maps (both affines) == the fp32 sliding-window result on the bf16-valued input, rounded once."""
    naff = {'none': 0, 'ln': 1, 'adaln': 1, 'both': 2}[affine]
    groups, gpw, blocks = _sw_geometry(C, *dc.SW_SHAPE_INACTIVE)
    assert groups % gpw != 0 and blocks < 8                                # inactive lanes in the last wave (clamped to the last group)
    assert _sw_geometry(C, *dc.SW_SHAPE_REMAP)[2] % 8 != 0 and _sw_geometry(C, *dc.SW_SHAPE_REMAP)[2] > 8   # ragged XCD remap
    for B, H, W in dc.SW_SHAPES:
        assert dc.choice(L, fmt, naff, 0, B, H, W, C, k) == (0, 1, 1, 1)
        g = torch.Generator().manual_seed(C * 10 + k + H + 3 * W)
        x = torch.randn(B, H, W, C, generator=g)
        xin = x.to(torch.bfloat16).cuda() if fmt == 'bf16' else x.cuda()
        xf = xin.float().contiguous()
        prm = Params(g, B, C, k, affine, False)
        what = f'{fmt} C={C} k={k} {affine} {B}x{H}x{W}'
        y32 = _run(L, prm, 'f32', xf, what).view(torch.float32).view(B, H, W, C)
        err = _worst(y32, _ref64(xf, prm.wt, prm.bias, k, prm.affines()))
        print(f'{what}: worst |err| / max(1, |ref|) = {err:.3e}')
        assert err <= TOL, (what, err)
        if fmt == 'bf16':
            _check_relation('bf16', _run(L, prm, 'bf16', xin, what), y32.view(-1, C), B * H * W, C, what)


@pytest.mark.parametrize('fmt,C,k,B,H,W', dc.SW_TH2_CASES)
def test_sliding_window_two_row_instance(L, fmt, C, k, B, H, W):
    """Both affines on a map of >= 100 000 pixels with an odd number of rows: two output rows per group, the last group cut."""
    assert dc.choice(L, fmt, 2, 0, B, H, W, C, k) == (0, 1, 2, 1)
    g = torch.Generator().manual_seed(C + H + W)
    x = torch.randn(B, H, W, C, generator=g).cuda()
    prm = Params(g, B, C, k, 'both', False)
    y32 = _run(L, prm, 'f32', x, f'two-row C={C}').view(torch.float32).view(B, H, W, C)
    err = _worst(y32, _ref64(x, prm.wt, prm.bias, k, prm.affines()))
    print(f'two-row C={C}: worst |err| / max(1, |ref|) = {err:.3e}')
    assert err <= TOL, err


# ------------------------------------------------------------------------------------------------ argument errors
def test_launch_rejects_exactly_what_the_query_rejects(L):
    """On small valid buffers: every (fmt, C, k, affines) -- and the per-image forms -- returns -22 from the launch where the query
    says -22, and launches (0) everywhere else."""
    B, H, W = 1, 2, 6
    g = torch.Generator().manual_seed(1)
    x32 = torch.randn(B, H, W, 512, generator=g).cuda()
    x16 = x32.to(torch.bfloat16)
    n = 0
    for C in (64, 128, 144, 192, 256, 288, 320, 384, 512):
        for k in (1, 2, 3, 5, 7, 9):
            prms = {a: Params(g, B, C, min(k, 7), a, False) for a in ('none', 'adaln', 'ln', 'both')}
            prms['v'] = Params(g, B, C, min(k, 7), 'adaln', True)
            for a, prm in prms.items():
                prm.k = k
                for fmt in dc.FMTS:
                    want = dc.choice(L, fmt, {'none': 0, 'adaln': 1, 'ln': 1, 'both': 2, 'v': 1}[a], a == 'v', B, H, W, C, k)[0]
                    out = Guarded(fmt, B, H, W, 512)
                    rc = prm.launch(L, fmt, x16 if fmt in dc.LOWP else x32, out.ptr())
                    assert rc == want and rc in (0, -22), (fmt, C, k, a, rc, want)
                    n += rc == 0
    torch.cuda.synchronize()
    assert n == (4 * 5 * 4 * 4) + (2 * 4 * 4) + (2 * 5 * 4)      # channel-per-lane (none / adaln / ln / _v), C = 144 / 288 fp32, both affines
