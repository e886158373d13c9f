"""QRes-VAE (`qres34m`, fixed-rate hierarchical VAE) inference codec on MI355X.

API surface of the reference's `HierarchicalVAE` (lvae/models/qresvae/model.py:457-725) for the encode/decode path:
`compress_mode`, `compress` (-> list), `decompress`, `compress_file` / `decompress_file` (pickle container, :690-725),
`max_stride`, nn.Module behaviour, reference state-dict key names (incl. the reference's `downsapmle` spelling).
As for QARV, the module tree only owns parameters; the network runs as native HIP launches recorded in plans:

  MyConvNeXtBlock (:168-182)      -> lvae_dwconv_ln_f32 (affine LN) + fc1/GELU GEMM + fc2/gamma/residual GEMM
  MyConvNeXtPatchDown (:184-192)  -> the same + A_PATCH2 GEMM
  VDBlock (:143-149)              -> 4 GEMMs: c1 with GELU-on-load of its input (optionally a fused torch.cat of two
                                     sources), c2/c3 as A_CONV3 (or plain for k<3), GELU fused in each epilogue
  z_proj (:235-239)               -> A_CONV3/plain GEMM + GELU, then 1x1 GEMM with the residual add into the feature
  prior/posterior heads, coder    -> lvae_prior_index_f32 / lvae_quantize_f32 / lvae_dequantize_f32 + host rANS

The generative surface (:578-638) replays the same plans block by block: `cond_sample` / `uncond_sample` replace each block's
dequantize launch by lvae_latent_sample_box_f32 (prior draw, given latent, or both split by a paint box) and the lossless model's pixel
decoder by lvae_pixel_sample_f32; `forward_get_latents` takes each block's -ln P map (lvae_gaussian_nll_map_f32) right behind its
quantize launch; `inpaint` alternates the two.
"""
import ctypes
import io
import math
import pickle
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from ... import _native
from ...engine import ptr
from ...utils import coding
from ..base import CodecBase, CodecPlan, PackedWeights, on_model_device
from ..entropy_coding import DiscretizedGaussian, log_spaced_table, rans_decode_streams, rans_encode_streams
from ..qarv.model import UpParams, _conv


def box_slices(box, h, w):
    """(r0, r1, c0, c1) of the reference's `slice(round(y1*h), round(y2*h))`, `slice(round(x1*w), round(x2*w))` on an h x w map, with
    Python's round (ties to even) and slicing rules (negative / out-of-range bounds); an empty range gives r0 == r1 (or c0 == c1)."""
    x1, y1, x2, y2 = box
    rows, cols = range(h)[round(y1 * h):round(y2 * h)], range(w)[round(x1 * w):round(x2 * w)]
    if len(rows) == 0 or len(cols) == 0:
        return (0, 0, 0, 0)
    return (rows.start, rows.stop, cols.start, cols.stop)


def latent_box(box, h, w):
    """The paint box on one latent map (QLatentBlockX.forward_uncond): None -- the given latent is kept whole -- on a map with
    min(h, w) == 1, else box_slices."""
    return None if min(h, w) == 1 else box_slices(box, h, w)


# ----------------------------------------------------------------------------------------------- parameter holders
class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class MyCNXParams(nn.Module):
    """timm ConvNeXtBlock as subclassed by the reference (:162-166): conv_dw, norm (affine LN), mlp, gamma (C,)."""
    kind = 'cnx'

    def __init__(self, dim, kernel_size=7, mlp_ratio=2):
        super().__init__()
        self.dim, self.kernel_size, self.hidden = dim, kernel_size, int(mlp_ratio * dim)
        self.conv_dw = nn.Conv2d(dim, dim, kernel_size=kernel_size, padding=(kernel_size - 1) // 2, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, self.hidden)
        self.gamma = nn.Parameter(1e-6 * torch.ones(dim))


class DeconvParams(nn.ConvTranspose2d):
    """common.deconv (common.py:40-45): ConvTranspose2d(k, stride 2, padding k//2, output_padding 1): doubles the resolution."""
    kind = 'deconv'

    def __init__(self, cin, cout, kernel_size=5):
        super().__init__(cin, cout, kernel_size=kernel_size, stride=2, output_padding=1, padding=kernel_size // 2)
        self.cin, self.cout, self.k, self.rate = cin, cout, kernel_size, 2


class NearestUpParams(nn.Upsample):
    """torch.nn.Upsample(scale_factor=s), nearest (qres17m, zoo.py:143)."""
    kind = 'nearest'

    def __init__(self, scale_factor):
        super().__init__(scale_factor=scale_factor)
        self.rate = int(scale_factor)


class MyCNXDownParams(MyCNXParams):
    kind = 'cnxdown'

    def __init__(self, in_ch, out_ch, kernel_size=7, down_rate=2):
        super().__init__(in_ch, kernel_size)
        assert down_rate in (2, 4)
        self.downsapmle = _conv(in_ch, out_ch, down_rate, down_rate, 0)          # [sic] reference attribute name (:187)
        self.out_ch, self.down_rate = out_ch, down_rate


class StemParams(nn.Conv2d):
    kind = 'down'

    def __init__(self, cin, cout, rate):
        super().__init__(cin, cout, rate, rate, 0)
        self.bias.data.mul_(0.0)
        self.rate = rate


class VDParams(nn.Module):
    """VDBlock (:120-141): c1 1x1, c2/c3 3x3 (or 1x1), c4 1x1."""
    def __init__(self, cin, hid, cout, use_3x3, zero_last=False):
        super().__init__()
        k, p = (3, 1) if use_3x3 else (1, 0)
        self.c1, self.c2, self.c3, self.c4 = _conv(cin, hid, 1), _conv(hid, hid, k, 1, p), _conv(hid, hid, k, 1, p), _conv(hid, cout, 1)
        if zero_last:
            self.c4.weight.data.mul_(0.0)
        self.cin, self.hid, self.cout, self.k = cin, hid, cout, k


class QLBParams(nn.Module):
    """QLatentBlockX (:210-243)."""
    kind = 'qlb'

    def __init__(self, width, zdim, kernel_size=7):
        super().__init__()
        self.width, self.zdim, self.kernel_size = width, zdim, kernel_size
        hid = int(width * 0.25)
        use3 = kernel_size >= 3
        self.hid, self.k = hid, (3 if use3 else 1)
        self.resnet_front = MyCNXParams(width, kernel_size)
        self.resnet_end = MyCNXParams(width, kernel_size)
        self.posterior = VDParams(2 * width, hid, zdim, use3)
        self.prior = VDParams(width, hid, 2 * zdim, use3, zero_last=True)
        self.z_proj = nn.Sequential(_conv(zdim, hid // 2, self.k, 1, (self.k - 1) // 2), nn.GELU(), _conv(hid // 2, width, 1))
        self.discrete_gaussian = DiscretizedGaussian(scale_table=None, cdf_form='erfc', scale_bound=0.11, persistent_table=True)
        self.discrete_gaussian.register_buffer('scale_bound', torch.Tensor([0.11]))

    def residual_scaling(self, N):
        self.z_proj[2].weight.data.mul_(math.sqrt(1 / 3 * N))     # (:242-243), operator precedence as in the reference


class _Holder(nn.Module):
    pass


class GaussianNLLOutParams(nn.Module):
    """GaussianNLLOutputNet (:16-94) of qres34m_lossless: conv_mean / conv_scale = patch_upsample(cin, 3, rate 4), and the
    per-pixel entropy model (stock GaussianConditional, scale_bound 0.11, 128 log-spaced scales 0.11..20: update() :59-67)."""
    def __init__(self, cin, im_channels=3, rate=4, bin_size=1 / 127.5):
        super().__init__()
        from ..qarv.model import UpParams
        self.conv_mean, self.conv_scale = UpParams(cin, im_channels, rate), UpParams(cin, im_channels, rate)
        self.cin, self.rate, self.bin_size = cin, rate, bin_size
        self.discrete_gaussian = DiscretizedGaussian(scale_table=None, cdf_form='erfc', scale_bound=0.11, persistent_table=True)
        self.discrete_gaussian.register_buffer('scale_bound', torch.Tensor([0.11]))

    def update(self):
        table = log_spaced_table(0.11, 20, 128)
        self.discrete_gaussian.update_scale_table(table, force=True)


# ----------------------------------------------------------------------------------------------- packed weights
class _Packed(PackedWeights):
    def __init__(self, model, dev):
        super().__init__(model, dev)
        f32 = dict(device=dev, dtype=torch.float32)
        put = self.put

        def cnx(p, m):
            C, k = m.dim, m.kernel_size
            put(p + '.dw_w', m.conv_dw.weight.reshape(C, k * k).t()); put(p + '.dw_b', m.conv_dw.bias)
            put(p + '.ln_w', m.norm.weight); put(p + '.ln_b', m.norm.bias)
            put(p + '.fc1_w', m.mlp.fc1.weight); put(p + '.fc1_b', m.mlp.fc1.bias)
            put(p + '.fc2_w', m.mlp.fc2.weight); put(p + '.fc2_b', m.mlp.fc2.bias)
            put(p + '.gamma', m.gamma.reshape(C))

        def convw(name, c, pad_in=0, pad_out=0):
            w, b = c.weight, c.bias
            if pad_in:
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, pad_in))        # zero weights for padded input channels
            if pad_out:                                                         # zero rows: padded output channels are exactly 0
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, pad_out))
                b = torch.nn.functional.pad(b, (0, pad_out))
            put(name + '.w', w.permute(0, 2, 3, 1).reshape(w.shape[0], -1))     # [Cout][(i,j,ci)]  (== [Cout][Cin] for 1x1)
            put(name + '.b', b)

        def vd(p, m):
            for n in ('c1', 'c2', 'c3', 'c4'):
                convw(f'{p}.{n}', getattr(m, n))

        for i, m in enumerate(model.encoder.enc_blocks):
            p = f'encoder.enc_blocks.{i}'
            if m.kind == 'down':
                put(p + '.w', m.weight.reshape(m.out_channels, -1).t()); put(p + '.b', m.bias)
            else:
                cnx(p, m)
                if m.kind == 'cnxdown' and m.down_rate == 2:
                    convw(p + '.downsapmle', m.downsapmle)
                elif m.kind == 'cnxdown':
                    # 4x4/s4 conv as two 2x2 patch gathers: an exact space-to-depth (identity weights, channel order (i, j, ci))
                    # and a 2x2/s2 conv over the 4C-channel map whose k index (I, J, i, j, ci) is input pixel (2I+i, 2J+j)
                    C, w = m.dim, m.downsapmle.weight                           # [Cout][C][4][4]
                    put(p + '.s2d.w', torch.eye(4 * C)); put(p + '.s2d.b', torch.zeros(4 * C))
                    w6 = w.reshape(w.shape[0], C, 2, 2, 2, 2)                   # [n][ci][I][i][J][j]
                    put(p + '.downsapmle.w', w6.permute(0, 2, 4, 3, 5, 1).reshape(w.shape[0], 16 * C))
                    put(p + '.downsapmle.b', m.downsapmle.bias)
        for i, m in enumerate(model.decoder.dec_blocks):
            p = f'decoder.dec_blocks.{i}'
            if m.kind == 'up':
                w, b = m[0].weight.reshape(m.cout * m.rate ** 2, m.cin), m[0].bias
                if m.cout > 3:
                    r2 = m.rate ** 2
                    w = w.reshape(m.cout, r2, m.cin).permute(1, 0, 2).reshape(r2 * m.cout, m.cin)
                    b = b.reshape(m.cout, r2).t().reshape(-1)
                else:
                    # the eval plan stores the final conv raw (before the clamp) as an NHWC map: the pixel-shuffle column order (i, j, c)
                    # of the same rows -- every output element is the same dot product, so the same bits as the ST_IMAGE store
                    r2 = m.rate ** 2
                    put(p + '.w_raw', w.reshape(m.cout, r2, m.cin).permute(1, 0, 2).reshape(r2 * m.cout, m.cin))
                    put(p + '.b_raw', b.reshape(m.cout, r2).t().reshape(-1))
                put(p + '.w', w); put(p + '.b', b)
            elif m.kind == 'deconv':
                # stride-2 transposed conv as ONE 3x3-gather GEMM with a PixelShuffle store: output pixel (2a+py, 2b+px) reads the
                # input pixels (a+di, b+dj), di, dj in {-1, 0, 1}, through kernel tap (py + p - 2 di, px + p - 2 dj) when it exists
                k, pd, cin, cout = m.k, m.k // 2, m.cin, m.cout
                wt = m.weight                                                   # [Cin][Cout][k][k]
                wp = torch.zeros(2, 2, cout, 3, 3, cin, dtype=wt.dtype)
                for py in range(2):
                    for px in range(2):
                        for di in (-1, 0, 1):
                            for dj in (-1, 0, 1):
                                ky, kx = py + pd - 2 * di, px + pd - 2 * dj
                                if 0 <= ky < k and 0 <= kx < k:
                                    wp[py, px, :, di + 1, dj + 1, :] = wt[:, :, ky, kx].t()
                put(p + '.w', wp.reshape(4 * cout, 9 * cin)); put(p + '.b', m.bias.repeat(4))
            elif m.kind == 'nearest':
                C, r2 = m.channels, m.rate ** 2
                put(p + '.w', torch.eye(C).repeat(r2, 1)); put(p + '.b', torch.zeros(r2 * C))
            else:
                cnx(p + '.resnet_front', m.resnet_front); cnx(p + '.resnet_end', m.resnet_end)
                vd(p + '.posterior', m.posterior); vd(p + '.prior', m.prior)
                zp, hp = (m.zdim + 3) // 4 * 4, (m.hid // 2 + 3) // 4 * 4      # GEMM K must be a multiple of 4 (16-B operand loads)
                convw(p + '.z_proj.0', m.z_proj[0], pad_in=zp - m.zdim, pad_out=hp - m.hid // 2)
                convw(p + '.z_proj.2', m.z_proj[2], pad_in=hp - m.hid // 2)
        put('bias', model.decoder.bias.reshape(-1))
        on = model.out_net
        if isinstance(on, GaussianNLLOutParams):
            # one GEMM for conv_mean | conv_scale with the PixelShuffle folded into the row order: row (i*r + j)*6 + c is
            # mean channel c (c < 3) or scale channel c - 3 of sub-pixel (i, j); conv output channel c*r^2 + i*r + j (common.py:33-38)
            r2 = on.rate ** 2
            wm, ws = on.conv_mean[0].weight.reshape(3, r2, on.cin), on.conv_scale[0].weight.reshape(3, r2, on.cin)
            bm, bs = on.conv_mean[0].bias.reshape(3, r2), on.conv_scale[0].bias.reshape(3, r2)
            put('out_net.w', torch.cat([wm, ws], 0).permute(1, 0, 2).reshape(r2 * 6, on.cin))
            put('out_net.b', torch.cat([bm, bs], 0).t().reshape(-1))
            odg = on.discrete_gaussian
            self.out_scale_table = odg.scale_table.detach().to(**f32).contiguous()
            self.out_scale_bound = float(odg.lower_bound_scale.bound.item())


class _QresPlan(CodecPlan):
    def __init__(self, model, pk, B, H, W, encode, evaluate=False, pos=False):
        """encode: the encode plan ('enc'); evaluate (with encode): the eval plan of forward() ('eval') -- the encode plan with each
        block's per-channel rate behind its quantize launch (kl_chan, fp64 [L][B][z_l] at chan_off[l]), and the distortion in place of
        the coder's sinks: the lossy models' final conv stored raw + lvae_rd_image_f32, the lossless model's lvae_pixel_nll_f32 on the
        out-net map (rd_sums, fp64 [B][2]; `out` = im_hat).  pos (with evaluate): the position plan of rate_map() ('evalp') -- the eval
        plan without the per-channel launches; CodecBase._run_with_pos launches lvae_gaussian_nll_pos_f32 in their place (qcuts) into
        `pos_bufs` (one fp64 (B, h, w) buffer per block), and the lossless model's pixel stage goes to `pix_pos` (fp64 (B, H, W))."""
        super().__init__(model, pk, B)
        evaluate = bool(evaluate and encode)
        pos = bool(pos and evaluate)
        lib = self.lib
        nH, nW = H // 64, W // 64
        # latent I/O sizes: resolution doubles at every rate-2 upsample of the top-down path
        tot, s = 0, 1
        for m in model.decoder.dec_blocks:
            if m.kind == 'qlb':
                tot += m.zdim * nH * s * nW * s
            elif not (m.kind == 'up' and m.cout <= 3):
                s *= m.rate
        self.evaluate = evaluate
        if evaluate:
            self.kl_chan = None if pos else self.new(B * sum(m.zdim for m in model.decoder.dec_blocks if m.kind == 'qlb'), torch.float64)
            self.rd_sums = self.new(B * 2, torch.float64)
            self.rd_ws = self.new(B * _native.EVAL_CHUNKS * 2, torch.float64)     # per-chunk partials of the distortion kernel
            self.chan_off = []
        self.alloc_symbols(tot * B, host=not evaluate)       # (the eval plan's symbols never leave the device)
        feats = {}
        if encode:
            self.im = self.new(B * 3 * H * W)
            h, w, x = H, W, None
            for i, m in enumerate(model.encoder.enc_blocks):
                p = f'encoder.enc_blocks.{i}'
                if m.kind == 'down':
                    h, w = h // 4, w // 4
                    x = self.new(B * h * w * m.out_channels)
                    self.add(lib.lvae_stem_f32, (self.im.data_ptr(), pk.p(p + '.w'), pk.p(p + '.b'), x.data_ptr(), B, H, W,
                                                 m.out_channels, model.im_shift, model.im_scale, self.status_ptr()), p + '.stem')
                elif m.kind == 'cnx':
                    self.cnx(p, m, x.data_ptr(), x.data_ptr(), h, w)
                else:           # CNX out of place (x is this level's encoder feature), then 2x2/s2 conv
                    t = self.buf('cnxdown_tmp', x.numel())
                    self.cnx(p, m, x.data_ptr(), t.data_ptr(), h, w)
                    feats[h] = x
                    h, w = h // 2, w // 2
                    if m.down_rate == 4:
                        s2d = self.buf('s2d', B * h * w * 4 * m.dim)
                        self.gemm(A0=t.data_ptr(), K0=m.dim, M=B * h * w, N=4 * m.dim, K=4 * m.dim, Wt=pk.p(p + '.s2d.w'),
                                  bias=pk.p(p + '.s2d.b'), out=s2d.data_ptr(), a_mode=_native.A_PATCH2, H=h, W=w, exact=True,
                                  label=p + '.space_to_depth')
                        h, w = h // 2, w // 2
                        nx = self.new(B * h * w * m.out_ch)
                        self.gemm(A0=s2d.data_ptr(), K0=4 * m.dim, M=B * h * w, N=m.out_ch, K=16 * m.dim, Wt=pk.p(p + '.downsapmle.w'),
                                  bias=pk.p(p + '.downsapmle.b'), out=nx.data_ptr(), a_mode=_native.A_PATCH2, H=h, W=w, label=p + '.down4')
                    else:
                        nx = self.new(B * h * w * m.out_ch)
                        self.gemm(A0=t.data_ptr(), K0=m.dim, M=B * h * w, N=m.out_ch, K=4 * m.dim, Wt=pk.p(p + '.downsapmle.w'),
                                  bias=pk.p(p + '.downsapmle.b'), out=nx.data_ptr(), a_mode=_native.A_PATCH2, H=h, W=w, label=p + '.down')
                    x = nx
            feats[h] = x
        # top-down path
        h, w = nH, nW
        width = model.decoder.dec_blocks[0].width
        f = self.new(B * h * w * width)
        self.add(lib.lvae_bias_expand_f32, (pk.p('bias'), f.data_ptr(), B * h * w, width), 'bias')
        self.out = None
        for i, m in enumerate(model.decoder.dec_blocks):
            p = f'decoder.dec_blocks.{i}'
            if m.kind == 'deconv':
                nf = self.new(B * h * w * 4 * m.cout)
                self.gemm(A0=f.data_ptr(), K0=m.cin, M=B * h * w, N=4 * m.cout, K=9 * m.cin, Wt=pk.p(p + '.w'), bias=pk.p(p + '.b'),
                          out=nf.data_ptr(), a_mode=_native.A_CONV3, store=_native.ST_SHUFFLE, r=2, H=h, W=w, label=p + '.deconv')
                f, h, w = nf, h * 2, w * 2
                continue
            if m.kind == 'nearest':
                C = m.channels
                nf = self.new(B * h * w * m.rate ** 2 * C)
                self.gemm(A0=f.data_ptr(), K0=C, M=B * h * w, N=m.rate ** 2 * C, Wt=pk.p(p + '.w'), bias=pk.p(p + '.b'), out=nf.data_ptr(),
                          store=_native.ST_SHUFFLE, r=m.rate, H=h, W=w, exact=True, label=p + '.nearest')
                f, h, w = nf, h * m.rate, w * m.rate
                continue
            if m.kind == 'up':
                nf = self.new(B * h * w * m.rate ** 2 * m.cout)
                final = m.cout <= 3
                if final and evaluate:
                    # the ST_IMAGE launch below with the raw NHWC store (same tile and kernel: the choice depends on the shape alone)
                    self.gemm(A0=f.data_ptr(), K0=m.cin, M=B * h * w, N=m.cout * m.rate ** 2, Wt=pk.p(p + '.w_raw'), bias=pk.p(p + '.b_raw'),
                              out=nf.data_ptr(), store=_native.ST_SHUFFLE, r=m.rate, H=h, W=w, label=p + '.up_raw')
                    h, w = h * m.rate, w * m.rate
                    self.x_raw = nf                             # test access: the reconstruction before the clamp, NHWC [B*H*W][3]
                    im_hat = self.new(B * 3 * h * w)
                    self.add(lib.lvae_rd_image_f32, (nf.data_ptr(), self.im.data_ptr(), im_hat.data_ptr(), self.rd_sums.data_ptr(),
                                                     self.rd_ws.data_ptr(), B, h, w,
                                                     self.status_ptr()), 'rd_image')
                    self.out = im_hat.view(B, 3, h, w)
                    continue
                self.gemm(A0=f.data_ptr(), K0=m.cin, M=B * h * w, N=m.cout * m.rate ** 2, Wt=pk.p(p + '.w'), bias=pk.p(p + '.b'),
                          out=nf.data_ptr(), store=_native.ST_IMAGE if final else _native.ST_SHUFFLE, r=m.rate, H=h, W=w, label=p + '.up')
                f, h, w = nf, h * m.rate, w * m.rate
                if final:
                    self.out = nf.view(B, m.cout, h, w)
                continue
            M, z, hid = B * h * w, m.zdim, m.hid
            zp = (z + 3) // 4 * 4
            self.cnx(p + '.resnet_front', m.resnet_front, f.data_ptr(), f.data_ptr(), h, w)
            prm = self.buf('prm', M * 2 * z)
            self.vdblock(p + '.prior', m.prior, f.data_ptr(), None, prm.data_ptr(), h, w)
            pm = self.new(M * z)
            ioff = sum(a * b for a, b in self.lat_shapes) * B
            self.lat_shapes.append((z, h * w)); self.idx_off.append(ioff); self.sym_off.append(ioff)
            self.pm_bufs.append(pm); self.lat_hw.append((h, w))
            self.add(lib.lvae_prior_index_f32, (prm.data_ptr(), pm.data_ptr(), ptr(self.idx_all, ioff), pk.scale_table.data_ptr(),
                                                pk.scale_table.numel(), pk.scale_bound, B, h * w, z, self.status_ptr()), p + '.prior_index')
            zhat = self.buf('zhat', M * zp)
            self.prm_bufs.append(prm); self.zhat_bufs.append(zhat); self.zhat_ld.append(zp)
            if encode:
                qm = self.buf('qm', M * z)
                self.vdblock(p + '.posterior', m.posterior, f.data_ptr(), feats[h].data_ptr(), qm.data_ptr(), h, w)
                self.add(lib.lvae_quantize_f32, (qm.data_ptr(), pm.data_ptr(), ptr(self.sym_all, ioff), zhat.data_ptr(), B, h * w, z, zp, self.status_ptr()),
                         p + '.quantize')
                self.qm_bufs.append(qm)
                self.qcuts.append(len(self.ops))
                if evaluate and not pos:            # prm still holds this block's prior (scratch shared by every block)
                    co = B * sum(zz for zz, _ in self.lat_shapes[:-1])
                    self.chan_off.append(co)
                    self.add(lib.lvae_gaussian_nll_chan_f32, (prm.data_ptr(), ptr(self.sym_all, ioff), ptr(self.kl_chan, co), pk.scale_bound,
                                                              B, h * w, z, 1), p + '.nll_chan')
            else:
                self.cuts.append(len(self.ops))
                self.add(lib.lvae_dequantize_f32, (ptr(self.sym_all, ioff), pm.data_ptr(), zhat.data_ptr(), B, h * w, z, zp), p + '.dequantize')
            hp = (hid // 2 + 3) // 4 * 4
            v = self.buf('zproj_h', M * hp)
            conv3 = m.k == 3
            self.gemm(A0=zhat.data_ptr(), K0=zp, M=M, N=hp, K=(9 * zp if conv3 else zp), Wt=pk.p(p + '.z_proj.0.w'),
                      bias=pk.p(p + '.z_proj.0.b'), out=v.data_ptr(), a_mode=_native.A_CONV3 if conv3 else _native.A_PLAIN, H=h, W=w,
                      epi=_native.EPI_BIAS_GELU, label=p + '.z_proj.0')
            self.gemm(A0=v.data_ptr(), K0=hp, M=M, N=m.width, Wt=pk.p(p + '.z_proj.2.w'), bias=pk.p(p + '.z_proj.2.b'),
                      res=f.data_ptr(), ldres=m.width, out=f.data_ptr(), epi=_native.EPI_RES, label=p + '.z_proj.2')
            self.cnx(p + '.resnet_end', m.resnet_end, f.data_ptr(), f.data_ptr(), h, w)
        self.lossless = isinstance(model.out_net, GaussianNLLOutParams)
        if pos:
            self.alloc_pos()
            self.pix_pos = self.new(B * H * W, torch.float64) if self.lossless else None
        if self.lossless:
            # GaussianNLLOutputNet.compress / decompress (:69-94): per-pixel coding of the 3*H*W image samples
            on = model.out_net
            Ho, Wo = h * on.rate, w * on.rate
            assert (Ho, Wo) == (H, W)
            raw = self.new(B * Ho * Wo * 6)
            self.px_raw = raw                               # test access: conv_mean | conv_scale after PixelShuffle, NHWC [B*H*W][6]
            self.gemm(A0=f.data_ptr(), K0=on.cin, M=B * h * w, N=6 * on.rate ** 2, Wt=pk.p('out_net.w'), bias=pk.p('out_net.b'),
                      out=raw.data_ptr(), store=_native.ST_SHUFFLE, r=on.rate, H=h, W=w, label='out_net.conv')
            if evaluate:                # forward_loss: the pixel likelihood of the unrounded mean, no coder parameters
                im_hat = self.new(B * 3 * H * W)
                self.nll_op = len(self.ops)                 # rate_map without im_hat replays up to here: px_raw is all it needs
                self.add(lib.lvae_pixel_nll_f32, (raw.data_ptr(), self.im.data_ptr(), im_hat.data_ptr(), self.rd_sums.data_ptr(),
                                                  self.rd_ws.data_ptr(), B, H, W,
                                                  self.status_ptr()), 'out_net.nll')
                self.out = im_hat.view(B, 3, H, W)
                return
            npx = B * 3 * H * W
            self.px_pm = self.new(npx)
            self.px_sym, self.px_idx = self.new(npx, torch.int32), self.new(npx, torch.uint8)
            self.px_sym_host = torch.empty(npx, dtype=torch.int32).pin_memory()
            self.px_idx_host = torch.empty(npx, dtype=torch.uint8).pin_memory()
            self.px_sym_np, self.px_idx_np = self.px_sym_host.numpy(), self.px_idx_host.numpy()
            self.px_params_op = len(self.ops)               # sampling replays up to here and draws the pixels from px_raw instead
            self.add(lib.lvae_lossless_params_f32, (raw.data_ptr(), self.im.data_ptr() if encode else None, self.px_pm.data_ptr(),
                                                    self.px_idx.data_ptr(), self.px_sym.data_ptr() if encode else None,
                                                    pk.out_scale_table.data_ptr(), pk.out_scale_table.numel(), pk.out_scale_bound,
                                                    B, H, W, self.status_ptr()), 'out_net.params')
            if not encode:
                self.cuts.append(len(self.ops))
                out = self.new(npx)
                self.add(lib.lvae_lossless_output_f32, (self.px_sym.data_ptr(), self.px_pm.data_ptr(), out.data_ptr(), npx, self.status_ptr()), 'out_net.output')
                self.out = out.view(B, 3, H, W)
        if not encode:
            assert self.out is not None

    def dwln_add(self, fmt, p, x, y, H, W, C, k):
        """MyConvNeXtBlock (:168-182): the affine is the block's LayerNorm weights."""
        pk = self.pk
        self.add(getattr(self.lib, 'lvae_dwconv_ln_' + fmt), (x, pk.p(p + '.dw_w'), pk.p(p + '.dw_b'), pk.p(p + '.ln_w'), pk.p(p + '.ln_b'), None, None, y, self.B, H, W, C, k), p + '.dwln')

    def vdblock(self, p, m, a0, a1, out, H, W):
        """c4(g(c3(g(c2(g(c1(g(x)))))))) with x = a0 or cat[a0, a1] (each of width cin or cin/2)."""
        pk = self.pk
        M, hid = self.B * H * W, m.hid
        t1, t2 = self.buf('vd1', M * hid), self.buf('vd2', M * hid)
        k0 = m.cin if a1 is None else m.cin // 2
        self.gemm(A0=a0, K0=k0, A1=a1, K1=(0 if a1 is None else k0), lda1=(0 if a1 is None else k0), M=M, N=hid,
                  Wt=pk.p(p + '.c1.w'), bias=pk.p(p + '.c1.b'), out=t1.data_ptr(), a_gelu=1, epi=_native.EPI_BIAS_GELU, label=p + '.c1')
        mode = _native.A_CONV3 if m.k == 3 else _native.A_PLAIN
        kk = 9 * hid if m.k == 3 else hid
        self.gemm(A0=t1.data_ptr(), K0=hid, M=M, N=hid, K=kk, Wt=pk.p(p + '.c2.w'), bias=pk.p(p + '.c2.b'), out=t2.data_ptr(),
                  a_mode=mode, H=H, W=W, epi=_native.EPI_BIAS_GELU, label=p + '.c2')
        self.gemm(A0=t2.data_ptr(), K0=hid, M=M, N=hid, K=kk, Wt=pk.p(p + '.c3.w'), bias=pk.p(p + '.c3.b'), out=t1.data_ptr(),
                  a_mode=mode, H=H, W=W, epi=_native.EPI_BIAS_GELU, label=p + '.c3')
        self.gemm(A0=t1.data_ptr(), K0=hid, M=M, N=m.cout, Wt=pk.p(p + '.c4.w'), bias=pk.p(p + '.c4.b'), out=out, label=p + '.c4')


# ----------------------------------------------------------------------------------------------- the model
class HierarchicalVAE(CodecBase):
    log2_e = math.log2(math.e)

    def __init__(self, config: dict):
        super().__init__()
        self.encoder = _Holder()
        self.encoder.enc_blocks = nn.ModuleList(config.pop('enc_blocks'))
        self.decoder = _Holder()
        self.decoder.dec_blocks = nn.ModuleList(config.pop('dec_blocks'))
        width = self.decoder.dec_blocks[0].width
        cur = width
        for b in self.decoder.dec_blocks:                     # nn.Upsample has no channel count of its own
            if b.kind == 'nearest':
                b.channels = cur
            elif b.kind in ('up', 'deconv'):
                cur = b.cout
        self.decoder.bias = nn.Parameter(torch.zeros(1, width, 1, 1))
        n_res = len([b for b in self.decoder.dec_blocks if hasattr(b, 'residual_scaling')])
        for b in self.decoder.dec_blocks:                     # TopDownDecoder._init_weights (:373-377)
            if hasattr(b, 'residual_scaling'):
                b.residual_scaling(n_res)
        self.out_net = config.pop('out_net', nn.Identity())
        self.im_shift, self.im_scale = float(config['im_shift']), float(config['im_scale'])
        self.max_stride = config['max_stride']
        self.register_buffer('_dummy', torch.zeros(1), persistent=False)
        self.compressing = False
        self.num_latents = sum(1 for b in self.decoder.dec_blocks if b.kind == 'qlb')
        self._stats_log = dict()
        self._init_codec_base()

    def _latent_blocks(self):
        return [b for b in self.decoder.dec_blocks if b.kind == 'qlb']

    def load_state_dict(self, state_dict, strict=True, **k):
        """Reference key names; entropy-model buffers (`*.discrete_gaussian.*`) absent from / extra in a checkpoint are
        tolerated (their set differs between CompressAI versions; the tables are rebuilt by compress_mode())."""
        own = self.state_dict()
        sd = {kk: v for kk, v in state_dict.items() if not ('.discrete_gaussian.' in kk and (kk not in own or own[kk].shape != v.shape))}
        for kk, v in own.items():
            if '.discrete_gaussian.' in kk and kk not in sd:
                sd[kk] = v
        return super().load_state_dict(sd, strict=strict, **k)

    def _build_packed(self, dev):
        return _Packed(self, dev)

    def _plan_key(self, kind, B, H, W, group=0):
        return (kind, B, H, W, group, self._prec)

    def _build_plan(self, kind, B, H, W, group=0):
        return _QresPlan(self, self._packed, B, H, W, encode=(kind in ('enc', 'eval', 'evalp')), evaluate=(kind in ('eval', 'evalp')), pos=(kind == 'evalp'))

    def compress_mode(self, mode=True):
        """(:640-647) -> QLatentBlockX.update (:317-325): 64 log-spaced scales 0.1..20, stock erfc-form tables."""
        if mode:
            table = log_spaced_table(0.1, 20, 64)
            dgs = self._build_cdf_tables(lambda dg: dg.update_scale_table(table, force=True))
            for dg in dgs[1:]:
                dg.scale_table = dgs[0].scale_table
            if isinstance(self.out_net, GaussianNLLOutParams):            # (:645-646)
                self.out_net.update()
            self._log_precision()
            # the packed device copy holds the scale table: one built before this call (encode_trace(), or a compress() that
            # stopped at 'Uninitialized CDFs') would keep the empty pre-update table
            self._invalidate()
        self.compressing = mode

    @torch.no_grad()
    @on_model_device
    def compress_batch(self, im, u8=None):
        """(B,3,H,W) -> list of B compressed objects, each `[ [bytes] x 12, (1, C, H/64, W/64) ]` as `compress()` returns.
        u8 (compress_images): a utils.image.U8Batch in place of `im` (then None), converted straight into each group's plan input."""
        if u8 is None:
            assert im.dim() == 4 and im.shape[1] == 3
        B, _, H, W = u8.shape if u8 is not None else im.shape
        assert H % self.max_stride == 0 and W % self.max_stride == 0, f'{(B, 3, H, W)=}'
        self._prepare()
        tables = self._dg().host_tables()
        groups = self._groups(B, 'enc')
        nthreads = self._coder_threads_per_group(len(groups))
        width = self.decoder.dec_blocks[0].width

        def encode_group(g, start, n, stream):
            pl = self._plan('enc', n, H, W, g)
            self._load_input(pl.im.view(n, 3, H, W), im, u8, start, n)
            pl.run(stream=stream.cuda_stream)
            pl.sym_host.copy_(pl.sym_all, non_blocking=True)
            pl.idx_host.copy_(pl.idx_all, non_blocking=True)
            if pl.lossless:
                pl.px_sym_host.copy_(pl.px_sym, non_blocking=True)
                pl.px_idx_host.copy_(pl.px_idx, non_blocking=True)
            pl.fetch_status()
            stream.synchronize()
            pl.raise_if_flagged(where='while encoding')      # out-of-range input / NaN or inf in a prior parameter or posterior mean
            sv, iv = [], []
            for b in range(n):
                for li, (z, hw) in enumerate(pl.lat_shapes):
                    o = pl.sym_off[li] + b * z * hw
                    sv.append(pl.sym_np[o:o + z * hw]); iv.append(pl.idx_np[o:o + z * hw])
            strings = rans_encode_streams(tables, sv, iv, nthreads)
            nl = len(pl.lat_shapes)
            objs = [[[s] for s in strings[b * nl:(b + 1) * nl]] + [(1, width, H // 64, W // 64)] for b in range(n)]
            if pl.lossless:                                  # final string of the output net (:664-667)
                px = 3 * H * W
                fin = rans_encode_streams(self.out_net.discrete_gaussian.host_tables(),
                                          [pl.px_sym_np[b * px:(b + 1) * px] for b in range(n)],
                                          [pl.px_idx_np[b * px:(b + 1) * px] for b in range(n)], nthreads)
                for b in range(n):
                    objs[b].append([fin[b]])
            return objs

        out = []
        for part in self._run_groups(encode_group, groups):
            out += part
        return out

    @torch.no_grad()
    @on_model_device
    def decompress_batch(self, objs):
        B = len(objs)
        lossless = isinstance(self.out_net, GaussianNLLOutParams)
        si = -2 if lossless else -1                          # position of the feature-shape tuple (:660-667)
        shape = tuple(objs[0][si])
        assert all(tuple(o[si]) == shape for o in objs) and shape[0] == 1
        nH, nW = shape[2], shape[3]
        H, W = nH * 64, nW * 64
        self._prepare()
        tables = self._dg().host_tables()
        groups = self._groups(B, 'dec')
        nthreads = self._coder_threads_per_group(len(groups))
        out = torch.empty(B, 3, H, W, device=self._dummy.device)

        def decode_group(g, start, n, stream):
            pl = self._plan('dec', n, H, W, g)
            assert all(len(objs[start + b]) - 1 == len(pl.cuts) for b in range(n)), 'wrong number of latent strings'
            if self.native_group_loops and not pl.lossless:
                # the loop below as ONE foreign call (csrc/plan_runtime.cpp::lvae_decode_blocks; lossless plans keep the loop: their
                # last stream uses the output net's tables)
                self._decode_group_native(pl, pl.cuts, pl.idx_off, n, [[objs[start + b][li][0] for li in range(len(pl.cuts))] for b in range(n)],
                                          tables, nthreads, stream)
                out[start:start + n].copy_(pl.out, non_blocking=True)
                return
            # (every entry but the feature-shape tuple: one string per cut, the lossless model's last being its pixels')
            strings = [[s[0] for s in o[:si] + o[len(o) + si + 1:]] for o in objs[start:start + n]]
            self._decode_group_loop(pl, n, strings, tables, nthreads, stream)
            out[start:start + n].copy_(pl.out, non_blocking=True)

        self._run_groups(decode_group, groups)
        self._check_decoded(groups, lambda g, n: self._plan('dec', n, H, W, g))
        return out

    def _decode_block(self, pl, li, n, strings, tables, nthreads, stream):
        if not (pl.lossless and li == len(pl.cuts) - 1):
            return super()._decode_block(pl, li, n, strings, tables, nthreads, stream)
        px = pl.px_idx.numel() // n                         # the per-pixel stream of the output net (:680-682)
        pl.px_idx_host.copy_(pl.px_idx, non_blocking=True)
        stream.synchronize()
        t1 = time.time()
        rans_decode_streams(self.out_net.discrete_gaussian.host_tables(), strings,
                            [pl.px_idx_np[b * px:(b + 1) * px] for b in range(n)],
                            [pl.px_sym_np[b * px:(b + 1) * px] for b in range(n)], nthreads)
        pl.px_sym.copy_(pl.px_sym_host, non_blocking=True)
        return t1

    def _pack_blob(self, body, size):
        """(:689-707): pickle of [strings..., feature shape, (h, w)], written through a file object as compress_file always has."""
        buf = io.BytesIO()
        pickle.dump(body + [tuple(size)], file=buf)
        return buf.getvalue()

    def _unpack_blob(self, blob):
        obj = pickle.loads(blob)
        size = obj.pop()
        return obj, size, tuple(obj[-2 if isinstance(self.out_net, GaussianNLLOutParams) else -1])

    @torch.no_grad()
    @on_model_device
    def encode_trace(self, im, full=False, force_z=None):
        """Per-block symbols / indexes of the encode plan (parity tests); `full` / `force_z` as in the qarv model's encode_trace."""
        B, _, H, W = im.shape
        self._prepare()
        pl = self._plan('enc', B, H, W)
        pl.im.view(B, 3, H, W).copy_(im)
        return self._trace(pl, B, full, force_z)

    # ---- the eval-mode forward pass (reference qresvae/model.py:517-576): rate and distortion without entropy coding
    @torch.no_grad()
    @on_model_device
    def forward(self, im, return_rec=False):
        """The reference's `model(im)`: one run of the eval plan (the encode plan with each block's per-channel rate,
        lvae_gaussian_nll_chan_f32, and the distortion kernel in place of the coder's sinks).  Returns an OrderedDict
          loss   0-d tensor on the model device, (kl + out_loss).mean(0)
          kl     nats per dimension, batch mean
          mse    (lossy models) the out net's loss: mean((x_hat - x_target)^2) * mse_lmb on the UNCLAMPED reconstruction, batch mean
          nll    (lossless model) -log P per dimension of the pixels under the out net's discretised Gaussian, batch mean
          bppix, psnr (from the batch-mean MSE of im_hat), and im_hat (B, 3, H, W) when return_rec
        and fills self._stats_log['{train|eval}_bpdim' / '_bppix' / '_channels'].  The statistics are always the eval-mode (quantised)
        ones: the package has no training path, and model.train() adds no training noise -- it only changes the _stats_log key.
        Deterministic: two calls on the same input return the same bits.  A NaN / inf raises NonFiniteError."""
        im = im.to(self._dummy.device)
        assert im.dim() == 4 and im.shape[1] == 3 and not im.requires_grad, f'{im.shape=}'
        B, imC, imH, imW = im.shape
        assert imH % self.max_stride == 0 and imW % self.max_stride == 0, f'{im.shape=}'
        self._ensure_tables()
        self._prepare()
        pl = self._plan('eval', B, imH, imW)
        pl.im.view(B, 3, imH, imW).copy_(im)
        pl.run()
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        pl.raise_if_flagged(where='in forward()')       # out-of-range input: AssertionError, as the reference's preprocess_input
        kl_chan, rd = pl.kl_chan.cpu(), pl.rd_sums.view(B, 2).cpu()
        ndims = imC * imH * imW
        chans = [kl_chan[o:o + B * z].view(B, z) for o, (z, _) in zip(pl.chan_off, pl.lat_shapes)]     # nats per (image, channel)
        kl_divergences = [c.sum(1) for c in chans]
        kl = sum(kl_divergences) / ndims
        if pl.lossless:
            out_loss, loss_name = rd[:, 0] / ndims, 'nll'
        else:
            out_loss, loss_name = rd[:, 0] / ndims * self.mse_lmb, 'mse'
        im_mse = float(rd[:, 1].sum()) / (B * ndims)
        nats_per_dim = float(kl.mean(0))
        kls = torch.stack([k.mean(0) / ndims for k in kl_divergences])
        bpdim = kls * self.log2_e
        mode = 'train' if self.training else 'eval'
        self._stats_log[f'{mode}_bpdim'] = bpdim.tolist()
        self._stats_log[f'{mode}_bppix'] = (bpdim * imC).tolist()
        self._stats_log[f'{mode}_channels'] = [(c.mean(0) / (imH * imW) * self.log2_e).tolist() for c in chans]
        stats = OrderedDict()
        stats['loss'] = (kl + out_loss).mean(0).to(device=self._dummy.device, dtype=torch.float32)
        stats['kl'] = nats_per_dim
        stats[loss_name] = float(out_loss.mean(0))
        stats['bppix'] = nats_per_dim * self.log2_e * imC
        stats['psnr'] = -10 * math.log10(im_mse)
        if return_rec:
            stats['im_hat'] = pl.out.clone()
        return stats

    def _rate_map_run(self, im, u8, B, H, W, lmb, return_rec):
        """CodecBase.rate_map: one run of the 'evalp' plan (forward()'s launches, the position kernel in place of the per-channel one), then
        the lossless model's pixel stage by position from the out-net map the plan left.  Without return_rec the launches that only make
        im_hat are left out: the lossy models stop behind the last block's position kernel, the lossless one in front of
        lvae_pixel_nll_f32 (whose terms lvae_pixel_nll_pos_f32 evaluates)."""
        self._ensure_tables()
        self._prepare()
        pl = self._plan('evalp', B, H, W)
        self._load_input(pl.im.view(B, 3, H, W), im, u8, 0, B)
        self._run_with_pos(pl, 1, upto=None if return_rec else (pl.nll_op if pl.lossless else pl.qcuts[-1]))
        if pl.lossless:
            st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
            _native.check(pl.lib.lvae_pixel_nll_pos_f32(pl.px_raw.data_ptr(), pl.im.data_ptr(), pl.pix_pos.data_ptr(), B, H, W, pl.status_ptr(), st),
                          'lvae_pixel_nll_pos_f32')
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        pl.raise_if_flagged(where='in rate_map()')
        return pl, pl.pix_pos, (pl.out.clone() if return_rec else None)

    @torch.no_grad()
    def forward_eval(self, *args, **kwargs):
        """(:572-576) = forward."""
        return self.forward(*args, **kwargs)

    # ---- the generative API (reference qresvae/model.py:578-638): sampling, latents, inpainting.  Latents and pixels are drawn by the
    # device Philox stream (lvae_latent_sample_box_f32 / lvae_pixel_sample_f32), not by torch's RNG: a call is reproducible by its
    # `seed`, and at temperature 0 (no noise) its result is the reference's.
    @torch.no_grad()
    @on_model_device
    def cond_sample(self, latents, nhw_repeat=None, temprature=1.0, paint_box=None, *, seed=None, return_latents=False):
        """Decoder output for a list of latents (:591-603, forward_with_latents :403-417, QLatentBlockX.forward_uncond :284-315).
        latents[i] is a (B, z_i, h_i, w_i) tensor (e.g. a `forward_get_latents` z) or None:
          None                    -> the block is drawn from the prior, z = pm + pv*t*N(0,1) + t*U(-1/2, 1/2);
          given, paint_box None   -> used verbatim;
          given, paint_box        -> drawn inside the box (x1, y1, x2, y2) in [0, 1] units, rows round(y1*h):round(y2*h) and columns
                                     round(x1*w):round(x2*w) of the block's map, kept outside it; a map with min(h, w) == 1 is kept whole.
        nhw_repeat = (B, h, w) of the top latent map; None takes it from latents[0].  The lossless model draws its pixels too
        (GaussianNLLOutputNet.sample, continuous mode).  seed: the Philox key (default: a fresh one from torch's CPU generator, so
        torch.manual_seed makes calls reproducible).  return_latents=True (not in the reference) also returns the latents used.
        With nothing drawn, or t = 0, a NaN / inf raises NonFiniteError; otherwise the sample is returned whatever it holds."""
        if nhw_repeat is None:
            assert latents[0] is not None, 'nhw_repeat should be provided when latents[0] is None'
            B, _, nH, nW = latents[0].shape
        else:
            B, nH, nW = nhw_repeat
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._ensure_tables()
        self._prepare()
        pl = self._plan('dec', B, nH * 64, nW * 64)
        return self._sample(pl, latents, float(temprature), paint_box, int(seed), 0, return_latents)

    @torch.no_grad()
    def uncond_sample(self, nhw_repeat, temprature=1.0, *, seed=None, return_latents=False):
        """Generate new images from the prior alone (:578-589); nhw_repeat = (B, h, w) of the top latent map (images of 64h x 64w)."""
        return self.cond_sample([None] * self.num_latents, nhw_repeat, temprature, seed=seed, return_latents=return_latents)

    def _ensure_tables(self):
        """The plans' prior heads index into the scale table, which compress_mode() builds (a fixed log-spaced table, no weights
        involved); the reference's generative calls do not need it, so they build it here when it is missing."""
        if self._dg().scale_table.numel() == 0:
            self.compress_mode()

    def _sample(self, pl, latents, t, paint_box, seed, salt, return_latents):
        """Replay the decode plan block by block; each block's dequantize launch (at `cuts[li]`) is replaced by the box sampler writing
        the same z buffer.  Counters: latent block li at li << 40, the lossless model's pixels at L << 40, plus `salt`."""
        L, B = len(pl.lat_shapes), pl.B
        assert len(latents) == L, f'{len(latents)} latents for {L} latent blocks'
        st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
        lo, used, drawn, keep = 0, [], False, []
        for li in range(L):
            cut = pl.cuts[li]
            pl.run(lo, cut)
            z, hw = pl.lat_shapes[li]
            h, w = pl.lat_hw[li]
            lat = latents[li]
            if lat is None:
                box, lat_ptr = (0, h, 0, w), None
            else:
                assert tuple(lat.shape) == (B, z, h, w), f'latent {li}: shape {tuple(lat.shape)}, expected {(B, z, h, w)}'
                lat = lat.to(pl.device, torch.float32).contiguous()
                keep.append(lat)
                box = latent_box(paint_box, h, w) if paint_box is not None else None
                box, lat_ptr = (box or (0, 0, 0, 0)), lat.data_ptr()
            drawn = drawn or (box[1] > box[0] and box[3] > box[2])
            rc = pl.lib.lvae_latent_sample_box_f32(pl.prm_bufs[li].data_ptr(), lat_ptr, pl.zhat_bufs[li].data_ptr(), B, h, w, z,
                                                   pl.zhat_ld[li], *box, t, seed, (li << 40) + salt, st)
            _native.check(rc, 'lvae_latent_sample_box_f32')
            lo = cut + 1
            if return_latents:
                ld = pl.zhat_ld[li]
                zs = pl.zhat_bufs[li][:B * hw * ld].view(B, hw, ld)[:, :, :z]
                used.append(zs.permute(0, 2, 1).reshape(B, z, h, w).clone())
        if pl.lossless:
            H, W = pl.out.shape[2:]
            pl.run(lo, pl.px_params_op)
            rc = pl.lib.lvae_pixel_sample_f32(pl.px_raw.data_ptr(), pl.out.data_ptr(), B, H, W, t, seed, (L << 40) + salt,
                                              pl.status_ptr(), st)
            _native.check(rc, 'lvae_pixel_sample_f32')
            drawn = True
        else:
            pl.run(lo, None)
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        if drawn and t != 0.0:
            # random numbers of the model's own scale (with untrained weights the deeper blocks' prior scales are astronomically large):
            # whatever they lead to is the sample, as in the reference -- clear the word, no error
            pl.status.zero_(); pl.status_host.zero_()
        else:
            pl.raise_if_flagged(where='in cond_sample()')
        out = pl.out.clone()
        return (out, used) if return_latents else out

    @torch.no_grad()
    @on_model_device
    def forward_get_latents(self, im):
        """The eval-mode forward pass of the reference (:605-611, QLatentBlockX.forward_train :257-282): per latent block
        dict(z=(B, z, h, w) quantised latent symbols + pm, kl=(B, z, h, w) -ln P of each element under the prior, CompressAI
        GaussianConditional likelihood: scale bound 0.11, erfc form, P >= 1e-9).  Runs the encode plan up to the last latent."""
        B, _, H, W = im.shape
        assert H % self.max_stride == 0 and W % self.max_stride == 0, f'{im.shape=}'
        self._ensure_tables()
        pk = self._prepare()
        pl = self._plan('enc', B, H, W)
        pl.im.view(B, 3, H, W).copy_(im)
        st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
        kls, lo = [], 0
        for li, cut in enumerate(pl.qcuts):
            pl.run(lo, cut)
            lo = cut
            # prm is scratch shared by every block: the block's kl map is taken right behind its quantize launch
            z, hw = pl.lat_shapes[li]
            kl = torch.empty(B, z, *pl.lat_hw[li], device=pl.device)
            rc = pl.lib.lvae_gaussian_nll_map_f32(pl.prm_bufs[li].data_ptr(), ptr(pl.sym_all, pl.sym_off[li]), kl.data_ptr(),
                                                  pk.scale_bound, B, hw, z, 1, st)
            _native.check(rc, 'lvae_gaussian_nll_map_f32')
            kls.append(kl)
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        pl.raise_if_flagged(where='in forward_get_latents()')
        out = []
        for li, (z, hw) in enumerate(pl.lat_shapes):
            o = pl.sym_off[li]
            sym = pl.sym_all[o:o + B * z * hw].view(B, z, hw).float()
            pm = pl.pm_bufs[li].view(B, hw, z).permute(0, 2, 1)
            out.append(dict(z=(sym + pm).reshape(B, z, *pl.lat_hw[li]), kl=kls[li]))
        return out

    @torch.no_grad()
    @on_model_device
    def inpaint(self, im, paint_box, steps=1, temprature=1.0, *, seed=None):
        """Inpainting (:613-638): `steps` rounds of forward_get_latents -> cond_sample(paint_box) on the image with the box replaced by
        the previous round's clamped sample.  Returns the last whole sample (not a composite).  Round s draws at counter salt s << 48."""
        _, _, H, W = im.shape
        r0, r1, c0, c1 = box_slices(paint_box, H, W)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        im = im.to(self._dummy.device)
        im_input = im.clone()
        for s in range(steps):
            latents = [st['z'] for st in self.forward_get_latents(im_input)]
            pl = self._plan('dec', im.shape[0], H, W)
            im_sample = self._sample(pl, latents, float(temprature), paint_box, int(seed), s << 48, False)
            im_sample.clamp_(min=0, max=1)
            im_input = im.clone()
            im_input[:, :, r0:r1, c0:c1] = im_sample[:, :, r0:r1, c0:c1]
        return im_sample
