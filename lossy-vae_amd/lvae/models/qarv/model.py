"""QARV (variable-rate hierarchical VAE) inference codec on MI355X.

API surface of the reference's `VariableRateLossyVAE` (lvae/models/qarv/model.py:169-581) for the encode/decode
path: `compress_mode`, `compress`, `decompress`, `compress_file`, `decompress_file`, `default_lmb`, `lmb_range`,
`max_stride`, `num_latents`, nn.Module behaviour (`.to`, `.eval`, `.parameters`, `load_state_dict` with the
reference's key names).  Bitstreams use the reference's container (qarv/model.py:525-528,567).

Nothing here calls a PyTorch compute kernel on the hot path: the module tree below only OWNS parameters under the
reference's names; `_prepare()` repacks them once into NHWC/GEMM-friendly device arrays and `_EncPlan`/`_DecPlan`
record the whole network as native HIP launches (lvae/engine.py).  Extension over the reference: `compress_batch` /
`decompress_batch` code B images per call (reference: batch 1 only, model.py:521) -- the GPU part runs batched, the
rANS streams of the B images x 9 latent blocks are coded by parallel host threads.
"""
import ctypes
import math
import os
import struct
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from ... import _native
from ...engine import ptr
from ...utils import coding
from ..base import CodecBase, CodecPlan, PackedWeights, on_model_device
from ..entropy_coding import DiscretizedGaussian, rans_encode_streams

EMBED_DIM = 256
# `model.side_streams` (default on since round 5): encode plans up to this many pixels per launch run posterior0 and the prior heads on a
# side stream (single images / small batches: the GPU is far from full and every launch of a branch is latency on the critical path:
# 0.3 ms of a single-image encode); larger batches fill the chip anyway.  Rounds 2-4 kept it opt-in: round 2 had seen run-to-run
# different bitstreams with kernels of two streams sharing CUs -- since traced, at ISA level, to a packed-FMA operand form
# (`op_sel` on src1: tools/ubench/pk_opsel_probe.hip, profiles/r04_ubench_pk_opsel_erratum_probe.txt) that the depthwise kernel no
# longer uses; the two pipeline groups of every batched call share CUs the same way.  Results do not depend on the option (same
# kernels, same inputs): tests/test_gpu_model.py::test_encode_is_stable_under_stream_concurrency.
SIDE_STREAM_MAX_PIXELS = 2 * 512 * 768


# ----------------------------------------------------------------------------------------------- parameter holders
class _Marker(nn.Module):
    """Parameter-less placeholder keeping list indices aligned with the reference (SetKey / CompresionStopFlag,
    lvae/models/common.py:48-66)."""
    def __init__(self, kind, key=None):
        super().__init__()
        self.kind, self.key = kind, key


class _MlpParams(nn.Module):
    def __init__(self, dim, hidden, out_dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, out_dim)


class CNXParams(nn.Module):
    """Parameters of one ConvNeXtBlockAdaLN (lvae/models/common.py:110-140): conv_dw, embedding_layer.1, mlp.fc1/fc2,
    gamma (1,C,1,1) initialised to 1e-6."""
    kind = 'cnx'

    def __init__(self, dim, kernel_size=7, mlp_ratio=2, embed_dim=EMBED_DIM):
        super().__init__()
        self.dim, self.kernel_size, self.hidden = dim, kernel_size, int(mlp_ratio * dim)
        self.conv_dw = nn.Conv2d(dim, dim, kernel_size=kernel_size, padding=(kernel_size - 1) // 2, groups=dim)
        self.embedding_layer = nn.Sequential(nn.Identity(), nn.Linear(embed_dim, 2 * dim), nn.Identity())
        self.mlp = _MlpParams(dim, self.hidden, dim)
        self.gamma = nn.Parameter(torch.full(size=(1, dim, 1, 1), fill_value=1e-6))


def _conv(cin, cout, k, stride=1, padding=0):
    c = nn.Conv2d(cin, cout, k, stride, padding)
    c.bias.data.mul_(0.0)          # get_conv(zero_bias=True), common.py:8-14
    return c


class DownParams(nn.Conv2d):
    """patch_downsample (common.py:29-30): conv kernel=stride=rate."""
    kind = 'down'

    def __init__(self, cin, cout, rate):
        super().__init__(cin, cout, rate, rate, 0)
        self.bias.data.mul_(0.0)
        self.rate = rate


class UpParams(nn.Sequential):
    """patch_upsample (common.py:33-38): conv1x1 to cout*rate^2 channels + PixelShuffle(rate)."""
    kind = 'up'

    def __init__(self, cin, cout, rate):
        super().__init__(_conv(cin, cout * rate * rate, 1), nn.Identity())
        self.cin, self.cout, self.rate = cin, cout, rate


class VRLVParams(nn.Module):
    """Parameters of one VRLVBlockBase (qarv/model.py:19-42)."""
    kind = 'vrlv'

    def __init__(self, width, zdim, enc_key, enc_width, kernel_size=7, mlp_ratio=2):
        super().__init__()
        self.width, self.zdim, self.enc_key, self.enc_width, self.kernel_size = width, zdim, enc_key, enc_width, kernel_size
        self.resnet_front = CNXParams(width, kernel_size, mlp_ratio)
        self.resnet_end = CNXParams(width, kernel_size, mlp_ratio)
        self.posterior0 = CNXParams(enc_width, kernel_size)
        self.posterior1 = CNXParams(width, kernel_size)
        self.posterior2 = CNXParams(width, kernel_size)
        self.post_merge = _conv(width + enc_width, width, 1)
        self.posterior = _conv(width, zdim, 3, 1, 1)
        self.z_proj = _conv(zdim, width, 1)
        self.prior = _conv(width, zdim * 2, 1)
        self.discrete_gaussian = DiscretizedGaussian(cdf_form='erf')
        self.is_latent_block = True


class _Encoder(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.enc_blocks = nn.ModuleList(blocks)


# ----------------------------------------------------------------------------------------------- launch plans
class _Packed(PackedWeights):
    """qarv layout: NHWC / GEMM-friendly weights, the lambda embedding and one AdaLN matrix for all blocks."""

    def __init__(self, model, device):
        super().__init__(model, device)
        self.adaln_off = {}
        f32 = dict(device=device, dtype=torch.float32)
        ws, bs = [], []
        total = 0
        put = self.put

        def cnx(p, m):
            nonlocal total
            C, k = m.dim, m.kernel_size
            put(p + '.dw_w', m.conv_dw.weight.reshape(C, k * k).t())            # [k*k][C]
            put(p + '.dw_b', m.conv_dw.bias)
            put(p + '.fc1_w', m.mlp.fc1.weight); put(p + '.fc1_b', m.mlp.fc1.bias)
            put(p + '.fc2_w', m.mlp.fc2.weight); put(p + '.fc2_b', m.mlp.fc2.bias)
            put(p + '.gamma', m.gamma.reshape(C))
            lin = m.embedding_layer[1]
            b = lin.bias.detach().clone().float()
            b[C:] += 1.0                       # second half is `scale`; the kernel consumes (1 + scale) (common.py:151-152)
            ws.append(lin.weight.detach().float()); bs.append(b)
            self.adaln_off[p] = total
            total += 2 * C

        for i, m in enumerate(model.encoder.enc_blocks):
            p = f'encoder.enc_blocks.{i}'
            if m.kind == 'cnx':
                cnx(p, m)
            elif m.kind == 'down' and m.rate == 4:
                put(p + '.w', m.weight.reshape(m.out_channels, -1).t())           # [48][Cout], k=(ci*4+i)*4+j
                put(p + '.b', m.bias)
            elif m.kind == 'down':
                put(p + '.w', m.weight.permute(0, 2, 3, 1).reshape(m.out_channels, -1))   # [Cout][(i,j,ci)]
                put(p + '.b', m.bias)
        for i, m in enumerate(model.dec_blocks):
            p = f'dec_blocks.{i}'
            if m.kind == 'cnx':
                cnx(p, m)
            elif m.kind == 'up':
                w = m[0].weight.reshape(m.cout * m.rate ** 2, m.cin)
                b = m[0].bias
                r2 = m.rate ** 2
                if m.cout > 3:      # NHWC pixel-shuffle store wants columns ordered (i, j, c)
                    w = w.reshape(m.cout, r2, m.cin).permute(1, 0, 2).reshape(r2 * m.cout, m.cin)
                    b = b.reshape(m.cout, r2).t().reshape(-1)
                else:               # the eval decode plan's raw NHWC store of the final conv: the same rows in that order (same bits per element)
                    put(p + '.w_raw', w.reshape(m.cout, r2, m.cin).permute(1, 0, 2).reshape(r2 * m.cout, m.cin))
                    put(p + '.b_raw', b.reshape(m.cout, r2).t().reshape(-1))
                put(p + '.w', w); put(p + '.b', b)
            elif m.kind == 'vrlv':
                for sub in ('resnet_front', 'resnet_end', 'posterior0', 'posterior1', 'posterior2'):
                    cnx(f'{p}.{sub}', getattr(m, sub))
                put(p + '.post_merge.w', m.post_merge.weight.reshape(m.width, -1)); put(p + '.post_merge.b', m.post_merge.bias)
                put(p + '.posterior.w', m.posterior.weight.permute(0, 2, 3, 1).reshape(m.zdim, -1))
                put(p + '.posterior.b', m.posterior.bias)
                put(p + '.z_proj.w', m.z_proj.weight.reshape(m.width, m.zdim)); put(p + '.z_proj.b', m.z_proj.bias)
                put(p + '.prior.w', m.prior.weight.reshape(2 * m.zdim, m.width)); put(p + '.prior.b', m.prior.bias)
        put('bias', model.bias.reshape(-1))
        put('lmb.0.w', model.lmb_embedding[0].weight); put('lmb.0.b', model.lmb_embedding[0].bias)
        put('lmb.2.w', model.lmb_embedding[2].weight); put('lmb.2.b', model.lmb_embedding[2].bias)
        put('adaln.w', torch.cat(ws, 0)); put('adaln.b', torch.cat(bs, 0))
        self.adaln_total = total
        self.adaln = torch.zeros(total, **f32)          # per-lambda (shift | 1+scale) vectors of all blocks
        self.emb_in = torch.zeros(EMBED_DIM, **f32)
        self.emb_h = torch.zeros(EMBED_DIM, **f32)
        self.emb = torch.zeros(EMBED_DIM, **f32)
        self.tab_cap, self.adaln_tab = 0, None          # per-image lambdas: [tab_cap][adaln_total] table (model._set_lmb with a sequence)


class _NetPlan(CodecPlan):
    """Shared recording helpers for the encode and decode plans."""
    lp_storage = use_mlp_sk = True

    def __init__(self, model, pk, B, vec=False):
        super().__init__(model, pk, B)
        # vec: one lambda PER IMAGE.  The depthwise launches then read image b's (shift | 1+scale) vectors from row b of a slab this plan
        # owns ([B][adaln_total], filled by load_lmb before a run) instead of the model-wide pk.adaln.  The slab is the plan's own because
        # plans are cached with their addresses baked in while a pipeline group's first image index is not part of the cache key
        self.vec = bool(vec)
        self.adaln_slab = torch.zeros(B * pk.adaln_total, dtype=torch.float32, device=pk.device) if vec else None
        self.prm_ptrs, self.zhat_ptrs = [], []  # per latent block: raw prior conv output / latent buffer (scratch may be re-grown)

    def load_lmb(self, table, start):
        """vec plans: rows start .. start + B of the model's per-image table -> this plan's slab, on the current stream (the stream the
        plan is about to run on: ordered behind the table's GEMVs by the caller, and behind this plan's previous run)."""
        n = self.pk.adaln_total
        self.adaln_slab.copy_(table[start * n:(start + self.B) * n], non_blocking=True)

    def dwln_add(self, fmt, p, x, y, H, W, C, k):
        """Record the depthwise + LayerNorm + AdaLN launch of block p: lvae_dwconv_ln_<fmt> with the model-wide vectors, its _v form with
        the slab's."""
        pk = self.pk
        off = pk.adaln_off[p]
        if self.vec:
            self.add(getattr(self.lib, f'lvae_dwconv_ln_{fmt}_v'), (x, pk.p(p + '.dw_w'), pk.p(p + '.dw_b'), ptr(self.adaln_slab, off),
                                                                   ptr(self.adaln_slab, off + C), y, self.B, H, W, C, k, pk.adaln_total), p + '.dwln')
        else:
            self.add(getattr(self.lib, f'lvae_dwconv_ln_{fmt}'), (x, pk.p(p + '.dw_w'), pk.p(p + '.dw_b'), None, None, ptr(pk.adaln, off),
                                                                 ptr(pk.adaln, off + C), y, self.B, H, W, C, k), p + '.dwln')

    def cnx(self, p, m, x, out, H, W):
        """ConvNeXtBlockAdaLN (common.py:142-161).  The hidden-map scratch is sized at every block, also where the MLP runs fused: the
        encoder's first (largest) blocks then size it for the whole plan."""
        self.buf(self.sname('hid'), self.B * H * W * m.hidden, self.adt)
        super().cnx(p, m, x, out, H, W)

    def upsample(self, p, m, x, out, H, W, raw=False):
        """raw (final conv only): the launch of the ST_IMAGE store with the raw NHWC fp32 store of the pre-clamp output instead."""
        pk = self.pk
        M = self.B * H * W
        final = m.cout <= 3
        if raw:
            assert final
            self.gemm(A0=x, K0=m.cin, M=M, N=m.cout * m.rate ** 2, Wt=pk.p(p + '.w_raw'), bias=pk.p(p + '.b_raw'), out=out,
                      store=_native.ST_SHUFFLE, r=m.rate, H=H, W=W, out_bf16=0, label=p + '.up_raw')
            return
        self.gemm(A0=x, K0=m.cin, M=M, N=m.cout * m.rate ** 2, Wt=pk.p(p + '.w'), bias=pk.p(p + '.b'), out=out,
                  store=_native.ST_IMAGE if final else _native.ST_SHUFFLE, r=m.rate, H=H, W=W, label=p + '.up')

    def prior(self, p, m, f, H, W, side_head=False):
        """transform_prior (qarv/model.py:44-54) + build_indexes (:106/:112). Returns pm buffer."""
        pk, lib, B = self.pk, self.lib, self.B
        M, z = B * H * W, m.zdim
        self.cnx(p + '.resnet_front', m.resnet_front, f, f, H, W)
        if side_head:          # encoder: the prior head is off the critical path until quantize -- it runs beside posterior1 / post_merge
            self.fork(p + '.fork_prior')
            self.side_begin()
        prm = self.buf('prm', M * 2 * z)
        # (split-K launches leave their reduce pass to the index kernel: one launch less per latent block on both chains, same bits)
        planes = self.gemm(A0=f, K0=m.width, M=M, N=2 * z, Wt=pk.p(p + '.prior.w'), bias=pk.p(p + '.prior.b'),
                           out=prm.data_ptr(), out_bf16=0, defer_reduce=(self.prec != 3 and self.DEFER_HEAD_REDUCE), label=p + '.prior')
        pm = self.new(M * z)
        self.pm_bufs.append(pm)
        self.prm_ptrs.append(prm.data_ptr())
        self.prm_bufs.append(prm)
        ioff = sum(s[0] * s[1] for s in self.lat_shapes) * B
        self.lat_shapes.append((z, H * W))
        self.idx_off.append(ioff)
        if planes is not None:
            self.add(lib.lvae_prior_index_sk_f32, (planes[0], planes[1], pk.p(p + '.prior.b'), prm.data_ptr(), pm.data_ptr(), ptr(self.idx_all, ioff),
                                                   pk.scale_table.data_ptr(), pk.scale_table.numel(), pk.scale_bound, B, H * W, z, self.status_ptr()),
                     p + '.prior_index')
        else:
            self.add(lib.lvae_prior_index_f32, (prm.data_ptr(), pm.data_ptr(), ptr(self.idx_all, ioff), pk.scale_table.data_ptr(),
                                                pk.scale_table.numel(), pk.scale_bound, B, H * W, z, self.status_ptr()), p + '.prior_index')
        self.side_end()
        return pm, ioff

    def fuse_and_end(self, p, m, f, zhat, H, W):
        """fuse_feature_and_z + resnet_end (qarv/model.py:72-75,117-118)."""
        pk = self.pk
        M = self.B * H * W
        self.gemm(A0=zhat, K0=m.zdim, M=M, N=m.width, Wt=pk.p(p + '.z_proj.w'), bias=pk.p(p + '.z_proj.b'), res=f,
                  ldres=m.width, out=f, epi=_native.EPI_RES, a_bf16=0, label=p + '.z_proj')
        self.cnx(p + '.resnet_end', m.resnet_end, f, f, H, W)

    def alloc_latent_io(self, nH, nW, host=True):
        """Device symbol / index buffers of every latent block; host=True adds the coder's pinned host copies."""
        B = self.B
        total, s = 0, 1
        # latent resolution per block follows the top-down path: starts at (nH,nW), doubles at each upsample
        for m in self.model.dec_blocks:
            if m.kind == 'vrlv':
                total += m.zdim * nH * s * nW * s
            elif m.kind == 'up':
                s *= m.rate
            elif m.kind == 'stop':
                break
        self.alloc_symbols(total * B, host)


class _EncPlan(_NetPlan):
    """forward_end2end(mode='compress') (qarv/model.py:294-315) for B images of size HxW."""

    def __init__(self, model, pk, B, H, W, with_bits=False, chan_bits=False, pos_bits=False, vec=False):
        """with_bits ('encb'): each block's rate per image in `nats` ([block][image], accumulated); chan_bits ('ence', the encoder half of
        forward()): per image and channel in `kl_chan` (fp64 [L][B][z_l] at chan_off[l], lvae_gaussian_nll_chan_f32: deterministic);
        pos_bits ('encp', rate_map): per position in `pos_bufs` (one fp64 (B, h, w) buffer per block, lvae_gaussian_nll_pos_f32 where
        chan_bits has its kernel -- launched by CodecBase._run_with_pos at qcuts, the plan records the 'enc' launches)."""
        super().__init__(model, pk, B, vec)
        lib = self.lib
        self.im = self.new(B * 3 * H * W)
        if getattr(model, 'side_streams', False):
            self.enable_side_stream()
        # small plans: every block's posterior0 and prior head beside the main branch (pure launch latency there)
        small_side = self.side_stream is not None and B * H * W <= SIDE_STREAM_MAX_PIXELS
        # every plan: posterior0 of the stride-8 / 16 latent blocks -- a ConvNeXt block on the ENCODER feature alone (qarv/model.py:58-59),
        # the only large launches of the encode that do not sit on its dependency chain -- is hoisted to the point where the bottom-up
        # path leaves stride 16 and runs on the side stream under the stride-32 / 64 stages of both paths, whose launches (M = 96 ... 384
        # rows per image) leave the chip almost empty (round 5; same kernels, same inputs, same bits)
        hoisted = {}                                    # dec_blocks index -> buffer holding posterior0's output
        self.alloc_latent_io(H // 64, W // 64, host=not (chan_bits or pos_bits))         # forward()'s symbols never leave the device
        self.nats = self.new(model.num_latents * B, torch.float64) if with_bits else None   # [block][image] sum(-ln P)
        if chan_bits:
            self.kl_chan = self.new(B * sum(m.zdim for m in model.dec_blocks if m.kind == 'vrlv'), torch.float64)
            self.chan_off = []
        feats = {}
        tapped = set()
        h, w = H, W
        x = None
        for i, m in enumerate(model.encoder.enc_blocks):
            p = f'encoder.enc_blocks.{i}'
            if m.kind == 'down' and m.rate == 4:
                h, w = h // 4, w // 4
                x = self.new(B * h * w * m.out_channels, self.adt)
                self.add(lib.lvae_stem_bf16 if self.lp else lib.lvae_stem_f32, (self.im.data_ptr(), pk.p(p + '.w'), pk.p(p + '.b'), x.data_ptr(), B, H, W,
                                             m.out_channels, model.im_shift, model.im_scale, self.status_ptr()), p + '.stem')
                self.flops += 2 * B * h * w * m.out_channels * 48
            elif m.kind == 'down':
                if self.side_stream is not None and (h, w) == (H // 16, W // 16) and not hoisted:
                    self._hoist_posterior0(model, feats, hoisted, H, W)
                h, w = h // 2, w // 2
                nx = self.new(B * h * w * m.out_channels, self.adt)
                self.gemm(A0=x.data_ptr(), K0=m.in_channels, M=B * h * w, N=m.out_channels, K=4 * m.in_channels,
                          Wt=pk.p(p + '.w'), bias=pk.p(p + '.b'), out=nx.data_ptr(), a_mode=_native.A_PATCH2, H=h, W=w,
                          label=p + '.down')
                x = nx
            elif m.kind == 'cnx':
                if x.data_ptr() in tapped:               # feature was tapped by SetKey: keep it, write elsewhere
                    nx = self.new(x.numel(), self.adt)
                    self.cnx(p, m, x.data_ptr(), nx.data_ptr(), h, w)
                    x = nx
                else:
                    self.cnx(p, m, x.data_ptr(), x.data_ptr(), h, w)
            elif m.kind == 'key':
                feats[m.key] = (x, h, w)
                tapped.add(x.data_ptr())
        # top-down path
        h, w = H // 64, W // 64
        width = model.dec_blocks[0].width
        f = self.new(B * h * w * width, self.adt)
        self.add(lib.lvae_bias_expand_bf16 if self.lp else lib.lvae_bias_expand_f32, (pk.p('bias'), f.data_ptr(), B * h * w, width), 'bias')
        for i, m in enumerate(model.dec_blocks):
            p = f'dec_blocks.{i}'
            if m.kind == 'vrlv':
                M, z = B * h * w, m.zdim
                ef, eh, ew = feats[m.enc_key]
                assert (eh, ew) == (h, w)
                g = self.buf('post_g', M * m.width, self.adt)
                mg = self.buf('post_m', M * m.width, self.adt)
                # posterior0 works on the ENCODER feature only (qarv/model.py:56-70): hoisted (above), or -- small plans -- on the side
                # stream beside resnet_front (and the prior head beside posterior1), or in line; side work is joined before post_merge
                if i in hoisted:
                    e = hoisted[i]
                else:
                    e = self.buf('post_e', M * m.enc_width, self.adt)
                    if small_side:
                        self.fork(p + '.fork_post0')
                        self.side_begin()
                    self.cnx(p + '.posterior0', m.posterior0, ef.data_ptr(), e.data_ptr(), h, w)
                    self.side_end()
                # (prior heads on the side stream in EVERY plan were measured too: +0.27 ms per encode at batch 8, profiles/r05_ab_encode_side_stream.txt)
                head_side = small_side
                pm, ioff = self.prior(p, m, f.data_ptr(), h, w, side_head=head_side)
                self.cnx(p + '.posterior1', m.posterior1, f.data_ptr(), g.data_ptr(), h, w)
                if head_side or i in hoisted:
                    self.join(p + '.join')
                self.gemm(A0=g.data_ptr(), K0=m.width, A1=e.data_ptr(), K1=m.enc_width, lda1=m.enc_width, M=M, N=m.width,
                          Wt=pk.p(p + '.post_merge.w'), bias=pk.p(p + '.post_merge.b'), out=mg.data_ptr(),
                          label=p + '.post_merge')
                self.cnx(p + '.posterior2', m.posterior2, mg.data_ptr(), mg.data_ptr(), h, w)
                qm = self.buf('qm', M * z)
                planes = self.gemm(A0=mg.data_ptr(), K0=m.width, M=M, N=z, K=9 * m.width, Wt=pk.p(p + '.posterior.w'),
                                   bias=pk.p(p + '.posterior.b'), out=qm.data_ptr(), a_mode=_native.A_CONV3, H=h, W=w, out_bf16=0,
                                   defer_reduce=(self.prec != 3 and self.DEFER_HEAD_REDUCE), label=p + '.posterior')
                zhat = self.buf('zhat', M * z)
                self.qm_bufs.append(qm); self.zhat_bufs.append(zhat); self.zhat_ld.append(z)
                self.sym_off.append(ioff)
                if planes:      # split-K planes of the posterior head: summed (slice order, + bias) by the quantize launch itself
                    self.add(lib.lvae_quantize_sk_f32, (planes[0], planes[1], pk.p(p + '.posterior.b'), qm.data_ptr(), pm.data_ptr(),
                                                        ptr(self.sym_all, ioff), zhat.data_ptr(), B, h * w, z, z, self.status_ptr()), p + '.quantize')
                else:
                    self.add(lib.lvae_quantize_f32, (qm.data_ptr(), pm.data_ptr(), ptr(self.sym_all, ioff), zhat.data_ptr(),
                                                     B, h * w, z, z, self.status_ptr()), p + '.quantize')
                self.qcuts.append(len(self.ops))        # this block's symbols and indexes are final from here on
                if pos_bits:
                    self.lat_hw.append((h, w))
                if with_bits:       # eval-mode likelihood of the quantised latent (qarv/model.py:95-96), prm still holds this block
                    li = len(self.sym_off) - 1
                    self.add(lib.lvae_gaussian_nll_f32, (self.bufs['prm'].data_ptr(), ptr(self.sym_all, ioff), ptr(self.nats, li * B),
                                                         pk.scale_bound, B, h * w, z, 0), p + '.nll')
                if chan_bits:
                    co = B * sum(zz for zz, _ in self.lat_shapes[:-1])
                    self.chan_off.append(co)
                    self.add(lib.lvae_gaussian_nll_chan_f32, (self.bufs['prm'].data_ptr(), ptr(self.sym_all, ioff), ptr(self.kl_chan, co),
                                                              pk.scale_bound, B, h * w, z, 0), p + '.nll_chan')
                self.fuse_and_end(p, m, f.data_ptr(), zhat.data_ptr(), h, w)
            elif m.kind == 'cnx':
                self.cnx(p, m, f.data_ptr(), f.data_ptr(), h, w)
            elif m.kind == 'up':
                nf = self.new(B * h * w * m.rate ** 2 * m.cout, self.adt)
                self.upsample(p, m, f.data_ptr(), nf.data_ptr(), h, w)
                f = nf
                h, w = h * m.rate, w * m.rate
            elif m.kind == 'stop':
                break                                                     # qarv/model.py:310-312
        if pos_bits:
            self.alloc_pos()

    def _hoist_posterior0(self, model, feats, hoisted, H, W):
        """Record posterior0 of every latent block whose encoder feature is already there (strides 8 and 16) on the side stream,
        the blocks the top-down path reaches first (stride 16) first."""
        todo, s = [], 1
        for i, m in enumerate(model.dec_blocks):
            if m.kind == 'vrlv' and m.enc_key in feats:
                todo.append((i, m))
            elif m.kind == 'stop':
                break
        if not todo:
            return
        self.fork('hoist.fork')
        self.side_begin()
        for i, m in todo:                               # dec_blocks order = the order the top-down path needs them in
            ef, eh, ew = feats[m.enc_key]
            e = self.new(self.B * eh * ew * m.enc_width, self.adt)
            self.cnx(f'dec_blocks.{i}.posterior0', m.posterior0, ef.data_ptr(), e.data_ptr(), eh, ew)
            hoisted[i] = e
        self.side_end()


class _DecPlan(_NetPlan):
    """decompress() (qarv/model.py:531-557): 9 GPU segments separated by host rANS decodes.  evaluate ('evald', the decoder half of
    forward()): the final conv stored raw (NHWC fp32 [B*H*W][3], `x_raw`) and lvae_rd_image_f32 against `im` -> `out` (im_hat), `rd_sums`
    (fp64 [B][2]: sum (x_hat - x_target)^2, sum (im_hat - im)^2)."""

    def __init__(self, model, pk, B, nH, nW, evaluate=False, vec=False):
        super().__init__(model, pk, B, vec)
        lib = self.lib
        self.alloc_latent_io(nH, nW, host=not evaluate)
        h, w = nH, nW
        width = model.dec_blocks[0].width
        f = self.new(B * h * w * width, self.adt)
        self.add(lib.lvae_bias_expand_bf16 if self.lp else lib.lvae_bias_expand_f32, (pk.p('bias'), f.data_ptr(), B * h * w, width), 'bias')
        self.out = None
        for i, m in enumerate(model.dec_blocks):
            p = f'dec_blocks.{i}'
            if m.kind == 'vrlv':
                M, z = B * h * w, m.zdim
                pm, ioff = self.prior(p, m, f.data_ptr(), h, w)
                self.cuts.append(len(self.ops))
                self.sym_off.append(ioff)
                self.lat_hw.append((h, w))
                zhat = self.buf('zhat', M * z)
                self.zhat_ptrs.append(zhat.data_ptr())
                self.zhat_bufs.append(zhat)
                self.add(lib.lvae_dequantize_f32, (ptr(self.sym_all, ioff), pm.data_ptr(), zhat.data_ptr(), B, h * w, z, z),
                         p + '.dequantize')
                self.fuse_and_end(p, m, f.data_ptr(), zhat.data_ptr(), h, w)
            elif m.kind == 'cnx':
                self.cnx(p, m, f.data_ptr(), f.data_ptr(), h, w)
            elif m.kind == 'up':
                final = m.cout <= 3
                nf = self.new(B * h * w * m.rate ** 2 * m.cout, torch.float32 if final else self.adt)
                self.upsample(p, m, f.data_ptr(), nf.data_ptr(), h, w, raw=final and evaluate)
                f = nf
                h, w = h * m.rate, w * m.rate
                if final and evaluate:
                    self.x_raw, self.im, self.rd_sums = nf, self.new(B * 3 * h * w), self.new(B * 2, torch.float64)
                    self.rd_ws = self.new(B * _native.EVAL_CHUNKS * 2, torch.float64)     # per-chunk partials of lvae_rd_image_f32
                    im_hat = self.new(B * 3 * h * w)
                    self.add(lib.lvae_rd_image_f32, (nf.data_ptr(), self.im.data_ptr(), im_hat.data_ptr(), self.rd_sums.data_ptr(),
                                                     self.rd_ws.data_ptr(), B, h, w,
                                                     self.status_ptr()), 'rd_image')
                    self.out = im_hat.view(B, m.cout, h, w)
                elif final:
                    self.out = nf.view(B, m.cout, h, w)
        assert self.out is not None


# ----------------------------------------------------------------------------------------------- the model
class VariableRateLossyVAE(CodecBase):
    log2_e = math.log2(math.e)
    MAX_LMB = 8192

    def __init__(self, config: dict):
        super().__init__()
        self.encoder = _Encoder(config.pop('enc_blocks'))
        self.dec_blocks = nn.ModuleList(config.pop('dec_blocks'))
        width = self.dec_blocks[0].width
        self.bias = nn.Parameter(torch.zeros(1, width, 1, 1))
        self.num_latents = len([b for b in self.dec_blocks if getattr(b, 'is_latent_block', False)])

        _low, _high = config['lmb_range']
        self.lmb_range = (float(_low), float(_high))
        self.default_lmb = self.lmb_range[1]
        self.lmb_embed_dim = config['lmb_embed_dim']
        self.lmb_embedding = nn.Sequential(
            nn.Linear(self.lmb_embed_dim[0], self.lmb_embed_dim[1]), nn.GELU(),
            nn.Linear(self.lmb_embed_dim[1], self.lmb_embed_dim[1]))
        self._sin_period = config['sin_period']

        self.im_shift = float(config['im_shift'])
        self.im_scale = float(config['im_scale'])
        self.max_stride = config['max_stride']
        self.register_buffer('_dummy', torch.zeros(1), persistent=False)
        self.compressing = False
        self._init_codec_base()
        self._cur_lmb = None
        self._cur_lmbs = None             # tuple of fp32 lambdas whose vectors the per-image table holds
        self.timing = {} if os.environ.get('LVAE_TIMING') else None      # host-side phase timers (debug)
        # independent encoder branches on a second HIP stream (see SIDE_STREAM_MAX_PIXELS, _EncPlan); False gives the same bits
        self.side_streams = True

    # ---- helpers
    def _latent_blocks(self):
        return [b for b in self.dec_blocks if getattr(b, 'is_latent_block', False)]

    def _invalidate(self):
        super()._invalidate()
        self._cur_lmb = self._cur_lmbs = None

    def _build_packed(self, dev):
        return _Packed(self, dev)

    def _lmb_features(self, lmb):
        """Sinusoidal features of one lambda (qarv/model.py:266-287) on the host, fp32: 128 cos + 128 sin."""
        s = np.log(np.float32(lmb)) * np.float32(self._sin_period) / np.float32(math.log(self.MAX_LMB))
        dim = self.lmb_embed_dim[0]
        expo = np.linspace(0, 1, dim // 2, dtype=np.float32)
        freqs = np.power(np.float32(self._sin_period), -expo).astype(np.float32)
        args = (np.float32(s) * freqs).astype(np.float32)
        return np.concatenate([np.cos(args), np.sin(args)]).astype(np.float32)

    def _lmb_arg(self, lmb, B, default=True):
        """The `lmb` argument of the batch interfaces -> a float (one lambda for the call: None, a number, a one-element tensor, or B
        equal values) or a list of B fp32-valued floats (one per image).  default=False (lambdas read from stream headers): values pass
        through as written, a zero is not replaced by default_lmb."""
        if lmb is None:
            return self.default_lmb
        if isinstance(lmb, torch.Tensor):
            lmb = lmb.item() if lmb.numel() == 1 and lmb.dim() == 0 else lmb.detach().cpu().reshape(-1).tolist()
        elif isinstance(lmb, np.ndarray):
            lmb = lmb.reshape(-1).tolist()
        if isinstance(lmb, (list, tuple)):
            assert len(lmb) == B, f'{len(lmb)} lambdas for a batch of {B}'
            vals = [float(np.float32(v)) for v in lmb]
            if all(v == vals[0] for v in vals):
                return (vals[0] or self.default_lmb) if default else vals[0]
            return vals
        return (lmb or self.default_lmb) if default else lmb

    def _set_lmb(self, lmb):
        """_get_lmb_embedding (qarv/model.py:266-287) + every block's AdaLN embedding_layer (common.py:150-151), once
        per lambda: sinusoidal features on the host (128 cos + 128 sin), then three GEMV launches.  A list / tuple of lambdas fills
        row i of the per-image table pk.adaln_tab with lambda i's vectors instead (three batched launches; row i has the bits the
        single-lambda launches give for lambda i, so streams coded from the table decode against pk.adaln and the other way round)."""
        pk = self._prepare()
        many = isinstance(lmb, (list, tuple))
        key = tuple(float(np.float32(v)) for v in lmb) if many else float(np.float32(lmb))
        if (self._cur_lmbs if many else self._cur_lmb) == key:
            return
        if torch.cuda.current_device() != pk.adaln.device.index:   # raw launches below: make the model's GPU the current one
            with torch.cuda.device(pk.adaln.device):
                return self._set_lmb(lmb)
        dim, hid = self.lmb_embed_dim
        lib = _native.lib()
        st = torch.cuda.current_stream(pk.adaln.device).cuda_stream
        if many:
            n = len(key)
            if n > pk.tab_cap:
                cap = max(8, n)
                f32 = dict(device=pk.adaln.device, dtype=torch.float32)
                pk.tab_in, pk.tab_h, pk.tab_emb = torch.zeros(cap * dim, **f32), torch.zeros(cap * hid, **f32), torch.zeros(cap * hid, **f32)
                pk.adaln_tab, pk.tab_cap = torch.zeros(cap * pk.adaln_total, **f32), cap
            pk.tab_in[:n * dim].copy_(torch.from_numpy(np.concatenate([self._lmb_features(v) for v in key])))
            _native.check(lib.lvae_gemv_batch_f32(pk.p('lmb.0.w'), pk.p('lmb.0.b'), pk.tab_in.data_ptr(), pk.tab_h.data_ptr(), hid, dim, n, 0, 1, st),
                          'gemv lmb.0')
            _native.check(lib.lvae_gemv_batch_f32(pk.p('lmb.2.w'), pk.p('lmb.2.b'), pk.tab_h.data_ptr(), pk.tab_emb.data_ptr(), hid, hid, n, 0, 0, st),
                          'gemv lmb.2')
            _native.check(lib.lvae_gemv_batch_f32(pk.p('adaln.w'), pk.p('adaln.b'), pk.tab_emb.data_ptr(), pk.adaln_tab.data_ptr(), pk.adaln_total,
                                                  hid, n, 1, 0, st), 'gemv adaln')
            self._cur_lmbs = key
            return
        pk.emb_in.copy_(torch.from_numpy(self._lmb_features(key)))
        _native.check(lib.lvae_gemv_f32(pk.p('lmb.0.w'), pk.p('lmb.0.b'), pk.emb_in.data_ptr(), pk.emb_h.data_ptr(),
                                        hid, dim, 0, 1, st), 'gemv lmb.0')
        _native.check(lib.lvae_gemv_f32(pk.p('lmb.2.w'), pk.p('lmb.2.b'), pk.emb_h.data_ptr(), pk.emb.data_ptr(),
                                        hid, hid, 0, 0, st), 'gemv lmb.2')
        _native.check(lib.lvae_gemv_f32(pk.p('adaln.w'), pk.p('adaln.b'), pk.emb.data_ptr(), pk.adaln.data_ptr(),
                                        pk.adaln_total, hid, 1, 0, st), 'gemv adaln')
        self._cur_lmb = key

    def _use_lmb(self, pl, start=0):
        """Before a plan runs on the current stream: a plan with per-image lambdas gets rows start .. start + B of the table."""
        if pl.vec:
            pl.load_lmb(self._packed.adaln_tab, start)

    def _plan_key(self, kind, B, a, b, group=0, vec=False):
        return (kind, B, a, b, group, bool(getattr(self, 'side_streams', False)) and kind != 'dec', self._prec) + (('vec',) if vec else ())

    def _build_plan(self, kind, B, a, b, group=0, vec=False):
        if kind in ('enc', 'encb', 'ence', 'encp'):
            return _EncPlan(self, self._packed, B, a, b, with_bits=(kind == 'encb'), chan_bits=(kind == 'ence'), pos_bits=(kind == 'encp'), vec=vec)
        return _DecPlan(self, self._packed, B, a, b, evaluate=(kind == 'evald'), vec=vec)

    # ---- reference API
    def compress_mode(self, mode=True):
        """qarv/model.py:509-514: (re)build the CDF tables of every latent block."""
        if mode:
            self._build_cdf_tables(lambda dg: dg.update())
            self._log_precision()
        self.compressing = mode

    @torch.no_grad()
    @on_model_device
    def compress_batch(self, im, lmb=None, u8=None):
        """Encode a (B,3,H,W) batch -> list of B byte strings.  lmb: None (default_lmb), a number, or a sequence / 1-D tensor of B
        lambdas, one per image; string b is identical to `compress(im[b:b+1], lmb[b])` and carries its own lambda in its header.
        u8 (compress_images): a utils.image.U8Batch in place of `im` (then None) -- 8-bit images already on the device, converted by
        lvae_image_u8_to_f32 straight into each group's plan input."""
        if u8 is None:
            assert im.dim() == 4 and im.shape[1] == 3 and not im.requires_grad
        B, _, H, W = u8.shape if u8 is not None else im.shape
        assert (H % self.max_stride == 0) and (W % self.max_stride == 0), f'{(B, 3, H, W)=}'
        lmb = self._lmb_arg(lmb, B)
        vec = isinstance(lmb, list)
        self._prepare()
        self._set_lmb(lmb)
        tables = self._dg().host_tables()
        shape_str = struct.pack('3H', 1, H // self.max_stride, W // self.max_stride)
        headers = [struct.pack('f', v) + shape_str for v in (lmb if vec else [lmb] * B)]
        groups = self._groups(B, 'enc')
        nthreads = self._coder_threads_per_group(len(groups))
        T = self.timing

        def encode_group(g, start, n, stream):
            pl = self._plan('enc', n, H, W, g, vec=vec)
            t0 = time.time()
            self._load_input(pl.im.view(n, 3, H, W), im, u8, start, n)
            self._use_lmb(pl, start)
            if self.native_group_loops:
                # the loop below as ONE foreign call (csrc/plan_runtime.cpp::lvae_encode_blocks): no interpreter between the launches,
                # the event waits and the coder calls, and no interpreter lock shared with the other group's thread
                per_block = self._encode_group_native(pl, pl.qcuts, pl.sym_off, n, tables, nthreads, stream, T)
                nl = len(pl.lat_shapes)
                assert nl == self.num_latents
                strings = [per_block[li][b] for b in range(n) for li in range(nl)]
                res = [headers[start + b] + coding.pack_byte_strings(strings[b * nl:(b + 1) * nl]) for b in range(n)]
                if T is not None:
                    T['enc_group_total'] = T.get('enc_group_total', 0) + time.time() - t0
                return res
            # Progressive hand-over: after each latent block's quantize launch, its symbols / indexes are copied to pinned host
            # memory and an event is recorded; the host then entropy-codes block i while the GPU is still computing blocks > i
            # (only the last block's streams are coded after the GPU has finished).
            lo, evs = 0, []
            for li, cut in enumerate(pl.qcuts):
                pl.run(lo, cut, stream=stream.cuda_stream)
                lo = cut
                z, hw = pl.lat_shapes[li]
                o, cnt = pl.sym_off[li], n * z * hw
                pl.sym_host[o:o + cnt].copy_(pl.sym_all[o:o + cnt], non_blocking=True)
                pl.idx_host[o:o + cnt].copy_(pl.idx_all[o:o + cnt], non_blocking=True)
                if li == len(pl.qcuts) - 1:
                    pl.fetch_status()
                ev = torch.cuda.Event()
                ev.record(stream)
                evs.append(ev)
            # (the launches after the last quantize -- z_proj / resnet_end of the last latent block, which the reference also runs
            # before it meets CompresionStopFlag -- do not influence the bitstream and are skipped)
            t1 = time.time()
            nl = len(pl.lat_shapes)
            per_block, t_wait = [], 0.0
            evs[-1].synchronize()       # (debug loop: the status word is read once, behind the last block -- no progressive hand-over)
            pl.raise_if_flagged(where='while encoding')
            for li, ev in enumerate(evs):
                tw = time.time()
                ev.synchronize()
                t_wait += time.time() - tw
                z, hw = pl.lat_shapes[li]
                o = pl.sym_off[li]
                sv = [pl.sym_np[o + b * z * hw:o + (b + 1) * z * hw] for b in range(n)]
                iv = [pl.idx_np[o + b * z * hw:o + (b + 1) * z * hw] for b in range(n)]
                per_block.append(rans_encode_streams(tables, sv, iv, nthreads))
            tw = time.time()
            stream.synchronize()
            t2 = t1 + t_wait + (time.time() - tw)
            strings = [per_block[li][b] for b in range(n) for li in range(nl)]
            t_gpu_done = time.time()
            assert nl == self.num_latents
            res = [headers[start + b] + coding.pack_byte_strings(strings[b * nl:(b + 1) * nl]) for b in range(n)]
            if T is not None:
                t3 = time.time()
                T['enc_launch'] = T.get('enc_launch', 0) + t1 - t0
                T['enc_gpu_wait'] = T.get('enc_gpu_wait', 0) + t2 - t1
                T['enc_rans'] = T.get('enc_rans', 0) + t3 - t2
                T['enc_last_wait'] = T.get('enc_last_wait', 0) + t_gpu_done - tw          # final stream.synchronize()
                T['enc_after_gpu'] = T.get('enc_after_gpu', 0) + t3 - t_gpu_done           # container packing after the GPU is done
                T['enc_group_total'] = T.get('enc_group_total', 0) + t3 - t0
            return res

        out = []
        for part in self._run_groups(encode_group, groups):
            out += part
        return out

    @torch.no_grad()
    def compress(self, im, lmb=None):
        """qarv/model.py:516-529 (single image)."""
        assert im.shape[0] == 1, f'Right now only support a single image, got {im.shape=}'
        return self.compress_batch(im, lmb)[0]

    @torch.no_grad()
    @on_model_device
    def decompress_batch(self, strings):
        """Decode a list of byte strings that share the latent shape (their lambdas may differ) -> (B,3,H,W) tensor in [0,1]; row b
        equals `decompress(strings[b])`."""
        t_entry = time.time()
        B = len(strings)
        heads = [struct.unpack('f', s[:4]) + struct.unpack('3H', s[4:10]) for s in strings]
        _, nB, nH, nW = heads[0]
        assert nB == 1 and all(h[1:] == heads[0][1:] for h in heads), 'batch must share the latent shape'
        lmb = self._lmb_arg([h[0] for h in heads], B, default=False)
        vec = isinstance(lmb, list)
        if not all(isinstance(s, bytes) for s in strings):
            strings = [bytes(s) for s in strings]
        lv = None if self.native_group_loops else [coding.unpack_byte_string(s[10:]) for s in strings]

        def stream_views(start, n, nb):
            """[image][block] -> (container, offset, length): the container's payloads (utils/coding.py: 'B' count, count x 'I' lengths,
            payloads) as views -- the native decode loop reads them in place, nothing is sliced out (2.4 MB of copies per batch of 8)."""
            out = []
            for b in range(n):
                s = strings[start + b]
                num = s[10]
                lengths = struct.unpack_from(f'{num}I', s, 11)
                o = 11 + 4 * num
                assert num == nb, f'expected {nb} strings per image'
                assert sum(lengths) == len(s) - o, f'{sum(lengths)=} should equal to {len(s) - o=}'
                v = []
                for ln in lengths:
                    v.append((s, o, ln))
                    o += ln
                out.append(v)
            return out
        t_a = time.time()
        self._prepare()
        self._set_lmb(lmb)
        tables = self._dg().host_tables()
        groups = self._groups(B, 'dec')
        nthreads = self._coder_threads_per_group(len(groups))
        T = self.timing
        out = torch.empty(B, 3, nH * self.max_stride, nW * self.max_stride, device=self._dummy.device)
        t_b = time.time()
        if T is not None:
            T['dec_head_parse'] = T.get('dec_head_parse', 0) + t_a - t_entry
            T['dec_head_setup'] = T.get('dec_head_setup', 0) + t_b - t_a

        def decode_group(g, start, n, stream):
            if T is not None:
                T['dec_head_thread'] = T.get('dec_head_thread', 0) + time.time() - t_b          # submit -> the group's thread runs
            pl = self._plan('dec', n, nH, nW, g, vec=vec)
            self._use_lmb(pl, start)
            if T is not None:
                T['dec_head'] = T.get('dec_head', 0) + time.time() - t_entry                    # entry -> this group's first launch
            if self.native_group_loops:
                # the loop below as ONE foreign call (csrc/plan_runtime.cpp::lvae_decode_blocks)
                self._decode_group_native(pl, pl.cuts, pl.idx_off, n, lambda: stream_views(start, n, len(pl.cuts)), tables, nthreads, stream, T)
                out[start:start + n].copy_(pl.out, non_blocking=True)
                return None
            assert all(len(lv[start + b]) == len(pl.cuts) for b in range(n)), f'expected {len(pl.cuts)} strings per image'
            self._decode_group_loop(pl, n, lv[start:start + n], tables, nthreads, stream, T)
            out[start:start + n].copy_(pl.out, non_blocking=True)
            return None

        if T is not None:
            t_g = time.time()
        self._run_groups(decode_group, groups)
        self._check_decoded(groups, lambda g, n: self._plan('dec', n, nH, nW, g, vec=vec))
        if T is not None:
            T['dec_groups_total'] = T.get('dec_groups_total', 0) + time.time() - t_g
            T['dec_calls'] = T.get('dec_calls', 0) + 1
        return out

    variable_rate = True

    def _pack_blob(self, body, size):
        return struct.pack('2H', *size) + body

    def _unpack_blob(self, blob):
        return blob[4:], struct.unpack('2H', blob[:4]), bytes(blob[8:14])         # key: the 3H latent shape behind the lambda

    def _blob_lmb(self, blob):
        return struct.unpack('f', blob[4:8])[0]

    @torch.no_grad()
    def compress_file(self, img_path, output_path, lmb=None):
        """qarv/model.py:559-570."""
        self._compress_to_files([img_path], [output_path], lmb=lmb)

    @torch.no_grad()
    def compress_files(self, img_paths, output_paths, lmb=None, images=None):
        """Batched compress_file: images whose PADDED sizes agree are coded by one compress_batch call (GPU work batched, the B x 9
        rANS streams coded in parallel); every output file is byte-identical to what compress_file writes for that image.  lmb: one
        lambda, or one per file (a sequence).  `images`: the files' contents, already decoded (PIL images or uint8 tensors)."""
        self._compress_to_files(images if images is not None else list(img_paths), output_paths, lmb=lmb)

    @torch.no_grad()
    def compress_to_target(self, im, target_bytes, n_probe=8, max_rounds=50, tol=1, verbose=False):
        """Rate targeting for ONE image (1,3,H,W): a multi-section search over lambda in log space (lvae/utils/rate_search.py).  Each
        round encodes n_probe copies of the image in ONE compress_batch call at n_probe log-evenly spaced lambdas strictly inside the
        current bracket (first: lmb_range) and narrows the bracket to the two neighbouring probes that enclose the target, so the
        bracket shrinks by n_probe + 1 per round (a bisection: by 2, one encode per round).  It stops when a probe is within `tol` bytes
        of the target, when the bracket's ends are adjacent fp32 values, or after max_rounds rounds.
        The size counted is what compress_file would write: the stream plus the 4-byte '2H' prefix (image height, width).
        Returns (string, lmb, n_rounds): the largest stream seen that is <= target_bytes (if none was, the smallest seen), the fp32
        lambda it was coded at -- string == compress(im, lmb) -- and the number of rounds (= compress_batch calls)."""
        from ...utils.rate_search import multisection_search
        assert im.dim() == 4 and im.shape[0] == 1, f'a single image, got {im.shape=}'
        rep = im.expand(n_probe, -1, -1, -1)
        coded = []

        def sizes_of(lmbs):
            strings = self.compress_batch(rep[:len(lmbs)], lmbs)
            sizes = [len(x) + 4 for x in strings]
            coded.extend(strings)
            if verbose:
                print(f'round {len(coded) // len(lmbs) - 1}: ' + ', '.join(f'lmb={v:.3f} -> {n}B' for v, n in zip(lmbs, sizes)) + f', target={target_bytes}B')
            return sizes
        best, history, rounds = multisection_search(sizes_of, self.lmb_range[0], self.lmb_range[1], target_bytes, n_probe=n_probe,
                                                    max_rounds=max_rounds, tol=tol)
        return coded[best], float(np.float32(history[best][0])), rounds

    # ---- the eval-mode forward pass (reference qarv/model.py:258-363)
    def sample_lmb(self, n):
        """(:258-264) n lambdas drawn uniformly in lmb^(1/3) over lmb_range, with torch's RNG on the model device."""
        low, high = self.lmb_range
        p = 3.0
        low, high = math.pow(low, 1 / p), math.pow(high, 1 / p)
        transformed_lmb = low + (high - low) * torch.rand(n, device=self._dummy.device)
        return torch.pow(transformed_lmb, exponent=p)

    def expand_to_tensor(self, input_, n):
        """(:266-273) a float / int / one-element tensor -> an (n,) tensor on the model device; an (n,) tensor as it is."""
        assert isinstance(input_, (torch.Tensor, float, int)), f'{type(input_)=}'
        if isinstance(input_, torch.Tensor) and (input_.numel() == 1):
            input_ = input_.item()
        if isinstance(input_, (float, int)):
            input_ = torch.full(size=(n,), fill_value=float(input_), device=self._dummy.device)
        assert input_.shape == (n,), f'{input_=}, {input_.shape=}'
        return input_

    @torch.no_grad()
    @on_model_device
    def forward(self, batch, lmb=None, return_rec=False):
        """The reference's `model(batch, lmb)` (:317-363) without entropy coding: batch = a (B, 3, H, W) tensor or an (im, label) pair;
        lmb = None (sample_lmb(B)), a float or a (B,) tensor.  Returns an OrderedDict: loss (0-d tensor on the model device,
        mean of kl + lmb * mse), bppix, mse (mean((x_hat - x_target)^2) on the UNCLAMPED reconstruction, batch mean), psnr (from the
        batch-mean MSE of im_hat) and im_hat (B, 3, H, W) when return_rec.
        The whole batch is ONE run of the 'ence' encode plan (with the per-channel rate) and one of the 'evald' decode plan fed with its
        symbols (the final conv stored raw + lvae_rd_image_f32), whatever the lambdas are: with distinct lambdas the plans read one AdaLN
        vector pair per image (_NetPlan.vec) -- a batch with per-image lambdas gives the bits of per-image calls.
        Eval-mode (quantised) statistics only: model.train() adds no training noise.  Deterministic: two calls on the same input (and
        lambdas) return the same bits.  A NaN / inf raises NonFiniteError, an input outside [0, 1] AssertionError."""
        im = batch[0] if isinstance(batch, (tuple, list)) else batch
        im = im.to(self._dummy.device)
        assert im.dim() == 4 and im.shape[1] == 3 and not im.requires_grad, f'{im.shape=}'
        nB, imC, imH, imW = im.shape
        assert (imH % self.max_stride == 0) and (imW % self.max_stride == 0), f'{im.shape=}'
        if lmb is None:
            lmb = self.sample_lmb(n=nB)
        lmb = self.expand_to_tensor(lmb, n=nB)
        self._prepare()
        lv = [float(np.float32(v)) for v in lmb.tolist()]          # the plans' embedding is built from the fp32 value (_set_lmb)
        arg = self._lmb_arg(lv, nB)
        vec = isinstance(arg, list)
        ndims = imC * imH * imW
        self._set_lmb(arg)
        enc = self._plan('ence', nB, imH, imW, vec=vec)
        dec = self._plan('evald', nB, imH // self.max_stride, imW // self.max_stride, vec=vec)
        enc.im.view(nB, 3, imH, imW).copy_(im)
        dec.im.view(nB, 3, imH, imW).copy_(im)
        self._use_lmb(enc)
        enc.run()
        enc.fetch_status()
        torch.cuda.current_stream(enc.device).synchronize()
        enc.raise_if_flagged(where='in forward() (encoder)')
        dec.sym_all.copy_(enc.sym_all)                              # the encoder stops at CompresionStopFlag: decode its symbols
        self._use_lmb(dec)
        dec.run()
        dec.fetch_status()
        torch.cuda.current_stream(dec.device).synchronize()
        dec.raise_if_flagged(where='in forward() (decoder)')
        kl_chan = enc.kl_chan.cpu()
        kl = sum(kl_chan[o:o + nB * z].view(nB, z).sum(1) for o, (z, _) in zip(enc.chan_off, enc.lat_shapes)) / ndims
        rd = dec.rd_sums.view(nB, 2).cpu()
        im_hat = dec.out.clone() if return_rec else None
        distortion = rd[:, 0] / ndims
        lmb64 = torch.tensor(lv, dtype=torch.float64)
        stats = OrderedDict()
        stats['loss'] = (kl + lmb64 * distortion).mean(0).to(device=self._dummy.device, dtype=torch.float32)
        stats['bppix'] = float(kl.mean(0)) * self.log2_e * imC
        stats['mse'] = float(distortion.mean(0))
        stats['psnr'] = -10 * math.log10(float(rd[:, 1].sum()) / (nB * ndims))
        if return_rec:
            stats['im_hat'] = im_hat
        return stats

    # ---- coder-free paths
    @torch.no_grad()
    @on_model_device
    def estimate(self, im, lmb=None):
        """Eval-mode forward (forward_end2end in eval mode, qarv/model.py:94-97,294-315) without entropy coding:
        returns (im_hat (B,3,H,W) in [0,1], nats (num_latents, B) float64 = sum(-ln P) per latent block and image).  lmb: one lambda or B."""
        B, _, H, W = im.shape
        lmb = self._lmb_arg(lmb, B)
        vec = isinstance(lmb, list)
        assert (H % self.max_stride == 0) and (W % self.max_stride == 0)
        self._prepare(); self._set_lmb(lmb)
        enc = self._plan('encb', B, H, W, vec=vec)
        dec = self._plan('dec', B, H // self.max_stride, W // self.max_stride, vec=vec)
        enc.im.view(B, 3, H, W).copy_(im)
        enc.nats.zero_()
        self._use_lmb(enc)
        enc.run()
        enc.fetch_status()
        torch.cuda.current_stream(enc.device).synchronize()
        enc.raise_if_flagged(where='in estimate() (encoder)')
        # the encoder stops at CompresionStopFlag; reconstruct by feeding its symbols to the decode plan (same latent layout)
        dec.sym_all.copy_(enc.sym_all)
        self._use_lmb(dec)
        dec.run()
        dec.fetch_status()
        torch.cuda.current_stream(dec.device).synchronize()
        dec.raise_if_flagged(where='in estimate() (decoder)')
        return dec.out.clone(), enc.nats.view(self.num_latents, B).clone()

    @torch.no_grad()
    @on_model_device
    def conditional_sample(self, lmb, latents, emb=None, bhw_repeat=None, t=1.0, seed=None, return_latents=False):
        """Decoder output conditioned on a list of latents (qarv/model.py:365-395).  latents[i] is a (B, z_i, h_i, w_i) tensor on
        the model device (integer + prior mean, what `get_latents` / the decoder produce) or None; a missing latent is drawn from
        the prior at temperature t, z = pm + pv*N(0,1)*t + U(-.5,.5)*t (:98-100), by the device RNG of `lvae_prior_sample_f32`
        (Philox4x32-10 keyed by `seed`; default: a fresh seed per call from torch's CPU generator).  t = 0 is deterministic.
        `emb` is accepted for signature compatibility and must be None (the embedding is always derived from lmb).
        return_latents=True (not in the reference) also returns the latents actually used, [(B, z_i, h_i, w_i)]."""
        assert emb is None, 'explicit embeddings are not supported: pass lmb'
        assert len(latents) == self.num_latents
        if latents[0] is None:
            assert bhw_repeat is not None, 'bhw_repeat should be provided'
            B, nH, nW = bhw_repeat
        else:
            B, _, nH, nW = latents[0].shape
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        lmb = self._lmb_arg(lmb, B)                                  # one lambda, or one per image
        vec = isinstance(lmb, list)
        self._prepare(); self._set_lmb(lmb if vec else float(lmb))
        pl = self._plan('dec', B, nH, nW, vec=vec)
        self._use_lmb(pl)
        st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
        lo, used = 0, []
        for li, cut in enumerate(pl.cuts):
            pl.run(lo, cut)
            zdim, hw = pl.lat_shapes[li]
            if latents[li] is None:
                # the launch at `cut` is this block's dequantize: replaced by a draw from the prior written to the same buffer
                rc = pl.lib.lvae_prior_sample_f32(pl.prm_ptrs[li], pl.zhat_ptrs[li], B * hw, zdim, zdim, float(t),
                                                  seed, li << 40, st)
                if rc:
                    raise RuntimeError(f'lvae_prior_sample_f32 failed: {rc}')
                lo = cut + 1
                if return_latents:
                    zs = pl.zhat_bufs[li][:B * hw * zdim].view(B, hw, zdim)
                    used.append(zs.permute(0, 2, 1).reshape(B, zdim, *pl.lat_hw[li]).clone())
            else:
                assert tuple(latents[li].shape) == (B, zdim, *pl.lat_hw[li]), f'latent {li}: shape {tuple(latents[li].shape)}'
                # the supplied latent is used VERBATIM (qarv/model.py:101-103, `z = latent`): it goes straight into this block's
                # z buffer (NCHW -> NHWC rows) and the dequantize launch at `cut` is skipped -- no re-quantisation against the
                # current prior mean, so edited / interpolated latents and the 'exclude' / 'reverse' / 'single' modes of
                # scripts/qarv/robust-decoding.py behave as in the reference
                zt = latents[li].to(pl.device, torch.float32).permute(0, 2, 3, 1).reshape(-1)
                pl.zhat_bufs[li][:zt.numel()].copy_(zt)
                lo = cut + 1
                if return_latents:
                    used.append(latents[li])
        pl.run(lo, None)
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        if all(z is not None for z in latents) or float(t) == 0.0:
            pl.raise_if_flagged(where='in conditional_sample()')
        else:
            # latents drawn from the prior at t > 0 are random numbers of the model's own scale (with untrained weights the deeper blocks'
            # prior scales are astronomically large): whatever they lead to is the sample, as in the reference -- clear the word, no error
            pl.status.zero_(); pl.status_host.zero_()
        return (pl.out.clone(), used) if return_latents else pl.out.clone()

    @torch.no_grad()
    def unconditional_sample(self, lmb, bhw_repeat, t=1.0, seed=None, return_latents=False):
        """qarv/model.py:397-404: generate images from the prior alone."""
        return self.conditional_sample(lmb, [None] * self.num_latents, bhw_repeat=bhw_repeat, t=t, seed=seed,
                                       return_latents=return_latents)

    @torch.no_grad()
    def get_latents(self, im, lmb=None):
        """What scripts/qarv/robust-decoding.py reads from forward_end2end(..., get_latent=True) in eval mode
        (qarv/model.py:94-97,294-315): per latent block the quantized latent z = symbols + prior mean as a (B, z, h, w) tensor and
        its rate in nats per image, (num_latents, B)."""
        B, _, H, W = im.shape
        lmb = self._lmb_arg(lmb, B)
        _, nats = self.estimate(im, lmb)
        dec = self._plan('dec', B, H // self.max_stride, W // self.max_stride, vec=isinstance(lmb, list))
        zs = []
        for li, (zdim, hw) in enumerate(dec.lat_shapes):
            o = dec.sym_off[li]
            sym = dec.sym_all[o:o + B * zdim * hw].view(B, zdim, hw).float()
            pm = dec.pm_bufs[li].view(B, hw, zdim).permute(0, 2, 1)
            zs.append((sym + pm).reshape(B, zdim, *dec.lat_hw[li]).contiguous())
        return zs, nats

    def _rate_map_run(self, im, u8, B, H, W, lmb, return_rec):
        """CodecBase.rate_map: the 'encp' plan up to the last block's position kernel; im_hat from the 'evald' plan forward() runs."""
        lmb = self._lmb_arg(lmb, B)
        vec = isinstance(lmb, list)
        self._prepare(); self._set_lmb(lmb)
        enc = self._plan('encp', B, H, W, vec=vec)
        self._load_input(enc.im.view(B, 3, H, W), im, u8, 0, B)
        self._use_lmb(enc)
        self._run_with_pos(enc, 0, upto=enc.qcuts[-1])
        enc.fetch_status()
        torch.cuda.current_stream(enc.device).synchronize()
        enc.raise_if_flagged(where='in rate_map() (encoder)')
        if not return_rec:
            return enc, None, None
        dec = self._plan('evald', B, H // self.max_stride, W // self.max_stride, vec=vec)
        dec.im.view(B, 3, H, W).copy_(enc.im.view(B, 3, H, W))
        dec.sym_all.copy_(enc.sym_all)
        self._use_lmb(dec)
        dec.run()
        dec.fetch_status()
        torch.cuda.current_stream(dec.device).synchronize()
        dec.raise_if_flagged(where='in rate_map() (decoder)')
        return enc, None, dec.out.clone()

    @torch.no_grad()
    @on_model_device
    def _estimate_chan(self, im, lmb):
        """estimate() with a reproducible rate: (im_hat (B,3,H,W) in [0,1], nats (B,) float64 = sum(-ln P) per image).  The rate comes
        from the per-channel kernel of forward() (lvae_gaussian_nll_chan_f32: fixed summation order per image and channel, no atomics)
        instead of estimate's per-block atomic sums, and the channels of an image are added in a fixed order on the host, so an image's
        value does not depend on the batch it is in or on the run."""
        B, _, H, W = im.shape
        lmb = self._lmb_arg(lmb, B)
        vec = isinstance(lmb, list)
        assert (H % self.max_stride == 0) and (W % self.max_stride == 0)
        self._prepare(); self._set_lmb(lmb)
        enc = self._plan('ence', B, H, W, vec=vec)
        dec = self._plan('dec', B, H // self.max_stride, W // self.max_stride, vec=vec)
        enc.im.view(B, 3, H, W).copy_(im)
        self._use_lmb(enc)
        enc.run()
        enc.fetch_status()
        torch.cuda.current_stream(enc.device).synchronize()
        enc.raise_if_flagged(where='in self_evaluate() (encoder)')
        dec.sym_all.copy_(enc.sym_all)
        self._use_lmb(dec)
        dec.run()
        dec.fetch_status()
        torch.cuda.current_stream(dec.device).synchronize()
        dec.raise_if_flagged(where='in self_evaluate() (decoder)')
        kl_chan = enc.kl_chan.cpu()
        nats = torch.zeros(B, dtype=torch.float64)
        for b in range(B):                      # blocks in order, each block's z channels as one 1-D sum: the same operations for any B
            for o, (z, _) in zip(enc.chan_off, enc.lat_shapes):
                nats[b] += kl_chan[o + b * z:o + (b + 1) * z].sum()
        return dec.out.clone(), nats

    @torch.no_grad()
    def _evaluate_image(self, impath, lmbs):
        """One image of self_evaluate at every lambda of `lmbs`, as ONE batch (the padded image replicated): [(kl, mse)] per lambda --
        kl in nats per dimension of the original image, mse of the cropped, clamped reconstruction (qarv/model.py:427-473)."""
        from PIL import Image
        img = Image.open(impath)
        h, w = img.height, img.width
        im = coding.pil_to_tensor01(coding.pad_divisible_by(img, div=self.max_stride)).unsqueeze_(0).to(self._dummy.device)
        im_hat, nats = self._estimate_chan(im.expand(len(lmbs), -1, -1, -1), list(lmbs))
        real = coding.pil_to_tensor01(img).to(im_hat.device)
        return [(float(nats[j]) / (3 * h * w), float((real - im_hat[j, :, :h, :w]).square().mean())) for j in range(len(lmbs))]

    @staticmethod
    def _add_image_stats(tot, kl, mse, lmb, log2_e):
        distortion = 4.0 * mse      # mse between (x_hat, x_target) in (-1,1) units; uses the CLAMPED reconstruction
        tot['loss'] += kl + lmb * distortion
        tot['bpp'] += kl * log2_e * 3
        tot['psnr'] += -10 * math.log10(mse)

    @torch.no_grad()
    def _self_evaluate(self, img_paths, lmb: float):
        """qarv/model.py:427-473 (per-image loop at one lambda; estimated bpp from the likelihoods, PSNR on the cropped reconstruction)."""
        tot = {'loss': 0.0, 'bpp': 0.0, 'psnr': 0.0}
        for impath in img_paths:
            (kl, mse), = self._evaluate_image(impath, [lmb])
            self._add_image_stats(tot, kl, mse, lmb, self.log2_e)
        n = len(img_paths)
        out = {k: v / n for k, v in tot.items()}
        out['lambda'] = lmb
        return out

    @torch.no_grad()
    def self_evaluate(self, img_dir, lmb_range=None, steps=8, log_dir=None):
        """qarv/model.py:491-507: estimated-rate RD sweep over `steps` lambdas log-spaced in lmb_range.  Each image runs ONCE, as a batch
        of `steps` copies with one lambda each; per lambda the images are accumulated in path order, so the result equals the
        reference's loop (`_self_evaluate` per lambda) float for float.  The plans of an image size hold `steps` copies of its feature
        maps at once: for multi-megapixel sets lower `steps` if memory is short."""
        from collections import defaultdict
        from pathlib import Path
        img_paths = sorted(Path(img_dir).rglob('*.*'))
        start, end = self.lmb_range if (lmb_range is None) else lmb_range
        lambdas = torch.linspace(math.log(start), math.log(end), steps=steps).exp().tolist()
        tots = [{'loss': 0.0, 'bpp': 0.0, 'psnr': 0.0} for _ in lambdas]
        for impath in img_paths:
            for tot, lmb, (kl, mse) in zip(tots, lambdas, self._evaluate_image(impath, lambdas)):
                self._add_image_stats(tot, kl, mse, lmb, self.log2_e)
        stats = defaultdict(list)
        n = len(img_paths)
        for tot, lmb in zip(tots, lambdas):
            for k, v in tot.items():
                stats[k].append(v / n)
            stats['lambda'].append(lmb)
        return stats

    # ---- debugging / test access (not on the hot path)
    @torch.no_grad()
    @on_model_device
    def encode_trace(self, im, lmb=None, full=False, force_z=None):
        """Run the encode plan and return per-block int arrays (symbols, indexes in NCHW order) for parity tests.
        full=True adds the float tensors behind them per block -- pm, lv (raw log-variance parameter), qm, as (B, z, hw) arrays --
        and force_z (a list of (B, z, h, w) tensors or None per block) replaces the latent a block hands on to the blocks below
        it (teacher forcing: with the oracle's latents every block sees the oracle's inputs up to rounding noise, so a flip is
        never the cascade of an earlier one)."""
        B, _, H, W = im.shape
        lmb = self._lmb_arg(lmb, B)                                  # one lambda, or one per image
        self._prepare(); self._set_lmb(lmb)
        pl = self._plan('enc', B, H, W, vec=isinstance(lmb, list))
        pl.im.view(B, 3, H, W).copy_(im)
        self._use_lmb(pl)
        return self._trace(pl, B, full, force_z)
