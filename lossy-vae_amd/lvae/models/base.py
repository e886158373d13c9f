"""Shared host-side machinery of the codecs: batch -> pipeline groups (one HIP stream + one host thread each, so that a
group's host rANS coding overlaps the other group's GPU work), coder thread budget."""
import ctypes
import functools
import logging
import math
import os
import threading
import time

import numpy as np
import torch
import torch.nn as nn

from .. import _native
from ..engine import NonFiniteError, Plan
from .entropy_coding import rans_decode_streams

_W16_LOCK = threading.Lock()


def split_bf16x3(t):
    """Exact 3-term bf16 split of an fp32 tensor: returns a (3, *t.shape) bf16 tensor [hi, mid, lo] with hi+mid+lo == t up to
    2^-25 |t| (same arithmetic as the kernel applies to activations: RNE conversions, exact fp32 residuals)."""
    hi = t.to(torch.bfloat16)
    r1 = t - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], 0).contiguous()


def pack_bf16x3(t):
    """The prec-2 weight buffer of lvae_gemm_f32 for an [N][K] fp32 weight: the three bf16 planes hi | mid | lo ([3][N][K]),
    followed -- when K % 32 == 0 -- by the same values in k16-interleaved order [N][K/16][3][16] (what the double-buffered
    gemm_x3k16_kernel streams: one 16-deep stage of one row is 96 contiguous bytes)."""
    planes = split_bf16x3(t)
    n, k = t.shape
    if k % 32:
        return planes.reshape(-1)
    inter = planes.view(3, n, k // 16, 16).permute(1, 2, 0, 3).contiguous()
    return torch.cat([planes.reshape(-1), inter.reshape(-1)])


def split_f16x2(t):
    """2-term fp16 split of an fp32 tensor: (2, *t.shape) fp16 [hi, lo'] with hi + lo' / 2048 == t up to 2^-24 |t| -- the
    arithmetic csrc/gemm_h2.hip applies to activations: hi = f16(t) (RNE), lo' = f16((t - hi) * 2048) (the residual is exact)."""
    hi = t.to(torch.float16)
    lo = ((t - hi.float()) * 2048.0).to(torch.float16)
    return torch.stack([hi, lo], 0).contiguous()


def pack_f16x2(t):
    """The prec-4 weight buffer of lvae_gemm_f32 for an [N][K] fp32 weight (K % 16 == 0): fp16 planes hi | lo' in k16-interleaved
    order [N][K/16][2][16] -- one 16-deep stage of one row is 64 contiguous bytes.  None when a weight does not fit fp16's range
    (the caller keeps that GEMM on the bf16x3 arithmetic)."""
    n, k = t.shape
    if k % 16 or not bool(torch.isfinite(t).all()) or float(t.abs().max()) >= 65504.0:
        return None
    planes = split_f16x2(t.float())
    return planes.view(2, n, k // 16, 16).permute(1, 2, 0, 3).contiguous().reshape(-1)


def pack_f16x2_k32(t):
    """An [N][K] fp32 matrix (K % 32 == 0) in the plane format H2K32 = [N][K/32][2][32] fp16 (include/lvae_hip.h: lvae_gemm_desc.a_h2):
    per row and 32 k, the 32 hi terms then the 32 lo' terms -- what csrc/gemm_h2p.hip streams for both operands.  None when a value
    does not fit fp16's range."""
    n, k = t.shape
    if k % 32 or not bool(torch.isfinite(t).all()) or float(t.abs().max()) >= 65504.0:
        return None
    planes = split_f16x2(t.float())
    return planes.view(2, n, k // 32, 32).permute(1, 2, 0, 3).contiguous().reshape(-1)


def unpack_f16x2_k32(buf, n, k):
    """Inverse of the H2K32 layout (tests): (hi, lo') fp16 tensors [n][k] of a buffer holding n rows of k elements."""
    v = buf.view(torch.float16).reshape(n, k // 32, 2, 32)
    return v[:, :, 0, :].reshape(n, k), v[:, :, 1, :].reshape(n, k)


def pack_mxfp8(t):
    """The prec-3 weight buffer of lvae_gemm_f32 for an [N][K] fp32 weight: OCP MX-fp8 -- e4m3 elements with one E8M0
    (power-of-two) scale per 32 consecutive k of a row -- as a uint8 tensor: [N][Kp] element bytes followed by [N][Kp/32] scale
    bytes, Kp = K rounded up to a multiple of 64 (zero padded).  Block scale: 2^e with amax / 2^e in (224, 448] (e4m3's largest
    finite value is 448); elements rounded to nearest even by torch's float8_e4m3fn conversion -- the same rule the kernel applies
    to activations with v_cvt_pk_fp8_f32."""
    n, k = t.shape
    kp = (k + 63) // 64 * 64
    w = torch.zeros(n, kp, dtype=torch.float32, device=t.device)
    w[:, :k] = t.float()
    blk = w.view(n, kp // 32, 32)
    amax = blk.abs().amax(dim=2)
    bits = amax.view(torch.int32)
    eb = ((bits >> 23) & 0xff) - 8
    eb = eb + ((bits & 0x7fffff) > 0x600000).to(torch.int32)
    eb = eb.clamp(1, 254)
    inv = ((254 - eb) << 23).view(torch.float32)                      # 2^(127 - eb), exact
    q = (blk * inv.unsqueeze(2)).to(torch.float8_e4m3fn).view(torch.uint8).reshape(n, kp)
    return torch.cat([q.reshape(-1), eb.to(torch.uint8).reshape(-1)]).contiguous()


def pack_mxfp8_q8(t):
    """An [N][K] fp32 matrix (K % 64 == 0) in the MX-fp8 operand format Q8 of csrc/gemm_q8.hip (include/lvae_hip.h: lvae_gemm_desc.a_h2
    with prec 3): N*K e4m3 bytes row-major, then the E8M0 block scales as [K/64][N][2].  Same element / scale rule as pack_mxfp8."""
    n, k = t.shape
    assert k % 64 == 0
    buf = pack_mxfp8(t)
    data, sc = buf[:n * k], buf[n * k:].view(n, k // 64, 2)
    return torch.cat([data, sc.permute(1, 0, 2).contiguous().reshape(-1)]).contiguous()


def unpack_mxfp8_q8(buf, n, k):
    """Inverse of the Q8 layout (tests): the fp32 values an [n][k] Q8 buffer stands for."""
    buf = buf.view(torch.uint8).reshape(-1)
    data, sc = buf[:n * k], buf[n * k:n * k + n * k // 32].view(k // 64, n, 2).permute(1, 0, 2).contiguous().reshape(-1)
    return unpack_mxfp8(torch.cat([data, sc]), n, k)


def unpack_mxfp8(buf, n, k):
    """Inverse of pack_mxfp8 (tests): the fp32 values the MX-fp8 weights stand for, [N][K]."""
    kp = (k + 63) // 64 * 64
    q = buf[:n * kp].view(torch.float8_e4m3fn).float().view(n, kp // 32, 32)
    eb = buf[n * kp:].to(torch.int32).view(n, kp // 32)
    scale = torch.pow(2.0, (eb - 127).double()).float()
    return (q * scale.unsqueeze(2)).view(n, kp)[:, :k].contiguous()


class LazyW16:
    """{address of an fp32 GEMM weight: address of its reduced-precision copy}, filled ON FIRST USE by Plan.gemm: only tensors
    that are actually passed as `Wt` get a bf16 / bf16x3 copy (the packed dict also holds the AdaLN matrix, depthwise tables,
    biases ... which never are).  Thread-safe: plans are recorded concurrently by the pipeline-group threads."""

    def __init__(self, tensors, mode):
        self.by_ptr = {t.data_ptr(): t for t in tensors.values()
                       if t.dim() == 2 and t.dtype == torch.float32 and t.shape[1] % 8 == 0}
        self.mode, self.map, self.keep = mode, {}, []

    def get(self, ptr):
        h = self.map.get(ptr)
        if h is not None:
            return h
        t = self.by_ptr.get(ptr)
        if t is None:
            return None
        with _W16_LOCK:
            h = self.map.get(ptr)
            if h is None:
                c = (pack_bf16x3(t) if self.mode == 'bf16x3' else pack_mxfp8(t) if self.mode == 'fp8'
                     else pack_f16x2(t) if self.mode == 'f16x2' else pack_f16x2_k32(t) if self.mode == 'f16x2k32'
                     else (pack_mxfp8_q8(t) if t.shape[1] % 64 == 0 else None) if self.mode == 'mxfp8q8'
                     else t.to(torch.bfloat16).contiguous())
                if c is None:                       # f16x2: a weight outside fp16's range
                    self.map[ptr] = 0
                    return None
                self.keep.append(c)
                h = self.map[ptr] = c.data_ptr()
        return h or None


# GEMM arithmetic of newly built models.  A bitstream decodes only under the arithmetic that produced it (the priors must match bit
# for bit) and the container -- the reference's, byte for byte -- does not record it: the default is FIXED here (no environment
# override), another mode is an explicit `model.set_gemm_precision(...)` call that must be made identically on both sides
# (DESIGN.md 4).  compress_mode() logs the active mode once per model.
DEFAULT_PRECISION = 'f16x2'
PRECISIONS = ('fp32', 'bf16', 'bf16x3', 'f16x2', 'fp8')
PREC_CODE = {'fp32': 0, 'bf16': 1, 'bf16x3': 2, 'fp8': 3, 'f16x2': 4}        # lvae_gemm_desc.prec
assert DEFAULT_PRECISION in PRECISIONS, DEFAULT_PRECISION
_log = logging.getLogger('lvae')


class PackedWeights:
    """Device-resident, kernel-friendly copies of a model's weights (built once per device / weight version).  A model's subclass fills
    `t` (name -> fp32 tensor) in its own layout."""

    def __init__(self, model, device):
        self.t, self.device, self._w16 = {}, device, {}
        dg = model._dg()
        self.scale_table = dg.scale_table.detach().to(device=device, dtype=torch.float32).contiguous()
        self.scale_bound = float(dg.lower_bound_scale.bound.item())

    def put(self, name, t):
        self.t[name] = t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def p(self, name):
        return self.t[name].data_ptr()

    def bf16_map(self, mode):
        """The LazyW16 of a mode, built once, under a lock: plans are recorded concurrently by the pipeline-group threads, and a second
        builder would free the first one's copies while its plan still points at them."""
        with _W16_LOCK:
            if mode not in self._w16:
                self._w16[mode] = LazyW16(self.t, mode)
        return self._w16[mode]


class CodecPlan(Plan):
    """What the models' plans share: the GEMM arithmetic and its weight maps, the per-latent-block lists the coder loops and the test
    hooks read, and the ConvNeXt-block recorder."""
    lp_storage = False        # the plan has the reduced-precision 'fp8' form (bf16 feature maps, MX-fp8 GEMMs, BASELINE config 5)
    use_mlp_sk = False        # small-map MLPs as the fused split-K launch (csrc/mlp_sk.hip)

    def __init__(self, model, pk, B):
        super().__init__(pk.device)
        self.model, self.pk, self.B = model, pk, B
        if model._prec == 'fp8' and not self.lp_storage:
            raise NotImplementedError("the 'fp8' mode (bf16 activation storage + MX-fp8 GEMMs, BASELINE config 5) is built for qarv_base")
        self.prec = PREC_CODE[model._prec]
        self.prec_name = model._prec
        self.w16 = pk.bf16_map(model._prec) if self.prec else None
        self.w16_x3 = pk.bf16_map('bf16x3') if self.prec == 4 else None
        self.w16_k32 = pk.bf16_map('f16x2k32') if self.prec == 4 else None
        self.w16_q8 = pk.bf16_map('mxfp8q8') if self.prec == 3 else None
        self.lp = self.prec == 3                # feature maps stored as bf16
        self.adt = torch.bfloat16 if self.lp else torch.float32
        self.lat_shapes, self.lat_hw = [], []   # per latent block: (z, h * w), (h, w)
        self.idx_off, self.sym_off = [], []     # ... element offsets into idx_all / sym_all
        self.cuts, self.qcuts = [], []          # decode plans: op index after each prior_index; encode plans: after each quantize launch
        self.pm_bufs = []                       # ... prior means [M][z] (NHWC rows)
        self.prm_bufs, self.qm_bufs, self.zhat_bufs, self.zhat_ld = [], [], [], []   # test access (CodecBase._trace_blocks), the generative API

    def alloc_symbols(self, n_sym, host=True):
        """Device symbol / index buffers of every latent block; host=True adds the coder's pinned host copies."""
        self.n_sym = n_sym
        self.sym_all, self.idx_all = self.new(n_sym, torch.int32), self.new(n_sym, torch.uint8)
        if host:
            self.sym_host = torch.empty(n_sym, dtype=torch.int32).pin_memory()
            self.idx_host = torch.empty(n_sym, dtype=torch.uint8).pin_memory()
            self.sym_np, self.idx_np = self.sym_host.numpy(), self.idx_host.numpy()

    def alloc_pos(self):
        """Position plans (rate_map): one fp64 buffer per latent block, (B, h, w) nats, written by lvae_gaussian_nll_pos_f32 behind that
        block's quantize launch (CodecBase._run_with_pos)."""
        self.pos_bufs = [self.new(self.B * hw, torch.float64) for _, hw in self.lat_shapes]

    def dwln_add(self, fmt, p, x, y, H, W, C, k):
        """Record block p's depthwise + LayerNorm launch with output format `fmt` ('f32' | 'h2' | 'bf16' | 'q8': lvae_dwconv_ln_<fmt>) as
        p + '.dwln', with the model's affine: LayerNorm weights, or AdaLN vectors."""
        raise NotImplementedError

    def cnx(self, p, m, x, out, H, W):
        """A ConvNeXt block = depthwise+LN(+affine) kernel, fc1+GELU GEMM, fc2+gamma+residual GEMM."""
        pk = self.pk
        C, k, hid = m.dim, m.kernel_size, m.hidden
        M = self.B * H * W
        y = self.buf(self.sname('y'), M * C, self.adt).data_ptr()
        mlp = dict(y=y, M=M, C=C, hid=hid, w1=pk.p(p + '.fc1_w'), b1=pk.p(p + '.fc1_b'), w2=pk.p(p + '.fc2_w'), b2=pk.p(p + '.fc2_b'),
                   gamma=pk.p(p + '.gamma'), res=x, out=out, label=p + '.mlp')
        # f16x2 plans: y and the hidden map have one consumer each (fc1 / fc2), so their producers store them pre-split (hi / lo' fp16
        # planes, 4 bytes per element like fp32) and the two GEMMs stream both operands by LDS-DMA with no conversion in the main loop
        # (reduced-precision plans: the same idea with MX-fp8 -- the producers quantise, csrc/gemm_q8.hip streams)
        # (small maps: the split-K layers -- pre-split + serial split-K where the batch makes that the faster form, same bits: engine.mlp_pipeline)
        if self.mlp_fused_ok(C, hid, k, M=M, rows_per_image=H * W):
            # the stride-4 blocks: fc1 -> GELU -> fc2 as one launch, the hidden tile never leaves the CU (csrc/mlp_h2c.hip)
            self.dwln_add('h2', p, x, y, H, W, C, k)
            self.mlp_fused(**mlp)
            return
        sk = self.mlp_sk_ok(C, hid, k, H * W, M) if self.use_mlp_sk else None
        if sk is not None:
            # stride-32 / 64 maps (both GEMMs split-K): fc1 -> GELU -> fc2's partial sums as one launch, then the reduce launch
            self.dwln_add('h2', p, x, y, H, W, C, k)
            self.mlp_sk(S1=sk[0], S2=sk[1], **mlp)
            return
        h = self.buf(self.sname('hid'), M * hid, self.adt).data_ptr()
        if self.mlp_q8_ok(C, hid, k):
            pre1, pre2, S1, S2 = True, True, None, None
        else:
            pre1, pre2, S1, S2 = self.mlp_pipeline(C, hid, k, H * W)
        fmt = ('q8' if pre1 else 'bf16') if self.lp else ('h2' if pre1 else 'f32')
        self.dwln_add(fmt, p, x, y, H, W, C, k)
        self.gemm(A0=y, K0=C, M=M, N=hid, Wt=pk.p(p + '.fc1_w'), bias=pk.p(p + '.fc1_b'), out=h,
                  epi=_native.EPI_BIAS_GELU, a_h2=pre1, out_h2=pre2, ksplit=S1, label=p + '.fc1')
        self.gemm(A0=h, K0=hid, M=M, N=C, Wt=pk.p(p + '.fc2_w'), bias=pk.p(p + '.fc2_b'),
                  gamma=pk.p(p + '.gamma'), res=x, ldres=C, out=out, epi=_native.EPI_GAMMA_RES, a_h2=pre2, ksplit=S2, label=p + '.fc2')


def on_model_device(fn):
    """Entry points that launch raw HIP kernels run with the MODEL's GPU as the current device (the launches go to streams of
    that device; the caller's current device may be another GPU of the node)."""
    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        dev = self._dummy.device
        if dev.type == 'cuda' and torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                return fn(self, *a, **k)
        return fn(self, *a, **k)
    return wrapper


class CodecBase(nn.Module):
    def _init_codec_base(self):
        self.coder_threads = 0          # 0 = all hardware threads
        self.pipeline_groups = int(os.environ.get('LVAE_GROUPS', '2'))
        self.enc_groups = int(os.environ.get('LVAE_ENC_GROUPS', '0'))      # 0 = use pipeline_groups
        self.dec_groups = int(os.environ.get('LVAE_DEC_GROUPS', '0'))
        self._streams = []
        self._pool = None
        # measurement hook (bench.py's roofline pass): the groups of a call run ONE AFTER THE OTHER, each on its own stream, instead of
        # concurrently from their threads -- the same plans and launches as the product configuration, but a launch bracketed by HIP
        # events on its stream is then alone on the GPU
        self.serial_groups = False
        # default: fp32-class accuracy on the bf16 matrix cores (same parity as the exact fp32 MFMA path, 1.2-1.5x faster)
        self._prec = DEFAULT_PRECISION
        self._packed, self._plans = None, {}

    # ---- packed weights and launch plans: built on first use, dropped when the weights move or change.  A model supplies
    # _latent_blocks(), _build_packed(dev), _plan_key(kind, ...) and _build_plan(kind, ...)
    def _invalidate(self):
        self._packed, self._plans = None, {}

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._invalidate()
        return super().load_state_dict(*a, **k)

    def _prepare(self):
        dev = self._dummy.device
        if self._packed is None or self._packed.device != dev:
            if dev.type != 'cuda':
                raise RuntimeError('lvae (MI355X build): compress/decompress run on the GPU only; move the model with '
                                   '.to("cuda") -- there is deliberately no CPU fallback')
            _native.lib()
            self._invalidate()
            with torch.no_grad():
                self._packed = self._build_packed(dev)
        return self._packed

    def _plan(self, kind, *a, **k):
        key = self._plan_key(kind, *a, **k)
        pl = self._plans.get(key)
        if pl is None:
            self._prepare()
            pl = self._plans[key] = self._build_plan(kind, *a, **k)
        return pl

    def _dg(self):
        for b in self._latent_blocks():
            return b.discrete_gaussian
        raise RuntimeError('no latent block')

    def _build_cdf_tables(self, build):
        """compress_mode(): `build(dg)` on the first latent block's entropy model; all blocks share one scale table, hence identical
        rows, so the others alias its CDF tables.  -> the blocks' entropy models."""
        first, *rest = dgs = [b.discrete_gaussian for b in self._latent_blocks()]
        build(first)
        for dg in rest:
            dg._quantized_cdf, dg._offset, dg._cdf_length, dg._host = first._quantized_cdf, first._offset, first._cdf_length, None
        return dgs

    def set_gemm_precision(self, mode):
        """'fp32': exact fp32 MFMA (fmaf chains); 'bf16x3': fp32-class accuracy from three-term bf16 splits on the bf16 MFMA
        (2.7x less matrix-pipe time); 'f16x2': fp32-class accuracy from two-term fp16 splits, three fp16 MFMAs per product step
        (half of bf16x3's again; GEMMs it does not cover -- 2x2 patch gathers, K % 32 != 0 -- run as bf16x3); 'bf16': operands rounded to bf16, fp32 activations in HBM; 'fp8': BASELINE config 5 --
        activations STORED as bf16 and every channel-mixing GEMM on the block-scaled MX-fp8 MFMA (visibly different numerics,
        half the HBM traffic).  Bitstreams are only decodable in the mode that produced them (the priors must match bit for bit)."""
        assert mode in PRECISIONS
        self._prec = mode
        self._prec_logged = None

    def _log_precision(self):
        """Called by compress_mode(): one log line per model and mode naming the arithmetic its bitstreams are tied to."""
        if getattr(self, '_prec_logged', None) != self._prec:
            self._prec_logged = self._prec
            # WARNING level: the container (the reference's, byte for byte) does not record the arithmetic, and a stream decoded under
            # another one fails -- with lvae.NonFiniteError at best, as a wrong picture at worst.  Builds before round 3 defaulted to 'bf16x3'.
            _log.warning("lvae: %s codes with GEMM arithmetic %r%s; a bitstream decodes only under the arithmetic that wrote it "
                         "(streams of builds that defaulted to 'bf16x3' need model.set_gemm_precision('bf16x3') on this side too)",
                         type(self).__name__, self._prec, ' (package default)' if self._prec == DEFAULT_PRECISION else ' (set explicitly)')

    # ---- one pipeline group's decode / encode as ONE foreign call (csrc/plan_runtime.cpp: lvae_decode_blocks / lvae_encode_blocks)
    native_group_loops = True             # False: the per-block Python loops (tests and bench.py compare the two)

    # The coder's arrays travel without copies (round 5): the index / quantize / dequantize launches of a group's native loops are recorded
    # with the plan's PINNED HOST arrays as their raster operands (device-mapped host memory; the kernels touch the raster in runs of 64
    # consecutive entries, csrc/pointwise.hip), so a decode has no blit launch between a segment and the coder or between the coder and the
    # next segment, and an encode none behind its segments.  The per-block Python loops and the test hooks keep the device arrays.

    @staticmethod
    def _alias_host(pl, seg, n_ops):
        """A copy of a native segment whose launches address pl.sym_host / pl.idx_host wherever the recorded ones address pl.sym_all / pl.idx_all."""
        raster_ops = {_native.OP_KINDS[k] for k in ('lvae_prior_index_f32', 'lvae_prior_index_sk_f32', 'lvae_quantize_f32', 'lvae_quantize_sk_f32', 'lvae_dequantize_f32')}
        spans = [(pl.sym_all.data_ptr(), pl.sym_all.numel() * 4, pl.sym_host.data_ptr()), (pl.idx_all.data_ptr(), pl.idx_all.numel(), pl.idx_host.data_ptr())]
        out = (_native.Op * max(1, n_ops))()
        ctypes.memmove(out, seg, ctypes.sizeof(_native.Op) * n_ops)
        for o in out[:n_ops]:
            if o.kind not in raster_ops:
                continue
            for j in range(len(o.p)):
                a = o.p[j]
                if a:
                    for lo_, size, host in spans:
                        if lo_ <= a < lo_ + size:
                            o.p[j] = host + (a - lo_)
        return out

    @classmethod
    def _group_blocks(cls_, pl, kind, cuts, offs, n):
        """The plan's latent blocks as a native array, cached on the plan: `cuts` = op index after each block's segment, `offs` = its
        element offset into sym_all / idx_all; per_image from pl.lat_shapes."""
        key = '_native_blocks_' + kind
        cached = getattr(pl, key, None)
        if cached is None:
            cls = _native.DecBlock if kind == 'dec' else _native.EncBlock
            arr = (cls * len(cuts))()
            segs, lo = [], 0
            for li, cut in enumerate(cuts):
                seg, n_ops = pl._segment(lo, cut)
                seg = cls_._alias_host(pl, seg, n_ops)     # the launches write / read the pinned host arrays: no device arrays, no copies
                segs.append(seg)
                z, hw = pl.lat_shapes[li]
                o = offs[li]
                b = arr[li]
                b.ops, b.n_ops, b.per_image = ctypes.cast(seg, ctypes.c_void_p).value, n_ops, z * hw
                b.idx_dev, b.idx_host = None, pl.idx_host.data_ptr() + o
                b.sym_dev, b.sym_host = None, pl.sym_host.data_ptr() + 4 * o
                lo = cut
            tail, n_tail = pl._segment(lo, len(pl.ops)) if kind == 'dec' else (None, 0)
            if n_tail:                                     # (the last block's symbols are read by the tail's first launch)
                tail = cls_._alias_host(pl, tail, n_tail)
            early = None
            if kind == 'dec' and len(cuts):                # the same blocks with block 0's launches taken out: _decode_group_native issues
                early = (cls * len(cuts))()                # that segment itself, before it looks at the strings
                ctypes.memmove(early, arr, ctypes.sizeof(arr))
                early[0].n_ops = 0
            cached = (arr, segs, tail, n_tail, early)
            setattr(pl, key, cached)
        return cached

    def _decode_group_native(self, pl, cuts, offs, n, strings, tables, nthreads, stream, T=None):
        """strings[b][li]: image b's stream of latent block li.  Runs the group's whole decode; the caller copies pl.out afterwards."""
        arr, segs, tail, n_tail, early = self._group_blocks(pl, 'dec', cuts, offs, n)
        nb = len(cuts)
        # The first segment (bias -> ... -> prior of the top latent block) does not depend on the bitstream: it is on its way to the GPU
        # before this thread turns to the strings (header parsing, container offsets, pointer tables: ~0.1-0.2 ms of interpreter time
        # per group that used to precede the first launch -- tools/dec_timeline.py).  The foreign call releases the interpreter lock,
        # so the other group's thread prepares meanwhile.
        if early is not None:
            with torch.cuda.device(pl.device):
                pl._run_native(0, cuts[0], stream.cuda_stream, seg=(segs[0], arr[0].n_ops))
            arr = early
        if callable(strings):
            strings = strings()                            # [image][block] -> bytes, or (bytes-like container, offset, length): no copies
        qcdf, cdf_len, offset = tables
        addr, size = [], []
        for li in range(nb):                               # block-major
            for b in range(n):
                s_ = strings[b][li]
                if isinstance(s_, tuple):
                    base, off, ln = s_
                    assert isinstance(base, bytes)
                    addr.append(ctypes.cast(ctypes.c_char_p(base), ctypes.c_void_p).value + off); size.append(ln)
                else:
                    addr.append(ctypes.cast(ctypes.c_char_p(s_), ctypes.c_void_p).value if len(s_) else None); size.append(len(s_))
        sp = (ctypes.c_void_p * len(addr))(*addr)
        sl = (ctypes.c_size_t * len(size))(*size)
        fb, fo = ctypes.c_int(-1), ctypes.c_int(-1)
        trace = getattr(self, 'dec_trace', None)             # measurement hook (tools/dec_timeline.py): a list collects per-block stamps
        secs = (ctypes.c_double * (64 if trace is not None else 2))()
        if trace is not None:
            secs[0], secs[1] = -64.0, _native.TRACE_MAGIC          # timeline request: capacity AND the magic word (include/lvae_hip.h)
        ss = pl.side_stream.cuda_stream if pl.side_stream is not None else None
        st_dev = pl.status_ptr()
        with torch.cuda.device(pl.device):
            rc = _native.lib().lvae_decode_blocks(arr, nb, n, sp, sl, qcdf.ctypes.data, qcdf.shape[1], cdf_len.ctypes.data, offset.ctypes.data,
                                                  ctypes.cast(tail, ctypes.c_void_p) if n_tail else None, n_tail, st_dev, pl.status_host.data_ptr(),
                                                  ctypes.c_void_p(stream.cuda_stream),
                                                  ctypes.c_void_p(ss) if ss is not None else None, int(nthreads), ctypes.byref(fb), ctypes.byref(fo), secs)
        if rc != 0:
            # every error exit leaves the plan's status word CLEAN: a bit that stayed set on the device (a corrupt stream decoded against
            # garbage, a failed launch) would otherwise fail the next, healthy call on this cached plan
            stream.synchronize()
            word = int(pl.status_host[0]) if rc == -75 else 0
            self._reset_status(pl)
            if rc == -75:       # a stream that did not decode because its scale indexes came from NaN / inf prior parameters
                raise NonFiniteError(word, getattr(pl, 'prec_name', None), f'while decoding (latent block {fb.value} of {nb})')
            if rc == -74:
                raise ValueError(f'rANS decode failed in latent block {fb.value} (corrupt or truncated bitstream)')
            raise RuntimeError(f'native decode failed: rc={rc} at latent block {fb.value}, launch {fo.value}')
        if trace is not None:
            trace.append((n, nb, list(secs)))
        if T is not None:
            T['dec_gpu_seg'] = T.get('dec_gpu_seg', 0) + secs[0]
            T['dec_rans'] = T.get('dec_rans', 0) + secs[1]

    def _encode_group_native(self, pl, cuts, offs, n, tables, nthreads, stream, T=None):
        """Runs the group's whole encode (launches, progressive hand-over, rANS).  -> strings[li][b] (bytes)."""
        arr, _segs, _tail, _nt, _early = self._group_blocks(pl, 'enc', cuts, offs, n)
        nb = len(cuts)
        qcdf, cdf_len, offset = tables
        caps = [8 * pl.lat_shapes[li][0] * pl.lat_shapes[li][1] + 64 for li in range(nb)]
        outs = getattr(pl, '_native_enc_out', None)
        if outs is None:                                   # output buffers live on the plan (one per block and image)
            outs = pl._native_enc_out = [np.empty(caps[li], dtype=np.uint8) for li in range(nb) for _ in range(n)]
        op = (ctypes.c_void_p * len(outs))(*[x.ctypes.data for x in outs])
        oc = (ctypes.c_size_t * len(outs))(*[caps[li] for li in range(nb) for _ in range(n)])
        out_len = (ctypes.c_long * len(outs))()
        fb, fo = ctypes.c_int(-1), ctypes.c_int(-1)
        secs = (ctypes.c_double * 3)()
        ss = pl.side_stream.cuda_stream if pl.side_stream is not None else None
        st_dev = pl.status_ptr()
        with torch.cuda.device(pl.device):
            rc = _native.lib().lvae_encode_blocks(arr, nb, n, op, oc, out_len, qcdf.ctypes.data, qcdf.shape[1], cdf_len.ctypes.data, offset.ctypes.data,
                                                  st_dev, pl.status_host.data_ptr(), ctypes.c_void_p(stream.cuda_stream),
                                                  ctypes.c_void_p(ss) if ss is not None else None, int(nthreads), ctypes.byref(fb), ctypes.byref(fo), secs)
        if rc in (-34, -75):    # out-of-range input (the reference's assert) / NaN or inf in a prior parameter or posterior mean
            word = int(pl.status_host[0])
            self._reset_status(pl)
            pl.raise_if_flagged(word, where='while encoding')
            raise RuntimeError(f'native encode reported rc={rc} without a status word')
        if rc != 0:
            self._reset_status(pl)
            raise RuntimeError(f'native encode failed: rc={rc} at latent block {fb.value}, launch {fo.value}')
        if T is not None:
            T['enc_launch'] = T.get('enc_launch', 0) + secs[0]
            T['enc_gpu_wait'] = T.get('enc_gpu_wait', 0) + secs[1]
            T['enc_rans'] = T.get('enc_rans', 0) + secs[2]
        return [[outs[li * n + b][:out_len[li * n + b]].tobytes() for b in range(n)] for li in range(nb)]

    def _decode_group_loop(self, pl, n, strings, tables, nthreads, stream, T=None):
        """A group's decode as a Python loop: the segment up to each cut of pl.cuts, then the host decode of that block's streams
        (strings[b][li]: image b's stream for cut li), then the tail; the caller copies pl.out afterwards."""
        lo = 0
        for li, cut in enumerate(pl.cuts):
            t0 = time.time()
            pl.run(lo, cut, stream=stream.cuda_stream)
            lo = cut
            t1 = self._decode_block(pl, li, n, [s[li] for s in strings], tables, nthreads, stream)
            if T is not None:
                t2 = time.time()
                T['dec_gpu_seg'] = T.get('dec_gpu_seg', 0) + t1 - t0
                T['dec_rans'] = T.get('dec_rans', 0) + t2 - t1
        pl.run(lo, None, stream=stream.cuda_stream)
        pl.fetch_status()                               # read by _check_decoded() after the groups have finished

    def _decode_block(self, pl, li, n, strings, tables, nthreads, stream):
        """The host step behind cut li: indexes to pinned memory, rANS decode of the n streams, symbols back to the device.  -> the time
        at which the GPU segment in front of it had finished."""
        z, hw = pl.lat_shapes[li]
        o, cnt = pl.idx_off[li], n * z * hw
        pl.idx_host[o:o + cnt].copy_(pl.idx_all[o:o + cnt], non_blocking=True)
        stream.synchronize()
        t1 = time.time()
        iv = [pl.idx_np[o + b * z * hw:o + (b + 1) * z * hw] for b in range(n)]
        sv = [pl.sym_np[o + b * z * hw:o + (b + 1) * z * hw] for b in range(n)]
        rans_decode_streams(tables, strings, iv, sv, nthreads)
        pl.sym_all[o:o + cnt].copy_(pl.sym_host[o:o + cnt], non_blocking=True)
        return t1

    @staticmethod
    def _reset_status(pl):
        """Error exits of the native group loops: wait for the plan's device, then zero its status word and the pinned mirror."""
        if getattr(pl, 'status', None) is not None:
            torch.cuda.synchronize(pl.device)
            pl.status.zero_()
            pl.status_host.zero_()
            torch.cuda.synchronize(pl.device)

    def _check_decoded(self, groups, plan_of):
        """decompress_batch's last step: every group's decode has been queued (its status word travels to pinned memory behind its
        tail segment); wait for the caller's stream -- which waits for the groups' -- and raise if a NaN / inf reached a prior
        parameter or the reconstruction.  The reference's protocol synchronises right after decompress() anyway
        (scripts/speedtest-lvae.py:34-36), so this costs nothing there; the reconstruction is never handed on unchecked."""
        torch.cuda.current_stream(self._dummy.device).synchronize()
        err = None
        for g, (_start, n) in enumerate(groups):
            try:
                plan_of(g, n).raise_if_flagged(where='while decoding')
            except ArithmeticError as e:                   # clear every group's word before raising
                err = err or e
        if err is not None:
            raise err

    # ---- 8-bit images in and out (lvae/utils/image.py, csrc/image_io.hip): the file formats of compress_file / decompress_file as bytes
    variable_rate = False                 # compress_batch takes `lmb`

    def _pack_blob(self, body, size):
        """One compress_batch result + the image's own (h, w) -> the bytes compress_file writes (the model's container)."""
        raise NotImplementedError

    def _unpack_blob(self, blob):
        """Inverse of _pack_blob: (decompress_batch input, (h, w), a key that blobs of one decompress_batch call share)."""
        raise NotImplementedError

    @staticmethod
    def _load_input(dst, im, u8, start, n):
        """Images start .. start + n of a compress_batch call -> `dst`, an (n, 3, H, W) view of an encode plan's input, on the current
        stream: a copy of the fp32 rows of `im`, or -- `u8`, a utils.image.U8Batch -- the conversion kernel writing there directly."""
        if u8 is not None:
            u8.fill(dst, start, n)
        else:
            dst.copy_(im[start:start + n])

    @torch.no_grad()
    def compress_images(self, images, lmb=None):
        """A list of (h, w, 3) uint8 images -- tensors on the CPU or the model's device, numpy arrays, PIL images -- whose sizes PADDED to
        multiples of max_stride agree (their own sizes may differ) -> list of bytes, element i being exactly the file compress_file
        writes for image i.  lmb: as in compress_batch (variable-rate models only).  The bytes of each image go to the device as they
        are (3 per pixel, unpadded); padding and the division by 255 happen where each pipeline group's plan reads its input."""
        from ..utils.image import U8Batch
        return self._compress_byte_batch(U8Batch(images, self.max_stride, self._dummy.device), lmb, 'compress_images')

    def _compress_byte_batch(self, batch, lmb, who):
        """compress_batch on a batch of 8-bit inputs (utils.image.U8Batch, utils.yuv.Yuv420Batch / YuvBatch: `.shape`, `.sizes`, `.device`, `.fill`)
        -> the models' containers, one per input."""
        _, _, H, W = batch.shape
        d = self.max_stride
        assert all((d * math.ceil(h / d), d * math.ceil(w / d)) == (H, W) for h, w in batch.sizes), f'{who}: padded sizes differ'
        if self.variable_rate:
            bodies = self.compress_batch(None, lmb=lmb, u8=batch)
        else:
            if lmb is not None:
                raise ValueError(f'{type(self).__name__} is a fixed-rate model: it takes no lmb')
            bodies = self.compress_batch(None, u8=batch)
        return [self._pack_blob(body, size) for body, size in zip(bodies, batch.sizes)]

    def _decompress_blobs(self, blobs, convert):
        """Blobs -> convert(decompress_batch's (n, 3, H, W) output, [(h, w)]) per group of blobs that share a latent shape, in input order."""
        parsed = [self._unpack_blob(b) for b in blobs]
        by_key = {}
        for i, (_, _, key) in enumerate(parsed):
            by_key.setdefault(key, []).append(i)
        out = [None] * len(blobs)
        for idxs in by_key.values():
            x = self.decompress_batch([parsed[i][0] for i in idxs])
            for i, item in zip(idxs, convert(x, [parsed[i][1] for i in idxs])):
                out[i] = item
        return out

    # ---- 8-bit YUV 4:2:0 frames in and out (lvae/utils/yuv.py, csrc/yuv_io.hip): an image codec run as an intra-frame coder
    @torch.no_grad()
    def compress_yuv420(self, frames, lmb=None, matrix='bt709', range='limited', chroma='bilinear'):
        """A list of utils.yuv.Yuv420Frame (I420 or NV12 planes on the CPU or the model's device) whose sizes PADDED to multiples of
        max_stride agree -> list of bytes, element i being the model's own container: exactly the file compress_file would write for the
        RGB image utils.yuv.to_rgb01 gives for frame i.  lmb: as in compress_images.  The planes go to the device as they are (1.5 bytes
        per pixel); chroma upsampling ('nearest' | 'bilinear', centre siting), the matrix ('bt601' | 'bt709'), the range ('limited' |
        'full') and the padding happen where each pipeline group's plan reads its input.  The colour parameters are NOT stored in the
        stream -- the containers do not change -- so decompress_yuv420 has to be given the same matrix and range."""
        from ..utils.yuv import Yuv420Frame, _as_frames
        return self.compress_yuv(_as_frames(frames, Yuv420Frame), lmb, matrix, range, chroma)

    @torch.no_grad()
    def decompress_yuv420(self, blobs, fmt='i420', matrix='bt709', range='limited'):
        """compress_yuv420 (or compress_images / compress_file) bytes -> list of utils.yuv.Yuv420Frame of layout `fmt` on the model's device,
        each cropped to the size in its header (which must be even) and converted on the device (utils.yuv.from_rgb01: forward matrix,
        2x2 chroma mean, round-half-even).  matrix / range: the stream does not record them; pass what the encoder was given."""
        from ..utils.yuv import _check
        _check(matrix, range, fmt=fmt)
        return self.decompress_yuv(blobs, matrix=matrix, range=range, layout=fmt)

    # ---- THE pair for YUV frames of every kind (utils.yuv.FrameFormat): 8 / 10 / 12 bits at 4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar,
    # centre- or left-sited chroma; the 8-bit 4:2:0 pair above forwards here
    @torch.no_grad()
    def compress_yuv(self, frames, lmb=None, matrix='bt709', range='limited', chroma='bilinear', siting='center'):
        """compress_yuv420 for a list of utils.yuv.YuvFrame that share depth and subsampling and whose sizes PADDED to multiples of
        max_stride agree -> list of bytes, element i being the model's own container: the file compress_file would write for the RGB image
        utils.yuv.to_rgb01_any gives for frame i.  matrix: 'bt601' | 'bt709' | 'bt2020'; siting: 'center' | 'left' (H.264 / HEVC co-sited
        chroma).  The planes go to the device as their file holds them (1 or 2 bytes per sample).  Neither the colour parameters nor depth,
        subsampling and siting are stored in the stream: decompress_yuv has to be given the encoder's (compress_yuv_sequence stores them).
        A list of utils.yuv.YuvSpFrame (P010 / P012 / P210 / P212) is taken as well: its two planes are uploaded as they are and each
        pipeline group's plan input is filled by lvae_image_yuvsp_to_f32, so the blobs are byte for byte those of the frames' to_planar().
        So is a list of utils.yuv.Yuv420Frame (what compress_yuv420 passes on), which takes siting='center' and no 'bt2020'.  Frames of
        different kinds may not be mixed in one call."""
        from ..utils.yuv import FrameFormat
        frames, fmt = FrameFormat.shared(frames, 'compress_yuv')
        return self._compress_byte_batch(fmt.batch(frames, self.max_stride, self._dummy.device, matrix, range, chroma, siting), lmb, 'compress_yuv')

    @torch.no_grad()
    def decompress_yuv(self, blobs, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar'):
        """compress_yuv (or compress_images / compress_file) bytes -> list of utils.yuv.YuvFrame of `depth` and `subsampling` on the
        model's device, each cropped to the size in its header and converted on the device (utils.yuv.from_rgb01_any).  A depth above 8
        keeps precision of the fp32 reconstruction that 8-bit codes drop.  ValueError: a header's size does not fit the subsampling.
        depth / siting / matrix / range: the stream does not record them; pass what the encoder was given.  layout 'semiplanar' (depth
        10 | 12, subsampling '420' | '422'): utils.yuv.YuvSpFrames holding the same codes, written in that layout by the kernel.  layout
        'i420' | 'nv12' (depth 8, '420', 'center', no 'bt2020'): utils.yuv.Yuv420Frames, what decompress_yuv420 returns."""
        from ..utils.yuv import _check2, _extent_ok, check_layout, from_rgb01_any
        _check2(range=range)
        check_layout(layout, depth, subsampling, siting, matrix)
        for i, b in enumerate(blobs):
            h, w = self._unpack_blob(b)[1]
            if not _extent_ok(h, w, subsampling):
                raise ValueError(f'decompress_yuv: blob {i} holds a {h} x {w} image, which does not fit subsampling {subsampling}')
        conv = lambda x, sizes: from_rgb01_any(x, sizes, depth=depth, subsampling=subsampling, siting=siting, matrix=matrix, range=range,
                                               layout=layout)
        return self._decompress_blobs(blobs, conv)

    # ---- self-describing YUV sequences (lvae/utils/yuvseq.py: the `LVYS` container around the frames' unchanged blobs)
    @property
    def _registry_name(self):
        """The name get_model built this model under (the class's name for a model built by hand): what a sequence container records."""
        return getattr(self, 'model_name', None) or type(self).__name__

    @torch.no_grad()
    def compress_yuv_sequence(self, frames_or_path, width=None, height=None, depth=8, subsampling='420', layout='planar', siting='center',
                              matrix='bt709', range='limited', chroma='bilinear', frames=None, lmb=None, max_batch=8, tile=None, overlap=0,
                              scale=None, size=None, filter='lanczos3'):
        """A sequence of frames -> the bytes of one self-describing container (utils.yuvseq.pack_sequence).  frames_or_path: a list of
        frames of ONE kind and size -- utils.yuv.YuvFrame, YuvSpFrame or Yuv420Frame; depth, subsampling and layout are then the frames' --
        or the path of a raw file of `width` x `height` frames of `depth`, `subsampling` and `layout` ('planar' | 'semiplanar' | 'i420' |
        'nv12'), of which `max_batch` at a time are read, uploaded and coded (all of them, or the first `frames`).  Frame k's blob is
        compress_yuv([frame k], ...)[0], whatever max_batch: batch rows are bit-equal to single calls.
        lmb: None, one value or -- variable-rate models -- one value per frame.  The header records size, depth, subsampling, siting,
        matrix, range, chroma, the layout, this model's registry name and its GEMM precision: decompress_yuv_sequence needs nothing else.
        tile = (th, tw), overlap: every frame is coded in tiles and its entry is compress_yuv_tiled(frame k, tile, overlap, ...), a tiled
        container (the tiles of ONE frame then share a batch, `max_batch` at a time); the header does not change -- a frame's entry is
        opaque bytes behind the length table -- and with tile=None every byte is as before.
        scale or size = (h, w), filter: every frame is coded at reduced resolution and its entry is compress_yuv_scaled([frame k], ...)[0],
        a scaled container; again the header does not change, and with neither every byte is as before.  ValueError: both of them, or
        either together with tile."""
        from ..utils import resample, yuv, yuvseq
        scaled = scale is not None or size is not None
        if scaled:
            if tile is not None:
                raise ValueError('compress_yuv_sequence: scale / size and tile may not be combined (scaled and tiled coding are separate)')
            if scale is not None and size is not None:
                raise ValueError('compress_yuv_sequence: give one of scale and size, not both')
            resample._filter(filter)
        if lmb is not None and not self.variable_rate:
            raise ValueError(f'{type(self).__name__} is a fixed-rate model: it takes no lmb')
        if isinstance(frames_or_path, (str, os.PathLike)):
            if width is None or height is None:
                raise ValueError('compress_yuv_sequence: a raw file needs width and height')
            fmt = yuv.FrameFormat(layout, depth, subsampling, siting, matrix)
            path, limit = frames_or_path, None if frames is None else int(frames)
            per, nbytes = fmt.frame_bytes(width, height), os.path.getsize(path)
            if nbytes == 0 or nbytes % per:
                raise ValueError(f'compress_yuv_sequence: {path} holds {nbytes} bytes, not a whole number of {width}x{height} frames of {per} bytes')
            total = nbytes // per if limit is None else min(limit, nbytes // per)
            source = lambda start, n: fmt.read(path, width, height, frames=min(n, total - start), start=start) if start < total else []
        else:
            source, fmt = yuv.FrameFormat.shared(frames_or_path, 'compress_yuv_sequence')
            (height, width) = source[0].size
            if any(yuv.FrameFormat.of(f) != fmt or f.size != (height, width) for f in source):
                raise ValueError('compress_yuv_sequence: the frames of a sequence share one kind, one plane layout and one size')
            yuvseq.check_layout(*fmt, siting, matrix)
        compress = lambda chunk, **kw: self.compress_yuv(chunk, matrix=matrix, range=range, chroma=chroma, siting=siting, **kw)
        if scaled:
            resample.scaled_size(height, width, scale=scale, size=size)
            compress = lambda chunk, **kw: self.compress_yuv_scaled(chunk, scale=scale, size=size, filter=filter, matrix=matrix, range=range,
                                                                    chroma=chroma, siting=siting, **kw)
        if tile is not None:
            self._tile_args(tile, overlap)

            def compress(chunk, lmb=None):
                per = lmb if isinstance(lmb, list) else [lmb] * len(chunk)
                return [self.compress_yuv_tiled(f, tile=tile, overlap=overlap, lmb=v, max_batch=max_batch, matrix=matrix, range=range,
                                                chroma=chroma, siting=siting) for f, v in zip(chunk, per)]
        blobs = yuvseq.code_sequence(compress, source, max_batch, lmb)
        meta = dict(fmt._asdict(), width=width, height=height, siting=siting, matrix=matrix, range=range, chroma=chroma,
                    model=self._registry_name, gemm=self._prec)
        return yuvseq.pack_sequence(meta, blobs)

    def yuv_sequence_info(self, blob):
        """utils.yuvseq.yuv_sequence_info (header parsing only, no GPU) plus 'lmb': the frames' lambdas from their blobs' own headers on
        variable-rate models (as tiled_info), else None; a frame that was coded in tiles has tiled_info's (rows, cols) nested list, one
        coded at reduced resolution the lambda of its payload (scaled_info)."""
        from ..utils import resample, tiling, yuvseq
        info = yuvseq.yuv_sequence_info(blob)
        lmb_of = lambda fb: (self.tiled_info(fb)['lmb'] if tiling.is_tiled(fb) else self.scaled_info(fb)['lmb'] if resample.is_scaled(fb)
                             else self._blob_lmb(fb))
        info['lmb'] = [lmb_of(yuvseq.frame_blob(blob, info, k)) for k in range(info['frames'])] if self.variable_rate else None
        return info

    @torch.no_grad()
    def decompress_yuv_sequence(self, blob, frames=None, layout=None, out_path=None, max_batch=8):
        """A compress_yuv_sequence container -> its frames on the model's device, with NO colour parameter: size, depth, subsampling, siting,
        matrix and range come from the header.  frames: None (all), a range or a list of indexes -- only those blobs are read, through the
        length table, and decoded, `max_batch` at a time.  layout: None = the source's; 'planar' (YuvFrame), 'semiplanar' (YuvSpFrame) or,
        for 8-bit 4:2:0 centre-sited sequences, 'i420' / 'nv12' (Yuv420Frame).  out_path: write the frames to that raw file instead and
        return their number.  ValueError: a malformed container (utils.yuvseq.yuv_sequence_info), a header whose model name or GEMM
        precision is not this model's (both names are in the message; set_gemm_precision selects the arithmetic), a layout the header's
        parameters do not have.  A frame entry that is a tiled container (compress_yuv_sequence(tile=...)) is recognised by its magic and
        decoded by decompress_yuv_tiled; one that is a scaled container (compress_yuv_sequence(scale=...)) likewise, by
        decompress_yuv_scaled, at the sequence's frame size."""
        from ..utils import resample, tiling, yuv, yuvseq
        info = yuvseq.yuv_sequence_info(blob)
        if info['model'] != self._registry_name:
            raise ValueError(f"decompress_yuv_sequence: the sequence was written by model {info['model']!r}, this model is {self._registry_name!r}")
        if info['gemm'] != self._prec:
            raise ValueError(f"decompress_yuv_sequence: the sequence was written under GEMM precision {info['gemm']!r}, this model runs "
                             f"{self._prec!r}; call set_gemm_precision({info['gemm']!r}) first")
        how = {k: info[k] for k in ('depth', 'subsampling', 'siting', 'matrix', 'range')}
        how['layout'] = info['layout'] if layout is None else layout
        yuvseq.check_layout(**{k: v for k, v in how.items() if k != 'range'})
        decode = lambda bl: self.decompress_yuv(bl, **how)
        decode_tiled = lambda b: self.decompress_yuv_tiled(b, max_batch=max_batch, **how)
        idxs, step, out = yuvseq.frame_indexes(info, frames), max(1, int(max_batch)), []
        for o in range(0, len(idxs), step):
            entries = [yuvseq.frame_blob(blob, info, k) for k in idxs[o:o + step]]
            whole = [b for b in entries if not tiling.is_tiled(b) and not resample.is_scaled(b)]
            small = [b for b in entries if resample.is_scaled(b)]
            got, got_small = iter(decode(whole) if whole else []), iter(self.decompress_yuv_scaled(small, **how) if small else [])
            # a frame coded in tiles: a tiled container; one coded at reduced resolution: a scaled container
            got = [decode_tiled(b) if tiling.is_tiled(b) else next(got_small) if resample.is_scaled(b) else next(got) for b in entries]
            for f in got:
                if f.size != (info['height'], info['width']):
                    raise ValueError(f"YUV sequence container: a frame holds {f.size[1]} x {f.size[0]} pixels, the header says {info['width']} x {info['height']}")
            if out_path is None:
                out += got
            else:
                yuv.write_frames(got, out_path, append=o > 0)
        return out if out_path is None else len(idxs)

    @torch.no_grad()
    def decompress_images(self, blobs):
        """compress_images / compress_file bytes -> list of (h, w, 3) uint8 tensors on the model's device, each cropped to the size in
        its header and rounded on the device (round-half-even of x * 255).  Blobs that share a latent shape are decoded as one batch."""
        from ..utils.image import to_u8
        return self._decompress_blobs(blobs, to_u8)

    @torch.no_grad()
    def decompress_to_files(self, bits_paths, image_paths):
        """Files written by compress_file(s) -> PNGs: decompress_images, one device-to-host copy of h * w * 3 bytes per image, save_u8."""
        from ..utils.image import save_u8
        blobs = []
        for p in bits_paths:
            with open(p, 'rb') as f:
                blobs.append(f.read())
        ims = self.decompress_images(blobs)
        host = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True).copy_(t, non_blocking=True) for t in ims]
        torch.cuda.current_stream(self._dummy.device).synchronize()
        for t, p in zip(host, image_paths):
            save_u8(t, p)

    def _compress_to_files(self, images, output_paths, lmb=None):
        for blob, out in zip(self.compress_images(images, lmb=lmb), output_paths):
            with open(out, 'wb') as f:
                f.write(blob)

    # ---- rate maps (csrc/rate_map.hip): where an image's estimated bits go
    LOG2E = 1.4426950408889634            # the fp64 constant of lvae_rate_map_f32

    @staticmethod
    def _run_with_pos(pl, cdf_form, upto=None):
        """Replay a plan that owns `pos_bufs` (CodecPlan.alloc_pos) on the current stream with lvae_gaussian_nll_pos_f32 behind each latent
        block's quantize launch (pl.qcuts), where the per-channel kernel of the eval plans stands: the scratch `prm` still holds that
        block's prior there.  The position kernel has no lvae_op kind (the table of kinds is pinned at its 26 rows), so the plan is
        replayed as one native range per block -- len(qcuts) + 1 lvae_run_ops calls in place of one -- with the kernel launched between
        them, on the same stream (a side-stream prior head of the next block is forked behind it).  upto: the op index the replay stops
        at behind the last block's position kernel (None: the plan's end; pl.qcuts[-1]: nothing more)."""
        lib = pl.lib
        st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
        lo = 0
        for li, cut in enumerate(pl.qcuts):
            pl.run(lo, cut)
            lo = cut
            z, hw = pl.lat_shapes[li]
            _native.check(lib.lvae_gaussian_nll_pos_f32(pl.prm_bufs[li].data_ptr(), pl.sym_all.data_ptr() + 4 * pl.sym_off[li],
                                                        pl.pos_bufs[li].data_ptr(), pl.pk.scale_bound, pl.B, hw, z, cdf_form, st),
                          'lvae_gaussian_nll_pos_f32')
        if upto is None or upto > lo:
            pl.run(lo, upto)

    def _rate_map_run(self, im, u8, B, H, W, lmb, return_rec):
        """The model's part of rate_map: load the input (_load_input), run its position plan and -- return_rec -- what forward() runs for
        im_hat, raise as forward() does.  -> (the plan that owns pos_bufs / lat_hw, the pixel stage's (B*H*W,) fp64 map or None, im_hat
        (B, 3, H, W) or None)."""
        raise NotImplementedError

    @torch.no_grad()
    @on_model_device
    def rate_map(self, im, lmb=None, blocks=False, return_rec=False):
        """Where an image's bits go: the eval-mode rate estimate of forward() kept per pixel.  im: a (B, 3, H, W) fp32 tensor in [0, 1]
        with H, W multiples of max_stride (forward()'s contract: AssertionError outside [0, 1], NonFiniteError), or a list of (h, w, 3)
        uint8 images of one padded size (whatever compress_images takes; uploaded and replicate-padded by the same path).  lmb:
        variable-rate models only (None = default_lmb, a number, or one per image); the others raise TypeError.
        -> a (B, 1, H, W) fp32 tensor on the model's device in BITS PER PIXEL AT THAT PIXEL -- each latent block's position-wise rate
        (lvae_gaussian_nll_pos_f32) spread over the s x s pixels a position stands for, blocks added in order, then the lossless model's
        pixel stage (lvae_rate_map_f32: fp64, rounded to fp32 once; one launch for the batch) -- so map.sum() is the image's estimated
        size in bits.  The list form returns a list of (1, h, w) tensors, each written at its image's own size by the kernel (the
        padding's bits are left out): the crops differ between images, so there it is one lvae_rate_map_f32 launch per image.
        blocks=True: also a list with one (B, h_i, w_i) fp64 tensor per latent block, in nats (the lossless model appends its (B, H, W)
        pixel stage).  return_rec=True: also im_hat, the bits of forward(..., return_rec=True)['im_hat'] (list form: (3, h, w) crops).
        Deterministic: two calls return the same bits; on variable-rate models row i of a batch with per-image lambdas is the single call."""
        if lmb is not None and not self.variable_rate:
            raise TypeError(f'{type(self).__name__} is a fixed-rate model: rate_map takes no lmb')
        u8 = None
        if isinstance(im, (list, tuple)):
            from ..utils.image import U8Batch
            u8 = U8Batch(im, self.max_stride, self._dummy.device)
            B, _, H, W = u8.shape
            d = self.max_stride
            assert all((d * math.ceil(h / d), d * math.ceil(w / d)) == (H, W) for h, w in u8.sizes), 'rate_map: padded sizes differ'
            im = None
        else:
            im = im.to(self._dummy.device)
            assert im.dim() == 4 and im.shape[1] == 3 and im.dtype == torch.float32 and not im.requires_grad, f'{im.shape=}'
            B, _, H, W = im.shape
        assert H % self.max_stride == 0 and W % self.max_stride == 0, f'{(B, 3, H, W)=}'
        pl, pix, im_hat = self._rate_map_run(im, u8, B, H, W, lmb, return_rec)
        n = len(pl.pos_bufs)
        lat_h = (ctypes.c_int * n)(*[h for h, _ in pl.lat_hw])
        lat_w = (ctypes.c_int * n)(*[w for _, w in pl.lat_hw])
        lib = _native.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream(pl.device).cuda_stream)
        dev = pl.device

        def compose(out, b0, nb, row, ch, cw):
            pos = (ctypes.c_void_p * n)(*[t.data_ptr() + 8 * b0 * h * w for t, (h, w) in zip(pl.pos_bufs, pl.lat_hw)])
            _native.check(lib.lvae_rate_map_f32(pos, lat_h, lat_w, n, None if pix is None else pix.data_ptr() + 8 * b0 * H * W, nb, H, W,
                                                out.data_ptr(), ch * row, row, ch, cw, st), 'lvae_rate_map_f32')

        if u8 is None:
            out = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
            compose(out, 0, B, W, H, W)
        else:
            out = [torch.empty(1, h, w, dtype=torch.float32, device=dev) for h, w in u8.sizes]
            for b, (h, w) in enumerate(u8.sizes):
                compose(out[b], b, 1, w, h, w)
            if im_hat is not None:
                im_hat = [im_hat[b, :, :h, :w].clone() for b, (h, w) in enumerate(u8.sizes)]
        res = [out]
        if blocks:
            res.append([t.view(B, h, w).clone() for t, (h, w) in zip(pl.pos_bufs, pl.lat_hw)] + ([pix.view(B, H, W).clone()] if pix is not None else []))
        if return_rec:
            res.append(im_hat)
        return res[0] if len(res) == 1 else tuple(res)

    # ---- tiled coding of large images (lvae/utils/tiling.py: grid, weights, container; csrc/tile_stitch.hip: the blend).  A tile's bytes
    # are exactly compress_images' for that crop, so the streams of the models do not change; all tiles of an image share one shape,
    # hence one launch plan, and activation memory follows the tile and max_batch, not the image.
    def _blob_lmb(self, blob):
        """The lambda a compress_images blob was coded at (variable-rate models; header parsing only)."""
        return None

    def _tile_args(self, tile, overlap):
        th, tw = (int(v) for v in tile)
        d = self.max_stride
        if th <= 0 or tw <= 0 or th % d or tw % d:
            raise ValueError(f'tile {(th, tw)}: both sides must be positive multiples of max_stride = {d}')
        return th, tw, int(overlap)

    @torch.no_grad()
    def compress_tiled(self, image, tile=(512, 768), overlap=0, lmb=None, max_batch=8):
        """One (h, w, 3) uint8 image (anything compress_images takes) -> the bytes of a tiled container (utils.tiling.pack_tiled).  The
        image is uploaded once; its tiles (utils.tiling.tile_grid) are views of it, coded `max_batch` at a time through compress_images,
        so tile k's blob is compress_images([image[y:y + th, x:x + tw]])[0].  tile: (th, tw), multiples of max_stride; overlap: pixels
        neighbouring tiles share (blended on decode).  lmb: None, a number or -- variable-rate models -- a (rows, cols) array with one
        lambda per tile; fixed-rate models raise ValueError on anything but None."""
        from ..utils import tiling
        from ..utils.image import _as_u8
        th, tw, overlap = self._tile_args(tile, overlap)
        if lmb is not None and not self.variable_rate:
            raise ValueError(f'{type(self).__name__} is a fixed-rate model: it takes no lmb')
        img = _as_u8(image).to(self._dummy.device, non_blocking=True)
        h, w = int(img.shape[0]), int(img.shape[1])
        ys, xs = tiling.tile_grid(h, w, th, tw, overlap)
        views = [img[y:y + th, x:x + tw] for y in ys for x in xs]
        return tiling.pack_tiled(h, w, th, tw, overlap, self._code_tiles(self.compress_images, views, len(ys), len(xs), lmb, max_batch))

    def _code_tiles(self, compress, views, rows, cols, lmb, max_batch):
        """The tiles of a rows x cols grid (row-major `views`) -> their blobs, `max_batch` at a time through compress(chunk, lmb=...).
        lmb: None, a number or a (rows, cols) array."""
        lmbs = None
        if lmb is not None and not isinstance(lmb, (int, float)):
            lmbs = np.asarray(lmb.detach().cpu() if isinstance(lmb, torch.Tensor) else lmb, dtype=np.float64)
            if lmbs.ndim == 0:
                lmb, lmbs = float(lmbs), None
            elif lmbs.shape != (rows, cols):
                raise ValueError(f'lmb map of shape {lmbs.shape} for a {rows} x {cols} tile grid')
            else:
                lmbs = lmbs.reshape(-1).tolist()
        blobs, step = [], max(1, int(max_batch))
        for o in range(0, len(views), step):
            kw = {} if lmb is None else {'lmb': lmbs[o:o + step] if lmbs is not None else lmb}
            blobs += compress(views[o:o + step], **kw)
        return blobs

    def tiled_info(self, blob):
        """Header parsing only (no GPU): dict(h, w, tile, overlap, rows, cols, ys, xs, lengths, lmb) of a tiled container; lmb: the
        (rows, cols) nested list of the tiles' lambdas on variable-rate models, else None."""
        from ..utils import tiling
        c = tiling.unpack_tiled(blob)
        lm = None
        if self.variable_rate:
            flat = [self._blob_lmb(t) for t in c['tiles']]
            lm = [flat[r * c['cols']:(r + 1) * c['cols']] for r in range(c['rows'])]
        return dict(h=c['h'], w=c['w'], tile=(c['th'], c['tw']), overlap=c['overlap'], rows=c['rows'], cols=c['cols'], ys=c['ys'], xs=c['xs'],
                    lengths=c['lengths'], lmb=lm)

    @torch.no_grad()
    def _decode_tiles(self, blob, box, max_batch, before=0):
        """The tile loop of every tiled decode: the tiles of a container that meet box = (y0, x0, hh, ww) (None: the image; `before`: the
        box widened by that many columns on the left, for this purpose only), decoded `max_batch` at a time -> (the arguments of
        stitch_tiles / stitch_tiles_yuv up to the box: tiles with None for those not decoded, h, w, th, tw, overlap; the box as ints)."""
        from ..utils import tiling
        c = tiling.unpack_tiled(blob)
        h, w, th, tw = c['h'], c['w'], c['th'], c['tw']
        self._tile_args((th, tw), c['overlap'])
        if box is None:
            box = (0, 0, h, w)
        y0, x0, hh, ww = (int(v) for v in box)
        if y0 < 0 or x0 < 0 or hh <= 0 or ww <= 0 or y0 + hh > h or x0 + ww > w:
            raise ValueError(f'box {(y0, x0, hh, ww)} is not inside the {h} x {w} image')
        d = self.max_stride
        eth, etw = min(th, d * math.ceil(h / d)), min(tw, d * math.ceil(w / d))      # what a tile's reconstruction holds
        xl = max(x0 - before, 0)
        need = tiling.tiles_in_box(c['ys'], c['xs'], th, tw, (y0, xl, hh, x0 + ww - xl))
        tiles, step = [None] * len(c['tiles']), max(1, int(max_batch))
        for o in range(0, len(need), step):
            idxs = need[o:o + step]
            parsed = [self._unpack_blob(c['tiles'][k]) for k in idxs]
            for k, (_, size, _) in zip(idxs, parsed):
                if tuple(size) != (min(h, th), min(w, tw)):
                    raise ValueError(f'tiled container: tile {k} holds {tuple(size)} pixels, the grid says {(min(h, th), min(w, tw))}')
            x = self.decompress_batch([p[0] for p in parsed])
            if tuple(x.shape[1:]) != (3, eth, etw):
                raise ValueError(f'tiled container: tiles decode to {tuple(x.shape[2:])}, the header says {(eth, etw)}')
            for i, k in enumerate(idxs):
                tiles[k] = x[i]
        return (tiles, h, w, eth, etw, c['overlap']), (y0, x0, hh, ww)

    def _decode_tiled(self, blob, box, out, max_batch):
        from ..utils.image import stitch_tiles
        if out not in ('u8', 'f32'):
            raise ValueError(f"out is 'u8' or 'f32', got {out!r}")
        args, box = self._decode_tiles(blob, box, max_batch)
        return stitch_tiles(*args, box=box, out=out)

    def decompress_tiled(self, blob, out='u8', max_batch=8):
        """compress_tiled bytes -> the (h, w, 3) uint8 image on the model's device, or (out='f32') the (1, 3, h, w) fp32 one: tiles decoded
        `max_batch` at a time with decompress_batch, overlaps blended and rounded on the device (lvae_tile_stitch)."""
        return self._decode_tiled(blob, None, out, max_batch)

    def decompress_region(self, blob, box, out='u8', max_batch=8):
        """box = (y0, x0, hh, ww) of a tiled image: only the tiles that intersect the box are decoded and only the window is stitched;
        equal to decompress_tiled(blob)[y0:y0 + hh, x0:x0 + ww]."""
        return self._decode_tiled(blob, box, out, max_batch)

    # ---- tiled coding of YUV frames: the tiles are views of the frame's planes on the way in (the YUV kernels read any row stride), and
    # the blend of the decoded tiles writes YUV planes on the way out (csrc/tile_stitch_yuv.hip).  The container is compress_tiled's.
    @torch.no_grad()
    def compress_yuv_tiled(self, frame, tile=(512, 768), overlap=0, lmb=None, max_batch=8, matrix='bt709', range='limited', chroma='bilinear',
                           siting='center'):
        """One utils.yuv.YuvFrame, YuvSpFrame or Yuv420Frame -> the bytes of a tiled container (utils.tiling.pack_tiled, as compress_tiled).
        The frame is uploaded once; its tiles (utils.tiling.tile_grid) are frames whose planes are views of its planes, coded `max_batch`
        at a time through compress_yuv, so tile k's blob is compress_yuv([that crop as a frame])[0].
        tile, lmb, max_batch: as in compress_tiled.  overlap: even where the chroma is subsampled (both axes at '420', the width at
        '422'), so that every tile starts on the chroma grid -- ValueError otherwise.  matrix .. siting: as in compress_yuv; a Yuv420Frame
        takes siting='center' only.  Neither the colour parameters nor depth, subsampling and siting are stored."""
        from ..utils import tiling, yuv
        th, tw, overlap = self._tile_args(tile, overlap)
        if lmb is not None and not self.variable_rate:
            raise ValueError(f'{type(self).__name__} is a fixed-rate model: it takes no lmb')
        fmt = yuv.FrameFormat.of(frame)
        yuv.check_layout(*fmt, siting, matrix)
        if overlap % 2 and yuv.SHIFTS[fmt.subsampling][0]:
            raise ValueError(f'compress_yuv_tiled: overlap {overlap} is odd: tiles of a {fmt.subsampling} frame start on the chroma grid, so '
                             'the overlap is even')
        h, w = frame.size
        ys, xs = tiling.tile_grid(h, w, th, tw, overlap)
        fr = frame.to(self._dummy.device, non_blocking=True)
        compress = lambda chunk, **kw: self.compress_yuv(chunk, matrix=matrix, range=range, chroma=chroma, siting=siting, **kw)
        views = [fmt.crop(fr, y, x, th, tw) for y in ys for x in xs]
        return tiling.pack_tiled(h, w, th, tw, overlap, self._code_tiles(compress, views, len(ys), len(xs), lmb, max_batch))

    def _decode_yuv_tiled(self, blob, box, depth, subsampling, siting, matrix, range, layout, max_batch):
        from ..utils import tiling, yuv
        who = 'decompress_yuv_tiled' if box is None else 'decompress_yuv_region'
        yuv._check2(range=range)
        yuv.check_layout(layout, depth, subsampling, siting, matrix)
        c = tiling.unpack_tiled(blob)
        if not yuv._extent_ok(c['h'], c['w'], subsampling):
            raise ValueError(f"{who}: the container holds a {c['h']} x {c['w']} image, which does not fit subsampling {subsampling}")
        if box is not None:
            yuv.check_chroma_box(tuple(int(v) for v in box), subsampling, who)
        args, box = self._decode_tiles(blob, box, max_batch, before=1 if siting == 'left' and yuv.SHIFTS[subsampling][0] else 0)
        return yuv.stitch_tiles_yuv(*args, box=box, depth=depth, subsampling=subsampling, siting=siting, matrix=matrix, range=range, layout=layout)

    def decompress_yuv_tiled(self, blob, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar', max_batch=8):
        """compress_yuv_tiled (or compress_tiled) bytes -> the frame on the model's device: tiles decoded `max_batch` at a time with
        decompress_batch, then blended, converted and written as YUV planes by one kernel (utils.yuv.stitch_tiles_yuv) -- the bits of
        utils.yuv.from_rgb01_any on decompress_tiled(blob, out='f32'), without that image.  depth .. range: as in decompress_yuv, the
        container does not record them; layout: 'planar' (YuvFrame), 'semiplanar' (YuvSpFrame), 'i420' / 'nv12' (Yuv420Frame)."""
        return self._decode_yuv_tiled(blob, None, depth, subsampling, siting, matrix, range, layout, max_batch)

    def decompress_yuv_region(self, blob, box, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar',
                              max_batch=8):
        """box = (y0, x0, hh, ww) of a tiled frame, on the chroma grid (ValueError otherwise): only the tiles the box touches are decoded
        -- with siting='left' and x0 > 0 also those that hold column x0 - 1, which the first chroma column reads -- and only the window
        is written; equal, plane by plane, to the crop of decompress_yuv_tiled's frame."""
        return self._decode_yuv_tiled(blob, box, depth, subsampling, siting, matrix, range, layout, max_batch)

    def compress_file_tiled(self, img_path, out_path, tile=(512, 768), overlap=0, lmb=None, max_batch=8):
        blob = self.compress_tiled(img_path, tile=tile, overlap=overlap, lmb=lmb, max_batch=max_batch)
        with open(out_path, 'wb') as f:
            f.write(blob)
        return len(blob)

    def decompress_file_tiled(self, bits_path, png_path=None, box=None, out='u8', max_batch=8):
        """A compress_file_tiled file -> the image (box: a region of it) as decompress_tiled returns it; png_path: also written as a PNG."""
        from ..utils.image import save_u8
        with open(bits_path, 'rb') as f:
            blob = f.read()
        x = self._decode_tiled(blob, box, out, max_batch)
        if png_path is not None:
            save_u8(x if out == 'u8' else self._decode_tiled(blob, box, 'u8', max_batch), png_path)
        return x

    # ---- reduced-resolution coding (lvae/utils/resample.py: the resampler's definition and the `LVRS` container; csrc/resample.hip: the
    # kernels).  An image is resampled where the encode plan reads its input, coded at the smaller size by the unchanged path, and
    # resampled back from the decoder's padded batch where it lies; the payload is the model's own blob for the coded-resolution image.
    @torch.no_grad()
    def compress_scaled(self, images, scale=None, size=None, filter='lanczos3', lmb=None):
        """A list of (h, w, 3) uint8 images of ONE size (anything compress_images takes) -> list of bytes, one scaled container
        (utils.resample.pack_scaled) per image.  Exactly one of `scale` -- the coded size is (max(1, round(h * scale)), max(1, round(w *
        scale))) -- and `size` = (h, w) of the coded image; ValueError otherwise, or for a ratio outside [1/8, 8] on an axis.  The images are
        uploaded once, as bytes; lvae_resample_u8_to_f32 resamples them (`filter`: 'bilinear' | 'bicubic' | 'lanczos3'), clamped to [0, 1]
        and replicate-padded, into each pipeline group's plan input.  The payload is the blob of the model's float path on
        utils.image.resize(to_float01(img), coded size, clamp=True), replicate-padded -- the resampled image is never rounded to bytes;
        with scale=1.0 it is compress_images' bytes.
        lmb: as in compress_images."""
        from ..utils import resample
        from ..utils.image import ScaledU8Batch, _as_u8
        resample._filter(filter)
        ts = [_as_u8(im) for im in images]
        if not ts:
            raise ValueError('compress_scaled: no images')
        h, w = int(ts[0].shape[0]), int(ts[0].shape[1])
        coded = resample.scaled_size(h, w, scale=scale, size=size)
        batch = ScaledU8Batch(ts, coded, filter, self.max_stride, self._dummy.device)
        return [resample.pack_scaled(filter, (h, w), coded, blob) for blob in self._compress_byte_batch(batch, lmb, 'compress_scaled')]

    def scaled_info(self, blob):
        """utils.resample.scaled_info (header parsing only, no GPU) plus 'lmb': the lambda the payload was coded at on variable-rate
        models, else None."""
        from ..utils import resample
        info, payload = resample.unpack_scaled(blob)
        info['lmb'] = self._blob_lmb(payload) if self.variable_rate else None
        return info

    @torch.no_grad()
    def decompress_scaled(self, blobs, out='u8', size=None):
        """compress_scaled containers -> the images at their ORIGINAL sizes, on the model's device: out='u8': (h, w, 3) uint8 tensors
        (rint(clamp(v, 0, 1) * 255), ties to even); out='f32': (1, 3, h, w) fp32 tensors, not clamped.  size: None, 'coded' (the coded
        image, no resampling: decompress_images of the payload for out='u8') or (h, w), a preview at that size.  Payloads of one latent
        shape decode as one batch, and the containers' filters resample the decoder's padded batch in place (lvae_resample_f32_to_u8 /
        lvae_resample_f32).  ValueError: a malformed container, a payload whose size is not the header's coded size."""
        from ..utils import resample
        from ..utils.image import _resample_f32, to_u8
        if out not in ('u8', 'f32'):
            raise ValueError(f"out is 'u8' or 'f32', got {out!r}")
        if size is not None and size != 'coded':
            size = tuple(int(v) for v in size)
            if len(size) != 2:
                raise ValueError(f"size is None, 'coded' or (h, w), got {size!r}")
        infos, bodies, groups = [], [], {}
        for i, b in enumerate(blobs):
            info, payload = resample.unpack_scaled(b)
            body, coded, key = self._unpack_blob(payload)
            if tuple(coded) != info['coded']:
                raise ValueError(f"scaled container {i}: the payload holds a {tuple(coded)} image, the header says {info['coded']}")
            if size not in (None, 'coded'):
                resample.check_ratio(info['coded'][0], size[0])
                resample.check_ratio(info['coded'][1], size[1])
            infos.append(info)
            bodies.append(body)
            groups.setdefault(key, []).append(i)           # as _decompress_blobs: payloads that share a latent shape are one batch
        result = [None] * len(blobs)
        for idxs in groups.values():
            x = self.decompress_batch([bodies[i] for i in idxs])
            if size == 'coded':
                coded = [infos[i]['coded'] for i in idxs]
                items = to_u8(x, coded) if out == 'u8' else [x[r:r + 1, :, :ch, :cw] for r, (ch, cw) in enumerate(coded)]
                for i, item in zip(idxs, items):
                    result[i] = item
                continue
            calls = {}                                     # one resampling call per (coded size, target size, filter) of the batch
            for r, i in enumerate(idxs):
                target = infos[i]['size'] if size is None else size
                calls.setdefault((infos[i]['coded'], target, infos[i]['filter']), []).append((r, i))
            for ((ch, cw), target, filt), rows in calls.items():
                got = _resample_f32([x[r, :, :ch, :cw] for r, _ in rows], target, filt, False, out)
                for k, (_, i) in enumerate(rows):
                    result[i] = got[k] if out == 'u8' else got[k:k + 1]
        return result

    # ---- YUV frames at reduced resolution: the two families above as one (csrc/resample_yuv.hip, utils.yuv.ScaledYuvBatch /
    # from_rgb01_scaled).  The container is the unchanged `LVRS` one, so scaled_info reads it as it is.
    @torch.no_grad()
    def compress_yuv_scaled(self, frames, scale=None, size=None, filter='lanczos3', lmb=None, matrix='bt709', range='limited', chroma='bilinear',
                            siting='center'):
        """compress_scaled for YUV frames: a list of frames of ONE kind and size (anything compress_yuv takes: utils.yuv.YuvFrame,
        YuvSpFrame or Yuv420Frame, on the CPU or the model's device) -> list of bytes, one scaled container (utils.resample.pack_scaled)
        per frame.  scale / size / filter / lmb: as in compress_scaled.  The planes go to the device as their file holds them and
        lvae_resample_yuv_to_f32 converts and resamples them into each pipeline group's plan input -- no full-resolution RGB image exists
        anywhere.  The payload is the model's own blob: that of the float path on
        utils.image.resize(utils.yuv.to_rgb01_any(frame), coded size, clamp=True), replicate-padded; with scale=1.0 it is compress_yuv's
        bytes.  The colour parameters, depth, subsampling and siting are NOT stored, as in compress_yuv: decompress_yuv_scaled has to be
        given them (compress_yuv_sequence(scale=...) stores them)."""
        from ..utils import resample
        from ..utils.yuv import FrameFormat
        resample._filter(filter)
        frames, fmt = FrameFormat.shared(frames, 'compress_yuv_scaled')
        h, w = frames[0].size
        coded = resample.scaled_size(h, w, scale=scale, size=size)
        batch = fmt.batch(frames, self.max_stride, self._dummy.device, matrix, range, chroma, siting, coded=coded, filter=filter)
        return [resample.pack_scaled(filter, (h, w), coded, blob) for blob in self._compress_byte_batch(batch, lmb, 'compress_yuv_scaled')]

    @torch.no_grad()
    def decompress_yuv_scaled(self, blobs, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar',
                              size=None):
        """compress_yuv_scaled (or compress_scaled) containers -> frames of the kind decompress_yuv's arguments name, on the model's device.
        size: None = each frame at its ORIGINAL size; 'coded' = the coded frame, no resampling (decompress_yuv of the payload); (h, w) = a
        preview at that size.  Payloads of one latent shape decode as one batch, and lvae_resample_f32_to_yuv resamples the decoder's
        padded batch, where it lies, straight into the planes: it equals
        utils.yuv.from_rgb01_any(decompress_scaled(blobs, out='f32', size=size), ...) plane by plane, with no fp32 image in between.
        ValueError: a malformed container, a payload whose size is not the header's coded size, a target size that does not fit the
        subsampling (the message names both), a layout these parameters do not have."""
        from ..utils import resample
        from ..utils.yuv import _check2, _extent_ok, check_layout, from_rgb01_any, from_rgb01_scaled
        _check2(range=range)
        check_layout(layout, depth, subsampling, siting, matrix)
        if size is not None and size != 'coded':
            size = tuple(int(v) for v in size)
            if len(size) != 2:
                raise ValueError(f"size is None, 'coded' or (h, w), got {size!r}")
        how = dict(depth=depth, subsampling=subsampling, siting=siting, matrix=matrix, range=range, layout=layout)
        infos, bodies, groups = [], [], {}
        for i, b in enumerate(blobs):
            info, payload = resample.unpack_scaled(b)
            body, coded, key = self._unpack_blob(payload)
            if tuple(coded) != info['coded']:
                raise ValueError(f"scaled container {i}: the payload holds a {tuple(coded)} image, the header says {info['coded']}")
            target = info['coded'] if size == 'coded' else info['size'] if size is None else size
            if not _extent_ok(target[0], target[1], subsampling):
                raise ValueError(f'decompress_yuv_scaled: container {i} is asked for a {target[0]} x {target[1]} frame, which does not fit '
                                 f'subsampling {subsampling}')
            if size != 'coded':
                resample.check_ratio(info['coded'][0], target[0])
                resample.check_ratio(info['coded'][1], target[1])
            infos.append(dict(info, target=tuple(target)))
            bodies.append(body)
            groups.setdefault(key, []).append(i)           # as _decompress_blobs: payloads that share a latent shape are one batch
        result = [None] * len(blobs)
        for idxs in groups.values():
            x = self.decompress_batch([bodies[i] for i in idxs])
            if size == 'coded':
                for i, item in zip(idxs, from_rgb01_any(x, [infos[i]['coded'] for i in idxs], **how)):
                    result[i] = item
                continue
            calls = {}                                     # one launch per (coded size, target size, filter) of the batch
            for r, i in enumerate(idxs):
                calls.setdefault((infos[i]['coded'], infos[i]['target'], infos[i]['filter']), []).append((r, i))
            for ((ch, cw), target, filt), rows in calls.items():
                got = from_rgb01_scaled([x[r, :, :ch, :cw] for r, _ in rows], target, filt, **how)
                for k, (_, i) in enumerate(rows):
                    result[i] = got[k]
        return result

    def compress_file_scaled(self, img_path, out_path, scale=None, size=None, filter='lanczos3', lmb=None):
        blob = self.compress_scaled([img_path], scale=scale, size=size, filter=filter, lmb=lmb)[0]
        with open(out_path, 'wb') as f:
            f.write(blob)
        return len(blob)

    def decompress_file_scaled(self, bits_path, png_path=None, out='u8', size=None):
        """A compress_file_scaled file -> the image as decompress_scaled returns it; png_path: also written as a PNG."""
        from ..utils.image import save_u8
        with open(bits_path, 'rb') as f:
            blob = f.read()
        x = self.decompress_scaled([blob], out=out, size=size)[0]
        if png_path is not None:
            save_u8(x if out == 'u8' else self.decompress_scaled([blob], out='u8', size=size)[0], png_path)
        return x

    # ---- the reference's single-image and file API, on the batch interfaces.  A variable-rate model adds `lmb` to the compress side
    @torch.no_grad()
    def compress(self, im):
        assert im.shape[0] == 1, 'use compress_batch for more than one image'
        return self.compress_batch(im)[0]

    @torch.no_grad()
    def decompress(self, compressed):
        return self.decompress_batch([compressed])

    @torch.no_grad()
    def compress_file(self, img_path, output_path):
        self._compress_to_files([img_path], [output_path])

    @torch.no_grad()
    def compress_files(self, img_paths, output_paths, images=None):
        """Batched compress_file (same padded size): one compress_batch call; files identical to compress_file's.  `images`: the files'
        contents, already decoded (PIL images or uint8 tensors)."""
        self._compress_to_files(images if images is not None else list(img_paths), output_paths)

    @torch.no_grad()
    def decompress_file(self, bits_path):
        return self.decompress_files([bits_path])[0]

    @torch.no_grad()
    def decompress_files(self, bits_paths):
        """Batched decompress_file for files of one latent shape -> list of (1,3,h,w) tensors, each cropped to the size in its header."""
        bodies, sizes = [], []
        for p in bits_paths:
            with open(p, 'rb') as f:
                body, size, _ = self._unpack_blob(f.read())
            bodies.append(body); sizes.append(size)
        out = self.decompress_batch(bodies)
        return [out[i:i + 1, :, :h, :w] for i, (h, w) in enumerate(sizes)]

    # ---- test access (not on the hot path)
    @torch.no_grad()
    def _trace(self, pl, B, full=False, force_z=None):
        """encode_trace() once the plan's input is loaded: per latent block dict(symbols, indexes), (B, z, hw) int arrays in the coder's
        NCHW raster order, from ONE run of the plan; full / force_z: _trace_blocks."""
        if full or force_z is not None:
            return self._trace_blocks(pl, B, force_z)
        pl.run()
        pl.fetch_status()
        torch.cuda.current_stream(pl.device).synchronize()
        pl.raise_if_flagged(where='(encode trace)')
        sym, idx = pl.sym_all.cpu().numpy(), pl.idx_all.cpu().numpy()
        return [dict(symbols=sym[o:o + B * z * hw].reshape(B, z, hw).copy(), indexes=idx[o:o + B * z * hw].reshape(B, z, hw).copy())
                for o, (z, hw) in zip(pl.sym_off, pl.lat_shapes)]

    @torch.no_grad()
    def _trace_blocks(self, pl, B, force_z=None):
        """Run an encode plan latent block by latent block (`pl.qcuts`: the op index right after each block's quantize launch)
        and copy out, per block, what the launches left in their buffers: symbols, indexes, pm, lv (the raw log-variance
        parameter, before softplus), qm -- numpy arrays shaped (B, z, hw) in the coder's NCHW raster order.  force_z[li], a
        (B, z, h, w) tensor or a pair (batch rows, (len(rows), z, h, w) tensor), overwrites the block's quantised latent before the
        blocks below it run (teacher forcing)."""
        out, lo = [], 0
        for li, cut in enumerate(pl.qcuts):
            pl.run(lo, cut)
            lo = cut
            pl.fetch_status()
            torch.cuda.synchronize(pl.device)
            pl.raise_if_flagged(where=f'(encode trace, latent block {li})')
            z, hw = pl.lat_shapes[li]
            M, o = B * hw, pl.sym_off[li]
            prm = pl.prm_bufs[li][:M * 2 * z].view(B, hw, 2 * z)
            nchw = lambda t: t.permute(0, 2, 1).contiguous().cpu().numpy()
            out.append(dict(symbols=pl.sym_all[o:o + M * z].view(B, z, hw).cpu().numpy(),
                            indexes=pl.idx_all[o:o + M * z].view(B, z, hw).cpu().numpy(),
                            pm=nchw(prm[:, :, :z]), lv=nchw(prm[:, :, z:]),
                            qm=nchw(pl.qm_bufs[li][:M * z].view(B, hw, z))))
            if force_z is not None and force_z[li] is not None:
                ld = pl.zhat_ld[li]
                rows, zt = force_z[li] if isinstance(force_z[li], tuple) else (list(range(B)), force_z[li])
                zt = zt.to(pl.device, torch.float32).reshape(len(rows), z, hw).permute(0, 2, 1)
                pl.zhat_bufs[li][:M * ld].view(B, hw, ld)[rows, :, :z] = zt
        torch.cuda.synchronize(pl.device)
        return out

    def _coder_threads_per_group(self, n_groups):
        if n_groups == 1:
            return self.coder_threads
        return max(1, (self.coder_threads or len(os.sched_getaffinity(0))) // n_groups)

    def _groups(self, B, kind=None):
        """Split a batch of B into contiguous groups [(start, size)] for the stream/thread pipeline."""
        want = {'enc': self.enc_groups, 'dec': self.dec_groups}.get(kind, 0) or self.pipeline_groups
        G = max(1, min(int(want), B))
        if B < 4:
            G = 1
        base, rem = divmod(B, G)
        out, o = [], 0
        for g in range(G):
            n = base + (1 if g < rem else 0)
            out.append((o, n))
            o += n
        return out

    def _run_groups(self, fn, groups):
        """Run fn(g, start, size, stream) for every group: inline for one group, else one host thread + HIP stream each."""
        dev = self._dummy.device
        while len(self._streams) < len(groups):
            self._streams.append(torch.cuda.Stream(device=dev))
        if len(groups) == 1:        # inline, but still on a side stream (the legacy default stream cannot be graph-captured)
            st, cur = self._streams[0], torch.cuda.current_stream(dev)
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                res = [fn(0, groups[0][0], groups[0][1], st)]
            cur.wait_stream(st)
            return res
        if self.serial_groups:
            cur, res = torch.cuda.current_stream(dev), []
            for g in range(len(groups)):
                st = self._streams[g]
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    res.append(fn(g, groups[g][0], groups[g][1], st))
                st.synchronize()
                cur.wait_stream(st)
            return res
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=8)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))        # lambda tables / inputs produced on the caller's stream

        def work(g):
            st = self._streams[g]
            st.wait_event(ev)
            with torch.cuda.stream(st):
                return fn(g, groups[g][0], groups[g][1], st)
        # the last group runs on the calling thread (no hand-over latency for it; the pool threads have theirs first)
        futs = [self._pool.submit(work, g) for g in range(len(groups) - 1)]
        res, err, last = [], None, None
        try:
            last = work(len(groups) - 1)
        except BaseException as e:                        # noqa: BLE001
            err = e
        for f in futs:                                    # every group finishes before an error is raised: the plans and streams
            try:                                          # of a failed call must be idle when the caller tries again
                res.append(f.result())
            except BaseException as e:                    # noqa: BLE001
                err = err or e
        res.append(last)
        if err is not None:
            raise err
        cur = torch.cuda.current_stream(dev)
        for g in range(len(groups)):                      # caller's stream sees the groups' results
            cur.wait_stream(self._streams[g])
        return res

