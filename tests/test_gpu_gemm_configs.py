"""-m gpu: every tile configuration of the fp32 / bf16 / bf16x3 GEMM family (csrc/gemm_f32.hip: 12 configurations x 3 arithmetics x 3
operand-A gather modes) and every store form of the shared epilogue (csrc/gemm_common.h: gemm_epilogue), at the ragged shapes of
tests/gemm_cases.py (whose arithmetic tests/test_gemm_cases_host.py checks without a GPU).

What is asserted.  The launch the library chooses itself (cfg = 0) is compared with an fp64 evaluation of the same product / convolution
and epilogue; every forced configuration (cfg = 1 .. lvae_gemm_num_configs()) must then equal that launch word for word -- the claim
of include/lvae_hip.h ("results are bit-identical for every choice") that the codec rests on, since encoder and decoder, batched and
single-image calls land on different configurations for the same layer.

Bounds (none taken from the code under test): prec 0: 2e-5 absolute on O(1) data, the bound of tests/test_gpu_kernels.py; prec 2:
error <= 2 x the prec 0 error + 1e-6, both measured here against the same fp64 reference (tests/test_gpu_bf16.py); prec 1: 3e-5
against the fp64 product of the bf16-rounded operands (tests/test_gpu_bf16.py); prec 4 (store forms only): 3e-5
(tests/test_gpu_f16x2.py).

prec 1 with GELU applied to A on load: the operand is bf16(gelu_f32(a)), and the reference is the fp64 product of bf16(gelu_f64(a)).
The two roundings can differ only where gelu_f64(a) lies within the fp32 GELU's error of a bf16 rounding midpoint; that error is at
most 2e-7 max(1, |a|) (tests/test_gpu_kernels.py::test_gelu_erf_accuracy asserts it of the device function; one fp32 ulp is added for
the conversions).  Such operands are found in fp64 (`Problem.flip_slack`): an output that reads none of them is held to 3e-5 like
every other prec 1 case, one that reads some is allowed, on top, sum_k |bf16 above - bf16 below| |w[n][k]| over exactly those
operands (x 1.13, the largest slope of GELU, behind a GELU epilogue).  A missing or misplaced GELU is an error of O(0.1) in every
output and fails either way.  The test prints how many operands are in doubt and how many outputs exceed 3e-5.

Outputs are prefilled with NaN and over-allocated by one row (and by ldo - N columns where the case pads): no NaN may be left inside,
every guard element must still be NaN.  Padding columns of A are NaN as well: a mis-strided operand read poisons the result."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc

pytestmark = pytest.mark.gpu

NAN = float('nan')
TOL = {0: 2e-5, 1: 3e-5, 2: 2e-5, 4: 3e-5}
ALL_CFGS = tuple(range(gc.NUM_CONFIGS + 1))             # 0 = the library's choice, then every forced configuration


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    lib = _native.lib()
    assert lib.lvae_gemm_num_configs() == gc.NUM_CONFIGS
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(L, **kw):
    """lvae_gemm_f32 with the given descriptor fields -> return code (no synchronisation)."""
    from lvae._native import GemmDesc
    d = GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    return L.lvae_gemm_f32(ctypes.byref(d), _st())


def _weights16(Wt, prec):
    from lvae.models.base import pack_bf16x3, pack_f16x2
    if prec == 1:
        return Wt.to(torch.bfloat16).contiguous()
    if prec == 2:
        return pack_bf16x3(Wt)
    if prec == 4:
        w = pack_f16x2(Wt)
        assert w is not None
        return w
    return None


def _epilogue64(acc, bias, gamma, res, epi):
    v = acc + bias.double()
    if epi == gc.EPI_BIAS_GELU:
        return F.gelu(v)
    if epi == gc.EPI_GAMMA_RES:
        return res.double() + gamma.double() * v
    if epi == gc.EPI_RES:
        return res.double() + v
    return v


def _assert_same_words(outs, names, rows, cols):
    """outs[1:] equal outs[0] as int32 words; one device reduction, details only on failure."""
    words = torch.stack([o.reshape(-1) for o in outs]).view(torch.int32)
    bad = (words[1:] != words[0]).sum(1).tolist()
    if any(bad):
        msg = []
        for i, n in enumerate(bad):
            if n:
                first = int((words[i + 1] != words[0]).nonzero()[0])
                msg.append(f'{names[i + 1]}: {n} words differ from {names[0]}, first at (row {first // cols}, column {first % cols})')
        raise AssertionError(f'{rows} x {cols}: ' + '; '.join(msg))


class Problem:
    """Inputs of one case on the GPU (built once), its fp64 reference, and launches into fresh NaN-filled outputs."""

    def __init__(self, c, seed):
        g = torch.Generator().manual_seed(seed)
        self.c = c
        M, N, K = c.M, c.N, c.K
        if c.a_mode == gc.A_PLAIN:
            self.A0 = torch.full((M, c.lda0), NAN)
            self.A0[:, :c.K0] = torch.randn(M, c.K0, generator=g)
            self.A1 = None
            if c.K1:
                self.A1 = torch.full((M, c.lda1), NAN)
                self.A1[:, :c.K1] = torch.randn(M, c.K1, generator=g)
                self.A1 = self.A1.cuda()
        elif c.a_mode == gc.A_PATCH2:
            self.A0, self.A1 = torch.randn(c.B, 2 * c.H, 2 * c.W, c.K0, generator=g), None
        else:
            self.A0, self.A1 = torch.randn(c.B, c.H, c.W, c.K0, generator=g), None
        self.A0 = self.A0.cuda()
        self.Wt = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
        self.bias, self.gamma = torch.randn(N, generator=g).cuda(), torch.rand(N, generator=g).cuda()
        self.res = torch.randn(M + 1, c.ldo, generator=g).cuda()
        self.W16 = {}

    def _product(self, a, W):
        """The case's linear operator in fp64: a = the A operand as stored ([M][K] columns of the sources, or the NHWC map), W [N][K]."""
        c = self.c
        if c.a_mode == gc.A_PLAIN:
            return a @ W.t()
        x = a.permute(0, 3, 1, 2)
        if c.a_mode == gc.A_PATCH2:      # K order (i, j, ci)
            y = F.conv2d(x, W.view(c.N, 2, 2, c.K0).permute(0, 3, 1, 2), stride=2)
        else:
            y = F.conv2d(x, W.view(c.N, 3, 3, c.K0).permute(0, 3, 1, 2), padding=1)
        return y.permute(0, 2, 3, 1).reshape(c.M, c.N)

    def _a(self):
        c = self.c
        if c.a_mode != gc.A_PLAIN:
            return self.A0
        return self.A0[:, :c.K0] if not c.K1 else torch.cat([self.A0[:, :c.K0], self.A1[:, :c.K1]], 1)

    def acc64(self, prec):
        """sum_k A[m][k] W[n][k] in fp64 (prec 1: of the bf16-rounded operands; GELU on load in fp64, then the rounding), [M][N]."""
        rnd = (lambda t: t.float().to(torch.bfloat16).double()) if prec == 1 else (lambda t: t.double())
        a = self._a()
        return self._product(rnd(F.gelu(a.double())) if self.c.a_gelu else rnd(a), rnd(self.Wt))

    def flip_slack(self):
        """prec 1 with GELU on load (module docstring): -> (what each output may differ by because an operand's bf16 rounding is
        decided by the fp32 GELU's last bits [M][N], number of such operands).  An operand is in doubt when gelu_f64(a) -+ delta round
        to different bf16 values, delta = 2e-7 max(1, |a|) + 2^-23 |gelu(a)|; it may then be either of the two."""
        c = self.c
        assert c.a_gelu
        a = self._a().double()
        g = F.gelu(a)
        delta = 2e-7 * a.abs().clamp(min=1.0) + 2.0 ** -23 * g.abs()
        lo, hi = (g - delta).float().to(torch.bfloat16).double(), (g + delta).float().to(torch.bfloat16).double()
        slack = self._product(hi - lo, self.Wt.to(torch.bfloat16).double().abs())
        if c.epi == gc.EPI_BIAS_GELU:
            slack = slack * 1.13
        assert c.epi in (gc.EPI_BIAS, gc.EPI_BIAS_GELU)
        return slack, int((hi != lo).sum())

    def ref64(self, prec):
        c = self.c
        return _epilogue64(self.acc64(prec), self.bias, self.gamma, self.res[:c.M, :c.N], c.epi)

    def launch(self, L, prec, cfg, expect=0):
        c = self.c
        if prec and prec not in self.W16:
            self.W16[prec] = _weights16(self.Wt, prec)
        out = torch.full((c.M + 1, c.ldo), NAN, device='cuda')
        rc = _launch(L, A0=self.A0, A1=self.A1, lda0=c.lda0, lda1=c.lda1, K0=c.K0, K1=c.K1, H=c.H, W=c.W, Wt=self.Wt, ldw=c.K,
                     Wt16=self.W16.get(prec), bias=self.bias, gamma=self.gamma, res=self.res, ldres=c.ldo, out=out, ldo=c.ldo,
                     M=c.M, N=c.N, K=c.K, a_mode=c.a_mode, epi=c.epi, a_gelu=c.a_gelu, prec=prec, cfg=cfg)
        assert rc == expect, (rc, cfg)
        return out

    def check_guards_all(self, outs, names):
        """check_guards for every output of a list in one device reduction (the message then names the configuration at fault)."""
        c = self.c
        st = torch.isnan(torch.stack(outs))
        bad = torch.stack([st[:, :c.M, :c.N].flatten(1).sum(1), (~st[:, c.M]).flatten(1).sum(1),
                           (~st[:, :c.M, c.N:]).flatten(1).sum(1)], 1).tolist()
        for name, (inside, row, cols) in zip(names, bad):
            assert inside == 0, f'{name}: {inside} output elements are NaN (never written, or an operand read outside its row)'
            assert row == 0, f'{name}: wrote {row} elements of the row beyond M'
            assert cols == 0, f'{name}: wrote {cols} elements in columns [N, ldo)'

    def check_guards(self, out, what):
        c = self.c
        left = int(torch.isnan(out[:c.M, :c.N]).sum())
        assert left == 0, f'{what}: {left} output elements are NaN (never written, or an operand read outside its row)'
        assert bool(torch.isnan(out[c.M]).all()), f'{what}: wrote a row beyond M'
        assert bool(torch.isnan(out[:c.M, c.N:]).all()), f'{what}: wrote columns in [N, ldo)'


_CASES = gc.all_cases()


@pytest.mark.parametrize('prec,case', _CASES, ids=[f'prec{p}-{gc.case_id(c)}' for p, c in _CASES])
def test_every_configuration_equals_the_chosen_one_and_fp64(L, prec, case):
    p = Problem(case, seed=1000 * prec + sum(case[1:4]) + 7 * case.epi)
    outs = [p.launch(L, prec, cfg) for cfg in ALL_CFGS]
    e0 = None
    if prec == 2:
        e0 = p.launch(L, 0, 0)
    torch.cuda.synchronize()
    p.check_guards_all(outs, [f'cfg {k}' for k in ALL_CFGS])
    ref = p.ref64(prec)
    diff = (outs[0][:case.M, :case.N].double() - ref).abs()
    err = float(diff.max())
    print(f'prec {prec} {gc.case_id(case)}: max error against fp64 {err:.3e}')
    if prec == 1 and case.a_gelu:                        # (see the module docstring)
        slack, doubtful = p.flip_slack()
        print(f'    {doubtful} operands with a bf16 rounding in doubt, {int((slack > 0).sum())} outputs read one, '
              f'{int((diff >= TOL[1]).sum())} outputs differ by 3e-5 or more, largest allowance {float(slack.max()):.3e}')
        over = diff - slack
        assert float(over.max()) < TOL[1], (float(over.max()), err)
    else:
        assert err < TOL[prec], err
    if prec == 2:
        err0 = float((e0[:case.M, :case.N].double() - ref).abs().max())
        print(f'    prec 0 error {err0:.3e}')
        assert err <= 2 * err0 + 1e-6, (err, err0)
    # word for word, guards included (their NaN prefill has one bit pattern)
    _assert_same_words(outs, [f'cfg {k}' for k in ALL_CFGS], case.M + 1, case.ldo)


@pytest.mark.parametrize('prec', gc.PRECS)
def test_rows_do_not_depend_on_m(L, prec):
    """Rows [100, 163) of the 549-row call equal the same rows computed as a 63-row call, under a configuration with BM = 64 and one
    with BM = 256 (and the library's choice, which differs between the two M)."""
    big = gc._plain(gc.RAGGED_M, 292, 96, gc.EPI_GAMMA_RES)
    pb = Problem(big, seed=31 + prec)
    small = gc._plain(63, 292, 96, gc.EPI_GAMMA_RES)
    ps = Problem(small, seed=0)
    ps.A0, ps.Wt, ps.bias, ps.gamma = pb.A0[100:163].contiguous(), pb.Wt, pb.bias, pb.gamma
    ps.res = torch.cat([pb.res[100:163], pb.res[:1]]).contiguous()
    ids = [c.id for c in gc.CONFIGS if c.BM == 64][:1] + [c.id for c in gc.CONFIGS if c.BM == 256][:1]
    assert len(ids) == 2
    for cfg in [0] + [i + 1 for i in ids]:
        ob, os_ = pb.launch(L, prec, cfg), ps.launch(L, prec, cfg)
        torch.cuda.synchronize()
        ps.check_guards(os_, f'cfg {cfg}, M = 63')
        _assert_same_words([ob[100:163].contiguous(), os_[:63].contiguous()], [f'cfg {cfg} M = 549 rows 100..162', 'M = 63'], 63, 292)


def test_asymmetric_identity_every_configuration(L):
    """A = I and W[n][k] = ((n K + k) % 251) / 251: under prec 0 every configuration returns W transposed exactly -- a transposed or
    mis-strided C write that random data within tolerance can hide."""
    K, N = 96, 100
    A = torch.eye(K, device='cuda')
    Wt = (torch.arange(N * K, device='cuda', dtype=torch.float32).reshape(N, K) % 251) / 251
    want = Wt.t().contiguous()
    for cfg in ALL_CFGS:
        out = torch.full((K + 1, N), NAN, device='cuda')
        assert _launch(L, A0=A, lda0=K, K0=K, Wt=Wt, ldw=K, out=out, ldo=N, M=K, N=N, K=K, cfg=cfg) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:K], want), f'cfg {cfg}: {int((out[:K] != want).sum())} elements differ from W^T'
        assert bool(torch.isnan(out[K]).all())


# ------------------------------------------------------------------------------------------------ split-K
_SPLIT = gc.split_cases()


@pytest.mark.parametrize('s', _SPLIT, ids=[f'prec{s.prec}-M{s.M}-N{s.N}-K{s.K}-S{s.S}-epi{s.epi}' for s in _SPLIT])
def test_split_k_every_configuration(L, s):
    """Every configuration, with the reduce launch and with arrival counters, equals the library's choice with the reduce launch; the
    counters are zero afterwards; a second launch on the same workspace and counters gives the same bits; S slices against one slice
    by the rule of test_gpu_kernels.py::test_gemm_split_k."""
    M, N, K, S = s.M, s.N, s.K, s.S
    case = gc._plain(M, N, K, s.epi)
    p = Problem(case, seed=5000 + 100 * s.prec + M + N + K + S)
    W16 = _weights16(p.Wt, s.prec)
    ws = torch.empty(S * M * N, device='cuda')
    cnt = torch.zeros(gc.split_cnt_entries(M, N), dtype=torch.int32, device='cuda')

    def run(cfg, ksplit, counters, refill=True):
        out = torch.full((M + 1, N), NAN, device='cuda')
        if refill:
            ws.fill_(NAN)
        rc = _launch(L, A0=p.A0, lda0=K, K0=K, Wt=p.Wt, ldw=K, Wt16=W16, bias=p.bias, gamma=p.gamma, res=p.res, ldres=N, out=out, ldo=N,
                     M=M, N=N, K=K, epi=s.epi, prec=s.prec, cfg=cfg, ksplit=ksplit, ws=ws if ksplit > 1 else None,
                     cnt=cnt if (counters and ksplit > 1) else None)
        assert rc == 0, (rc, cfg)
        return out

    o1 = run(0, 1, False)
    outs, names = [], []
    for cfg in ALL_CFGS:
        for counters in (False, True):
            outs.append(run(cfg, S, counters))
            names.append(f"cfg {cfg} {'counters' if counters else 'reduce launch'}")
    outs.append(run(gc.NUM_CONFIGS, S, True, refill=False))          # back to back on the workspace the launch before left behind
    names.append('second launch on the same workspace and counters')
    torch.cuda.synchronize()
    p.check_guards(outs[0], names[0])
    assert int(cnt.abs().sum()) == 0, 'arrival counters not left at zero'
    _assert_same_words(outs, names, M + 1, N)
    ref = p.ref64(s.prec)
    e1, eS = float((o1[:M].double() - ref).abs().max()), float((outs[0][:M].double() - ref).abs().max())
    print(f'split-K prec {s.prec} M {M} N {N} K {K} S {S}: error one slice {e1:.3e}, S slices {eS:.3e}')
    assert e1 < TOL[s.prec], e1
    assert eS <= 2 * e1 + 2e-6, (e1, eS)


# ------------------------------------------------------------------------------------------------ return codes
@pytest.mark.parametrize('prec', gc.PRECS)
def test_a_configuration_beyond_the_last_is_an_argument_error(L, prec):
    assert L.lvae_gemm_num_configs() == 12
    for a_mode in gc.A_MODES:
        p = Problem(gc.cases(prec, a_mode)[0], seed=1)
        for cfg in (gc.NUM_CONFIGS + 1, 100):
            out = p.launch(L, prec, cfg, expect=-22)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())
        p.launch(L, prec, gc.NUM_CONFIGS)
    M, N, K = 63, 64, 256
    p = Problem(gc._plain(M, N, K, 0), seed=2)
    out, ws = torch.full((M, N), NAN, device='cuda'), torch.full((2 * M * N,), NAN, device='cuda')
    rc = _launch(L, A0=p.A0, lda0=K, K0=K, Wt=p.Wt, ldw=K, Wt16=_weights16(p.Wt, prec), bias=p.bias, out=out, ldo=N, M=M, N=N, K=K,
                 prec=prec, cfg=gc.NUM_CONFIGS + 1, ksplit=2, ws=ws)
    torch.cuda.synchronize()
    assert rc == -22 and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ store forms
def _cfgs_of(prec):
    return (0, 1, 2) if prec == 4 else ALL_CFGS           # prec 4: gemm_h2_kernel's 64- and 128-wide tiles


class StoreProblem:
    """A 1 x 1 convolution over an NHWC map stored through PixelShuffle(r): ST_SHUFFLE (NHWC, columns pre-permuted to (i r + j) Cout + c)
    or ST_IMAGE (NCHW, clamp(-1, 1) / 2 + 1 / 2, columns in torch's order c r^2 + i r + j).  The reference is F.pixel_shuffle of
    F.conv2d in fp64 with the weights in torch's order."""

    def __init__(self, store, r, N, K, seed):
        g = torch.Generator().manual_seed(seed)
        self.store, self.r, self.N, self.K = store, r, N, K
        self.B, self.H, self.W = gc.STORE_MAP
        self.M = self.B * self.H * self.W
        self.cout = N // (r * r)
        self.x = torch.randn(self.M, K, generator=g).cuda()
        self.w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()          # torch's column order
        self.b = torch.randn(N, generator=g).cuda()
        if store == gc.ST_SHUFFLE:
            self.wk = self.w.reshape(self.cout, r * r, K).permute(1, 0, 2).reshape(N, K).contiguous()
            self.bk = self.b.reshape(self.cout, r * r).t().reshape(-1).contiguous()
        else:
            self.wk, self.bk = self.w, self.b
        self.W16 = {}
        self.status = torch.zeros(1, dtype=torch.int32, device='cuda')

    def ref64(self):
        x = self.x.double().view(self.B, self.H, self.W, self.K).permute(0, 3, 1, 2)
        y = F.pixel_shuffle(F.conv2d(x, self.w.double()[:, :, None, None], self.b.double()), self.r)
        if self.store == gc.ST_IMAGE:
            return (y.clamp(-1, 1) * 0.5 + 0.5).reshape(-1)
        return y.permute(0, 2, 3, 1).reshape(-1)

    def launch(self, L, prec, cfg, image=None, bias=None):
        """image = b: that image alone, as a one-image call."""
        if prec and prec not in self.W16:
            self.W16[prec] = _weights16(self.wk, prec)
        x, M = self.x, self.M
        if image is not None:
            M = self.H * self.W
            x = self.x[image * M:(image + 1) * M].contiguous()
        out = torch.full((M * self.N + 64,), NAN, device='cuda')
        rc = _launch(L, A0=x, lda0=self.K, K0=self.K, H=self.H, W=self.W, Wt=self.wk, ldw=self.K, Wt16=self.W16.get(prec),
                     bias=self.bk if bias is None else bias, out=out, M=M, N=self.N, K=self.K, store=self.store, r=self.r, prec=prec,
                     cfg=cfg, status=self.status if self.store == gc.ST_IMAGE else None)
        assert rc == 0, (rc, cfg)
        return out


_STORES = ([(gc.ST_SHUFFLE, r, r * r * co, K, prec) for r, co in gc.SHUFFLE_SHAPES for K in gc.STORE_KS for prec in gc.STORE_PRECS]
           + [(gc.ST_IMAGE, r, N, K, prec) for r, N in gc.IMAGE_SHAPES for K in gc.STORE_KS for prec in gc.STORE_PRECS])


@pytest.mark.parametrize('store,r,N,K,prec', _STORES,
                         ids=[f"{'shuffle' if s == gc.ST_SHUFFLE else 'image'}-r{r}-N{N}-K{K}-prec{p}" for s, r, N, K, p in _STORES])
def test_store_forms(L, store, r, N, K, prec):
    p = StoreProblem(store, r, N, K, seed=store * 1000 + N + K)
    cfgs = _cfgs_of(prec)
    outs = [p.launch(L, prec, cfg) for cfg in cfgs]
    alone = [p.launch(L, prec, 0, image=b) for b in range(p.B)]
    torch.cuda.synchronize()
    n = p.M * N
    assert int(torch.isnan(outs[0][:n]).sum()) == 0 and bool(torch.isnan(outs[0][n:]).all())
    err = float((outs[0][:n].double() - p.ref64()).abs().max())
    print(f'store {store} r {r} N {N} K {K} prec {prec}: max error against fp64 {err:.3e}')
    assert err < TOL[prec], err
    _assert_same_words(outs, [f'cfg {k}' for k in cfgs], p.M, N)
    per = n // p.B                                           # both layouts are image-major
    for b in range(p.B):
        assert bool(torch.isnan(alone[b][per:]).all())
        _assert_same_words([outs[0][b * per:(b + 1) * per].contiguous(), alone[b][:per].contiguous()],
                           [f'image {b} of the batch', 'the same image alone'], p.H * p.W, N)
    if store != gc.ST_IMAGE:
        return
    # the status word: untouched by finite data in every configuration (it was handed to all the launches above) ...
    assert int(p.status.item()) == 0
    # ... and LVAE_STATUS_NONFINITE_IMAGE from each configuration once a bias makes one column infinite before the clamp
    bias = p.bk.clone()
    bias[N - 2] = float('inf')
    for cfg in cfgs:
        p.status.zero_()
        out = p.launch(L, prec, cfg, bias=bias)
        torch.cuda.synchronize()
        assert int(p.status.item()) == 8, f'cfg {cfg}: status {int(p.status.item())}'
        assert int(torch.isnan(out[:n]).sum()) == 0
