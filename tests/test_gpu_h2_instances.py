"""-m gpu: every kernel instance of the f16x2 GEMM family (prec 4: csrc/gemm_h2.hip, 10 instances; csrc/gemm_h2n.hip, 6;
csrc/gemm_h2p.hip, 7) at the smallest shapes that straddle its tiles, stages and chunks -- the table of tests/h2_cases.py, whose
arithmetic tests/test_h2_cases_host.py checks against lvae_gemm_h2_choice without a GPU; every launch here asks that function about
its descriptor first, and it must give the launch's return code and the instance the form names.  Large shapes stay in tests/test_gpu_f16x2.py.

One test id is (kernel, case); inside, every launch form that takes the case runs (h2_cases.forms: forced tile widths, the narrow-
output kernel, every pre-split tile, the split-K forms), and

  a. plain products with EPI_BIAS are held to the kernel's own arithmetic: an fp64 evaluation of H + X / 2048 from split_f16x2 of both
     operands, within (K / 16 + 2 S + 4) 2^-24 (|A| |W|^T + |bias|) elementwise -- one rounding of H per k16 instruction, one for the
     fma and one for the bias per slice, S - 1 adds of the fold, and the margin of 4 that
     test_gpu_f16x2.py::test_gemm_f16x2_matches_its_own_arithmetic has.  A swapped plane, a missing cross term or a wrong k mapping is
     orders of magnitude above it;
  b. every case is held to fp64 of the unrounded operands with the fp64 epilogue (GELU on load and F.conv2d for the gathers in fp64)
     within 3e-5 absolute on O(1) data -- the bound tests/test_gpu_gemm_configs.py (TOL[4]) and tests/test_gpu_f16x2.py have for this
     arithmetic;
  c. all forms must agree word for word (the family's contract: the dispatcher picks by speed alone);
  d. out_h2 planes must be split_f16x2 of the fp32 result of the same launch without out_h2;
  e. rows inside the 549-row launch must equal the same rows launched alone;
  f. K = 16 (mod 32) has one kernel: (a) and (b) carry those cases, and the refusals around them are asserted as -22;
  g. every gemm_h2p / gemm_h2n form is launched twice into fresh outputs: nothing may depend on what the launch before left in LDS.

Every operand lies exactly inside a larger poisoned buffer (fp32: NaN; packed weights and H2K32 planes: 0x7e00 halves, an fp16 NaN),
padding columns of A are NaN, outputs are prefilled with NaN (0x7e00 halves under out_h2): a read beyond an operand that reaches a
stored value shows as a NaN inside [M][N], a write beyond it as a guard element that is no longer NaN.  After every launch: rc == 0, no
NaN inside [M][N], columns [N, ldo) and both guards untouched."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import h2_cases as hc

pytestmark = pytest.mark.gpu

NAN = float('nan')
TOL = 3e-5
GUARD = 64                                   # 4-byte words in front of and behind every buffer
H_NAN = 0x7e00


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _native.lib()


def _cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope='module')
def cu():
    n = _cu()
    assert n >= hc.fold_tiles(hc.RAGGED_M, hc.FOLD_THRESHOLD_N), n
    return n


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(L, **kw):
    """lvae_gemm_f32 with the given descriptor fields -> (return code (no synchronisation), what lvae_gemm_h2_choice said of the same
    descriptor just before: (return code, instance, split-K form))."""
    from lvae._native import GemmDesc
    d = GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    said = hc.choice(L, d, _cu())
    return L.lvae_gemm_f32(ctypes.byref(d), _st()), said


def _embed(t):
    """t (1-D, fp32 or fp16) -> its copy on the GPU with GUARD poisoned words on either side (kept alive by the view's base)."""
    if t.dtype == torch.float16:
        n = t.numel()
        buf = torch.full((n + 4 * GUARD,), H_NAN, dtype=torch.int16, device='cuda')
        buf[2 * GUARD:2 * GUARD + n] = t.cuda().view(torch.int16)
        return buf[2 * GUARD:2 * GUARD + n]
    assert t.dtype == torch.float32
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), NAN, device='cuda')
    buf[GUARD:GUARD + n] = t.cuda()
    return buf[GUARD:GUARD + n]


def _epilogue64(acc, bias, gamma, res, epi):
    v = acc + bias.double()
    if epi == hc.EPI_BIAS_GELU:
        return F.gelu(v)
    if epi == hc.EPI_GAMMA_RES:
        return res.double() + gamma.double() * v
    if epi == hc.EPI_RES:
        return res.double() + v
    return v


def _assert_same_words(outs, names, cols):
    """outs[1:] equal outs[0] as int32 words; one device reduction, details only on failure."""
    words = torch.stack([o.reshape(-1) for o in outs]).view(torch.int32)
    bad = (words[1:] != words[0]).sum(1).tolist()
    if any(bad):
        msg = []
        for i, n in enumerate(bad):
            if n:
                first = int((words[i + 1] != words[0]).nonzero()[0])
                msg.append(f'{names[i + 1]}: {n} words differ from {names[0]}, first at (row {first // cols}, column {first % cols})')
        raise AssertionError('; '.join(msg))


class Problem:
    """Inputs of one case on the GPU (built once), its fp64 references, and launches into fresh poisoned outputs."""

    def __init__(self, c, seed):
        g = torch.Generator().manual_seed(seed)
        self.c = c
        M, N, K = c.M, c.N, c.K
        if c.a_mode == hc.A_PLAIN:
            self.srcs = [torch.randn(M, k, generator=g) for k in (c.K0, c.K1) if k]
            self.srcs[0][:, 7] = 0.0                                   # one all-zero k column
            if M >= 3:
                for s in self.srcs:
                    s[M // 3] = 0.0                                    # one all-zero row (signed zeros of the partial sums)
        else:
            hw = (2 * c.H, 2 * c.W) if c.a_mode == hc.A_PATCH2 else (c.H, c.W)
            self.srcs = [torch.randn(c.B, hw[0], hw[1], c.K0, generator=g)]
            self.srcs[0][..., 7] = 0.0
            self.srcs[0][c.B - 1, hw[0] // 2, hw[1] // 2] = 0.0
        Wt = torch.randn(N, K, generator=g) / K ** 0.5
        bias, gamma = torch.randn(N, generator=g), torch.rand(N, generator=g)
        self.res_rows = torch.randn(M, c.ldo, generator=g)
        from lvae.models.base import pack_f16x2, pack_f16x2_k32
        self.Wt, self.bias, self.gamma = _embed(Wt.reshape(-1)).view(N, K), _embed(bias), _embed(gamma)
        self.W16 = _embed(pack_f16x2(self.Wt))
        self.Wk32 = _embed(pack_f16x2_k32(self.Wt)) if K % 32 == 0 else None
        self.ws, self.cnt = None, None
        self._place()

    def _place(self):
        """The A operand(s) and the residual of the case as it stands (after a change of self.c / self.srcs / self.res_rows)."""
        from lvae.models.base import pack_f16x2_k32
        c = self.c
        self.A, self.Ak32 = [None, None], None
        if c.a_mode == hc.A_PLAIN:
            for i, (s, lda) in enumerate(zip(self.srcs, (c.lda0, c.lda1))):
                rows = torch.full((c.M, lda), NAN)
                rows[:, :s.shape[1]] = s
                self.A[i] = _embed(rows.reshape(-1)[:(c.M - 1) * lda + s.shape[1]].contiguous())
            if not c.K1 and c.lda0 == c.K and c.K % 32 == 0:
                self.Ak32 = _embed(pack_f16x2_k32(self.srcs[0].cuda()))
        else:
            self.A[0] = _embed(self.srcs[0].reshape(-1))
        self.res = _embed(self.res_rows.reshape(-1))

    def contiguous(self):
        """The same product with A materialised as one contiguous [M][K] operand."""
        q = copy.copy(self)
        q.c = self.c._replace(K0=self.c.K, K1=0, lda0=self.c.K, lda1=0)
        q.srcs = [torch.cat(self.srcs, 1).contiguous()]
        q._place()
        return q

    def rows(self, r0, n):
        """Rows [r0, r0 + n) as a problem of their own."""
        q = copy.copy(self)
        q.c = self.c._replace(M=n)
        q.srcs = [s[r0:r0 + n].contiguous() for s in self.srcs]
        q.res_rows = self.res_rows[r0:r0 + n].contiguous()
        q._place()
        return q

    # ---- references
    def _product(self, a, W):
        c = self.c
        if c.a_mode == hc.A_PLAIN:
            return a @ W.t()
        x = a.permute(0, 3, 1, 2)
        if c.a_mode == hc.A_PATCH2:      # K order (i, j, ci)
            y = F.conv2d(x, W.view(c.N, 2, 2, c.K0).permute(0, 3, 1, 2), stride=2)
        else:                            # K order (tap, ci)
            y = F.conv2d(x, W.view(c.N, 3, 3, c.K0).permute(0, 3, 1, 2), padding=1)
        return y.permute(0, 2, 3, 1).reshape(c.M, c.N)

    def _a(self):
        return (torch.cat(self.srcs, 1) if len(self.srcs) > 1 else self.srcs[0]).cuda()

    def ref64(self):
        c = self.c
        a = self._a().double()
        acc = self._product(F.gelu(a) if c.a_gelu else a, self.Wt.double())
        return _epilogue64(acc, self.bias, self.gamma, self.res.view(c.M, c.ldo)[:, :c.N], c.epi)

    def own64(self):
        """(fp64 value of the kernel's three cross terms + bias, elementwise bound) -- docstring (a)."""
        from lvae.models.base import split_f16x2
        c = self.c
        assert not c.a_gelu and c.epi == hc.EPI_BIAS
        a = self._a()
        a2, w2 = split_f16x2(a).double(), split_f16x2(self.Wt.contiguous()).double()
        H = self._product(a2[0], w2[0])
        X = self._product(a2[1], w2[0]) + self._product(a2[0], w2[1])
        bound = (c.K / 16 + 2 * c.S + 4) * 2.0 ** -24 * (self._product(a.double().abs(), self.Wt.double().abs()) + self.bias.double().abs())
        return H + X / 2048.0 + self.bias.double(), bound

    # ---- launches
    def launch(self, L, f, c=None, expect=0):
        """Form f of case c (default: the problem's) -> the poisoned output buffer, GUARD words around [M][ldo]."""
        c = c or self.c
        n = c.M * c.ldo
        if c.out_h2:
            out = torch.full((2 * (n + 2 * GUARD),), H_NAN, dtype=torch.int16, device='cuda').view(torch.float32)
        else:
            out = torch.full((n + 2 * GUARD,), NAN, device='cuda')
        kw = {}
        if c.S > 1:
            if self.ws is None or self.ws.numel() < c.S * c.M * c.N:
                self.ws = _embed(torch.full((c.S * c.M * c.N,), NAN))
                self.cnt = torch.zeros(hc.split_cnt_entries(c.M, c.N), dtype=torch.int32, device='cuda')
            self.ws.fill_(NAN)
            kw = dict(ksplit=c.S, ws=self.ws, cnt=self.cnt if f.cnt else None)
        if f.a_h2:
            assert self.Ak32 is not None
            kw.update(A0=self.Ak32, lda0=c.K, Wt16=self.Wk32, a_h2=1)
        else:
            kw.update(A0=self.A[0], A1=self.A[1], lda0=c.lda0, lda1=c.lda1, Wt16=self.W16)
        rc, said = _launch(L, K0=c.K0, K1=c.K1, H=c.H, W=c.W, Wt=self.Wt, ldw=c.K, bias=self.bias, gamma=self.gamma, res=self.res, ldres=c.ldo,
                     out=out[GUARD:], ldo=c.ldo, M=c.M, N=c.N, K=c.K, a_mode=c.a_mode, epi=c.epi, a_gelu=c.a_gelu, prec=4, cfg=f.cfg,
                     out_h2=c.out_h2, **kw)
        assert said[0] == expect, f'{f.name}: lvae_gemm_h2_choice returns {said[0]}'
        assert rc == expect, f'{f.name}: return code {rc}'
        if f.instance is not None:
            assert said[1] == f.instance, f'{f.name}: lvae_gemm_h2_choice names {said[1]}'
        return out

    def view(self, out, c=None):
        c = c or self.c
        return out[GUARD:GUARD + c.M * c.ldo].view(c.M, c.ldo)

    def check_guards(self, outs, names, c=None):
        """No NaN inside [M][N]; columns [N, ldo) and both guards untouched -- for every output of a list in one device reduction."""
        c = c or self.c
        n = c.M * c.ldo
        if c.out_h2:                               # halves: the planes of [M][N] (ldo == N), 0x7e00 around them
            st = torch.stack(outs).view(torch.int16)
            inside = torch.isnan(st[:, 2 * GUARD:2 * GUARD + 2 * n].view(torch.float16)).flatten(1).sum(1)
            guard = (st[:, :2 * GUARD] != H_NAN).sum(1) + (st[:, 2 * GUARD + 2 * n:] != H_NAN).sum(1)
            cols = torch.zeros_like(guard)
        else:
            st = torch.isnan(torch.stack(outs))
            body = st[:, GUARD:GUARD + n].view(len(outs), c.M, c.ldo)
            inside = body[:, :, :c.N].flatten(1).sum(1)
            cols = (~body[:, :, c.N:]).flatten(1).sum(1)
            guard = (~st[:, :GUARD]).sum(1) + (~st[:, GUARD + n:]).sum(1)
        for name, (i, co, gu) in zip(names, torch.stack([inside, cols, guard], 1).tolist()):
            assert i == 0, f'{name}: {i} output elements are NaN (never written, or an operand read outside its extent)'
            assert co == 0, f'{name}: wrote {co} elements in columns [N, ldo)'
            assert gu == 0, f'{name}: wrote {gu} elements in front of or behind the output'


def _seed(c):
    return 17 + c.M + 3 * c.N + 5 * c.K + 7 * c.epi + 11 * c.S + c.a_gelu + c.ldo + c.lda0


def _launch_forms(L, p, fs, c=None):
    """Every form of the list (the gemm_h2p / gemm_h2n ones twice) -> outputs, names."""
    outs, names = [], []
    for f in fs:
        outs.append(p.launch(L, f, c))
        names.append(f.name)
        if f.a_h2 or f.cfg == 3:
            outs.append(p.launch(L, f, c))
            names.append(f.name + ', second launch')
    return outs, names


def _check_values(p, out, what):
    """(a) where it applies and (b) of the module docstring on one output; prints the measured figures."""
    c = p.c
    got = p.view(out)[:, :c.N].double()
    err = float((got - p.ref64()).abs().max())
    line = f'h2-instances {what} {hc.case_id(c)}: max error against fp64 {err:.3e}'
    ratio = None
    if not c.a_gelu and c.epi == hc.EPI_BIAS:
        own, bound = p.own64()
        ratio = float(((got - own).abs() / bound).max())
        line += f', deviation from its own arithmetic / bound {ratio:.3f}'
    print(line)
    assert ratio is None or ratio <= 1.0, f'{ratio} times the bound of its own arithmetic'
    assert err < TOL, err


def _run(L, cu, what, case, pick):
    p = Problem(case, _seed(case))
    fs = [f for f in hc.forms(case, cu) if pick(f)]
    assert fs, 'no form takes this case'
    outs, names = _launch_forms(L, p, fs)
    if case.a_mode == hc.A_PLAIN and (case.K1 or case.lda0 != case.K0):
        q = p.contiguous()
        outs.append(q.launch(L, fs[0]))
        names.append(f'{fs[0].name} on the contiguous operand')
    torch.cuda.synchronize()
    p.check_guards(outs, names)
    _check_values(p, outs[0], what)
    _assert_same_words(outs, names, case.ldo)
    if case.S > 1:
        assert int(p.cnt.abs().sum()) == 0, 'arrival counters not left at zero'


_H2 = hc.h2_cases()
_H2P = hc.h2p_cases()
_H2N = hc.h2n_cases()
_SPLIT = hc.split_cases()
_OUT_H2 = hc.out_h2_cases()


@pytest.mark.parametrize('case', _H2, ids=[hc.case_id(c) for c in _H2])
def test_gemm_h2_instances(L, cu, case):
    """gemm_h2_kernel with TN = 1 and 2 forced, the library's choice, and gemm_h2n_kernel where it takes the shape."""
    _run(L, cu, 'h2', case, lambda f: not f.a_h2)


@pytest.mark.parametrize('case', _H2P, ids=[hc.case_id(c) for c in _H2P])
def test_gemm_h2p_instances(L, cu, case):
    """Every forced tile of gemm_h2p_kernel on the pre-split operands against gemm_h2_kernel on the fp32 operand."""
    _run(L, cu, 'h2p', case, lambda f: f.a_h2 or f.cfg == 1)


@pytest.mark.parametrize('case', _H2N, ids=[hc.case_id(c) for c in _H2N])
def test_gemm_h2n_instances(L, cu, case):
    """gemm_h2n_kernel (cfg = 3) against gemm_h2_kernel where K % 32 == 0; alone with fp64 and its own arithmetic where K = 16 (mod 32)."""
    _run(L, cu, 'h2n', case, lambda f: not f.a_h2)


@pytest.mark.parametrize('case', _SPLIT, ids=[hc.case_id(c) for c in _SPLIT])
def test_split_k_forms(L, cu, case):
    """The reduce-launch form and the counter form of gemm_h2_kernel under both tile widths, FOLD, and the serial form of
    gemm_h2n_kernel, wherever N and K allow them: the same bits, the counters zero afterwards, no workspace word read by the serial
    forms (it is NaN throughout)."""
    _run(L, cu, 'split-K', case, lambda f: True)


def _assert_planes_are_the_split(p, planes, o32, c, name):
    from lvae.models.base import split_f16x2, unpack_f16x2_k32
    n = c.M * c.N
    hi, lo = unpack_f16x2_k32(planes[GUARD:GUARD + n], c.M, c.N)
    want = split_f16x2(p.view(o32, c)[:, :c.N].contiguous())
    assert torch.equal(hi, want[0]), f'{name}: {int((hi != want[0]).sum())} hi terms differ from the split of the fp32 result'
    assert torch.equal(lo, want[1]), f"{name}: {int((lo != want[1]).sum())} lo' terms differ from the split of the fp32 result"


@pytest.mark.parametrize('case', _OUT_H2, ids=[hc.case_id(c) for c in _OUT_H2])
def test_out_h2_is_the_split_of_the_fp32_result(L, cu, case):
    """gemm_h2_kernel with both TN, every forced gemm_h2p tile and (S = 3) FOLD: the stored planes are split_f16x2 of the fp32 result of
    the same launch without out_h2, under a cut last n-tile too; the fp32 results of all the forms agree."""
    p = Problem(case, _seed(case))
    c32 = case._replace(out_h2=0)
    fs = hc.forms(case, cu)
    assert {f.instance for f in fs} >= ({hc.instance_of(hc.FOLD_LOADERS)} if case.S > 1 else
                                        {('h2', 1, 0, 0), ('h2', 2, 0, 0)} | {hc.instance_of(t) for t in hc.H2P_TILES})
    planes, names = _launch_forms(L, p, fs)
    o32 = [p.launch(L, f, c32) for f in fs]
    others = [f for f in hc.forms(c32, cu) if f not in fs]             # S = 3: the parallel and the gemm_h2n serial form
    o32 += [p.launch(L, f, c32) for f in others]
    torch.cuda.synchronize()
    p.check_guards(planes, names)
    p.check_guards(o32, [f.name for f in fs + others], c32)
    q = copy.copy(p)
    q.c = c32
    _check_values(q, o32[0], 'out_h2')
    _assert_same_words(o32, [f.name for f in fs + others], case.N)
    _assert_same_words(planes, names, case.N)
    _assert_planes_are_the_split(p, planes[0], o32[0], case, names[0])


@pytest.mark.parametrize('side,N,epi', hc.FOLD_THRESHOLD_SPECS, ids=[f'{s}-N{n}-epi{e}' for s, n, e in hc.FOLD_THRESHOLD_SPECS])
def test_fold_on_either_side_of_the_cu_count(L, cu, side, N, epi):
    """The two FOLD instances: ceil(M / 128) ceil(N / 64) <= CU count runs the one with loader waves, more tiles the one without.  M is
    derived from this device's count, so that each side is met whatever the count is; every case against the parallel forms, and the
    pre-split store against the fp32 one where the epilogue has it."""
    case = hc.fold_threshold_case(cu, side, N, epi)
    tiles = hc.fold_tiles(case.M, case.N)
    assert (tiles <= cu) == (side == 'below') and case.M % 128
    p = Problem(case, _seed(case))
    fs = hc.forms(case, cu)
    (fold,) = [f for f in fs if f.a_h2]
    assert fold.instance == hc.instance_of(hc.FOLD_LOADERS if side == 'below' else hc.FOLD_PLAIN)
    outs, names = _launch_forms(L, p, fs)
    ch2 = case._replace(out_h2=1)
    planes = _launch_forms(L, p, [fold], ch2) if hc.h2p_takes(ch2) else None
    torch.cuda.synchronize()
    p.check_guards(outs, names)
    _check_values(p, outs[0], f'fold ({tiles} tiles on {cu} CUs)')
    _assert_same_words(outs, names, case.N)
    assert int(p.cnt.abs().sum()) == 0, 'arrival counters not left at zero'
    if planes:
        p.check_guards(planes[0], planes[1], ch2)
        _assert_same_words(planes[0], planes[1], case.N)
        _assert_planes_are_the_split(p, planes[0][0], outs[names.index(fold.name)], ch2, fold.name)


@pytest.mark.parametrize('kernel', sorted(hc.ROW_CASES))
def test_rows_do_not_depend_on_m(L, cu, kernel):
    """Rows of the 549-row launch equal the same rows launched alone -- a slice that starts mid-tile and the single last row -- under
    every form of the kernel."""
    case = hc.ROW_CASES[kernel]
    p = Problem(case, _seed(case) + 1)
    pick = {'h2': lambda f: not f.a_h2 and f.cfg != 3, 'h2p': lambda f: f.a_h2, 'h2n': lambda f: f.cfg in (0, 3)}[kernel]
    fs = [f for f in hc.forms(case, cu) if pick(f)]
    assert fs
    big = [p.launch(L, f) for f in fs]
    for r0, n in hc.ROW_SLICES:
        q = p.rows(r0, n)
        small = [q.launch(L, f) for f in fs]
        torch.cuda.synchronize()
        q.check_guards(small, [f.name for f in fs])
        for f, ob, os_ in zip(fs, big, small):
            _assert_same_words([p.view(ob)[r0:r0 + n].contiguous(), q.view(os_)],
                               [f'{f.name}, rows {r0}..{r0 + n - 1} of M = {case.M}', f'the same rows alone'], case.ldo)


_REFUSALS = hc.refusals()


@pytest.mark.parametrize('case,cfg,rc', _REFUSALS, ids=[f'{hc.case_id(c)}-cfg{k}' for c, k, _ in _REFUSALS])
def test_refusals(L, case, cfg, rc):
    """What the family does not take is an argument error before any launch: K = 16 (mod 32) on gemm_h2_kernel (cfg = 1 / 2; the 3x3
    gather over 16 channels with GELU on load or more than 96 columns has no f16x2 kernel at all), and beyond 96 columns."""
    p = Problem(case, 1)
    out = p.launch(L, hc.Form(f'cfg {cfg}', 0, cfg, False, None), expect=rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
