"""gpu: the native replay of a launch plan (lvae_run_ops: csrc/plan_runtime.cpp, casts derived in csrc/plan_ops.h) against the same
launches issued one by one through ctypes.

Every plan below is run twice from the same state -- all device tensors the plan owns are restored to one snapshot in between, scratch
included -- once as `pl.run()` and once as one foreign call per recorded op, `fn(*args, stream)`, on the same stream (ORDER entries as
lvae_stream_order).  Afterwards every owned tensor must hold the same bytes.  A cast that reads the wrong slot gives another launch, so
it shows here; the kinds no plan reaches are covered by the CPU routing check alone (tests/test_abi.py) and are listed in NOT_REACHED."""
import ctypes

import pytest
import torch

from lvae import _native, engine

# Kinds that none of the plans below records.  qarv_base is the only model with fp8 and per-image-lambda plans, and each of its blocks
# has a channel-per-lane depthwise instance with pre-converted MLP operands: its fp8 plans take the _q8 forms, never _bf16, and its vec
# plans the _h2_v / _q8_v forms, never _f32_v (lvae_dwconv_ln_f32 itself comes from qres17m's C = 144 / 288 blocks).  No posterior head
# of these image sizes leaves its split-K planes to the quantize launch.
NOT_REACHED = frozenset({'lvae_dwconv_ln_bf16', 'lvae_dwconv_ln_bf16_v', 'lvae_dwconv_ln_f32_v', 'lvae_quantize_sk_f32'})


def _owned(pl):
    """name -> device tensor, for everything the plan allocated: scratch, kept tensors (symbols, indexes, outputs, statistics), the status
    word, a vec plan's AdaLN slab."""
    ts = dict(pl.bufs)
    ts.update({f'keep[{k}]': t for k, t in enumerate(pl.keep) if isinstance(t, torch.Tensor)})
    for name in ('sym_all', 'idx_all', 'out', 'status', 'adaln_slab', 'im'):
        t = getattr(pl, name, None)
        if t is not None:
            ts['pl.' + name] = t
    assert all(t.is_cuda and t.is_contiguous() for t in ts.values())
    return ts


def _issue_one_by_one(pl, lib, s):
    ss = pl.side_stream.cuda_stream if pl.side_stream is not None else None
    for fn, args, label, side in pl.ops:
        if fn is engine._ORDER:
            a, b = (s, ss) if args[0] else (ss, s)
            rc = lib.lvae_stream_order(ctypes.c_void_p(a), ctypes.c_void_p(b), args[1])
        else:
            rc = fn(*args, ctypes.c_void_p(ss if side else s))
        assert rc == 0, (label, rc)


def _replay_both_ways(pl, seed):
    """-> (names of the owned tensors that differ, kinds replayed)."""
    lib = _native.lib()
    pl.status_ptr()
    ts = _owned(pl)
    gen = torch.Generator().manual_seed(seed)
    if getattr(pl, 'im', None) is not None:
        pl.im.copy_(torch.rand(pl.im.numel(), generator=gen))
    for name in ('sym_all', 'idx_all', 'status'):           # decode plans run on zero symbols: no coder is involved
        ts['pl.' + name].zero_()
    torch.cuda.synchronize()
    start = {k: t.clone() for k, t in ts.items()}
    st = torch.cuda.Stream()
    after = []
    for run in (lambda: pl.run(stream=st.cuda_stream), lambda: _issue_one_by_one(pl, lib, st.cuda_stream)):
        run()
        torch.cuda.synchronize()
        after.append({k: t.clone() for k, t in ts.items()})
        for k, t in ts.items():
            t.copy_(start[k])
        torch.cuda.synchronize()
    kinds = {'ORDER' if fn is engine._ORDER else fn.lvae_name for fn, _a, _l, _s in pl.ops}
    return [k for k in ts if not torch.equal(after[0][k].view(torch.uint8), after[1][k].view(torch.uint8))], kinds


@pytest.fixture(scope='module')
def replayed(product_model):
    """{case: differing tensors}, kinds replayed -- B = 2 at 64x64 (one max_stride tile: the smallest image, and already the split-K and
    mlp_sk forms) for every plan kind, and B = 5 at 64x128 for the two pipeline-group sizes."""
    import lvae
    diffs, kinds = {}, set()

    def case(name, m, kind, n, a, b, **kw):
        pl = m._plan(kind, n, a, b, **kw)
        if kw.get('vec'):
            m._set_lmb([32.0 * 4 ** i for i in range(n)])         # one lambda per image
            m._use_lmb(pl)
        d, k = _replay_both_ways(pl, len(diffs))
        diffs[f'{name} {m._prec} {kind} n={n} {a}x{b}' + (' vec' if kw.get('vec') else '')] = d
        kinds.update(k)

    m = product_model
    base = m._prec
    try:
        m._set_lmb(m.default_lmb)
        for prec in ('f16x2', 'fp8'):
            m.set_gemm_precision(prec)
            for vec in (False, True):
                for kind in ('enc', 'encb', 'ence', 'dec', 'evald'):
                    case('qarv_base', m, kind, 2, *((64, 64) if kind.startswith('enc') else (1, 1)), vec=vec)
        m.set_gemm_precision('f16x2')
        assert sorted({n for _, n in m._groups(5, 'enc')} | {n for _, n in m._groups(5, 'dec')}) == [2, 3]
        for n in (2, 3):
            case('qarv_base', m, 'enc', n, 64, 128)
            case('qarv_base', m, 'dec', n, 1, 2)
    finally:
        m.set_gemm_precision(base)
    for name in ('qres34m_lossless', 'qres17m'):
        torch.manual_seed(0)
        q = lvae.get_model(name).to('cuda:0').eval()
        q.compress_mode()
        for kind in ('enc', 'dec', 'eval'):
            case(name, q, kind, 2, 64, 64)
    return diffs, kinds


@pytest.mark.gpu
def test_native_replay_equals_one_call_per_launch(replayed):
    diffs, _ = replayed
    assert len(diffs) == 2 * 2 * 5 + 4 + 2 * 3
    assert {c: d for c, d in diffs.items() if d} == {}


@pytest.mark.gpu
def test_replay_reaches_every_kind_but_the_listed(replayed):
    _, kinds = replayed
    print('kinds not reached:', sorted(set(_native.OP_KINDS) - kinds))
    assert 'ORDER' in kinds
    assert kinds - {'ORDER'} == set(_native.OP_KINDS) - NOT_REACHED
