"""not-gpu: the multi-section rate search (lvae/utils/rate_search.py) on synthetic size functions, and the declarations of the
per-image-lambda entry points (header, ctypes table, plan op kinds)."""
import math
import os
import re

import numpy as np
import pytest

from lvae import _native
from lvae.utils.rate_search import multisection_search, probe_lambdas

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = 16.0, 2048.0            # qarv_base's lmb_range


def smooth(lmb):                 # strictly growing, ~ the shape of a real rate curve
    return int(2000 * lmb ** 0.6)


def steps(lmb):                  # plateaus: 1000-byte steps, four per octave
    return 1000 * int(4 * math.log2(lmb))


CASES = [(smooth, 20000), (smooth, 77777), (smooth, 5000 + 4242), (steps, 17500), (steps, 21000), (steps, 40999),
         (smooth, 10), (smooth, 10 ** 9), (steps, 10), (steps, 10 ** 9)]         # the last four: target outside the range of sizes


def fp32_adjacent(a, b):
    return bool(np.nextafter(np.float32(a), np.float32(np.inf)) >= np.float32(b))


def bisection(size, target, max_iter=50, tol=1):
    """scripts/qarv/test-at-target-bytes.py::binary_search_lmb on a size function (its update rule and log-midpoint, verbatim), ended
    also when the bracket has no fp32 value left inside.  -> (visited lambdas, sizes)."""
    lo, hi = LO, HI
    lmb = math.exp(0.5 * (math.log(lo) + math.log(hi)))
    seen = []
    for _ in range(max_iter):
        if fp32_adjacent(lo, hi):
            break
        n_bytes = size(lmb)
        seen.append((lmb, n_bytes))
        if abs(n_bytes - target) <= tol:
            break
        if n_bytes > target:
            hi = lmb
        else:
            lo = lmb
        lmb = math.exp(0.5 * (math.log(lo) + math.log(hi)))
    return seen


def run(size, target, n_probe, **kw):
    calls = []

    def sizes_of(lmbs):
        calls.append(list(lmbs))
        return [size(v) for v in lmbs]
    best, history, rounds = multisection_search(sizes_of, LO, HI, target, n_probe=n_probe, **kw)
    return best, history, rounds, calls


@pytest.mark.parametrize('n_probe', [1, 2, 3, 8, 15])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_search_returns_the_best_fit_and_stays_inside_its_bracket(case, n_probe):
    size, target = CASES[case]
    best, history, rounds, calls = run(size, target, n_probe)
    assert rounds == len(calls) and len(history) == sum(len(c) for c in calls) and all(len(c) == n_probe for c in calls)
    assert [s for _, s in history] == [size(v) for v, _ in history]
    # the return rule: the largest size <= target when one was seen, else the smallest seen
    sizes = [s for _, s in history]
    fits = [s for s in sizes if s <= target]
    assert history[best][1] == (max(fits) if fits else min(sizes))
    if size(LO * (1 + 1e-6)) <= target:                  # a size <= target exists inside the range: one must be returned
        assert history[best][1] <= target
    # every round's probes lie strictly inside the bracket the earlier rounds left, in ascending order
    lo, hi = LO, HI
    for c in calls:
        assert all(lo < v < hi for v in c) and c == sorted(c), (lo, hi, c)
        over = [j for j, v in enumerate(c) if size(v) > target]
        j = over[0] if over else len(c)
        hi = c[j] if j < len(c) else hi
        lo = c[j - 1] if j > 0 else lo
    # stopped for a reason: a probe within tol, or nothing left between the ends in fp32
    assert any(abs(s - target) <= 1 for s in sizes) or fp32_adjacent(lo, hi)


@pytest.mark.parametrize('n_probe', [2, 3, 8, 15])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_rounds_against_bisection(case, n_probe):
    """n_probe probes per round shrink the bracket by n_probe + 1: never more rounds than ceil(bisection's rounds / log2(n_probe + 1))."""
    size, target = CASES[case]
    r_bisect = len(bisection(size, target))
    _, _, rounds, _ = run(size, target, n_probe)
    print(f'{size.__name__} target {target}: bisection {r_bisect} rounds, n_probe={n_probe}: {rounds}')
    assert rounds <= math.ceil(r_bisect / math.log2(n_probe + 1)), (rounds, r_bisect)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_one_probe_is_the_scripts_bisection(case):
    size, target = CASES[case]
    seen = bisection(size, target)
    _, history, rounds, _ = run(size, target, 1)
    assert rounds == len(seen)
    assert [np.float32(v) for v, _ in history] == [np.float32(v) for v, _ in seen]


def test_probe_lambdas_are_log_even():
    p = probe_lambdas(LO, HI, 6)                         # 7 octaves in 7 steps: the powers of two in between
    assert np.allclose(p, [32, 64, 128, 256, 512, 1024], rtol=1e-12)
    assert probe_lambdas(3.0, 48.0, 1) == [math.exp(0.5 * (math.log(3.0) + math.log(48.0)))]


def test_max_rounds_and_tolerance():
    _, history, rounds, _ = run(steps, 17500, 8, max_rounds=2)
    assert rounds == 2 and len(history) == 16
    _, history, rounds, _ = run(smooth, 20000, 8, tol=10 ** 6)
    assert rounds == 1


# ---- declarations of the new entry points
NEW = {'lvae_dwconv_ln_f32_v': 13, 'lvae_dwconv_ln_h2_v': 13, 'lvae_dwconv_ln_bf16_v': 13, 'lvae_dwconv_ln_q8_v': 13, 'lvae_gemv_batch_f32': 10}


def test_new_symbols_declared_with_matching_argument_counts():
    src = open(os.path.join(REPO, 'include', 'lvae_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
        assert m, f'{name} is not declared in include/lvae_hip.h'
        assert len(m.group(1).split(',')) == nargs, name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs, name
    enum = src[src.index('LVAE_OP_GEMM = 1'):src.index('LVAE_OP_ORDER')]
    names = [n.strip() for n in enum.replace('LVAE_OP_GEMM = 1', 'LVAE_OP_GEMM').split(',') if n.strip()]
    for name in NEW:
        if 'dwconv' in name:                             # plan ops: the enum position is the ctypes table's kind
            assert names.index('LVAE_OP_' + name[len('lvae_'):].upper()) + 1 == _native.OP_KINDS[name], name
    assert _native.OP_ORDER == len(names) + 1


def test_new_entry_points_validate_arguments_without_gpu():
    L = _native.lib()
    for name in NEW:
        if 'dwconv' in name:
            assert getattr(L, name)(None, None, None, None, None, None, 1, 8, 8, 128, 7, 0, None) == -22
    assert L.lvae_gemv_batch_f32(None, None, None, None, 4, 4, 2, 0, 0, None) == -22
