"""Rate targeting for the variable-rate model: a multi-section search over lambda in log space.

Host logic only (no GPU, no torch): the caller supplies `sizes_of(list_of_lmb) -> list_of_int`, one coded size per lambda, which the
model implements as ONE batched encode of `n_probe` copies of the image (VariableRateLossyVAE.compress_to_target).  With `n_probe`
probes per round the bracket shrinks by n_probe + 1 per round where a bisection (scripts/qarv/test-at-target-bytes.py) halves it.
"""
import math

import numpy as np


def probe_lambdas(lo, hi, n_probe):
    """n_probe lambdas log-evenly spaced strictly inside (lo, hi); n_probe = 1 gives the bisection's log-midpoint exp((ln lo + ln hi) / 2)."""
    la, lb = math.log(lo), math.log(hi)
    return [math.exp(((n_probe + 1 - j) * la + j * lb) / (n_probe + 1)) for j in range(1, n_probe + 1)]


def _fp32_adjacent(lo, hi):
    """Do lo and hi round to the same or to neighbouring fp32 values?  (The coder sees lambda as fp32: nothing lies in between.)"""
    a, b = np.float32(lo), np.float32(hi)
    return bool(np.nextafter(a, np.float32(np.inf)) >= b)


def multisection_search(sizes_of, lo, hi, target, n_probe=8, max_rounds=50, tol=1):
    """Search lambda in [lo, hi] for a coded size of `target`, the size growing with lambda.

    Each round calls sizes_of() ONCE with n_probe lambdas (probe_lambdas) strictly inside the current bracket -- first (lo, hi) -- and
    narrows the bracket to the two neighbouring probes (or bracket ends) that enclose the target: the upper end becomes the first probe
    whose size exceeds the target, the lower end the probe before it.  It stops when a probe is within `tol` of the target, when the
    bracket's ends are equal or adjacent as fp32 values, or after max_rounds rounds.

    Returns (index, history, n_rounds): history = [(lmb, size)] of every probe in the order visited, index = the entry to use -- the
    largest size <= target (the larger lambda among equal sizes); if every probe exceeded the target, the smallest size seen."""
    assert 0 < lo < hi and n_probe >= 1 and max_rounds >= 1
    history, rounds = [], 0
    while rounds < max_rounds and not _fp32_adjacent(lo, hi):
        lmbs = probe_lambdas(lo, hi, n_probe)
        sizes = [int(s) for s in sizes_of(list(lmbs))]
        assert len(sizes) == len(lmbs)
        rounds += 1
        history += list(zip(lmbs, sizes))
        if any(abs(s - target) <= tol for s in sizes):
            break
        over = [j for j, s in enumerate(sizes) if s > target]
        j = over[0] if over else len(lmbs)
        if j < len(lmbs):
            hi = lmbs[j]
        if j > 0:
            lo = lmbs[j - 1]
    assert history, 'the bracket is empty in fp32: nothing was probed'
    fits = [i for i, (_, s) in enumerate(history) if s <= target]
    if fits:
        best = max(fits, key=lambda i: (history[i][1], history[i][0]))
    else:
        best = min(range(len(history)), key=lambda i: (history[i][1], history[i][0]))
    return best, history, rounds
