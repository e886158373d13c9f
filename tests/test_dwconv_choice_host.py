"""not-gpu: lvae_dwconv_ln_choice -- which depthwise + LayerNorm kernel a launch runs (host arithmetic, no HIP call).  Pins of the
launches the product runs, the -22 rule, and the closure that keeps tests/test_gpu_dwconv_instances.py honest: the instances a launch
can reach are exactly the ones its case table (tests/dwconv_cases.py) names."""
import itertools

import pytest

import dwconv_cases as dc
from lvae import _native


@pytest.fixture(scope='module')
def L():
    return _native.lib()


# (formats, C, k, B, H, W) -> (TH, tpw); one affine, channel-per-lane kernel.  Derived from the launcher's estimate as it stood before
# the query existed (a Python transcription agreed with the query on 200 000 random launches when these were written).
PINS = [
    (('f32', 'h2'), 192, 7, (8, 128, 192), (8, 1)),        # the product's B = 8, 128 x 192 maps
    (('f32', 'h2'), 128, 7, (8, 128, 192), (8, 1)),
    (('f32',), 192, 7, (1, 128, 192), (4, 1)),
    (('f32',), 384, 5, (8, 64, 96), (8, 1)),
    (('f32',), 512, 3, (8, 32, 48), (4, 1)),
    (('f32',), 128, 1, (8, 128, 192), (1, 4)),             # four tiles per workgroup
    (('f32',), 128, 1, (3, 69, 75), (1, 2)),
    (('f32',), 384, 1, (3, 92, 98), (1, 8)),
    (('f32',), 128, 3, (1, 45, 51), (1, 1)),
    (('f32',), 128, 3, (7, 45, 51), (4, 1)),
    (('f32',), 128, 3, (25, 45, 51), (8, 1)),
    (('f32',), 512, 7, (3, 49, 49), (8, 1)),
    (('bf16', 'q8'), 512, 7, (3, 49, 49), (4, 1)),
]


@pytest.mark.parametrize('fmts,C,k,bhw,want', PINS)
def test_pinned_choices(L, fmts, C, k, bhw, want):
    for fmt in fmts:
        for per_image in (0, 1):
            assert dc.choice(L, fmt, 1, per_image, *bhw, C, k) == (0, 0) + want, (fmt, per_image)
        assert dc.choice(L, fmt, 0, 0, *bhw, C, k) == (0, 0) + want, fmt     # the affine does not enter the estimate


def test_choice_does_not_depend_on_the_output_format(L):
    """f32 / h2 share the fp32-map instances' estimate, bf16 / q8 the bf16-map one."""
    for C, k, B, H, W in itertools.product(dc.CL_WIDTHS, dc.KS, (1, 3, 8), (9, 49, 128, 250), (11, 49, 192, 401)):
        assert dc.choice(L, 'f32', 1, 0, B, H, W, C, k) == dc.choice(L, 'h2', 1, 0, B, H, W, C, k)
        assert dc.choice(L, 'bf16', 1, 0, B, H, W, C, k) == dc.choice(L, 'q8', 1, 0, B, H, W, C, k)


def test_return_codes(L):
    bhw = (2, 9, 11)
    for C, k in itertools.product(dc.SW_ONLY_WIDTHS, dc.KS):
        for aff in (0, 1, 2):
            assert dc.choice(L, 'f32', aff, 0, *bhw, C, k) == (0, 1, 1, 1)                # sliding window, fp32 maps only
            for fmt in ('h2', 'q8', 'bf16'):
                assert dc.choice(L, fmt, aff, 0, *bhw, C, k)[0] == -22, (fmt, C, k, aff)
        for fmt in dc.FMTS:
            assert dc.choice(L, fmt, 1, 1, *bhw, C, k)[0] == -22                          # per-image vectors: channel-per-lane only
    for C, k in itertools.product(dc.CL_WIDTHS, dc.KS):
        for fmt in ('f32', 'bf16'):
            assert dc.choice(L, fmt, 2, 0, *bhw, C, k) == (0, 1, 1, 1)                    # both affines: sliding window
        for fmt in ('h2', 'q8'):
            assert dc.choice(L, fmt, 2, 0, *bhw, C, k)[0] == -22
        for fmt in dc.FMTS:
            assert dc.choice(L, fmt, 1, 0, *bhw, C, k)[:2] == (0, 0)
            assert dc.choice(L, fmt, 0, 1, *bhw, C, k)[0] == -22                          # _v without its vectors
            assert dc.choice(L, fmt, 2, 1, *bhw, C, k)[0] == -22
    for C in dc.CL_WIDTHS + dc.SW_ONLY_WIDTHS + (64, 100, 320, 1024):
        for k in (0, 2, 4, 6, 8, 9, -1):
            for fmt, aff in itertools.product(dc.FMTS, (0, 1, 2)):
                assert dc.choice(L, fmt, aff, 0, *bhw, C, k)[0] == -22, (fmt, aff, C, k)
    for C in (64, 100, 320, 1024):
        for k, fmt, aff in itertools.product(dc.KS, dc.FMTS, (0, 1, 2)):
            assert dc.choice(L, fmt, aff, 0, *bhw, C, k)[0] == -22, (fmt, aff, C, k)
    for bad in ((0, 9, 11), (2, 0, 11), (2, 9, 0), (-1, 9, 11)):
        assert dc.choice(L, 'f32', 1, 0, *bad, 128, 7)[0] == -22
    assert dc.choice(L, 4, 1, 0, *bhw, 128, 7)[0] == -22 and dc.choice(L, -1, 1, 0, *bhw, 128, 7)[0] == -22
    assert dc.choice(L, 'f32', 3, 0, *bhw, 128, 7)[0] == -22 and dc.choice(L, 'f32', -1, 0, *bhw, 128, 7)[0] == -22
    # one image's map must fit a 2 GiB buffer descriptor in the channel-per-lane kernel: 1024 x 1024 x 512 fp32 does not, as bf16 it does
    assert dc.choice(L, 'f32', 1, 0, 1, 1024, 1024, 512, 3)[0] == -22 and dc.choice(L, 'bf16', 1, 0, 1, 1024, 1024, 512, 3)[:2] == (0, 0)
    # the outputs may be NULL
    assert L.lvae_dwconv_ln_choice(0, 1, 0, 2, 9, 11, 128, 7, None, None, None) == 0


def test_two_row_sliding_window_instance(L):
    """Both affines, k = 7, C <= 192, fp32 maps, >= 100 000 pixels in the batch: two output rows per pixel group."""
    for C in (128, 192):
        assert dc.choice(L, 'f32', 2, 0, 1, 251, 401, C, 7) == (0, 1, 2, 1)
        assert dc.choice(L, 'f32', 2, 0, 1, 249, 401, C, 7) == (0, 1, 1, 1)                # 99 849 pixels
        assert dc.choice(L, 'f32', 2, 0, 1, 251, 401, C, 5) == (0, 1, 1, 1)
        assert dc.choice(L, 'bf16', 2, 0, 1, 251, 401, C, 7) == (0, 1, 1, 1)
    for C in (144, 256, 288, 384, 512):
        assert dc.choice(L, 'f32', 2, 0, 1, 251, 401, C, 7) == (0, 1, 1, 1)


SWEEP_B = (1, 2, 3, 8, 25, 64)
SWEEP_HW = (1, 2, 3, 5, 8, 9, 13, 17, 24, 33, 45, 49, 64, 69, 85, 92, 113, 128, 141, 192, 250, 251, 320, 400)


@pytest.fixture(scope='module')
def reachable(L):
    """Every (family, fmt, C, k, TH, tpw > 1) some launch of the sweep runs."""
    seen = set()
    for fmt, aff, C, k in itertools.product(dc.FMTS, (0, 1, 2), dc.CL_WIDTHS + dc.SW_ONLY_WIDTHS, dc.KS):
        for per_image in ((0, 1) if aff == 1 else (0,)):
            if dc.choice(L, fmt, aff, per_image, 2, 9, 11, C, k)[0] != 0:
                continue                                     # an argument error at every size (test_return_codes)
            for B, H, W in itertools.product(SWEEP_B, SWEEP_HW, SWEEP_HW):
                rc, fam, th, tpw = dc.choice(L, fmt, aff, per_image, B, H, W, C, k)
                assert rc == 0, (fmt, aff, per_image, B, H, W, C, k)
                assert fam == (0 if C in dc.CL_WIDTHS and aff < 2 else 1) and (tpw == 1 or (fam == 0 and k == 1))
                seen.add((fam, fmt, C, k, th, tpw > 1))
    return seen


def test_reachable_instances_are_the_case_table(reachable):
    named = dc.named_instances()
    assert reachable == named, (sorted(reachable - named), sorted(named - reachable))


def test_unreachable_instances(reachable):
    """The compiled channel-per-lane instances are the reachable ones plus the six listed as dead (dwconv_cases.CL_UNREACHABLE)."""
    cl = {i for i in reachable if i[0] == 0}
    assert not (cl & dc.CL_UNREACHABLE)
    assert cl | dc.CL_UNREACHABLE == dc.compiled_cl_instances()
    assert len(dc.CL_UNREACHABLE) == 6


def test_case_table_is_what_it_says(L):
    """Every listed case reports its instance, is ragged the way the table's header says, and the rotation gives every (fmt, TH) at
    least two affine modes and, for TH > 1, a case through the _v entry point."""
    modes, through_v = {}, set()
    for fmt, C, k, th, tpw, B, H, W, affine, per_image in dc.CL_CASES:
        assert dc.choice(L, fmt, 0 if affine == 'none' else 1, per_image, B, H, W, C, k) == (0, 0, th, tpw), (fmt, C, k, th, tpw)
        assert B >= 2 and W % 8 != 0 and B * H * W * C <= 16e6
        if th > 1:
            assert H % th != 0 and (th != 8 or H % 8 in (1, 2))
        if tpw > 1:
            assert -(-H // th) % tpw != 0
        if per_image:
            assert B == 3 and affine == 'adaln' and th > 1
            through_v.add((fmt, th))
        modes.setdefault((fmt, th), set()).add(affine)
    assert all(len(m) >= 2 for m in modes.values()), modes
    assert through_v == {(fmt, th) for fmt in dc.FMTS for th in (4, 8)}
    assert {H % 8 for fmt, C, k, th, tpw, B, H, W, *_ in dc.CL_CASES if th == 8} == {1, 2}
    for (lowp, C, k), (H, W, batches) in dc.CL_ACROSS_TH.items():
        ths = [dc.choice(L, 'bf16' if lowp else 'f32', 1, 0, B, H, W, C, k)[2] for B in batches]
        assert ths == [1, 4, 8][:len(batches)] and len(batches) >= 2 and H % 4 != 0 and W % 8 != 0, (lowp, C, k, ths)
        assert (len(batches) == 3) == ((0, 'bf16' if lowp else 'f32', C, k, 8, False) not in dc.CL_UNREACHABLE)
        assert max(batches) * H * W * C <= 16e6
    for fmt, C, k, B, H, W in dc.SW_TH2_CASES:
        assert dc.choice(L, fmt, 2, 0, B, H, W, C, k) == (0, 1, 2, 1) and B * H * W >= 100000 and H % 2 == 1
