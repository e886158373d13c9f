"""The case table of the depthwise + LayerNorm kernel instances, shared by tests/test_gpu_dwconv_instances.py (which runs every case
on the GPU) and tests/test_dwconv_choice_host.py (which sweeps lvae_dwconv_ln_choice without a GPU and asserts that the instances a
launch can reach are exactly the ones named here).  An instance is (family, fmt, C, k, tile rows TH, tiles per workgroup > 1?).

Every shape below was found with lvae_dwconv_ln_choice as the smallest map of its kind; each GPU case asserts that the query still
reports the instance it is listed for, so a change of the launcher's estimate fails here loudly instead of moving the coverage."""
import ctypes

FMTS = ('f32', 'bf16', 'h2', 'q8')                     # a name's code is its index (the `fmt` of lvae_dwconv_ln_choice)
LOWP = ('bf16', 'q8')                                  # formats whose input map is bf16 (their own instances and LDS footprint)
CL_WIDTHS = (128, 192, 256, 384, 512)                  # csrc/dwconv_cl.hip
SW_ONLY_WIDTHS = (144, 288)                            # sliding window only (qres17m)
KS = (1, 3, 5, 7)
AFFINE_MODES = ('adaln', 'ln', 'none')


def choice(L, fmt, affines, per_image, B, H, W, C, k):
    """lvae_dwconv_ln_choice -> (rc, family, tile_rows, tiles_per_wg); the last three are None when rc != 0."""
    f, t, p = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.lvae_dwconv_ln_choice(FMTS.index(fmt) if isinstance(fmt, str) else fmt, affines, int(per_image), B, H, W, C, k,
                                 ctypes.byref(f), ctypes.byref(t), ctypes.byref(p))
    return (rc, f.value, t.value, p.value) if rc == 0 else (rc, None, None, None)


# ------------------------------------------------------------------------------------------------ channel-per-lane kernel
# (bf16 map?, C, k) -> [(TH, tpw, B, H, W)].  B >= 2 distinct images, W % 8 != 0, H % TH != 0; at TH = 8 the last tile is shorter than
# the halo (H % 8 = 1, or 2 at k = 5).  k = 1: tpw = 1, the smallest map with tpw = 2 and an odd number of tiles, and the largest tpw a
# map of at most 16 M elements reaches (8) with ceil(H / TH) % tpw != 0.  At most 14.5 M elements per launch.
CL_SHAPES = {
    (False, 128, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 87, 90), (1, 8, 2, 233, 243)],
    (False, 128, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 70, 73), (8, 1, 3, 145, 145)],
    (False, 128, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 70, 73), (8, 1, 3, 146, 146)],
    (False, 128, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 57, 67), (8, 1, 3, 121, 131)],
    (False, 192, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 65, 75), (1, 8, 2, 183, 186)],
    (False, 192, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 54, 57), (8, 1, 3, 113, 113)],
    (False, 192, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 54, 57), (8, 1, 3, 114, 114)],
    (False, 192, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 97, 107)],
    (False, 256, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 57, 67), (1, 8, 2, 163, 169)],
    (False, 256, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 97, 107)],
    (False, 256, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 98, 108)],
    (False, 256, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 43, 43), (8, 1, 3, 89, 89)],
    (False, 384, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 43, 43), (1, 8, 2, 113, 123)],
    (False, 384, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (False, 384, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 74, 74)],
    (False, 384, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (False, 512, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 43, 43), (1, 8, 2, 113, 123)],
    (False, 512, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (False, 512, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35)],
    (False, 512, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 22, 25), (8, 1, 3, 49, 49)],
    (True, 128, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 87, 90), (1, 8, 2, 233, 243)],
    (True, 128, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 70, 73), (8, 1, 3, 145, 145)],
    (True, 128, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 70, 73), (8, 1, 3, 146, 146)],
    (True, 128, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 70, 73), (8, 1, 3, 145, 145)],
    (True, 192, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 65, 75), (1, 8, 2, 183, 186)],
    (True, 192, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 54, 57), (8, 1, 3, 113, 113)],
    (True, 192, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 54, 57), (8, 1, 3, 114, 114)],
    (True, 192, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 54, 57), (8, 1, 3, 113, 113)],
    (True, 256, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 57, 67), (1, 8, 2, 163, 169)],
    (True, 256, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 97, 107)],
    (True, 256, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 98, 108)],
    (True, 256, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 49, 49), (8, 1, 3, 97, 107)],
    (True, 384, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 43, 43), (1, 8, 2, 113, 123)],
    (True, 384, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (True, 384, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 74, 74)],
    (True, 384, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (True, 512, 1): [(1, 1, 2, 9, 9), (1, 2, 2, 43, 43), (1, 8, 2, 113, 123)],
    (True, 512, 3): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35), (8, 1, 3, 73, 73)],
    (True, 512, 5): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35)],
    (True, 512, 7): [(1, 1, 2, 9, 12), (4, 1, 3, 35, 35)],
}

# Compiled but never launched: TH = 8 at C = 512 / k = 5 (every format) and at C = 512 / k = 7 on bf16 maps.  C = 512 is 8 waves per
# workgroup, so the 3-waves-per-SIMD budget of the k >= 5, TH = 8 instances admits ONE workgroup per CU (slots = 256) where the TH = 4
# instance has two (4 waves per SIMD, and its LDS -- 77 KB at k = 5, 61 KB at k = 7 on bf16 maps -- fits twice in 160 KB; the fp32
# k = 7 instance needs 93 KB, fits once, and so is reachable).  With w4 <= 2 w8 workgroups, ceil(w4 / 512) <= ceil(w8 / 256): TH = 4
# needs no more rounds, and each of its rounds is shorter (3 + 4 + k + 1 against 3 + 8 + k + 1 row steps), so TH = 8 never wins.
CL_UNREACHABLE = {(0, fmt, 512, 5, 8, False) for fmt in FMTS} | {(0, fmt, 512, 7, 8, False) for fmt in LOWP}


def _cl_cases():
    """One case per (fmt, C, k, reachable instance): (fmt, C, k, TH, tpw, B, H, W, affine, per_image).  The affine mode rotates over
    the cases; the ragged TH > 1 cases of k = 3 and k = 7 go through the _v entry point (B = 3, per-image AdaLN vectors)."""
    out = []
    for fmt in FMTS:
        n = 0
        for C in CL_WIDTHS:
            for k in KS:
                for th, tpw, B, H, W in CL_SHAPES[(fmt in LOWP, C, k)]:
                    per_image = th > 1 and k in (3, 7)
                    assert not per_image or B == 3
                    out.append((fmt, C, k, th, tpw, B, H, W, 'adaln' if per_image else AFFINE_MODES[n % 3], per_image))
                    n += 1
    return out


CL_CASES = _cl_cases()

# Same bits whatever the tile height: (bf16 map?, C, k) -> (H, W, batch sizes whose launches run different TH, in the order 1, 4, 8).
# H % 8 is 1 or 3 and W % 8 != 0.  At most 6.9 M elements per launch.
CL_ACROSS_TH = {
    (False, 128, 3): (41, 41, (1, 9, 32)), (False, 128, 5): (41, 41, (1, 9, 32)), (False, 128, 7): (30, 33, (1, 12, 40)),
    (False, 192, 3): (25, 25, (1, 16, 50)), (False, 192, 5): (25, 25, (1, 16, 50)), (False, 192, 7): (25, 25, (1, 12, 40)),
    (False, 256, 3): (25, 25, (1, 12, 40)), (False, 256, 5): (25, 25, (1, 12, 40)), (False, 256, 7): (17, 27, (1, 12, 40)),
    (False, 384, 3): (17, 17, (1, 12, 40)), (False, 384, 5): (17, 17, (1, 12, 40)), (False, 384, 7): (17, 17, (1, 12, 40)),
    (False, 512, 3): (17, 17, (1, 12, 40)), (False, 512, 5): (19, 19, (1, 9)), (False, 512, 7): (17, 17, (1, 7, 20)),
    (True, 128, 3): (41, 41, (1, 9, 32)), (True, 128, 5): (41, 41, (1, 9, 32)), (True, 128, 7): (41, 41, (1, 9, 32)),
    (True, 192, 3): (25, 25, (1, 16, 50)), (True, 192, 5): (25, 25, (1, 16, 50)), (True, 192, 7): (25, 25, (1, 16, 50)),
    (True, 256, 3): (25, 25, (1, 12, 40)), (True, 256, 5): (25, 25, (1, 12, 40)), (True, 256, 7): (25, 25, (1, 12, 40)),
    (True, 384, 3): (17, 17, (1, 12, 40)), (True, 384, 5): (17, 17, (1, 12, 40)), (True, 384, 7): (17, 17, (1, 12, 40)),
    (True, 512, 3): (17, 17, (1, 12, 40)), (True, 512, 5): (19, 19, (1, 9)), (True, 512, 7): (19, 19, (1, 9)),
}

# ------------------------------------------------------------------------------------------------ sliding-window kernel
# Shapes every sliding-window case runs (all at one output row per group): the three of test_dwconv_ln; W % 4 = 1 with B = 3; a map
# whose pixel-group count leaves inactive lanes in the last wave of a grid of fewer than 8 blocks; a grid that is no multiple of 8 blocks.
SW_SHAPES = [(1, 1, 1), (2, 9, 11), (1, 2, 6), (3, 5, 13), (1, 3, 9), (2, 23, 45)]
SW_SHAPE_INACTIVE, SW_SHAPE_REMAP = (1, 3, 9), (2, 23, 45)
SW_AFFINES = ('ln', 'adaln', 'none', 'both')           # 'ln' is what qres17m runs
# (fmt, C, k, affine) of every sliding-window case at TH = 1: C = 144 / 288 with every affine mode (fp32 maps), the channel-per-lane
# widths with both affines (fp32 and bf16 maps)
SW_CASES = ([('f32', C, k, a) for C in SW_ONLY_WIDTHS for k in KS for a in SW_AFFINES]
            + [(fmt, C, k, 'both') for fmt in ('f32', 'bf16') for C in CL_WIDTHS for k in KS])
# the two-row instance: both affines, k = 7, C <= 192, one image of >= 100 000 pixels with odd H
SW_TH2_CASES = [('f32', 128, 7, 1, 251, 401), ('f32', 192, 7, 1, 251, 401)]


def named_instances():
    """The set of (family, fmt, C, k, TH, tpw > 1) the GPU test's tables name."""
    s = {(0, fmt, C, k, th, tpw > 1) for fmt, C, k, th, tpw, *_ in CL_CASES}
    s |= {(1, fmt, C, k, 1, False) for fmt, C, k, _ in SW_CASES}
    s |= {(1, fmt, C, k, 2, False) for fmt, C, k, *_ in SW_TH2_CASES}
    return s


def compiled_cl_instances():
    """Every (0, fmt, C, k, TH, tpw > 1) csrc/dwconv_cl*.hip instantiates: TH in 1 / 4 / 8 for k > 1, one-row tiles with one or several
    tiles per workgroup at k = 1."""
    return ({(0, fmt, C, k, th, False) for fmt in FMTS for C in CL_WIDTHS for k in KS if k > 1 for th in (1, 4, 8)}
            | {(0, fmt, C, 1, 1, many) for fmt in FMTS for C in CL_WIDTHS for many in (False, True)})
