"""not-gpu: the arithmetic of tests/gemm_cases.py.  The configuration list and the remaps are compared with the text of
csrc/gemm_f32.hip (the `typedef Cfg<...>` lines, launch_mode's switch and its `id = ` remaps), and every shape is checked to
straddle the tiles it is listed for -- so that an edit of a shape, or a new configuration in the source, fails here instead of
quietly narrowing what tests/test_gpu_gemm_configs.py covers."""
import os
import re

import pytest

import gemm_cases as gc

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lossy-vae_amd', 'csrc', 'gemm_f32.hip')


@pytest.fixture(scope='module')
def src():
    with open(SRC) as f:
        return f.read()


def test_config_table_is_the_source(src):
    tiles = {}
    for args, name in re.findall(r'typedef Cfg<([\d, ]+)> (Cfg\w+);', src):
        a = [int(x) for x in args.split(',')]
        wgm, wgn, tm, tn = a[:4]
        nbuf = a[4] if len(a) > 4 else 2
        bk = a[5] if len(a) > 5 else 32
        tiles[name] = (32 * wgm * tm, 32 * wgn * tn, bk, nbuf)
    switch = src[src.index('switch (id) {'):]
    switch = switch[:switch.index('\n    }\n')]
    by_id = {int(i): n for i, n in re.findall(r'case (\d+): return launch_cfg<(Cfg\w+), AMODE>', switch)}
    (default,) = re.findall(r'default: return launch_cfg<(Cfg\w+), AMODE>', switch)
    assert gc.DEFAULT_ID not in by_id
    by_id[gc.DEFAULT_ID] = default
    assert sorted(by_id) == list(range(gc.NUM_CONFIGS)) == [c.id for c in gc.CONFIGS]
    assert len(set(by_id.values())) == gc.NUM_CONFIGS == len(tiles)
    for c in gc.CONFIGS:
        assert by_id[c.id] == c.name, c
        assert tiles[c.name] == (c.BM, c.BN, c.BK, c.stages), c
    assert re.search(r'lvae_gemm_num_configs\(void\) \{ return (\d+); \}', src).group(1) == str(gc.NUM_CONFIGS)


def test_remaps_are_the_source(src):
    found = re.findall(r'if \((d->prec [!=]= \d|ksp\(d\) > 1) && id == (\d+)\) id = (\d+);', src)
    norm = {'d->prec != 0': 'prec != 0', 'd->prec == 2': 'prec == 2', 'ksp(d) > 1': 'split'}
    assert tuple((norm[c], int(a), int(b)) for c, a, b in found) == gc.REMAPS
    # the kernels the remaps exist for: no bf16 / bf16x3 main loop for a 64-deep configuration, split-K slices counted in 32-deep tiles
    for c in gc.CONFIGS:
        for prec in (1, 2):
            assert gc.CONFIGS[gc.effective_id(c.id, prec)].BK == 32
            e = gc.CONFIGS[gc.effective_id(c.id, prec)]
            if c.id != 7:
                assert (e.BM, e.BN) == (c.BM, c.BN)
        for prec in gc.PRECS:
            assert gc.CONFIGS[gc.effective_id(c.id, prec, split=True)].BK == 32
        assert gc.effective_id(c.id, 0) == c.id


def test_every_instance_is_named():
    """Three translation units x three arithmetics x 12 ids: each has a case, and after the remaps the forced ids reach every kernel
    instance a launch can run -- 12 under prec 0, 10 under prec 1 (no 64-deep ones), 9 under prec 2 (nor CfgD256)."""
    named = set()
    for a in gc.A_MODES:
        for p in gc.PRECS:
            assert gc.cases(p, a), (a, p)
            assert all(c.a_mode == a for c in gc.cases(p, a))
            for c in gc.CONFIGS:                     # the GPU test forces cfg = 1 .. NUM_CONFIGS in every case
                named.add((a, p, gc.effective_id(c.id, p)))
    assert named == gc.reachable_instances()
    per = {(a, p): sorted(i for aa, pp, i in named if (aa, pp) == (a, p)) for a in gc.A_MODES for p in gc.PRECS}
    for a in gc.A_MODES:
        assert per[(a, 0)] == list(range(12))
        assert per[(a, 1)] == list(range(10))
        assert per[(a, 2)] == [0, 1, 2, 3, 4, 5, 6, 8, 9]


@pytest.mark.parametrize('cfg', gc.CONFIGS, ids=lambda c: c.name)
def test_ragged_shapes_straddle_every_tile(cfg):
    M = gc.RAGGED_M
    assert M > cfg.BM and M % cfg.BM != 0
    for N in gc.RAGGED_NS:
        assert N % cfg.BN != 0 and -(-N // cfg.BN) >= 2, N
    assert gc.NARROW_N < cfg.BN
    assert any(N % 4 == 0 for N in gc.RAGGED_NS) and any(N % 4 != 0 for N in gc.RAGGED_NS)
    assert 1 in gc.PLAIN_MS and any(1 < m < cfg.BM for m in gc.PLAIN_MS)
    for prec in gc.PRECS:
        shapes = {(c.M, c.N) for c in gc.plain_cases(prec)}
        assert {(M, N) for N in gc.PLAIN_NS} <= shapes
        for N in gc.PLAIN_NS:                          # the ragged rows meet every K and every epilogue
            got = {(c.K, c.epi) for c in gc.plain_cases(prec) if (c.M, c.N) == (M, N) and not c.K1 and not c.a_gelu}
            assert got >= {(K, e) for K in gc.PLAIN_KS[prec] for e in gc.EPIS}
    # the gather map: more than one m-tile with a cut last one, an image boundary inside a tile, a tile boundary inside an image
    B, H, W = gc.GATHER_MAP
    rows = B * H * W
    assert rows > cfg.BM and rows % cfg.BM != 0
    assert (H * W) % cfg.BM != 0 and B >= 2 and cfg.BM % W != 0
    for a in (gc.A_PATCH2, gc.A_CONV3):
        for prec in gc.PRECS:
            ns = {c.N for c in gc.cases(prec, a) if c.M == rows}
            assert any(N < cfg.BN for N in ns)
            assert any(N % cfg.BN != 0 and N > cfg.BN for N in ns) or cfg.BN >= 128      # 100 columns: several tiles up to BN = 64
    bs, hs, ws = gc.STORE_MAP
    assert (bs * hs * ws) % cfg.BM != 0 and bs >= 2


@pytest.mark.parametrize('cfg', gc.CONFIGS, ids=lambda c: c.name)
@pytest.mark.parametrize('prec', gc.PRECS)
def test_k_list_crosses_every_k_tile(cfg, prec):
    kt = gc.k_tile(gc.CONFIGS[gc.effective_id(cfg.id, prec)], prec)
    ks = gc.PLAIN_KS[prec]
    tiles = [-(-k // kt) for k in ks]
    assert any(k < kt for k in ks)
    assert any(k > kt and k % kt != 0 for k in ks)
    assert any(t % 2 == 1 and t >= 3 for t in tiles), tiles        # both LDS stages refilled, the loop ends on the first
    assert any(t % 2 == 0 for t in tiles), tiles
    assert all(k % 4 == 0 for k in ks) and (prec == 0 or all(k % 8 == 0 for k in ks))
    assert 8 in ks                                                # the product's fuse_feature_and_z


def test_case_arguments_are_ones_the_library_takes():
    seen = set()
    for prec, c in gc.all_cases():
        assert (prec, c) not in seen
        seen.add((prec, c))
        assert c.K % 4 == 0 and c.K0 % 4 == 0 and c.K1 % 4 == 0 and (prec == 0 or c.K % 8 == 0)
        assert c.ldo >= c.N and c.epi in gc.EPIS
        if c.a_mode == gc.A_PLAIN:
            assert c.K0 + c.K1 == c.K and c.lda0 >= c.K0 and c.lda0 % 4 == 0 and c.lda1 % 4 == 0 and (c.lda1 >= c.K1)
        else:
            assert c.M == c.B * c.H * c.W and c.K == (4 if c.a_mode == gc.A_PATCH2 else 9) * c.K0 and c.K1 == 0
    plain = gc.plain_cases(0)
    assert any(c.lda0 > c.K0 and not c.K1 for c in plain)
    assert any(c.ldo > c.N and c.ldo % 4 == 0 and c.N % 4 == 0 for c in plain)            # 16-byte stores into padded rows
    assert any(c.ldo % 4 != 0 and c.N % 4 == 0 for c in plain)                            # scalar stores forced by ldo alone
    assert any(c.ldo > c.N and c.N % 4 != 0 for c in plain)
    assert any(c.K1 and c.lda0 > c.K0 and c.lda1 > c.K1 for c in plain)
    assert any(c.a_gelu for c in plain) and any(c.a_gelu for c in gc.conv3_cases(0))
    assert any(c.H == 1 and c.W == 1 for c in gc.conv3_cases(0))
    assert len(seen) == 363


def test_split_k_cases():
    for s in gc.split_cases():
        assert s.K % (32 * s.S) == 0 and (s.prec != 1 or s.K % (64 * s.S) == 0) and s.N % 4 == 0
    for prec in gc.PRECS:
        got = {(s.M, s.N, s.S) for s in gc.split_cases() if s.prec == prec and s.K == 256}
        assert got == {(M, N, S) for M in (63, 549) for N in (64, 292) for S in (2, 4)}
    assert any(s.prec == 1 and (s.K // s.S) // 64 >= 2 for s in gc.split_cases())
    assert {s.epi for s in gc.split_cases()} == set(gc.EPIS)
    # one counter per tile of the smallest tile any configuration has
    bm, bn = min(c.BM for c in gc.CONFIGS), min(c.BN for c in gc.CONFIGS)
    for s in gc.split_cases():
        assert gc.split_cnt_entries(s.M, s.N) >= max(-(-s.M // c.BM) * -(-s.N // c.BN) for c in gc.CONFIGS)
        assert gc.split_cnt_entries(s.M, s.N) == -(-s.M // bm) * -(-s.N // bn)


def test_store_shapes():
    widths = sorted({c.BN for c in gc.CONFIGS})
    r, cout = gc.SHUFFLE_SHAPES[0]
    n = r * r * cout
    assert cout % 4 == 0
    for bn in widths:
        if bn >= 128:       # a group boundary strictly inside the first tile
            assert any(0 < g * cout < min(bn, n) and (g * cout) % 32 != 0 for g in range(1, r * r))
        assert n % bn != 0 or bn == 32
    assert any(co % 4 != 0 for _, co in gc.SHUFFLE_SHAPES)
    assert all(k % 32 == 0 for k in gc.STORE_KS)
    assert all(n % (r * r) == 0 and n // (r * r) == 3 for r, n in gc.IMAGE_SHAPES)
