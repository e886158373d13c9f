"""not-gpu: the arithmetic of tests/h2_cases.py.  Every form of the table is put to lvae_gemm_h2_choice -- the function the launch path
switches on (csrc/gemm_h2_choice.h) -- which must take it, name the table's instance and split-K form, and refuse the table's refusals;
the instantiations and the geometry constants of csrc/gemm_h2.hip, csrc/gemm_h2n.hip and csrc/gemm_h2p.hip (the launch_*<...> argument
lists, N_CS, n_d<NB>(), the tile sizes) are compared with the table, every instance must have a case, and every shape is checked to
straddle what it is listed for -- so that an edit of a shape, a rule or a new instance in the source fails here instead of quietly
narrowing what tests/test_gpu_h2_instances.py covers."""
import os
import re

import pytest

import h2_cases as hc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lossy-vae_amd', 'csrc')
AMODE = {'LVAE_A_PLAIN': hc.A_PLAIN, 'LVAE_A_PATCH2': hc.A_PATCH2, 'LVAE_A_CONV3': hc.A_CONV3}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope='module')
def h2():
    return _read('gemm_h2.hip')


@pytest.fixture(scope='module')
def h2n():
    return _read('gemm_h2n.hip')


@pytest.fixture(scope='module')
def h2p():
    return _read('gemm_h2p.hip')


@pytest.fixture(scope='module')
def L():
    from lvae import _native
    return _native.lib()


def _tile(args):
    a = [x.strip() for x in args.split(',')]
    assert 3 <= len(a) <= 5, args
    fold = {'true': True, 'false': False}[a[3]] if len(a) > 3 else False
    return hc.Tile(None, int(a[0]), int(a[1]), int(a[2]), fold, int(a[4]) if len(a) > 4 else 0)


CUS = (64, 256, 304)


def _sweep(cu):
    return [c for _, c in hc.all_cases()] + [hc.fold_threshold_case(cu, *s) for s in hc.FOLD_THRESHOLD_SPECS]


# ------------------------------------------------------------------------------------------------ the table is what a launch runs
def test_forms_run_the_instances_the_table_names(L):
    """Every form of every case, on devices of 64, 256 and 304 CUs: the library takes it, runs the instance the table names (where the
    table leaves the choice to the library: one that a forced form of the case names) and reduces split-K the way the form says.  Over
    the sweep the library reaches exactly the 23 instances of the table."""
    reached = set()
    for cu in CUS:
        for c in _sweep(cu):
            fs = hc.forms(c, cu)
            named = {f.instance for f in fs if f.instance is not None}
            for f in fs:
                rc, inst, splitk = hc.choice(L, hc.desc(c, f), cu)
                assert rc == 0, (cu, hc.case_id(c), f.name, rc)
                assert inst == f.instance if f.instance is not None else inst in named, (cu, hc.case_id(c), f.name, inst)
                assert splitk == hc.form_splitk(c, f), (cu, hc.case_id(c), f.name, splitk)
                reached.add(inst)
    assert reached == hc.all_instances(), reached ^ hc.all_instances()


def test_refusals_get_their_return_code(L):
    assert len(hc.refusals()) >= 12
    for cu in CUS:
        for c, cfg, want in hc.refusals():
            rc, _, _ = hc.choice(L, hc.desc(c, hc.Form(f'cfg {cfg}', 0, cfg, False, None)), cu)
            assert rc == want, (hc.case_id(c), cfg, rc)


def test_sources_instantiate_what_the_table_names(h2, h2n, h2p):
    """An instantiation added to a source without a case fails here; so does a change of the geometry the shapes are built around.
    (Which instance a launch runs is not read from the text: test_forms_run_the_instances_the_table_names asks the library.)"""
    # gemm_h2p.hip: the launch_h2p<...> argument lists are the five tiles and the FOLD pair
    assert re.search(r'template <int WM, int TN, int NBUF, bool FOLD = false, int NLOAD = 0>\s*int launch_h2p\(', h2p)
    found = [_tile(a) for a in re.findall(r'launch_h2p<([^>]+)>\(d, st\)', h2p)]
    assert len(re.findall(r'launch_h2p<', h2p)) == len(found) == len(hc.H2P_TILES) + 2 == 7
    assert {hc.instance_of(t) for t in found} == {hc.instance_of(t) for t in hc.H2P_TILES + (hc.FOLD_LOADERS, hc.FOLD_PLAIN)}
    for t in hc.H2P_TILES:                                   # cfg = 10 WM + TN, 23 the two-slot form of 21
        assert t.cfg == 10 * t.WM + t.TN or (t.cfg == 23 and (t.WM, t.TN, t.NBUF) == (2, 1, 2))
        assert t.NBUF in (2, 3) and not t.FOLD and not t.NLOAD
    assert sorted(hc.H2P_FORCE_CODES) == sorted(t.cfg for t in hc.H2P_TILES) and hc.H2P_DEFAULT in hc.H2P_FORCE_CODES
    assert len(re.findall(r'constexpr int BM = 64 \* WM, BN = 64 \* TN', h2p)) == 2                 # the kernel and its launcher
    assert 'const int nq = d.K / 32;' in h2p and hc.H2P_STAGE == 32
    assert (hc.tile_bm(hc.FOLD_LOADERS), hc.tile_bn(hc.FOLD_LOADERS)) == (128, 64) == (hc.tile_bm(hc.FOLD_PLAIN), hc.tile_bn(hc.FOLD_PLAIN))
    # gemm_h2.hip: two tile widths in the macro, five uses of it
    assert len(re.findall(r'launch_h2<', h2)) == 2
    assert tuple(int(x) for x in re.findall(r'launch_h2<(\d), G, AM>', h2)) == hc.H2_TNS
    uses = re.findall(r'LVAE_H2_LAUNCH\((true|false), (LVAE_A_\w+)\)', h2)
    assert tuple((int(g == 'true'), AMODE[a]) for g, a in uses) == hc.H2_LAUNCHES and len(set(uses)) == 5
    # tile: Cfg<WGM = 2, WGN = 2, TM = 2, TN> -> 32 * 2 * 2 rows, 32 * 2 * TN columns
    assert 'using C = Cfg<2, 2, 2, TN, 1, 32>;' in h2 and hc.H2_BM == 32 * 2 * 2 and hc.h2_bn(1) == 32 * 2
    assert 'constexpr int BN = 64 * TN' in h2 and '(d->M + 127) / 128' in h2
    # the look-ahead the K list is built around: stage 0 stored, k16 tiles 1 and 2 in registers
    assert 'load_set(1, nq > 1 ? 1 : nq - 1);' in h2 and 'load_set(0, nq > 2 ? 2 : nq - 1);' in h2
    # gemm_h2n.hip: three block counts in the macro, two uses of it
    assert len(re.findall(r'launch_h2n<', h2n)) == 3
    assert tuple(int(x) for x in re.findall(r'launch_h2n<(\d), AM>', h2n)) == hc.H2N_NBS
    uses = re.findall(r'LVAE_H2N_LAUNCH\((LVAE_A_\w+)\)', h2n)
    assert sorted(AMODE[a] for a in uses) == sorted(hc.H2N_AMODES) and len(uses) == 2
    assert hc.H2N_MAX_N == 32 * max(hc.H2N_NBS)
    assert f'constexpr int N_CS = {hc.H2N_CHUNK};' in h2n
    (nd,) = re.findall(r'template <int NB> constexpr int n_d\(\) \{ return (.*); \}', h2n)
    assert nd == 'NB <= 2 ? 8 : 4' and hc.H2N_PREFETCH == {nb: (8 if nb <= 2 else 4) for nb in hc.H2N_NBS}
    assert all(hc.H2N_CHUNK % v == 0 for v in hc.H2N_PREFETCH.values())
    assert 'dim3((d->M + 255) / 256), dim3(512)' in h2n and hc.H2N_BM == 256 == 8 * hc.H2N_WAVE_ROWS


def test_every_instance_has_a_case():
    assert len(hc.all_instances()) == 10 + 6 + 7
    for cu in (64, 256, 304):
        seen = {}
        cases = hc.all_cases() + [('fold', hc.fold_threshold_case(cu, *s)) for s in hc.FOLD_THRESHOLD_SPECS]
        for what, c in cases:
            for f in hc.forms(c, cu):
                if f.instance is not None:
                    seen.setdefault(f.instance, []).append((what, c))
        assert set(seen) == hc.all_instances(), hc.all_instances() ^ set(seen)
    # the forced forms of gemm_h2_kernel meet every instance with both tile widths, with and without split-K
    for g, am in hc.H2_LAUNCHES:
        for tn in hc.H2_TNS:
            assert any(what == 'h2' for what, _ in seen[('h2', tn, g, am)])
    # every pre-split tile meets every plain case it can take, and out_h2
    for t in hc.H2P_TILES:
        kinds = {what for what, _ in seen[hc.instance_of(t)]}
        assert {'h2p', 'out_h2'} <= kinds
        assert len([1 for what, _ in seen[hc.instance_of(t)] if what == 'h2p']) == len(hc.h2p_cases())
    assert any(c.out_h2 for _, c in seen[hc.instance_of(hc.FOLD_LOADERS)])
    for nb in hc.H2N_NBS:
        for am in hc.H2N_AMODES:
            cs = [c for _, c in seen[('h2n', nb, am)]]
            assert any(c.S > 1 for c in cs) and any(c.S == 1 and c.K % 32 == 16 for c in cs) and set(c.epi for c in cs) == set(hc.EPIS)


def test_forms_are_what_the_entry_points_take():
    seen = set()
    for what, c in hc.all_cases():
        assert (what, c) not in seen
        seen.add((what, c))
        fs = hc.forms(c)
        assert fs and len({f.name for f in fs}) == len(fs), c
        assert c.ldo >= c.N and c.epi in hc.EPIS and c.K % 16 == 0 and c.S >= 1
        assert {'h2': hc.h2_takes, 'h2p': hc.h2p_takes, 'h2n': hc.h2n_takes}.get(what, lambda c: True)(c), (what, c)
        if c.a_mode == hc.A_PLAIN:
            assert c.K0 + c.K1 == c.K and c.lda0 >= c.K0 and c.lda1 >= c.K1
        else:
            assert c.M == c.B * c.H * c.W and c.K == (4 if c.a_mode == hc.A_PATCH2 else 9) * c.K0 and c.K1 == 0
        if c.K % 32:                                # one kernel only
            assert {f.instance for f in fs} == {hc.h2n_instance(c)} and c.N <= hc.H2N_MAX_N
        for f in fs:
            if f.instance and f.instance[0] == 'h2':
                assert f.cfg == f.instance[1] and not f.a_h2 and hc.h2_takes(c)
            if f.instance and f.instance[0] == 'h2n':
                assert f.cfg == 3 or (c.K % 32 and f.cfg == 0)
                assert f.instance[1] == -(-c.N // 32) and hc.h2n_takes(c)
            if f.instance and f.instance[0] == 'h2p':
                assert f.a_h2 and hc.h2p_takes(c) and (f.cfg in hc.H2P_FORCE_CODES) == (c.S == 1)
            if f.cnt:
                assert c.S > 1 and not f.a_h2 and f.cfg in hc.H2_TNS
    # what a refusal records is what the rules above say
    for c, cfg, rc in hc.refusals():
        assert rc == hc.EINVAL and not hc.h2_takes(c) and (cfg in (1, 2) or not hc.h2n_takes(c))
    assert any(c.a_mode == hc.A_CONV3 and c.a_gelu for c, _, _ in hc.refusals())
    assert any(c.a_mode == hc.A_PLAIN and c.N > hc.H2N_MAX_N and cfg == 0 for c, cfg, _ in hc.refusals())
    assert any(c.a_mode == hc.A_PLAIN and c.K % 32 == 16 and cfg == 1 for c, cfg, _ in hc.refusals())


# ------------------------------------------------------------------------------------------------ the shapes straddle what they say
ROW_TILES = sorted({hc.H2_BM, hc.H2N_BM} | {hc.tile_bm(t) for t in hc.H2P_TILES})
COL_TILES = sorted({hc.h2_bn(tn) for tn in hc.H2_TNS} | {hc.tile_bn(t) for t in hc.H2P_TILES})


def test_m_and_n_straddle_every_tile():
    assert ROW_TILES == [128, 256] and COL_TILES == [64, 128]
    M = hc.RAGGED_M
    for bm in [64] + ROW_TILES:
        assert M > bm and M % bm != 0
    assert M % hc.H2N_BM == hc.H2N_WAVE_ROWS + 5                      # the last workgroup: one full wave and one of 5 rows
    assert hc.PLAIN_MS == (1, 63, M) and 63 < min(ROW_TILES) and 63 > hc.H2N_WAVE_ROWS
    for bn in COL_TILES:
        assert hc.NARROW_N < bn
        for N in hc.RAGGED_NS:
            assert N % bn != 0 and -(-N // bn) >= 3
    assert [N % 4 for N in hc.RAGGED_NS] == [2, 0] and hc.PLAIN_NS == (hc.NARROW_N,) + hc.RAGGED_NS and hc.NARROW_N % 4 == 0
    for lst, ms in ((hc.plain_cases(), hc.PLAIN_MS), (hc.h2n_plain_cases(), hc.PLAIN_MS)):
        ns, ks = (hc.PLAIN_NS, hc.PLAIN_KS) if lst[0].K in hc.PLAIN_KS else (hc.H2N_NS, hc.H2N_KS)
        for m in ms:
            got = {(c.N, c.K) for c in lst if c.M == m and not c.K1 and not c.a_gelu and c.lda0 == c.K0 and c.ldo == c.N}
            assert got == {(N, K) for N in ns for K in ks}, m
        got = {(c.N, c.K, c.epi) for c in lst if c.M == M and not c.K1 and not c.a_gelu and c.lda0 == c.K0 and c.ldo == c.N}
        assert got == {(N, K, e) for N in ns for K in ks for e in hc.EPIS}             # the ragged rows meet every epilogue
    plain = hc.plain_cases()
    assert any(c.lda0 > c.K0 and not c.K1 for c in plain)
    assert {c.ldo for c in plain if c.ldo != c.N} == {296, 293, 295}
    assert any(c.ldo > c.N and c.ldo % 4 == 0 and c.N % 4 == 0 for c in plain)            # 16-byte stores into padded rows
    assert any(c.ldo % 4 != 0 and c.N % 4 == 0 for c in plain)                            # scalar stores forced by ldo alone
    assert any(c.ldo > c.N and c.N % 4 != 0 for c in plain)
    assert any((c.K0, c.K1) == (16, 48) and c.lda0 > c.K0 and c.lda1 > c.K1 for c in plain)
    assert any(c.a_gelu for c in plain)
    # the pre-split kernel sees all of it but a padded / second source and GELU on load
    assert {(c.M, c.N, c.K, c.epi, c.ldo) for c in hc.h2p_cases()} == {(c.M, c.N, c.K, c.epi, c.ldo) for c in plain
                                                                       if not c.K1 and c.lda0 == c.K0 and not c.a_gelu}
    # gemm_h2n: a full and a cut last 32-column block for every NB, the scalar path on a cut block
    for nb in hc.H2N_NBS:
        ns = [N for N in hc.H2N_NS if -(-N // 32) == nb]
        assert any(N % 32 == 0 for N in ns) and any(N % 32 != 0 for N in ns), nb
    assert any(N % 4 != 0 for N in hc.H2N_NS) and max(hc.H2N_NS) == hc.H2N_MAX_N
    h2n = hc.h2n_plain_cases()
    assert any(c.ldo > c.N and c.ldo % 4 == 0 for c in h2n) and any(c.ldo % 4 != 0 and c.N % 4 == 0 for c in h2n)
    assert any(c.ldo > c.N and c.N % 4 != 0 for c in h2n) and any(c.lda0 > c.K0 for c in h2n)


def test_k_crosses_every_pipeline_depth():
    ks = hc.PLAIN_KS
    assert all(k % 32 == 0 for k in ks) and [k // hc.H2P_STAGE for k in ks] == [1, 2, 3, 4, 5, 8]
    # gemm_h2_kernel: k16 stage 0 stored and stages 1, 2 loaded before the loop
    assert min(ks) // 16 < 3 and sorted(ks)[1] // 16 > 3
    # gemm_h2p_kernel: NBUF - 1 stages in flight; below it (the clamp of the prologue), on it, and every remainder of the ring
    for t in hc.H2P_TILES + (hc.FOLD_LOADERS, hc.FOLD_PLAIN):
        nqs = [k // hc.H2P_STAGE for k in ks]
        assert any(nq == t.NBUF - 1 for nq in nqs)
        assert t.NBUF == 2 or any(nq < t.NBUF - 1 for nq in nqs)
        assert {nq % t.NBUF for nq in nqs if nq >= t.NBUF} == set(range(t.NBUF))
    # gemm_h2n_kernel
    steps = [k // 16 for k in hc.H2N_KS]
    assert steps == [1, 3, 8, 9, 17] and steps[0] < min(hc.H2N_PREFETCH.values())
    assert hc.H2N_KS[1] % 32 == 16 and steps[1] < min(hc.H2N_PREFETCH.values())
    assert steps[2] == hc.H2N_CHUNK and steps[3] == hc.H2N_CHUNK + 1 and steps[4] == 2 * hc.H2N_CHUNK + 1 and hc.H2N_KS[4] % 32 == 16
    cins = sorted({c.K0 for c in hc.h2n_conv3_cases()})
    assert cins == [16, 48] and 9 * 48 // 16 == 3 * hc.H2N_CHUNK + 3
    for nb in hc.H2N_NBS:
        for cin in cins:
            assert any(c.K0 == cin and -(-c.N // 32) == nb for c in hc.h2n_conv3_cases())


def test_gather_maps():
    B, H, W = hc.gc.GATHER_MAP
    rows = B * H * W
    for bm in ROW_TILES:
        assert rows > bm and rows % bm != 0 and (H * W) % bm != 0 and B >= 2 and bm % W != 0
    assert (H * W) % hc.H2N_WAVE_ROWS != 0
    conv3, patch2 = hc.conv3_cases(), hc.patch2_cases()
    for lst in (conv3, patch2, hc.h2n_conv3_cases()):
        assert any((c.B, c.H, c.W) == (B, H, W) for c in lst)
    assert {c.K0 for c in patch2} == {8, 40} and {c.K0 for c in conv3} == {32}
    assert {c.K0 for c, _, _ in hc.conv3_refusals()} == {16}
    for a_gelu in (0, 1):
        for bn in COL_TILES:
            ns = {c.N for c in conv3 if c.a_gelu == a_gelu and c.M == rows}
            assert any(N < bn for N in ns) and any(N > bn and N % bn for N in ns)
        assert any(c.a_gelu == a_gelu and (c.H, c.W) == (1, 1) for c in conv3)
    assert any((c.H, c.W) == (1, 1) for c in hc.h2n_conv3_cases())
    for bn in COL_TILES:
        ns = {c.N for c in patch2}
        assert any(N < bn for N in ns) and any(N > bn and N % bn for N in ns)
    for lst in (conv3, patch2):
        assert {c.epi for c in lst} == set(hc.EPIS)


def test_out_h2_cases():
    cs = hc.out_h2_cases()
    assert {c.N for c in cs} == set(hc.OUT_H2_NS) == {32, 96, 288} and all(c.N % 32 == 0 and c.ldo == c.N and c.out_h2 for c in cs)
    assert {(c.N, c.epi, c.S) for c in cs} == {(N, e, S) for N in hc.OUT_H2_NS for e in (hc.EPI_BIAS, hc.EPI_BIAS_GELU) for S in (1, 3)}
    for bn in COL_TILES:
        assert 288 % bn != 0 and 288 > bn and 32 < bn
    for c in cs:
        assert c.M == hc.RAGGED_M
        inst = {f.instance for f in hc.forms(c)}
        if c.S == 1:
            assert inst >= {hc.h2_instance(c, 1), hc.h2_instance(c, 2)} | {hc.instance_of(t) for t in hc.H2P_TILES}
        else:
            assert inst == {hc.instance_of(hc.FOLD_LOADERS)} and c.K // hc.H2P_STAGE // c.S == 1


def test_split_k_cases():
    for c in hc.split_cases():
        assert c.S > 1 and c.N % 4 == 0 and c.ldo == c.N and hc.forms(c)
    par = hc.parallel_split_cases()
    assert {(c.M, c.N, c.K, c.S) for c in par} == {(M, N, 256, S) for M in (63, hc.RAGGED_M) for N in (64, 292) for S in (2, 4)}
    for c in par:
        names = [f.name for f in hc.forms(c)]
        assert {'cfg 1 reduce launch', 'cfg 1 counters', 'cfg 2 reduce launch', 'cfg 2 counters'} <= set(names)
        assert any(f.a_h2 for f in hc.forms(c)) and (c.N > hc.H2N_MAX_N or 'cfg 3 serial' in names)
    assert {hc.cnt_in_kernel(c) for c in par} == {True, False}
    assert {c.epi for c in par} == set(hc.EPIS)
    fold = hc.fold_cases()
    assert {(c.K, c.S) for c in fold} == {(256, 2), (256, 4), (256, 8), (96, 3)} and {c.N for c in fold} == {64, 292}
    assert sorted({c.K // hc.H2P_STAGE // c.S for c in fold}) == [1, 2, 4]
    assert any(c.K // hc.H2P_STAGE == hc.FOLD_LOADERS.NBUF and c.K // hc.H2P_STAGE // c.S == 1 for c in fold)
    assert all(hc.h2p_takes(c) and hc.h2_takes(c) for c in fold) and {c.epi for c in fold} == set(hc.EPIS)
    for N in (64, 292):                         # every straight-line tail of FOLD and the generic one
        assert {c.epi for c in fold if c.N == N} == set(hc.EPIS)
    ser = hc.h2n_serial_cases()
    assert {(c.K, c.S) for c in ser} == {(96, 2), (96, 3), (288, 2), (432, 3)}
    assert {-(-c.N // 32) for c in ser} == set(hc.H2N_NBS)
    for c in ser:
        per = c.K // 16 // c.S
        assert hc.h2n_takes(c) and (c.K // 16) % c.S == 0
        assert (c.K != 96 or per < hc.H2N_CHUNK) and (c.K != 288 or (per % hc.H2N_CHUNK != 0 and per > hc.H2N_CHUNK))
        assert (c.K != 432) or (c.a_mode == hc.A_CONV3 and per == 9)
        if len(hc.forms(c)) == 1:               # no second form: the own-arithmetic bound carries the case
            assert any(o.epi == hc.EPI_BIAS and o._replace(epi=c.epi) == c for o in ser)
        else:
            assert (c.K, c.S) == (96, 3)
    assert hc.split_cnt_entries(hc.RAGGED_M, 292) >= -(-hc.RAGGED_M // hc.H2_BM) * -(-292 // 64)


def test_fold_threshold_for_any_cu_count():
    assert hc.fold_threshold_ms(256) == (549, 33 * 128 - 5) and hc.fold_tiles(33 * 128 - 5, 512) == 264 and hc.fold_tiles(549, 512) == 40
    for cu in range(45, 513):
        for side, N, epi in hc.FOLD_THRESHOLD_SPECS:
            c = hc.fold_threshold_case(cu, side, N, epi)
            assert c.M % 128 != 0 and c.M > 128 and c.S == 2 and hc.h2p_takes(c) and hc.h2_takes(c)
            assert hc.fold_loaders(c.M, c.N, cu) == (side == 'below')
            (f,) = [f for f in hc.forms(c, cu) if f.a_h2]
            assert f.instance == hc.instance_of(hc.FOLD_LOADERS if side == 'below' else hc.FOLD_PLAIN)
            if side == 'above':                 # the smallest ragged M above
                assert hc.fold_loaders(c.M - 128, c.N, cu)
    specs = hc.FOLD_THRESHOLD_SPECS
    for side in ('below', 'above'):
        assert {e for s, _, e in specs if s == side} == set(hc.EPIS)
        assert {N % 64 == 0 for s, N, _ in specs if s == side} == {True, False}
        assert any(N % 32 == 0 and e == hc.EPI_BIAS_GELU for s, N, e in specs if s == side)          # also run with out_h2


def test_row_slices():
    for kernel, c in hc.ROW_CASES.items():
        assert c.M == hc.RAGGED_M and hc.forms(c) and {'h2': hc.h2_takes, 'h2p': hc.h2p_takes, 'h2n': hc.h2n_takes}[kernel](c)
    assert hc.ROW_CASES['h2n'].K % 32 == 16
    (r0, n), (r1, n1) = hc.ROW_SLICES
    assert r0 % hc.H2N_WAVE_ROWS != 0 and all(r0 // bm != (r0 + n - 1) // bm for bm in (64, 128)) and r0 + n <= hc.RAGGED_M
    assert (r1, n1) == (hc.RAGGED_M - 1, 1)
