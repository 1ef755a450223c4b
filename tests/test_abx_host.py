"""CPU checks of the ABX feature: the numpy oracle against brute force (cost, carried length, tie rule, cheapest path of a given length),
a hand-computed ABX example through counts, table and score, the .ali reader and its refusals, spans to rows, cell keys, seeded
subsampling, the exported symbols and source lists, every -22 / ValueError of st_dtw_pairs and st_abx_count before a device is touched,
and the --abx-ali-dir parser rules."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import abx_oracle as O  # noqa: E402
import dtw_oracle  # noqa: E402


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('n', [1, 2, 3, 4])
@pytest.mark.parametrize('m', [1, 2, 3, 4])
def test_oracle_cost_and_length_equal_brute_force(n, m):
    for seed in range(6):
        rs = np.random.RandomState(100 * n + 10 * m + seed)
        x, y = rs.randn(n, 1 + seed % 3), rs.randn(m, 1 + seed % 3)
        bf = dtw_oracle.brute_force(x, y)
        d = O.distances(x, y, 'euclid')
        c, L = O.dtw_len(d)
        assert abs(c - bf[0][0]) <= 1e-12 * max(1.0, bf[0][0]) and max(n, m) <= L <= n + m - 1
        assert L == len(dtw_oracle.dtw(x, y)[1])                       # the carried length is the length of the traced-back path
        if len(bf) == 1 or bf[1][0] - bf[0][0] > 1e-9:
            assert L == len(bf[0][1])
        c32, L32 = O.dtw_len(O.distances(x.astype(np.float32), y.astype(np.float32), 'euclid', np.float32))
        assert c32.dtype == np.float32 and abs(float(c32) - bf[0][0]) <= 1e-5 * max(1.0, bf[0][0])
        # the cheapest path of every length, against the enumeration
        for K in range(0, n + m + 1):
            want = min([cost for cost, cells in bf if len(cells) == K], default=np.inf)
            got = O.min_cost_with_len(d, K)
            assert (got == want == np.inf) or abs(got - want) <= 1e-12 * max(1.0, want), (K, got, want)
        assert abs(min(O.min_cost_with_len(d, K) for K in range(1, n + m)) - bf[0][0]) <= 1e-12 * max(1.0, bf[0][0])


def test_oracle_tie_rule_on_constant_input():
    for metric in O.METRICS:
        for n in (1, 2, 5, 17):
            x = np.full((n, 2), 0.5)
            assert O.pair(x, x, metric)[1:] == (0.0, n)                                    # square: the pure diagonal
            assert O.dtw_len(np.ones((n, 1)))[1] == n and O.dtw_len(np.ones((1, n)))[1] == n
    # every cost equal, n != m: the diagonal wins every tie, then (i-1, j), then (i, j-1): the traced path has max(n, m) cells
    for n, m in ((4, 2), (2, 4), (3, 7), (64, 1), (5, 64)):
        c, L = O.dtw_len(np.ones((n, m)))
        assert L == max(n, m) == len(dtw_oracle.dtw(np.ones((n, 1)), np.zeros((m, 1)))[1]) and c == max(n, m)
    # a tie between the diagonal and (i-1, j) at the corner goes to the diagonal; a strictly cheaper detour is taken
    assert O.dtw_len(np.array([[1.0, 5.0], [0.0, 1.0]])) == (2.0, 2)
    assert O.dtw_len(np.array([[1.0, 5.0], [0.0, 1.0], [0.0, 1.0]])) == (2.0, 3)
    assert O.dtw_len(np.array([[1.0, 0.0], [9.0, 1.0]])) == (2.0, 2) and O.dtw_len(np.array([[1.0, -0.5], [9.0, 1.0]])) == (1.5, 3)
    assert O.dtw_len(np.array([[1.0, 9.0, 9.0], [0.0, 9.0, 9.0], [0.0, 0.0, 1.0]])) == (2.0, 4)      # down the first column, then along the last row
    d = np.array([[1.0, np.nan], [0.0, 1.0]])
    assert np.isnan(O.dtw_len(d)[0]) and O.dtw_len(d)[1] == 0


def test_oracle_frame_distances():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    y = np.array([[6.0, 8.0], [0.0, 0.0], [0.0, 2.0], [-1.0, 0.0]])
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        ang = O.distances(x, y, 'angular', dtype)
        assert ang.dtype == dtype
        want = np.array([[0.0, 0.5, np.arccos(0.8) / np.pi, 1 - np.arccos(0.6) / np.pi], [0.5, 0.0, 0.5, 0.5], [np.arccos(0.6) / np.pi, 0.5, 0.5, 1.0]])
        assert np.abs(ang - want).max() <= tol
        assert np.abs(O.distances(x, y, 'euclid', dtype) - np.array([[5, 5, np.sqrt(13), np.sqrt(32)], [10, 0, 2, 1], [np.sqrt(89), 1, np.sqrt(5), 2]])).max() <= 10 * tol
    p, q = np.array([[0.5, 0.5, 0.0]]), np.array([[0.25, 0.25, 0.5], [0.5, 0.5, 0.0]])
    kl = O.distances(p, q, 'kl')
    want = 0.5 * (2 * 0.25 * (np.log(0.5 + 1e-10) - np.log(0.25 + 1e-10)) - 0.5 * (np.log(1e-10) - np.log(0.5 + 1e-10)))
    assert abs(kl[0, 0] - want) <= 1e-12 and kl[0, 1] == 0.0
    assert np.isnan(O.distances(np.array([[0.5, -0.1]]), q[:, :2], 'kl')).all()
    assert O.eps(5, 7, 13, 'euclid') < O.eps(5, 7, 13, 'angular') < O.eps(5, 7, 13, 'kl') < 1e-4


# ---------------------------------------------------------------- a hand-computed example
HAND = {('a1', 'a2'): 1, ('a1', 'b1'): 2, ('a2', 'b1'): 1,
        ('a3', 'a4'): 3, ('a3', 'c1'): 1, ('a3', 'c2'): 3, ('a4', 'c1'): 4, ('a4', 'c2'): 2, ('c1', 'c2'): 2,
        ('a3', 'b2'): 5, ('a4', 'b2'): 5, ('b2', 'c1'): 5, ('b2', 'c2'): 5}


def test_hand_computed_example_through_counts_table_and_score():
    """cell 10: a1 a2 | b1; cell 20: a3 a4 | b2 | c1 c2 (labels a = 0, b = 1, c = 2).  By hand:
    cell 10 (a, b): X = a1: d(a2, a1) = 1 < d(b1, a1) = 2, right; X = a2: d(a1, a2) = 1 == d(b1, a2) = 1, tied -> (0, 1, 0, 2), error 0.25
    cell 20 (a, b): 3 < 5 twice -> (0, 0, 0, 2); (a, c): X = a3: 3 > 1 wrong, 3 == 3 tied; X = a4: 3 < 4 right, 3 > 2 wrong -> (2, 1, 0, 4), 0.625
    cell 20 (c, a): X = c1: 2 > 1 wrong, 2 < 4 right; X = c2: 2 < 3 right, 2 == 2 tied -> (1, 1, 0, 4), 0.375; (c, b): 2 < 5 twice -> (0, 0, 0, 2)
    table: (a, b) over two cells (0.25 + 0) / 2 = 0.125; score = (0.125 + 0.625 + 0.375 + 0) / 4 = 0.28125"""
    from semi_tts_amd import abx as A
    names = ['c2', 'a1', 'b2', 'a4', 'b1', 'c1', 'a2', 'a3']                                   # any order
    label = np.array(['abc'.index(s[0]) for s in names])
    cell = np.array([10 if s in ('a1', 'a2', 'b1') else 20 for s in names])
    dist = lambda p, q: float(HAND[tuple(sorted((names[p], names[q])))])                        # noqa: E731
    pl = A.plan(label, cell, max_items=50, seed=0)
    assert [names[k] for k in pl.keep] == ['a1', 'a2', 'b1', 'a4', 'a3', 'b2', 'c2', 'c1'] and pl.dmat_len == 9 + 25
    assert len(pl.pair_a) == 3 + 10 and (np.diff(pl.pair_a.astype(int)[:3]) >= 0).all() and pl.pair_a.dtype == np.int32
    dmat = np.zeros(pl.dmat_len)
    for a, b, ab, ba in zip(pl.pair_a, pl.pair_b, pl.pos_ab, pl.pos_ba):
        dmat[ab] = dmat[ba] = dist(a, b)
    counts = [O.triple_counts(dmat[off:off + nc * nc].reshape(nc, nc), range(a0, a1), range(b0, b1)) for off, nc, a0, a1, b0, b1 in pl.blocks]
    got = {(int(c), int(a), int(b)): v for c, a, b, v in zip(pl.block_cell, pl.block_a, pl.block_b, counts)}
    want = {(10, 0, 1): (0, 1, 0, 2), (20, 0, 1): (0, 0, 0, 2), (20, 0, 2): (2, 1, 0, 4), (20, 2, 0): (1, 1, 0, 4), (20, 2, 1): (0, 0, 0, 2)}
    assert got == want
    agg = A.aggregate(pl.block_a, pl.block_b, counts)
    assert agg.table == [(0, 1, 2, 4, 0.125), (0, 2, 1, 4, 0.625), (2, 0, 1, 4, 0.375), (2, 1, 1, 2, 0.0)] and agg.score == 0.28125
    assert A.format_abx_csv(agg.table, 'abc') == ('phone_a,phone_b,cells,triples,error\na,b,2,4,0.125000\na,c,1,4,0.625000\n'
                                                  'c,a,1,4,0.375000\nc,b,1,2,0.000000\n')
    # the oracle's own brute force says the same
    blocks, table, score = O.abx(dist, label, cell)
    assert blocks == want and score == 0.28125 and table[(0, 1)] == (2, 4, 0.125)
    # NaN triples leave the denominator; a block without a triple left has no error and no row
    agg = A.aggregate([0, 0, 1], [1, 1, 0], [(1, 0, 2, 4), (0, 0, 2, 2), (0, 2, 0, 2)])
    assert agg.table == [(0, 1, 1, 2, 0.5), (1, 0, 1, 2, 0.5)] and agg.score == 0.5 and np.isnan(agg.block_error[1])
    assert np.isnan(A.aggregate([], [], np.zeros((0, 4))).score)
    assert O.triple_counts(dmat[:9].reshape(3, 3), [0, 1], [2]) == O.triple_counts_fast(dmat[:9].reshape(3, 3), [0, 1], [2]) == (0, 1, 0, 2)


def test_subsampling_is_deterministic_per_seed():
    from semi_tts_amd import abx as A
    rs = np.random.RandomState(0)
    label, cell = rs.randint(0, 3, 200), rs.randint(0, 2, 200)
    a, b, c = A.subsample(label, cell, 7, 3), A.subsample(label, cell, 7, 3), A.subsample(label, cell, 7, 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and len(a) == len(c) == 6 * 7 == len(set(a.tolist()))
    key = list(zip(cell[a].tolist(), label[a].tolist(), a.tolist()))
    assert key == sorted(key)                                       # by cell, then label, then index
    assert np.array_equal(A.subsample(label, cell, 200, 0), np.lexsort((np.arange(200), label, cell)))      # nothing to cut: no draw
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_items'):
            A.subsample(label, cell, bad, 0)
    with pytest.raises(ValueError, match='one of each'):
        A.plan(label, cell[:5])
    pl = A.plan([0, 0, 1], [0, 0, 1])                               # no cell with two phones: nothing to compute
    assert len(pl.blocks) == 0 and len(pl.pair_a) == 0 and pl.dmat_len == 0


# ---------------------------------------------------------------- .ali files, spans, cells
def _ali(path, body, header='# score=-12.500000 frames=20 frame_s=0.050000'):
    path.write_text((header + '\n' if header else '') + body)
    return str(path)


def test_ali_reader_and_every_refusal(tmp_path):
    from semi_tts_amd import abx as A
    from semi_tts_amd.ctc_align import format_ali
    f = tmp_path / 'u.ali'
    f.write_text(format_ali(-3.25, 20, 0.05, [5, 6, 5], [2, 6, 11], [4, 9, 15], vocab=None))
    ali = A.read_ali(str(f))
    assert ali == A.Ali(20, 0.05, ['5', '6', '5'], [2, 6, 11], [4, 9, 15])
    f.write_text(format_ali(-3.25, 20, 0.05, [3, 4], [0, 6], [4, 20], vocab=['<p>', '<s>', '<e>', 'AA', 'B']))
    assert A.read_ali(str(f)).symbols == ['AA', 'B']
    cases = [('', 'u.ali: no .* header', None), ('AA\t1\t2\n', 'u.ali: no .* header', None),
             ('AA\t1\t2\n', 'u.ali: the header needs', '# score=1.0 frame_s=0.05'), ('AA\t1\t2\n', 'u.ali: the header needs', '# frames=x frame_s=0.05'),
             ('AA\t1\t2\n', 'both must be positive', '# frames=0 frame_s=0.05'), ('AA\t1\t2\n', 'both must be positive', '# frames=5 frame_s=0'),
             ('AA\t1\n', 'u.ali: malformed line', 0), ('AA\tx\t2\n', 'u.ali: malformed line', 0), ('AA\t3\t2\n', 'u.ali: line .*0 <= start <= end', 0),
             ('AA\t-1\t2\n', 'u.ali: line', 0), ('AA\t1\t21\n', 'u.ali: line', 0), ('AA\t5\t6\nB\t4\t7\n', 'starts must not decrease', 0),
             ('', 'u.ali has no tokens', 0), ('# only a comment\n', 'u.ali has no tokens', 0)]
    for body, msg, header in cases:
        with pytest.raises(ValueError, match=msg):
            A.read_ali(_ali(f, body, *([] if header == 0 else [header])))
    f.write_text(format_ali(float('-inf'), 20, 0.05, [5], [2], [4]))                       # an utterance the aligner gave up on
    with pytest.raises(ValueError, match='u.ali has no tokens'):
        A.read_ali(str(f))
    with pytest.raises(ValueError, match='missing.ali is not a readable'):
        A.read_ali(str(tmp_path / 'missing.ali'))
    # pairing with the waveforms
    (tmp_path / 'w').mkdir()
    with pytest.raises(ValueError, match='no .ali files'):
        A.ali_pairs(str(tmp_path / 'w'), str(tmp_path / 'w'))
    _ali(f, 'AA\t1\t2\n')
    _ali(tmp_path / 'b.x.ali', 'AA\t1\t2\n')
    with pytest.raises(ValueError, match=r'b\.x\.ali has no waveform .*b\.x\.wav'):
        A.ali_pairs(str(tmp_path), str(tmp_path / 'w'))
    for w in ('b.x.wav', 'u.wav', 'other.wav'):
        (tmp_path / 'w' / w).write_bytes(b'')
    assert A.ali_pairs(str(tmp_path), str(tmp_path / 'w')) == [('b.x.ali', 'b.x', 'b.x.wav'), ('u.ali', 'u', 'u.wav')]
    # the speaker map
    m = tmp_path / 'spk.csv'
    m.write_text('key,speaker\nu,s1\n# note\n\nb.x , s2\n')
    assert A.read_spk_map(str(m)) == {'u': 's1', 'b.x': 's2'}
    m.write_text('u,s1,extra\n')
    with pytest.raises(ValueError, match='spk.csv: line 1'):
        A.read_spk_map(str(m))


def test_spans_become_rows_and_items():
    from semi_tts_amd import abx as A
    # 50 ms alignment frames onto 10 ms feature rows: exact multiples; halves round up; the end is clipped to the feature's length
    assert [A.frame_to_row(t, 0.05, 0.01, 100) for t in (0, 1, 7, 20, 21)] == [0, 5, 35, 100, 100]
    assert A.frame_to_row(1, 0.05, 0.1, 9) == 1 and A.frame_to_row(3, 0.05, 0.1, 9) == 2 and A.frame_to_row(2, 0.05, 0.1, 9) == 1
    assert A.frame_to_row(5, 0.0125, 0.05, 3) == 1 and A.frame_to_row(1, 0.0125, 0.05, 3) == 0 and A.frame_to_row(-2, 0.05, 0.05, 3) == 0
    ali = A.Ali(20, 0.05, ['sil', 'AA', 'B', 'AA', 'sil'], [2, 4, 5, 6, 19], [4, 5, 6, 12, 20])
    items, stats = A.utterance_items(ali, 0.05, 20)
    # token k runs to the next token's start (its trailing blanks are its own), the last one to `frames`; rows before the first start are nobody's
    assert items == [('sil', 2, 2, '<s>', 'AA'), ('AA', 4, 1, 'sil', 'B'), ('B', 5, 1, 'AA', 'AA'), ('AA', 6, 13, 'B', 'sil'), ('sil', 19, 1, 'AA', '</s>')]
    assert stats == {'sil': [2, 2, 0, 0], 'AA': [2, 2, 0, 0], 'B': [1, 1, 0, 0]}
    items, stats = A.utterance_items(ali, 0.05, 20, ignore=('sil',), min_frames=2)
    assert items == [('AA', 6, 13, 'B', 'sil')] and stats == {'AA': [2, 1, 1, 0], 'B': [1, 0, 1, 0]}       # sil is context, never an item
    assert A.utterance_items(ali, 0.01, 80)[0][3] == ('AA', 30, 50, 'B', 'sil')      # the features end at row 80: the span is clipped there
    items, stats = A.utterance_items(ali, 0.01, 95)                        # 5 rows a frame, features end at row 95: AA is 65 rows, sil none
    assert items == [('sil', 10, 10, '<s>', 'AA'), ('AA', 20, 5, 'sil', 'B'), ('B', 25, 5, 'AA', 'AA')]
    assert stats == {'sil': [2, 1, 1, 0], 'AA': [2, 1, 0, 1], 'B': [1, 1, 0, 0]}
    items, _ = A.utterance_items(A.Ali(20, 0.05, ['AA'], [0], [3]), 0.05 * 20 / 64, 64)
    assert items == [('AA', 0, 64, '<s>', '</s>')]                          # 64 rows are still taken
    assert A.format_phones_csv(stats) == 'phone,tokens,items,too_short,too_long\nAA,2,1,0,1\nB,1,1,0,0\nsil,2,1,1,0\n'


def test_cell_keys_for_both_contexts():
    from semi_tts_amd import abx as A
    assert A.cell_key('s1', 'sil', 'B') == ('s1', 'sil', 'B') == A.cell_key('s1', 'sil', 'B', 'triphone')
    assert A.cell_key('s1', 'sil', 'B', 'none') == ('s1',) != A.cell_key('s2', 'sil', 'B', 'none')
    assert A.cell_key('s1', A.EDGE_LEFT, 'B') != A.cell_key('s1', 'sil', 'B') and A.EDGE_LEFT != A.EDGE_RIGHT
    with pytest.raises(ValueError, match='context'):
        A.cell_key('s1', 'a', 'b', 'diphone')


# ---------------------------------------------------------------- the library
def test_exports_and_source_lists():
    from semi_tts_amd import _lib, build
    assert build.ABX_SOURCES == ['abx.hip'] and len(build.SOURCES) == 20 and 'abx.hip' not in build.SOURCES
    declared = _lib.check_header_symbols()
    assert 'st_dtw_pairs' in declared and 'st_abx_count' in declared
    assert len(_lib.SIGNATURES['st_dtw_pairs']) == 16 and len(_lib.SIGNATURES['st_abx_count']) == 6
    hdr = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    assert 'may differ in\n * path_len' in hdr or 'may differ in path_len' in hdr             # d(a, b) against d(b, a) under exact ties


def test_c_entries_refuse_each_limit_without_a_device():
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def pairs(feat=p, n_rows=8, D=4, st=4, n_items=2, P=1, metric=1, max_len=8, dist=p, a=p):
        return lib.st_dtw_pairs(feat, n_rows, D, st, p, p, n_items, a, p, P, metric, max_len, dist, None, None, None)
    for kw in (dict(P=0), dict(P=-1), dict(D=0), dict(D=513, st=513), dict(st=3), dict(max_len=0), dict(max_len=65), dict(metric=-1), dict(metric=3),
               dict(n_items=0), dict(n_rows=0), dict(feat=None), dict(dist=None), dict(a=None)):
        assert pairs(**kw) == -22, kw
        assert b'st_dtw_pairs' in lib.st_last_error()

    def count(dmat=p, n=16, blk=p, NB=1, out=p):
        return lib.st_abx_count(dmat, n, blk, NB, out, None)
    for kw in (dict(NB=0), dict(NB=-3), dict(n=0), dict(dmat=None), dict(blk=None), dict(out=None)):
        assert count(**kw) == -22, kw
        assert b'st_abx_count' in lib.st_last_error()


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import _lib, metrics, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)
    feat = torch.rand(10, 4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)             # noqa: E731
    for f in (feat, [[1.0]]):
        with pytest.raises(ValueError, match='GPU tensor'):
            ops.dtw_pairs(f, i32(0), i32(2), i32(0), i32(0))
        with pytest.raises(ValueError, match='GPU tensor'):
            metrics.dtw_pairs(f, [0], [2], [0], [0])
        with pytest.raises(ValueError, match='GPU tensor'):
            metrics.abx(f, [0], [2], [0], [0])
        with pytest.raises(ValueError, match='GPU tensor'):
            ops.abx_count(f, torch.zeros(1, 6, dtype=torch.int64))
    # a meta tensor stands in for a device tensor: the checks read .is_cuda / .device / .shape / .dtype / .stride() only
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    mf = feat.to('meta')
    s, ln, a, b = (i32(0, 3).to('meta'), i32(3, 4).to('meta'), i32(0, 1, 0).to('meta'), i32(1, 0, 0).to('meta'))
    cases = [
        (dict(feat=mf.double()), 'float32'), (dict(feat=mf[0]), 'feat must be'), (dict(feat=mf[:0]), 'n_rows >= 1'), (dict(feat=mf[:, :0]), 'D <= 512'),
        (dict(feat=torch.empty(3, 513, device='meta')), 'D <= 512'), (dict(feat=mf.t()), 'strides'), (dict(feat=mf[:, :1].expand(10, 4)), 'strides'),
        (dict(feat=mf[:1].expand(10, 4)), 'strides'), (dict(metric='cosine'), 'metric'), (dict(metric=3), 'metric'), (dict(metric=1.0), 'metric'),
        (dict(metric=True), 'metric'), (dict(max_len=0), 'max_len'), (dict(max_len=65), 'max_len'), (dict(max_len=2.0), 'max_len'),
        (dict(item_start=s.long()), 'item_start'), (dict(item_start=i32(0, 3)), 'item_start'), (dict(item_len=ln[:1]), 'as many of each'),
        (dict(item_start=s[:0], item_len=ln[:0]), 'at least one item'), (dict(item_len=ln.float()), 'item_len'), (dict(pair_a=a[:0], pair_b=b[:0]), 'at least one pair'),
        (dict(pair_b=b[:2]), 'as many of each'), (dict(pair_a=a.view(3, 1)), 'pair_a'), (dict(pair_b=[1, 0, 0]), 'pair_b'), (dict(pair_a=a.long()), 'pair_a'),
        (dict(item_len=torch.empty(4, dtype=torch.int32, device='meta')[::2]), 'item_len'),
    ]
    base = dict(feat=mf, item_start=s, item_len=ln, pair_a=a, pair_b=b)
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.dtw_pairs(**dict(base, **kw))
    for kw in (dict(), dict(metric='kl', want_cost=True), dict(metric=0, max_len=1), dict(feat=torch.empty(10, 9, device='meta')[:, 2:6])):
        with pytest.raises(AssertionError, match='reached the device'):
            ops.dtw_pairs(**dict(base, **kw))
    with pytest.raises(ValueError, match='int32 integers'):
        metrics.dtw_pairs(mf, [0.5], [2], [0], [0])
    with pytest.raises(ValueError, match='max_len'):
        metrics.dtw_pairs(mf, s, ln, a, b, max_len=70)
    dm, blk = torch.zeros(9).to('meta'), torch.zeros(2, 6, dtype=torch.int64).to('meta')
    for kw, msg in [(dict(dmat=dm.double()), 'dmat must be'), (dict(dmat=dm.view(3, 3)), 'dmat must be'), (dict(dmat=dm[::2]), 'dmat must be'),
                    (dict(dmat=dm[:0]), 'at least one distance'), (dict(blk=blk.int()), 'blk must be'), (dict(blk=blk[:, :5]), 'blk'),
                    (dict(blk=blk[:0]), 'NB >= 1'), (dict(blk=blk[0]), 'blk must be'), (dict(blk=torch.zeros(2, 6, dtype=torch.int64)), 'blk must be')]:
        with pytest.raises(ValueError, match=msg):
            ops.abx_count(**dict(dict(dmat=dm, blk=blk), **kw))
    with pytest.raises(AssertionError, match='reached the device'):
        ops.abx_count(dm, blk)
    with pytest.raises(ValueError, match='one of each'):
        metrics.abx(mf, [0, 3], [3], [0, 1], [0, 0])


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']
_ABX = ['--abx-ali-dir', 'ali', '--abx-wav-dir', 'wav']


def test_abx_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + _ABX)
    assert (p.abx_ali_dir, p.abx_wav_dir, p.abx_feat, p.abx_metric, p.abx_context, p.abx_ignore, p.abx_max_items, p.abx_min_frames, p.abx_spk_map) == \
        ('ali', 'wav', 'mfcc', 'angular', 'triphone', (), 50, 1, None)
    p = entry.parse_args(CFG + _ABX + ['--abx-feat', 'code', '--abx-context', 'none', '--abx-ignore', 'sil, sp,', '--abx-max-items', '7', '--abx-min-frames',
                                       '2', '--abx-spk-map', 'm.csv', '--seed', '3', '--batch-size', '4', '--resample', '--trim-silence', '--normalize-loudness'])
    assert (p.abx_feat, p.abx_metric, p.abx_context, p.abx_ignore, p.abx_max_items, p.abx_min_frames, p.abx_spk_map, p.seed, p.batch_size) == \
        ('code', 'kl', 'none', ('sil', 'sp'), 7, 2, 'm.csv', 3, 4)
    assert entry.parse_args(CFG + _ABX + ['--abx-feat', 'code', '--abx-metric', 'euclid']).abx_metric == 'euclid'
    assert entry.parse_args(CFG + _ABX + ['--abx-feat', 'latent']).abx_metric == 'angular'
    p = entry.parse_args(CFG)
    assert p.abx_ali_dir is None and p.abx_feat is None and p.abx_metric is None


_NO_COMBINE = '--abx-ali-dir does not combine with --'
_NEEDS = 'belong to --abx-ali-dir; they need that flag'


@pytest.mark.parametrize('argv,msg', [
    (CFG + _ABX + ['--gen-specgram'], _NO_COMBINE + 'gen-specgram'),
    (CFG + _ABX + ['--tts-only'], _NO_COMBINE + 'tts-only'),
    (CFG + _ABX + ['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
    (CFG + _ABX + ['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
    (CFG + _ABX + ['--transcribe-wav-dir', 't'], _NO_COMBINE + 'transcribe-wav-dir'),
    (CFG + _ABX + ['--align-wav-dir', 'a'], _NO_COMBINE + 'align-wav-dir'),
    (CFG + _ABX + ['--vocode-dir', 'v'], _NO_COMBINE + 'vocode-dir'),
    (CFG + _ABX + ['--resample-wav-dir', 'r', '--resample-out', 'o'], _NO_COMBINE + 'resample-wav-dir'),
    (CFG + _ABX + ['--feat-wav-dir', 'f', '--feat', 'mfcc'], _NO_COMBINE + 'feat-wav-dir'),
    (CFG + _ABX + ['--mcd-wav-dir', 's', '--mcd-ref-dir', 'r'], _NO_COMBINE + 'mcd-wav-dir'),
    (CFG + _ABX + ['--synth-phn-dir', 's'], _NO_COMBINE + 'synth-phn-dir'),
    (CFG + _ABX + ['--trim-wav-dir', 't', '--trim-out', 'o'], _NO_COMBINE + 'trim-wav-dir'),
    (CFG + _ABX + ['--loudness-wav-dir', 'l'], _NO_COMBINE + 'loudness-wav-dir'),
    (CFG + _ABX + ['--build-lm-phn-dir', 'p', '--lm', 'x.npy', '--lm-order', '2'], _NO_COMBINE + 'build-lm-phn-dir'),
    (CFG + _ABX + ['--score-phn-dir', 'h', '--score-ref-dir', 'r'], 'does not combine with --'),
    (CFG + _ABX + ['--corpus'], 'does not combine with --'),
    (CFG + ['--abx-ali-dir', 'ali'], '--abx-ali-dir needs --config (its data.audio and model) and --abx-wav-dir DIR'),
    (_ABX, '--abx-ali-dir needs --config (its data.audio and model) and --abx-wav-dir DIR'),
    (CFG + ['--abx-wav-dir', 'wav'], _NEEDS),
    (CFG + ['--abx-feat', 'mel'], _NEEDS),
    (CFG + ['--abx-metric', 'kl'], _NEEDS),
    (CFG + ['--abx-context', 'none'], _NEEDS),
    (CFG + ['--abx-spk-map', 'm.csv'], _NEEDS),
    (CFG + ['--abx-ignore', 'sil'], _NEEDS),
    (CFG + ['--abx-max-items', '5'], _NEEDS),
    (CFG + ['--mcd-wav-dir', 's', '--mcd-ref-dir', 'r', '--abx-min-frames', '2'], _NEEDS),
    (CFG + _ABX + ['--abx-max-items', '1'], '--abx-max-items must be >= 2 and --abx-min-frames in [1, 64]'),
    (CFG + _ABX + ['--abx-min-frames', '0'], '--abx-max-items must be >= 2 and --abx-min-frames in [1, 64]'),
    (CFG + _ABX + ['--abx-min-frames', '65'], '--abx-max-items must be >= 2 and --abx-min-frames in [1, 64]'),
    (CFG + _ABX + ['--abx-feat', 'post'], 'invalid choice'),
    (CFG + _ABX + ['--abx-metric', 'cosine'], 'invalid choice'),
])
def test_abx_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


def test_scorer_names_the_file_before_any_device_work(tmp_path, monkeypatch):
    """AbxScorer.load_data: a missing waveform, a malformed .ali, an .ali without tokens, a file the speaker map lacks, an unreadable
    waveform and a foreign sample rate are ValueErrors naming the file (no GPU needed)"""
    import yaml
    from semi_tts_amd import audio, solver
    from semi_tts_amd.audio import write_wav
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    config = yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
    sr = config['data']['audio']['sample_rate']
    ali, wav = tmp_path / 'ali', tmp_path / 'wav'
    ali.mkdir()
    wav.mkdir()
    rs = np.random.RandomState(0)

    class P:
        abx_ali_dir, abx_wav_dir, name, logdir, batch_size, abx_spk_map, resample = str(ali), str(wav), 'abx', str(tmp_path / 'log'), 4, None, False
    sc = solver.AbxScorer(config, P(), 'test')
    assert (sc.feat, sc.metric, sc.context, sc.max_items, sc.min_frames) == ('mfcc', 'angular', 'triphone', 50, 1)
    with pytest.raises(ValueError, match='no .ali files'):
        sc.load_data()
    _ali(ali / 'a.ali', 'AA\t1\t2\n')
    _ali(ali / 'b.ali', 'AA\t1\t2\nB\t2\n')
    with pytest.raises(ValueError, match=r'a\.ali has no waveform .*a\.wav'):
        sc.load_data()
    write_wav(str(wav / 'a.wav'), 0.1 * rs.randn(sr // 2), sr)
    (wav / 'b.wav').write_bytes(b'not a wav file')
    with pytest.raises(ValueError, match=r'b\.ali: malformed line'):
        sc.load_data()
    _ali(ali / 'b.ali', '')
    with pytest.raises(ValueError, match=r'b\.ali has no tokens'):
        sc.load_data()
    _ali(ali / 'b.ali', 'B\t0\t20\n')
    with pytest.raises(ValueError, match=r'b\.wav is not a readable'):
        sc.load_data()
    write_wav(str(wav / 'b.wav'), 0.1 * rs.randn(sr // 2), sr // 2)
    with pytest.raises(ValueError, match=r'Expected %d but get %d .*b\.wav' % (sr, sr // 2)):
        sc.load_data()
    P.resample = True
    assert solver.AbxScorer(config, P(), 'test').load_data().speakers == ['spk', 'spk']
    P.resample = False
    write_wav(str(wav / 'b.wav'), 0.1 * rs.randn(sr // 2), sr)
    (tmp_path / 'spk.csv').write_text('a,s1\n')
    P.abx_spk_map = str(tmp_path / 'spk.csv')
    with pytest.raises(ValueError, match=r'spk\.csv has no row for b\.ali'):
        solver.AbxScorer(config, P(), 'test').load_data()
    (tmp_path / 'spk.csv').write_text('a,s1\nb,s2\n')
    sc = solver.AbxScorer(config, P(), 'test').load_data()
    assert sc.speakers == ['s1', 's2'] and [p[1] for p in sc.pairs] == ['a', 'b'] and sc.set_model().model is None
    assert abs(sc.frame_s() - (sr // 100) / sr) < 1e-12
    assert not os.path.exists(P.logdir)                                     # nothing is written before exec
    P.abx_feat = 'code'
    assert solver.abx_metric(P) == 'kl' and solver.AbxScorer(config, P(), 'test').metric == 'kl'
