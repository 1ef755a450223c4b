"""CPU checks of across-speaker ABX: a hand-computed example through counts, group errors, table and score, the layout plan_across
makes (cross-speaker pairs only, contiguous ranges, the own-speaker range inside xr, plan's keep, no matrix without a group),
aggregate_across against the oracle on random counts, every ValueError of metrics.abx_across / ops.abx_across and every -22 of
st_abx_across before a device is touched, the exported symbol, and the parser rules of --abx-mode and --abx-max-gb."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import abx_across_oracle as X  # noqa: E402

NAN = float('nan')
# item id -> (context, speaker, label); labels a = 0, b = 1, c = 2.  Context 0 in plan order: s0 a, s0 b, s1 a, s1 b, s2 b, s2 c (speaker 2
# lacks a) = ids 1, 4, 6, 0, 7, 3; context 1: s0 a, s0 c, s1 a = ids 8, 2, 5
ITEMS = [(0, 1, 1), (0, 0, 0), (1, 0, 2), (0, 2, 2), (0, 0, 1), (1, 1, 0), (0, 1, 0), (0, 2, 1), (1, 0, 0)]
DIST = {(1, 6): 1, (1, 0): 2, (4, 6): 3, (4, 0): 1, (1, 7): 2, (1, 3): 4, (4, 7): 2, (4, 3): NAN, (6, 7): 5, (6, 3): 1, (0, 7): 1, (0, 3): 1,
        (8, 5): 3, (2, 5): 2}
# by hand, (context, speaker, a, b): (wrong, tied, nan, triples, x_speakers), error
#   c0 s0 a b: X = s1's a: d(A, X) = 1 < d(B, X) = 3                                                   -> 0
#   c0 s0 b a: X = s1's b: 1 < 2; X = s2's b: 2 == 2, a tie                                             -> (0 + 1/2) / 2
#   c0 s1 a b: X = s0's a: 1 < 2                                                                       -> 0
#   c0 s1 b a: X = s0's b: 1 < 3; X = s2's b: 1 < 5                                                     -> 0
#   c0 s2 b c: X = s0's b: d(B, X) is NaN, that pair score is absent; X = s1's b: 1 == 1, a tie         -> 1/2 over ONE speaker
#   c1 s0 a c: X = s1's a: 3 > 2, wrong                                                                -> 1
HAND = {(0, 0, 0, 1): ((0, 0, 0, 1, 1), 0.0), (0, 0, 1, 0): ((0, 1, 0, 2, 2), 0.25), (0, 1, 0, 1): ((0, 0, 0, 1, 1), 0.0),
        (0, 1, 1, 0): ((0, 0, 0, 2, 2), 0.0), (0, 2, 1, 2): ((0, 1, 1, 2, 1), 0.5), (1, 0, 0, 2): ((1, 0, 0, 1, 1), 1.0)}
HAND_TABLE = [(0, 1, 2, 2, 0.0), (0, 2, 1, 1, 1.0), (1, 0, 2, 4, 0.125), (1, 2, 1, 1, 0.5)]
HAND_SCORE = (0.0 + 1.0 + 0.125 + 0.5) / 4
HAND_SPEAKERS = [(0, 3, 1.25 / 3), (1, 2, 0.0), (2, 1, 0.5)]


def _dist(p, q):
    return float(DIST[(p, q)] if (p, q) in DIST else DIST[(q, p)])


def _columns():
    return tuple(np.array([it[k] for it in ITEMS]) for k in (2, 0, 1))          # label, context, speaker


def _evaluate(pl, dist):
    """the plan's groups through the oracle's brute force -> (err (NG,), count (NG, 5)): what st_abx_across returns"""
    dmat = np.full(pl.dmat_len, np.nan)
    for a, b, p, q in zip(pl.pair_a, pl.pair_b, pl.pos_ab, pl.pos_ba):
        dmat[p] = dmat[q] = dist(int(a), int(b))
    err, cnt = [], []
    for off, nc, a_lo, a_hi, b_lo, b_hi, x0, x1 in pl.grp:
        e, c = X.group(dmat[off:off + nc * nc].reshape(nc, nc), (a_lo, a_hi), (b_lo, b_hi), [tuple(r) for r in pl.xr[x0:x1]])
        err.append(e)
        cnt.append(c)
    return np.array(err), np.array(cnt, np.int64).reshape(-1, 5)


def test_hand_computed_example_through_counts_errors_table_and_score():
    from semi_tts_amd import abx as A
    label, context, speaker = _columns()
    pl = A.plan_across(label, context, speaker)
    keys = list(zip(pl.grp_context.tolist(), pl.grp_speaker.tolist(), pl.grp_a.tolist(), pl.grp_b.tolist()))
    assert keys == sorted(HAND)
    err, cnt = _evaluate(pl, _dist)
    for k, e, c in zip(keys, err, cnt):
        assert tuple(c) == HAND[k][0] and e == HAND[k][1], k
    agg = A.aggregate_across(pl.grp_a, pl.grp_b, pl.grp_speaker, err, cnt)
    assert agg.table == HAND_TABLE and agg.score == HAND_SCORE and agg.speakers == HAND_SPEAKERS
    # the oracle's own walk over the items agrees with the hand
    groups, table, score, speakers = X.abx_across(_dist, label, context, speaker)
    assert {k: (v[1], v[0]) for k, v in groups.items()} == HAND
    assert [(a, b) + table[(a, b)] for a, b in sorted(table)] == HAND_TABLE and score == HAND_SCORE
    assert [(s,) + speakers[s] for s in sorted(speakers)] == HAND_SPEAKERS
    assert A.format_abx_across_csv(agg.table, 'abc') == ('phone_a,phone_b,groups,triples,error\na,b,2,2,0.000000\na,c,1,1,1.000000\n'
                                                         'b,a,2,4,0.125000\nb,c,1,1,0.500000\n')
    assert A.format_abx_across_speakers_csv(agg.speakers, ['s0', 's1', 's2']) == 'speaker,groups,error\ns0,3,0.416667\ns1,2,0.000000\ns2,1,0.500000\n'


def test_plan_across_layout():
    from semi_tts_amd import abx as A
    label, context, speaker = _columns()
    pl = A.plan_across(label, context, speaker)
    assert pl.keep.tolist() == [1, 4, 6, 0, 7, 3, 8, 2, 5] and pl.dmat_len == 36 + 9
    # exactly the cross-speaker pairs, each once, first item first in context order
    got = list(zip(pl.pair_a.tolist(), pl.pair_b.tolist()))
    assert len(got) == len(set(got)) == len(DIST) and {tuple(sorted(p)) for p in got} == {tuple(sorted(p)) for p in DIST}
    order = {q: i for i, q in enumerate(pl.keep.tolist())}
    assert all(order[a] < order[b] and ITEMS[a][0] == ITEMS[b][0] and ITEMS[a][1] != ITEMS[b][1] for a, b in got)
    assert pl.pair_a.dtype == pl.pair_b.dtype == np.int32 and pl.grp.dtype == pl.xr.dtype == np.int64 and pl.grp.shape == (6, 8) and pl.xr.shape[1] == 2
    # mirrored positions of one matrix entry
    for p, q, g in zip(pl.pos_ab, pl.pos_ba, got):
        off, nc = (0, 6) if p < 36 else (36, 3)
        i, j = divmod(int(p) - off, nc)
        assert int(q) == off + j * nc + i and i < j and pl.keep[(0 if off == 0 else 6) + i] == g[0] and pl.keep[(0 if off == 0 else 6) + j] == g[1]
    # ranges are contiguous runs of one (speaker, label); the own range is an entry of the group's xr slice, in ascending speaker order
    ks, kl = speaker[pl.keep], label[pl.keep]
    for row, c, s, a, b in zip(pl.grp, pl.grp_context, pl.grp_speaker, pl.grp_a, pl.grp_b):
        off, nc, a_lo, a_hi, b_lo, b_hi, x0, x1 = row.tolist()
        base = 0 if off == 0 else 6
        assert (ks[base + a_lo:base + a_hi] == s).all() and (kl[base + a_lo:base + a_hi] == a).all() and a_hi > a_lo
        assert (ks[base + b_lo:base + b_hi] == s).all() and (kl[base + b_lo:base + b_hi] == b).all() and b_hi > b_lo
        xs = [tuple(r) for r in pl.xr[x0:x1].tolist()]
        assert xs.count((a_lo, a_hi)) == 1 and len(xs) >= 2
        assert all((kl[base + lo:base + hi] == a).all() and len(set(ks[base + lo:base + hi].tolist())) == 1 for lo, hi in xs)
        assert [int(ks[base + lo]) for lo, _ in xs] == sorted(int(ks[base + lo]) for lo, _ in xs)
    # a context without a group gets no matrix and no pair: context 2 has two speakers without a common label, context 3 one speaker
    label2 = np.concatenate([label, [0, 1, 0, 1]])
    context2 = np.concatenate([context, [2, 2, 3, 3]])
    speaker2 = np.concatenate([speaker, [0, 1, 0, 0]])
    more = A.plan_across(label2, context2, speaker2)
    assert more.dmat_len == pl.dmat_len and np.array_equal(more.grp, pl.grp) and np.array_equal(more.pair_a, pl.pair_a) and len(more.keep) == 13
    none = A.plan_across([0, 1], [0, 0], [0, 0])
    assert none.dmat_len == 0 and none.grp.shape == (0, 8) and none.xr.shape == (0, 2) and len(none.pair_a) == 0
    assert A.plan_across([], [], []).grp.shape == (0, 8)
    with pytest.raises(ValueError, match='one of each per item'):
        A.plan_across([0, 1], [0], [0, 0])


def test_plan_across_keeps_what_plan_keeps():
    from semi_tts_amd import abx as A
    rs = np.random.RandomState(5)
    n = 400
    label, context, speaker = rs.randint(0, 4, n), rs.randint(0, 3, n), rs.randint(0, 5, n)
    cell = np.unique(np.stack([context, speaker], 1), axis=0, return_inverse=True)[1].reshape(-1)
    for max_items, seed in ((3, 0), (3, 7), (50, 0)):
        pl = A.plan_across(label, context, speaker, max_items, seed)
        assert np.array_equal(pl.keep, A.plan(label, cell, max_items, seed).keep)
        assert max_items == 50 or len(pl.keep) < n
        key = list(zip(context[pl.keep].tolist(), speaker[pl.keep].tolist(), label[pl.keep].tolist(), pl.keep.tolist()))
        assert key == sorted(key)
    # the byte rule: 4 bytes a matrix entry, 28 a pair, refused before anything is laid out
    pl = A.plan_across(label, context, speaker)
    need = 4 * pl.dmat_len + 28 * len(pl.pair_a)
    assert A.plan_across(label, context, speaker, max_bytes=need).dmat_len == pl.dmat_len
    with pytest.raises(ValueError, match=r'lower --abx-max-items or use --abx-context triphone'):
        A.plan_across(label, context, speaker, max_bytes=need - 1)


def test_aggregate_across_against_the_oracle_on_random_counts():
    from semi_tts_amd import abx as A
    rs = np.random.RandomState(9)
    keys = sorted({(int(c), int(s), int(a), int(b)) for c, s, a, b in rs.randint(0, 6, (900, 4)) if a != b})
    groups = {}
    for k in keys:
        tri = int(rs.randint(0, 50))
        nan = int(rs.randint(0, tri + 1)) if rs.rand() < 0.3 else 0
        wrong = int(rs.randint(0, tri - nan + 1))
        tied = int(rs.randint(0, tri - nan - wrong + 1))
        present = int(rs.randint(1, 4)) if tri - nan > 0 else 0
        groups[k] = ((wrong + 0.5 * tied) / (tri - nan) / rs.randint(1, 3) if present else NAN, (wrong, tied, nan, tri, present))
    assert sum(1 for v in groups.values() if v[0] != v[0]) > 5
    table, score, speakers = X.aggregate(groups)
    agg = A.aggregate_across([k[2] for k in keys], [k[3] for k in keys], [k[1] for k in keys], [groups[k][0] for k in keys],
                             [groups[k][1] for k in keys])
    assert [(a, b, g, t) for a, b, g, t, _ in agg.table] == [(a, b) + table[(a, b)][:2] for a, b in sorted(table)] and len(agg.table) == 30
    assert [e for *_, e in agg.table] == [table[k][2] for k in sorted(table)]              # the same sequential sums: bit for bit
    assert abs(agg.score - score) <= 1e-12
    assert agg.speakers == [(s,) + speakers[s] for s in sorted(speakers)]
    empty = A.aggregate_across([0], [1], [0], [NAN], [(0, 0, 0, 0, 0)])
    assert empty.table == [] and math.isnan(empty.score) and empty.speakers == []
    with pytest.raises(ValueError, match='one of each per group'):
        A.aggregate_across([0, 1], [1], [0], [0.5], [(0, 0, 0, 1, 1)])


# ---------------------------------------------------------------- the library
def test_symbol_is_declared_bound_and_built():
    from semi_tts_amd import _lib, build
    assert 'st_abx_across' in _lib.check_header_symbols() and len(_lib.SIGNATURES['st_abx_across']) == 9
    assert build.ABX_SOURCES == ['abx.hip'] and 'st_abx_across' in open(os.path.join(build.CSRC, 'abx.hip')).read()
    hdr = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    assert 'int st_abx_across(const float* dmat, long dmat_len, const int64_t* grp /* (NG, 8) */, int NG' in hdr


def test_c_entry_refuses_each_limit_without_a_device():
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def across(dmat=p, n=16, grp=p, NG=1, xr=p, NX=1, err=p, count=p):
        return lib.st_abx_across(dmat, n, grp, NG, xr, NX, err, count, None)
    for kw in (dict(NG=0), dict(NG=-2), dict(n=0), dict(n=-1), dict(NX=0), dict(NX=-5), dict(dmat=None), dict(grp=None), dict(xr=None), dict(err=None),
               dict(count=None)):
        assert across(**kw) == -22, kw
        assert b'st_abx_across' in lib.st_last_error()


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import _lib, metrics, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)
    feat = torch.rand(10, 4)
    for f in (feat, [[1.0]]):
        with pytest.raises(ValueError, match='GPU tensor'):
            metrics.abx_across(f, [0], [2], [0], [0], [0])
        with pytest.raises(ValueError, match='GPU tensor'):
            ops.abx_across(f, torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64))
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    mf = feat.to('meta')
    dm, grp, xr = torch.zeros(9).to('meta'), torch.zeros(2, 8, dtype=torch.int64).to('meta'), torch.zeros(3, 2, dtype=torch.int64).to('meta')
    for kw, msg in [(dict(dmat=dm.double()), 'dmat must be'), (dict(dmat=dm.view(3, 3)), 'dmat must be'), (dict(dmat=dm[::2]), 'dmat must be'),
                    (dict(dmat=dm[:0]), 'at least one distance'), (dict(grp=grp.int()), 'grp must be'), (dict(grp=torch.zeros(2, 6, dtype=torch.int64).to('meta')), r'\(NG, 8\)'),
                    (dict(grp=grp[:0]), 'NG >= 1'), (dict(grp=grp[0]), 'grp must be'), (dict(grp=torch.zeros(2, 8, dtype=torch.int64)), 'grp must be'),
                    (dict(xr=xr.int()), 'xr must be'), (dict(xr=torch.zeros(3, 1, dtype=torch.int64).to('meta')), r'\(NX, 2\)'), (dict(xr=xr[:0]), 'NX >= 1'), (dict(xr=xr[0]), 'xr must be'),
                    (dict(xr=torch.zeros(3, 2, dtype=torch.int64)), 'xr must be')]:
        with pytest.raises(ValueError, match=msg):
            ops.abx_across(**dict(dict(dmat=dm, grp=grp, xr=xr), **kw))
    with pytest.raises(AssertionError, match='reached the device'):
        ops.abx_across(dm, grp, xr)
    # metrics.abx_across: table lengths, speakers, bytes
    label, context, speaker = _columns()
    start, length = np.arange(9) , np.ones(9, np.int64)
    for k in range(5):
        cols = [start, length, label, context, speaker]
        cols[k] = cols[k][:-1]
        with pytest.raises(ValueError, match='one of each per item'):
            metrics.abx_across(mf, *cols)
    with pytest.raises(ValueError, match='fewer than two speakers'):
        metrics.abx_across(mf, start, length, label, context, np.zeros(9, int))
    with pytest.raises(ValueError, match=r'more than 435 bytes \(480 bytes.*lower --abx-max-items or use --abx-context triphone'):
        metrics.abx_across(mf, start, length, label, context, speaker, max_bytes=435)
    with pytest.raises(ValueError, match='max_items'):
        metrics.abx_across(mf, start, length, label, context, speaker, max_items=0)
    with pytest.raises(ValueError, match='metric'):
        metrics.abx_across(mf, start, length, label, context, speaker, metric='cosine')
    with pytest.raises(AssertionError, match='reached the device'):
        metrics.abx_across(mf, start, length, label, context, speaker, 'euclid', max_bytes=4 * 45 + 28 * 14)
    # without a group nothing is launched
    res = metrics.abx_across(mf, [0, 1], [1, 1], [0, 1], [0, 0], [0, 1])
    assert res.table == [] and math.isnan(res.score) and res.speakers == [] and res.pairs == 0 and res.counts.shape == (0, 5) and res.keep.tolist() == [0, 1]


# ---------------------------------------------------------------- main.py flags
def _entry():
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']
_ABX = ['--abx-ali-dir', 'ali', '--abx-wav-dir', 'wav']


def test_abx_mode_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + _ABX)
    assert (p.abx_mode, p.abx_max_gb) == ('within', 8.0)
    p = entry.parse_args(CFG + _ABX + ['--abx-mode', 'within', '--abx-spk-map', 'm.csv'])
    assert (p.abx_mode, p.abx_max_gb, p.abx_spk_map) == ('within', 8.0, 'm.csv')
    p = entry.parse_args(CFG + _ABX + ['--abx-mode', 'across', '--abx-spk-map', 'm.csv'])
    assert (p.abx_mode, p.abx_max_gb) == ('across', 8.0)
    p = entry.parse_args(CFG + _ABX + ['--abx-mode', 'both', '--abx-spk-map', 'm.csv', '--abx-max-gb', '0.5', '--abx-context', 'none'])
    assert (p.abx_mode, p.abx_max_gb, p.abx_context) == ('both', 0.5, 'none')
    p = entry.parse_args(CFG)
    assert p.abx_mode is None and p.abx_max_gb is None


@pytest.mark.parametrize('argv,msg', [
    (CFG + _ABX + ['--abx-mode', 'across'], '--abx-mode across takes X from another speaker: it needs --abx-spk-map'),
    (CFG + _ABX + ['--abx-mode', 'both'], '--abx-mode both takes X from another speaker: it needs --abx-spk-map'),
    (CFG + _ABX + ['--abx-mode', 'between'], 'invalid choice'),
    (CFG + _ABX + ['--abx-max-gb', '2'], '--abx-max-gb takes a positive number of GiB and belongs to --abx-mode across or both'),
    (CFG + _ABX + ['--abx-mode', 'within', '--abx-max-gb', '2'], '--abx-max-gb takes a positive number of GiB and belongs to --abx-mode across or both'),
    (CFG + _ABX + ['--abx-mode', 'across', '--abx-spk-map', 'm.csv', '--abx-max-gb', '0'], '--abx-max-gb takes a positive number'),
    (CFG + _ABX + ['--abx-mode', 'across', '--abx-spk-map', 'm.csv', '--abx-max-gb', '-1'], '--abx-max-gb takes a positive number'),
    (CFG + _ABX + ['--abx-mode', 'across', '--abx-spk-map', 'm.csv', '--abx-max-gb', 'nan'], '--abx-max-gb takes a positive number'),
    (CFG + ['--abx-mode', 'across'], '--abx-mode and --abx-max-gb belong to --abx-ali-dir; they need that flag'),
    (CFG + ['--abx-max-gb', '4'], '--abx-mode and --abx-max-gb belong to --abx-ali-dir; they need that flag'),
])
def test_abx_mode_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


def test_scorer_refuses_fewer_than_two_speakers_before_any_device_work(tmp_path, monkeypatch):
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
    for stem in 'ab':
        (ali / (stem + '.ali')).write_text('# score=-1.0 frames=12 frame_s=0.05\nAA\t1\t5\nB\t5\t9\n')
        write_wav(str(wav / (stem + '.wav')), 0.1 * rs.randn(sr // 2), sr)

    class P:
        abx_ali_dir, abx_wav_dir, name, logdir, batch_size, abx_spk_map, resample, abx_mode = str(ali), str(wav), 'abx', str(tmp_path / 'log'), 4, None, False, 'across'
    with pytest.raises(ValueError, match=r'--abx-mode across needs --abx-spk-map FILE with at least two speakers among the files \(got no map\)'):
        solver.AbxScorer(config, P(), 'test').load_data()
    (tmp_path / 'one.csv').write_text('a,s1\nb,s1\n')
    P.abx_spk_map, P.abx_mode = str(tmp_path / 'one.csv'), 'both'
    with pytest.raises(ValueError, match=r'--abx-mode both needs --abx-spk-map FILE with at least two speakers among the files \(got 1 speaker\)'):
        solver.AbxScorer(config, P(), 'test').load_data()
    (tmp_path / 'two.csv').write_text('a,s1\nb,s2\n')
    P.abx_spk_map = str(tmp_path / 'two.csv')
    sc = solver.AbxScorer(config, P(), 'test').load_data()
    assert sc.speakers == ['s1', 's2'] and sc.abx_mode == 'both' and sc.max_bytes == 8 << 30
    P.abx_spk_map, P.abx_mode = str(tmp_path / 'one.csv'), 'within'
    assert solver.AbxScorer(config, P(), 'test').load_data().speakers == ['s1', 's1']
