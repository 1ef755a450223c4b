"""st_abx_across on the device against the brute force of tests/abx_across_oracle.py (counts exact, err bit for bit), metrics.abx_across
against the oracle's walk over the items, and --abx-mode across / both end to end.

What varies inside the kernel is the width W of the lanes a range gets -- the power of two that holds the widest n_x n_a of the group's
list: 1, 2, ..., 32, and 64 (strided over past 64 pairs) --, hence the ranges of one pass (64 / W) and the passes of a list; the sizes
below reach W = 1 with 65 ranges (two passes of 64), W = 16 with up to 66 ranges (17 passes), W = 32, W = 64 unstrided and strided."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import abx_across_oracle as X  # noqa: E402
import abx_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _matrices():
    """four matrices of small integers (ties abound), NOT symmetric: d(., X) must come from row X.  -> (list, offsets, dmat_len)"""
    rs = np.random.RandomState(3)
    mats = []
    for nc, p_nan in ((6, 0.0), (210, 0.02), (50, 0.0), (8, 1.0)):
        d = rs.randint(0, 4, (nc, nc)).astype(np.float32)
        d[rs.rand(nc, nc) < p_nan] = np.nan
        mats.append(d)
    mats[2][27, 30] = np.nan                      # d(B, X) of B = 30, X = 27: every A of the 20 x 20 group, 20 triples
    mats[2][44, 1] = np.nan                       # d(A, X) of A = 1, X = 44: one triple of the last fixed case
    mats[1][12:15, :] = np.nan                    # a whole X range of matrix 1: the rows of range 4 = [12, 15)
    offs = np.concatenate([[0], np.cumsum([m.size for m in mats])]).astype(np.int64)
    return mats, offs[:-1], int(offs[-1])


R1 = [(3 * k, 3 * k + 1 + k % 3) for k in range(66)]      # matrix 1: 66 ranges of 1..3 items
S1 = [(k, k + 1) for k in range(70)]                        # matrix 1: 70 ranges of one item


def _cases():
    """(matrix, a range, b range, the X ranges of its list) of every shape the kernel treats differently"""
    cases = [
        (0, (0, 1), (1, 2), [(0, 1), (3, 4)]),                              # a single triple: n_a = n_b = n_x = 1
        (0, (0, 2), (2, 3), [(0, 2)]),                                      # the only X range is its own: no pair score
        (0, (0, 2), (2, 2), [(0, 2), (3, 5)]),                              # an empty B range
        (0, (0, 2), (3, 2), [(0, 2), (3, 5)]),                              # an inverted B range
        (0, (0, 2), (2, 3), [(0, 2), (5, 3), (4, 4)]),                      # inverted and empty X ranges beside the own
        (0, (1, 3), (3, 4), [(-3, 1), (1, 3), (4, 11)]),                    # X ranges that partly leave [0, n_c]
        (0, (-5, 2), (4, 9), [(0, 2), (2, 4)]),                             # a and b clamped; the own range is met after clamping
        (2, (0, 20), (28, 31), [(0, 20), (20, 40)]),                        # 20 x 20 (X, A) pairs: more than a wave's lanes; one NaN triple
        (2, (0, 5), (40, 42), [(0, 5), (5, 10), (10, 15)]),                 # 25 pairs a range: W = 32
        (2, (0, 6), (40, 43), [(0, 6), (6, 14), (14, 15)]),                 # 48 pairs: W = 64, one sweep
        (2, (0, 2), (40, 41), [(2, 3), (0, 2), (3, 30)]),                   # widths 1 and 27 in one list
        (3, (0, 2), (2, 4), [(0, 2), (4, 6), (6, 8)]),                      # NaN everywhere: every pair score absent
        (1, (198, 200), (204, 207), [(12, 15), (198, 200), (30, 32)]),      # a whole X range of NaN, one clean
        (2, (0, 2), (40, 41), [(0, 2), (44, 46)]),                          # a NaN in one triple
    ]
    for n in (1, 2, 63, 64, 65):
        cases.append((1, R1[0], (200, 203), R1[:n + 1]))                    # n foreign ranges after the own
        cases.append((1, R1[n // 2], (203, 204), R1[:n]))                   # n ranges, the own in the middle
        cases.append((1, (205, 206), (200, 202), R1[:n]))                   # n ranges, none its own
        cases.append((1, S1[n - 1], (100, 101), S1[:n]))                    # one item a range: W = 1, 64 ranges a pass
    return cases


def _assemble(cases, offs, mats):
    """-> (grp (NG, 8), xr (NX, 2)): every case with an xr slice of its own, the slices laid end to end"""
    grp, xr = [], []
    for m, a, b, xs in cases:
        grp.append((offs[m], len(mats[m]), a[0], a[1], b[0], b[1], len(xr), len(xr) + len(xs)))
        xr += xs
    return np.asarray(grp, np.int64), np.asarray(xr, np.int64)


def _want(mats, offs, dmat_len, grp, xr):
    where = {int(o): m for o, m in zip(offs, mats)}
    err, cnt = [], []
    for off, nc, a_lo, a_hi, b_lo, b_hi, x0, x1 in grp.tolist():
        good = off in where and nc == len(where[off]) and 0 <= x0 <= len(xr) and 0 <= x1 <= len(xr)
        e, c = X.group(where[off], (a_lo, a_hi), (b_lo, b_hi), [tuple(r) for r in xr[x0:x1].tolist()]) if good else (NAN, (-1,) * 5)
        err.append(e)
        cnt.append(c)
    return np.array(err, np.float64), np.array(cnt, np.int64).reshape(-1, 5)


def _run(dmat, grp, xr):
    from semi_tts_amd import ops
    err, cnt = ops.abx_across(dmat, torch.from_numpy(np.array(grp)).to(DEV), torch.from_numpy(np.array(xr)).to(DEV))    # (copies: the fixture's are read-only)
    torch.cuda.synchronize()
    assert err.dtype == torch.float64 and cnt.dtype == torch.int64 and err.shape == (len(grp),) and cnt.shape == (len(grp), 5)
    return err.cpu().numpy(), cnt.cpu().numpy()


@pytest.fixture(scope='module')
def world():
    """the matrices on the device, the cases as one table, and what brute force says of them (computed once, never changed)"""
    mats, offs, dmat_len = _matrices()
    cases = _cases()
    grp, xr = _assemble(cases, offs, mats)
    err, cnt = _want(mats, offs, dmat_len, grp, xr)
    dmat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(DEV)
    for v in (grp, xr, err, cnt):
        v.setflags(write=False)
    return dict(mats=mats, offs=offs, dmat_len=dmat_len, cases=cases, grp=grp, xr=xr, err=err, cnt=cnt, dmat=dmat)


# ---------------------------------------------------------------- 1. the kernel
def test_every_shape_equals_brute_force(world):
    w = world
    err, cnt = _run(w['dmat'], w['grp'], w['xr'])
    for q, case in enumerate(w['cases']):
        assert cnt[q].tolist() == w['cnt'][q].tolist() and _bits(err[q]) == _bits(w['err'][q]), (case[:3], len(case[3]), cnt[q], w['cnt'][q], err[q], w['err'][q])
    # what the cases are there for did occur
    c = w['cnt']
    assert c[0].tolist()[3:] == [1, 1] and c[1].tolist() == [0, 0, 0, 0, 0] and np.isnan(w['err'][1])
    assert c[2].tolist() == [0] * 5 and c[3].tolist() == [0] * 5 and np.isnan(w['err'][2])
    assert c[5, 3] == 2 * 1 * (1 + 2) and c[6, 3] == 2 * 2 * 2                       # the clamped ranges: [0, 1) and [4, 6); a = [0, 2), b = [4, 6)
    assert c[7].tolist()[2:] == [20, 20 * 20 * 3, 1] and c[11].tolist() == [0, 0, 16, 16, 0] and np.isnan(w['err'][11])
    assert c[12, 4] == 1 and c[12, 2] >= 2 * 3 * 3 and c[13].tolist()[2:] == [1, 4, 1]
    # (a list of n ranges gives a few pair scores fewer than n: the rows of NaN above are ranges of R1 and S1 too)
    assert (c[:, 1] > 0).sum() > 20 and c[14:, 4].max() >= 62 and [len(x[3]) for x in w['cases'][14:]][-4:] == [66, 65, 65, 65]


def test_one_group_and_three_hundred(world):
    w = world
    rs = np.random.RandomState(17)
    pick = rs.randint(0, len(w['grp']), 300)
    err, cnt = _run(w['dmat'], w['grp'][pick], w['xr'])
    assert np.array_equal(cnt, w['cnt'][pick]) and np.array_equal(_bits(err), _bits(w['err'][pick]))
    for q in (0, 7, len(w['grp']) - 1):
        err, cnt = _run(w['dmat'], w['grp'][q:q + 1], w['xr'])
        assert np.array_equal(cnt, w['cnt'][q:q + 1]) and np.array_equal(_bits(err), _bits(w['err'][q:q + 1]))


def test_bad_matrix_and_bad_slice_leave_their_neighbours_alone(world):
    w = world
    grp = w['grp'][[0, 7, 7, 7, 7, 7, 7, 7, 9]].copy()
    NX, L = len(w['xr']), w['dmat_len']
    grp[1, 0] = -1                                  # the matrix starts before dmat
    grp[2, 0] = L - 50 * 50 + 1                     # ... ends past it
    grp[3, 1] = -2                                  # n_c < 0
    grp[4, 1] = (1 << 20) + 1                       # n_c above 2^20
    grp[5, 7] = NX + 1                              # the slice ends past xr
    grp[6, 6] = -1                                  # ... starts before it
    grp[7, 6] = NX + 3                              # ... starts past it
    err, cnt = _run(w['dmat'], grp, w['xr'])
    assert (cnt[1:8] == -1).all() and np.isnan(err[1:8]).all()
    for q, src in ((0, 0), (8, 9)):
        assert np.array_equal(cnt[q], w['cnt'][src]) and _bits(err[q]) == _bits(w['err'][src])
    # an inverted slice inside xr is an empty list; a matrix that ends exactly with dmat is read
    grp = w['grp'][[7, 11]].copy()
    grp[0, 6], grp[0, 7] = 5, 2
    err, cnt = _run(w['dmat'], grp, w['xr'])
    assert cnt[0].tolist() == [0] * 5 and np.isnan(err[0]) and np.array_equal(cnt[1], w['cnt'][11])


def test_permuted_and_alone_are_bitwise_the_same(world):
    w = world
    first = _run(w['dmat'], w['grp'], w['xr'])
    again = _run(w['dmat'], w['grp'], w['xr'])
    perm = np.random.RandomState(2).permutation(len(w['grp']))
    moved = _run(w['dmat'], w['grp'][perm], w['xr'])
    assert np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(first[1], again[1])
    assert np.array_equal(_bits(moved[0]), _bits(first[0][perm])) and np.array_equal(moved[1], first[1][perm])
    for q in (5, 7, 12, len(w['grp']) - 2):
        alone = _run(w['dmat'], w['grp'][q:q + 1], w['xr'])
        assert _bits(alone[0][0]) == _bits(first[0][q]) and np.array_equal(alone[1][0], first[1][q])


# ---------------------------------------------------------------- 2. metrics.abx_across
def _pack(items):
    starts = np.concatenate([[0], np.cumsum([len(x) for x in items])[:-1]]).astype(np.int64)
    return torch.from_numpy(np.concatenate(items, 0)).to(DEV), starts, np.array([len(x) for x in items], np.int64)


def _tokens():
    """3 speakers x 3 labels x 2 contexts, 1..3 items each (one (context, speaker, label) left out) of 1..6 frames x 5 integer columns"""
    rs = np.random.RandomState(41)
    label, context, speaker, items = [], [], [], []
    for c in range(2):
        for s in range(3):
            for lab in range(3):
                if (c, s, lab) == (1, 2, 0):
                    continue
                for _ in range(rs.randint(1, 4)):
                    label.append(lab)
                    context.append(c)
                    speaker.append(s)
                    items.append(rs.randint(0, 2, (rs.randint(1, 7), 5)).astype(np.float32))       # (0 / 1: distances repeat, ties occur)
    perm = rs.permutation(len(label))
    return [items[p] for p in perm], np.array(label)[perm], np.array(context)[perm], np.array(speaker)[perm]


def _same_as_oracle(res, groups, table, score, speakers):
    keys = list(zip(res.grp_context.tolist(), res.grp_speaker.tolist(), res.grp_a.tolist(), res.grp_b.tolist()))
    assert keys == sorted(groups) and len(keys) == 18 + 14         # every (speaker, a, b) of context 0; context 1 without speaker 2's a
    for k, e, c in zip(keys, res.err, res.counts):
        assert tuple(c.tolist()) == groups[k][1] and _bits(e) == _bits(groups[k][0]), (k, c, e, groups[k])
    assert res.table == [(a, b) + table[(a, b)] for a, b in sorted(table)] and len(res.table) == 6
    assert abs(res.score - score) <= 1e-12 and 0.0 < score < 1.0
    assert res.speakers == [(s,) + speakers[s] for s in sorted(speakers)]


def test_abx_across_integer_items_equal_the_oracle():
    from semi_tts_amd.metrics import abx_across
    items, label, context, speaker = _tokens()
    feat, starts, lens = _pack(items)
    res = abx_across(feat, starts, lens, label, context, speaker, 'euclid')
    dist = lambda p, q: float(O.pair(items[p], items[q], 'euclid', np.float32)[0])       # noqa: E731
    groups, table, score, speakers = X.abx_across(dist, label, context, speaker, items=res.keep)
    _same_as_oracle(res, groups, table, score, speakers)
    assert res.counts[:, 1].sum() > 0 and len(res.keep) == len(label)                    # ties occur
    n = {c: int((context == c).sum()) for c in (0, 1)}
    same = sum(int(((context == c) & (speaker == s)).sum()) ** 2 for c in (0, 1) for s in range(3))
    assert res.pairs == (n[0] ** 2 + n[1] ** 2 - same) // 2
    # subsampled: the oracle on the same subsample
    sub = abx_across(feat, starts, lens, label, context, speaker, 'euclid', max_items=2, seed=3)
    assert len(sub.keep) < len(label)
    groups, table, score, speakers = X.abx_across(dist, label, context, speaker, items=sub.keep)
    keys = list(zip(sub.grp_context.tolist(), sub.grp_speaker.tolist(), sub.grp_a.tolist(), sub.grp_b.tolist()))
    assert keys == sorted(groups) and all(tuple(c.tolist()) == groups[k][1] and _bits(e) == _bits(groups[k][0]) for k, e, c in zip(keys, sub.err, sub.counts))
    assert abs(sub.score - score) <= 1e-12


def test_same_speaker_entries_are_never_read(monkeypatch):
    """the matrices are filled with NaN before the mirrored store: were an entry between two items of one speaker (or the diagonal) read,
    the nan column would count it"""
    from semi_tts_amd import metrics
    items, label, context, speaker = _tokens()
    feat, starts, lens = _pack(items)
    clean = metrics.abx_across(feat, starts, lens, label, context, speaker, 'euclid')
    filled = []

    def nan_first(dist, pl, dev):
        dmat = torch.full((pl.dmat_len,), NAN, device=dev, dtype=torch.float32)
        dmat[torch.from_numpy(np.concatenate([pl.pos_ab, pl.pos_ba])).to(dev)] = torch.cat([dist, dist])
        filled.append(int(torch.isnan(dmat).sum()))
        return dmat
    monkeypatch.setattr(metrics, '_abx_across_dmat', nan_first)
    res = metrics.abx_across(feat, starts, lens, label, context, speaker, 'euclid')
    assert filled and filled[0] > len(label)                                             # the same-speaker entries did hold NaN
    assert (res.counts[:, 2] == 0).all() and np.array_equal(res.counts, clean.counts) and np.array_equal(_bits(res.err), _bits(clean.err))
    assert res.table == clean.table and res.score == clean.score


# ---------------------------------------------------------------- 3. the command line
SR = 22050
ALI = {     # symbol, start frame, end frame at frame_s = 0.05: 12 frames = 0.6 s
    'u1': [('sil', 0, 2), ('a', 2, 4), ('sil', 4, 6), ('b', 6, 9), ('sil', 9, 12)],
    'u2': [('sil', 1, 2), ('b', 2, 5), ('sil', 5, 7), ('a', 7, 9), ('sil', 9, 11)],
    'u3': [('sil', 0, 3), ('a', 3, 6), ('c', 6, 9), ('sil', 9, 12)],
    'u4': [('c', 0, 3), ('sil', 3, 5), ('b', 5, 8), ('a', 8, 12)],
}
SPK = {'u1': 'ann', 'u2': 'ann', 'u3': 'bob', 'u4': 'bob'}       # without sil: ann has a x 2, b x 2; bob a x 2, b x 1, c x 2


def _wave(L, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / SR
    ph = 2 * np.pi * np.cumsum(120 + 80 * rs.rand() + 40 * np.sin(2 * np.pi * 3 * t + rs.rand())) / SR
    return (0.5 * sum(np.sin((h + 1) * ph + rs.rand()) / (h + 1) for h in range(5)) * (0.3 + 0.7 * rs.rand(L // 2205 + 1).repeat(2205)[:L])
            + 0.01 * rs.randn(L)).astype(np.float32)


@pytest.fixture()
def abx_dirs(tmp_path):
    from semi_tts_amd.audio import write_wav
    ali_dir, wav_dir = tmp_path / 'ali', tmp_path / 'wav'
    ali_dir.mkdir()
    wav_dir.mkdir()
    for k, (stem, toks) in enumerate(ALI.items()):
        write_wav(wav_dir / (stem + '.wav'), _wave(13230 + 441 * k, 60 + k), SR)
        (ali_dir / (stem + '.ali')).write_text('# score=-1.000000 frames=12 frame_s=0.050000\n' + ''.join(
            '%s\t%d\t%d\t%.6f\t%.6f\n' % (s, a, b, a * 0.05, b * 0.05) for s, a, b in toks))
    (tmp_path / 'spk.csv').write_text('key,speaker\n' + ''.join('%s,%s\n' % kv for kv in SPK.items()))
    (tmp_path / 'one.csv').write_text(''.join('%s,ann\n' % k for k in SPK))
    return ali_dir, wav_dir, tmp_path / 'log', tmp_path


def test_abx_mode_across_and_both_end_to_end(abx_dirs, capsys):
    import main
    import yaml
    from semi_tts_amd import abx as A
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.metrics import abx_across
    ali_dir, wav_dir, log, tmp = abx_dirs
    cfg = os.path.join(REPO, 'config', 'supervised.yaml')
    base = ['--config', cfg, '--abx-ali-dir', str(ali_dir), '--abx-wav-dir', str(wav_dir), '--abx-context', 'none', '--abx-ignore', 'sil',
            '--abx-spk-map', str(tmp / 'spk.csv'), '--logdir', str(log), '--batch-size', '3']
    for mode in ('within', 'across', 'both'):
        main.main(base + ['--name', mode] + ([] if mode == 'within' else ['--abx-mode', mode]))
    out = capsys.readouterr().out
    assert sorted(os.listdir(log / 'within')) == ['abx.csv', 'abx_phones.csv']
    assert sorted(os.listdir(log / 'across')) == ['abx_across.csv', 'abx_across_speakers.csv', 'abx_phones.csv']
    assert sorted(os.listdir(log / 'both')) == ['abx.csv', 'abx_across.csv', 'abx_across_speakers.csv', 'abx_phones.csv']
    read = lambda mode, name: (log / mode / name).read_bytes()                            # noqa: E731
    assert read('both', 'abx.csv') == read('within', 'abx.csv') and read('both', 'abx_across.csv') == read('across', 'abx_across.csv')
    assert read('both', 'abx_across_speakers.csv') == read('across', 'abx_across_speakers.csv')
    assert read('both', 'abx_phones.csv') == read('within', 'abx_phones.csv') == read('across', 'abx_phones.csv')
    # the same features, file by file, and the items by hand
    conv = load_audio_transform(**yaml.load(open(cfg), Loader=yaml.FullLoader)['data']['audio'])
    hop = conv.hop_length_mfcc
    parts, rows, first = [], [], 0
    for stem in sorted(ALI):
        x = conv.load(wav_dir / (stem + '.wav'))[0]
        n = 1 + len(x) // hop
        parts.append(conv.extract_mfcc_batch([x])[0, :n])
        its, _ = A.utterance_items(A.read_ali(str(ali_dir / (stem + '.ali'))), hop / float(SR), n, ('sil',), 1)
        rows += [(s, first + r0, ln, SPK[stem]) for s, r0, ln, p, q in its]
        first += n
    names, spk = ['a', 'b', 'c'], ['ann', 'bob']
    res = abx_across(torch.cat(parts, 0).contiguous(), [r[1] for r in rows], [r[2] for r in rows], [names.index(r[0]) for r in rows],
                     [0] * len(rows), [spk.index(r[3]) for r in rows], 'angular', 50, 0)
    assert (log / 'across' / 'abx_across.csv').read_text() == A.format_abx_across_csv(res.table, names)
    assert (log / 'across' / 'abx_across_speakers.csv').read_text() == A.format_abx_across_speakers_csv(res.speakers, spk)
    # ann: (a, b), (b, a); bob: (a, b), (b, a) -- c is bob's alone, so it is a B but never an a: (a, c), (b, c)
    assert [r[:3] for r in res.table] == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 1)] and np.isfinite(res.score) and res.pairs == 4 * 5
    line = 'across-speaker ABX error of mfcc (angular, context none): %.2f %% over %d phone pairs, %d groups, %d triples, %d pairs of DTW' % (
        100 * res.score, len(res.table), sum(r[2] for r in res.table), sum(r[3] for r in res.table), res.pairs)
    assert out.count(line) == 2 and out.count('[INFO] ABX error of mfcc') == 2


def test_abx_mode_refusals(abx_dirs, capsys):
    import main
    ali_dir, wav_dir, log, tmp = abx_dirs
    base = ['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--abx-ali-dir', str(ali_dir), '--abx-wav-dir', str(wav_dir), '--logdir', str(log)]
    for mode in ('across', 'both'):
        with pytest.raises(SystemExit):
            main.main(base + ['--abx-mode', mode])
        assert '--abx-mode %s takes X from another speaker: it needs --abx-spk-map' % mode in capsys.readouterr().err
        with pytest.raises(ValueError, match=r'--abx-mode %s needs --abx-spk-map FILE with at least two speakers among the files \(got 1 speaker\)' % mode):
            main.main(base + ['--abx-mode', mode, '--abx-spk-map', str(tmp / 'one.csv')])
    assert not os.path.exists(log)
    # two speakers among the files, one among the kept items: bob's only file holds nothing but what --abx-ignore drops
    (tmp / 'two.csv').write_text('u1,ann\nu2,ann\nu3,bob\nu4,ann\n')
    for mode in ('across', 'both'):
        with pytest.raises(ValueError, match=r'--abx-mode %s: the kept items come from fewer than two speakers; --abx-spk-map' % mode):
            main.main(base + ['--abx-mode', mode, '--abx-spk-map', str(tmp / 'two.csv'), '--abx-ignore', 'sil,a,c'])
    assert not os.path.exists(log)
