"""st_edit_align on the device against the integer oracle of tests/edit_align_oracle.py -- integers only, equality only -- and the
--score-phn-dir path end to end.

The kernel has three forms, chosen from the padded widths (Lr, Lh) alone:
  * Lh <= 256: 4 hypothesis columns per lane, the 2-bit moves always in LDS (64 bytes a reference row) -- every small case, (257, 130),
    (1024, 1) scored alone (80 KiB of LDS: past the 48 KiB that need the opt-in), and Lh = 256 exactly;
  * Lh > 256, moves in LDS: 16 columns per lane, 256 bytes a row, while 12 (Lr + Lh) + 256 Lr bytes fit the CU -- (130, 257), more
    columns than one pass of 64 lanes x 4 covers, and (597, 257), the last Lr that fits at Lh = 257;
  * Lh > 256, moves in the workspace: (598, 257), the first Lr that does not fit, and (1024, 1024) with (1024, 1) as the second pair
    of the same call, whose table starts at an offset.
test_forms_are_the_ones_named pins these through st_edit_align_workspace_bytes."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import edit_align_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = 10 ** 12 + 7             # past every length: an id that is never a token (and does not fit int32)


def _run(hyp, hyp_len, ref, ref_len=None, ignore=(), V=64, confusion=None, want_ali=True, device_lens=False):
    """hyp (B, N, Lh), ref (B, Lr) int64 arrays -> (counts, ali_len, ali, confusion) as numpy arrays"""
    from semi_tts_amd import ops
    h, r = torch.from_numpy(np.ascontiguousarray(hyp, np.int64)).to(DEV), torch.from_numpy(np.ascontiguousarray(ref, np.int64)).to(DEV)
    if device_lens:
        hyp_len = torch.tensor(hyp_len, dtype=torch.int64).to(DEV)
        ref_len = None if ref_len is None else torch.tensor(ref_len, dtype=torch.int32).to(DEV)
    conf = torch.zeros(V + 1, V + 1, dtype=torch.int32, device=DEV) if confusion is None else confusion
    counts, ali_len, ali, conf = ops.edit_align(h, hyp_len, r, ref_len, ignore, V, conf, want_ali)
    return counts.cpu().numpy(), ali_len.cpu().numpy(), None if ali is None else ali.cpu().numpy(), conf.cpu().numpy()


def _batch(pairs, Lr=None, Lh=None):
    """[(ref, hyp)] -> hyp (B, 1, Lh), hyp_len (B, 1), ref (B, Lr), ref_len (B,) padded with POISON"""
    Lr = Lr or max(1, max(len(r) for r, _ in pairs))
    Lh = Lh or max(1, max(len(h) for _, h in pairs))
    return (O.pad([h for _, h in pairs], Lh, POISON)[:, None], [[len(h)] for _, h in pairs], O.pad([r for r, _ in pairs], Lr, POISON),
            [len(r) for r, _ in pairs])


def _assert_equal(got, want, what=''):
    for name, g, w in zip(('counts', 'ali_len', 'ali', 'confusion'), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


def _check(pairs, V=64, ignore=(), Lr=None, Lh=None, **kw):
    hyp, hyp_len, ref, ref_len = _batch(pairs, Lr, Lh)
    got = _run(hyp, hyp_len, ref, ref_len, ignore, V, **kw)
    _assert_equal(got, O.batch(hyp, hyp_len, ref, ref_len, ignore, V), [(len(r), len(h)) for r, h in pairs][:8])
    return got


SMALL = [(n, m) for n in (0, 1, 2, 3, 63, 64, 65) for m in (0, 1, 2, 5, 64, 66)]


@pytest.mark.parametrize('alphabet', [2, 3, 40])
def test_every_small_shape(alphabet):
    """every (n, m) of SMALL: counts, ali_len and all of ali with its -1 tail equal the oracle -- each pair alone at its own widths
    (n or m = 0 at width 1), then all of them as one ragged batch"""
    rs = np.random.RandomState(alphabet)
    pairs = [O.random_pair(rs, n, m, alphabet) for n, m in SMALL]
    for pair in pairs:
        _check([pair])
    _check(pairs)


def test_ragged_batch_never_reads_past_the_lengths():
    """B = 5 with poison ids past every length; the same batch with other ids there gives the same tensors; a pair equals itself alone"""
    rs = np.random.RandomState(5)
    pairs = [O.random_pair(rs, n, m, 3) for n, m in ((17, 30), (0, 4), (33, 1), (40, 40), (5, 0))]
    got = _check(pairs, Lr=48, Lh=50)
    hyp, hyp_len, ref, ref_len = _batch(pairs, 48, 50)
    hyp2, ref2 = np.where(hyp == POISON, 4, hyp), np.where(ref == POISON, 3, ref)
    _assert_equal(_run(hyp2, hyp_len, ref2, ref_len), got)
    for b, pair in enumerate(pairs):
        alone = _check([pair], Lr=48, Lh=50)
        assert np.array_equal(alone[0][0], got[0][b]) and np.array_equal(alone[2][0], got[2][b])


def test_ignored_ids_on_both_sides():
    rs = np.random.RandomState(11)
    pairs = []
    for n, m in ((30, 28), (64, 70), (1, 9), (130, 100)):
        r, h = O.random_pair(rs, n, m, 6, first=0)                  # ids 0 .. 5, of which 0, 1, 2 and 5 are dropped wherever they sit
        pairs.append((r, h))
    pairs.append(([0, 1, 2, 5, 0], [3, 4]))                         # a reference that is empty once filtered
    pairs.append(([3, 4], [2, 2, 2]))                               # ... a hypothesis
    for ignore in ((0, 1, 2, 5), (0, 1, 2), (4,), tuple(range(100, 164))):
        _check(pairs, V=6, ignore=ignore)


def test_device_lengths_are_clamped():
    rs = np.random.RandomState(13)
    pairs = [O.random_pair(rs, 20, 24, 3) for _ in range(4)]
    hyp, _, ref, _ = _batch(pairs)
    hyp_len, ref_len = [[99], [-5], [24], [7]], [20, 1 << 30, -1, 12]
    got = _run(hyp, hyp_len, ref, ref_len, device_lens=True)
    _assert_equal(got, O.batch(hyp, hyp_len, ref, ref_len, (), 64))
    assert got[0][1, 0].tolist() == [0, 0, 20, 0] and got[0][2, 0].tolist() == [0, 0, 0, 24]       # (1 << 30 -> Lr, -5 -> 0; -1 -> 0)
    _assert_equal(_run(hyp, hyp_len, ref, None, device_lens=True), O.batch(hyp, hyp_len, ref, None, (), 64))


def test_forms_are_the_ones_named():
    from semi_tts_amd import _lib
    ws = _lib.load().st_edit_align_workspace_bytes
    assert [int(ws(1, Lr, Lh)) for Lr, Lh in ((257, 130), (1024, 1), (1024, 256), (130, 257), (597, 257))] == [0] * 5
    assert int(ws(1, 598, 257)) == 598 * 256 and int(ws(2, 1024, 1024)) == 2 * 1024 * 256


@pytest.mark.parametrize('n,m,alphabet', [(257, 130, 2), (130, 257, 2), (256, 256, 3), (255, 257, 3), (300, 300, 40), (1024, 1, 2),
                                          (597, 257, 3), (598, 257, 3)])
def test_both_sides_of_every_boundary(n, m, alphabet):
    """one pair at exactly its own widths (see the module docstring for the form each shape reaches), a second short pair behind it"""
    rs = np.random.RandomState(n + m)
    ref, hyp = O.random_pair(rs, n, m, alphabet)
    if alphabet == 40:                                                      # (a hypothesis that resembles its reference)
        ref, hyp = O.edited_pair(rs, n, alphabet, 0.3)
        hyp = (hyp + ref)[:m]
    _check([(ref, hyp), O.random_pair(rs, min(7, n), min(5, m), alphabet)], Lr=n, Lh=m)


def test_largest_table_in_the_workspace():
    """(1024, 1024), the limit, with (1024, 1) as the second pair of the call: its moves start 256 KiB into the workspace"""
    rs = np.random.RandomState(1024)
    ref, hyp = O.edited_pair(rs, 1024, 3, 0.3)
    got = _check([(ref, (hyp + hyp)[:1024]), (ref[::-1], [4])], V=8)
    assert got[1].tolist() == [[got[0][0, 0].sum()], [1024]]


def test_n_paths_equal_the_paths_alone():
    from semi_tts_amd import metrics
    rs = np.random.RandomState(4)
    B, N, Lr, Lh, V = 3, 4, 40, 44, 8
    refs = [rs.randint(3, 6, size=n).tolist() for n in (40, 25, 31)]
    hyps = [[rs.randint(3, 6, size=m).tolist() for m in ms] for ms in ((44, 30, 0, 41), (25, 25, 26, 1), (31, 28, 33, 30))]
    hyps[1][1] = list(refs[1])                                              # utterance 1: paths 1 and 3 both exact -> the lowest k = 1
    hyps[1][3] = list(refs[1])
    hyps[2] = [hyps[2][0]] * 4                                              # utterance 2: all paths tie -> k = 0
    hyp = np.stack([O.pad(h, Lh, POISON) for h in hyps])
    hyp_len = [[len(t) for t in h] for h in hyps]
    ref = O.pad(refs, Lr, POISON)
    ref_len = [len(r) for r in refs]
    got = _run(hyp, hyp_len, ref, ref_len, V=V)
    _assert_equal(got, O.batch(hyp, hyp_len, ref, ref_len, (), V))
    for k in range(N):                                                      # every path equals that path scored alone
        alone = _run(hyp[:, k:k + 1], [[l[k]] for l in hyp_len], ref, ref_len, V=V)
        assert np.array_equal(alone[0][:, 0], got[0][:, k]) and np.array_equal(alone[2][:, 0], got[2][:, k])
        if k == 0:
            assert np.array_equal(alone[3], got[3])                         # the confusion matrix comes from path 0 only
    res = metrics.align_transcripts(torch.from_numpy(hyp).to(DEV), hyp_len, torch.from_numpy(ref).to(DEV), ref_len, ignore=(), n_classes=V)
    assert np.array_equal(res.confusion.cpu().numpy(), got[3]) and res.dist.shape == (B, N) and res.ali.shape == (B, N, Lr + Lh, 2)
    assert np.array_equal(res.dist.cpu().numpy(), got[0][:, :, 1:].sum(axis=2))
    assert np.array_equal(res.ref_len.cpu().numpy(), np.repeat(np.asarray(ref_len)[:, None], N, 1)) and np.array_equal(res.hyp_len.cpu().numpy(), hyp_len)
    nb = metrics.nbest_per(res.dist)
    dist = got[0][:, :, 1:].sum(axis=2)
    assert nb.dist.cpu().tolist() == dist.min(axis=1).tolist() and nb.path.cpu().tolist() == dist.argmin(axis=1).tolist()
    assert nb.path.cpu().tolist()[1:] == [1, 0] and nb.dist.cpu().tolist()[1] == 0
    single = metrics.align_transcripts(torch.from_numpy(hyp[:, 0]).to(DEV), [l[0] for l in hyp_len], torch.from_numpy(ref).to(DEV), ref_len, ignore=())
    assert single.correct.shape == (B,) and single.ali.shape == (B, Lr + Lh, 2) and single.confusion is None
    assert np.array_equal(single.ali.cpu().numpy(), got[2][:, 0])


def test_confusion_accumulates_and_skips_foreign_tokens():
    rs = np.random.RandomState(21)
    V = 6
    a = [O.random_pair(rs, n, m, 3) for n, m in ((50, 47), (20, 33), (0, 6))]
    b = [O.random_pair(rs, n, m, 5) for n, m in ((64, 64), (31, 2))]            # ids 3 .. 7: 6 and 7 lie outside [0, V)
    ha, la, ra, rla = _batch(a)
    hb, lb, rb, rlb = _batch(b)
    wa, wb = O.batch(ha, la, ra, rla, (), V), O.batch(hb, lb, rb, rlb, (), V)
    conf = torch.zeros(V + 1, V + 1, dtype=torch.int32, device=DEV)
    _run(ha, la, ra, rla, V=V, confusion=conf)
    gb = _run(hb, lb, rb, rlb, V=V, confusion=conf)
    assert np.array_equal(conf.cpu().numpy(), wa[3] + wb[3])                    # two calls into one tensor: the oracle's sum
    assert np.array_equal(gb[0], wb[0]) and wb[3].sum() < wb[1].sum()           # the counts include the foreign tokens, the matrix does not
    only_foreign = [([6, 7, 6], [7, 7]), ([7], [])]
    got = _check(only_foreign, V=V)
    assert got[3].sum() == 0 and got[0].sum() == 4
    again = _run(ha, la, ra, rla, V=V)                                          # two runs: identical tensors
    _assert_equal(again, _run(ha, la, ra, rla, V=V))
    _assert_equal(again, wa)
    assert _run(ha, la, ra, rla, V=V, want_ali=False)[2] is None


def test_distance_equals_the_shipped_kernel():
    """dist and ref_len equal ops.hyp_edit_distance on the same inputs and the same ignore"""
    from semi_tts_amd import ops
    rs = np.random.RandomState(31)
    pairs = [O.edited_pair(rs, n, 40, 0.15, first=0) for n in (40, 77, 100, 3, 64, 200)] + [O.random_pair(rs, 90, 70, 3, first=0)]
    hyp, hyp_len, ref, ref_len = _batch(pairs)
    ref = np.where(ref == POISON, 0, ref)                                       # (the shipped kernel takes all L: pad with an ignored id)
    for ignore in ((0, 1, 2, 42), (0,)):
        counts = _run(hyp, hyp_len, ref, None, ignore)[0][:, 0]
        dist, n_ref = ops.hyp_edit_distance(torch.from_numpy(hyp[:, 0]).to(DEV), torch.tensor([l[0] for l in hyp_len], dtype=torch.int32).to(DEV),
                                            torch.from_numpy(ref).to(DEV), ignore)
        assert np.array_equal(dist.cpu().numpy(), counts[:, 1:].sum(axis=1)) and np.array_equal(n_ref.cpu().numpy(), counts[:, :3].sum(axis=1))


VOCAB = ['<pad>', '<space>', '<eos>', 'AA', 'B', 'CH', 'D', 'EH']


def test_score_phn_dir_end_to_end(tmp_path, capsys):
    import main
    hyp_dir, ref_dir, log = tmp_path / 'hyp', tmp_path / 'ref', tmp_path / 'log'
    hyp_dir.mkdir()
    ref_dir.mkdir()
    (tmp_path / 'v.vocab').write_text('\n'.join(VOCAB[3:]) + '\n')
    refs = {'a': [3, 4, 5, 6, 3, 4, 5, 6, 2], 'b': [3, 3, 1, 4], 'c': [7, 6, 5], 'd': [4, 4, 4, 4], 'e': [5], 'f': [6, 7, 6, 7, 6]}
    hyps = {'a-pred': [[3, 5, 5, 3, 4, 6, 5, 6]], 'b': [[3, 4, 4], [3, 3, 4], [4]], 'c': [[]], 'd': [[4, 4, 4, 4]], 'e': [[5, 5, 1, 5]],
            'f': [[7, 6, 7, 6], [6, 7, 6, 7, 6]]}
    for key, r in refs.items():
        (ref_dir / (key + '.phn')).write_text(' '.join(VOCAB[t] for t in r) + '\n')
    for name, paths in hyps.items():
        (hyp_dir / (name + '.phn')).write_text(''.join('%.6f\t%s\n' % (-1.0 - k, ' '.join(VOCAB[t] for t in p)) for k, p in enumerate(paths)))
    argv = ['--score-phn-dir', str(hyp_dir), '--score-ref-dir', str(ref_dir), '--vocab', str(tmp_path / 'v.vocab'), '--logdir', str(log)]
    main.main(argv + ['--name', 'all', '--score-nbest', '--score-ali', '--batch-size', '4'])
    main.main(argv + ['--name', 'plain', '--score-ignore', '0,1,2,7'])
    out = capsys.readouterr().out
    names = sorted(hyps)
    V = len(VOCAB)

    def want(ignore, nbest):
        rows, conf, alis = [], np.zeros((V + 1, V + 1), np.int64), {}
        for name in names:
            key = name[:-5] if name.endswith('-pred') else name
            res = [O.align(refs[key], p, ignore) for p in hyps[name]]
            dists = [sum(c[1:]) for c, _ in res]
            rows.append((name + '.phn', res[0][0]) + ((min(dists), dists.index(min(dists))) if nbest else ()))
            O.add_confusion(conf, res[0][1], V)
            alis[key] = res[0][1]
        return rows, conf, alis
    rows, conf, alis = want((0, 1, 2), True)
    assert (log / 'all' / 'per.csv').read_text() == O.per_text(rows, nbest=True)
    assert np.array_equal(np.load(log / 'all' / 'confusion.npy'), conf) and np.load(log / 'all' / 'confusion.npy').dtype == np.int64
    assert (log / 'all' / 'confusions.csv').read_text() == O.confusions_text(conf, VOCAB)
    assert (log / 'all' / 'phones.csv').read_text() == O.phones_text(conf, VOCAB)
    for key, pairs in alis.items():
        assert (log / 'all' / (key + '.ops')).read_text() == O.ops_text(pairs, VOCAB)
    assert rows[1][2:] == (0, 1) and rows[5][2:] == (0, 1) and rows[2][1] == (0, 0, 3, 0)      # b, f: the second path is better; c: all deleted
    rows, conf, _ = want((0, 1, 2, 7), False)
    assert (log / 'plain' / 'per.csv').read_text() == O.per_text(rows)
    assert (log / 'plain' / 'confusions.csv').read_text() == O.confusions_text(conf, VOCAB)
    assert (log / 'plain' / 'phones.csv').read_text() == O.phones_text(conf, VOCAB)
    assert sorted(os.listdir(log / 'plain')) == ['confusion.npy', 'confusions.csv', 'per.csv', 'phones.csv']
    tot = np.sum([r[1] for r in want((0, 1, 2), True)[0]], axis=0)
    assert 'corpus %.4f' % (tot[1:].sum() / tot[:3].sum()) in out and 'n-best oracle' in out
    # a directory against itself: PER 0, a diagonal matrix, an empty confusions.csv body
    main.main(['--score-phn-dir', str(ref_dir), '--score-ref-dir', str(ref_dir), '--logdir', str(log), '--name', 'self', '--vocab', str(tmp_path / 'v.vocab')])
    conf = np.load(log / 'self' / 'confusion.npy')
    assert np.array_equal(conf, np.diag(np.diag(conf))) and conf.sum() == sum(len([t for t in r if t > 2]) for r in refs.values())
    assert (log / 'self' / 'confusions.csv').read_text() == 'ref,hyp,count\n'
    assert all(line.endswith(',0,0,0,0.000000') for line in (log / 'self' / 'per.csv').read_text().splitlines()[1:])
    os.remove(ref_dir / 'c.phn')
    with pytest.raises(ValueError, match=r'c\.phn has no reference'):
        main.main(argv + ['--name', 'missing'])
    assert not (log / 'missing').exists()
