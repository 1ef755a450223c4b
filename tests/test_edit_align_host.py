"""CPU checks of the transcript scorer: the identities of the integer oracle (tests/edit_align_oracle.py) on random and adversarial
pairs, the exported symbols and the workspace size, the argument checks of st_edit_align / ops.edit_align / metrics.align_transcripts
(they fire before any device is touched), the reader of multi-line hypothesis files, the pairing rules, the exact text of per.csv,
confusions.csv, phones.csv and .ops for a hand-made example, and the --score-phn-dir parser rules."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import edit_align_oracle as O  # noqa: E402


# ---------------------------------------------------------------- the oracle
def test_oracle_identities_on_random_pairs():
    rs = np.random.RandomState(7)
    n_pairs = 0
    for alphabet in (2, 3, 40):
        for _ in range(120):
            n, m = int(rs.randint(0, 13)), int(rs.randint(0, 13))
            r, h = O.random_pair(rs, n, m, alphabet)
            (c, s, d, i), pairs = O.align(r, h)
            assert c + s + d == n and c + s + i == m and len(pairs) == c + s + d + i
            assert s + d + i == O.levenshtein(r, h) == O.levenshtein(h, r) == int(O.table(r, h)[n, m])
            assert O.is_cover(pairs, r, h)
            V = 3 + alphabet
            conf = O.add_confusion(np.zeros((V + 1, V + 1), np.int64), pairs, V)
            assert conf[:V, :V].trace() == c and conf[:V, :V].sum() - c == s and conf[:V, V].sum() == d and conf[V, :V].sum() == i
            assert conf[V, V] == 0
            for t in range(V):
                assert conf[t, :].sum() == r.count(t) and conf[:, t].sum() == h.count(t)
            n_pairs += 1
    assert n_pairs == 360


def test_oracle_distance_equals_brute_force():
    rs = np.random.RandomState(1)
    for alphabet in (2, 3):
        for n in range(5):
            for m in range(5):
                r, h = O.random_pair(rs, n, m, alphabet)
                assert sum(O.align(r, h)[0][1:]) == O.brute_force_distance(r, h)


def test_oracle_tie_rule():
    # every cell a tie: the diagonal first on the way back from the corner, then the deletion (i-1, j), then the insertion (i, j-1)
    assert O.align([5, 5, 5, 5], [6, 6])[1] == [(5, -1), (5, -1), (5, 6), (5, 6)]
    assert O.align([5, 5], [6, 6, 6, 6])[1] == [(-1, 6), (-1, 6), (5, 6), (5, 6)]
    assert O.align([3, 4], [4, 3]) == ((0, 2, 0, 0), [(3, 4), (4, 3)])                  # two substitutions, not delete + insert
    assert O.align([3, 4, 3], [4, 3])[1] == [(3, -1), (4, 4), (3, 3)]
    assert O.align([], []) == ((0, 0, 0, 0), [])
    assert O.align([7, 8], []) == ((0, 0, 2, 0), [(7, -1), (8, -1)])
    assert O.align([], [7, 8]) == ((0, 0, 0, 2), [(-1, 7), (-1, 8)])
    assert O.align([0, 7, 1, 8, 2], [2, 2, 7, 9], ignore=(0, 1, 2)) == ((1, 1, 0, 0), [(7, 7), (8, 9)])
    assert not O.is_cover([(-1, -1)], [], []) and not O.is_cover([(3, 3)], [3], [4])


def test_oracle_batch_clamps_lengths_and_takes_confusion_from_path_0():
    hyp = np.array([[[3, 4, 5], [3, 9, 9]]])
    ref = np.array([[3, 4, 6, 7]])
    counts, ali_len, ali, conf = O.batch(hyp, [[7, -2]], ref, [3], (), 8)
    assert counts.tolist() == [[[2, 1, 0, 0], [0, 0, 3, 0]]] and ali_len.tolist() == [[3, 3]]
    assert ali[0, 0].tolist() == [[3, 3], [4, 4], [6, 5]] + [[-1, -1]] * 4
    assert conf.sum() == 3 and conf[6, 5] == 1 and conf[3, 3] == 1
    assert O.batch(hyp, [[3, 3]], ref, None, (), 5)[3].sum() == 2                      # 5, 6, 7 lie outside [0, 5): their pairs touch no cell


# ---------------------------------------------------------------- the library
def test_library_exports_and_workspace():
    from semi_tts_amd import _lib, build
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'st_edit_align') and hasattr(lib, 'st_edit_align_workspace_bytes')
    assert len(_lib.SIGNATURES['st_edit_align']) == 17 and build.SCORE_SOURCES == ['edit_align.hip']
    assert os.path.exists(os.path.join(build.CSRC, 'edit_align.hip'))
    ws = lib.st_edit_align_workspace_bytes
    ws.argtypes, ws.restype = [ctypes.c_int] * 3, ctypes.c_size_t
    for Lr, Lh in ((100, 100), (1024, 256), (1, 1), (563, 1024), (597, 257)):       # the moves fit LDS: no workspace
        assert ws(32, Lr, Lh) == 0, (Lr, Lh)
    assert ws(1, 1024, 1024) == 1024 * 256 and ws(3, 564, 1024) == 3 * 564 * 256 and ws(2, 598, 257) == 2 * 598 * 256
    assert ws(0, 1024, 1024) == 0 and ws(1, 1025, 1024) == 0 and ws(1, 1024, 0) == 0    # outside the limits: nothing to hold


def test_c_entry_refuses_each_limit_without_a_device():
    """the limit checks precede the launch: -22 and a message naming the entry point, with pointers that are never dereferenced"""
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(B=1, N=1, Lh=4, Lr=4, n_ignore=0, ignore=None, V=4, hyp=p, counts=p, ws=None):
        return lib.st_edit_align(hyp, p, B, N, Lh, p, None, Lr, ignore, n_ignore, V, counts, p, None, None, ws, None)
    for kw in (dict(B=0), dict(N=0), dict(B=1 << 20, N=1 << 10), dict(Lh=0), dict(Lr=0), dict(Lh=1025), dict(Lr=1025), dict(V=0), dict(V=1025),
               dict(n_ignore=-1), dict(n_ignore=65, ignore=p), dict(n_ignore=2), dict(hyp=None), dict(counts=None),
               dict(Lr=1024, Lh=1024)):                                  # (the last: a table that needs the workspace, none given)
        assert call(**kw) == -22, kw
        assert b'st_edit_align' in lib.st_last_error()


# ---------------------------------------------------------------- ops argument checks
def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops, metrics
    _no_device(monkeypatch)
    hyp, ref = torch.zeros(2, 3, 5, dtype=torch.int64), torch.zeros(2, 6, dtype=torch.int64)
    for kw in (dict(hyp=hyp, ref=ref), dict(hyp=[[1]], ref=ref)):                      # CPU tensors, not tensors
        with pytest.raises(ValueError, match='GPU tensor'):
            ops.edit_align(hyp_len=[[1] * 3] * 2, **kw)
    # the remaining checks read .is_cuda / .device / .shape / .dtype only: a meta tensor stands in for a device tensor
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    mh, mr = hyp.to('meta'), ref.to('meta')
    hl = [[5, 0, 3], [1, 2, 3]]
    big = torch.empty(1, 1, 1025, dtype=torch.int64, device='meta')
    cases = [
        (dict(hyp=mh, ref=ref), 'ref must be'),
        (dict(hyp=mh.int(), ref=mr), 'int64'),
        (dict(hyp=mh[0], ref=mr), r'\(B, N, Lh\)'),
        (dict(hyp=mh, ref=mr[:1]), 'must match'),
        (dict(hyp=mh[:0], ref=mr[:0], hyp_len=[]), 'B=0'),
        (dict(hyp=mh[:, :0], ref=mr, hyp_len=[[], []]), 'N=0'),
        (dict(hyp=mh[:, :, :0], ref=mr), 'Lh=0'),
        (dict(hyp=mh, ref=mr[:, :0]), 'Lr=0'),
        (dict(hyp=big, ref=mr[:1], hyp_len=[[3]]), 'Lh=1025'),
        (dict(hyp=mh[:1, :1], ref=big[0], hyp_len=[[3]]), 'Lr=1025'),
        (dict(hyp=mh, ref=mr, n_classes=0), 'n_classes'),
        (dict(hyp=mh, ref=mr, n_classes=1025), 'n_classes'),
        (dict(hyp=mh, ref=mr, n_classes=2.0), 'n_classes'),
        (dict(hyp=mh, ref=mr, ignore=range(65)), 'at most 64'),
        (dict(hyp=mh, ref=mr, ignore=(2 ** 31,)), 'int32'),
        (dict(hyp=mh, ref=mr, ignore=3), 'ignore'),
        (dict(hyp=mh, ref=mr, hyp_len=[[6, 0, 0], [0, 0, 0]]), 'hyp_len'),
        (dict(hyp=mh, ref=mr, hyp_len=[[-1, 0, 0], [0, 0, 0]]), 'hyp_len'),
        (dict(hyp=mh, ref=mr, hyp_len=[1, 2]), 'hyp_len'),
        (dict(hyp=mh, ref=mr, hyp_len=torch.ones(2, 3).to('meta')), 'hyp_len'),
        (dict(hyp=mh, ref=mr, hyp_len=torch.ones(2, 2, dtype=torch.int32).to('meta')), 'hyp_len'),
        (dict(hyp=mh, ref=mr, ref_len=[7, 1]), 'ref_len'),
        (dict(hyp=mh, ref=mr, ref_len=[1]), 'ref_len'),
        (dict(hyp=mh, ref=mr, ref_len=torch.ones(2).to('meta')), 'ref_len'),
        (dict(hyp=mh, ref=mr, n_classes=4, confusion=torch.zeros(5, 5, dtype=torch.int32)), 'confusion'),
        (dict(hyp=mh, ref=mr, n_classes=4, confusion=torch.zeros(4, 5, dtype=torch.int32).to('meta')), 'confusion'),
        (dict(hyp=mh, ref=mr, n_classes=4, confusion=torch.zeros(5, 5, dtype=torch.int64).to('meta')), 'confusion'),
    ]
    for kw, msg in cases:
        kw.setdefault('hyp_len', hl)
        with pytest.raises(ValueError, match=msg):
            ops.edit_align(**kw)
    with pytest.raises(ValueError, match='Lh=1025'):
        metrics.align_transcripts(big[0], [3], mr[:1])
    with pytest.raises(ValueError, match='n_classes'):
        metrics.align_transcripts(mh, hl, mr, n_classes=0)
    with pytest.raises(ValueError, match=r'\(B, Lh\) or \(B, N, Lh\)'):
        metrics.align_transcripts(mh[0, 0], [3], mr)
    with pytest.raises(ValueError, match='N >= 1'):
        metrics.nbest_per(torch.zeros(3))
    assert ops.EA_MAX_L == 1024 and ops.EA_MAX_V == 1024 and ops.EA_MAX_IGNORE == 64
    # arguments the kernel takes get as far as the library (and no further here)
    for kw in (dict(), dict(ref_len=[6, 0], ignore=(0, 1, 2), n_classes=7, want_ali=False), dict(hyp_len=torch.tensor(hl).to('meta')),
               dict(n_classes=4, confusion=torch.zeros(5, 5, dtype=torch.int32).to('meta'))):
        kw.setdefault('hyp_len', hl)
        with pytest.raises(AssertionError, match='reached the device'):
            ops.edit_align(mh, ref=mr, **kw)
    with pytest.raises(AssertionError, match='reached the device'):
        metrics.align_transcripts(mh[:, 0], [5, 1], mr, n_classes=6)


def test_nbest_per_picks_the_lowest_path_among_ties():
    from semi_tts_amd import metrics
    nb = metrics.nbest_per(torch.tensor([[3, 1, 1, 2], [0, 0, 0, 0], [5, 4, 3, 3]], dtype=torch.int32))
    assert nb.dist.tolist() == [1, 0, 3] and nb.path.tolist() == [1, 0, 2]


# ---------------------------------------------------------------- files
def test_read_phn_paths(tmp_path):
    from semi_tts_amd.ctc_align import read_phn, read_phn_paths
    vocab = ['<pad>', '<space>', '<eos>', 'AA', 'B']
    f = tmp_path / 'a.phn'
    f.write_text('\n-1.500000\tAA B 7\n\n-2.250000\tB\n-3.000000\t\n  \nAA AA\n')
    assert read_phn_paths(str(f), vocab) == [[3, 4, 7], [4], [], [3, 3]]
    assert read_phn(str(f), vocab) == read_phn_paths(str(f), vocab)[0]
    f.write_text('')
    assert read_phn_paths(str(f)) == [[]] and read_phn(str(f)) == []
    f.write_text('3 4 5\n')
    assert read_phn_paths(str(f)) == [[3, 4, 5]]
    f.write_text('-1.0\t3 4\n-2.0\t3 ZZ\n')
    with pytest.raises(ValueError, match=r"a\.phn: unknown symbol 'ZZ'"):
        read_phn_paths(str(f), vocab)
    assert read_phn(str(f), vocab) == [3, 4]                                # (the first line alone is what read_phn reads)
    f.write_text('0\t' + ' '.join(['3'] * 1025) + '\n')
    with pytest.raises(ValueError, match=r'a\.phn: 1025 tokens'):
        read_phn_paths(str(f))
    with pytest.raises(ValueError, match='cannot read'):
        read_phn_paths(str(tmp_path / 'none.phn'))


def test_pairing_maps_pred_files_and_names_a_missing_partner(tmp_path):
    from semi_tts_amd.solver import phn_pairs
    hyp, ref = tmp_path / 'hyp', tmp_path / 'ref'
    hyp.mkdir()
    ref.mkdir()
    with pytest.raises(ValueError, match='no .phn files'):
        phn_pairs(str(hyp), str(ref))
    for f in ('b.phn', 'a-pred.phn', 'notes.txt'):
        (hyp / f).write_text('')
    (ref / 'a.phn').write_text('')
    with pytest.raises(ValueError, match=r'b\.phn has no reference .*ref.b\.phn'):
        phn_pairs(str(hyp), str(ref))
    (ref / 'b.phn').write_text('')
    assert phn_pairs(str(hyp), str(ref)) == [('a-pred.phn', 'a', 'a.phn'), ('b.phn', 'b', 'b.phn')]
    (hyp / 'b-pred.phn').write_text('')
    with pytest.raises(ValueError, match=r'b-pred\.phn and b\.phn share'):
        phn_pairs(str(hyp), str(ref))


class _Paras:
    vocab, name, batch_size, score_nbest, score_ali, score_ignore = None, 'score', 4, False, False, (0, 1, 2)

    def __init__(self, tmp_path, **kw):
        self.score_phn_dir, self.score_ref_dir, self.logdir = str(tmp_path / 'hyp'), str(tmp_path / 'ref'), str(tmp_path / 'log')
        for k, v in kw.items():
            setattr(self, k, v)


def test_scorer_checks_every_file_before_any_device_work(tmp_path, monkeypatch):
    from semi_tts_amd import solver
    _no_device(monkeypatch)
    hyp, ref = tmp_path / 'hyp', tmp_path / 'ref'
    hyp.mkdir()
    ref.mkdir()
    (hyp / 'a-pred.phn').write_text('-1.0\t3 4 5\n-2.0\t3 4\n')
    (hyp / 'b.phn').write_text('-1.0\t6 QQ\n')
    (ref / 'a.phn').write_text('3 4 5 9\n')
    sc = solver.PhnScorer(None, _Paras(tmp_path), 'test')
    with pytest.raises(ValueError, match=r'b\.phn has no reference'):
        sc.load_data()
    (ref / 'b.phn').write_bytes(b'\xff\xfe\x00')
    with pytest.raises(ValueError, match=r"hyp.b\.phn: unknown symbol 'QQ'"):
        sc.load_data()
    (hyp / 'b.phn').write_text('-1.0\t6 7\n')
    with pytest.raises(ValueError, match=r'ref.b\.phn: cannot read'):
        sc.load_data()
    (ref / 'b.phn').write_text('2000\n')
    with pytest.raises(ValueError, match=r'2001 classes .*at most 1024'):
        sc.load_data()
    (ref / 'b.phn').write_text('6\n')
    assert sc.load_data() is sc and sc.n_classes == 10 and sc.hyps == [[[3, 4, 5]], [[6, 7]]] and sc.refs == [[3, 4, 5, 9], [6]]
    vocab = tmp_path / 'v.vocab'
    vocab.write_text('AA\nB\n')
    sc = solver.PhnScorer(None, _Paras(tmp_path, vocab=str(vocab), score_nbest=True), 'test').load_data()
    assert sc.n_classes == 5 and sc.hyps[0] == [[3, 4, 5], [3, 4]]
    assert not os.path.exists(str(tmp_path / 'log'))                        # nothing is written before exec


VOCAB = ['<pad>', '<space>', '<eos>', 'AA', 'B', 'CH', 'D']


def test_exact_text_of_the_written_files():
    """a hand-made example, every character written out: reference AA B CH D AA B CH D against AA CH CH AA B D CH D (B deleted, D heard as
    CH, a D inserted), and AA AA against nothing"""
    from semi_tts_amd import solver
    c1, p1 = O.align([3, 4, 5, 6, 3, 4, 5, 6], [3, 5, 5, 3, 4, 6, 5, 6])
    assert c1 == (6, 1, 1, 1) and p1 == [(3, 3), (4, -1), (5, 5), (6, 5), (3, 3), (4, 4), (-1, 6), (5, 5), (6, 6)]
    c2, p2 = O.align([3, 3], [])
    conf = np.zeros((8, 8), np.int64)
    O.add_confusion(conf, p1, 7)
    O.add_confusion(conf, p2, 7)
    per = '\n'.join([solver.PER_HEADER, solver.per_row('u1-pred.phn', c1), solver.per_row('u2.phn', c2), solver.per_row('u3.phn', (0, 0, 0, 2))]) + '\n'
    assert per == ('file,ref_tokens,hyp_tokens,correct,sub,del,ins,per\n'
                   'u1-pred.phn,8,8,6,1,1,1,0.375000\n'
                   'u2.phn,2,0,0,0,2,0,1.000000\n'
                   'u3.phn,0,2,0,0,0,2,nan\n')
    assert per == O.per_text([('u1-pred.phn', c1), ('u2.phn', c2), ('u3.phn', (0, 0, 0, 2))])
    assert solver.per_row('u1.phn', c1, (2, 3)) == 'u1.phn,8,8,6,1,1,1,0.375000,0.250000,3'
    assert solver.per_row('u3.phn', (0, 0, 0, 2), (2, 0)) == 'u3.phn,0,2,0,0,0,2,nan,nan,0'
    assert solver.PER_NBEST_HEADER + '\n' + solver.per_row('u1.phn', c1, (2, 3)) + '\n' == O.per_text([('u1.phn', c1, 2, 3)], nbest=True)
    text = solver.format_confusions(conf, VOCAB)
    assert text == ('ref,hyp,count\n'
                    'AA,<del>,2\n'
                    'B,<del>,1\n'
                    'D,CH,1\n'
                    '<ins>,D,1\n')
    assert text == O.confusions_text(conf, VOCAB)
    assert solver.format_confusions(conf) == 'ref,hyp,count\n3,<del>,2\n4,<del>,1\n6,5,1\n<ins>,6,1\n' == O.confusions_text(conf)
    text = solver.format_phones(conf, VOCAB)
    assert text == ('phone,ref_count,correct,sub,del,ins_as_hyp\n'
                    'AA,4,2,0,2,0\n'
                    'B,2,1,0,1,0\n'
                    'CH,2,2,0,0,0\n'
                    'D,2,1,1,0,1\n')
    assert text == O.phones_text(conf, VOCAB) and solver.format_phones(conf) == O.phones_text(conf)
    text = solver.format_ops(np.asarray(p1, np.int32), VOCAB)
    assert text == ('REF: AA B CH D  AA B * CH D\n'
                    'HYP: AA * CH CH AA B D CH D\n'
                    'OP:  C  D C  S  C  C I C  C\n')
    assert text == O.ops_text(p1, VOCAB)
    assert solver.format_ops(np.zeros((0, 2), np.int32)) == 'REF:\nHYP:\nOP:\n' == O.ops_text([])
    assert solver.format_ops(np.asarray(p2, np.int32)) == 'REF: 3 3\nHYP: * *\nOP:  D D\n' == O.ops_text(p2)
    # identical sides: a diagonal matrix and an empty body
    d = np.diag([0, 0, 0, 4, 1, 1, 1, 0])
    assert solver.format_confusions(d, VOCAB) == 'ref,hyp,count\n'
    assert solver.format_phones(d, VOCAB) == 'phone,ref_count,correct,sub,del,ins_as_hyp\nAA,4,4,0,0,0\nB,1,1,0,0,0\nCH,1,1,0,0,0\nD,1,1,0,0,0\n'


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']
_SC = ['--score-phn-dir', 'hyp', '--score-ref-dir', 'ref']


def test_score_flags_parse():
    entry = _entry()
    p = entry.parse_args(_SC + ['--score-nbest', '--score-ali', '--score-ignore', '0,1,2,42', '--vocab', 'v', '--batch-size', '4'])
    assert (p.score_phn_dir, p.score_ref_dir, p.score_nbest, p.score_ali, p.score_ignore, p.vocab, p.batch_size) == \
        ('hyp', 'ref', True, True, (0, 1, 2, 42), 'v', 4)
    p = entry.parse_args(_SC)                                               # no --config is needed
    assert p.score_ignore == (0, 1, 2) and p.score_nbest is False and p.score_ali is False and p.config is None
    assert entry.parse_args(_SC + ['--score-ignore', ''])                   .score_ignore == ()
    p = entry.parse_args(CFG)
    assert p.score_phn_dir is None and p.score_ref_dir is None and p.score_ignore is None
    assert 'cal_per' in entry.parser.format_help()


_NO_COMBINE = '--score-phn-dir does not combine with --'
_BELONG = '--score-ref-dir, --score-ignore, --score-nbest and --score-ali belong to --score-phn-dir'


@pytest.mark.parametrize('argv,msg', [
    (CFG + _SC + ['--gen-specgram'], _NO_COMBINE + 'gen-specgram'),
    (CFG + _SC + ['--tts-only'], _NO_COMBINE + 'tts-only'),
    (CFG + _SC + ['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
    (CFG + _SC + ['--corpus'], 'does not combine with --'),
    (CFG + _SC + ['--transcribe-wav-dir', 't'], _NO_COMBINE + 'transcribe-wav-dir'),
    (CFG + _SC + ['--align-wav-dir', 'a'], _NO_COMBINE + 'align-wav-dir'),
    (CFG + _SC + ['--vocode-dir', 'v'], _NO_COMBINE + 'vocode-dir'),
    (CFG + _SC + ['--feat-wav-dir', 'f', '--feat', 'mfcc'], _NO_COMBINE + 'feat-wav-dir'),
    (CFG + _SC + ['--mcd-wav-dir', 's', '--mcd-ref-dir', 'r'], _NO_COMBINE + 'mcd-wav-dir'),
    (CFG + _SC + ['--synth-phn-dir', 's'], _NO_COMBINE + 'synth-phn-dir'),
    (CFG + _SC + ['--trim-wav-dir', 's', '--trim-out', 'o'], _NO_COMBINE + 'trim-wav-dir'),
    (['--score-phn-dir', 'hyp'], '--score-phn-dir needs --score-ref-dir DIR'),
    (_SC + ['--score-ignore', '0,x'], '--score-ignore takes comma-separated integer ids'),
    (_SC + ['--score-ignore', '-1'], '--score-ignore takes at most 64 ids'),
    (_SC + ['--score-ignore', ','.join(str(i) for i in range(65))], '--score-ignore takes at most 64 ids'),
    (CFG + ['--score-ref-dir', 'ref'], _BELONG),
    (CFG + ['--score-nbest'], _BELONG),
    (CFG + ['--score-ali'], _BELONG),
    (CFG + ['--score-ignore', '0'], _BELONG),
    (CFG + ['--mcd-wav-dir', 's', '--mcd-ref-dir', 'r', '--score-ali'], _BELONG),
])
def test_score_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err
