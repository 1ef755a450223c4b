"""CPU checks of the LM-fused CTC beam search: the float64 oracle (tests/ctc_beam_lm_oracle.py) against brute force plus the prefix
bonus, the n-gram tables of semi_tts_amd/ngram.py, the argument checks of the ops layer (they fire before any device is touched), the
--lm / --build-lm-phn-dir parser rules and the table-building mode end to end."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import ctc_beam_oracle as O  # noqa: E402
import ctc_beam_lm_oracle as L  # noqa: E402

TINY = [(4, 3, 0, 2), (6, 3, 2, 3), (3, 4, 0, 3), (4, 4, 3, 2), (6, 2, 1, 1), (3, 4, 1, 4)]        # (T, V, blank, order)


def tiny_case(T, V, blank, order):
    """-> (log-probabilities (T, V) float64, fp32 bonus table (V^(order-1), V)) of one tiny problem"""
    rs = np.random.RandomState(100 * T + 10 * V + order)
    lp = np.log(rs.dirichlet(np.ones(V), T))
    bonus = (rs.randn(V ** (order - 1), V) * 1.5).astype(np.float32)
    return lp, bonus


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('T,V,blank,order', TINY)
def test_oracle_equals_brute_force_plus_prefix_bonus(T, V, blank, order):
    """a beam wide enough for every prefix: the fused score of a prefix is its exact CTC log-probability plus the bonuses of its
    symbols, whatever merges happened on the way"""
    lp, bonus = tiny_case(T, V, blank, order)
    bos = 1 if V > 1 else 0
    W = O.n_prefixes(T, V)
    hyps, scores, _ = L.beam_search(lp, W, W, bonus, blank, bos)
    want = sorted(((lab, sc + L.prefix_bonus(lab, bonus, bos)) for lab, sc in O.brute_force(lp, blank) if np.isfinite(sc)),
                  key=lambda x: -x[1])
    assert len(hyps) == W and len(set(hyps)) == W                       # every prefix once: exact merging
    got = [(h, s) for h, s in zip(hyps, scores) if np.isfinite(s)]      # (a labelling longer than the frames allow is -inf in both)
    assert [g[0] for g in got] == [w[0] for w in want]
    assert np.max(np.abs(np.array([g[1] for g in got]) - np.array([w[1] for w in want]))) <= 1e-9


def test_oracle_zero_table_is_the_acoustic_search_and_rows_follow_the_layout():
    rs = np.random.RandomState(0)
    lp = np.log(rs.dirichlet(np.ones(5), 12))
    for order in (1, 2, 3):
        zero = np.zeros((5 ** (order - 1), 5), np.float32)
        a, b = L.beam_search(lp, 4, 3, zero), O.beam_search(lp, 4, 3)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # start (0, bos), then the last two symbols: V = 5, order 3
    assert L.start_row(5, 3, 1) == 1 and L.next_row(1, 4, 5, 3) == 1 * 5 + 4 and L.next_row(9, 2, 5, 3) == 4 * 5 + 2
    assert L.start_row(5, 1, 1) == 0 and L.next_row(0, 3, 5, 1) == 0
    bonus = rs.randn(25, 5).astype(np.float32)
    assert abs(L.prefix_bonus((4, 2, 3), bonus) - (float(bonus[1, 4]) + float(bonus[9, 2]) + float(bonus[22, 3]))) < 1e-12


def test_oracle_forbidden_symbol():
    rs = np.random.RandomState(1)
    lp = np.log(rs.dirichlet(np.ones(4), 8))
    bonus = np.zeros((4, 4), np.float32)
    bonus[:, 2] = -np.inf
    hyps, scores, _ = L.beam_search(lp, 6, 6, bonus)
    assert all(2 not in h for h, s in zip(hyps, scores) if np.isfinite(s)) and np.isfinite(scores[0])


# ---------------------------------------------------------------- ngram.py
def test_count_and_table_against_a_hand_count():
    from semi_tts_amd import ngram
    V = 4
    seqs = [[2, 3, 2], [3, 3], []]
    c1 = ngram.count_ngrams(seqs, V, 1)
    assert c1.shape == (1, V) and c1.dtype == np.int64 and c1.tolist() == [[0, 0, 2, 3]]
    c2 = ngram.count_ngrams(seqs, V, 2)                          # contexts: bos = 1 first, then the previous symbol
    want = np.zeros((V, V), np.int64)
    want[1, 2], want[2, 3], want[3, 2], want[1, 3], want[3, 3] = 1, 1, 1, 1, 1
    assert np.array_equal(c2, want)
    c3 = ngram.count_ngrams(seqs, V, 3)                          # contexts: (0, 1), (1, 2), (2, 3); (0, 1), (1, 3)
    want = np.zeros((V * V, V), np.int64)
    want[0 * V + 1, 2], want[1 * V + 2, 3], want[2 * V + 3, 2], want[0 * V + 1, 3], want[1 * V + 3, 3] = 1, 1, 1, 1, 1
    assert np.array_equal(c3, want)
    assert ngram.count_ngrams([[2]], V, 2, bos=3)[3, 2] == 1
    t = ngram.ngram_table(c2, smooth=1.0, blank=0)
    assert t.dtype == np.float32 and t.shape == (V, V)
    np.testing.assert_allclose(t.sum(1), 1.0, atol=1e-6)
    assert np.all(t[:, 0] == 0.0)
    np.testing.assert_allclose(t[1], [0, 1 / 5, 2 / 5, 2 / 5], atol=1e-7)         # counts (., 0, 1, 1) + 1 over the non-blank columns
    np.testing.assert_allclose(t[0], [0, 1 / 3, 1 / 3, 1 / 3], atol=1e-7)         # never seen: uniform
    t0 = ngram.ngram_table(c2, smooth=0.0, blank=0)
    np.testing.assert_allclose(t0[0], [0, 1 / 3, 1 / 3, 1 / 3], atol=1e-7)        # ... without smoothing too
    np.testing.assert_allclose(t0[3], [0, 0, 0.5, 0.5], atol=1e-7)
    tb = ngram.ngram_table(c2, smooth=1.0, blank=3)
    assert np.all(tb[:, 3] == 0.0) and abs(tb[2].sum() - 1.0) < 1e-6
    for bad in (dict(V=1, order=2), dict(V=4, order=0), dict(V=4, order=5), dict(V=1024, order=3)):
        with pytest.raises(ValueError, match='order'):
            ngram.count_ngrams(seqs, **bad)
    with pytest.raises(ValueError, match='id 4'):
        ngram.count_ngrams([[4]], V, 2)
    with pytest.raises(ValueError, match='bos'):
        ngram.count_ngrams(seqs, V, 2, bos=4)
    with pytest.raises(ValueError, match='shape'):
        ngram.ngram_table(np.zeros((3, 4)))


def test_save_load_round_trip_and_row_index(tmp_path):
    from semi_tts_amd import ngram
    rs = np.random.RandomState(2)
    V = 5
    for order in (1, 2, 3, 4):
        table = rs.dirichlet(np.ones(V), V ** (order - 1)).astype(np.float32)
        p = str(tmp_path / ('t%d.npy' % order))
        ngram.save_table(p, table)
        assert os.path.exists(p)                                               # exactly at the path: no suffix appended
        raw = np.load(p)                                                       # what the reference's NgramPrior does
        assert raw.dtype == np.float32 and np.array_equal(raw, table)
        back = ngram.load_table(p)
        assert back.dtype == np.float32 and np.array_equal(back, table) and ngram.table_order(back.shape) == order
        for _ in range(5):
            ctx = rs.randint(0, V, order - 1).tolist()
            assert ngram.context_row(ctx, V) == sum(ctx[i] * V ** (order - 2 - i) for i in range(order - 1))
    # the start context (0, ..., 0, bos) is row bos, and counting walks the rows the same way
    assert ngram.context_row([0, 0, 1], V) == 1 and ngram.context_row([], V) == 0
    c = ngram.count_ngrams([[3, 4, 2, 3]], V, 4)
    for ctx, nxt in (([0, 0, 1], 3), ([0, 1, 3], 4), ([1, 3, 4], 2), ([3, 4, 2], 3)):
        assert c[ngram.context_row(ctx, V), nxt] == 1
    assert c.sum() == 4
    # a unigram stored as a vector (the reference's unigram file) and a float64 table load too; other shapes do not
    np.save(str(tmp_path / 'u.npy'), np.full(V, 0.2))
    assert ngram.load_table(str(tmp_path / 'u.npy')).shape == (1, V)
    np.save(str(tmp_path / 'bad.npy'), np.zeros((7, V)))
    with pytest.raises(ValueError, match=r'bad\.npy'):
        ngram.load_table(str(tmp_path / 'bad.npy'))
    with pytest.raises(ValueError, match=r'missing\.npy'):
        ngram.load_table(str(tmp_path / 'missing.npy'))
    with pytest.raises(ValueError, match='shape'):
        ngram.save_table(str(tmp_path / 'x.npy'), np.zeros((7, V)))


def test_fusion_table_values_and_refusals():
    from semi_tts_amd import ngram
    rs = np.random.RandomState(3)
    table = rs.dirichlet(np.ones(6), 6).astype(np.float32)
    table[:, 0] = 0.0
    f = ngram.fusion_table(table, 0.8, 0.3)
    assert f.dtype == np.float32 and f.flags['C_CONTIGUOUS'] and f.shape == table.shape
    want = (0.8 * np.log(table.astype(np.float64) + 1e-10) + 0.3).astype(np.float32)
    assert np.array_equal(f, want)
    assert ngram.EPS == 1e-10
    assert np.all(ngram.fusion_table(table, 0.0, 0.0) == 0.0)
    z = ngram.fusion_table(table, 1.0, 0.0, eps=0.0)                             # a zero probability without eps: forbidden
    assert np.all(np.isneginf(z[:, 0])) and np.all(np.isfinite(z[:, 1:]))
    bad = table.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match='finite probabilities'):
        ngram.fusion_table(bad, 0.5, 0.0)
    bad[2, 3] = -0.1
    with pytest.raises(ValueError, match='finite probabilities'):
        ngram.fusion_table(bad, 0.5, 0.0)
    bad[2, 3] = np.inf
    with pytest.raises(ValueError, match='finite probabilities'):
        ngram.fusion_table(bad, 0.5, 0.0)
    for w, b in ((np.nan, 0.0), (np.inf, 0.0), (0.5, np.nan), (0.5, -np.inf)):
        with pytest.raises(ValueError, match='finite'):
            ngram.fusion_table(table, w, b)
    with pytest.raises(ValueError, match=r'\+inf'):
        ngram.fusion_table(table, -1.0, 0.0, eps=0.0)
    with pytest.raises(ValueError, match='shape'):
        ngram.fusion_table(np.zeros((5, 6)), 0.5, 0.0)


# ---------------------------------------------------------------- ops argument checks
def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def _cuda_view(t):
    # the ops checks read .is_cuda / .device / .shape / .dtype only: a meta tensor stands in for a device tensor on the CPU
    return t.to('meta')


def test_bonus_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops, ctc_decode
    _no_device(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    good = _cuda_view(torch.rand(2, 5, 4))
    b2 = _cuda_view(torch.zeros(4, 4))
    cases = [
        (dict(bonus=torch.zeros(4, 4)), 'bonus must be'),                        # on the CPU
        (dict(bonus=np.zeros((4, 4), np.float32)), 'bonus must be'),
        (dict(bonus=_cuda_view(torch.zeros(4, 4, dtype=torch.float64))), 'bonus must be'),
        (dict(bonus=_cuda_view(torch.zeros(16))), 'bonus must be'),
        (dict(bonus=_cuda_view(torch.zeros(4, 8))[:, ::2]), 'contiguous'),
        (dict(bonus=_cuda_view(torch.zeros(5, 4))), r'no \(V\^\(order-1\), V\) table'),     # 5 rows: no power of 4
        (dict(bonus=_cuda_view(torch.zeros(4, 5))), r'no \(V\^\(order-1\), V\) table'),     # the width of another vocabulary
        (dict(bonus=_cuda_view(torch.zeros(4 ** 4, 4))), r'no \(V\^\(order-1\), V\) table'),   # order 5
        (dict(bonus=b2, order=3), 'has order 2'),
        (dict(bonus=b2, bos=4), 'bos'),
        (dict(bonus=b2, bos=-1), 'bos'),
        (dict(order=2), 'without a bonus'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.ctc_beam_search(good, **kw)
    wide = _cuda_view(torch.rand(1, 3, 1024))
    with pytest.raises(ValueError, match=r'2\^26'):
        ops.ctc_beam_search(wide, bonus=_cuda_view(torch.zeros(1024 * 1024, 1024)))        # V^3 = 2^30 elements
    with pytest.raises(ValueError, match='one of them'):
        ctc_decode.beam_search(good, lm=np.zeros((4, 4), np.float32), bonus=b2)
    # what the kernel takes gets as far as the library (and no further here): every order, the order given or inferred
    for order in (1, 2, 3, 4):
        for given in (None, order):
            with pytest.raises(AssertionError, match='reached the device'):
                ops.ctc_beam_search(good, bonus=_cuda_view(torch.zeros(4 ** (order - 1), 4)), order=given, bos=3)
    with pytest.raises(AssertionError, match='reached the device'):
        ctc_decode.beam_search(good, bonus=b2)
    from semi_tts_amd import ngram
    assert [ngram.order_of(r, 43) for r in (1, 43, 43 ** 2, 43 ** 3, 43 ** 4, 44)] == [1, 2, 3, 4, None, None]
    assert (ops.CB_MAX_ORDER, ops.CB_MAX_TABLE) == (ngram.MAX_ORDER, ngram.MAX_TABLE) == (4, 1 << 26)


def test_lm_tables_are_refused_on_the_host(monkeypatch):
    """beam_search(lm=...) builds the fused table on the host first: a bad table or one of another width raises before any kernel"""
    from semi_tts_amd import ctc_decode
    _no_device(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    good = _cuda_view(torch.rand(2, 5, 4))
    bad = np.full((4, 4), 0.25, np.float32)
    bad[1, 1] = np.nan
    with pytest.raises(ValueError, match='finite probabilities'):
        ctc_decode.beam_search(good, lm=bad)
    with pytest.raises(ValueError, match='5 classes, the posteriors 4'):
        ctc_decode.beam_search(good, lm=np.full((5, 5), 0.2, np.float32))
    with pytest.raises(ValueError, match='finite'):
        ctc_decode.beam_search(good, lm=np.full((4, 4), 0.25, np.float32), lm_weight=float('nan'))
    with pytest.raises(ValueError, match='must be a numpy array'):
        ctc_decode.beam_search(good, lm=[[0.5, 0.5], [0.5, 0.5]])
    with pytest.raises(ValueError, match=r'nowhere\.npy'):
        ctc_decode.beam_search(good, lm='/nonexistent/nowhere.npy')


def test_transcribe_and_beam_per_sum_take_the_lm_keywords():
    import inspect
    from semi_tts_amd.vqvae import VQVAE
    from semi_tts_amd import metrics, ctc_decode, ops
    for fn in (VQVAE.transcribe, metrics.beam_per_sum, ctc_decode.beam_search):
        p = inspect.signature(fn).parameters
        assert (p['lm'].default, p['lm_weight'].default, p['ins_bonus'].default) == (None, 0.5, 0.0), fn
    p = inspect.signature(ops.ctc_beam_search).parameters
    assert (p['bonus'].default, p['order'].default, p['bos'].default) == (None, None, 1)
    assert inspect.signature(ctc_decode.beam_search).parameters['bos'].default == 1


# ---------------------------------------------------------------- the header and the library
def test_header_declares_and_library_exports_the_entry_point():
    from semi_tts_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    m = re.search(r'int st_ctc_beam_search_lm\(([^;]*)\);', hdr)
    assert m, 'st_ctc_beam_search_lm is not declared'
    args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    names = [a.split()[-1].lstrip('*') for a in args.split(',')]
    assert names == ['prob', 'B', 'T', 'V', 'lengths', 'W', 'N', 'blank', 'log_input', 'eps', 'bonus', 'order', 'bos', 'hyp', 'hyp_len',
                     'score', 'ws', 'stream']
    assert len(_lib.SIGNATURES['st_ctc_beam_search_lm']) == len(names)
    assert 'st_ctc_beam_search_lm' in _lib.check_header_symbols()              # exported by the built library, bound by ctypes
    for word in ('-inf', 'NaN', 'bos', '2^26', 'never read'):
        assert word in hdr[hdr.index('st_ctc_beam_search_lm'):m.end()], word


# ---------------------------------------------------------------- main.py flags
def _entry():
    import main as entry
    return entry


CFG = ['--config', 'config/semi-single-spkr-paired-data.yaml']


def test_lm_flags_parse_and_default():
    entry = _entry()
    p = entry.parse_args(CFG + ['--transcribe-wav-dir', 'wavs', '--lm', 'phn.npy', '--lm-weight', '0.8', '--ins-bonus', '-0.25'])
    assert (p.lm, p.lm_weight, p.ins_bonus, p.build_lm_phn_dir) == ('phn.npy', 0.8, -0.25, None)
    p = entry.parse_args(CFG + ['--transcribe-wav-dir', 'wavs', '--lm', 'phn.npy'])
    assert (p.lm, p.lm_weight, p.ins_bonus) == ('phn.npy', 0.5, 0.0)
    p = entry.parse_args(CFG + ['--transcribe-wav-dir', 'wavs'])
    assert (p.lm, p.lm_weight, p.ins_bonus, p.lm_order, p.lm_smooth, p.build_lm_phn_dir) == (None, 0.5, 0.0, None, 1.0, None)
    p = entry.parse_args(CFG)
    assert p.lm is None and p.build_lm_phn_dir is None
    p = entry.parse_args(['--build-lm-phn-dir', 'phn', '--lm-order', '3', '--lm', 'out.npy', '--lm-smooth', '0.5', '--vocab', 'v'])
    assert (p.build_lm_phn_dir, p.lm_order, p.lm, p.lm_smooth, p.vocab) == ('phn', 3, 'out.npy', 0.5, 'v')
    p = entry.parse_args(['--build-lm-phn-dir', 'phn', '--lm-order', '1', '--lm', 'out.npy'])
    assert p.lm_smooth == 1.0


_BUILD = ['--build-lm-phn-dir', 'phn', '--lm-order', '2', '--lm', 'out.npy']
_NO_COMBINE = '--build-lm-phn-dir does not combine with --'


@pytest.mark.parametrize('argv,msg', [
    (CFG + ['--lm', 'phn.npy'], '--lm names the n-gram table of --transcribe-wav-dir or --build-lm-phn-dir'),
    (CFG + ['--align-wav-dir', 'wavs', '--lm', 'phn.npy'], '--lm names the n-gram table'),
    (CFG + ['--gen-specgram', '--lm', 'phn.npy'], '--lm names the n-gram table'),
    (CFG + ['--transcribe-wav-dir', 'wavs', '--lm-weight', '0.5'], '--lm-weight and --ins-bonus weight the table of --lm'),
    (CFG + ['--transcribe-wav-dir', 'wavs', '--ins-bonus', '0.5'], '--lm-weight and --ins-bonus weight the table of --lm'),
    (CFG + ['--transcribe-wav-dir', 'wavs', '--lm', 'f', '--lm-weight', 'nan'], '--lm-weight must be finite'),
    (CFG + ['--transcribe-wav-dir', 'wavs', '--lm', 'f', '--ins-bonus', 'inf'], '--ins-bonus must be finite'),
    (CFG + ['--transcribe-wav-dir', 'wavs', '--lm', 'f', '--lm-order', '2'], '--lm-order and --lm-smooth belong to --build-lm-phn-dir'),
    (CFG + ['--lm-smooth', '2'], '--lm-order and --lm-smooth belong to --build-lm-phn-dir'),
    (['--build-lm-phn-dir', 'phn', '--lm-order', '2'], '--build-lm-phn-dir needs --lm FILE'),
    (['--build-lm-phn-dir', 'phn', '--lm', 'out.npy'], '--build-lm-phn-dir needs --lm FILE'),
    (['--build-lm-phn-dir', 'phn', '--lm', 'out.npy', '--lm-order', '0'], '1 <= --lm-order <= 4'),
    (['--build-lm-phn-dir', 'phn', '--lm', 'out.npy', '--lm-order', '5'], '1 <= --lm-order <= 4'),
    (_BUILD + ['--lm-smooth', '-1'], '--lm-smooth must be finite and >= 0'),
    (_BUILD + ['--lm-smooth', 'nan'], '--lm-smooth must be finite and >= 0'),
    (_BUILD + ['--lm-weight', '0.5'], '--lm-weight and --ins-bonus belong to --transcribe-wav-dir'),
    (_BUILD + ['--transcribe-wav-dir', 'w'], _NO_COMBINE + 'transcribe-wav-dir'),
    (_BUILD + ['--align-wav-dir', 'w'], _NO_COMBINE + 'align-wav-dir'),
    (_BUILD + ['--gen-specgram'], _NO_COMBINE + 'gen-specgram'),
    (_BUILD + ['--tts-only'], _NO_COMBINE + 'tts-only'),
    (_BUILD + ['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
    (_BUILD + ['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
])
def test_lm_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


# ---------------------------------------------------------------- --build-lm-phn-dir end to end
def test_build_lm_phn_dir_end_to_end(tmp_path, capsys, monkeypatch):
    """reads every .phn with ctc_align.read_phn (score<TAB>tokens lines and bare ones, symbols and ids), skips id 0, writes the table
    and one summary line -- with every CUDA entry of torch poisoned: the mode never touches the GPU"""
    from semi_tts_amd import ngram
    from semi_tts_amd.solver import format_phn, SPECIAL_TOKENS
    entry = _entry()

    def poisoned(*a, **k):
        raise AssertionError('touched the GPU')
    for name in ('is_available', 'manual_seed_all', 'current_device', 'device_count', 'set_device'):
        monkeypatch.setattr(torch.cuda, name, poisoned)
    phones = ['AA', 'AE', 'AH', 'B']
    vocab = tmp_path / 'phn.vocab'
    vocab.write_text('\n'.join(phones) + '\n')
    voc = list(SPECIAL_TOKENS) + phones
    d = tmp_path / 'phn'
    d.mkdir()
    (d / 'b.phn').write_text(format_phn([-3.5, -4.0], [[3, 0, 4, 3], [5]], voc))    # the best path only; the <pad> is skipped
    (d / 'a.phn').write_text('AH 6 AH\n')                                          # a bare line, an id among symbols
    (d / 'c.phn').write_text('\n')                                                 # an empty transcript
    (d / 'notes.txt').write_text('ZZ\n')                                           # not a transcript
    seqs = [[5, 6, 5], [3, 4, 3], []]
    out = tmp_path / 'lm' / 'phn.2gram.npy'
    out.parent.mkdir()
    entry.main(['--build-lm-phn-dir', str(d), '--lm-order', '2', '--lm', str(out), '--vocab', str(vocab), '--lm-smooth', '0.5'])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and '2-gram' in lines[0] and '3 .phn files' in lines[0] and '6 tokens' in lines[0] and str(out) in lines[0]
    table = ngram.load_table(str(out))
    assert table.shape == (43, 43)
    assert np.array_equal(table, ngram.ngram_table(ngram.count_ngrams(seqs, 43, 2), 0.5))
    np.testing.assert_allclose(table.sum(1), 1.0, atol=1e-5)
    assert np.all(table[:, 0] == 0.0) and table[5, 6] > table[5, 7] and table[1, 5] == table[1, 3] > table[1, 4]
    # order 3 without a vocabulary: ids only; an unknown symbol or an id outside the classes stops the run before anything is written
    for f in ('a.phn', 'b.phn'):
        (d / f).unlink()
    (d / 'd.phn').write_text('7 8 7 8\n')
    out3 = tmp_path / 'lm' / 'phn.3gram.npy'
    entry.main(['--build-lm-phn-dir', str(d), '--lm-order', '3', '--lm', str(out3)])
    t3 = ngram.load_table(str(out3))
    assert t3.shape == (43 * 43, 43) and np.argmax(t3[7 * 43 + 8]) == 7 and np.argmax(t3[0 * 43 + 1]) == 7
    (d / 'e.phn').write_text('7 43\n')
    out4 = tmp_path / 'lm' / 'never.npy'
    with pytest.raises(ValueError, match=r'e\.phn.*43'):
        entry.main(['--build-lm-phn-dir', str(d), '--lm-order', '1', '--lm', str(out4)])
    (d / 'e.phn').write_text('AA\n')
    with pytest.raises(ValueError, match=r'e\.phn.*AA'):
        entry.main(['--build-lm-phn-dir', str(d), '--lm-order', '1', '--lm', str(out4)])
    assert not out4.exists()
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match='no .phn files'):
        entry.main(['--build-lm-phn-dir', str(empty), '--lm-order', '1', '--lm', str(out4)])


def test_transcriber_refuses_a_table_of_another_width_in_load_data(tmp_path, monkeypatch):
    """Transcriber.load_data reads --lm and compares its width with the searched posteriors' (no GPU needed: the constructor is bypassed)"""
    from semi_tts_amd import solver, audio, ngram

    class Conv:
        n_mels = 80
    monkeypatch.setattr(audio, 'load_audio_transform', lambda **kw: Conv())
    (tmp_path / 'a.wav').write_bytes(b'')
    ngram.save_table(str(tmp_path / 'v43.npy'), np.full((43, 43), 1 / 43, np.float32))
    ngram.save_table(str(tmp_path / 'v64.npy'), np.full((1, 64), 1 / 64, np.float32))
    tr = solver.Transcriber.__new__(solver.Transcriber)
    tr.config = {'data': {'audio': {}}, 'model': {'codebook': {'latent_dim': 64}}}
    tr.n_mels, tr.vocab_size = 80, 43

    class P:
        transcribe_wav_dir = str(tmp_path)
        vocab = None
        asr_output = 'code'
        lm = str(tmp_path / 'v43.npy')
    tr.paras = P()
    tr.load_data()
    assert tr.lm.shape == (43, 43)
    P.lm = str(tmp_path / 'v64.npy')
    with pytest.raises(ValueError, match=r'v64\.npy.*64 classes.*43'):
        tr.load_data()
    P.asr_output = 'post'                                    # the ASR postnet has latent_dim classes
    tr.load_data()
    assert tr.lm.shape == (1, 64)
    P.lm = str(tmp_path / 'v43.npy')
    with pytest.raises(ValueError, match=r'v43\.npy.*43 classes.*64'):
        tr.load_data()
    P.lm = None
    tr.load_data()
    assert tr.lm is None
