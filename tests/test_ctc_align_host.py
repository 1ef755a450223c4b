"""CPU checks of the CTC forced aligner: the numpy oracle against brute force, the .phn / .ali / segments.csv helpers, the argument checks
of the ops layer (they fire before any device is touched) and the --align-wav-dir parser rules."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import ctc_align_oracle as O  # noqa: E402


def _all_targets(V, blank, max_len):
    syms = [v for v in range(V) if v != blank]
    for S in range(max_len + 1):
        for y in itertools.product(syms, repeat=S):
            yield list(y)


@pytest.mark.parametrize('T,blank,seed', [(0, 0, 9), (1, 0, 0), (2, 1, 1), (3, 0, 2), (4, 2, 3), (5, 0, 4), (6, 1, 5), (6, 0, 6)])
def test_oracle_equals_brute_force(T, blank, seed):
    """every target of length 0 .. 3 over V = 3 (repeated tokens and infeasible lengths among them): the Viterbi score is the best
    score of any label sequence collapsing to the targets, the path is that sequence wherever it is unique, and the spans are its"""
    V = 3
    lp = np.log(O.softmax(np.random.RandomState(seed).randn(T, V) * 2.0).astype(np.float64))
    for tg in _all_targets(V, blank, 3):
        bf = O.brute_force(lp, tg, blank)
        for dtype in (np.float64, np.float32):
            score, states, labels, ts, te = O.align(lp, tg, blank, dtype)
            if not bf:
                assert T < len(tg) + O.n_repeats(tg)
                assert score == -np.inf and np.all(labels == -1) and np.all(ts == -1) and np.all(te == -1)
                continue
            assert abs(score - bf[0][1]) <= (1e-12 if dtype is np.float64 else 1e-5), (tg, dtype)
            assert O.is_alignment(labels, tg, blank)
            assert abs(O.path_score(lp, labels) - bf[0][1]) <= (1e-12 if dtype is np.float64 else 1e-5)
            if len(bf) == 1 or bf[0][1] - bf[1][1] > 1e-4:
                assert tuple(labels.tolist()) == bf[0][0], (tg, dtype)
            for k in range(len(tg)):
                fr = [t for t in range(T) if states[t] == 2 * k + 1]
                assert fr == list(range(ts[k], te[k])) and fr and all(labels[t] == tg[k] for t in fr)
            assert score <= O.forward_loglik(lp, tg, blank) + 1e-5


def test_oracle_ties_and_refusals():
    # all log-probabilities equal: the end prefers n - 1 and the stay wins every tie on the way back, so the path found reaches the last
    # state as early as the trellis allows (the skip from y0 to y1 included) and stays there
    lp = np.full((6, 3), np.log(1.0 / 3.0))
    score, states, labels, ts, te = O.align(lp, [1, 2], 0)
    assert states.tolist() == [1, 3, 4, 4, 4, 4] and labels.tolist() == [1, 2, 0, 0, 0, 0]
    assert (ts.tolist(), te.tolist()) == ([0, 1], [1, 2]) and abs(score - 6 * np.log(1 / 3)) < 1e-12
    assert O.align(lp, [1, 1], 0)[1].tolist() == [1, 2, 3, 4, 4, 4]                     # the blank between equal targets is kept
    assert O.align(lp[:3], [1, 1], 0)[1].tolist() == [1, 2, 3]                          # length == S + repeats: the one feasible path
    assert O.align(lp[:2], [1, 1], 0)[0] == -np.inf
    assert np.isnan(O.align(lp, [1, 3], 0)[0]) and np.isnan(O.align(lp, [-1], 0)[0])    # a target outside [0, V)
    bad = lp.copy()
    bad[2, 2] = np.nan
    assert np.isnan(O.align(bad, [1, 2], 0)[0]) and np.isfinite(O.align(bad, [1], 0)[0])   # only the columns of ext count
    sc = O.align(lp, [], 0)
    assert abs(sc[0] - 6 * np.log(1 / 3)) < 1e-12 and sc[2].tolist() == [0] * 6
    assert O.align(lp[:0], [], 0)[0] == 0.0 and O.align(lp[:0], [1], 0)[0] == -np.inf
    assert O.targets_of([3, 0, 4, 4, 0, 5], 5, 0) == [3, 4, 4] and O.targets_of([3, 0, 4], None, 3) == [0, 4]


def test_generator_places_every_target():
    rs = np.random.RandomState(0)
    prob, text, tl = O.peaked(rs, 8, 40, 7, 0.3, 12)
    assert prob.shape == (8, 40, 7) and prob.dtype == np.float32 and np.all(tl >= 1) and np.all(tl <= 12)
    for b in range(8):
        tg = O.targets_of(text[b], tl[b])
        assert len(tg) == tl[b]
        assert O.collapse(prob[b].argmax(-1)) == tg              # at temperature 0.3 the peaks are the argmax


# ---------------------------------------------------------------- .phn / .ali / segments.csv
def test_read_phn_round_trip_and_errors(tmp_path):
    from semi_tts_amd.solver import format_phn
    from semi_tts_amd.ctc_align import read_phn
    vocab = ['<pad>', '<space>', '<eos>', 'AA', 'AE', 'AH']
    for voc in (vocab, None):
        for ids in ([3, 5, 3, 1], [4, 9, 60], []):
            p = tmp_path / 'a.phn'
            p.write_text(format_phn([-1.5, -2.0], [ids, [3]], voc))             # the best path is the first line
            assert read_phn(str(p), voc) == ids
    p = tmp_path / 'b.phn'
    p.write_text('\n\nAA  AH 7\nAE\n')                                          # no score column; the first non-empty line
    assert read_phn(str(p), vocab) == [3, 5, 7]
    p.write_text('x\ty\tAE AE\n')
    assert read_phn(str(p), vocab) == [4, 4]                                    # what follows the LAST tab
    p.write_text('')
    assert read_phn(str(p), vocab) == []
    p.write_text('-inf\t\n')
    assert read_phn(str(p), None) == []
    p.write_text('AA ZZ\n')
    with pytest.raises(ValueError, match=r'b\.phn.*ZZ'):
        read_phn(str(p), vocab)
    with pytest.raises(ValueError, match=r'b\.phn.*AA'):
        read_phn(str(p), None)                                                  # symbols need a vocabulary
    p.write_text('-3\n')
    with pytest.raises(ValueError, match=r'b\.phn'):
        read_phn(str(p), vocab)
    p.write_text(' '.join(['3'] * 1025) + '\n')
    with pytest.raises(ValueError, match=r'b\.phn.*1025'):
        read_phn(str(p), vocab)
    p.write_text(' '.join(['3'] * 1024) + '\n')
    assert len(read_phn(str(p), vocab)) == 1024
    with pytest.raises(ValueError, match=r'missing\.phn'):
        read_phn(str(tmp_path / 'missing.phn'), vocab)
    with pytest.raises(ValueError, match=str(tmp_path.name)):
        read_phn(str(tmp_path), vocab)                                          # a directory: unreadable


def test_format_ali_and_segment_row():
    from semi_tts_amd.ctc_align import format_ali, segment_row, segment_key, SEGMENTS_HEADER
    vocab = ['<pad>', '<space>', '<eos>', 'AA', 'AE', 'AH']
    frame_s = 2 * 256 / 22050
    txt = format_ali(-12.3456789, 20, frame_s, [3, 5, 77], [2, 7, 11], [5, 9, 18], vocab)
    want = ['# score=-12.345679 frames=20 frame_s=0.023220',
            'AA\t2\t5\t%.6f\t%.6f' % (2 * frame_s, 5 * frame_s),
            'AH\t7\t9\t%.6f\t%.6f' % (7 * frame_s, 9 * frame_s),
            '77\t11\t18\t%.6f\t%.6f' % (11 * frame_s, 18 * frame_s)]
    assert txt == '\n'.join(want) + '\n'
    assert format_ali(-1.0, 4, 0.5, [4], [1], [3], None) == '# score=-1.000000 frames=4 frame_s=0.500000\n4\t1\t3\t0.500000\t1.500000\n'
    assert format_ali(float('-inf'), 3, 0.5, [3, 3, 3, 3], [-1] * 4, [-1] * 4, vocab) == '# score=-inf frames=3 frame_s=0.500000\n'
    assert format_ali(float('nan'), 3, 0.5, [3], [-1], [-1], vocab) == '# score=nan frames=3 frame_s=0.500000\n'
    assert format_ali(-2.0, 3, 0.5, [], [], [], vocab) == '# score=-2.000000 frames=3 frame_s=0.500000\n'
    assert segment_key('dir/p225_001.mic1.wav') == 'p225_001' and SEGMENTS_HEADER == 'file,seg'
    row = segment_row('u3.wav', [2, 7, 11], 20, frame_s)
    assert row == 'u3,%.4f_%.4f_%.4f' % (7 * frame_s, 11 * frame_s, 20 * frame_s)
    assert segment_row('u4.wav', [5], 20, 0.5) == 'u4,10.0000' and segment_row('u5.wav', [], 20, 0.5) is None
    # read back by the reference's rule (src/audio.py:425-432: boundaries as ratios of the last one): increasing, ending at 1
    key, seg = row.split(',')
    t = [float(x) for x in seg.split('_')]
    ratio = [x / t[-1] for x in t]
    assert ratio[-1] == 1.0 and all(a < b for a, b in zip(ratio[:-1], ratio[1:])) and len(ratio) == 3


def test_segments_csv_is_read_by_pandas_like_the_reference(tmp_path):
    pd = pytest.importorskip('pandas')
    from semi_tts_amd.ctc_align import segment_row, SEGMENTS_HEADER
    p = tmp_path / 'segments.csv'
    p.write_text('\n'.join([SEGMENTS_HEADER, segment_row('a.wav', [0, 3], 10, 0.1), segment_row('b.x.wav', [1], 4, 0.1)]) + '\n')
    table = pd.read_csv(str(p), index_col=0)
    assert list(table.index) == ['a', 'b'] and table.loc['a', 'seg'] == '0.3000_1.0000'


# ---------------------------------------------------------------- ops argument checks
def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def _cuda_view(t):
    # the ops checks read .is_cuda / .device / .shape / .dtype only: a meta tensor stands in for a device tensor on the CPU
    return t.to('meta')


def test_forced_align_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops
    _no_device(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    good = _cuda_view(torch.rand(2, 5, 4))
    text = _cuda_view(torch.zeros(2, 3, dtype=torch.int64))
    cases = [
        (dict(prob=torch.rand(2, 5, 4), text=text), 'GPU tensor'),                       # a CPU tensor
        (dict(prob=[[0.5]], text=text), 'GPU tensor'),
        (dict(prob=_cuda_view(torch.rand(2, 5, 4, dtype=torch.float64)), text=text), 'float32'),
        (dict(prob=_cuda_view(torch.rand(5, 4)), text=text), 'float32'),
        (dict(prob=good, text=torch.zeros(2, 3, dtype=torch.int64)), 'text must be'),   # text on the CPU
        (dict(prob=good, text=[[1, 2, 3]] * 2), 'text must be'),
        (dict(prob=good, text=_cuda_view(torch.zeros(2, 3, dtype=torch.int32))), 'int64'),
        (dict(prob=good, text=_cuda_view(torch.zeros(6, dtype=torch.int64))), 'int64'),
        (dict(prob=good, text=_cuda_view(torch.zeros(3, 3, dtype=torch.int64))), 'utterances'),
        (dict(prob=_cuda_view(torch.rand(0, 5, 4)), text=_cuda_view(torch.zeros(0, 3, dtype=torch.int64))), 'B=0'),
        (dict(prob=_cuda_view(torch.rand(1, 4097, 4)), text=text[:1]), 'T=4097'),
        (dict(prob=_cuda_view(torch.rand(1, 5, 1)), text=text[:1]), 'V=1'),
        (dict(prob=_cuda_view(torch.rand(1, 5, 10241)), text=text[:1]), 'V=10241'),
        (dict(prob=good, text=_cuda_view(torch.zeros(2, 1025, dtype=torch.int64))), 'L=1025'),
        (dict(prob=good, text=_cuda_view(torch.zeros(2, 0, dtype=torch.int64))), 'L=0'),
        (dict(prob=good, text=text, blank=4), 'blank'),
        (dict(prob=good, text=text, blank=-1), 'blank'),
        (dict(prob=good, text=text, eps=-1.0), 'eps'),
        (dict(prob=good, text=text, lengths=[1, 6]), 'lengths'),
        (dict(prob=good, text=text, lengths=[1, -1]), 'lengths'),
        (dict(prob=good, text=text, lengths=[1]), 'lengths'),
        (dict(prob=good, text=text, lengths=torch.tensor([1.0, 2.0])), 'lengths'),
        (dict(prob=good, text=text, lengths=_cuda_view(torch.tensor([1, 2, 3]))), 'lengths'),
        (dict(prob=good, text=text, text_lengths=[1, 4]), 'text_lengths'),
        (dict(prob=good, text=text, text_lengths=[-1, 2]), 'text_lengths'),
        (dict(prob=good, text=text, text_lengths=[1, 2, 3]), 'text_lengths'),
        (dict(prob=good, text=text, text_lengths=_cuda_view(torch.tensor([1.0, 2.0]))), 'text_lengths'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.ctc_forced_align(**kw)
    from semi_tts_amd import ctc_align
    with pytest.raises(ValueError, match='blank'):
        ctc_align.forced_align(good, text, blank=9)
    # arguments the kernel takes get as far as the library (and no further here)
    with pytest.raises(AssertionError, match='reached the device'):
        ops.ctc_forced_align(good, text, lengths=[5, 0], text_lengths=[3, 0], blank=3)


def test_align_refuses_a_missing_postnet_and_bad_sources():
    from semi_tts_amd.vqvae import VQVAE

    class Fake:
        use_asr_postnet = False
    with pytest.raises(ValueError, match="source must be"):
        VQVAE.align(Fake(), None, [4], None, source='logits')
    with pytest.raises(ValueError, match='needs an ASRPostnet'):
        VQVAE.align(Fake(), None, [4], None, source='post')


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/semi-single-spkr-paired-data.yaml']


def test_align_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + ['--align-wav-dir', 'wavs', '--phn-dir', 'phn', '--vocab', 'phn.vocab', '--asr-output', 'post',
                                '--batch-size', '4'])
    assert (p.align_wav_dir, p.phn_dir, p.vocab, p.asr_output, p.batch_size) == ('wavs', 'phn', 'phn.vocab', 'post', 4)
    p = entry.parse_args(CFG + ['--align-wav-dir', 'wavs'])
    assert (p.phn_dir, p.vocab, p.asr_output, p.transcribe_wav_dir) == (None, None, 'code', None)
    p = entry.parse_args(CFG)
    assert p.align_wav_dir is None and p.phn_dir is None


_NO_COMBINE = '--align-wav-dir does not combine with --'


@pytest.mark.parametrize('extra,msg', [(['--gen-specgram'], _NO_COMBINE + 'gen-specgram'), (['--tts-only'], _NO_COMBINE + 'tts-only'),
                                       (['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
                                       (['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
                                       (['--transcribe-wav-dir', 't'], _NO_COMBINE + 'transcribe-wav-dir'),
                                       (['--asr-output', 'logits'], "--asr-output: invalid choice: 'logits'")])
def test_align_flag_refusals(extra, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(CFG + ['--align-wav-dir', 'wavs'] + extra)
    assert msg in capsys.readouterr().err


@pytest.mark.parametrize('other', [[], ['--transcribe-wav-dir', 'wavs'], ['--gen-specgram']])
def test_phn_dir_needs_align_wav_dir(other, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(CFG + other + ['--phn-dir', 'phn'])
    assert '--phn-dir names the transcripts of --align-wav-dir' in capsys.readouterr().err


def test_aligner_reads_every_transcript_before_any_batch(tmp_path, monkeypatch):
    """Aligner.load_data names the file of a missing transcript (no GPU needed: the solver's constructor is bypassed)"""
    from semi_tts_amd import solver, audio

    class Conv:
        n_mels = 80
    monkeypatch.setattr(audio, 'load_audio_transform', lambda **kw: Conv())
    for f in ('b.wav', 'a.wav', 'c.WAV', 'notes.txt'):
        (tmp_path / f).write_bytes(b'')
    (tmp_path / 'a.phn').write_text('-1.0\t3 4\n')
    (tmp_path / 'c.phn').write_text('5\n')
    al = solver.Aligner.__new__(solver.Aligner)
    al.config = {'data': {'audio': {}}}
    al.n_mels = 80

    class P:
        align_wav_dir = str(tmp_path)
        phn_dir = None
        vocab = None
    al.paras = P()
    with pytest.raises(ValueError, match=r'b\.phn'):
        al.load_data()
    (tmp_path / 'b.phn').write_text('\n')
    al.load_data()
    assert al.files == ['a.wav', 'b.wav', 'c.WAV'] and al.transcripts == [[3, 4], [], [5]]
    other = tmp_path / 'phn'
    other.mkdir()
    P.phn_dir = str(other)
    with pytest.raises(ValueError, match=r'phn.a\.phn'):
        al.load_data()
