"""CPU checks of synthesis from phone transcripts: the numpy oracle of the end-of-speech kernel on hand-computed cases, the exported
symbol and its limit checks, the argument checks of ops.attn_endpoint (they fire before any device is touched), the --synth-phn-dir
parser rules, transcript validation, the decode-length formula and the layout of a synth.csv row."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import attn_endpoint_oracle as O  # noqa: E402


# ---------------------------------------------------------------- the oracle, by hand
def test_row_peak_rules():
    nan, inf = float('nan'), float('inf')
    assert O.row_peak([0.1, 0.7, 0.2]) == (1, 0.7)
    assert O.row_peak([0.4, 0.1, 0.4]) == (0, 0.4)                  # a tie: the lower column
    assert O.row_peak([nan, 0.1, nan, 0.3]) == (3, 0.3)             # NaN never wins
    assert O.row_peak([nan, nan]) == (0, 0.0)                       # no non-NaN entry
    assert O.row_peak([0.2, inf, inf]) == (1, inf)
    assert O.row_peak([-inf, nan]) == (0, -inf)                     # -inf is an entry
    assert O.row_peak([-0.0, 0.0]) == (0, 0.0)                      # equal values: the lower column
    assert O.row_peak([5.0]) == (0, 5.0)


def test_staircase_by_hand():
    """3 phones of 2, 1 and 2 steps, S = 8, K = 3: peaks 0 0 1 2 2 2 2 2, the flags (peak >= 2) start at step 3, end = 3 + 3 = 6"""
    a, cols = O.staircase([2, 1, 2], 8, 4)
    assert cols.tolist() == [0, 0, 1, 2, 2, 2, 2, 2]
    r = O.endpoint(a, 3, patience=3, max_jump=4)
    assert (r.end, r.reached, r.n_back, r.n_skip, r.covered, r.nonfinite) == (6, 1, 0, 0, 3, 0)
    assert r.peak.tolist() == cols.tolist() and r.dur.tolist() == [2, 1, 3, 0]
    assert abs(r.focus - 0.75) < 1e-7
    # patience 1: the first flagged step ends it; patience 5: steps 3 .. 7; patience 6: no run of 6 in 5 flagged steps
    assert O.endpoint(a, 3, 1).end == 4 and O.endpoint(a, 3, 5)[:2] == (8, 1) and O.endpoint(a, 3, 6)[:2] == (8, 0)
    assert O.endpoint(a, 3, 9)[:2] == (8, 0)                        # K > S
    # n = 1: every row flags, end = K; n = 4 (the peak never reaches column 3): not reached, counts over all 8 steps
    assert O.endpoint(a, 1, 3)[:2] == (3, 1) and O.endpoint(a, 1, 3).dur.tolist() == [2, 1, 0, 0]
    r = O.endpoint(a, 4, 3)
    assert (r.end, r.reached, r.covered) == (8, 0, 3) and r.dur.tolist() == [2, 1, 5, 0]


def test_defects_by_hand():
    L = 8
    cols = [0, 1, 2, 1, 2, 7, 7, 3, 7, 7, 7, 7]                     # back at t = 3 and t = 7; skips (> +4) at t = 5; broken run at t = 7
    a = O.from_peaks(cols, L)
    r = O.endpoint(a, 8, patience=3, max_jump=4)
    assert (r.end, r.reached, r.n_back, r.n_skip, r.covered) == (11, 1, 2, 1, 5)
    assert r.dur.tolist() == [1, 2, 2, 1, 0, 0, 0, 5]
    assert O.endpoint(a, 8, 3, max_jump=3).n_skip == 2              # 3 -> 7 at t = 8 is a jump of 4
    # a run of K - 1 flags that touches the last step is no detection
    assert O.endpoint(a[:10], 8, 3)[:2] == (10, 0) and O.endpoint(a[:11], 8, 3)[:2] == (11, 1)
    # the appended token and the padding take part: a peak past n - 1 flags too
    assert O.endpoint(O.from_peaks([0, 5, 6, 7], L), 2, 3)[:2] == (4, 1)
    # ties: the lower column wins, wherever the other one is
    t = O.with_tie(O.from_peaks([5, 5, 5], L), 1, 2)
    assert O.endpoint(t, 3, 1).peak.tolist() == [5, 2, 5]
    # non-finite entries: flagged, peaks defined
    b = a.copy()
    b[0, :] = np.nan
    b[1, 1] = np.nan
    b[2, 0] = np.inf
    r = O.endpoint(b, 8, 3)
    assert r.nonfinite == 1 and r.peak[:3].tolist() == [0, 0, 0] and r.focus == float('inf')
    rb = O.endpoint_batch(np.stack([a, b]), [8, 8])
    assert rb.end.tolist() == [11, 11] and rb.nonfinite.tolist() == [0, 1] and rb.peak.shape == (2, 12) and rb.dur.shape == (2, 8)


# ---------------------------------------------------------------- the library
def test_library_exports_the_entry_and_refuses_each_limit_without_a_device():
    """the limit checks precede the launch: -22 and a message naming the entry point, with pointers that are never dereferenced"""
    from semi_tts_amd import _lib, build
    assert 'attn_stats.hip' in build.SOURCES and len(build.SOURCES) == 20
    assert len(_lib.SIGNATURES['st_attn_endpoint']) == 14
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(B=1, S=4, L=4, K=3, J=4, a_sb=16, a_st=4, a=p, n=p):
        return lib.st_attn_endpoint(a, a_sb, a_st, n, B, S, L, K, J, p, p, p, p, None)
    for kw in (dict(B=0), dict(S=0), dict(S=4097), dict(L=0), dict(L=2049, a_st=2049), dict(a_st=3), dict(a_sb=-1), dict(K=0), dict(J=0),
               dict(a=None), dict(n=None)):
        assert call(**kw) == -22, kw
        assert b'st_attn_endpoint' in lib.st_last_error()


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import _lib, metrics, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)
    x = torch.rand(2, 5, 4)
    for a in (x, [[[1.0]]]):                                         # a CPU tensor, not a tensor
        with pytest.raises(ValueError, match='GPU tensor'):
            metrics.attention_endpoints(a, [1, 1])
    # the remaining checks read .is_cuda / .device / .shape / .dtype / .stride() only: a meta tensor stands in for a device tensor
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    m = x.to('meta')
    cases = [
        (dict(align=m.double(), enc_len=[1, 1]), 'float32'),
        (dict(align=m[0], enc_len=[1]), 'GPU tensor'),
        (dict(align=m[:0], enc_len=[]), 'B=0'),
        (dict(align=m[:, :0], enc_len=[1, 1]), 'S=0'),
        (dict(align=m[:, :, :0], enc_len=[1, 1]), 'L=0'),
        (dict(align=torch.empty(1, 4097, 2, device='meta'), enc_len=[1]), 'S=4097'),
        (dict(align=torch.empty(1, 2, 2049, device='meta'), enc_len=[1]), 'L=2049'),
        (dict(align=m.transpose(1, 2), enc_len=[1, 1]), 'strides'),                  # the last dimension is not contiguous
        (dict(align=m[:, :1].expand(2, 5, 4), enc_len=[1, 1]), 'strides'),           # rows 0 floats apart
        (dict(align=m, enc_len=[1, 0]), r'enc_len.*\[1, 0\]'),
        (dict(align=m, enc_len=[5, 1]), r'enc_len.*\[5, 1\]'),
        (dict(align=m, enc_len=[1]), 'enc_len'),
        (dict(align=m, enc_len=[1.0, 2.0]), 'enc_len'),
        (dict(align=m, enc_len=torch.tensor([1.0, 2.0]).to('meta')), 'enc_len'),
        (dict(align=m, enc_len=torch.tensor([1, 2, 3]).to('meta')), 'enc_len'),
        (dict(align=m, enc_len=[1, 1], patience=0), 'patience.*0'),
        (dict(align=m, enc_len=[1, 1], patience=2.0), 'patience'),
        (dict(align=m, enc_len=[1, 1], patience=2 ** 31), 'patience'),
        (dict(align=m, enc_len=[1, 1], max_jump=0), 'max_jump.*0'),
        (dict(align=m, enc_len=[1, 1], max_jump=-3), 'max_jump.*-3'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            metrics.attention_endpoints(**kw)
    # arguments the kernel takes get as far as the library (and no further here)
    wide = torch.rand(3, 9, 12).to('meta')
    for kw in (dict(align=m, enc_len=[4, 1]), dict(align=m, enc_len=np.array([2, 3]), patience=1, max_jump=1),
               dict(align=m, enc_len=torch.tensor([1, 9]).to('meta')),                # a device tensor is clamped by the kernel
               dict(align=wide[1:, :7, :5], enc_len=[5, 5])):                          # a sliced view keeps its strides
        with pytest.raises(AssertionError, match='reached the device'):
            ops.attn_endpoint(**kw)


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']
_SYN = ['--synth-phn-dir', 'phn']
_NO_COMBINE = '--synth-phn-dir does not combine with --'
_BELONG = '--synth-sid, --end-patience, --end-max-jump and --max-frames-per-phone belong to --synth-phn-dir'


def test_synth_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + _SYN + ['--synth-sid', '7', '--end-patience', '5', '--end-max-jump', '2', '--max-frames-per-phone', '9.5',
                                       '--vocab', 'v', '--gen-wav', '--gen-wav-feat', 'mel', '--batch-size', '4', '--load', 'c.pth'])
    assert (p.synth_phn_dir, p.synth_sid, p.end_patience, p.end_max_jump, p.max_frames_per_phone) == ('phn', 7, 5, 2, 9.5)
    assert (p.vocab, p.gen_wav, p.gen_wav_feat, p.batch_size, p.load) == ('v', True, 'mel', 4, 'c.pth')
    p = entry.parse_args(CFG + _SYN)
    assert (p.synth_sid, p.end_patience, p.end_max_jump, p.max_frames_per_phone, p.gen_wav) == (0, 3, 4, None, False)
    p = entry.parse_args(CFG)
    assert p.synth_phn_dir is None and (p.synth_sid, p.end_patience, p.end_max_jump) == (0, 3, 4)


def test_gen_wav_is_read_by_the_new_mode(capsys):
    entry = _entry()
    entry.parse_args(CFG + _SYN + ['--gen-wav'])
    assert 'gen-wav accepted for compatibility' not in capsys.readouterr().out
    entry.parse_args(CFG + ['--gen-wav'])
    assert 'gen-wav accepted for compatibility' in capsys.readouterr().out


@pytest.mark.parametrize('argv,msg', [
    (CFG + _SYN + ['--gen-specgram'], _NO_COMBINE + 'gen-specgram'),
    (CFG + _SYN + ['--tts-only'], _NO_COMBINE + 'tts-only'),
    (CFG + _SYN + ['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
    (CFG + _SYN + ['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
    (CFG + _SYN + ['--transcribe-wav-dir', 't'], 'does not combine with --'),           # (that mode's own block answers first)
    (CFG + _SYN + ['--align-wav-dir', 'a'], _NO_COMBINE + 'align-wav-dir'),
    (CFG + _SYN + ['--vocode-dir', 'v'], _NO_COMBINE + 'vocode-dir'),
    (CFG + _SYN + ['--resample-wav-dir', 'r', '--resample-out', 'o'], _NO_COMBINE + 'resample-wav-dir'),
    (CFG + _SYN + ['--feat-wav-dir', 'f', '--feat', 'mfcc'], _NO_COMBINE + 'feat-wav-dir'),
    (CFG + _SYN + ['--mcd-wav-dir', 's', '--mcd-ref-dir', 'r'], _NO_COMBINE + 'mcd-wav-dir'),
    (CFG + _SYN + ['--build-lm-phn-dir', 'p', '--lm', 'x.npy', '--lm-order', '2'], _NO_COMBINE + 'build-lm-phn-dir'),
    (_SYN, '--synth-phn-dir needs --config'),
    (CFG + ['--synth-sid', '1'], _BELONG),
    (CFG + ['--end-patience', '3'], _BELONG),
    (CFG + ['--end-max-jump', '4'], _BELONG),
    (CFG + ['--max-frames-per-phone', '12'], _BELONG),
    (CFG + ['--gen-specgram', '--end-patience', '3'], _BELONG),
    (CFG + _SYN + ['--synth-sid', '-1'], '--synth-sid must be >= 0'),
    (CFG + _SYN + ['--end-patience', '0'], '--end-patience must be >= 1'),
    (CFG + _SYN + ['--end-max-jump', '0'], '--end-max-jump must be >= 1'),
    (CFG + _SYN + ['--max-frames-per-phone', '0'], '--max-frames-per-phone must be finite and positive'),
    (CFG + _SYN + ['--max-frames-per-phone', 'inf'], '--max-frames-per-phone must be finite and positive'),
    (CFG + _SYN + ['--max-frames-per-phone', 'nan'], '--max-frames-per-phone must be finite and positive'),
    (CFG + _SYN + ['--gen-wav-feat', 'mel'], '--gen-wav-feat chooses what'),             # without --gen-wav
])
def test_synth_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


# ---------------------------------------------------------------- transcripts
def test_transcript_validation_names_the_file(tmp_path):
    from semi_tts_amd.solver import read_synth_transcripts, read_vocab
    from semi_tts_amd.vqvae import check_transcript
    assert check_transcript([3, 42, 1], 43) == [3, 42, 1]
    for ids, msg in (([], 'empty'), ([3, 0, 4], 'token 1 is id 0'), ([3, 43], 'token 1 is id 43'), ([-2], 'token 0 is id -2'), ([2.5], 'not an id')):
        with pytest.raises(ValueError, match=msg):
            check_transcript(ids, 43)
    d = tmp_path / 'phn'
    d.mkdir()
    with pytest.raises(ValueError, match='no .phn files'):
        read_synth_transcripts(str(d), None, 43)
    vocab = tmp_path / 'phn.vocab'
    vocab.write_text('\n'.join('P%d' % i for i in range(40)) + '\n')
    voc = read_vocab(str(vocab))
    (d / 'b.phn').write_text('-12.500000\t5 6 7\n-13.000000\t5 6\n')        # what --transcribe-wav-dir writes: the first path is read
    (d / 'a.phn').write_text('P0 P39 4\n')
    (d / 'notes.txt').write_text('x')
    assert read_synth_transcripts(str(d), voc, 43) == (['a.phn', 'b.phn'], [[3, 42, 4], [5, 6, 7]])
    for text, msg in (('\n', r'c\.phn: empty transcript'), ('3 0 4\n', r'c\.phn: token 1 is id 0'), ('3 43\n', r'c\.phn: token 1 is id 43'),
                      ('3 <pad>\n', r'c\.phn: token 1 is id 0'), ('3 XX\n', r'c\.phn.*unknown symbol')):
        (d / 'c.phn').write_text(text)
        with pytest.raises(ValueError, match=msg):
            read_synth_transcripts(str(d), voc, 43)


# ---------------------------------------------------------------- the decode length and the csv row
def test_decode_length_formula():
    from semi_tts_amd import vqvae
    from semi_tts_amd.vqvae import synth_frames
    assert vqvae.SYNTH_MAX_FRAMES_PER_PHONE == 2.0 * vqvae.FRAME_PHN_RATIO == 12.0 and vqvae.INFERENCE_MARGIN_FRAMES == 40
    assert synth_frames(1, 3) == 54                                 # 12 + 40 = 52 -> 18 steps of 3
    assert synth_frames(12, 3) == 186                               # 144 + 40 = 184 -> 62 steps
    assert synth_frames(5, 2) == 100 and synth_frames(5, 1) == 100 and synth_frames(5, 7) == 105
    assert synth_frames(5, 3, 4.5) == 63                            # 22.5 + 40 = 62.5 -> 21 steps
    assert synth_frames(10, 5, 6.0) == 100
    for n in (1, 7, 100):
        for r in (1, 2, 3, 5):
            f = synth_frames(n, r)
            assert f % r == 0 and 0 <= f - (12 * n + 40) < r
    for kw in (dict(n_max=0, r=3), dict(n_max=3, r=0), dict(n_max=3, r=3, max_frames_per_phone=0.0),
               dict(n_max=3, r=3, max_frames_per_phone=float('inf')), dict(n_max=3, r=3, max_frames_per_phone=float('nan'))):
        with pytest.raises(ValueError, match='synth_frames'):
            synth_frames(**kw)


def test_synth_csv_row_layout():
    from semi_tts_amd.solver import SYNTH_HEADER, synth_row
    assert SYNTH_HEADER == 'file,tokens,steps,frames,seconds,reached,focus,backward,skips,covered'
    row = synth_row('u1.phn', 12, 31, 93, 1.15, 1, 0.73456, 2, 0, 11)
    assert row == 'u1.phn,12,31,93,1.1500,1,0.7346,2,0,11'
    assert len(row.split(',')) == len(SYNTH_HEADER.split(','))
    assert synth_row('x.phn', 1, 18, 54, 0.6625, 0, float('nan'), 0, 0, 1) == 'x.phn,1,18,54,0.6625,0,nan,0,0,1'
