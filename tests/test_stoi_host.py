"""The CPU side of the intelligibility measure: the float64 oracle's own properties (tests/stoi_oracle.py), the guards of the case table
the GPU tests compare integers on (tests/stoi_cases.py), every refusal that has to come before a device is touched, and
solver.StoiScorer's pairing, length rules and stoi.csv with the scoring call replaced by the oracle."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_cases as SC    # noqa: E402
import stoi_oracle as SO   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174),
         (174, 219)]


# ---------------------------------------------------------------- the oracle
def test_band_edges_are_the_published_table():
    from semi_tts_amd import ops
    assert SO.EDGES == EDGES and list(ops.STOI_BAND_EDGES) == EDGES
    assert (ops.STOI_FS, ops.STOI_FRAME, ops.STOI_HOP, ops.STOI_NFFT, ops.STOI_BANDS, ops.STOI_SEG) == (SO.FS, SO.N_FRAME, SO.HOP, SO.NFFT, SO.J, SO.N_SEG)
    assert ops.STOI_SENTINEL == SO.SENTINEL and ops.STOI_CHUNK == SC.CHUNK


def test_window_is_hanning_258_without_its_zeros():
    assert np.abs(SO.window() - np.hanning(258)[1:-1]).max() < 1e-15


@pytest.mark.parametrize('L', [4097, 7000, 30000])
def test_identical_signals_score_one(L):
    c = SC.by_name('L%d/none' % L)
    r = SC.oracle(c)
    assert abs(r['score'][0] - 1.0) < 1e-12 and abs(r['score'][1] - 1.0) < 1e-12


def test_frame_counts_and_the_4096_4097_boundary():
    from semi_tts_amd import ops
    for L in (1, 200, 256, 257, 384, 385, 4096, 4097, 4225, 7000, 1 << 22):
        assert ops.stoi_frames(L) == SO.n_frames(L), L
    assert [SO.n_frames(L) for L in (200, 256, 257, 384, 385)] == [0, 0, 1, 1, 2]
    assert SC.oracle(SC.by_name('L200/none'))['counts'] == (0, 0, 0, 0)
    assert SC.oracle(SC.by_name('L257/none'))['counts'] == (1, 1, 0, 0)
    a, b, c = (SC.oracle(SC.by_name('L%d/snr5' % L)) for L in (4096, 4097, 4225))
    assert a['counts'] == (30, 30, 29, 0) and a['score'] == (SO.SENTINEL, SO.SENTINEL)
    assert b['counts'] == (31, 31, 30, 1) and b['score'][0] != SO.SENTINEL
    assert c['counts'] == (32, 32, 31, 2)


def test_muted_stretches_are_dropped_and_the_scan_chunk_is_crossed():
    r = SC.oracle(SC.by_name('L7000/none'))
    F, K, M, S = r['counts']
    assert F == 53 and 30 < K < F and M == K - 1 and S == M - 29
    assert (np.diff(r['kept']) > 1).sum() == 3                     # three gaps
    F, K, _, _ = SC.oracle(SC.by_name('L37000/none'))['counts']
    assert K > SC.CHUNK and F > K                                  # the selection launch carries its scan across a chunk and drops frames


def test_digital_silence_scores_zero():
    x = SC.by_name('L7000/none')['x']
    z = np.zeros_like(x)
    for a, b in ((x, z), (z, x), (z, z)):
        r = SO.stoi(a, b)
        assert r['score'] == (0.0, 0.0) and r['counts'][3] >= 1, r['score']
    assert SO.stoi(z, z)['counts'] == (53, 53, 52, 23)             # every frame of a silent clean side is kept


def test_anti_phased_envelopes_score_negative():
    t = np.arange(8000) / 10000.0
    rs = np.random.RandomState(3)
    car = rs.randn(8000)
    env = 0.5 - 0.5 * np.cos(2 * np.pi * 4.0 * t)
    r = SO.stoi(car * (0.2 + env), car * (1.2 - env))
    assert r['score'][0] < 0.0


def test_the_score_falls_with_the_snr():
    for L in (7000, 30000):
        d = [SC.oracle(SC.by_name('L%d/%s' % (L, deg)))['score'] for deg in ('none', 'snr20', 'snr5', 'snr-5')]
        assert all(a[0] > b[0] and a[1] > b[1] for a, b in zip(d, d[1:])), d


def test_non_finite_input_gives_nan():
    c = SC.by_name('L7000/snr20')
    x, y = c['x'].copy(), c['y'].copy()
    x[1000] = np.nan
    r = SO.stoi(x, c['y'])
    assert np.isnan(r['score']).all() and r['counts'] == (53, 0, 0, 0)
    kept = SC.oracle(c)['kept']
    y[128 * int(kept[5]) + 17] = np.nan
    r = SO.stoi(c['x'], y)
    assert np.isnan(r['score']).all() and r['counts'] == SC.oracle(c)['counts']


# ---------------------------------------------------------------- guards: conditions on the case table, not measurements
def test_guard_every_integer_case_keeps_its_margin():
    """the GPU decides e + EPS > 0.01f (max + EPS) on fp32 norms whose relative error is far below 264 * 2^-24 = 1.6e-5 = 1.4e-4 dB;
    a case whose closest frame is 0.01 dB or more from the threshold decides alike in fp32 and in float64"""
    low = [(c['name'], m) for c in SC.CASES for m in [SO.margin_db(c['x'])] if not m >= SC.MARGIN_DB]
    assert not low, low


def test_guard_the_clipping_cases_clip_some_cells_and_not_all():
    clipping = [c for c in SC.CASES if SC.clips(c)]
    assert {c['deg'] for c in clipping} == set(SC.CLIPPING) and len(clipping) >= 12
    for c in clipping:
        assert 0.0 < SC.oracle(c)['clipped'] < 1.0, c['name']
    assert SC.oracle(SC.by_name('L4097/snr20'))['clipped'] == 0.0
    assert all(SC.oracle(c)['clipped'] == 0.0 for c in SC.CASES if c['deg'] == 'none')


def test_the_float32_form_is_float32_and_close():
    c = SC.by_name('L7000/snr5')
    r32, r64 = SC.oracle(c, np.float32), SC.oracle(c)
    assert r32['bands'].dtype == np.float32 and r32['norms'].dtype == np.float32 and r64['bands'].dtype == np.float64
    assert r32['counts'] == r64['counts'] and r32['score'] != r64['score']
    assert max(abs(a - b) for a, b in zip(r32['score'], r64['score'])) < 1e-5


# ---------------------------------------------------------------- refusals before a device is touched
@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to pick a device fails the test"""
    from semi_tts_amd import _lib, audio

    def touched(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(_lib, 'load', touched)
    monkeypatch.setattr(audio, '_device', touched)


def test_metrics_stoi_refuses_before_a_device(no_device):
    import torch
    from semi_tts_amd import ops
    from semi_tts_amd.metrics import stoi
    a, b = np.zeros(5000, np.float32), np.zeros(4999, np.float32)
    with pytest.raises(ValueError, match='pair 1 has 5000 clean and 4999 processed samples'):
        stoi([a, a], [a, b], 10000)
    with pytest.raises(ValueError, match='2 clean and 1 processed signals'):
        stoi([a, a], [a], 10000)
    with pytest.raises(ValueError, match='clean is an empty batch'):
        stoi([], [], 10000)
    with pytest.raises(ValueError, match='non-empty 1-D floating point or int16'):
        stoi([np.zeros(0, np.float32)], [np.zeros(0, np.float32)], 10000)
    with pytest.raises(ValueError, match='non-empty 1-D floating point or int16'):
        stoi([np.zeros((2, 50), np.float32)], [np.zeros((2, 50), np.float32)], 10000)
    for rate in (0, -8000, 22050.0, True, None):
        with pytest.raises(ValueError, match='resample: orig_sr must be a positive integer'):
            stoi([a], [a], rate)
    with pytest.raises(ValueError, match='floats of staged'):          # a ratio the resampler's kernel does not take
        stoi([a], [a], 10007)
    big = torch.zeros(ops.STOI_MAX_LEN + 1)
    with pytest.raises(ValueError, match='above the limit of %d' % ops.STOI_MAX_LEN):
        stoi([big], [big], 10000)
    with pytest.raises(ValueError, match='above the limit of %d' % ops.STOI_MAX_LEN):
        stoi([big[:ops.STOI_MAX_LEN // 2 + 2]], [big[:ops.STOI_MAX_LEN // 2 + 2]], 5000)


def test_ops_stoi_batch_refuses_before_a_device(no_device):
    import torch
    from semi_tts_amd import ops
    x = torch.zeros(100)
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.stoi_batch(x, x.clone(), [0], [100])
    for lens, msg in ((np.ones(65, np.int64), 'one call takes no more pairs'), (np.array([0]), r'must lie in \[1, 4194304\]'),
                      (np.array([ops.STOI_MAX_LEN + 1]), r'must lie in \[1, 4194304\]'), (np.array([2.0]), 'one call takes no more pairs')):
        with pytest.raises(ValueError, match=msg):
            ops._stoi_check(lens)
    with pytest.raises(ValueError, match='F_pad 1 below the 2 frames'):
        ops._stoi_check(np.array([385]), 1)
    assert ops._stoi_check(np.array([200])) == 1 and ops._stoi_check(np.array([385, 300])) == 2 and ops._stoi_check(np.array([], np.int64)) == 1
    with pytest.raises(ValueError, match="y must be a packed 1-D contiguous float32 tensor of x's size"):
        ops.stoi_batch(x, torch.zeros(99), [0], [100])


def test_build_lists_and_signatures():
    import ctypes as C
    from semi_tts_amd import _lib, build
    assert build.STOI_SOURCES == ['stoi.hip'] and os.path.isfile(os.path.join(build.CSRC, 'stoi.hip')) and len(build.SOURCES) == 20
    P, I = C.c_void_p, C.c_int
    assert _lib.SIGNATURES['st_stoi_batch'] == [C.POINTER(_lib.StWaveBatch), P, P, P, I, P, P, P, P, P]
    assert _lib.SIGNATURES['st_stoi_workspace_floats'] == [I, I] and _lib.SIGNATURES['st_stoi_frames'] == [I]
    header = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    for name in ('st_stoi_batch', 'st_stoi_workspace_floats', 'st_stoi_frames'):
        assert name + '(' in header


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


def test_stoi_flags_parse():
    entry = _entry()
    p = entry.parse_args(['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b'])
    assert (p.stoi_wav_dir, p.stoi_ref_dir, p.stoi_max_len_diff, p.config) == ('a', 'b', 0.05, None)
    p = entry.parse_args(['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-max-len-diff', '0', '--batch-size', '8'])
    assert p.stoi_max_len_diff == 0.0 and p.batch_size == 8
    p = entry.parse_args(['--config', 'x.yaml', '--mcd-wav-dir', 'a', '--mcd-ref-dir', 'b', '--trim-silence'])        # (as before)
    assert (p.stoi_wav_dir, p.stoi_ref_dir, p.stoi_max_len_diff) == (None, None, None) and p.trim_silence is True


@pytest.mark.parametrize('argv, msg', [
    (['--stoi-wav-dir', 'a'], '--stoi-wav-dir needs --stoi-ref-dir DIR'),
    (['--stoi-ref-dir', 'b'], 'belong to --stoi-wav-dir'),
    (['--config', 'x.yaml', '--stoi-max-len-diff', '0.1'], 'belong to --stoi-wav-dir'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--trim-silence'], '--stoi-wav-dir does not combine with --trim-silence: changing the two sides separately'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--normalize-loudness'], '--stoi-wav-dir does not combine with --normalize-loudness'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-max-len-diff', '-1'], '--stoi-max-len-diff must be finite and at least 0'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-max-len-diff', 'inf'], '--stoi-max-len-diff must be finite and at least 0'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--dev-batches', '2'], '--stoi-wav-dir does not combine with --dev-batches'),
] + [(['--config', 'x.yaml', '--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b'] + mode, '--stoi-wav-dir does not combine with --' + mode[0][2:]) for mode in (
    ['--gen-specgram'], ['--tts-only'], ['--unpair-wav-dir', 'd'], ['--transcribe-wav-dir', 'd'], ['--align-wav-dir', 'd'],
    ['--build-lm-phn-dir', 'd', '--lm', 't.npy', '--lm-order', '2'], ['--vocode-dir', 'd'], ['--resample-wav-dir', 'd', '--resample-out', 'e'],
    ['--feat-wav-dir', 'd', '--feat', 'mfcc'], ['--mcd-wav-dir', 'd', '--mcd-ref-dir', 'e'], ['--synth-phn-dir', 'd'],
    ['--score-phn-dir', 'd', '--score-ref-dir', 'e'], ['--abx-ali-dir', 'd', '--abx-wav-dir', 'e'])])
def test_stoi_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


# ---------------------------------------------------------------- solver.StoiScorer on tiny wavs, the scoring call replaced by the oracle
def _paras(tmp_path, **kw):
    d = dict(stoi_wav_dir=str(tmp_path / 'syn'), stoi_ref_dir=str(tmp_path / 'ref'), stoi_max_len_diff=0.05, batch_size=2, name='run',
             logdir=str(tmp_path / 'log'), verbose=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _pcm(x):
    return np.rint(np.clip(np.asarray(x, np.float64), -1.0, 1.0) * 32767.0) / 32768.0        # what read_wav gives back of write_wav


@pytest.fixture
def wavs(tmp_path):
    from semi_tts_amd.audio import write_wav
    (tmp_path / 'syn').mkdir()
    (tmp_path / 'ref').mkdir()
    table = {}
    for name, case, cut in (('a-pred.wav', 'L7000/snr5', 0), ('b.wav', 'L4096/snr20', 0), ('c.x.wav', 'L4225/burst', 100)):
        c = SC.by_name(case)
        key = name.split('.')[0].replace('-pred', '')
        write_wav(str(tmp_path / 'syn' / name), c['y'][:len(c['y']) - cut], 10000)
        write_wav(str(tmp_path / 'ref' / (key + '.wav')), c['x'], 10000)
        n = len(c['x']) - cut
        table[name] = (n, SO.stoi(_pcm(c['x'])[:n], _pcm(c['y'])[:n]))
    return table


def _oracle_stub(calls):
    import torch
    from semi_tts_amd.metrics import StoiResult

    def stub(clean, degraded, sample_rate, want_parts=False):
        calls.append((len(clean), sample_rate))
        res = [SO.stoi(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in zip(clean, degraded)]
        return StoiResult(torch.tensor([r['score'] for r in res], dtype=torch.float32), torch.tensor([r['counts'] for r in res], dtype=torch.int32),
                          None, None, None)
    return stub


def test_scorer_pairs_cuts_and_writes_the_csv(tmp_path, wavs, monkeypatch, capsys):
    from semi_tts_amd import metrics
    from semi_tts_amd.solver import STOI_HEADER, StoiScorer
    calls = []
    monkeypatch.setattr(metrics, 'stoi', _oracle_stub(calls))
    s = StoiScorer(None, _paras(tmp_path), 'test').load_data().set_model()
    assert s.pairs == [('a-pred.wav', 'a', 'a.wav'), ('b.wav', 'b', 'b.wav'), ('c.x.wav', 'c', 'c.wav')]
    assert s.samples == [7000, 4096, 4125] and s.rates == [10000] * 3        # c is cut to its shorter, processed side
    assert s.exec() == 3 and calls == [(2, 10000), (1, 10000)]               # --batch-size 2: one call and one host read a batch
    lines = open(str(tmp_path / 'log' / 'run' / 'stoi.csv')).read().split('\n')
    assert lines[0] == STOI_HEADER == 'file,samples,frames,kept,segments,stoi,estoi' and lines[-1] == '' and len(lines) == 5
    for line, name in zip(lines[1:4], ('a-pred.wav', 'b.wav', 'c.x.wav')):
        n, want = wavs[name]
        F, K, M, S = want['counts']
        assert line == '%s,%d,%d,%d,%d,%.6f,%.6f' % (name, n, F, K, S, np.float32(want['score'][0]), np.float32(want['score'][1]))
    assert lines[2] == 'b.wav,4096,30,30,0,0.000010,0.000010'                # the sentinel row
    out = capsys.readouterr().out
    assert '[WARNING]' in out and 'b.wav has 29 band frames' in out
    scored = [wavs[n][1]['score'] for n in ('a-pred.wav', 'c.x.wav')]        # the sentinel is left out of the means
    assert abs(s.mean_stoi - np.mean([v[0] for v in scored])) < 1e-6 and abs(s.mean_estoi - np.mean([v[1] for v in scored])) < 1e-6
    assert 'STOI of 3 pairs (2 scored)' in out


def test_scorer_stops_in_load_data_naming_the_file(tmp_path, wavs, no_device):
    import wave
    from semi_tts_amd.audio import write_wav
    from semi_tts_amd.solver import StoiScorer
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    load = lambda **kw: StoiScorer(None, _paras(tmp_path, **kw), 'test').load_data()      # noqa: E731
    with pytest.raises(ValueError, match=r'c\.x\.wav has 4125 samples and its recording .*c\.wav 4225: they differ by 0\.0100 s, above --stoi-max-len-diff 0\.005'):
        load(stoi_max_len_diff=0.005)
    assert load(stoi_max_len_diff=0.01).samples[2] == 4125
    write_wav(str(syn / 'd.wav'), np.zeros(300), 10000)
    with pytest.raises(ValueError, match=r'--stoi-wav-dir: d\.wav has no recording .*d\.wav'):
        load()
    write_wav(str(ref / 'd.wav'), np.zeros(300), 16000)
    with pytest.raises(ValueError, match=r'd\.wav is at 10000 Hz and its recording .*d\.wav at 16000 Hz'):
        load()
    write_wav(str(syn / 'd.wav'), np.zeros(300), 10007)
    write_wav(str(ref / 'd.wav'), np.zeros(300), 10007)
    with pytest.raises(ValueError, match=r'--stoi-wav-dir: .*d\.wav: resample: 10007 -> 10000 Hz'):
        load()
    for width, ch, msg in ((1, 1, '8-bit with 1 channels'), (2, 2, '16-bit with 2 channels')):
        with wave.open(str(syn / 'd.wav'), 'wb') as w:
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(10000)
            w.writeframes(b'\0' * 600)
        with pytest.raises(ValueError, match=r'd\.wav is %s; only 16-bit mono PCM is read' % msg):
            load()
    (syn / 'd.wav').write_bytes(b'not a wav')
    with pytest.raises(ValueError, match=r'd\.wav is not a readable \.wav file'):
        load()
    os.remove(str(syn / 'd.wav'))
    write_wav(str(syn / 'a.wav'), np.zeros(7000), 10000)
    with pytest.raises(ValueError, match=r'--stoi-wav-dir: a-pred\.wav and a\.wav share the recording a\.wav'):
        load()
    os.remove(str(syn / 'a.wav'))
    empty = tmp_path / 'none'
    empty.mkdir()
    with pytest.raises(ValueError, match='--stoi-wav-dir .*none: no .wav files'):
        load(stoi_wav_dir=str(empty))
    assert not (tmp_path / 'log').exists()


def test_mcd_pairs_keeps_its_messages(tmp_path):
    from semi_tts_amd.solver import mcd_pairs
    (tmp_path / 'e').mkdir()
    with pytest.raises(ValueError, match='--mcd-wav-dir .*: no .wav files'):
        mcd_pairs(str(tmp_path / 'e'), str(tmp_path / 'e'))
    (tmp_path / 'e' / 'x-pred.wav').write_bytes(b'')
    with pytest.raises(ValueError, match=r'--mcd-wav-dir: x-pred\.wav has no recording'):
        mcd_pairs(str(tmp_path / 'e'), str(tmp_path / 'f'))
