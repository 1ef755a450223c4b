"""CPU-side tests of the loudness path: the K-weighting coefficients and tables, the float64 oracle on known readings, the guard on the
shared case table, every refusal that needs no device, and the command-line rules.  Nothing here launches a kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_cases as LC   # noqa: E402
import loudness_oracle as LO  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
TABLE_48K = (([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585]),
             ([1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621]))


def test_coefficients_reproduce_the_standards_table():
    from semi_tts_amd.audio import kweight_coeffs
    for got in (kweight_coeffs(48000), LO.coeffs(48000)):
        for (b, a), (wb, wa) in zip(got, TABLE_48K):
            assert np.abs(np.asarray(b) - wb).max() <= 1e-12 and np.abs(np.asarray(a) - wa).max() <= 1e-12
    assert list(kweight_coeffs(16000)[1][0]) == [1.0, -2.0, 1.0]
    for fs in (8000, 11025, 16000, 22050, 44100, 48000):           # the product's and the oracle's formulas are written apart: they agree
        for (b, a), (wb, wa) in zip(kweight_coeffs(fs), LO.coeffs(fs)):
            assert np.abs(np.asarray(b) - wb).max() <= 1e-15 and np.abs(np.asarray(a) - wa).max() <= 1e-15


def test_oracle_reads_the_calibration_sine():
    """a 0 dBFS 997 Hz sine: -3.01 LKFS at 48 kHz (the standard's calibration), -2.970 at 16 kHz (the bilinear warp)"""
    for fs, want, tol in ((48000, -3.0103, 0.005), (16000, -2.970, 0.005)):
        m = LO.measure(np.sin(2.0 * np.pi * 997.0 * np.arange(3 * fs) / fs), fs)
        assert abs(m['lufs'] - want) <= tol and m['flags'] == 0 and m['n_blocks'] == 27 == m['n_abs'] == m['n_rel'], (fs, m['lufs'])
        assert abs(m['ungated'] - m['lufs']) < 1e-3 and abs(m['rel_gate'] - (m['lufs'] - 10.0)) < 1e-3


def test_oracle_gates_by_hand():
    """hop energies chosen so that the blocks sit at known levels: one block under -70, quiet blocks between the gates"""
    fs, hop = 8000, 800
    z = lambda l: 10.0 ** ((l + 0.691) / 10.0)                     # noqa: E731
    e = np.array([z(-20.0) * hop] * 8 + [z(-45.0) * hop] * 8 + [z(-90.0) * hop] * 8)
    g = LO.gate(e, fs)
    assert g['n_blocks'] == 21 and g['n_abs'] == 16 and abs(g['momentary_max'] + 20.0) < 1e-9
    assert g['n_rel'] == 8 and -30.0 > g['rel_gate'] > -35.0 and -20.0 > g['lufs'] > -21.0       # blocks 0 .. 7 hold at least one loud hop
    assert LO.gate(e[:3], fs)['n_blocks'] == 0 and np.isnan(LO.gate(e[:3], fs)['lufs'])
    q = LO.gate(np.full(6, z(-75.0) * hop), fs)
    assert q['n_abs'] == 0 and q['lufs'] == -np.inf and abs(q['ungated'] + 75.0) < 1e-9
    m = LO.measure(np.zeros(5000, np.float32), fs, -23.0)
    assert m['flags'] == LO.F_SILENT and m['gain'] == 1.0 and m['lufs'] == -np.inf
    assert LO.measure(np.ones(3199, np.float32), fs, -23.0)['flags'] == LO.F_SHORT
    x = np.ones(4000, np.float32)
    x[5] = np.inf
    assert LO.measure(x, fs, -23.0)['flags'] == LO.F_NONFINITE
    assert LO.to_pcm16(np.array([0.0, 1.0, -1.0, 2.0, 0.5, -0.25], np.float32)).tolist() == [0, 32767, -32767, 32767, 16384, -8192]


def test_guard_every_integer_case_keeps_its_margin():
    """every block of every case whose counts are compared keeps MARGIN_LU from -70 and from the relative gate, and each gain limit
    that a case is meant to hit binds with room: asserted, not skipped"""
    flags = set()
    for c in LC.integer_cases() + [k for fs in LC.RATES + (48000,) for k in LC.neighbours(fs)] + LC.ragged_pool(8000, 65):
        m = LO.measure(c['x'], c['fs'], c['target'], c['peak_db'], c['max_gain_db'])
        l = m['l'][np.isfinite(m['l'])]
        assert len(c['x']) <= 3 * c['fs']
        if len(l):
            assert np.abs(l + 70.0).min() >= LC.MARGIN_LU, c['name']
            if np.isfinite(m['rel_gate']):
                assert np.abs(l - m['rel_gate']).min() >= LC.MARGIN_LU, c['name']
        if m['flags'] in (0, 8, 16):                               # the limit that binds does so by more than 0.05 dB
            g0 = 10.0 ** ((c['target'] - m['lufs']) / 20.0)
            gp, gm = 10.0 ** (c['peak_db'] / 20.0) / m['peak'], 10.0 ** (c['max_gain_db'] / 20.0)
            assert abs(20.0 * np.log10(g0 / min(gp, gm))) >= LC.MARGIN_LU and abs(20.0 * np.log10(gp / gm)) >= LC.MARGIN_LU, c['name']
        if not c['name'].split('/')[1].startswith(('pool', 'full')):
            flags.add(m['flags'])
    assert flags == {0, 2, 4, 8, 16}
    by = {c['name']: LO.measure(c['x'], c['fs'], c['target']) for c in LC.kernel_cases() if c['fs'] == 8000}
    m = by['8000/loud_quiet_loud']
    assert m['n_abs'] == m['n_blocks'] > m['n_rel'] > 0            # the quiet middle: inside the absolute gate, outside the relative one
    m = by['8000/burst_then_silence']
    assert m['n_blocks'] > m['n_abs'] > m['n_rel'] > 0
    assert LO.measure(LC.wide_cases()[0]['x'], 48000)['n_abs'] == 1         # DC: only the block of the switch-on transient is audible


def test_case_table_straddles_the_kernel_constants():
    from semi_tts_amd import ops
    assert [ops.loudness_hop(fs) for fs in (8000, 11025, 16000, 48000)] == [800, 1103, 1600, 4800]
    assert [ops.loudness_run_length(fs) for fs in (8000, 11025, 16000, 44100, 48000)] == [4, 5, 7, 18, 19]
    for fs in LC.RATES:
        assert LC.hop_of(fs) == ops.loudness_hop(fs) and LC.run_of(fs) == ops.loudness_run_length(fs)
        hop, r = LC.hop_of(fs), LC.run_of(fs)
        lens = sorted(len(c['x']) for c in LC.length_cases(fs))
        assert {4 * hop - 1, 4 * hop, 4 * hop + 1, 7 * hop - 1} <= set(lens)
        assert any((L + 1) % r == 0 for L in lens) and any((L - 1) % r == 0 for L in lens)
    assert 256 * LC.run_of(11025) - LC.hop_of(11025) == 177        # the odd hop: 177 samples of padding in front of every hop
    assert len(LC.wide_cases()) == 2 and all(c['fs'] == 48000 for c in LC.wide_cases())


def test_tables_layout_and_powers():
    from semi_tts_amd import ops
    from semi_tts_amd.audio import kweight_coeffs, kweight_state_matrix, kweight_tables
    for fs in (8000, 11025, 48000):
        tab = kweight_tables(fs)
        assert tab.dtype == np.float64 and tab.shape == (ops.LOUDNESS_TABLE_DOUBLES,) and kweight_tables(fs) is tab
        (b, a), (_, p) = kweight_coeffs(fs)
        assert tab[:8].tolist() == [b[0], b[1], b[2], a[1], a[2], p[1], p[2], 0.0]
        A, hop, r = kweight_state_matrix(fs), ops.loudness_hop(fs), ops.loudness_run_length(fs)
        pad = 256 * r - hop
        assert 0 <= pad < 256
        assert np.array_equal(tab[8:24].reshape(4, 4), np.linalg.matrix_power(A, r))
        assert np.array_equal(tab[136:152].reshape(4, 4), np.linalg.matrix_power(A, hop))
        T = tab[152:].reshape(256, 4, 4)
        first = pad // r                                            # the last thread with no sample of the hop in front of its run
        assert all(np.array_equal(T[t], np.eye(4)) for t in range(first + 1)) and not np.array_equal(T[first + 1], np.eye(4))
        full = np.linalg.matrix_power(A, hop)                       # (the shelf's block of it underflows at 48 kHz: compare against the largest entry)
        assert np.abs(T[255] @ np.linalg.matrix_power(A, r) - full).max() <= 1e-9 * np.abs(full).max()
        # the state recurrence of the tables is the filter: 50 samples through A, B, C, D against the oracle's lfilter
        x = np.random.RandomState(1).randn(50)
        s, y = np.zeros(4), []
        Bv = np.array([b[1] - a[1] * b[0], b[2] - a[2] * b[0], (-2.0 - p[1]) * b[0], (1.0 - p[2]) * b[0]])
        for v in x:
            y.append(s[0] + s[2] + b[0] * v)
            s = A @ s + Bv * v
        want = LO.lfilter(*LO.coeffs(fs)[1], LO.lfilter(*LO.coeffs(fs)[0], x))
        assert np.abs(np.array(y) - want).max() <= 1e-12 * np.abs(want).max()
    for bad in (7999, 48001, 16000.0, True):
        with pytest.raises(ValueError, match='sample rate must be an integer in'):
            kweight_tables(bad)


# ---------------------------------------------------------------- refusals without a device
def test_loudness_check_passes():
    from semi_tts_amd import ops
    assert ops._loudness_check(np.array([1, 16000 * 3]), 16000) == (1600, 30)
    assert ops._loudness_check(np.array([5]), 8000, target=-23.0, H_pad=7) == (800, 7)
    assert ops._loudness_check(np.arange(1, 65), 48000, target=float('nan')) == (4800, 1)


@pytest.mark.parametrize('kw, msg', [
    (dict(lens=np.zeros(0, np.int64)), 'lens must be 1 .. 64 integers'),
    (dict(lens=np.ones(65, np.int64)), 'lens must be 1 .. 64 integers'),
    (dict(lens=np.ones((2, 2), np.int64)), 'lens must be 1 .. 64 integers'),
    (dict(lens=np.array([1.0])), 'lens must be 1 .. 64 integers'),
    (dict(lens=np.array([5, 0])), 'every length must lie in'),
    (dict(lens=np.array([2 ** 31])), 'every length must lie in'),
    (dict(sr=7999), 'sample rate must be an integer in'),
    (dict(sr=48001), 'sample rate must be an integer in'),
    (dict(sr=16000.0), 'sample rate must be an integer in'),
    (dict(H_pad=0, lens=np.array([1600])), 'H_pad 0 below the 1 hops'),
    (dict(H_pad=2.0), 'H_pad 2.0 below'),
    (dict(peak_db=float('nan')), 'peak_db must be a finite number'),
    (dict(peak_db=float('inf')), 'peak_db must be a finite number'),
    (dict(max_gain_db=float('-inf')), 'max_gain_db must be a finite number'),
    (dict(max_gain_db='30'), 'max_gain_db must be a finite number'),
    (dict(target=float('inf')), 'target must be a finite number'),
    (dict(target='x'), 'target must be a finite number'),
])
def test_loudness_check_refusals(kw, msg):
    from semi_tts_amd import ops
    args = dict(lens=np.array([4000, 100]), sr=16000)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        ops._loudness_check(**args)


def test_ops_refuse_host_tensors_before_a_device():
    from semi_tts_amd import ops
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.loudness(torch.zeros(100), [0], np.array([100]), 16000)
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.wave_gain(torch.zeros(100), [0], np.array([100]), torch.zeros(1, 8))
    with pytest.raises(ValueError, match='lens must be 1 .. 64 integers'):
        ops.wave_gain(torch.zeros(100), np.zeros(65, np.int64), np.ones(65, np.int64), torch.zeros(65, 8))


def test_converter_check_loudness():
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000)
    conv._check_loudness(target=-23.0, lens=np.arange(1, 200))     # (more than one call's worth: the converter splits)
    with pytest.raises(ValueError, match='peak_db must be a finite number'):
        conv._check_loudness(peak_db=float('nan'))
    with pytest.raises(TypeError):
        conv._check_loudness(top_db=3)
    with pytest.raises(ValueError, match='peak_db must be a finite number'):                     # before any file is opened
        conv.load_batch(['/nonexistent.wav'], loudness=dict(target=-23.0, peak_db=float('inf')))
    low = load_audio_transform(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=4000)
    with pytest.raises(ValueError, match='sample rate must be an integer in'):
        low._check_loudness(target=-23.0)


def test_build_list_and_signatures():
    import ctypes as C
    from semi_tts_amd import _lib, build
    assert build.LOUDNESS_SOURCES == ['loudness.hip'] and 'loudness.hip' not in build.SOURCES and len(build.SOURCES) == 20
    assert os.path.exists(os.path.join(build.CSRC, 'loudness.hip'))
    sig = _lib.SIGNATURES
    assert sig['st_loudness_run_length'] == [C.c_int]
    assert sig['st_loudness_batch'] == [C.POINTER(_lib.StWaveBatch), C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert sig['st_wave_gain'] == [C.POINTER(_lib.StWaveBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    hdr = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    for name in ('st_loudness_run_length', 'st_loudness_batch', 'st_wave_gain'):
        assert ('int %s(' % name) in hdr
    assert 'loudness range' in hdr and 'short-term loudness' in hdr and 'true (oversampled) peak' in hdr      # what is out of scope is said


def test_loudness_report_line():
    from semi_tts_amd.corpus import loudness_report
    info = dict(flags=np.array([0, 8, 16, 2, 4, 1, 0]), lufs=np.array([-20.0, -30.0, -60.0, np.nan, -np.inf, np.nan, -26.0]))
    line = loudness_report('paired', info, -23.0)
    assert line == ('paired: loudness of 7 utterances, mean -34.00 min -60.00 max -20.00 LUFS before | normalised to -23.0 LUFS | 1 peak-limited, '
                    '1 gain-limited | left alone: 1 non-finite, 1 under 400 ms, 1 silent')
    assert 'measured only' in loudness_report('dev', info, None)


# ---------------------------------------------------------------- the command line
CFG = ['--config', 'x.yaml']
REFUSALS = [
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-target', '-70.5'], '--loudness-target must lie in [-70, 0] LUFS'),
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-target', '0.1'], '--loudness-target must lie in [-70, 0] LUFS'),
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-target', 'nan'], '--loudness-target must lie in [-70, 0] LUFS'),
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-peak', '0.5'], '--loudness-peak must be finite and at most 0 dBFS'),
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-peak=-inf'], '--loudness-peak must be finite and at most 0 dBFS'),
    (CFG + ['--corpus', '--normalize-loudness', '--loudness-max-gain', '-1'], '--loudness-max-gain must be finite and at least 0 dB'),
    (CFG + ['--loudness-wav-dir', 'a', '--loudness-max-gain', 'inf'], '--loudness-max-gain must be finite and at least 0 dB'),
    (CFG + ['--align-wav-dir', 'd', '--normalize-loudness'], '--normalize-loudness does not combine with --align-wav-dir'),
    (CFG + ['--feat-wav-dir', 'd', '--feat', 'mfcc', '--segment-file', 's.csv', '--normalize-loudness'], '--normalize-loudness does not combine with --segment-file'),
    (CFG + ['--normalize-loudness'], '--normalize-loudness normalises what --corpus'),
    (CFG + ['--gen-specgram', '--normalize-loudness'], '--normalize-loudness normalises what --corpus'),
    (CFG + ['--synth-phn-dir', 'd', '--normalize-loudness'], '--normalize-loudness normalises what --corpus'),
    (CFG + ['--corpus', '--loudness-target', '-20'], 'they need one of them'),
    (CFG + ['--loudness-peak', '-2'], 'they need one of them'),
    (CFG + ['--vocode-dir', 'd', '--loudness-max-gain', '10'], 'they need one of them'),
    (CFG + ['--loudness-out', 'b'], '--loudness-out belongs to --loudness-wav-dir'),
    (CFG + ['--loudness-wav-dir', 'a', '--loudness-out', './a'], '--loudness-out must not be the directory --loudness-wav-dir reads'),
    (['--loudness-wav-dir', 'a'], '--loudness-wav-dir needs --config'),
    (CFG + ['--loudness-wav-dir', 'a', '--normalize-loudness'], '--loudness-wav-dir does not combine with --normalize-loudness'),
    (CFG + ['--loudness-wav-dir', 'a', '--transcribe-wav-dir', 'c'], '--loudness-wav-dir does not combine with --transcribe-wav-dir'),
    (CFG + ['--loudness-wav-dir', 'a', '--trim-wav-dir', 'c', '--trim-out', 'd'], '--loudness-wav-dir does not combine with --trim-wav-dir'),
    (CFG + ['--loudness-wav-dir', 'a', '--dev-batches', '2'], '--loudness-wav-dir does not combine with --dev-batches'),
    (CFG + ['--loudness-wav-dir', 'a', '--corpus'], 'it does not combine with --loudness-wav-dir'),
]
ACCEPTED = [
    CFG + ['--corpus', '--normalize-loudness'],
    CFG + ['--unpair-wav-dir', 'd', '--normalize-loudness', '--loudness-target', '-70'],
    CFG + ['--transcribe-wav-dir', 'd', '--normalize-loudness', '--loudness-target', '0', '--loudness-peak', '0', '--loudness-max-gain', '0'],
    CFG + ['--feat-wav-dir', 'd', '--feat', 'mel', '--normalize-loudness', '--trim-silence'],
    CFG + ['--mcd-wav-dir', 'd', '--mcd-ref-dir', 'e', '--normalize-loudness'],
    CFG + ['--vocode-dir', 'd', '--normalize-loudness'],
    CFG + ['--gen-specgram', '--gen-wav', '--normalize-loudness'],
    CFG + ['--synth-phn-dir', 'd', '--gen-wav', '--normalize-loudness'],
    CFG + ['--loudness-wav-dir', 'a', '--loudness-out', 'b', '--loudness-target', '-16', '--resample', '--trim-silence', '--trim-top-db', '40'],
    CFG + ['--loudness-wav-dir', 'a'],
]
_PROBE = """
import contextlib, io, json, sys
sys.path.insert(0, %r)
import main as entry
out = []
for argv in json.loads(sys.stdin.read()):
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            p = entry.parse_args(argv + ['--no-msg'])
        out.append([0, [p.normalize_loudness, p.loudness_wav_dir, p.loudness_out, p.loudness_target, p.loudness_peak, p.loudness_max_gain]])
    except SystemExit as e:
        out.append([e.code, err.getvalue()])
print(json.dumps(out))
"""


@pytest.fixture(scope='module')
def parsed():
    """every command line of both tables through main.py's parser in ONE child process"""
    r = subprocess.run([sys.executable, '-c', _PROBE % REPO], input=json.dumps([a for a, _ in REFUSALS] + ACCEPTED), capture_output=True, text=True,
                       cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_loudness_flag_refusals(parsed):
    for (argv, msg), (code, text) in zip(REFUSALS, parsed):
        assert code == 2 and msg in text, (argv, code, text)


def test_loudness_flags_parse(parsed):
    got = parsed[len(REFUSALS):]
    assert all(code == 0 for code, _ in got), got
    assert got[0][1] == [True, None, None, -23.0, -1.0, 30.0]
    assert got[2][1] == [True, None, None, 0.0, 0.0, 0.0] and got[1][1][3] == -70.0
    assert got[8][1] == [False, 'a', 'b', -16.0, -1.0, 30.0] and got[9][1] == [False, 'a', None, -23.0, -1.0, 30.0]


def test_main_py_itself_exits_with_the_parser_error():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'main.py')] + CFG + ['--normalize-loudness', '--align-wav-dir', 'd'], capture_output=True, text=True,
                       cwd=REPO, timeout=300)
    assert r.returncode == 2 and '--normalize-loudness does not combine with --align-wav-dir' in r.stderr


def test_loudness_args_and_writer_refuse_before_writing(tmp_path):
    import types
    from semi_tts_amd import solver
    from semi_tts_amd.audio import write_wav
    assert solver.loudness_args(types.SimpleNamespace()) is None
    assert solver.loudness_args(types.SimpleNamespace(normalize_loudness=True, loudness_target=-20.0)) == dict(target=-20.0, peak_db=-1.0, max_gain_db=30.0)
    audio = dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000)
    src = tmp_path / 'in'
    src.mkdir()
    pa = types.SimpleNamespace(loudness_wav_dir=str(src), loudness_out=str(tmp_path / 'out'), loudness_target=-23.0, loudness_peak=-1.0, loudness_max_gain=30.0,
                               batch_size=4, verbose=False, resample=False)
    with pytest.raises(ValueError, match='no .wav files'):
        solver.LoudnessWriter(dict(data=dict(audio=audio)), pa, 'test').load_data()
    write_wav(str(src / 'a.wav'), np.zeros(100), 8000)
    with pytest.raises(ValueError, match='Sample rate mismatch. Expected 16000 but get 8000'):
        solver.LoudnessWriter(dict(data=dict(audio=audio)), pa, 'test').load_data()
    pa.loudness_out = str(src)
    with pytest.raises(ValueError, match='is the directory --loudness-wav-dir reads'):
        solver.LoudnessWriter(dict(data=dict(audio=audio)), pa, 'test').load_data()
    assert sorted(os.listdir(str(tmp_path))) == ['in'] and os.listdir(str(src)) == ['a.wav']
