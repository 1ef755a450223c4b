"""The alignment feature on the CPU: the build lists, every refusal of ops / metrics / main.py / StoiScorer before a device is touched,
the guards of the case table (tests/xcorr_cases.py) and the oracle (tests/xcorr_oracle.py) against numpy.correlate."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_cases as SC      # noqa: E402
import xcorr_cases as XC     # noqa: E402
import xcorr_oracle as XO    # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- build lists and signatures
def test_build_lists_and_signatures():
    import ctypes as C
    from semi_tts_amd import _lib, build
    assert build.ALIGN_SOURCES == ['xcorr.hip'] and os.path.isfile(os.path.join(build.CSRC, 'xcorr.hip')) and len(build.SOURCES) == 20
    P, I, W = C.c_void_p, C.c_int, C.POINTER(_lib.StWaveBatch)
    assert _lib.SIGNATURES['st_xcorr_workspace_bytes'] == [I, I, I] and _lib.SIGNATURES['st_sisdr_workspace_bytes'] == [I, I]
    assert _lib.SIGNATURES['st_xcorr_delay'] == [W, W, I, P, P, P, P, P]
    assert _lib.SIGNATURES['st_sisdr_batch'] == [W, W, P, I, P, P, P, P]
    assert _lib.SIGNATURES['st_wave_gather'] == [P, C.c_long, P, P, C.c_long, P, P, I, P]
    assert _lib._RESTYPES['st_xcorr_workspace_bytes'] is C.c_size_t and _lib._RESTYPES['st_sisdr_workspace_bytes'] is C.c_size_t
    header = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    for name in ('st_xcorr_delay', 'st_xcorr_workspace_bytes', 'st_sisdr_batch', 'st_sisdr_workspace_bytes', 'st_wave_gather'):
        assert name + '(' in header


def test_constants():
    from semi_tts_amd import ops
    assert (ops.XCORR_MAX_BATCH, ops.XCORR_MAX_LAG, ops.XCORR_MAX_LEN) == (64, 16384, 1 << 22)
    assert ops.XCORR_LAG_TILE % 64 == 0 and ops.XCORR_CHUNK % 8 == 0
    M, C = ops.XCORR_MAX_CHUNKS, ops.XCORR_CHUNK
    assert [ops.xcorr_chunk_len(L) for L in (1, C, M * C, M * C + 1, 2 * M * C, 2 * M * C + 1, ops.XCORR_MAX_LEN)] == \
        [C, C, C, 2 * C, 2 * C, 3 * C, ops.XCORR_MAX_LEN // M]
    # the partial sums of the largest call stay modest: 64 pairs, 2^22 samples, +-16384 lags
    assert 64 * M * (2 * ops.XCORR_MAX_LAG + 1) * 8 < 600e6


# ---------------------------------------------------------------- refusals before a device is touched
@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to pick a device fails the test"""
    from semi_tts_amd import _lib, audio

    def touched(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(_lib, 'load', touched)
    monkeypatch.setattr(audio, '_device', touched)


def test_ops_refuse_before_a_device(no_device):
    import torch
    from semi_tts_amd import ops
    x = torch.zeros(100)
    one = np.array([100])
    for lens, msg in ((np.ones(65, np.int64), 'one call takes no more pairs'), (np.array([0]), r'must lie in \[1, 4194304\]'),
                      (np.array([ops.XCORR_MAX_LEN + 1]), r'must lie in \[1, 4194304\]'), (np.array([2.0]), 'one call takes no more pairs')):
        for what, fn in (('xcorr_delay', lambda a, b: ops.xcorr_delay(x, [0], a, x, [0], b, 1)), ('sisdr_batch', lambda a, b: ops.sisdr_batch(x, [0], a, x, [0], b))):
            with pytest.raises(ValueError, match=what + '.*' + msg):
                fn(lens, lens)
            if len(lens) == 1:
                with pytest.raises(ValueError, match=what + '.* of y .*' + msg):
                    fn(one, lens)
    with pytest.raises(ValueError, match='2 references and 1 processed'):
        ops.xcorr_delay(x, [0, 0], np.array([5, 5]), x, [0], one, 1)
    for lag in (-1, ops.XCORR_MAX_LAG + 1, 1.0, True, None):
        with pytest.raises(ValueError, match=r'max_lag must be an integer in \[0, 16384\]'):
            ops.xcorr_delay(x, [0], one, x, [0], one, lag)
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.xcorr_delay(x, [0], one, x, [0], one, 1)
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.sisdr_batch(x, [0], one, x, [0], one)
    with pytest.raises(ValueError, match='delay must be None or a contiguous'):
        ops.sisdr_batch(x, [0], one, x, [0], one, delay=3)
    with pytest.raises(ValueError, match=r'lens must be 0 .. 64 integers in \[1, 4194304\]'):
        ops.wave_gather(x, [0], x.clone(), [0], [0])
    with pytest.raises(ValueError, match=r'lens must be 0 .. 64 integers'):
        ops.wave_gather(x, np.zeros(65, np.int64), x.clone(), np.zeros(65, np.int64), np.ones(65, np.int64))
    with pytest.raises(ValueError, match='src_off and dst_off must hold 1 integers'):
        ops.wave_gather(x, [0, 1], x.clone(), [0], [5])
    with pytest.raises(ValueError, match='src must be a contiguous 1-D float32 GPU tensor'):
        ops.wave_gather(x, [0], x.clone(), [0], [5])


def test_metrics_refuse_before_a_device(no_device):
    import torch
    from semi_tts_amd import metrics, ops
    a, b = np.zeros(500, np.float32), np.zeros(400, np.float32)
    for who, fn in (('delay', lambda c, d: metrics.delay(c, d, 5)), ('si_sdr', lambda c, d: metrics.si_sdr(c, d)),
                    ('align_pairs', lambda c, d: metrics.align_pairs(c, d, 5))):
        with pytest.raises(ValueError, match=who + ': 2 clean and 1 processed signals'):
            fn([a, a], [b])
        with pytest.raises(ValueError, match=who + ': clean is an empty batch'):      # (the messages name the function that was called)
            fn([], [])
        with pytest.raises(ValueError, match=who + r': clean\[0\] must be a non-empty 1-D floating point or int16'):
            fn([np.zeros(0, np.float32)], [b])
        with pytest.raises(ValueError, match=who + r': degraded\[0\] must be a non-empty 1-D floating point or int16'):
            fn([a], [np.zeros((2, 50), np.float32)])
        with pytest.raises(ValueError, match=who + ': degraded must be a list of 1-D waveforms or a WaveBatch'):
            fn([a], 5)
        with pytest.raises(ValueError, match=who + ': the longest signal has .* above the limit of %d' % ops.XCORR_MAX_LEN):
            fn([a], [torch.zeros(ops.XCORR_MAX_LEN + 1)])
    for lag in (-1, ops.XCORR_MAX_LAG + 1, 2.5, True, None):
        with pytest.raises(ValueError, match=r'delay: max_lag must be an integer in \[0, 16384\]'):
            metrics.delay([a], [b], lag)
        with pytest.raises(ValueError, match=r'align_pairs: max_lag must be an integer'):
            metrics.align_pairs([a], [b], lag)
    for d in (1.5, True, 'x', 2 ** 31):
        with pytest.raises(ValueError, match='si_sdr: delay must be None, an int or the device tensor'):
            metrics.si_sdr([a], [b], d)
    with pytest.raises(ValueError, match=r'si_sdr: a delay tensor must be int32 of shape \(1,\) on the device'):
        metrics.si_sdr([a], [b], torch.zeros(1, dtype=torch.int32))
    assert metrics.overlap(100, 90, 0) == (0, 0, 90) and metrics.overlap(100, 90, 20) == (0, 20, 70) and metrics.overlap(100, 90, -20) == (20, 0, 80)
    assert metrics.overlap(100, 90, 95)[2] == -5


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


def test_flags_parse():
    entry = _entry()
    base = ['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b']
    p = entry.parse_args(base)
    assert (p.stoi_align, p.stoi_sdr, p.stoi_max_delay, p.stoi_max_len_diff) == (False, False, None, 0.05)
    p = entry.parse_args(base + ['--stoi-align'])
    assert (p.stoi_align, p.stoi_sdr, p.stoi_max_delay) == (True, False, 0.05)
    p = entry.parse_args(base + ['--stoi-align', '--stoi-max-delay', '0', '--stoi-sdr'])
    assert (p.stoi_align, p.stoi_sdr, p.stoi_max_delay) == (True, True, 0.0)
    p = entry.parse_args(base + ['--stoi-sdr'])
    assert (p.stoi_align, p.stoi_sdr, p.stoi_max_delay) == (False, True, None)


@pytest.mark.parametrize('argv, msg', [
    (['--config', 'x.yaml', '--stoi-align'], '--stoi-align, --stoi-max-delay and --stoi-sdr belong to --stoi-wav-dir; they need that flag'),
    (['--config', 'x.yaml', '--stoi-sdr'], '--stoi-align, --stoi-max-delay and --stoi-sdr belong to --stoi-wav-dir'),
    (['--config', 'x.yaml', '--stoi-max-delay', '0.1'], '--stoi-align, --stoi-max-delay and --stoi-sdr belong to --stoi-wav-dir'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-max-delay', '0.1'], '--stoi-max-delay belongs to --stoi-align; it needs that flag'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-align', '--stoi-max-delay', '-0.1'], '--stoi-max-delay must be finite and at least 0'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-align', '--stoi-max-delay', 'inf'], '--stoi-max-delay must be finite and at least 0'),
    (['--stoi-wav-dir', 'a', '--stoi-ref-dir', 'b', '--stoi-align', '--stoi-max-delay', 'nan'], '--stoi-max-delay must be finite and at least 0'),
    (['--stoi-wav-dir', 'a', '--stoi-align'], '--stoi-wav-dir needs --stoi-ref-dir DIR'),
])
def test_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


# ---------------------------------------------------------------- solver.StoiScorer.load_data on files in tmp_path
def _paras(tmp_path, **kw):
    d = dict(stoi_wav_dir=str(tmp_path / 'syn'), stoi_ref_dir=str(tmp_path / 'ref'), stoi_max_len_diff=0.05, batch_size=2, name='run',
             logdir=str(tmp_path / 'log'), verbose=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_scorer_checks_the_new_flags_in_load_data(tmp_path, no_device):
    from semi_tts_amd import ops
    from semi_tts_amd.audio import write_wav
    from semi_tts_amd.solver import StoiScorer
    (tmp_path / 'syn').mkdir()
    (tmp_path / 'ref').mkdir()
    c = SC.by_name('L7000/snr5')
    write_wav(str(tmp_path / 'syn' / 'a.wav'), c['y'][:6200], 10000)                   # 800 samples = 0.08 s shorter
    write_wav(str(tmp_path / 'ref' / 'a.wav'), c['x'], 10000)
    load = lambda **kw: StoiScorer(None, _paras(tmp_path, **kw), 'test').load_data()      # noqa: E731
    with pytest.raises(ValueError, match=r'a\.wav has 6200 samples and its recording .*a\.wav 7000: they differ by 0\.0800 s, above --stoi-max-len-diff 0\.05; '):
        load()                                                                      # (without the flags: the message of before)
    with pytest.raises(ValueError, match=r'they differ by 0\.0800 s, above --stoi-max-len-diff 0\.05 plus --stoi-max-delay 0\.02'):
        load(stoi_align=True, stoi_max_delay=0.02)
    s = load(stoi_align=True, stoi_max_delay=0.03)                                  # 0.05 + 0.03 covers it
    assert s.align and not s.sdr and s.lens == [(6200, 7000)] and s.samples == [6200] and s.lag(10000) == 300
    s = load(stoi_align=True)                                                       # the default bound: 0.05 s
    assert s.max_delay == 0.05 and s.lag(10000) == 500 and s.lag(22050) == 1102
    big = (ops.XCORR_MAX_LAG + 1) / 10000.0
    with pytest.raises(ValueError, match=r'--stoi-align: .*a\.wav is at 10000 Hz: --stoi-max-delay %g must be finite, at least 0 and at most 16384 samples = 1\.6384 s' % big):
        load(stoi_align=True, stoi_max_delay=big)
    assert load(stoi_align=True, stoi_max_delay=ops.XCORR_MAX_LAG / 10000.0).lag(10000) == ops.XCORR_MAX_LAG
    for bad in (-0.01, float('inf'), float('nan')):
        with pytest.raises(ValueError, match=r'--stoi-align: .*a\.wav is at 10000 Hz: --stoi-max-delay'):
            load(stoi_align=True, stoi_max_delay=bad)
    s = StoiScorer(None, _paras(tmp_path, stoi_max_len_diff=0.1), 'test')           # paras without the new attributes: all off
    assert (s.align, s.sdr, s.max_delay) == (False, False, 0.0) and s.load_data().samples == [6200]
    assert load(stoi_sdr=True, stoi_max_len_diff=0.1).sdr
    assert not (tmp_path / 'log').exists()


# ---------------------------------------------------------------- the case table's own guards
def test_guard_the_shapes_straddle_the_constants():
    C, T, M = XC.C, XC.T, XC.M
    lens = {len(c['x']) for c in XC.CASES} | {len(c['y']) for c in XC.CASES}
    assert {1, 2, C - 1, C, C + 1, 2 * C + 1, M * C, M * C + 1} <= lens
    assert {0, 1, T - 1, T, T + 1} <= {c['D'] for c in XC.CASES}
    assert any(len(c['x']) > len(c['y']) for c in XC.CASES) and any(len(c['x']) < len(c['y']) for c in XC.CASES)
    assert any(c['D'] > max(len(c['x']), len(c['y'])) for c in XC.CASES)
    planted = {(c['shift'], c['D']) for c in XC.CASES if c['shift'] is not None}
    assert {0, 1, -1} <= {s for s, _ in planted} and any(s == D > 0 for s, D in planted) and any(s == -D < 0 for s, D in planted)
    assert sum(not c['pcm'] and not c['nan'] for c in XC.CASES) >= 4 and sum(c['nan'] for c in XC.CASES) == 1 and sum(c['dc'] for c in XC.CASES) == 1


def test_guard_pcm_cases_are_pcm_and_every_planted_delay_is_found():
    for c in XC.CASES:
        assert (XO.is_pcm(c['x']) and XO.is_pcm(c['y'])) == c['pcm'], c['name']
        o = XC.oracle(c)
        if c['shift'] is not None:
            assert o['delay'] == c['shift'], (c['name'], o['delay'])
    assert XC.oracle(XC.by_name('tie/+-2'))['corr'][2] == XC.oracle(XC.by_name('tie/+-2'))['corr'][6] > 0
    assert XC.oracle(XC.by_name('negative'))['corr'].max() == 0.0
    assert np.isnan(XC.oracle(XC.by_name('zero-x'))['coef']) and XC.oracle(XC.by_name('nan-x'))['delay'] == 0


def test_guard_every_float_case_keeps_its_gap():
    """no exemption: the oracle's decision cannot flip under the float64 bound of the GPU test"""
    n = 0
    for c in XC.CASES:
        if not c['pcm'] and not c['nan']:
            r = XC.oracle(c)['corr']
            assert XO.gap(r, c['D']) >= XC.GAP, (c['name'], XO.gap(r, c['D']))
            s, k = XO.corr_abs(c['x'], c['y'], c['D'])
            assert (k * 2.0 ** -53 * s).max() < 0.01 * XC.GAP * abs(r).max(), c['name']      # the bound is far inside the gap
            n += 1
    assert n >= 4


def test_guard_every_zero_mean_case_has_a_small_mean_but_the_marked_one():
    seen_dc = False
    for c in XC.CASES:
        if not c['zero_mean']:
            continue
        n, sx, _, sxx, _, _ = XO.sums(c['x'], c['y'], XC.oracle(c)['delay'])
        share = (sx * sx / n) / sxx
        if c['dc']:
            seen_dc = True
            assert share > 0.5, (c['name'], share)
        else:
            assert share <= XC.MEAN_SHARE, (c['name'], share)
    assert seen_dc


def test_guard_pcm_scores_stay_under_60_db():
    """the GPU test's score tolerance holds for cases under 60 dB (the cancellation in Cxx Cyy - Cxy^2)"""
    for c in XC.CASES:
        if c['pcm']:
            for zm in ((False, True) if c['zero_mean'] else (False,)):
                v = XO.scores(XO.sums(c['x'], c['y'], XC.oracle(c)['delay']), zm)
                assert not np.isfinite(v[0]) or v[0] < 60.0, (c['name'], zm, v)


# ---------------------------------------------------------------- the oracle against numpy
@pytest.mark.parametrize('name', ['Lx>Ly/+D', 'Lx<Ly/-D', 'f/Lx>Ly/+D'])
def test_oracle_agrees_with_numpy_correlate(name):
    c = XC.by_name(name)
    x, y, D = c['x'].astype(np.float64), c['y'].astype(np.float64), c['D']
    full = np.correlate(y, x, 'full')                       # full[k] = sum_n y[n + k - (Lx - 1)] x[n]
    want = full[len(x) - 1 - D:len(x) + D]
    got = XC.oracle(c)['corr']
    assert got.shape == want.shape
    s, k = XO.corr_abs(x, y, D)
    assert (np.abs(got - want) <= k * 2.0 ** -53 * s).all()          # (numpy.correlate sums in float64; the oracle's own error is far smaller)
    assert int(np.argmax(want)) - D == XC.oracle(c)['delay']


def test_oracle_scores_on_a_scaled_copy():
    x = XC.by_name('Lx>Ly/+D')['x']
    s = XO.sums(x, 0.5 * x, 0)
    v = XO.scores(s, False)
    assert v[0] == np.inf and abs(v[1] - 6.0206) < 1e-4 and abs(v[2] + 6.0206) < 1e-4
    v = XO.scores(XO.sums(np.zeros(50, np.float32), x[:50], 0), True)        # a silent reference: 0 / 0 in SI-SDR and gain, log10(0) in SNR
    assert np.isnan(v[0]) and v[1] == -np.inf and np.isnan(v[2])
    assert (XO.sums(x, x, len(x) + 5) == 0).all() and np.isnan(XO.scores(XO.sums(x, x, len(x) + 5), True)).all()
