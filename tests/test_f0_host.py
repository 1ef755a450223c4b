"""CPU checks of the pitch feature: the numpy oracle on closed forms, its robust share on the GPU tests' signals, path_scores on hand-made
tracks, the exported symbols, every refusal of st_f0_yin and of ops.f0_yin / ops.f0_path_scores (they fire before any device is
touched), the lag range derived from fmin / fmax, and the main.py flag rules."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import f0_oracle as O  # noqa: E402


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('p', [20, 25, 37])
def test_oracle_pure_sine_of_integer_period(p):
    """tau* = p on every frame that is all signal, and f0 within the refinement's half lag of sr / p, inside its own interval.
    (The parabola runs on d', whose factor tau / c(tau) is not symmetric about p: at p = 20, W = 80 it gives a / c = 0.907,
    delta = -0.0245 and f0 = 100.122 Hz for the 100 Hz sine -- the definition's bias, 2 cents, not an error of the oracle; so the
    distance to sr / p is bounded by the half lag, not by the width of the rounding interval, which is 1.6e-4 Hz here.)"""
    sr, hop, W, tau_min, tau_max = 2000, 20, 80, 5, 40
    x = np.sin(2 * np.pi * np.arange(1000) / p)
    o = O.yin(x, sr, hop, W, tau_min, tau_max, 0.15)
    inner = slice(3, 1 + 1000 // hop - 8)                           # frames whose W + tau_max samples are all signal
    assert (o['tau'][inner] == p).all()
    assert (np.abs(o['f0'][inner] - sr / p) < sr / (p - 0.5) - sr / p).all()
    assert (np.abs(o['f0'][inner] - sr / p) < 0.005 * sr / p).all()                    # within 9 cents
    assert (o['f0_lo'][inner] <= o['f0'][inner]).all() and (o['f0'][inner] <= o['f0_hi'][inner]).all()
    assert (o['f0_hi'][inner] - o['f0_lo'][inner] < 1e-3).all() and o['robust'][inner].all()
    assert (o['aper'][inner] < 1e-9).all()


def test_oracle_zeros_noise_and_octave():
    sr, hop, W, tau_min, tau_max = 2000, 20, 80, 5, 40
    o = O.yin(np.zeros(500), sr, hop, W, tau_min, tau_max, 0.15)
    assert (o['tau'] == 0).all() and (o['f0'] == 0).all() and (o['aper'] == 1.0).all() and o['robust'].all()
    o = O.yin(np.random.RandomState(0).randn(2000), sr, hop, W, tau_min, tau_max, 0.15)
    assert (o['tau'] == 0).all() and (o['f0'] == 0).all() and (o['aper'] > 0.15).all()
    # a 5-harmonic 110 Hz tone at 22050 Hz: the period of 110 Hz (200.45 samples), not of 220 or 55
    sr, hop, tau_min, tau_max = 22050, 220, 44, 368
    x = O.harmonic(np.full(8000, 110.0), sr)
    o = O.yin(x, sr, hop, 2 * tau_max, tau_min, tau_max, 0.15)
    inner = slice(3, 1 + 8000 // hop - 6)
    assert set(o['tau'][inner].tolist()) <= {200, 201}
    assert (np.abs(o['f0'][inner] - 110.0) < 0.2).all()


def test_oracle_frames_and_padding():
    assert O.frame_count(1, 20) == 1 and O.frame_count(19, 20) == 1 and O.frame_count(20, 20) == 2
    s = O.slices(np.arange(1.0, 8.0), 3, 4, 2)
    assert s.shape == (3, 6)
    assert s[0].tolist() == [0, 0, 1, 2, 3, 4] and s[1].tolist() == [2, 3, 4, 5, 6, 7] and s[2].tolist() == [5, 6, 7, 0, 0, 0]
    assert O.eps(736, 368) == (2 * 736 + 368 + 8) * 2.0 ** -24


@pytest.mark.parametrize('framing', sorted(O.FRAMINGS))
def test_signals_are_robust_and_float32_agrees(framing):
    """the share of non-robust frames of every GPU test signal is at most 2 % (the GPU tests cap it at 5 %), and a float32 numpy
    evaluation of the definition gives the oracle's decision on every robust frame, inside its interval"""
    sr, hop, tau_min, tau_max, W, n = O.FRAMINGS[framing]
    for name in O.SIGNALS:
        x = O.signal(name, framing)
        assert x.dtype == np.float32 and x.shape == (n,)
        o = O.yin(x, sr, hop, W, tau_min, tau_max, 0.15)
        r = o['robust']
        assert (~r).mean() <= 0.02, (name, int((~r).sum()))
        f0, aper, tau = O.yin_f32(x, sr, hop, W, tau_min, tau_max, 0.15)
        assert (tau[r] == o['tau'][r]).all(), name
        assert ((f0[r] >= o['f0_lo'][r]) & (f0[r] <= o['f0_hi'][r])).all(), name
        assert (np.abs(aper[r] - o['aper'][r]) <= 2 * O.eps(W, tau_max) * o['aper'][r]).all(), name
    voiced = O.yin(O.signal('tone', framing), sr, hop, W, tau_min, tau_max, 0.15)['tau'] > 0
    assert voiced.mean() > 0.9


def test_path_scores_on_hand_made_tracks():
    nan = float('nan')
    fx = [100.0, 200.0, 0.0, nan, 100.0, 150.0]
    fy = [100.0, 100.0, 100.0, 0.0, nan, 125.0]
    path = [[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [-1, -1]]
    counts, s2, s1, sa = O.path_scores(fx, fy, path, 6)
    # pairs 0, 1, 5 are both voiced; 2 and 4 differ in voicing; 3 is unvoiced on both sides (NaN counts as unvoiced)
    assert counts == (6, 3, 2, 1)                                   # gross: 200 vs 100; 150 vs 125 is not (25 > 0.2 * 125 = 25 is false)
    c5 = 1200.0 * math.log2(150.0 / 125.0)
    assert abs(s1 - (1200.0 + c5)) < 1e-9 and abs(s2 - (1200.0 ** 2 + c5 ** 2)) < 1e-6 and abs(sa - s1) < 1e-9
    counts, s2, s1, _ = O.path_scores(fy, fx, [[1, 1], [0, 0], [5, 5]], 3)
    assert counts == (3, 3, 0, 1) and abs(s1 + 1200.0 + c5) < 1e-9   # the other way round: 100 vs 200 is 50 % off, 125 vs 150 is not
    assert O.path_scores(fx, fy, path, 0) == ((0, 0, 0, 0), 0.0, 0.0, 0.0)
    assert O.path_scores(fx, fy, [[0, 1], [0, 2], [1, 2]], 3)[0] == (3, 3, 0, 1)


# ---------------------------------------------------------------- the library
def test_library_exports_and_header():
    from semi_tts_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(REPO, 'include', 'semitts.h')).read()
    for name, n_args in (('st_f0_yin', 11), ('st_f0_path_scores', 13), ('st_f0_run_length', 3)):
        assert hasattr(lib, name) and name + '(' in hdr
        assert len(_lib.SIGNATURES[name]) == n_args
    assert 'st_f0_yin' in _lib.check_header_symbols()
    from semi_tts_amd import build
    assert build.PITCH_SOURCES == ['f0.hip'] and os.path.exists(os.path.join(build.CSRC, 'f0.hip'))


def test_run_length_matches_the_library():
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    assert ops.f0_run_length(220, 736, 368) == ops.F0_RUN == lib.st_f0_run_length(220, 736, 368)
    for hop, W, tau_max in ((20, 80, 40), (7, 63, 65), (1, 1, 3), (1024, 2048, 1024), (1100, 2048, 1024), (1500, 80, 40), (5000, 80, 40),
                            (20000, 2048, 1024), (2 ** 30, 80, 40)):
        r = lib.st_f0_run_length(hop, W, tau_max)
        assert r == ops.f0_run_length(hop, W, tau_max) and 1 <= r <= ops.F0_RUN
        assert r == 1 or (r - 1) * hop + W + tau_max <= ops.F0_MAX_SPAN
    assert lib.st_f0_run_length(0, 80, 40) == 0 and lib.st_f0_run_length(20, 2049, 40) == 0 and lib.st_f0_run_length(20, 80, 1025) == 0


def test_c_entry_refuses_each_limit_without_a_device():
    """the limit checks precede the launch: -22 and a message naming the entry point, with pointers that are never dereferenced"""
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(B=1, length=100, off=0, n_samples=1000, hop=20, W=80, tau_min=5, tau_max=40, sr=2000.0, thr=0.15, T_pad=6, x=p, f0=p):
        offs, lens = (ctypes.c_long * 64)(*([off] * 64)), (ctypes.c_int * 64)(*([length] * 64))
        w = _lib.StWaveBatch(x=x, n_samples=n_samples, off=ctypes.addressof(offs), len=ctypes.addressof(lens), B=B)
        return lib.st_f0_yin(ctypes.byref(w), hop, W, tau_min, tau_max, sr, thr, f0, None, T_pad, None)
    cases = [dict(B=0), dict(B=65), dict(length=0), dict(hop=0), dict(tau_min=1), dict(tau_min=40), dict(tau_min=41), dict(tau_max=1025, W=80),
             dict(W=0), dict(W=2049), dict(T_pad=5), dict(thr=0.0), dict(thr=-0.1), dict(thr=1.0000001), dict(thr=float('nan')),
             dict(thr=float('inf')), dict(sr=0.0), dict(sr=-1.0), dict(sr=float('inf')), dict(sr=float('nan')), dict(x=None), dict(f0=None),
             dict(off=-1), dict(off=901)]
    for kw in cases:
        assert call(**kw) == -22, kw
        assert b'st_f0_yin' in lib.st_last_error()
    ip = ctypes.addressof((ctypes.c_int * 64)())

    def scores(B=1, Tx=4, Ty=4, P=7, x_sb=4, y_sb=4, fx=p, path=ip, counts=ip):
        return lib.st_f0_path_scores(fx, x_sb, Tx, p, y_sb, Ty, path, ip, B, P, counts, p, None)
    for kw in (dict(B=0), dict(Tx=0), dict(Ty=0), dict(P=0), dict(x_sb=-1), dict(y_sb=-4), dict(fx=None), dict(path=None), dict(counts=None)):
        assert scores(**kw) == -22, kw
        assert b'st_f0_path_scores' in lib.st_last_error()


# ---------------------------------------------------------------- ops argument checks
def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def _meta_is_cuda(monkeypatch):
    # the checks read .is_cuda / .device / .shape / .dtype / .stride() only: a meta tensor stands in for a device tensor
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))


def test_f0_yin_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops
    _no_device(monkeypatch)
    good = dict(off=[0, 100], lens=[100, 60], hop=20, W=80, tau_min=5, tau_max=40, sample_rate=2000.0, threshold=0.15, T_pad=6)
    with pytest.raises(ValueError, match='GPU tensor'):
        ops.f0_yin(torch.zeros(160), **good)
    _meta_is_cuda(monkeypatch)
    x = torch.zeros(160, device='meta')
    cases = [
        (dict(hop=0), 'hop'), (dict(hop=2.5), 'hop must be an integer'),
        (dict(tau_min=1), 'tau_min < tau_max'), (dict(tau_min=40), 'tau_min < tau_max'), (dict(tau_max=1025), '<= 1024'),
        (dict(W=0), r'outside \[1, 2048\]'), (dict(W=2049), r'outside \[1, 2048\]'),
        (dict(threshold=0.0), 'threshold'), (dict(threshold=1.01), 'threshold'), (dict(threshold=float('nan')), 'threshold'),
        (dict(sample_rate=0.0), 'sample_rate'), (dict(sample_rate=float('inf')), 'sample_rate'), (dict(sample_rate=float('nan')), 'sample_rate'),
        (dict(lens=[100, 0]), 'lens'), (dict(lens=[], off=[]), 'lens'), (dict(lens=[100.0, 60.0]), 'lens'),
        (dict(off=[0, 101]), 'outside the 160 packed samples'), (dict(off=[-1, 100]), 'outside the 160 packed samples'), (dict(off=[0]), 'outside'),
        (dict(T_pad=5), 'T_pad 5 below the 6 frames'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.f0_yin(x, **dict(good, **kw))
    for bad in (x.double(), x.reshape(2, 80), torch.zeros(320, device='meta')[::2]):
        with pytest.raises(ValueError, match='packed 1-D contiguous float32'):
            ops.f0_yin(bad, **good)
    # arguments the kernel takes get as far as the library (and no further here)
    for kw in (dict(), dict(tau_min=2, tau_max=1024, W=2048), dict(threshold=1.0, W=1), dict(T_pad=9), dict(hop=1, T_pad=101)):
        with pytest.raises(AssertionError, match='reached the device'):
            ops.f0_yin(x, **dict(good, **kw))


def test_f0_path_scores_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import metrics, ops
    _no_device(monkeypatch)
    fx, fy = torch.zeros(2, 5), torch.zeros(2, 6)
    path, plen = torch.zeros(2, 10, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match='f0_x must be'):
        ops.f0_path_scores(fx, fy, path, plen)
    _meta_is_cuda(monkeypatch)
    fx, fy, path, plen = (t.to('meta') for t in (fx, fy, path, plen))
    cases = [
        ((fx, torch.zeros(2, 6), path, plen), 'f0_y must be'),
        ((fx.double(), fy, path, plen), 'f0_x must be'),
        ((fx[0], fy, path, plen), 'f0_x must be'),
        ((fx, fy[:1], path, plen), 'pairs'),
        ((fx[:0], fy[:0], path[:0], plen[:0]), 'pairs'),
        ((fx[:, :0], fy, path, plen), 'pairs'),
        ((torch.zeros(2, 10, device='meta')[:, ::2], fy, path, plen), 'unit stride'),
        ((fx, fy, path[:, :9], plen), r'\(2, 10, 2\)'),
        ((fx, fy, path.long(), plen), 'path must be'),
        ((fx, fy, torch.zeros(2, 10, 2, dtype=torch.int32), plen), 'path must be'),
        ((fx, fy, torch.zeros(2, 10, 4, dtype=torch.int32, device='meta')[:, :, ::2], plen), 'path must be'),
        ((fx, fy, None, plen), 'path must be'),
        ((fx, fy, path, plen.long()), 'path_len must be'),
        ((fx, fy, path, plen[:1]), 'path_len must be'),
        ((fx, fy, path, [3, 4]), 'path_len must be'),
    ]
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.f0_path_scores(*args)
    with pytest.raises(ValueError, match='path must be'):
        metrics.f0_scores(fx, fy, path[:, :3], plen)
    wide = torch.zeros(2, 40, device='meta')
    for args in ((fx, fy, path, plen), (wide[:, 3:8], wide[:, 10:16], path, plen)):        # a column window keeps its row stride
        with pytest.raises(AssertionError, match='reached the device'):
            ops.f0_path_scores(*args)
    with pytest.raises(AssertionError, match='reached the device'):
        metrics.f0_scores(fx, fy, path, plen)
    assert 'metrics.dtw' in ops.f0_path_scores.__doc__


# ---------------------------------------------------------------- the converter
def _converter():
    import yaml
    from semi_tts_amd.audio import load_audio_transform
    config = yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
    return load_audio_transform(**dict(config['data']['audio'])), config


def test_lags_from_fmin_fmax(monkeypatch):
    from semi_tts_amd import audio
    conv, _ = _converter()
    sr = conv.sr
    assert conv.f0_lags() == (sr // 500, -(-sr // 60), 2 * -(-sr // 60))
    if sr == 22050:
        assert conv.f0_lags() == (44, 368, 736) and conv.hop_length_mfcc == 220
    assert conv.f0_lags(100., 400., window=300) == (int(math.floor(sr / 400.)), int(math.ceil(sr / 100.)), 300)
    assert conv.f0_lags(sr / 1024.0, sr / 2.0)[:2] == (2, 1024)                # both limits, exactly
    for kw, msg in ((dict(fmin=sr / 1025.0), 'tau_max <= 1024'), (dict(fmax=sr / 1.9), 'tau_min >= 2'), (dict(fmin=0.0), '0 < fmin < fmax'),
                    (dict(fmin=500., fmax=60.), '0 < fmin < fmax'), (dict(fmin=400., fmax=400.), '0 < fmin < fmax'),
                    (dict(window=2049), 'W <= 2048'), (dict(window=0), '1 <= W'), (dict(fmin=float('nan')), 'fmin')):
        with pytest.raises(ValueError, match=msg):
            conv.f0_lags(**kw)
    # extract_f0_batch refuses before the device
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    wav = [torch.zeros(3000)]
    with pytest.raises(ValueError, match='tau_max <= 1024'):
        conv.extract_f0_batch(wav, fmin=10.)
    with pytest.raises(ValueError, match='threshold'):
        conv.extract_f0_batch(wav, threshold=0.0)
    with pytest.raises(ValueError, match='lens'):
        conv.extract_f0_batch([torch.zeros(0)])
    with pytest.raises(AssertionError, match='reached the device'):
        conv.extract_f0_batch(wav)
    with pytest.raises(AssertionError, match='reached the device'):
        conv.extract_f0_from_waveform(torch.zeros(2, 3000), channel=1)


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'config/supervised.yaml']
_MCD = ['--mcd-wav-dir', 'syn', '--mcd-ref-dir', 'ref']
_FEAT = ['--feat-wav-dir', 'd']


def test_f0_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + _FEAT + ['--feat', 'f0'])
    assert (p.feat, p.f0_min, p.f0_max, p.f0_threshold, p.mcd_f0) == ('f0', 60.0, 500.0, 0.15, False)
    p = entry.parse_args(CFG + _FEAT + ['--feat', 'f0', '--f0-min', '80', '--f0-max', '400', '--f0-threshold', '0.1'])
    assert (p.f0_min, p.f0_max, p.f0_threshold) == (80.0, 400.0, 0.1)
    p = entry.parse_args(CFG + _MCD + ['--mcd-f0', '--f0-max', '450'])
    assert p.mcd_f0 is True and p.mcd_path is False and (p.f0_min, p.f0_max, p.f0_threshold) == (60.0, 450.0, 0.15)
    p = entry.parse_args(CFG + _MCD)
    assert p.mcd_f0 is False and (p.f0_min, p.f0_max, p.f0_threshold) == (60.0, 500.0, 0.15)


_F0_NEED = '--f0-min, --f0-max and --f0-threshold set the pitch tracker of --feat f0 and --mcd-f0; they need one of them'


@pytest.mark.parametrize('argv,msg', [
    (CFG + ['--f0-min', '70'], _F0_NEED),
    (CFG + _MCD + ['--f0-max', '400'], _F0_NEED),
    (CFG + _FEAT + ['--feat', 'mfcc', '--f0-threshold', '0.2'], _F0_NEED),
    (CFG + ['--mcd-f0'], '--mcd-f0 belongs to --mcd-wav-dir'),
    (CFG + _FEAT + ['--feat', 'mfcc', '--mcd-f0'], '--mcd-f0 belongs to --mcd-wav-dir'),
    (CFG + _FEAT + ['--feat', 'f0', '--f0-min', '500', '--f0-max', '60'], '0 < --f0-min < --f0-max'),
    (CFG + _FEAT + ['--feat', 'f0', '--f0-min', '0'], '0 < --f0-min < --f0-max'),
    (CFG + _MCD + ['--mcd-f0', '--f0-threshold', '1.5'], '0 < --f0-threshold <= 1'),
    (CFG + _MCD + ['--mcd-f0', '--f0-threshold', '0'], '0 < --f0-threshold <= 1'),
    (CFG + _FEAT + ['--feat', 'pitch'], 'invalid choice'),
    (CFG + ['--feat', 'f0'], '--feat, --segment-file and --min-segment-len belong to --feat-wav-dir'),
])
def test_f0_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


def test_feature_writer_refuses_segments_and_bad_range_before_writing(tmp_path, monkeypatch):
    from semi_tts_amd import audio, solver
    from semi_tts_amd.audio import write_wav
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    _, config = _converter()
    sr = config['data']['audio']['sample_rate']
    wavs = tmp_path / 'wav'
    wavs.mkdir()
    write_wav(str(wavs / 'a.wav'), 0.1 * np.random.RandomState(0).randn(sr // 2), sr)
    (tmp_path / 'segments.csv').write_text('file,seg\na,0.5\n')

    class P:
        feat_wav_dir, feat, name, logdir, batch_size = str(wavs), 'f0', 'f0', str(tmp_path / 'log'), 4
        segment_file, min_segment_len, f0_min, f0_max, f0_threshold = str(tmp_path / 'segments.csv'), 2, 60.0, 500.0, 0.15
    with pytest.raises(ValueError, match='--feat f0 does not combine with --segment-file'):
        solver.FeatureWriter(config, P(), 'test').load_data()
    P.segment_file = None
    P.f0_min = 10.0
    with pytest.raises(ValueError, match='tau_max <= 1024'):
        solver.FeatureWriter(config, P(), 'test').load_data()
    P.f0_min = 60.0
    fw = solver.FeatureWriter(config, P(), 'test')
    assert fw.load_data() is fw and fw.f0_args == dict(fmin=60.0, fmax=500.0, threshold=0.15)
    assert not os.path.exists(P.logdir)                             # nothing is written before exec

    class M:
        mcd_wav_dir, mcd_ref_dir, mcd_path, mcd_f0, name, logdir, batch_size = str(wavs), str(wavs), False, True, 'm', str(tmp_path / 'log'), 4
        f0_min, f0_max, f0_threshold = 60.0, 20000.0, 0.15
    with pytest.raises(ValueError, match='tau_min >= 2'):
        solver.McdScorer(config, M(), 'test').load_data()
    assert solver.F0_HEADER == 'file,path_len,voiced_pairs,f0_rmse_cents,vuv_error,gross_error,mean_cents'
