"""CPU side of the Griffin-Lim vocoder (semi_tts_amd.audio): the fp64 oracle's own consistency, the blocked form of the inverse
pre-emphasis the final kernel uses, argument checks that fire before any device is touched, the .wav writer and the --gen-wav flag."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_oracle as O   # noqa: E402

AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


def _signal(B, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 22050
    f0 = 110 + 200 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    return 0.5 * torch.sin(2 * np.pi * f0 * t) + 0.05 * torch.randn(B, L, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('T', [5, 43, 258])
def test_oracle_istft_inverts_stft(T):
    x = _signal(2, O.HOP * (T - 1))
    y = O.stft(x)
    assert y.shape == (2, O.N_FFT // 2 + 1, T)
    assert torch.allclose(O.istft(y), x, atol=1e-10)


def test_oracle_inv_preemphasis_is_the_serial_loop():
    x = np.random.RandomState(1).randn(2, 3000)
    np.testing.assert_allclose(O.inv_preemphasis(x), O.inv_preemphasis_loop(x), rtol=1e-12, atol=1e-12)


def test_blocked_inv_preemphasis_matches_lfilter():
    x = np.random.RandomState(2).randn(2, 40000) * 0.1          # three tiles of the final kernel, the last partial
    ref = O.inv_preemphasis(x)
    got = O.inv_preemphasis_blocked(x)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-6
    np.testing.assert_allclose(got, ref, atol=1e-9 * np.abs(ref).max())


def test_stft_dims_of_the_configs():
    import yaml
    from semi_tts_amd.audio import stft_dims
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ('supervised.yaml', 'semi-single-spkr-paired-data.yaml', 'semi-multi-spkr-paired-data.yaml'):
        a = yaml.safe_load(open(os.path.join(root, 'config', name)))['data']['audio']
        assert stft_dims(a['num_freq'], a['frame_shift_ms'], a['frame_length_ms'], a['sample_rate']) == (2048, 275, 1102)


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import audio, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(audio.toolops, 'griffin_lim', no_device)
    monkeypatch.setattr(audio, '_device', no_device)
    conv = audio.load_audio_transform(**AUDIO_CFG)
    with pytest.raises(ValueError, match='too few'):
        conv.feat_to_wave(torch.rand(4, 1025))                       # T = 4 < 5
    with pytest.raises(ValueError, match='too few'):
        conv.feat_to_wave(torch.rand(2, 3, 1025))
    with pytest.raises(NotImplementedError, match='mel'):
        conv.feat_to_wave(torch.rand(2, 50, 80))
    with pytest.raises(ValueError, match='n_fft'):
        audio.griffin_lim(torch.rand(2, 601, 50), n_fft=1200)          # not a supported power of two
    with pytest.raises(ValueError, match='n_fft'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=1000)).feat_to_wave(torch.rand(50, 1000))
    with pytest.raises(ValueError, match='bins'):
        audio.griffin_lim(torch.rand(2, 1000, 50))                     # F does not match n_fft
    with pytest.raises(ValueError, match='phases'):
        audio.griffin_lim(torch.rand(1, 1025, 50), phases=np.zeros((1, 1025, 49), np.float32))


def test_minimum_length_is_five_frames():
    from semi_tts_amd.audio import check_dims
    check_dims(2048, 275, 1102, 5)
    with pytest.raises(ValueError):
        check_dims(2048, 275, 1102, 4)
    x = torch.zeros(1, 275 * 3)                                        # T = 4 frames: torch itself refuses the reflect padding
    with pytest.raises(RuntimeError):
        O.stft(x.double())


def test_draw_phases_follows_the_reference():
    from semi_tts_amd.audio import draw_phases
    np.random.seed(7)
    got = draw_phases((2, 3, 4))
    np.random.seed(7)
    ref = np.angle(np.exp(2j * np.pi * np.random.rand(2, 3, 4))).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, ref)


def test_write_wav_round_trip(tmp_path):
    from semi_tts_amd.audio import write_wav
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.7, -3.0, 1e-5, 0.25 / 32767])
    p = str(tmp_path / 'a.wav')
    write_wav(p, x, 22050)
    with wave.open(p, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, len(x))
        pcm = np.frombuffer(w.readframes(len(x)), dtype='<i2')
    assert pcm.tolist() == [0, 16384, -16384, 32767, -32767, 32767, -32767, 0, 0]


def test_gen_wav_flag_takes_effect_with_gen_specgram(capsys):
    import main
    p = main.parse_args(['--config', 'config/supervised.yaml', '--gen-specgram', '--gen-wav'])
    assert p.gen_wav
    assert 'gen-wav' not in capsys.readouterr().out
    main.parse_args(['--config', 'config/supervised.yaml', '--gen-wav'])       # training modes: still a no-op, as in the reference
    assert 'no effect' in capsys.readouterr().out
