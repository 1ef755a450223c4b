"""Feature extraction on the MI355X (st_audio_features, semi_tts_amd.audio) against the float64 torch CPU oracle
(tests/feat_oracle.py) and the reference's own outputs (tests/golden/audio_features.npz), at the configs' dimensions
(n_fft 2048, hop 275, win 1102, 80 mels at 22050 Hz)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_oracle as O   # noqa: E402
from semi_tts_amd.audio import SNR_OFF   # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'audio_features.npz')
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])
LIN_TOL, MEL_TOL = 5e-4, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd.audio import load_audio_transform
    return load_audio_transform(**AUDIO_CFG)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN))


def _speech(L, seed):
    """harmonic tone with gated silences (the 1e-5 clamp is reached)"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / O.SR
    f0 = 100 + 150 * rs.rand()
    x = sum(0.4 / (h + 1) * np.sin(2 * np.pi * f0 * (h + 1) * t + rs.rand()) for h in range(6))
    gate = (np.sin(2 * np.pi * 2 * t + 6 * rs.rand()) > -0.2)
    return (0.7 * x * gate + 0.002 * rs.randn(L)).astype(np.float32)


def _maxabs(got, ref):
    return float((torch.as_tensor(got).double().cpu() - torch.as_tensor(ref).double()).abs().max())


def _check_rows(got, ref_tn, T, what, tol):
    """got (T_pad, D) device rows against the oracle's (D, T); rows past T exactly 0"""
    err = _maxabs(got[:T], ref_tn.T)
    print('%s: max-abs %.2e' % (what, err))
    assert err <= tol, (what, err)
    assert bool((got[T:] == 0).all()), what


def test_clean_features_on_the_fixture(dev, conv, gold):
    fb = gold['fb']
    wavs = [torch.from_numpy(gold['wav0']), torch.from_numpy(gold['wav1'])]
    mel, aug, lin = conv.extract_batch(wavs, r=5, snr=SNR_OFF, stretch=1.0)
    assert mel.is_cuda and mel.shape == (2, 75, 80) and lin.shape == (2, 75, 1025)       # 71 frames -> 75: at least one padded
    for b, u in enumerate((1, 0)):                                                         # longest first
        T = 1 + len(gold['wav%d' % u]) // O.HOP
        ref_lin, ref_mel = O.features(gold['wav%d' % u], fb)
        _check_rows(lin[b], ref_lin, T, 'linear %d vs oracle' % u, LIN_TOL)
        _check_rows(mel[b], ref_mel, T, 'mel %d vs oracle' % u, MEL_TOL)
        _check_rows(lin[b], torch.from_numpy(gold['spec%d' % u]), T, 'linear %d vs reference' % u, LIN_TOL)
        _check_rows(mel[b], torch.from_numpy(gold['mel%d' % u]), T, 'mel %d vs reference' % u, MEL_TOL)


def test_augmented_mel_on_the_fixture(dev, conv, gold):
    for u in (0, 1):
        x = torch.from_numpy(gold['wav%d' % u])
        _, aug, _ = conv.extract_batch([x], snr=float(gold['snr%d' % u]), stretch=float(gold['stretch%d' % u]),
                                       noise=[torch.from_numpy(gold['noise%d' % u])])
        ref = torch.from_numpy(gold['aug%d' % u])
        assert aug.shape[1:] == ref.shape
        err = _maxabs(aug[0], ref)
        print('aug %d vs reference: %.2e' % (u, err))
        assert err <= MEL_TOL
        _, aug, _ = conv.extract_batch([x], snr=SNR_OFF, stretch=float(gold['stretch_clean%d' % u]))
        assert _maxabs(aug[0], gold['aug_clean%d' % u]) <= MEL_TOL


def test_ragged_batch(dev, conv):
    from semi_tts_amd.audio import mel_filterbank
    fb = mel_filterbank(O.SR, O.N_FFT, 80)
    lens = [O.N_FFT // 2 + 1, 22050, 40000, 275 * 60 + 131, 9000]      # one just above n_fft // 2, one not a multiple of hop
    wavs = [_speech(L, i) for i, L in enumerate(lens)]
    mel, aug, lin = conv.extract_batch([torch.from_numpy(w).to(dev) for w in wavs], r=3, snr=SNR_OFF, stretch=1.0)
    order = np.argsort(-np.array(lens), kind='stable')
    T_max = 1 + 40000 // O.HOP
    assert mel.shape == (5, T_max + 3 - T_max % 3, 80)
    for b, i in enumerate(order):
        T = 1 + lens[i] // O.HOP
        ref_lin, ref_mel = O.features(wavs[i], fb)
        _check_rows(lin[b], ref_lin, T, 'ragged linear L=%d' % lens[i], LIN_TOL)
        _check_rows(mel[b], ref_mel, T, 'ragged mel L=%d' % lens[i], MEL_TOL)
        # stretch 1.0 and no noise: the augmented mel is the clean one, padded to its own maximum
        assert aug.shape[1] == T_max
        assert torch.equal(aug[b, :T], mel[b, :T]) and bool((aug[b, T:] == 0).all())


@pytest.mark.parametrize('rate', [0.9, 1.0, 1.1])
@pytest.mark.parametrize('snr', [None, 15.0, 40.0])
def test_augmented_mel_with_explicit_noise(dev, conv, rate, snr):
    from semi_tts_amd.audio import mel_filterbank
    fb = mel_filterbank(O.SR, O.N_FFT, 80)
    lens = [30000, 17011]
    wavs = [_speech(L, 10 + i) for i, L in enumerate(lens)]
    noise = [np.random.RandomState(20 + i).randn(L).astype(np.float32) for i, L in enumerate(lens)]
    _, aug, _ = conv.extract_batch([torch.from_numpy(w) for w in wavs], snr=SNR_OFF if snr is None else snr, stretch=rate,
                                   noise=[torch.from_numpy(n) for n in noise])
    win, hop = O.stretch_dims(rate)
    assert aug.shape == (2, 1 + lens[0] // hop, 80)
    for b in range(2):
        T = 1 + lens[b] // hop
        _, ref = O.features(wavs[b], fb, win=win, hop=hop, noise=noise[b], snr=snr)
        _check_rows(aug[b], ref, T, 'aug rate %.1f snr %s L=%d' % (rate, snr, lens[b]), MEL_TOL)


def test_generator_is_seeded_and_repeatable(dev, conv):
    wavs = [torch.from_numpy(_speech(L, 30 + i)).to(dev) for i, L in enumerate([25000, 12000, 18000])]
    kw = dict(r=5, snr=[12.0, 30.0, 20.0], stretch=[0.93, 1.05, 1.0])
    a = conv.extract_batch(wavs, seed=7, **kw)
    b = conv.extract_batch(wavs, seed=7, **kw)
    c = conv.extract_batch(wavs, seed=8, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])      # clean features do not see the noise
    assert not torch.equal(a[1], c[1])


def test_generator_statistics_and_realised_snr(dev, conv):
    from semi_tts_amd import ops
    n = ops.feature_noise(1000000, 3, 12345, dev).double().cpu()
    assert abs(float(n.mean())) < 5e-3 and abs(float(n.var()) - 1) < 1e-2
    assert torch.equal(n, ops.feature_noise(1000000, 3, 12345, dev).double().cpu())
    assert not torch.equal(n[:1000], ops.feature_noise(1000, 4, 12345, dev).double().cpu())
    # the realised SNR of x + coeff n, n the generator's noise for utterance 0: within 0.05 dB of the request
    from semi_tts_amd.audio import mel_filterbank
    x = _speech(40000, 40)
    nz = ops.feature_noise(40000, 0, 99, dev).double().cpu().numpy()
    for snr in (10.0, 37.5):
        coeff = O.snr_coeff(x.astype(np.float64), nz, snr)
        realised = 10 * np.log10((x.astype(np.float64) ** 2).sum() / ((coeff * nz) ** 2).sum())
        assert abs(realised - snr) < 0.05
        # and the kernel adds exactly that noise: its augmented mel is the oracle's with the materialised noise
        _, aug, _ = conv.extract_batch([torch.from_numpy(x)], seed=99, snr=snr, stretch=1.0)
        _, ref = O.features(x, mel_filterbank(O.SR, O.N_FFT, 80), noise=nz, snr=snr)
        assert _maxabs(aug[0], ref.T) <= MEL_TOL


def test_reference_interfaces(dev, conv, tmp_path):
    from semi_tts_amd.audio import load_audio_transform, write_wav
    x = _speech(20000, 50)
    write_wav(tmp_path / 'u.wav', x, O.SR)
    wave = conv.load(tmp_path / 'u.wav')
    sp, msp = conv.extract_feature_from_waveform(wave)
    T = 1 + 20000 // O.HOP
    assert sp.shape == (1025, T) and msp.shape == (80, T) and not sp.is_cuda
    sp_d, _ = conv.extract_feature_from_waveform(wave.to(dev))
    assert sp_d.is_cuda and torch.equal(sp_d.cpu(), sp)
    _, msp_np = conv.extract_feature_from_waveform(wave, preemphasis=False)
    from semi_tts_amd.audio import mel_filterbank
    _, ref = O.features(wave[0].numpy(), mel_filterbank(O.SR, O.N_FFT, 80), preemph=0.0)
    assert _maxabs(msp_np, ref) <= MEL_TOL
    import random
    random.seed(0)
    msp2, msp_aug, sp2 = conv.wave_to_feat(tmp_path / 'u.wav')
    assert msp2.shape == (T, 80) and sp2.shape == (T, 1025) and msp_aug.shape[1] == 80
    assert torch.equal(msp2, msp.T) and torch.equal(sp2, sp.T)
    random.seed(0)
    snr = random.uniform(10, 100)
    win, hop = conv.stretch_dims(random.uniform(0.9, 1.1))
    assert 10 <= snr <= 100 and msp_aug.shape[0] == 1 + 20000 // hop
    mel_only = load_audio_transform(**dict(AUDIO_CFG, use_linear=False, snr_range=[-1, -1]))
    m, a, s = mel_only.wave_to_feat(tmp_path / 'u.wav')
    assert s is None and torch.equal(m, msp.T)
    mel, aug, lin = mel_only.extract_batch([wave[0]])
    assert lin is None and mel.shape == (1, T, 80)


def test_training_on_wav_files(dev, tmp_path):
    from semi_tts_amd.audio import write_wav
    wav_dir = tmp_path / 'wavs'
    wav_dir.mkdir()
    for i in range(8):
        write_wav(wav_dir / ('utt%02d.wav' % i), _speech(16000 + 2500 * i, 60 + i), O.SR)
    cmd = [sys.executable, os.path.join(REPO, 'main.py'), '--config', os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml'),
           '--unpair-wav-dir', str(wav_dir), '--max-step', '4', '--logdir', str(tmp_path / 'log'), '--ckpdir', str(tmp_path / 'ckpt')]
    p = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0
    losses = [float(line.split('Loss - ')[1].split()[0]) for line in p.stdout.splitlines() if 'Loss - ' in line]
    assert losses and all(np.isfinite(losses))
    used = [int(m.group(1)) for m in re.finditer(r'CTC-nan/unp-sph/unp-txt=\d+/(\d+)/\d+', p.stdout)]
    assert used and used[-1] >= 1             # step 2 (speech first) took a batch of the .wav files
