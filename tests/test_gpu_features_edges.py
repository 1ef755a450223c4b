"""Feature extraction (st_audio_features, semi_tts_amd.audio) on the MI355X away from the configs' dimensions (tests/audio_cases.py)
against the float64 oracle (tests/feat_oracle.py): n_fft 512 / 1024 / 4096, ragged batches down to n_fft / 2 + 1 samples, batches
mixing noisy and clean utterances, digital silence, a batch above the 64 utterances of one launch, and the built-in noise
generator against an independent numpy restatement of Philox4x32-10 + Box-Muller."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_cases as A   # noqa: E402
from semi_tts_amd.audio import SNR_OFF   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


_CONV = {}


def _conv(n_fft):
    """(converter, filterbank) of a configuration of audio_cases.FEAT_CONFIGS, built once"""
    from semi_tts_amd.audio import load_audio_transform, mel_filterbank
    if n_fft not in _CONV:
        c = A.FEAT_CONFIGS[n_fft]
        _CONV[n_fft] = (load_audio_transform(**c), mel_filterbank(c['sample_rate'], n_fft, c['num_mels']))
    return _CONV[n_fft]


def _check_rows(got, ref_tn, T, what, tol):
    """got (T_pad, D) device rows against the oracle's (D, T); rows past T exactly 0"""
    err = float((got[:T].double().cpu() - torch.as_tensor(ref_tn).double().T).abs().max())
    print('%s: max-abs %.2e' % (what, err))
    assert err <= tol, (what, err)
    assert bool((got[T:] == 0).all()), what


def _t(arrays):
    return [torch.from_numpy(a) for a in arrays]


# ---------------------------------------------------------------- other sizes
@pytest.mark.parametrize('n_fft', sorted(A.FEAT_CONFIGS))
def test_clean_features_at_other_sizes(dev, n_fft):
    conv, fb = _conv(n_fft)
    hop = conv.hop_length
    wavs, _ = A.feat_batch(n_fft)
    mel, aug, lin = conv.extract_batch([w.to(dev) for w in _t(wavs)], r=3, snr=SNR_OFF, stretch=1.0)
    T_max = 1 + len(wavs[0]) // hop
    assert mel.shape == (4, T_max + 3 - T_max % 3, conv.n_mels) and lin.shape == mel.shape[:2] + (n_fft // 2 + 1,)
    for b, x in enumerate(wavs):
        T = 1 + len(x) // hop
        ref_lin, ref_mel = A.feat_reference(x, fb, n_fft)
        _check_rows(lin[b], ref_lin, T, 'linear n_fft=%d L=%d' % (n_fft, len(x)), A.LIN_TOL)
        _check_rows(mel[b], ref_mel, T, 'mel n_fft=%d L=%d' % (n_fft, len(x)), A.MEL_TOL)
        assert torch.equal(aug[b, :T], mel[b, :T]) and bool((aug[b, T:] == 0).all())      # stretch 1.0, no noise: the clean mel


@pytest.mark.parametrize('snr', A.FEAT_SNRS)
@pytest.mark.parametrize('rate', A.FEAT_RATES)
@pytest.mark.parametrize('n_fft', sorted(A.FEAT_CONFIGS))
def test_augmented_mel_at_other_sizes(dev, n_fft, rate, snr):
    conv, fb = _conv(n_fft)
    wavs, noise = A.feat_batch(n_fft)
    _, aug, _ = conv.extract_batch(_t(wavs), snr=SNR_OFF if snr is None else snr, stretch=rate, noise=_t(noise))
    win, hop = A.feat_stretch_dims(n_fft, rate)
    assert aug.shape == (4, 1 + len(wavs[0]) // hop, conv.n_mels)
    for b, x in enumerate(wavs):
        _, ref = A.feat_reference(x, fb, n_fft, win=win, hop=hop, noise=noise[b], snr=snr)
        _check_rows(aug[b], ref, 1 + len(x) // hop, 'aug n_fft=%d rate %.1f snr %s L=%d' % (n_fft, rate, snr, len(x)), A.MEL_TOL)


# ---------------------------------------------------------------- mixed batch, silence
def test_batch_mixing_noisy_and_clean_utterances(dev):
    conv, fb = _conv(512)
    wavs = [A.speech(L, 70 + i) for i, L in enumerate(A.MIXED_LENS)]
    noise = [A.randn(L, 80 + i) for i, L in enumerate(A.MIXED_LENS)]
    _, aug, _ = conv.extract_batch(_t(wavs), snr=A.MIXED_SNR, stretch=1.0, noise=_t(noise))
    hop = conv.hop_length
    for b, (x, snr) in enumerate(zip(wavs, A.MIXED_SNR)):
        _, ref = A.feat_reference(x, fb, 512, noise=noise[b], snr=snr)
        _check_rows(aug[b], ref, 1 + len(x) // hop, 'mixed batch row %d L=%d snr %s' % (b, len(x), snr), A.MEL_TOL)
        if snr is not None:                                      # and the noise is visible at this bound
            _, clean = A.feat_reference(x, fb, 512)
            assert float((ref - clean).abs().max()) > 100 * A.MEL_TOL


@pytest.mark.parametrize('snr', [None, 20.0])
@pytest.mark.parametrize('explicit', [True, False])
def test_digital_silence(dev, snr, explicit):
    conv, fb = _conv(512)
    one = np.zeros(700, np.float32)
    one[333] = 0.5
    wavs = [A.speech(900, 91), np.zeros(800, np.float32), one]
    noise = [A.randn(len(w), 92 + i) for i, w in enumerate(wavs)]
    mel, aug, lin = conv.extract_batch(_t(wavs), snr=SNR_OFF if snr is None else snr, stretch=1.0, seed=5,
                                       noise=_t(noise) if explicit else None)
    for out in (mel, lin, aug):                                  # signal power 0: the coefficient is 0, every value exactly 0
        assert bool((out[1] == 0).all())
    assert float(mel[0].abs().max()) > 0 and float(aug[0].abs().max()) > 0
    hop = conv.hop_length
    ref_lin, ref_mel = A.feat_reference(one, fb, 512)
    _check_rows(lin[2], ref_lin, 1 + 700 // hop, 'one-sample utterance linear', A.LIN_TOL)
    _check_rows(mel[2], ref_mel, 1 + 700 // hop, 'one-sample utterance mel', A.MEL_TOL)
    from semi_tts_amd import ops
    nz = noise[2] if explicit else ops.feature_noise(700, 2, 5, dev).double().cpu().numpy()
    _, ref_aug = A.feat_reference(one, fb, 512, noise=nz, snr=snr)
    _check_rows(aug[2], ref_aug, 1 + 700 // hop, 'one-sample utterance aug snr %s' % snr, A.MEL_TOL)


# ---------------------------------------------------------------- above FEATURES_MAX_BATCH
def _big_wavs():
    return [A.speech(L, 100 + u) for u, L in enumerate(A.BIG_LENS)]


def test_batch_of_70_with_explicit_noise(dev):
    """the second chunk's pointer arithmetic: mel, linear, aug and every host array"""
    from semi_tts_amd import ops
    assert A.BIG_B > ops.FEATURES_MAX_BATCH
    conv, fb = _conv(512)
    wavs = _big_wavs()
    noise = [A.randn(L, 300 + u) for u, L in enumerate(A.BIG_LENS)]
    snr = [None if u % 5 == 4 else 10.0 + u % 7 for u in range(A.BIG_B)]
    mel, aug, lin = conv.extract_batch(_t(wavs), r=2, snr=snr, stretch=A.BIG_RATES, noise=_t(noise))
    worst = [0.0, 0.0, 0.0]
    for u, x in enumerate(wavs):
        T = 1 + len(x) // conv.hop_length
        ref_lin, ref_mel = A.feat_reference(x, fb, 512)
        win, hop = conv.stretch_dims(A.BIG_RATES[u])
        _, ref_aug = A.feat_reference(x, fb, 512, win=win, hop=hop, noise=noise[u], snr=snr[u])
        for j, (got, ref, Tj, tol) in enumerate([(lin[u], ref_lin, T, A.LIN_TOL), (mel[u], ref_mel, T, A.MEL_TOL),
                                                 (aug[u], ref_aug, 1 + len(x) // hop, A.MEL_TOL)]):
            err = float((got[:Tj].double().cpu() - ref.T).abs().max())
            worst[j] = max(worst[j], err)
            assert err <= tol and bool((got[Tj:] == 0).all()), (u, 'linear mel aug'.split()[j], err)
    print('batch of 70: max-abs linear %.2e, mel %.2e, aug %.2e' % tuple(worst))


def test_batch_of_70_generator_follows_the_batch_position(dev):
    """the noise of sorted utterance u is feature_noise(L_u, u, seed) in the second chunk (u >= 64) as in the first"""
    from semi_tts_amd import ops
    conv, fb = _conv(512)
    wavs = _big_wavs()
    _, aug, _ = conv.extract_batch(_t(wavs), seed=A.BIG_SEED, snr=A.BIG_SNR, stretch=A.BIG_RATES)
    for u in A.BIG_CHECKED:
        x = wavs[u]
        nz = ops.feature_noise(len(x), u, A.BIG_SEED, dev).double().cpu().numpy()
        win, hop = conv.stretch_dims(A.BIG_RATES[u])
        _, ref = A.feat_reference(x, fb, 512, win=win, hop=hop, noise=nz, snr=A.BIG_SNR)
        _check_rows(aug[u], ref, 1 + len(x) // hop, 'generated noise, utterance %d of 70' % u, A.MEL_TOL)
        if u >= 64:                      # the noise of the chunk-relative index is told apart at this bound
            other = ops.feature_noise(len(x), u - 64, A.BIG_SEED, dev).double().cpu().numpy()
            _, wrong = A.feat_reference(x, fb, 512, win=win, hop=hop, noise=other, snr=A.BIG_SNR)
            assert float((wrong - ref).abs().max()) > 100 * A.MEL_TOL


def test_equal_waveforms_get_different_noise_across_chunks(dev):
    conv, _ = _conv(512)
    x = torch.from_numpy(A.speech(640, 7))
    _, aug, _ = conv.extract_batch([x] * A.BIG_B, seed=A.BIG_SEED, snr=A.BIG_SNR, stretch=1.0)
    assert not torch.equal(aug[0], aug[64]) and not torch.equal(aug[5], aug[69])
    _, small, _ = conv.extract_batch([x] * 64, seed=A.BIG_SEED, snr=A.BIG_SNR, stretch=1.0)
    assert torch.equal(small, aug[:64])                              # the first 64 do not depend on what follows


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize('utt,seed', A.NOISE_STREAMS)
def test_generator_against_the_numpy_restatement(dev, utt, seed):
    from semi_tts_amd import ops
    got = ops.feature_noise(A.NOISE_N, utt, seed, dev)
    assert torch.equal(ops.feature_noise(1000, utt, seed, dev), got[:1000])             # the prefix property
    assert bool(torch.isfinite(got).all())
    got = got.double().cpu().numpy()
    compared = exempt = 0
    worst = 0.0
    for a, b in A.NOISE_WINDOWS:
        ref, m1 = A.feature_noise_ref(np.arange(a, b), utt, seed)
        keep = m1 < 2 ** 24 - A.NOISE_EXEMPT_U1
        err = np.abs(got[a:b] - ref)
        worst = max(worst, float(err[keep].max()))
        compared += b - a
        exempt += int((~keep).sum())
        assert float(err[~keep].max(initial=0.0)) < 1e-3                                 # exempt from the bound, not from being right
    print('generator utt %d seed %d: max-abs %.2e over %d samples, %d exempt' % (utt, seed, worst, compared, exempt))
    assert exempt <= A.NOISE_EXEMPT_MAX * compared
    assert worst <= A.NOISE_TOL, worst
