"""CPU side of the audio edge tests (tests/audio_cases.py): every case is accepted by the library's own checks and by the float64
oracles, the numpy restatement of Philox4x32-10 reproduces Random123's known answers, and the oracles alone stay inside every bound
the GPU tests apply: evaluated in float32 they differ from their float64 value by at most a quarter of it.

Measured float32-against-float64 drifts of the oracles (worst over the cases of a family; the bound in brackets):
  STFT          rel-L2 1.6e-7 (1e-6), max-abs / scale 1.9e-7 (1e-5)
  iSTFT         rel-L2 1.1e-7 (1e-6), max-abs / scale 3.9e-7 (1e-5)
  Griffin-Lim   rel-L2 3.5e-6 (1e-4), max-abs / scale 5.7e-6 (1e-3)     six sizes x {0, 1, 30} iterations, and with zero frames;
                                                                        4.3e-6 / 7.4e-6 with the magnitudes changed by an ulp
  options       rel-L2 3.1e-6 (1e-4), max-abs / scale 1.7e-5 (1e-3)     specgram_to_waveform, 30 iterations; 22 ... 34 % on the clip
  linear        max-abs 3.0e-5 (5e-4)                                   the clean framing (the augmented one writes a mel only)
  mel           max-abs 3.5e-6 (1e-4)                                   clean and augmented, three configurations
Serial float32 de-emphasis against float64 on the stand-in signals of the tile-edge cases: max-abs / scale 5.7e-7 ... 8.2e-7 (the
GPU bound is 8 times the figure of the actual input); the float64 blocked form against lfilter: <= 6e-16 of the scale."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_cases as A   # noqa: E402
import gl_oracle as GL   # noqa: E402

MARGIN = 4         # the oracle's own float32 drift times this stays inside the bound


def _drift(lo, hi):
    """(rel-L2, max-abs / scale) of a float32 evaluation against the float64 one"""
    lo, hi = torch.as_tensor(lo), torch.as_tensor(hi)
    if lo.is_complex() or hi.is_complex():
        lo, hi = torch.view_as_real(lo.to(torch.complex128)), torch.view_as_real(hi.to(torch.complex128))
    lo, hi = lo.double(), hi.double()
    return float((lo - hi).norm() / hi.norm()), float((lo - hi).abs().max() / hi.abs().max())


def _inside(d, tol, what):
    print('%s: float32 oracle drift rel L2 %.2e, max-abs / scale %.2e' % (what, d[0], d[1]))
    assert MARGIN * d[0] <= tol[0] and MARGIN * d[1] <= tol[1], (what, d)


# ---------------------------------------------------------------- A
@pytest.mark.parametrize('signal', sorted(A.SIGNALS))
@pytest.mark.parametrize('p', A.with_batches(A.STFT_CASES), ids=A.case_id)
def test_stft_cases(p, signal):
    from semi_tts_amd.audio import check_dims
    case, B = p
    n_fft, hop, win, L = case
    check_dims(n_fft, hop, win, max(A.n_frames(hop, L), n_fft // 2 // hop + 2))       # the dims; the frame count is iSTFT's business
    assert L > n_fft // 2
    x = A.stft_input(case, B, signal)
    ref = A.stft_reference(x, case)
    assert ref.shape == (B, n_fft // 2 + 1, A.n_frames(hop, L))
    _inside(_drift(A.stft_reference(x, case, torch.float32), ref), A.STFT_TOL, 'stft %s %s' % (A.case_id(p), signal))


@pytest.mark.parametrize('signal', sorted(A.SIGNALS))
@pytest.mark.parametrize('p', A.with_batches(A.ISTFT_CASES), ids=A.case_id)
def test_istft_cases(p, signal):
    from semi_tts_amd.audio import check_dims
    case, B = p
    n_fft, hop, win, L = case
    T = A.n_frames(hop, L)
    check_dims(n_fft, hop, win, T)
    spec = A.stft_reference(A.stft_input(case, B, signal), case).to(torch.complex64)     # what the kernel is given
    ref = A.istft_reference(spec, case)                                                  # torch.istft accepts the envelope
    assert ref.shape == (B, hop * (T - 1))
    _inside(_drift(A.istft_reference(spec, case, torch.float32), ref), A.STFT_TOL, 'istft %s %s' % (A.case_id(p), signal))


def test_case_tables_are_what_they_claim():
    assert len(A.STFT_CASES) == 9 and A.ISTFT_REFUSED == [A.STFT_CASES[0], A.STFT_CASES[7]]
    assert sorted({c[0] for c in A.STFT_BATCH_CASES}) == [512, 1024, 2048, 4096]
    assert all(c in A.ISTFT_CASES for c in A.STFT_BATCH_CASES)
    n, h, w, L = A.STFT_CASES[0]
    assert L == n // 2 + 1 and (A.n_frames(h, L) - 1) * h - n // 2 < 0 < L - 1          # frame T-1 starts before 0 and ends past L-1
    assert A.STFT_CASES[1][3] % 275 == 274
    assert all((c[0] - c[2]) % 2 == 1 for c in A.STFT_CASES[2:4])
    assert [hop * (T - 1) for hop, T in A.OLA_CASES] == [A.OLA_TILE - 1, A.OLA_TILE, A.OLA_TILE + 1, 2 * A.OLA_TILE + 1, 4900]
    assert 4900 < A.OLA_TILE // 2
    from semi_tts_amd.audio import stft_dims
    assert A.FEAT_DIMS == {n: stft_dims(c['num_freq'], c['frame_shift_ms'], c['frame_length_ms'], c['sample_rate'])
                           for n, c in A.FEAT_CONFIGS.items()}
    assert A.NOISE_N > 4096 * 256 and all(0 <= a < b <= A.NOISE_N and b - a == 4096 for a, b in A.NOISE_WINDOWS)
    assert A.NOISE_WINDOWS[1][0] < 4096 * 256 < A.NOISE_WINDOWS[1][1]


def test_refusals_are_refused_by_the_python_checks_too():
    from semi_tts_amd.audio import check_dims
    for _, (n_fft, hop, win), n, _ in A.REFUSALS[1:3]:
        with pytest.raises(ValueError, match='2 \\* hop <= win <= n_fft'):
            check_dims(n_fft, hop, win, 50)
    for n_fft, hop, win, L in A.ISTFT_REFUSED:
        with pytest.raises(ValueError, match='too few'):
            check_dims(n_fft, hop, win, A.n_frames(hop, L))
    for kind, (n_fft, hop, win), n, _ in A.REFUSALS:
        if kind == 'istft':
            with pytest.raises(ValueError, match='too few'):
                check_dims(n_fft, hop, win, n)
    n_fft, hop, win = A.REFUSALS[0][1]
    with pytest.raises(RuntimeError):                  # torch refuses L = n_fft / 2 as the library does
        GL.stft(torch.zeros(1, A.REFUSALS[0][2], dtype=torch.float64), n_fft, hop, win)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize('dims', A.GL_DIMS + ['zero'], ids=str)
def test_griffin_lim_cases(dims):
    from semi_tts_amd.audio import check_dims
    zero = dims == 'zero'
    dims = A.GL_ZERO_DIMS if zero else dims
    amp, ph = A.gl_input(dims, zero_frames=zero)
    check_dims(*dims, amp.shape[2])
    assert amp.shape == (2, dims[0] // 2 + 1, A.gl_frames(dims[0], dims[1]))
    if zero:
        assert dims[0] != 2048 and float(amp[0, :, :2].abs().max()) == 0 and float(amp[1, :, -3:].abs().max()) == 0
    for n_iter in A.GL_ITERS:
        ref = A.gl_reference(amp, ph, n_iter, dims)
        assert ref.dtype == torch.float64 and ref.shape == (2, dims[1] * (amp.shape[2] - 1))
        lo = A.gl_reference(amp, ph, n_iter, dims, torch.float32)
        assert lo.dtype == torch.float32
        _inside(_drift(lo, ref), A.GL_TOL, 'GL %s%s, %d iterations' % (dims, ' zero frames' if zero else '', n_iter))
    for seed in (1, 2, 3):                 # the input is not next to a fork of the phase projection: one-ulp changes drift no more
        near = A.gl_perturbed(amp, seed)
        d = _drift(A.gl_reference(near, ph, A.GL_ITERS[-1], dims, torch.float32), A.gl_reference(near, ph, A.GL_ITERS[-1], dims))
        _inside(d, A.GL_TOL, 'GL %s%s, magnitudes changed by an ulp (%d)' % (dims, ' zero frames' if zero else '', seed))


@pytest.mark.parametrize('name', sorted(A.OPTION_CASES))
def test_option_cases(name):
    from semi_tts_amd.audio import check_dims
    spec, ph, kw = A.option_input(name)
    check_dims(GL.N_FFT, GL.HOP, GL.WIN, A.OPT_T)
    assert spec.shape == ((A.OPT_B,) if name != 'two_d' else ()) + (GL.N_FFT // 2 + 1, A.OPT_T) and ph.shape == spec.shape
    ref = A.option_reference(spec, ph, kw)
    _inside(_drift(A.option_reference(spec, ph, kw, torch.float32), ref), A.GL_TOL, 'option %s' % name)
    on_clip = float((np.abs(ref) == 1).mean())
    print('option %s: %.1f %% of the reference on the clip' % (name, 100 * on_clip))
    assert 0.05 <= on_clip <= 0.5, (name, on_clip)          # the clip is reached, and a saturated output cannot hide an error
    if name == 'is_amp':                                   # the oracle ignores the power with isAmp, as src/audio.py:186-188 does
        assert np.array_equal(ref, A.option_reference(spec, ph, dict(kw, power=1.0)))


def test_unclipped_case_exceeds_one():
    amp, ph = A.unclipped_input()
    kw = dict(isAmp=True)
    ref = A.option_reference(amp, ph, kw, clip=False)
    assert float(np.abs(ref).max()) > 1.5
    _inside(_drift(A.option_reference(amp, ph, kw, torch.float32, clip=False), ref), A.GL_TOL, 'unclipped de-emphasis')


# ---------------------------------------------------------------- C
@pytest.mark.parametrize('hop,T', A.OLA_CASES)
def test_ola_cases_and_the_serial_float32_error(hop, T):
    from semi_tts_amd.audio import check_dims
    check_dims(A.OLA_N_FFT, hop, A.OLA_WIN, T)
    amp, ph = A.ola_input(hop, T)
    # the stand-in of the kernel's pre-scan samples: the oracle's iSTFT of the same spectrum, as float32 values
    x = GL.griffin_lim(amp.double(), torch.from_numpy(ph), 0, n_fft=A.OLA_N_FFT, hop=hop, win=A.OLA_WIN).float().numpy()
    assert x.shape == (A.OLA_B, hop * (T - 1))
    bound, ref = A.deemph_bound(x)
    scale = float(np.abs(ref).max())
    assert scale > 10 * float(np.abs(x).max())              # a large, slowly decaying component: the carry matters
    blocked = float(np.abs(GL.inv_preemphasis_blocked(x.astype(np.float64)) - ref).max())
    print('de-emphasis L=%d: serial float32 max-abs / scale %.2e, float64 blocked form %.2e (scale %.3g)'
          % (x.shape[1], bound / A.DEEMPH_SLACK / scale, blocked / scale, scale))
    assert 0 < bound / scale < 1e-4                         # a bound that binds: a dropped carry errs by the order of the scale
    assert MARGIN * blocked <= bound
    # resetting the carry per tile would be caught: its error at the first sample of the second tile is 0.97 y[tile - 1]
    if x.shape[1] > A.OLA_TILE:
        assert 0.97 * float(np.abs(ref[:, A.OLA_TILE - 1]).min()) > 100 * bound


# ---------------------------------------------------------------- D
def _fb(n_fft):
    from semi_tts_amd.audio import mel_filterbank
    c = A.FEAT_CONFIGS[n_fft]
    return mel_filterbank(c['sample_rate'], n_fft, c['num_mels'])


def _feat_inside(x, fb, n_fft, what, linear=False, **kw):
    """linear: the clean framing, whose linear spectrogram the kernel writes (the augmented framing gives a mel only)"""
    lin, mel = A.feat_reference(x, fb, n_fft, **kw)
    lin32, mel32 = A.feat_reference(x, fb, n_fft, dtype=torch.float32, **kw)
    dl, dm = float((lin32.double() - lin).abs().max()), float((mel32.double() - mel).abs().max())
    print('%s: float32 oracle drift linear %.2e, mel %.2e' % (what, dl, dm))
    assert (not linear or MARGIN * dl <= A.LIN_TOL) and MARGIN * dm <= A.MEL_TOL, (what, dl, dm)
    return lin, mel


@pytest.mark.parametrize('n_fft', sorted(A.FEAT_CONFIGS))
def test_feature_cases(n_fft):
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(**A.FEAT_CONFIGS[n_fft])
    assert (conv.n_fft, conv.hop_length, conv.win_length) == A.FEAT_DIMS[n_fft]
    lens = A.feat_lens(n_fft)
    assert lens == sorted(lens, reverse=True) and lens[-1] == n_fft // 2 + 1 and lens[0] == 3 * n_fft + 17
    aug = [conv.stretch_dims(r) for r in A.FEAT_RATES]
    assert aug == [A.feat_stretch_dims(n_fft, r) for r in A.FEAT_RATES]
    conv._check(lens, aug)
    fb = _fb(n_fft)
    wavs, noise = A.feat_batch(n_fft)
    for x, nz in zip(wavs, noise):
        lin, mel = _feat_inside(x, fb, n_fft, 'clean n_fft=%d L=%d' % (n_fft, len(x)), linear=True)
        assert lin.shape == (n_fft // 2 + 1, 1 + len(x) // conv.hop_length)
        for rate, (win, hop) in zip(A.FEAT_RATES, aug):
            for snr in A.FEAT_SNRS:
                _feat_inside(x, fb, n_fft, 'aug n_fft=%d L=%d rate %.1f snr %s' % (n_fft, len(x), rate, snr), win=win, hop=hop,
                             noise=nz, snr=snr)


def test_mixed_silent_and_big_batch_cases():
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(**A.FEAT_CONFIGS[512])
    fb = _fb(512)
    assert A.MIXED_LENS == sorted(A.MIXED_LENS, reverse=True)
    assert any(L == 257 and s is not None for L, s in zip(A.MIXED_LENS, A.MIXED_SNR))     # the shortest utterance among the noisy
    conv._check(A.MIXED_LENS)
    for i, (L, snr) in enumerate(zip(A.MIXED_LENS, A.MIXED_SNR)):
        _feat_inside(A.speech(L, 70 + i), fb, 512, 'mixed L=%d snr %s' % (L, snr), noise=A.randn(L, 80 + i), snr=snr)
    x = np.zeros(700, np.float32)
    x[333] = 0.5
    for snr in (None, 20.0):
        _feat_inside(x, fb, 512, 'one-sample utterance snr %s' % snr, noise=A.randn(700, 90), snr=snr)
    lin, mel = A.feat_reference(np.zeros(700, np.float32), fb, 512)
    assert float(lin.abs().max()) == 0 and float(mel.abs().max()) == 0                    # digital silence normalises to exactly 0
    assert A.BIG_B > 64 and A.BIG_LENS == sorted(A.BIG_LENS, reverse=True) and min(A.BIG_LENS) >= 300 and max(A.BIG_LENS) == 1000
    assert all(u < A.BIG_B for u in A.BIG_CHECKED) and {63, 64} <= set(A.BIG_CHECKED)
    conv._check(A.BIG_LENS, [conv.stretch_dims(r) for r in A.BIG_RATES])
    for u in A.BIG_CHECKED:                                                               # the noise stands in for the generator's
        win, hop = conv.stretch_dims(A.BIG_RATES[u])
        _feat_inside(A.speech(A.BIG_LENS[u], 100 + u), fb, 512, 'big batch utterance %d' % u, win=win, hop=hop,
                     noise=A.feature_noise_ref(np.arange(A.BIG_LENS[u]), u, A.BIG_SEED)[0], snr=A.BIG_SNR)


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize('ctr,key,want', A.PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    got = A.philox4x32_10(ctr, key)
    assert tuple(int(v[0]) for v in got) == want


def test_philox_is_elementwise():
    idx = np.arange(5, dtype=np.uint64) + np.uint64(2 ** 32 - 2)          # crosses into the high counter word
    both = A.philox4x32_10((idx & np.uint64(0xffffffff), idx >> np.uint64(32), np.full(5, 3), np.zeros(5)), (7, 9))
    for j in range(5):
        one = A.philox4x32_10((int(idx[j]) & 0xffffffff, int(idx[j]) >> 32, 3, 0), (7, 9))
        assert [int(v[j]) for v in both] == [int(v[0]) for v in one]


def test_generator_restatement_is_a_standard_normal_with_few_exemptions():
    for utt, seed in A.NOISE_STREAMS:
        idx = np.concatenate([np.arange(a, b) for a, b in A.NOISE_WINDOWS])
        v, m1 = A.feature_noise_ref(idx, utt, seed)
        assert np.isfinite(v).all() and abs(v.mean()) < 0.05 and abs(v.var() - 1) < 0.05 and np.abs(v).max() <= 5.78
        assert (m1 >= 1).all() and (m1 <= 2 ** 24).all()
        assert int((m1 >= 2 ** 24 - A.NOISE_EXEMPT_U1).sum()) <= A.NOISE_EXEMPT_MAX * idx.size
    a, _ = A.feature_noise_ref(np.arange(100), 0, 5)
    b, _ = A.feature_noise_ref(np.arange(100), 64, 5)
    assert not np.array_equal(a, b)                                        # the utterance index selects the stream
