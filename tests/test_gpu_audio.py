"""Griffin-Lim vocoder on the MI355X (semi_tts_amd/csrc/audio.hip) against the float64 torch CPU restatement (tests/gl_oracle.py),
at the configs' STFT dimensions (n_fft 2048, hop 275, win 1102)."""
import os
import sys
import types
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu

N_FFT, HOP, WIN, F = O.N_FFT, O.HOP, O.WIN, O.N_FFT // 2 + 1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


def _signal(B, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 22050
    f0 = 110 + 200 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = sum(0.4 / (h + 1) * torch.sin(2 * np.pi * f0 * (h + 1) * t) for h in range(6))
    return (x * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t)) + 0.02 * torch.randn(B, L, generator=g, dtype=torch.float64)).float()


def _close(got, ref, rel_l2, max_abs, what):
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    if got.is_complex() or ref.is_complex():
        got, ref = torch.view_as_real(got.to(torch.complex128)), torch.view_as_real(ref.to(torch.complex128))
    got, ref = got.double(), ref.double()
    scale = float(ref.abs().max())
    rl2 = float((got - ref).norm() / ref.norm())
    ma = float((got - ref).abs().max())
    print('%s: rel L2 %.2e, max-abs %.2e (scale %.3g)' % (what, rl2, ma, scale))
    assert rl2 <= rel_l2 and ma <= max_abs * scale, (what, rl2, ma, scale)


def _to_frames(spec_bft):
    """(B, F, T) complex -> the library's frame-major (B, T, F, 2) float32"""
    return torch.view_as_real(spec_bft.transpose(1, 2).to(torch.complex64).contiguous()).contiguous()


def _from_frames(spec_btf2):
    return torch.view_as_complex(spec_btf2.cpu().double().contiguous()).transpose(1, 2)


@pytest.mark.parametrize('B', [1, 3, 32])
@pytest.mark.parametrize('T', [5, 6, 43, 258, 355])
def test_stft_matches_torch(dev, B, T):
    from semi_tts_amd import ops
    x = _signal(B, HOP * (T - 1), seed=B * 1000 + T)
    got = ops.stft_fwd(x.to(dev), N_FFT, HOP, WIN)
    assert got.shape == (B, T, F, 2)
    _close(_from_frames(got), O.stft(x.double()), 1e-6, 1e-5, 'stft B=%d T=%d' % (B, T))


@pytest.mark.parametrize('B', [1, 3, 32])
@pytest.mark.parametrize('T', [5, 6, 43, 258, 355])
def test_istft_matches_torch(dev, B, T):
    from semi_tts_amd import ops
    x = _signal(B, HOP * (T - 1), seed=B * 1000 + T + 7)
    spec = _to_frames(O.stft(x.double()))
    got = ops.istft(spec.to(dev), N_FFT, HOP, WIN)
    assert got.shape == (B, HOP * (T - 1))
    _close(got.cpu(), O.istft(_from_frames(spec)), 1e-6, 1e-5, 'istft B=%d T=%d' % (B, T))


@pytest.mark.parametrize('n_fft,hop,win', [(512, 64, 400), (1024, 128, 1024), (4096, 512, 3000)])
def test_other_fft_sizes(dev, n_fft, hop, win):
    from semi_tts_amd import ops
    T = 2 + n_fft // 2 // hop + 7
    x = _signal(2, hop * (T - 1), seed=n_fft)
    got = ops.stft_fwd(x.to(dev), n_fft, hop, win)
    _close(_from_frames(got), O.stft(x.double(), n_fft, hop, win), 1e-6, 1e-5, 'stft n_fft=%d' % n_fft)
    spec = _to_frames(O.stft(x.double(), n_fft, hop, win))
    got = ops.istft(spec.to(dev), n_fft, hop, win)
    _close(got.cpu(), O.istft(_from_frames(spec), n_fft, hop, win), 1e-6, 1e-5, 'istft n_fft=%d' % n_fft)


def test_unsupported_dims_are_refused_by_the_library(dev):
    from semi_tts_amd import ops
    x = torch.zeros(1, 4000, device=dev)
    with pytest.raises(RuntimeError, match='n_fft'):
        ops.stft_fwd(x, 1536, 256, 1024)
    with pytest.raises(RuntimeError, match='hop'):
        ops.stft_fwd(x, 2048, 600, 1102)                       # 2 hop > win
    with pytest.raises(RuntimeError, match='reflect'):
        ops.istft(torch.zeros(1, 4, F, 2, device=dev), N_FFT, HOP, WIN)   # T = 4


def _phases(shape, seed):
    from semi_tts_amd.audio import draw_phases
    np.random.seed(seed)
    return draw_phases(shape)


def _real_amp(B=4, T=258):
    return O.stft(_signal(B, HOP * (T - 1), seed=11).double()).abs().float()     # (B, F, T)


def _check_gl(amp_bft, phases, what):
    from semi_tts_amd import audio
    for n_iter in (1, 30):
        got = audio.griffin_lim(amp_bft.cuda(), phases=phases, n_iter=n_iter)
        ref = O.griffin_lim(amp_bft.double(), torch.from_numpy(phases), n_iter)
        _close(got.cpu(), ref, 1e-4, 1e-3, '%s, %d iterations' % (what, n_iter))


def test_griffin_lim_real_signal(dev):
    amp = _real_amp()
    _check_gl(amp, _phases(tuple(amp.shape), 3), 'GL of a real signal')


def test_griffin_lim_zero_frames(dev):
    amp = _real_amp(B=3, T=61)
    amp[0, :, 10:20] = 0                  # whole silent frames: angle(0) = 0 inside the iterations
    amp[1, :, :2] = 0                     # at the reflected left edge
    amp[2, :, -3:] = 0                    # and the right one
    _check_gl(amp, _phases(tuple(amp.shape), 4), 'GL with zero frames')


def test_griffin_lim_is_bitwise_repeatable(dev):
    from semi_tts_amd import audio
    amp = _real_amp(B=32, T=258).to(dev)
    ph = _phases(tuple(amp.shape), 5)
    a = audio.griffin_lim(amp, phases=ph)
    b = audio.griffin_lim(amp, phases=ph)
    assert torch.equal(a, b)


def _normalise(amp_bft):
    """the inverse of the denormalisation (src/audio.py:172-173): a (B, T, F) feature in [0, 1]"""
    db = 20 * torch.log10(torch.clamp(amp_bft.double(), min=1e-5)) - O.REF_LEVEL_DB
    return torch.clamp((db - O.MIN_LEVEL_DB) / -O.MIN_LEVEL_DB, 0, 1).float().transpose(1, 2).contiguous()


def test_feat_to_wave_end_to_end(dev):
    from semi_tts_amd.audio import load_audio_transform
    import yaml
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'supervised.yaml')))['data']['audio']
    conv = load_audio_transform(**cfg)
    feat = _normalise(_real_amp(B=3, T=120))                        # (B, T, F), on the host: feat_to_wave moves it
    ph = _phases((3, F, 120), 6)
    wav, sr = conv.feat_to_wave(feat, phases=ph)
    assert sr == 22050 and wav.dtype == np.float64 and wav.shape == (3, HOP * 119)
    ref = O.feat_to_wave(feat, torch.from_numpy(ph))
    _close(wav, ref, 1e-4, 1e-3, 'feat_to_wave')
    one, _ = conv.feat_to_wave(feat[1].to(dev), phases=ph[1])       # (T, F) on the device
    assert one.shape == (HOP * 119,)
    np.testing.assert_array_equal(one, wav[1])


@pytest.fixture(scope='module')
def generated(dev, tmp_path_factory):
    """one C2 batch (B = 32, 258 decoded frames) through SpecgramGenerator, with and without --gen-wav"""
    import yaml
    from semi_tts_amd.solver import SpecgramGenerator
    config = yaml.safe_load(open(os.path.join(REPO, 'config', 'supervised.yaml')))
    out = {}
    for gen_wav in (False, True):
        d = str(tmp_path_factory.mktemp('gen%d' % gen_wav))
        paras = types.SimpleNamespace(name='t', logdir=d, load=None, seed=1, cpu=False, verbose=False, batch_size=32, frames=216,
                                      n_batches=1, gen_wav=gen_wav)
        s = SpecgramGenerator(config, paras, 'test')
        s.load_data()
        s.set_model()
        torch.manual_seed(1)                 # the prenet's inference dropout (main.py seeds these the same way)
        np.random.seed(1234)                 # the initial phases of Griffin-Lim
        assert s.exec() == 32
        out[gen_wav] = os.path.join(d, 't_0k')
    return out


def test_gen_wav_writes_matching_waveforms(generated):
    files = sorted(os.listdir(generated[True]))
    assert sorted(os.listdir(generated[False])) == [f for f in files if not f.endswith('-pred.wav')]
    for f in os.listdir(generated[False]):                           # the .npy outputs do not change
        with open(os.path.join(generated[False], f), 'rb') as a, open(os.path.join(generated[True], f), 'rb') as b:
            assert a.read() == b.read(), f
    names = ['utt%05d' % i for i in range(32)]
    assert [f for f in files if f.endswith('-pred.wav')] == [n + '-pred.wav' for n in names]
    lin = torch.from_numpy(np.stack([np.load(os.path.join(generated[True], n + '-spec.npy')) for n in names]))
    B, T, _ = lin.shape
    assert T == 258
    np.random.seed(1234)                                              # the phases gen_specgram drew
    from semi_tts_amd.audio import draw_phases
    ph = draw_phases((B, F, T))
    ref = np.rint(np.clip(O.feat_to_wave(lin, torch.from_numpy(ph)), -1, 1) * 32767)
    for i, n in enumerate(names):
        with wave.open(os.path.join(generated[True], n + '-pred.wav'), 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, HOP * (T - 1))
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float64)
        assert np.abs(pcm - ref[i]).max() <= 1, (n, np.abs(pcm - ref[i]).max())


def test_griffin_lim_decoder_output(generated):
    """GL of the linear spectrogram the decoder produced for the C2 batch, 1 and 30 iterations"""
    names = ['utt%05d' % i for i in range(32)]
    lin = torch.from_numpy(np.stack([np.load(os.path.join(generated[True], n + '-spec.npy')) for n in names]))
    amp = O.denormalize_to_amp(lin.double().transpose(1, 2)).float()
    _check_gl(amp, _phases(tuple(amp.shape), 8), 'GL of the decoder output')
