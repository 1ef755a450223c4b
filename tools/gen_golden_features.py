#!/usr/bin/env python3
"""Generate tests/golden/audio_features.npz by running the REAL reference's feature extraction.

Runs only in the build container (needs the reference tree, which never travels to the GPU box).  It imports the reference's
src/audio.py and calls AudioConverter.wave_to_feat / extract_feature_from_waveform on two synthetic utterances of different
lengths written as 16-bit .wav files.  torchaudio, librosa and pandas are not installed here, so they are stubbed: torchaudio by
a small shim on torch.stft (load, transforms.Spectrogram, transforms.MelScale with an `fb` tensor, functional.spectrogram:
torchaudio's own definitions), librosa and pandas by empty modules (nothing on this path calls them).  Recorded: the
reference's mel filterbank, the waveforms as the reference loaded them, the drawn SNR and stretch rates and noise, and every
output.  No reference source is copied anywhere.

    python tools/gen_golden_features.py [--ref /path/to/reference]      # (re)writes tests/golden/audio_features.npz
"""
import argparse
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'audio_features.npz')

import numpy as np   # noqa: E402
import torch         # noqa: E402

AUDIO = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
             use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])
LENGTHS = (12000, 19007)        # 44 and 70 frames at hop 275; the second not a multiple of the hop


def _torchaudio_shim():
    """the parts of torchaudio (0.4-era API) src/audio.py touches, restated on torch"""
    import wave
    ta = types.ModuleType('torchaudio')
    F = types.ModuleType('torchaudio.functional')
    T = types.ModuleType('torchaudio.transforms')

    def spectrogram(waveform, pad, window, n_fft, hop_length, win_length, power, normalized):
        if pad > 0:
            waveform = torch.nn.functional.pad(waveform, (pad, pad), 'constant')
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1])
        spec = torch.stft(x, n_fft, hop_length, win_length, window, center=True, pad_mode='reflect', normalized=False,
                          onesided=True, return_complex=True)
        spec = spec.reshape(shape[:-1] + spec.shape[-2:])
        if normalized:
            spec = spec / window.pow(2.0).sum().sqrt()
        return spec.abs().pow(power)
    F.spectrogram = spectrogram

    class Spectrogram(torch.nn.Module):
        def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2,
                     normalized=False):
            super().__init__()
            self.n_fft, self.win_length = n_fft, win_length or n_fft
            self.hop_length = hop_length or self.win_length // 2
            self.register_buffer('window', window_fn(self.win_length))
            self.pad, self.power, self.normalized = pad, power, normalized

        def forward(self, waveform):
            return spectrogram(waveform, self.pad, self.window, self.n_fft, self.hop_length, self.win_length, self.power,
                               self.normalized)

    class MelScale(torch.nn.Module):
        def __init__(self, n_mels=128, sample_rate=16000, f_min=0.0, f_max=None, n_stft=None):
            super().__init__()
            self.n_mels, self.sample_rate, self.f_min, self.f_max = n_mels, sample_rate, f_min, f_max
            self.register_buffer('fb', torch.empty(0))

        def forward(self, specgram):
            shape = specgram.size()
            specgram = specgram.reshape(-1, shape[-2], shape[-1])
            mel = torch.matmul(specgram.transpose(1, 2), self.fb).transpose(1, 2)
            return mel.reshape(shape[:-2] + mel.shape[-2:])
    T.Spectrogram, T.MelScale = Spectrogram, MelScale

    def load(path):
        with wave.open(str(path), 'rb') as w:
            sr, ch = w.getframerate(), w.getnchannels()
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
        return torch.from_numpy(np.ascontiguousarray(pcm.reshape(-1, ch).T, dtype=np.float32) / 32768.0), sr
    ta.load, ta.functional, ta.transforms = load, F, T
    ta.compliance = types.SimpleNamespace(kaldi=types.SimpleNamespace(mfcc=None))
    return {'torchaudio': ta, 'torchaudio.functional': F, 'torchaudio.transforms': T}


def utterance(L, seed):
    """a harmonic tone with a vibrato and gated silences (the clamp at 1e-5 is reached), quantised to 16 bits on write"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / AUDIO['sample_rate']
    f0 = 120 + 80 * rs.rand()
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.03 * np.sin(2 * np.pi * 5 * t))) / AUDIO['sample_rate']
    x = sum(0.5 / (h + 1) * np.sin((h + 1) * ph) for h in range(8))
    gate = (np.sin(2 * np.pi * 2.5 * t + rs.rand()) > -0.3).astype(np.float64)
    return 0.6 * x * gate + 0.003 * rs.randn(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    a = ap.parse_args()
    sys.modules.update(_torchaudio_shim())
    for m in ('librosa', 'pandas'):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, a.ref)
    sys.path.insert(0, REPO)
    from src.audio import load_audio_transform as ref_transform          # noqa: E402
    from lib.filters import create_mel_filterbank                         # noqa: E402
    from semi_tts_amd.audio import write_wav                              # noqa: E402
    torch.set_num_threads(1)
    conv = ref_transform(**AUDIO)
    rec = {'fb': create_mel_filterbank(AUDIO['sample_rate'], 2048, n_mels=80).astype(np.float32)}
    with tempfile.TemporaryDirectory() as d:
        for u, L in enumerate(LENGTHS):
            path = os.path.join(d, 'utt%d.wav' % u)
            write_wav(path, utterance(L, u), AUDIO['sample_rate'])
            wave = conv.load(path)
            rec['wav%d' % u] = wave[0].numpy()
            sp, msp = conv.extract_feature_from_waveform(wave.clone())
            rec['spec%d' % u], rec['mel%d' % u] = sp.numpy(), msp.numpy()
            # wave_to_feat: its draws are random.uniform (SNR, then stretch) and one torch.randn (the noise) in between
            random.seed(100 + u)
            torch.manual_seed(200 + u)
            msp_w, msp_aug, sp_w = conv.wave_to_feat(path)
            random.seed(100 + u)
            torch.manual_seed(200 + u)
            rec['snr%d' % u] = np.float64(random.uniform(*AUDIO['snr_range']))
            rec['noise%d' % u] = torch.randn(L).numpy()
            rec['stretch%d' % u] = np.float64(random.uniform(*AUDIO['time_stretch_range']))
            assert torch.equal(msp_w, msp.T) and torch.equal(sp_w, sp.T)
            rec['aug%d' % u] = msp_aug.numpy()
            # the SNR-off case (-1 in snr_range): the stretch is the only draw
            conv.snr_range = [-1, -1]
            random.seed(300 + u)
            _, msp_aug, _ = conv.wave_to_feat(path)
            random.seed(300 + u)
            rec['stretch_clean%d' % u] = np.float64(random.uniform(*AUDIO['time_stretch_range']))
            rec['aug_clean%d' % u] = msp_aug.numpy()
            conv.snr_range = AUDIO['snr_range']
    np.savez_compressed(OUT, **rec)
    print('wrote %s (%d bytes): %s' % (OUT, os.path.getsize(OUT), ', '.join('%s%s' % (k, tuple(np.shape(v))) for k, v in rec.items())))


if __name__ == '__main__':
    main()
