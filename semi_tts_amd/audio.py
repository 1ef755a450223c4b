"""Synthesis side of the reference's src/audio.py: linear spectrogram -> waveform by Griffin-Lim on the HIP kernels
(semi_tts_amd/csrc/audio.hip, include/semitts.h st_griffin_lim / st_stft_fwd / st_istft).

    conv = load_audio_transform(**config['data']['audio'])
    wav, sr = conv.feat_to_wave(linear_pred)          # (T, F) or (B, T, F), CPU or device tensor -> float64 numpy
    write_wav('utt-pred.wav', wav[0], sr)

Only the linear branch of feat_to_wave (src/audio.py:397-407) is here: the mel -> linear pseudo-inverse (:194-205) needs the
reference's librosa filterbank (lib/filters.py) and raises NotImplementedError.  Training-side feature extraction is not here.
"""
import wave

import numpy as np
import torch

from . import ops

GFL_ITER = 30                     # src/audio.py:15
MIN_LEVEL_DB = -100               # src/audio.py:17
REF_LEVEL_DB = 20                 # src/audio.py:18
INV_PREEMPHASIS_COEFF = 0.97      # the literal of src/audio.py:276 (_inv_preemphasis ignores preemphasis_coeff)
SUPPORTED_N_FFT = (512, 1024, 2048, 4096)

# the shipped configs' data.audio (identical in all three YAMLs): num_freq 1025, 12.5 / 50 ms at 22050 Hz
DEFAULT_N_FFT, DEFAULT_HOP, DEFAULT_WIN = 2048, 275, 1102


def stft_dims(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    """(n_fft, hop, win) exactly as AudioProcessor.__init__ derives them (src/audio.py:28-32)"""
    return (num_freq - 1) * 2, int(frame_shift_ms / 1000 * sample_rate), int(frame_length_ms / 1000 * sample_rate)


def check_dims(n_fft, hop, win, T):
    """raise ValueError for what the kernels do not take, before anything touches a device"""
    if n_fft not in SUPPORTED_N_FFT:
        raise ValueError('Griffin-Lim: n_fft %d not supported (one of %s)' % (n_fft, SUPPORTED_N_FFT))
    if not (0 < 2 * hop <= win <= n_fft):
        raise ValueError('Griffin-Lim: need 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)' % (hop, win, n_fft))
    if hop * (T - 1) <= n_fft // 2:
        # torch.stft's reflect padding of n_fft // 2 needs a longer signal than the hop * (T - 1) samples the iSTFT gives
        raise ValueError('Griffin-Lim: %d frames are too few: reflect padding needs hop * (T - 1) > n_fft // 2 (hop %d, n_fft %d), '
                         'i.e. T >= %d' % (T, hop, n_fft, n_fft // 2 // hop + 2))


def draw_phases(shape):
    """initial phases as src/audio.py:214-216: uniform in [0, 2 pi) from np.random, wrapped by np.angle(np.exp(1j phi)), float32"""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('semi_tts_amd.audio: Griffin-Lim runs on the HIP kernels and needs a GPU; there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _run(feat_btf, phases, n_fft, hop, win, n_iter, normalized, power, post):
    """feat_btf: (B, T, F) view, any strides; phases: (B, F, T) array/tensor or None (drawn).  -> (B, hop * (T - 1)) device tensor"""
    B, T, F = feat_btf.shape
    if F != n_fft // 2 + 1:
        raise ValueError('Griffin-Lim: %d frequency bins, expected n_fft // 2 + 1 = %d' % (F, n_fft // 2 + 1))
    check_dims(n_fft, hop, win, T)
    if phases is None:
        phases = draw_phases((B, F, T))
    phases = torch.as_tensor(phases, dtype=torch.float32)
    if tuple(phases.shape) != (B, F, T):
        raise ValueError('Griffin-Lim: phases of shape %s, expected %s' % (tuple(phases.shape), (B, F, T)))
    dev = feat_btf.device if feat_btf.is_cuda else _device()
    feat_btf = feat_btf.to(dev, torch.float32)
    return ops.griffin_lim(feat_btf, phases.to(dev).contiguous(), n_fft, hop, win, n_iter=n_iter, normalized=normalized,
                           power=power, post=post)


def griffin_lim(amp, phases=None, n_iter=GFL_ITER, n_fft=DEFAULT_N_FFT, hop=DEFAULT_HOP, win=DEFAULT_WIN):
    """AudioProcessor._griffin_lim (src/audio.py:208-226) on the device: magnitude (F, T) or (B, F, T) -> waveform (L,) or (B, L),
    L = hop * (T - 1), before inverse pre-emphasis.  phases: the initial phases, shaped like amp (None: drawn from np.random)."""
    squeeze = amp.dim() == 2
    a = amp.unsqueeze(0) if squeeze else amp
    if phases is not None and squeeze:
        phases = torch.as_tensor(phases).unsqueeze(0)
    wav = _run(a.transpose(1, 2), phases, n_fft, hop, win, n_iter, normalized=False, power=1.0, post=0)
    return wav[0] if squeeze else wav


class AudioConverter:
    """The synthesis methods of the reference's AudioProcessor / AudioConverter (src/audio.py:23, :292) for the linear branch."""

    def __init__(self, num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear=True,
                 **_unused):
        self.n_fft, self.hop_length, self.win_length = stft_dims(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
        self.num_freq, self.n_mels = num_freq, num_mels
        self.preemphasis_coeff = preemphasis_coeff       # read by the reference's _preemphasis only, never by the inverse (:274-276)
        self.sr = sample_rate
        self.use_linear = use_linear
        self.feat_dim = (num_mels, num_freq) if use_linear else (num_mels, None)      # src/audio.py:307

    def specgram_to_waveform(self, specgram, power=1.0, inv_preemphasis=True, isAmp=False, phases=None, n_iter=GFL_ITER):
        """src/audio.py:179-192: specgram (F, T) or (B, F, T) -> float64 numpy waveform(s), clipped to [-1, 1].
        Denormalisation, Griffin-Lim, inverse pre-emphasis and clip all run on the device."""
        squeeze = specgram.dim() == 2
        s = specgram.unsqueeze(0) if squeeze else specgram
        if phases is not None and squeeze:
            phases = torch.as_tensor(phases).unsqueeze(0)
        post = ops.GL_CLIP | (ops.GL_INV_PREEMPHASIS if inv_preemphasis else 0)
        wav = _run(s.transpose(1, 2), phases, self.n_fft, self.hop_length, self.win_length, n_iter, normalized=not isAmp,
                   power=power, post=post)
        wav = wav.cpu().numpy().astype(np.float64)
        return wav[0] if squeeze else wav

    def feat_to_wave(self, feat, phases=None):
        """src/audio.py:397-407: the decoder's (T, F) or (B, T, F) linear output -> (float64 waveform(s), sample rate).
        The reference transposes to (F, T) and draws its phases in that shape; here the first kernel reads (B, T, F) directly."""
        if feat.size(-1) == self.feat_dim[0] and feat.size(-1) != self.num_freq:
            raise NotImplementedError('feat_to_wave: mel input (%d bins): the mel -> linear pseudo-inverse of src/audio.py:194-205 '
                                      "needs librosa's filterbank and is not implemented; pass the linear spectrogram" % feat.size(-1))
        return self.specgram_to_waveform(feat.transpose(-2, -1), phases=phases), self.sr

    def gen_wav_device(self, lin, phases=None):
        """feat_to_wave for a device batch (B, T, F) without the host copy: -> (B, hop * (T - 1)) device tensor (SpecgramGenerator)"""
        if lin.size(-1) != self.num_freq:
            raise NotImplementedError('gen_wav: only the linear spectrogram (%d bins) is vocoded, got %d' % (self.num_freq, lin.size(-1)))
        return _run(lin, phases, self.n_fft, self.hop_length, self.win_length, GFL_ITER, normalized=True, power=1.0,
                    post=ops.GL_CLIP | ops.GL_INV_PREEMPHASIS)


def load_audio_transform(num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear=True,
                         **kwargs):
    """src/audio.py:439-448 (the training-side arguments -- snr_range, time_stretch_range, segment_* -- are accepted and unused)"""
    return AudioConverter(num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear, **kwargs)


def write_wav(path, wav, sr):
    """16-bit PCM mono .wav through the standard library (soundfile's default subtype for .wav): round(clip(x, -1, 1) * 32767)"""
    wav = np.asarray(wav, dtype=np.float64).reshape(-1)
    pcm = np.rint(np.clip(wav, -1.0, 1.0) * 32767.0).astype('<i2')
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(pcm.tobytes())
