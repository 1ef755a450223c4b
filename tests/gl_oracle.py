"""float64 torch CPU restatement of the reference's synthesis path (src/audio.py), the oracle of semi_tts_amd.audio.

The reference's audio module imports torchaudio and librosa (not installed), so no golden is recorded from it: this restates the
same lines with torch.stft / torch.istft (complex API; torch.istft without `length` = lib/istft.py's trim of n_fft // 2 at both
ends) and scipy.signal.lfilter.
"""
import numpy as np
import torch
from scipy import signal

GFL_ITER = 30            # src/audio.py:15
MIN_LEVEL_DB = -100      # src/audio.py:17
REF_LEVEL_DB = 20        # src/audio.py:18
N_FFT, HOP, WIN = 2048, 275, 1102     # (num_freq - 1) * 2, int(12.5 / 1000 * 22050), int(50 / 1000 * 22050)  (src/audio.py:28-32)


def window(win=WIN, dtype=torch.float64):
    return torch.hann_window(win, dtype=dtype)                                             # src/audio.py:35 (periodic)


def stft(x, n_fft=N_FFT, hop=HOP, win=WIN):
    """src/audio.py:234-246: x (B, L) -> (B, F, T) complex"""
    return torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=win, window=window(win, x.dtype), center=True,
                      pad_mode='reflect', normalized=False, onesided=True, return_complex=True)


def istft(y, n_fft=N_FFT, hop=HOP, win=WIN):
    """src/audio.py:248-262 (lib/istft.py): (B, F, T) complex -> (B, hop * (T - 1))"""
    return torch.istft(y, n_fft=n_fft, hop_length=hop, win_length=win, window=window(win, y.real.dtype), center=True,
                       normalized=False, onesided=True)


def denormalize_to_amp(feat, power=1.0):
    """src/audio.py:186-188, :281-288"""
    db = MIN_LEVEL_DB + torch.clamp(feat, min=0, max=1) * -MIN_LEVEL_DB
    return (10 ** (0.05 * (db + REF_LEVEL_DB))) ** power


def griffin_lim(magnitude, phases, n_iter=GFL_ITER, **dims):
    """src/audio.py:208-226 with given initial phases: magnitude, phases (B, F, T) -> (B, L)"""
    magnitude = magnitude.abs()
    y = torch.polar(magnitude, phases.to(magnitude.dtype))                                # _to_complex (:264-268)
    x = istft(y, **dims)
    for _ in range(n_iter):
        y = stft(x, **dims)
        ph = torch.angle(y)                                                                # _get_phase (:270-271); angle(0) = 0
        y = torch.polar(magnitude, ph)
        x = istft(y, **dims)
    return x


def inv_preemphasis(wav):
    """src/audio.py:274-276: the literal 0.97, along the last axis"""
    return signal.lfilter([1], [1, -0.97], wav)


def inv_preemphasis_loop(wav):
    """the same recurrence y[n] = x[n] + 0.97 y[n-1], spelled out"""
    wav = np.asarray(wav, dtype=np.float64)
    out = np.empty_like(wav)
    for idx in np.ndindex(*wav.shape[:-1]):
        y = 0.0
        for n in range(wav.shape[-1]):
            y = wav[idx + (n,)] + 0.97 * y
            out[idx + (n,)] = y
    return out


def inv_preemphasis_blocked(wav, chunk=16, tile=16384):
    """the blocked scan of the library's final kernel (audio.hip gl_ola_post_kernel), in float64: 16-sample chunks, a scan of the
    chunk ends, a carry from one tile into the next"""
    wav = np.asarray(wav, dtype=np.float64)
    a = 0.97
    out = np.empty_like(wav)
    for idx in np.ndindex(*wav.shape[:-1]):
        x = wav[idx]
        carry = 0.0
        for base in range(0, x.shape[0], tile):
            seg = np.zeros(tile)
            n = min(tile, x.shape[0] - base)
            seg[:n] = x[base:base + n]
            seg = seg.reshape(-1, chunk)
            local = np.zeros(seg.shape[0])
            for c in range(seg.shape[0]):
                y = 0.0
                for q in range(chunk):
                    y = seg[c, q] + a * y
                local[c] = y
            m = a ** chunk
            ends = np.empty_like(local)           # inclusive scan of chunk ends
            acc = 0.0
            for c in range(local.shape[0]):
                acc = local[c] + m * acc
                ends[c] = acc
            res = np.empty_like(seg)
            for c in range(seg.shape[0]):
                yp = carry if c == 0 else ends[c - 1] + m ** c * carry
                for q in range(chunk):
                    yp = seg[c, q] + a * yp
                    res[c, q] = yp
            carry = res[-1, -1]
            out[idx][base:base + n] = res.reshape(-1)[:n]
    return out


def feat_to_wave(feat_btf, phases, n_iter=GFL_ITER):
    """src/audio.py:397-407 + 179-192 for the linear branch: (B, T, F) normalised -> float64 waveform (B, L), clipped"""
    spec = feat_btf.double().transpose(-2, -1)                                              # (:401)
    amp = denormalize_to_amp(spec)
    wav = griffin_lim(amp, phases.double(), n_iter).numpy()
    return np.clip(inv_preemphasis(wav), -1, 1)
