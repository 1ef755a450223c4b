"""Float64 yardstick of the MFCC and phone-segment features (st_audio_mfcc, st_segment_gather, semi_tts_amd.audio): the normalised
mel of tests/feat_oracle.py at the MFCC framing (win = int(0.025 sr), hop = int(0.010 sr)), then what the reference's
extract_mfcc_from_waveform (src/audio.py:132-154) asks of librosa, stated through scipy, which is librosa's own implementation:
librosa.feature.mfcc(S=mel, n_mfcc=13) = scipy.fft.dct(mel, axis=0, type=2, norm='ortho')[:13] and librosa.feature.delta(c, order=o) =
scipy.signal.savgol_filter(c, 9, deriv=o, polyorder=o, axis=-1, mode='interp').  `segment` is the cutting rule of
AudioProcessor.segment (src/audio.py:94-117) in plain Python, written from its description.  The reference's MFCC path itself needs
librosa and torchaudio, which cannot run where the fixtures are made, so there is no golden file for it: scipy is the reference."""
import numpy as np
import scipy.fft
import scipy.signal

import feat_oracle as O

N_MFCC, WIDTH = 13, 9


def mfcc_dims(sr):
    """(win, hop) of the MFCC framing (src/audio.py:33-34)"""
    return int(25 / 1000 * sr), int(10 / 1000 * sr)


def mfcc(x, fb, sr=O.SR, n_fft=O.N_FFT, preemph=O.PREEMPH, n_mfcc=N_MFCC):
    """x (L,) -> (mfcc (3 * n_mfcc, T), mel (n_mels, T)) float64 numpy, T = 1 + L // hop"""
    win, hop = mfcc_dims(sr)
    _, mel = O.features(x, fb, n_fft=n_fft, hop=hop, win=win, preemph=preemph)
    mel = mel.numpy()
    c = scipy.fft.dct(mel, axis=0, type=2, norm='ortho')[:n_mfcc]
    d1 = scipy.signal.savgol_filter(c, WIDTH, deriv=1, polyorder=1, axis=-1, mode='interp')
    d2 = scipy.signal.savgol_filter(c, WIDTH, deriv=2, polyorder=2, axis=-1, mode='interp')
    return np.concatenate([c, d1, d2], axis=0), mel


def segment(feat, boundary, min_segment_len=2):
    """feat (T, D) array, boundary ratios -> (S, max_len, D): a boundary b ends a piece at frame round(b * T) (halves to even); a piece
    shorter than min_segment_len is not emitted and the next piece starts where the last emitted one ended; max_len is the longest
    candidate piece, emitted or not"""
    feat = np.asarray(feat)
    T, D = feat.shape
    cuts, start, max_len = [], 0, 0
    for b in boundary:
        end = round(b * T)
        max_len = max(max_len, end - start)
        if end - start >= min_segment_len:
            cuts.append((start, end))
            start = end
    out = np.zeros((len(cuts), max_len, D), feat.dtype)
    for s, (lo, hi) in enumerate(cuts):
        out[s, :hi - lo] = feat[lo:hi]
    return out
