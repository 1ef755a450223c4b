"""float64 numpy restatement of the reference's mel -> linear step (src/audio.py:194-205, with _db_to_amp / _denormalize of
:278-288), the oracle of st_mel_to_linear.  The basis -- pinverse(filterbank) transposed, (n_mels, F) -- is taken as given, in
float32: what is checked against this file is the product and the denormalisation, not the pseudo-inverse (test_vocode_host.py
compares that with torch.pinverse).
"""
import numpy as np

MIN_LEVEL_DB = -100      # src/audio.py:17
REF_LEVEL_DB = 20        # src/audio.py:18
U = 2.0 ** -24           # unit roundoff of float32


def db_to_amp(x):
    """src/audio.py:281-282"""
    return 10.0 ** (0.05 * x)


def denormalize(feat):
    """src/audio.py:287-288"""
    return MIN_LEVEL_DB + np.clip(feat, 0.0, 1.0) * -MIN_LEVEL_DB


def amplitude(mel, normalized=True):
    """the `melspecgram` of src/audio.py:203 from the float32 input, in float64 (normalized False: the input itself)"""
    mel = np.asarray(mel, np.float32).astype(np.float64)
    return db_to_amp(denormalize(mel) + REF_LEVEL_DB) if normalized else mel


def mel_to_linear(mel_btm, basis, normalized=True):
    """src/audio.py:202-205 time-major: mel (..., T, n_mels), basis (n_mels, F) float32 -> (lin (..., T, F) float64, signed;
    mag (..., T, F) = sum_m |basis[m, k]| |a[m]|, the scale of the dot product's rounding-error bound)"""
    a = amplitude(mel_btm, normalized)
    w = np.asarray(basis, np.float32).astype(np.float64)
    return a @ w, np.abs(a) @ np.abs(w)


def bound(mag, n_mels, normalized):
    """per-element bound on |device - oracle|.  normalized False: the standard bound of an n-term float32 dot product, here an
    fmaf chain -- (n_mels + 2) u sum |w| |a| (n roundings of the chain, the float32 inputs exact, one for the final abs / store
    slack).  normalized True: the amplitudes themselves carry a relative error: the argument y = 0.05 (db + 20) of 10^y is
    rounded to about 1e-6 absolute at |y| <= 4, times ln 10 in the result, plus a few u of powf -- 128 u covers it."""
    return (n_mels + (128 if normalized else 2)) * U * mag
