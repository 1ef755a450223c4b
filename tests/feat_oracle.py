"""Float64 torch CPU restatement of the reference's feature extraction (src/audio.py:156-177, 329-395, 409-437): pre-emphasis ->
torch.stft (centre, reflect padding, periodic Hann window of `win` in n_fft) -> magnitude -> mel filterbank -> dB normalisation,
with the noise of add_noise / snr_coeff added first when asked.  The yardstick of tests/test_features_host.py and
tests/test_gpu_features.py."""
import numpy as np
import torch

N_FFT, HOP, WIN, SR, PREEMPH = 2048, 275, 1102, 22050, 0.97


def snr_coeff(x, n, snr):
    """sqrt(sum x^2 / sum n^2 * 10^(-snr / 10))"""
    return float(np.sqrt((x ** 2).sum() / (n ** 2).sum() * 10 ** (-snr / 10)))


def normalize(a):
    return torch.clamp((20 * torch.log10(torch.clamp(a, min=1e-5)) - 20 + 100) / 100, 0, 1)


def features(x, fb, n_fft=N_FFT, hop=HOP, win=WIN, preemph=PREEMPH, noise=None, snr=None, dtype=torch.float64):
    """x (L,) -> (linear (F, T), mel (n_mels, T)) normalised, float64 (or `dtype`); noise / snr: add coeff * noise first"""
    x = torch.as_tensor(np.asarray(x, np.float64)).to(dtype)
    if snr is not None:
        n = torch.as_tensor(np.asarray(noise, np.float64)).to(dtype)
        x = x + snr_coeff(x.double().numpy(), n.double().numpy(), snr) * n
    if preemph:
        x = torch.cat([x[:1], x[1:] - preemph * x[:-1]])
    spec = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=dtype), center=True, pad_mode='reflect', normalized=False,
                      onesided=True, return_complex=True).abs()
    mel = torch.as_tensor(np.asarray(fb)).to(dtype) @ spec
    return normalize(spec), normalize(mel)


def stretch_dims(rate, sr=SR, frame_length_ms=50, frame_shift_ms=12.5):
    """(win, hop) of src/audio.py:366-373 at stretch `rate`"""
    stretch_sr = int(sr * rate)
    return int(frame_length_ms / 1000 * stretch_sr), int(frame_shift_ms / 1000 * stretch_sr)
