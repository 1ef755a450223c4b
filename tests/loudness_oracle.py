"""Float64 oracle of st_loudness_batch / st_wave_gain (ITU-R BS.1770-4 integrated loudness, mono): coefficients from the formulas,
scipy.signal.lfilter per stage, hop sums, blocks, gates, gain and the int16 formula.  Shares no code with the product."""
import math

import numpy as np
from scipy.signal import lfilter

F_NONFINITE, F_SHORT, F_SILENT, F_PEAK, F_GAIN = 1, 2, 4, 8, 16


def coeffs(fs):
    fs = float(fs)
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    b1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a1 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return (b1, a1), ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def hop_len(fs):
    return (int(fs) + 5) // 10


def hop_energies(x, fs):
    """float64 e[h] over the H = L // hop full hops of the K-weighted signal"""
    x = np.asarray(x, np.float64)
    (b1, a1), (b2, a2) = coeffs(fs)
    with np.errstate(invalid='ignore', over='ignore'):
        y = lfilter(b2, a2, lfilter(b1, a1, x))
        hop = hop_len(fs)
        H = len(x) // hop
        return (y[:H * hop].reshape(H, hop) ** 2).sum(1)


def lk(z):
    with np.errstate(divide='ignore'):
        return -0.691 + 10.0 * np.log10(z)


def gate(e, fs):
    """blocks and gates from hop energies e (H,) -> dict(n_blocks, n_abs, n_rel, lufs, momentary_max, rel_gate, ungated, l)"""
    e = np.asarray(e, np.float64)
    H = len(e)
    nb = max(H - 3, 0)
    nan = float('nan')
    if nb == 0:
        return dict(n_blocks=0, n_abs=0, n_rel=0, lufs=nan, momentary_max=nan, rel_gate=nan, ungated=nan, l=np.zeros(0))
    z = (e[0:nb] + e[1:nb + 1] + e[2:nb + 2] + e[3:nb + 3]) / (4.0 * hop_len(fs))
    l = lk(z)
    res = dict(n_blocks=nb, momentary_max=float(l.max()), ungated=float(lk(z.mean())), l=l)
    A = l > -70.0
    if not A.any():
        res.update(n_abs=0, n_rel=0, lufs=-math.inf, rel_gate=-math.inf)
        return res
    g = float(lk(z[A].mean())) - 10.0
    R = A & (l > g)
    res.update(n_abs=int(A.sum()), n_rel=int(R.sum()), lufs=float(lk(z[R].mean())), rel_gate=g)
    return res


def measure(x, fs, target=None, peak_db=-1.0, max_gain_db=30.0, energies=None):
    """-> dict(e, n_blocks, n_abs, n_rel, flags, lufs, momentary_max, rel_gate, ungated, peak, gain, l).  energies: use these hop
    energies instead of filtering x (the gating stage alone)."""
    x32 = np.asarray(x, np.float32)
    nan = float('nan')
    if not np.isfinite(x32).all():
        e = hop_energies(x32, fs)
        return dict(e=e, n_blocks=max(len(e) - 3, 0), n_abs=0, n_rel=0, flags=F_NONFINITE, lufs=nan, momentary_max=nan, rel_gate=nan,
                    ungated=nan, peak=nan, gain=1.0, l=np.zeros(0))
    e = hop_energies(x32, fs) if energies is None else np.asarray(energies, np.float64)
    res = gate(e, fs)
    res['e'] = e
    res['peak'] = float(np.abs(x32.astype(np.float64)).max())
    res['gain'] = 1.0
    res['flags'] = 0
    if res['n_blocks'] == 0:
        res['flags'] = F_SHORT
    elif res['n_abs'] == 0:
        res['flags'] = F_SILENT
    elif target is not None and not math.isnan(target):
        g0 = 10.0 ** ((target - res['lufs']) / 20.0)
        gp = 10.0 ** (peak_db / 20.0) / res['peak']
        gm = 10.0 ** (max_gain_db / 20.0)
        res['gain'] = min(g0, gp, gm)
        if gp < g0 and gp <= gm:
            res['flags'] = F_PEAK
        elif gm < g0:
            res['flags'] = F_GAIN
    return res


def apply_gain(x, g):
    """one fp32 product a sample"""
    return np.asarray(x, np.float32) * np.float32(g)


def to_pcm16(y):
    """a 16-bit .wav writer's formula on float32 samples y"""
    return np.rint(np.clip(np.asarray(y, np.float32).astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)
