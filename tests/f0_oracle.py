"""float64 numpy oracle of st_f0_yin and st_f0_path_scores (the definitions of include/semitts.h), with the robustness test and the
F0 interval the GPU tests assert on, and the test signals."""
import itertools

import numpy as np


def eps(W, tau_max):
    """relative error bound of an fp32 d'(tau): d carries at most W + 2 roundings (all terms non-negative), c tau_max more on top of
    those of its terms, the product and the quotient two more"""
    return (2 * W + tau_max + 8) * 2.0 ** -24


def frame_count(L, hop):
    return 1 + L // hop


def slices(x, hop, W, tau_max, dtype=np.float64):
    """(T, W + tau_max): row t = x[s0 .. s0 + W + tau_max), s0 = t hop - W // 2, zero outside the utterance"""
    x = np.asarray(x, dtype)
    T, half = frame_count(len(x), hop), W // 2
    xp = np.concatenate([np.zeros(half, dtype), x, np.zeros((T - 1) * hop + W + tau_max, dtype)])
    return xp[np.arange(T)[:, None] * hop + np.arange(W + tau_max)[None, :]]


def cmnd(x, hop, W, tau_max, dtype=np.float64):
    """d'(tau), (T, tau_max + 1), evaluated in `dtype` (float32: a stand-in for the kernel's arithmetic, in numpy's summation order)"""
    seg = slices(x, hop, W, tau_max, dtype)
    d = np.stack([((seg[:, :W] - seg[:, t:t + W]) ** 2).sum(axis=1, dtype=dtype) for t in range(tau_max + 1)], axis=1)
    c = np.cumsum(d[:, 1:], axis=1, dtype=dtype)
    out = np.ones_like(d)
    tau = np.arange(1, tau_max + 1).astype(dtype)
    with np.errstate(all='ignore'):
        out[:, 1:] = np.where(c > 0, d[:, 1:] * tau / c, dtype(1))
    return out


def pick(dp, sr, tau_min, tau_max, threshold, dtype=np.float64):
    """the search and the refinement on one frame's d' -> (f0, aper, tau*) (tau* = 0: unvoiced)"""
    rng = dp[tau_min:tau_max + 1]
    below = np.nonzero(rng < threshold)[0]
    if len(below) == 0:
        return dtype(0), rng.min(), 0
    t = tau_min + int(below[0])
    while t < tau_max and dp[t + 1] < dp[t]:
        t += 1
    a, b = dp[t - 1], dp[t]
    delta = dtype(0)
    if t < tau_max and a > b:
        c = dp[t + 1]
        delta = dtype(0.5) * (a - c) / ((a - b) + (c - b))
    return dtype(sr) / (dtype(t) + delta), b, t


def yin(x, sr, hop, W, tau_min, tau_max, threshold):
    """-> dict of per-frame arrays: f0, aper, tau (tau*, 0 where unvoiced), robust, f0_lo, f0_hi (float64 throughout).  A frame is
    robust when every comparison of the definition has a relative margin above 2 eps; [f0_lo, f0_hi] is sr / (tau* + delta) over the
    eight corners a (1 +- eps), b (1 +- eps), c (1 +- eps), widened by 2^-21 f0 for the final division."""
    e = eps(W, tau_max)
    dps = cmnd(x, hop, W, tau_max)
    T = dps.shape[0]
    out = {k: np.zeros(T) for k in ('f0', 'aper', 'f0_lo', 'f0_hi')}
    out['tau'], out['robust'] = np.zeros(T, np.int64), np.zeros(T, bool)
    for i, dp in enumerate(dps):
        f0, aper, t = pick(dp, sr, tau_min, tau_max, threshold)
        out['f0'][i], out['aper'][i], out['tau'][i] = f0, aper, t
        rng = dp[tau_min:tau_max + 1]
        if t == 0:
            out['robust'][i] = not (rng < threshold * (1 + 2 * e)).any()
            continue
        t0 = tau_min + int(np.nonzero(rng < threshold)[0][0])
        ok = not (dp[tau_min:t0] < threshold * (1 + 2 * e)).any() and dp[t0] < threshold * (1 - 2 * e)
        for u in range(t0, t):                                      # the descending steps
            ok = ok and dp[u + 1] * (1 + 2 * e) < dp[u]
        lo = hi = f0
        if t < tau_max:
            a, b, c = dp[t - 1], dp[t], dp[t + 1]
            ok = ok and c >= b * (1 + 2 * e) and abs(a - b) > 2 * e * b
            if a > b:
                fs = []
                for sa, sb, sc in itertools.product((1 - e, 1 + e), repeat=3):
                    den = a * sa - 2 * b * sb + c * sc
                    if den <= 0:
                        ok = False
                    else:
                        fs.append(sr / (t + 0.5 * (a * sa - c * sc) / den))
                if fs:
                    lo, hi = min(fs), max(fs)
        out['robust'][i] = ok
        out['f0_lo'][i], out['f0_hi'][i] = lo - 2.0 ** -21 * f0, hi + 2.0 ** -21 * f0
    return out


def yin_f32(x, sr, hop, W, tau_min, tau_max, threshold):
    """the same definition evaluated in float32 numpy -> (f0, aper, tau) arrays: what an fp32 implementation may give"""
    dps = cmnd(np.asarray(x, np.float32), hop, W, tau_max, np.float32)
    r = [pick(dp, sr, tau_min, tau_max, np.float32(threshold), np.float32) for dp in dps]
    return np.array([v[0] for v in r], np.float32), np.array([v[1] for v in r], np.float32), np.array([v[2] for v in r])


def path_scores(fx, fy, path, path_len):
    """float64 oracle of st_f0_path_scores for one pair -> (counts (n_pairs, n_both, n_vuv, n_gross), sum c^2, sum c, sum |c|)"""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    p = np.asarray(path)[:int(path_len)]
    a, c = fx[p[:, 0]], fy[p[:, 1]]
    with np.errstate(invalid='ignore'):
        va, vc = a > 0, c > 0
    both = va & vc
    a, c = a[both], c[both]
    cents = 1200.0 * np.log2(a / c)
    return ((len(p), int(both.sum()), int((va != vc).sum()), int((np.abs(a - c) > 0.2 * c).sum())),
            float((cents ** 2).sum()), float(cents.sum()), float(np.abs(cents).sum()))


# ---------------------------------------------------------------- test signals
SIGNALS = ('tone', 'vib', 'glide', 'noisy15', 'noise', 'silence', 'onoff', 'hi', 'lo')
# (sample rate, hop, tau_min, tau_max, W, samples): the configuration's framing, a small one, an odd one
FRAMINGS = {'config': (22050, 220, 44, 368, 736, 22050), 'small': (2000, 20, 5, 40, 80, 2000), 'odd': (2000, 7, 3, 65, 63, 1003)}


def harmonic(f, sr, n_harm=5):
    """sum of the first n_harm harmonics (amplitude 1 / k, those below 0.45 sr) of the instantaneous frequency f (Hz per sample)"""
    phase = 2 * np.pi * np.cumsum(np.asarray(f, np.float64)) / sr
    y = np.zeros(len(phase))
    for k in range(1, n_harm + 1):
        y += np.where(k * np.asarray(f) < 0.45 * sr, np.sin(k * phase) / k, 0.0)
    return 0.3 * y


def signal(name, framing):
    """one of SIGNALS at one of FRAMINGS as float32: a harmonic sum around the geometric middle of the lag range with RandomState(3)
    noise at 30 dB SNR unless the name says otherwise"""
    sr, _, tau_min, tau_max, _, n = FRAMINGS[framing]
    rs = np.random.RandomState(3)
    t = np.arange(n) / sr
    fc = sr / np.sqrt(tau_min * tau_max)
    noise = rs.randn(n)
    f = np.full(n, fc)
    snr = 30.0
    if name == 'vib':
        f = fc * (1 + 0.03 * np.sin(2 * np.pi * 5 * t))
    elif name == 'glide':
        f = fc * np.linspace(0.7, 1.4, n)
    elif name == 'noisy15':
        snr = 15.0
    elif name == 'hi':
        f = np.full(n, 0.9 * sr / tau_min)
    elif name == 'lo':
        f = np.full(n, 1.1 * sr / tau_max)
    if name == 'silence':
        return np.zeros(n, np.float32)
    if name == 'noise':
        return (0.1 * noise).astype(np.float32)
    y = harmonic(f, sr)
    if name == 'onoff':                                             # 2 Hz gating over a noise floor 40 dB below the tone
        y = y * (np.sin(2 * np.pi * 2 * t) > 0)
        snr = 40.0
    y = y + noise * np.sqrt(np.mean(harmonic(f, sr) ** 2) / np.mean(noise ** 2) * 10 ** (-snr / 10))
    return y.astype(np.float32)
