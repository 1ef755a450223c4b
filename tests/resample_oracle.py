"""Float64 numpy oracle of the sample-rate conversion (st_resample_batch, semi_tts_amd.audio.resample), written from the
definition in include/semitts.h / DESIGN.md 3.14 -- Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99, the defaults of
torchaudio.functional.resample:

    g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, W = lpw o / base, tau_m = m o / n
    y[m] = (base / o) sum_{|i - tau_m| < W} sinc(pi base (i - tau_m) / o) cos^2(pi base (i - tau_m) / (2 lpw o)) x[i]
    x[i] = 0 outside [0, L), m = 0 .. ceil(n L / o) - 1

table64: the weights per phase p = m mod n.  resample_compact: the sum above, over a table (float64, or the float32 one the
kernel reads).  resample_full: the same filter in the clamped-window form of 2 ceil(W) + o taps per phase, as a strided correlation."""
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99


def ratio(orig_sr, new_sr):
    g = math.gcd(orig_sr, new_sr)
    return orig_sr // g, new_sr // g


def out_len(L, orig_sr, new_sr):
    o, n = ratio(orig_sr, new_sr)
    return -((-n * L) // o)


def table64(orig_sr, new_sr, lpw=LPW, rolloff=ROLLOFF):
    """-> (o, n, taps, first (n,) int, table (n, taps) float64, W): output m of phase p is sum_k table[p, k] x[floor(tau_m) + first[p] + k];
    entries with |i - tau| >= W are exactly 0"""
    o, n = ratio(orig_sr, new_sr)
    base = min(o, n) * rolloff
    W = lpw * o / base
    frac = ((np.arange(n, dtype=np.int64) * o) % n) / float(n)
    first = np.floor(frac - W).astype(np.int64) + 1
    last = np.ceil(frac + W).astype(np.int64) - 1
    taps = int((last - first + 1).max())
    t = (first[:, None] + np.arange(taps)[None, :]) - frac[:, None]
    a = np.pi * base * t / o
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    h = (base / o) * sinc * np.cos(a / (2.0 * lpw)) ** 2
    return o, n, taps, first, np.where(np.abs(t) < W, h, 0.0), W


def resample_compact(x, orig_sr, new_sr, table=None, first=None, want_abs=False):
    """the definition's sum in float64 over `table` / `first` (default: table64's); want_abs: also sum_k |h_p[k] x[i_k]| per output"""
    x = np.asarray(x, np.float64)
    o, n, taps, first64, tab64, _ = table64(orig_sr, new_sr)
    table = tab64 if table is None else np.asarray(table, np.float64)
    first = first64 if first is None else np.asarray(first, np.int64)
    taps = table.shape[1]
    L = len(x)
    M = out_len(L, orig_sr, new_sr)
    m = np.arange(M, dtype=np.int64)
    p = m % n
    idx = (m * o // n + first[p])[:, None] + np.arange(taps)[None, :]
    xv = np.where((idx >= 0) & (idx < L), x[np.clip(idx, 0, L - 1)], 0.0)
    prod = table[p] * xv
    y = np.zeros(M)
    for k in range(taps):                          # ascending taps, like the kernel (in float64 the order is immaterial to the bound)
        y += prod[:, k]
    return (y, np.abs(prod).sum(1)) if want_abs else y


def resample_full(x, orig_sr, new_sr, lpw=LPW, rolloff=ROLLOFF):
    """the 'full' form: width = ceil(W), every phase has 2 width + o taps at input offsets -width .. width + o - 1 from q o (m = q n + p),
    the window argument clamped to [-lpw, lpw] instead of cut"""
    x = np.asarray(x, np.float64)
    o, n = ratio(orig_sr, new_sr)
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    j = np.arange(-width, width + o, dtype=np.float64)
    t = (j[None, :] / o - np.arange(n, dtype=np.float64)[:, None] / n) * base        # (n, 2 width + o)
    t = np.clip(t, -lpw, lpw)
    window = np.cos(t * np.pi / lpw / 2.0) ** 2
    a = t * np.pi
    kern = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a)) * window * (base / o)
    L = len(x)
    M = out_len(L, orig_sr, new_sr)
    Q = -(-M // n)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o + Q * o)])
    frames = np.stack([xp[q * o:q * o + 2 * width + o] for q in range(Q)])                # (Q, 2 width + o)
    return (frames @ kern.T).reshape(-1)[:M]
