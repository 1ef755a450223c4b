"""The numpy oracle of the alignment kernels (st_xcorr_delay, st_sisdr_batch; the definitions are in include/semitts.h).

Input that is 16-bit PCM / 32768 (`is_pcm`) is taken to integers: every sum is then int64 and EXACT, and its float64 value (times a
power of two) is exact too, so the GPU must agree bit for bit.  Any other input is summed in numpy.longdouble (64 bits of mantissa on
x86: the products, 48 bits, are exact there and the sum errs by 2^-11 of the float64 bound) and rounded once, so the oracle's own
error takes nothing visible of the bound the GPU is held to; `corr_abs` gives the sum of |x y| that bound is made of.  The decision and the score formulas are written as the header states them."""
import numpy as np

SCALE = 32768.0


def is_pcm(v):
    v = np.asarray(v, np.float64)
    return bool(np.isfinite(v).all() and (np.abs(v) <= 1.0).all() and (v * SCALE == np.rint(v * SCALE)).all())


def _ints(v):
    return np.rint(np.asarray(v, np.float64) * SCALE).astype(np.int64)


def lag_range(Lx, Ly, d):
    """the n of r[d]: [lo, hi), empty when hi <= lo"""
    return max(0, -d), min(Lx, Ly - d)


def corr(x, y, D):
    """r[d], d = -D .. D, as float64 (column d + D): exact for PCM input, a longdouble sum rounded once otherwise"""
    x, y = np.asarray(x), np.asarray(y)
    pcm = is_pcm(x) and is_pcm(y)
    xs, ys = (_ints(x), _ints(y)) if pcm else (x.astype(np.longdouble), y.astype(np.longdouble))
    out = np.zeros(2 * D + 1, np.int64 if pcm else np.longdouble)
    for d in range(-D, D + 1):
        lo, hi = lag_range(len(xs), len(ys), d)
        if hi > lo:
            out[d + D] = np.dot(xs[lo:hi], ys[lo + d:hi + d])
    if pcm:
        assert np.abs(out).max() < 2 ** 53
        return out.astype(np.float64) * 2.0 ** -30
    return out.astype(np.float64)


def corr_abs(x, y, D):
    """(sum |x y|, number of terms) per lag, float64: what the bound n 2^-53 sum |x_n y_{n + d}| is made of"""
    xs, ys = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
    s, n = np.zeros(2 * D + 1), np.zeros(2 * D + 1)
    for d in range(-D, D + 1):
        lo, hi = lag_range(len(xs), len(ys), d)
        if hi > lo:
            s[d + D], n[d + D] = np.dot(xs[lo:hi], ys[lo + d:hi + d]), hi - lo
    return s, n


def lag_order(D):
    """the lags in the order ties are broken: 0, +1, -1, +2, -2, ..."""
    out = [0]
    for k in range(1, D + 1):
        out += [k, -k]
    return out


def sum_sq(v):
    v = np.asarray(v)
    if is_pcm(v):
        return float(np.dot(_ints(v), _ints(v))) * 2.0 ** -30
    return float(np.dot(v.astype(np.longdouble), v.astype(np.longdouble)))


def delay(x, y, D):
    """-> dict(delay, coef (float32), corr): the lag of the largest r, ties in lag_order; a NaN in r: delay 0, coef NaN"""
    r = corr(x, y, D)
    if np.isnan(r).any():
        return dict(delay=0, coef=np.float32(np.nan), corr=r)
    best = None
    for d in lag_order(D):
        if best is None or r[d + D] > r[best + D]:
            best = d
    with np.errstate(invalid='ignore', divide='ignore'):
        coef = np.float32(np.float64(r[best + D]) / np.sqrt(np.float64(sum_sq(x)) * np.float64(sum_sq(y))))
    return dict(delay=best, coef=coef, corr=r)


def gap(r, D):
    """relative gap between the two largest values of r (1.0 when there is one lag)"""
    v = np.sort(r)[::-1]
    return 1.0 if len(v) < 2 else float((v[0] - v[1]) / abs(v[0])) if v[0] != 0 else 0.0


def overlap(Lx, Ly, d):
    x0, y0 = max(0, -d), max(0, d)
    return x0, y0, min(Lx - x0, Ly - y0)


def sums(x, y, d):
    """(n, sum x, sum y, sum x^2, sum y^2, sum x y) over the overlap the delay leaves, float64; all 0 when there is none"""
    x, y = np.asarray(x), np.asarray(y)
    x0, y0, n = overlap(len(x), len(y), d)
    if n <= 0:
        return np.zeros(6)
    u, v = x[x0:x0 + n], y[y0:y0 + n]
    if is_pcm(x) and is_pcm(y):
        a, b = _ints(u), _ints(v)
        return np.array([n, float(a.sum()) * 2.0 ** -15, float(b.sum()) * 2.0 ** -15, float(np.dot(a, a)) * 2.0 ** -30, float(np.dot(b, b)) * 2.0 ** -30,
                         float(np.dot(a, b)) * 2.0 ** -30])
    a, b = u.astype(np.longdouble), v.astype(np.longdouble)
    return np.array([n, a.sum(), b.sum(), np.dot(a, a), np.dot(b, b), np.dot(a, b)]).astype(np.float64)


def scores(s, zero_mean):
    """(SI-SDR dB, SNR dB, gain dB) in float64 from the six sums, every operation on its own; NaN thrice when n <= 0"""
    n, sx, sy, sxx, syy, sxy = (np.float64(v) for v in s)
    if n <= 0:
        return np.full(3, np.nan)
    with np.errstate(invalid='ignore', divide='ignore'):
        cxx, cyy, cxy = sxx, syy, sxy
        if zero_mean:
            cxx, cyy, cxy = sxx - (sx * sx) / n, syy - (sy * sy) / n, sxy - (sx * sy) / n
        t = cxy * cxy
        si = 10.0 * np.log10(t / (cxx * cyy - t))
        snr = 10.0 * np.log10(cxx / ((cxx - 2.0 * cxy) + cyy))
        g = 20.0 * np.log10(np.abs(cxy / cxx))
    return np.array([si, snr, g])


def sums_bound(x, y, d):
    """first-order bounds of the five float64 sums over the overlap for non-PCM input: n 2^-53 sum |term|"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0, n = overlap(len(x), len(y), d)
    u, v = np.abs(x[x0:x0 + n]), np.abs(y[y0:y0 + n])
    return n * 2.0 ** -53 * np.array([u.sum(), v.sum(), np.dot(u, u), np.dot(v, v), np.dot(u, v)])
