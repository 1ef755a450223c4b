"""Silence trimming by frame energy in float64 numpy: the definition st_trim_silence implements (include/semitts.h), which is that of
librosa.effects.trim / split with ref = max, center = True and zero padding, restated so that nobody needs librosa.

    utterance x of L samples, T = 1 + L // hop frames; frame t reads x[t hop - frame_length // 2 + j], j < frame_length, 0 outside [0, L)
    energy[t] = sum_j x^2 / frame_length
    e_t = max(energy[t], float32(1e-10)), ref = max_t e_t; frame t is non-silent iff e_t > ref * ratio, ratio = float32(10^(-top_db / 10))
    bounds = (max(0, f0 hop - pad), min(L, (f1 + 1) hop + pad), non-silent frames, 0), f0 / f1 the first / last non-silent frame
    intervals: the maximal runs [fa, fb] of non-silent frames as (fa hop, min(L, (fb + 1) hop)), no pad
    any non-finite energy: bounds (0, L, -1, 1), no intervals
"""
import numpy as np

FLOOR = float(np.float32(1e-10))
CHUNK = 256          # frames formed at a time (an (8192, 1) framing would otherwise hold T x 8192 doubles)


def ratio_of(top_db):
    """10^(-top_db / 10) in double, rounded once to float32 (what the host hands the kernel)"""
    return float(np.float32(10.0 ** (-float(top_db) / 10.0)))


def frame_energy(x, frame_length, hop, dtype=np.float64):
    """(T,) frame energies of one utterance in `dtype` (float64: the oracle; float32: the numpy form the benchmark times)"""
    x = np.asarray(x, dtype).reshape(-1)
    L = x.shape[0]
    T = 1 + L // hop
    half = frame_length // 2
    xp = np.zeros(half + max(L, (T - 1) * hop + frame_length), dtype)
    xp[half:half + L] = x
    out = np.empty(T, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        sq = xp * xp
        win = np.lib.stride_tricks.sliding_window_view(sq, frame_length)[::hop]
        for t0 in range(0, T, CHUNK):
            out[t0:t0 + CHUNK] = win[t0:min(T, t0 + CHUNK)].sum(axis=1) / dtype(frame_length)
    return out


def runs(mask):
    """maximal runs of True in a 1-D mask -> [(first, last)]"""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def trim(x, frame_length, hop, top_db, pad=0, max_iv=0, ratio=None):
    """-> dict(energy (T,) float64, bounds [start, end, n_nonsilent, flags], n_iv, intervals (max_iv, 2) with -1 past the runs,
    all_intervals (n_iv, 2))"""
    x = np.asarray(x, np.float64).reshape(-1)
    L = x.shape[0]
    energy = frame_energy(x, frame_length, hop)
    if not np.isfinite(energy).all():
        return dict(energy=energy, bounds=[0, L, -1, 1], n_iv=0, intervals=np.full((max_iv, 2), -1, np.int64),
                    all_intervals=np.zeros((0, 2), np.int64))
    ratio = ratio_of(top_db) if ratio is None else float(ratio)
    e = np.maximum(energy, FLOOR)
    loud = e > e.max() * ratio
    idx = np.flatnonzero(loud)
    f0, f1 = int(idx[0]), int(idx[-1])
    bounds = [max(0, f0 * hop - pad), min(L, (f1 + 1) * hop + pad), int(loud.sum()), 0]
    iv = np.array([(a * hop, min(L, (b + 1) * hop)) for a, b in runs(loud)], np.int64).reshape(-1, 2)
    out = np.full((max_iv, 2), -1, np.int64)
    out[:min(max_iv, len(iv))] = iv[:max_iv]
    return dict(energy=energy, bounds=bounds, n_iv=len(iv), intervals=out, all_intervals=iv)


def margin_db(x, frame_length, hop, top_db, ratio=None):
    """the smallest |10 log10(e_t / (ref ratio))| over the utterance's frames: how far, in dB, the closest frame is from flipping"""
    e = np.maximum(frame_energy(x, frame_length, hop), FLOOR)
    ratio = ratio_of(top_db) if ratio is None else float(ratio)
    with np.errstate(divide='ignore'):
        return float(np.abs(10.0 * np.log10(e / (e.max() * ratio))).min())
