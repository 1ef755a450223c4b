"""numpy oracle of the end-of-speech kernel (st_attn_endpoint): the definitions of include/semitts.h restated in float64, step by step,
without any of the kernel's structure (no lanes, no scan, no atomics), and a generator of constructed alignments."""
import collections

import numpy as np

Result = collections.namedtuple('Result', 'end reached n_back n_skip covered nonfinite focus peak dur')


def row_peak(row):
    """(peak, maxw) of one row: the lowest column among the maxima; a NaN never wins; (0, 0.0) when every entry is NaN"""
    row = np.asarray(row, np.float64)
    valid = ~np.isnan(row)
    if not valid.any():
        return 0, 0.0
    top = row[valid].max()
    return int(np.flatnonzero(row == top)[0]), float(top)


def endpoint(align, n, patience=3, max_jump=4):
    """one utterance: align (S, L), n real phones -> Result (focus a float64, peak (S,), dur (L,))"""
    align = np.asarray(align, np.float64)
    S, L = align.shape
    assert 1 <= n <= L and patience >= 1 and max_jump >= 1 and S >= 1
    pk = [row_peak(align[t]) for t in range(S)]
    peak = np.array([p for p, _ in pk], np.int32)
    maxw = np.array([w for _, w in pk], np.float64)
    flag = [int(p) >= n - 1 for p in peak]
    end, reached = S, 0
    for t0 in range(0, S - patience + 1):
        if all(flag[t0:t0 + patience]):
            end, reached = t0 + patience, 1
            break
    with np.errstate(invalid='ignore'):
        focus = float(np.sum(maxw[:end]) / end)
    n_back = sum(1 for t in range(1, end) if peak[t] < peak[t - 1])
    n_skip = sum(1 for t in range(1, end) if int(peak[t]) > int(peak[t - 1]) + max_jump)
    dur = np.zeros(L, np.int32)
    for t in range(end):
        dur[peak[t]] += 1
    covered = int(sum(1 for j in range(n) if dur[j] > 0))
    nonfinite = int(not np.isfinite(align).all())
    return Result(end, reached, n_back, n_skip, covered, nonfinite, focus, peak, dur)


def endpoint_batch(align, enc_len, patience=3, max_jump=4):
    """(B, S, L), (B,) -> Result of stacked arrays"""
    rs = [endpoint(a, int(n), patience, max_jump) for a, n in zip(align, enc_len)]
    return Result(*(np.array([getattr(r, k) for r in rs]) for k in Result._fields))


def staircase(durs, S, L, rs=None, peak_w=0.75, tail=None):
    """A monotone alignment (S, L) float32: the peak sits durs[j] steps on phone j = 0, 1, ... in turn and on column `tail` (default:
    the last phone, len(durs) - 1) for the steps left.  The peak weighs peak_w, the rest of the row is spread evenly (with rs: unevenly,
    every other entry still below the peak), so each row sums to about 1 and has one maximum.  -> (align, peaks (S,))"""
    n = len(durs)
    assert n <= L
    cols = [j for j, d in enumerate(durs) for _ in range(d)][:S]
    cols += [n - 1 if tail is None else tail] * (S - len(cols))
    return from_peaks(cols, L, rs, peak_w), np.array(cols, np.int32)


def from_peaks(cols, L, rs=None, peak_w=0.75):
    """(S, L) float32 whose row t has its single maximum peak_w at cols[t]"""
    S = len(cols)
    a = np.zeros((S, L), np.float32)
    for t, c in enumerate(cols):
        if L > 1:
            rest = np.full(L, (1.0 - peak_w) / (L - 1)) if rs is None else rs.dirichlet(np.ones(L)) * (1.0 - peak_w)
            a[t] = np.minimum(rest, 0.5 * peak_w).astype(np.float32)
        a[t, c] = peak_w
    return a


def random_peaks(rs, S, L, n):
    """a peak column per step: a walk that mostly stays or advances by one, sometimes skips ahead, falls back or visits the columns
    at and past the last phone n - 1 -- so runs of flagged steps of many lengths occur, broken and unbroken"""
    cols, c = [], 0
    for u in rs.rand(S).tolist():
        if u < 0.45:
            pass
        elif u < 0.75:
            c += 1
        elif u < 0.80:
            c += int(rs.randint(2, 9))
        elif u < 0.86:
            c -= int(rs.randint(1, 6))
        elif u < 0.94:
            c = n - 1 + int(rs.randint(0, max(1, L - n + 1)))
        else:
            c = int(rs.randint(0, L))
        c = min(max(c, 0), L - 1)
        cols.append(c)
    return cols


def with_tie(align, t, c_other):
    """row t gets a second entry equal to its maximum at column c_other"""
    a = np.array(align, np.float32)
    a[t, c_other] = a[t].max()
    return a
