"""numpy oracle of the CTC forced aligner (st_ctc_forced_align): the Viterbi recurrence of include/semitts.h restated in float64 or
float32, a brute force over every label sequence, and the helpers the tests share.

The recurrence, over the states ext = [blank, y0, blank, y1, ..., blank] (n = 2 S + 1):
    a_0[0] = lp[0][blank], a_0[1] = lp[0][y0], the rest -inf
    a_t[s] = best + lp[t][ext[s]],  best = max(a[s], a[s-1], and a[s-2] when ext[s] != blank and ext[s] != ext[s-2])
Ties: the stay wins, then s-1, then s-2 (a candidate replaces the best only when strictly greater).  End: the larger of a[n-1] and
a[n-2], n-1 on a tie.  Every sum is ONE addition in `dtype`, so the float32 form is what an fp32 device computes bit for bit.
"""
import itertools

import numpy as np

EPS = 1e-10


def log_probs(prob, log_input=False, eps=EPS):
    """float64 log-probabilities of fp32 posteriors (log_input: they already are)"""
    p = np.asarray(prob, np.float64)
    return p if log_input else np.log(p + eps)


def targets_of(text, text_length=None, blank=0):
    """the targets of one row of `text`: its first text_length entries (all of them when None) that are not blank, in order"""
    row = list(np.asarray(text).tolist())
    if text_length is not None:
        row = row[:max(0, min(int(text_length), len(row)))]
    return [int(x) for x in row if int(x) != blank]


def n_repeats(targets):
    return sum(1 for a, b in zip(targets[:-1], targets[1:]) if a == b)


def _empty(T, S, score):
    return score, np.full(T, -1, np.int64), np.full(T, -1, np.int64), np.full(S, -1, np.int64), np.full(S, -1, np.int64)


def align(lp, targets, blank=0, dtype=np.float64):
    """lp (T, V) log-probabilities of the valid frames, targets: the non-blank target ids.
    -> (score, states (T,), labels (T,), tok_start (S,), tok_end (S,)); states / labels / spans all -1 when the score is NaN (a target
    outside [0, V), or a NaN in a column of ext) or -inf by infeasibility (T < S + adjacent equal targets).  Order of the refusals:
    the target range, then feasibility, then NaN."""
    lp = np.asarray(lp, dtype)
    T, V = lp.shape
    targets = [int(x) for x in targets]
    S = len(targets)
    if any(not 0 <= y < V for y in targets):
        return _empty(T, S, dtype(np.nan))
    if T < S + n_repeats(targets):
        return _empty(T, S, dtype(-np.inf))
    n = 2 * S + 1
    ext = np.full(n, blank, np.int64)
    ext[1::2] = targets
    if np.isnan(lp[:, ext]).any():
        return _empty(T, S, dtype(np.nan))
    if T == 0:
        return _empty(0, 0, dtype(0.0))
    skip = np.zeros(n, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = dtype(-np.inf)
    a = np.full(n, ninf, dtype)
    a[0] = lp[0, blank]
    if n > 1:
        a[1] = lp[0, ext[1]]
    bp = np.zeros((T, n), np.int8)
    for t in range(1, T):
        a1 = np.concatenate([[ninf], a[:-1]]).astype(dtype)
        a2 = np.concatenate([[ninf, ninf], a[:-2]]).astype(dtype)[:n]
        a2 = np.where(skip, a2, ninf)
        best, b = a.copy(), np.zeros(n, np.int8)
        m = a1 > best
        best[m], b[m] = a1[m], 1
        m = a2 > best
        best[m], b[m] = a2[m], 2
        a = (best + lp[t, ext]).astype(dtype)
        bp[t] = b
    s = n - 1
    if n > 1 and a[n - 2] > a[n - 1]:
        s = n - 2
    score = a[s]
    states = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    labels = ext[states]
    tok_start, tok_end = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
    for k in range(S):
        fr = np.nonzero(states == 2 * k + 1)[0]
        tok_start[k], tok_end[k] = fr[0], fr[-1] + 1
    return score, states, labels, tok_start, tok_end


def batch_align(prob, text, lengths=None, text_lengths=None, blank=0, log_input=False, eps=EPS, dtype=np.float64, lp=None):
    """the kernel's outputs for a batch: (score (B,), path (B, T), tok_start (B, L), tok_end (B, L)).  `lp`: log-probabilities (B, T, V)
    to use instead of log_probs(prob) (the bit-exact tests pass the very fp32 array the device gets)."""
    if lp is None:
        lp = log_probs(prob, log_input, eps)
    B, T, _ = lp.shape
    text = np.asarray(text)
    L = text.shape[1]
    score = np.empty(B, dtype)
    path = np.full((B, T), -1, np.int64)
    ts, te = np.full((B, L), -1, np.int64), np.full((B, L), -1, np.int64)
    for b in range(B):
        n = T if lengths is None else max(0, min(int(lengths[b]), T))
        tg = targets_of(text[b], None if text_lengths is None else text_lengths[b], blank)
        sc, _, lab, s0, s1 = align(lp[b, :n], tg, blank, dtype)
        score[b] = sc
        path[b, :n] = lab
        ts[b, :len(tg)], te[b, :len(tg)] = s0, s1
    return score, path, ts, te


def collapse(path, blank=0):
    """the CTC collapse of a label path: runs merged, then blanks dropped"""
    out, prev = [], None
    for x in path:
        x = int(x)
        if x != prev and x != blank:
            out.append(x)
        prev = x
    return out


def is_alignment(path, targets, blank=0):
    return collapse(path, blank) == [int(x) for x in targets]


def path_score(lp, path):
    """the float64 log-probability of a label path"""
    lp = np.asarray(lp, np.float64)
    path = np.asarray(path, np.int64)
    return float(lp[np.arange(len(path)), path].sum()) if len(path) else 0.0


def brute_force(lp, targets, blank=0):
    """every label sequence of length T that collapses to `targets`, best first: [(path tuple, float64 score)]; [] when there is none"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    targets = [int(x) for x in targets]
    out = []
    for p in itertools.product(range(V), repeat=T):
        if collapse(p, blank) == targets:
            out.append((p, path_score(lp, p)))
    out.sort(key=lambda x: -x[1])
    return out


def forward_loglik(lp, targets, blank=0):
    """log p(targets | lp) by the float64 CTC forward algorithm (an upper bound of the best path's score)"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    n = 2 * len(targets) + 1
    ext = np.full(n, blank, np.int64)
    ext[1::2] = targets
    skip = np.zeros(n, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    if T == 0:
        return 0.0 if n == 1 else -np.inf
    a = np.full(n, -np.inf)
    a[:2] = lp[0, ext[:2]]
    for t in range(1, T):
        a1 = np.concatenate([[-np.inf], a[:-1]])
        a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]])[:n], -np.inf)
        a = np.logaddexp(np.logaddexp(a, a1), a2) + lp[t, ext]
    return float(np.logaddexp(a[-1], a[-2]) if n > 1 else a[-1])


def softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def peaked(rs, B, T, V, temp, max_targets, blank=0, counts=None):
    """CTC-like posteriors around known transcripts: per utterance 1 .. max_targets random non-blank targets, a random monotone
    placement of them over the T frames (blanks elsewhere, one forced between equal neighbours), peaks of height 6 on that placement
    plus Gaussian noise, at softmax temperature `temp`.  -> (prob (B, T, V) fp32, text (B, max_targets) int64 blank-padded,
    text_lengths (B,) int32).  counts: the number of targets per utterance instead of a random one."""
    text = np.full((B, max_targets), blank, np.int64)
    tl = np.zeros(B, np.int32)
    lab = np.full((B, T), blank, np.int64)
    nonblank = [v for v in range(V) if v != blank]
    for b in range(B):
        S = int(rs.randint(1, max_targets + 1)) if counts is None else int(counts[b])
        y = rs.choice(nonblank, S)
        while T < S + n_repeats(list(y[:S])):
            S -= 1
        y = y[:S]
        text[b, :S], tl[b] = y, S
        # state sequence: a random non-decreasing walk over ext that visits every odd state
        need = S + n_repeats(list(y))
        spare = T - need
        n = 2 * S + 1
        dur = np.zeros(n, np.int64)
        dur[1::2] = 1
        for k in range(1, S):
            if y[k] == y[k - 1]:
                dur[2 * k] = 1
        dur += rs.multinomial(spare, np.ones(n) / n)
        ext = np.full(n, blank, np.int64)
        ext[1::2] = y
        lab[b] = np.repeat(ext, dur)
    prob = softmax((rs.randn(B, T, V) + 6.0 * np.eye(V)[lab]) / temp)
    return prob, text, tl
