"""numpy oracle of the ABX kernels (st_dtw_pairs, st_abx_count) and of metrics.abx: the three frame distances in float64 and in
float32, the DTW recurrence with the path length carried beside the cost and the tie rule of include/semitts.h, the cheapest path of a
given length, brute-force triple counts and the ZeroSpeech aggregation.

    euclid   d = sqrt(sum_k (x_k - y_k)^2)
    angular  d = (2 / pi) atan2(|u - v|, |u + v|), u = x / |x| (a zero row stays zero)
    kl       d = 1/2 sum_k (x_k - y_k) (log(x_k + 1e-10) - log(y_k + 1e-10))
    D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), L(i, j) = L(chosen) + 1, L(0, 0) = 1
    ties: the diagonal, then (i-1, j), then (i, j-1) -- a candidate replaces the best only when strictly smaller
"""
import numpy as np

import dtw_oracle

METRICS = ('euclid', 'angular', 'kl')

# Largest observed error, in ulps of the result, of the device's atan2f / logf / sqrtf against float64 over the arguments the kernel
# passes them (tools/mb/abx_ulp.hip on an MI355X, 4 M samples each: 2.5935, 2.1392 and 0.5000); eps() budgets twice that.
ULP_ATAN2F, ULP_LOGF, ULP_SQRTF = 2.5935, 2.1392, 0.5
U = 2.0 ** -24          # the unit roundoff of fp32: one correctly rounded operation; k ulps of a function are 2 k U


def distances(x, y, metric, dtype=np.float64):
    """(n, m) matrix of d(i, j), every operation in `dtype` and in the kernel's order"""
    if metric == 'euclid':
        return dtw_oracle.distances(x, y, 1.0, dtype)
    x, y = np.asarray(x, dtype).reshape(len(x), -1), np.asarray(y, dtype).reshape(len(y), -1)
    n, m, D = len(x), len(y), x.shape[1]
    if metric == 'angular':
        def unit(a):
            s = np.zeros(len(a), dtype)
            for k in range(D):
                s += a[:, k] * a[:, k]
            nrm = np.sqrt(s)
            with np.errstate(divide='ignore'):
                r = np.where(nrm > 0, dtype(1) / np.where(nrm > 0, nrm, dtype(1)), dtype(0)).astype(dtype)
            return (a * r[:, None]).astype(dtype)
        u, v = unit(x), unit(y)
        sm, sp = np.zeros((n, m), dtype), np.zeros((n, m), dtype)
        for k in range(D):
            dm, dp = u[:, None, k] - v[None, :, k], u[:, None, k] + v[None, :, k]
            sm += dm * dm
            sp += dp * dp
        return np.minimum(dtype(2.0 / np.pi) * np.arctan2(np.sqrt(sm), np.sqrt(sp)), dtype(1)).astype(dtype)
    assert metric == 'kl'
    tiny = dtype(1e-10)
    with np.errstate(invalid='ignore', divide='ignore'):
        lx, ly = np.log(x + tiny), np.log(y + tiny)
    s = np.zeros((n, m), dtype)
    for k in range(D):
        s += (x[:, None, k] - y[None, :, k]) * (lx[:, None, k] - ly[None, :, k])
    s = (dtype(0.5) * s).astype(dtype)
    if (x < 0).any() or (y < 0).any():
        s[:] = np.nan
    return s


def accumulate_len(d):
    """-> (D, L): the accumulated cost and the carried path length of every cell, in d's dtype / int64"""
    n, m = d.shape
    inf = d.dtype.type(np.inf)
    D = np.full((n + 1, m + 1), inf, d.dtype)         # cell (i, j) at [i + 1, j + 1]; row / column 0 stand for the absent predecessors
    L = np.zeros((n + 1, m + 1), np.int64)
    D[1, 1], L[1, 1] = d[0, 0], 1
    for c in range(1, n + m - 1):
        i = np.arange(max(0, c - (m - 1)), min(n - 1, c) + 1)
        j = c - i
        best, bl = D[i, j].copy(), L[i, j].copy()                       # the diagonal
        up, ul = D[i, j + 1], L[i, j + 1]
        take = up < best
        best[take], bl[take] = up[take], ul[take]
        left, ll = D[i + 1, j], L[i + 1, j]
        take = left < best
        best[take], bl[take] = left[take], ll[take]
        D[i + 1, j + 1] = best + d[i, j]
        L[i + 1, j + 1] = bl + 1
    return D[1:, 1:], L[1:, 1:]


def dtw_len(d):
    """-> (cost, path_len) of a distance matrix: D(n-1, m-1) in d's dtype and L(n-1, m-1); (nan, 0) with a NaN in d"""
    if np.isnan(d).any():
        return d.dtype.type(np.nan), 0
    D, L = accumulate_len(d)
    return D[-1, -1], int(L[-1, -1])


def pair(x, y, metric, dtype=np.float64):
    """-> (dist, cost, path_len) of two items"""
    c, L = dtw_len(distances(x, y, metric, dtype))
    return (dtype(np.nan) if L == 0 else dtype(c) / dtype(L)), c, L


def min_cost_with_len(d, L):
    """the float64 minimum of the cost over the monotone paths of EXACTLY L cells (inf when there is none): a DP over (i, j, length),
    vectorised over the length and the cells of an anti-diagonal"""
    d = np.asarray(d, np.float64)
    n, m = d.shape
    K = n + m                       # lengths 0 .. n + m - 1
    if not 1 <= L < K:
        return np.inf
    M = np.full((n + 1, m + 1, K), np.inf)
    M[1, 1, 1] = d[0, 0]
    for c in range(1, n + m - 1):
        i = np.arange(max(0, c - (m - 1)), min(n - 1, c) + 1)
        j = c - i
        best = np.minimum(np.minimum(M[i, j], M[i, j + 1]), M[i + 1, j])   # (cells, K): the cheapest predecessor per length
        M[i + 1, j + 1, 1:] = best[:, :-1] + d[i, j][:, None]
    return float(M[n, m, L])


def eps(n, m, D, metric):
    """A derived bound, in the manner of dtw_oracle.eps, for the device's fp32 cost c against the float64 optimum:
    |c - opt| <= eps opt + eps (n + m).  Rounding is monotone, so the fp32 DP is the minimum over the paths of their sequentially rounded
    sums; a path has at most n + m - 1 cells, summed with at most n + m - 2 additions (relative (n + m - 2) U).  A cell's distance has a
    relative error `rel` U and, where the formula cancels, an absolute one `abs_` U; eps = (abs_ + rel + n + m - 2) U covers both: the
    relative terms against eps opt, the absolute ones (at most n + m - 1 cells) against eps (n + m).
    euclid:  difference U, square U (2 U carried + U), D - 1 additions, halved by the root, the root itself:
             rel = (D + 2) / 2 + 2 ULP_SQRTF' with ULP' = twice the measured ulps, in U (k ulps = 2 k U).
    angular: the squared norm of a row carries D U, its root D / 2 U + the root's error, the reciprocal U, the product U:
             a = D / 2 + 2 + 2 ULP_SQRTF' relative error of every component of u, i.e. a U absolute in the unit vector.  |u - v| and |u + v|
             (p and q, p^2 + q^2 = 4) then carry 2 a U absolute and r = (D + 2) / 2 + 2 ULP_SQRTF' relative each, and
             |d phi| = |q dp - p dq| / 4 <= (2 a (p + q) + 2 r p q) U / 4 <= (sqrt 2 a + r) U  -- absolute in the half angle phi,
             abs_ = (2 / pi) (sqrt 2 a + r); atan2f and the scaling are relative: rel = 2 ULP_ATAN2F' + 2.
    kl:      log(fl(x + 1e-10)) carries U (the addition) + 2 ULP_LOGF' U |log| with |log| <= 23.03; a difference of two logs twice that,
             absolute, times |x_k - y_k|, which sum to at most 2 over a pair of probability rows (2.001 with their own rounding), times
             the 1/2: abs_ = 2.001 (1 + 2 ULP_LOGF' 23.03); the difference, the product and the D - 1 additions are relative:
             rel = D + 2."""
    assert metric in METRICS
    ks, ka, kl = 2.0 * ULP_SQRTF, 2.0 * ULP_ATAN2F, 2.0 * ULP_LOGF          # twice the measured maxima
    if metric == 'euclid':
        abs_, rel = 0.0, (D + 2) / 2.0 + 2.0 * ks
    elif metric == 'angular':
        a = D / 2.0 + 2.0 + 2.0 * ks
        r = (D + 2) / 2.0 + 2.0 * ks
        abs_, rel = (2.0 / np.pi) * (np.sqrt(2.0) * a + r), 2.0 * ka + 2.0
    else:
        abs_, rel = 2.001 * (1.0 + 2.0 * kl * 23.03), D + 2.0
    return (abs_ + rel + n + m - 2) * U


def triple_counts(dm, a, b):
    """brute force over a dense matrix: (wrong, tied, nan, triples) for X, A in the index list a (A != X by index), B in b"""
    dm = np.asarray(dm)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    wrong = tied = nan = 0
    for x in a:
        for A in a:
            if A == x:
                continue
            ax = dm[A, x]
            for B in b:
                bx = dm[B, x]
                if np.isnan(ax) or np.isnan(bx):
                    nan += 1
                elif ax > bx:
                    wrong += 1
                elif ax == bx:
                    tied += 1
    return wrong, tied, nan, len(a) * (len(a) - 1) * len(b)


def triple_counts_fast(dm, a, b):
    """triple_counts by numpy broadcasting (the same numbers; for blocks of 10^5 and more triples)"""
    dm = np.asarray(dm)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if len(a) == 0 or len(b) == 0:
        return 0, 0, 0, len(a) * (len(a) - 1) * len(b)
    AX, BX = dm[np.ix_(a, a)], dm[np.ix_(b, a)]                     # (A, X), (B, X)
    off = (a[:, None] != a[None, :])[:, None, :]                     # A != X
    ax, bx = AX[:, None, :], BX[None, :, :]
    isnan = (np.isnan(ax) | np.isnan(bx)) & off
    with np.errstate(invalid='ignore'):
        wrong = ((ax > bx) & off & ~isnan).sum()
        tied = ((ax == bx) & off & ~isnan).sum()
    return int(wrong), int(tied), int(isnan.sum()), len(a) * (len(a) - 1) * len(b)


def abx(dist, label, cell, items=None):
    """the whole measure by brute force.  dist(p, q): the distance of items p and q (called once per unordered pair, with p before q
    in the order below); label / cell per item; items: the item indices that take part (None: all), ordered by (cell, label, index).
    -> (blocks {(cell, a, b): (wrong, tied, nan, triples)}, table {(a, b): (cells, triples - nan summed, error)}, score)"""
    label, cell = np.asarray(label), np.asarray(cell)
    items = np.arange(len(label)) if items is None else np.asarray(items)
    items = np.array(sorted(items.tolist(), key=lambda q: (cell[q], label[q], q)), np.int64)
    blocks = {}
    for c in sorted(set(cell[items].tolist())):
        mem = items[cell[items] == c]
        labs = sorted(set(label[mem].tolist()))
        if len(labs) < 2:
            continue
        dm = np.zeros((len(mem), len(mem)))
        for i in range(len(mem)):
            for j in range(i + 1, len(mem)):
                dm[i, j] = dm[j, i] = dist(int(mem[i]), int(mem[j]))
        for a in labs:
            ia = np.nonzero(label[mem] == a)[0]
            if len(ia) < 2:
                continue
            for b in labs:
                if b != a:
                    blocks[(c, a, b)] = triple_counts_fast(dm, ia, np.nonzero(label[mem] == b)[0])
    return (blocks,) + aggregate(blocks)


def aggregate(blocks):
    """{(cell, a, b): counts} -> (table {(a, b): (cells, valid triples, error)}, score): block error (wrong + tied / 2) / (triples - nan),
    the mean over the cells of a pair, then the mean over the ordered pairs (float64)"""
    per = {}
    for (c, a, b), (wrong, tied, nan, triples) in blocks.items():
        if triples - nan > 0:
            per.setdefault((a, b), []).append(((wrong + 0.5 * tied) / float(triples - nan), triples - nan))
    table = {k: (len(v), sum(t for _, t in v), float(np.mean([e for e, _ in v]))) for k, v in per.items()}
    score = float(np.mean([v[2] for v in table.values()])) if table else float('nan')
    return table, score
