"""numpy oracle of the DTW kernel (st_dtw_batch): the recurrence and the tie rule of include/semitts.h restated in float64 or float32,
one anti-diagonal of the grid per numpy step.

    d(i, j) = scale * sqrt(sum_k (x[i, k] - y[j, k])^2)                      (the sum over ascending k)
    D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)),   D(0, 0) = d(0, 0)
    ties: the diagonal, then (i-1, j), then (i, j-1) -- a candidate replaces the best only when strictly smaller

In float32 every operation is rounded as the kernel rounds it except the sum of squares, which the kernel may contract to fma; on the
integer-valued inputs of the exact tests every intermediate is exact either way.
"""
import numpy as np


def distances(x, y, scale=1.0, dtype=np.float64):
    """(n, m) matrix of d(i, j), every operation in `dtype`"""
    x, y = np.asarray(x, dtype).reshape(len(x), -1), np.asarray(y, dtype).reshape(len(y), -1)
    s = np.zeros((len(x), len(y)), dtype)
    for k in range(x.shape[1]):
        t = x[:, None, k] - y[None, :, k]
        s += t * t
    return (dtype(scale) * np.sqrt(s)).astype(dtype)


def accumulate(d):
    """the accumulated cost D and the back-pointer codes (0: diagonal, 1: (i-1, j), 2: (i, j-1)) of a distance matrix, in d's dtype"""
    n, m = d.shape
    inf = d.dtype.type(np.inf)
    D = np.full((n, m), inf, d.dtype)
    code = np.zeros((n, m), np.uint8)
    D[0, 0] = d[0, 0]
    for c in range(1, n + m - 1):
        i = np.arange(max(0, c - (m - 1)), min(n - 1, c) + 1)
        j = c - i
        diag = np.where((i > 0) & (j > 0), D[i - 1, j - 1], inf)        # (an index of -1 wraps; np.where drops what it reads)
        up = np.where(i > 0, D[i - 1, j], inf)
        left = np.where(j > 0, D[i, j - 1], inf)
        best, cd = diag.copy(), np.zeros(len(i), np.uint8)
        take = up < best
        best[take], cd[take] = up[take], 1
        take = left < best
        best[take], cd[take] = left[take], 2
        D[i, j] = best + d[i, j]
        code[i, j] = cd
    return D, code


def dtw(x, y, scale=1.0, dtype=np.float64):
    """-> (total, path): D(n-1, m-1) as a `dtype` scalar and the (P, 2) int32 cells of the traced path from (0, 0) to (n-1, m-1).
    An empty side or a NaN in either: (nan, an empty path)."""
    n, m = len(x), len(y)
    if n == 0 or m == 0 or np.isnan(np.asarray(x, np.float64)).any() or np.isnan(np.asarray(y, np.float64)).any():
        return dtype(np.nan), np.zeros((0, 2), np.int32)
    D, code = accumulate(distances(x, y, scale, dtype))
    i, j, cells = n - 1, m - 1, []
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        c = code[i, j]
        i, j = i - (c != 2), j - (c != 1)
    return D[n - 1, m - 1], np.array(cells[::-1], np.int32).reshape(-1, 2)


def path_cost(x, y, path, scale=1.0):
    """the float64 cost of a path: the sum of d over its cells"""
    x, y = np.asarray(x, np.float64).reshape(len(x), -1), np.asarray(y, np.float64).reshape(len(y), -1)
    path = np.asarray(path).reshape(-1, 2)
    return float((scale * np.sqrt(((x[path[:, 0]] - y[path[:, 1]]) ** 2).sum(-1))).sum())


def is_path(path, n, m):
    """a warping path of an n x m grid: from (0, 0) to (n-1, m-1) by steps (1, 1), (1, 0) or (0, 1)"""
    path = np.asarray(path).reshape(-1, 2)
    if len(path) == 0 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (n - 1, m - 1):
        return False
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    return steps <= {(1, 1), (1, 0), (0, 1)}


def eps(n, m, D):
    """relative distance of the fp32 optimum from the float64 one, from both sides: each d carries at most (D + 3) / 2 + 2 roundings
    (the difference, the square, D additions, the halving by the root, the scale), a path sums at most n + m - 1 of them by sequential
    additions, min is exact"""
    return (n + m - 1 + D + 4) * 2.0 ** -24


def brute_force(x, y, scale=1.0):
    """the float64 cost of every monotone path of a small grid -> sorted list of (cost, path as a tuple of cells)"""
    n, m = len(x), len(y)
    d = distances(x, y, scale, np.float64)
    out = []

    def walk(i, j, cost, cells):
        cost, cells = cost + d[i, j], cells + ((i, j),)
        if i == n - 1 and j == m - 1:
            out.append((cost, cells))
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, cost, cells)
        if i + 1 < n:
            walk(i + 1, j, cost, cells)
        if j + 1 < m:
            walk(i, j + 1, cost, cells)
    walk(0, 0, 0.0, ())
    return sorted(out)


def integer_pair(rs, n, m, D):
    """float32 inputs on which every distance is an integer: D = 1, integers in [-8, 8]; D = 3, integer multiples (in [-8, 8]) of
    (1, 2, 2) or (2, 3, 6), so the distance is 3 or 7 times an integer"""
    a, b = rs.randint(-8, 9, n).astype(np.float32), rs.randint(-8, 9, m).astype(np.float32)
    if D == 1:
        return a[:, None].copy(), b[:, None].copy()
    assert D == 3
    pat = np.array([(1, 2, 2), (2, 3, 6)][rs.randint(2)], np.float32)
    return a[:, None] * pat, b[:, None] * pat
