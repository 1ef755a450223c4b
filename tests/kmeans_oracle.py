"""numpy float64 oracle of the k-means ops (semi_tts_amd/csrc/kmeans.hip), written from the definitions in include/semitts.h: the nearest
centroid with the first minimum winning, the float64 mean of a cluster's members, the relocation of empty clusters to the farthest
points, k-means++ over a sequential running sum, and Lloyd's loop over them.  Inputs are float32 values held in float64 arrays."""
import numpy as np


def sqdist(x, c):
    """(N, K) float64 squared distances, the direct form sum_d (x - c)^2, formed in blocks of rows of at most 2^24 differences"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]), np.float64)
    rows = max(1, (1 << 24) // (c.shape[0] * c.shape[1]))
    for r0 in range(0, x.shape[0], rows):
        diff = x[r0:r0 + rows, None, :] - c[None, :, :]
        out[r0:r0 + rows] = np.einsum('nkd,nkd->nk', diff, diff)
    return out


def assign(x, c, d2=None):
    """-> (idx (N,) int32, the smallest k at the minimum, -1 for a row holding a NaN or an infinity; dist (N,) float64, NaN for such a row)"""
    x = np.asarray(x, np.float64)
    d2 = sqdist(x, c) if d2 is None else d2
    bad = ~np.isfinite(x).all(1)
    safe = np.where(bad[:, None], 0.0, d2)
    idx = safe.argmin(1).astype(np.int32)                   # (argmin returns the first minimum)
    dist = safe[np.arange(x.shape[0]), idx]
    idx[bad], dist[bad] = -1, np.nan
    return idx, dist


def tree_sum(v, nt):
    """the sum of v as a workgroup of nt threads forms it: thread t adds v[t], v[t + nt], .. in that order from 0, then a binary tree
    joins the threads (t with t + s, s = nt / 2 .. 1).  v (n,) or (m, n): one tree per row."""
    v = np.atleast_2d(np.asarray(v, np.float64))
    rows = -(-v.shape[1] // nt)
    pad = np.zeros((v.shape[0], rows * nt), np.float64)
    pad[:, :v.shape[1]] = v
    part = np.zeros((v.shape[0], nt), np.float64)
    for r in range(rows):
        part = part + pad[:, r * nt:(r + 1) * nt]
    s = nt // 2
    while s > 0:
        part[:, :s] = part[:, :s] + part[:, s:2 * s]
        s //= 2
    return part[:, 0] if part.shape[0] > 1 else part[0, 0]


def inertia_sum(dist, valid):
    """the sum of dist over the valid points in st_kmeans_update's order: chunks of 1024 points by 256 threads, the chunks by 1024"""
    d = np.where(valid, np.asarray(dist, np.float64), 0.0)
    nc = -(-len(d) // 1024)
    pad = np.zeros(nc * 1024, np.float64)
    pad[:len(d)] = d
    chunks = tree_sum(pad.reshape(nc, 1024), 256)
    return tree_sum(np.atleast_1d(chunks), 1024)


def shift_sum(cent_out, cent_in):
    """sum_k ||cent_out - cent_in||^2 in st_kmeans_update's order: a cluster's columns in ascending d, the clusters by 1024 threads"""
    sq = (np.asarray(cent_out, np.float32).astype(np.float64) - np.asarray(cent_in, np.float32).astype(np.float64)) ** 2
    per = np.zeros(sq.shape[0], np.float64)
    for d in range(sq.shape[1]):
        per = per + sq[:, d]
    return tree_sum(per, 1024)


def update(x, idx, dist, cent_in):
    """-> (cent_out (K, D) float32, count (K,) int32, stats (4,) float64, c64 (K, D): the float64 means before the rounding)"""
    x, cent_in = np.asarray(x, np.float64), np.asarray(cent_in, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist, np.float64)
    K = cent_in.shape[0]
    valid = (idx >= 0) & (idx < K)
    count = np.bincount(idx[valid], minlength=K).astype(np.int32)
    c64 = cent_in.astype(np.float64)
    for k in np.nonzero(count)[0]:
        c64[k] = x[valid & (idx == k)].sum(0) / float(count[k])
    cent_out = np.where(count[:, None] > 0, c64.astype(np.float32), cent_in)
    stats = np.array([inertia_sum(dist, valid), shift_sum(cent_out, cent_in), float((count == 0).sum()), float((~valid).sum())], np.float64)
    return cent_out, count, stats, c64


def relocate(x, idx, dist, count, cent):
    """the e-th empty cluster (ascending k) takes the row of the e-th valid point in the order (dist descending, index ascending)
    -> (cent (K, D) float32, the points taken)"""
    x, cent = np.asarray(x), np.array(cent, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist, np.float64)
    K = cent.shape[0]
    pts = np.nonzero((idx >= 0) & (idx < K) & ~np.isnan(dist))[0]
    order = pts[np.lexsort((pts, -dist[pts]))]
    empties = np.nonzero(np.asarray(count) == 0)[0]
    taken = order[:len(empties)]
    for e, n in enumerate(taken):
        cent[empties[e]] = x[n]
    return cent, taken


def pp_init(x, K, u):
    """k-means++: -> (picks (K,) int64, mind (N,) float64 after the last pick); ValueError when the weights run out before K picks"""
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    N = x.shape[0]
    picks = [min(int(np.floor(u[0] * N)), N - 1)]
    mind = np.full(N, np.inf)
    for j in range(1, K + 1):
        diff = x - x[picks[-1]]
        mind = np.fmin(mind, (diff * diff).sum(1))
        mind[np.isnan(x).any(1)] = np.nan
        if j == K:
            break
        w = np.where(mind > 0, mind, 0.0)
        cum = np.cumsum(w)                                  # (sequential, ascending n)
        total = cum[-1]
        if not total > 0:
            raise ValueError('fewer than K distinct rows')
        hit = np.nonzero((cum > u[j] * total) & (w > 0))[0]
        picks.append(int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1]))
    return np.array(picks, np.int64), mind


def column_variance(x):
    x = np.asarray(x, np.float64)
    return float(x.var(0).mean())


def lloyd(x, cent, iters=100, tol=1e-4):
    """-> (cent (K, D) float32, idx, dist of the final assignment, history [(iter, inertia, shift, empty)], converged)"""
    x = np.asarray(x, np.float64)
    cent = np.asarray(cent, np.float32)
    limit, history, converged = tol * column_variance(x), [], False
    for it in range(iters):
        idx, dist = assign(x, cent)
        out, count, stats, _ = update(x, idx, dist, cent)
        if stats[2] > 0:
            out, _ = relocate(x, idx, dist, count, out)
        history.append((it, stats[0], stats[1], int(stats[2])))
        cent = out
        if stats[2] == 0 and stats[1] <= limit:
            converged = True
            break
    idx, dist = assign(x, cent)
    return cent, idx, dist, history, converged
