"""k-means over frame features on the GPU: the discrete units of ZeroSpeech / HuBERT-style baselines, from features alone -- no
transcripts, no trained codebook.  Lloyd's algorithm over the kernels of semi_tts_amd/csrc/kmeans.hip: an iteration is one assign
launch (st_kmeans_assign), the update launches (st_kmeans_update) and one host read of the four statistics; empty clusters are moved to
the points farthest from their centroids (st_kmeans_relocate, launched only when the statistics count one); the seeding is k-means++
without a host read between the picks (st_kmeans_pp_step / st_kmeans_pp_pick), or K distinct rows.

    from semi_tts_amd.kmeans import fit, quantise
    km = fit(feat, 50)                               # feat (rows, D) float32 on the GPU, e.g. AbxScorer.features()[0]
    idx, dist = quantise(other, km.centroids)        # the unit of every row of another buffer

No centring or whitening, no mini-batches, no cosine distance."""
import collections

import numpy as np
import torch

from . import toolops

KMeansFit = collections.namedtuple('KMeansFit', 'centroids idx dist inertia n_iter converged history')
INITS = ('++', 'sample')


def quantise(x, centroids):
    """the nearest centroid of every row: x (N, D) float32 on one GPU, centroids (K, D) float32 -> (idx (N,) int32, the lowest k at the
    least squared distance, -1 for a row holding a NaN or an infinity; dist (N,) float32, that squared distance).  One launch (toolops.kmeans_assign)."""
    return toolops.kmeans_assign(x, centroids)


def column_variance(x):
    """the mean over the columns of x's per-column variance (over the rows without a NaN), the scale of sklearn's stopping rule: one
    assign against the zero row (dist = |x|^2) and ONE kmeans_update with K = 1, whose statistics are the sum of |x|^2 and |mean|^2"""
    zero = torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float32)
    idx, dist = toolops.kmeans_assign(x, zero)
    _, _, stats = toolops.kmeans_update(x, idx, dist, zero)
    s = stats.cpu().numpy()
    n = x.shape[0] - s[3]
    return max(float(s[0] / n - s[1]) / x.shape[1], 0.0) if n > 0 else 0.0


def _init(x, K, init, rng):
    if init == '++':
        return toolops.kmeans_pp_init(x, K, rng.random(K))[0]
    rows = rng.choice(x.shape[0], size=K, replace=False)
    return x.index_select(0, torch.from_numpy(np.sort(rows)).to(x.device)).contiguous()


def _lloyd(x, cent, iters, limit, on_step):
    history, converged, n_iter = [], False, 0
    for it in range(iters):
        idx, dist = toolops.kmeans_assign(x, cent)
        out, count, stats = toolops.kmeans_update(x, idx, dist, cent)
        inertia, shift, empty, _ = stats.cpu().numpy().tolist()                # (the iteration's one host read)
        if on_step is not None:
            on_step(it, cent, idx, out)
        if empty > 0:
            toolops.kmeans_relocate(x, idx, dist, count, out)
        history.append((it, inertia, shift, int(empty)))
        cent, n_iter = out, it + 1
        if empty == 0 and shift <= limit:
            converged = True
            break
    idx, dist = toolops.kmeans_assign(x, cent)
    inertia = float(torch.where(idx >= 0, dist, torch.zeros_like(dist)).double().sum().item())
    return KMeansFit(cent, idx, dist, inertia, n_iter, converged, history)


def fit_all(x, K, iters=100, tol=1e-4, init='++', seed=0, restarts=1, on_step=None):
    """the `restarts` fits of fit, from the seeds seed, seed + 1, .., in that order -> [KMeansFit]; fit returns the one of lowest inertia"""
    d = toolops._km_data('fit', x)
    if not toolops._is_int(K) or not 1 <= int(K) <= toolops.KM_MAX_K:
        raise ValueError('fit: K must be an integer in [1, %d] (got %r)' % (toolops.KM_MAX_K, K))
    if int(K) > d.N:
        raise ValueError('fit: K = %d clusters of N = %d rows' % (K, d.N))
    if init not in INITS:
        raise ValueError('fit: init %r is none of %s' % (init, list(INITS)))
    if not toolops._is_int(iters) or iters < 1 or not toolops._is_int(restarts) or restarts < 1 or not toolops._is_number(tol) or not tol >= 0:
        raise ValueError('fit: iters >= 1, restarts >= 1 and tol >= 0 (got %r, %r, %r)' % (iters, restarts, tol))
    limit = float(tol) * column_variance(x)
    return [_lloyd(x, _init(x, int(K), init, np.random.default_rng(int(seed) + r)), int(iters), limit, on_step) for r in range(int(restarts))]


def fit(x, K, iters=100, tol=1e-4, init='++', seed=0, restarts=1, on_step=None):
    """Lloyd's k-means of x (N, D) float32 on one GPU into K clusters -> KMeansFit(centroids (K, D) float32, idx (N,) int32, dist (N,)
    float32 -- quantise(x, centroids) --, inertia: the float64 sum of dist, n_iter, converged, history: [(iter, inertia, shift, empty)],
    inertia and empty clusters of the assignment the iteration started from, shift the squared move of the table).
    Stops when shift <= tol * (mean per-column variance of x), sklearn's rule, and no cluster is empty; or after `iters` iterations.
    init: '++' (k-means++, numbers drawn by numpy.random.default_rng(seed)) or 'sample' (K distinct rows drawn by it).  restarts: that
    many fits from the seeds seed, seed + 1, ..; the first one of lowest inertia is returned.  on_step(iter, cent_in, idx, cent_out) is
    called after every update, before an empty cluster is moved.  Fewer than K distinct rows (init '++') or than K rows raise ValueError."""
    return min(fit_all(x, K, iters, tol, init, seed, restarts, on_step), key=lambda r: r.inertia)
