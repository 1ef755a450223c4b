"""Dense phone n-gram tables for the LM-fused CTC beam search (st_ctc_beam_search_lm): counting, smoothing, the file format and the
fused bonus table.  Host side, numpy only.

    from semi_tts_amd import ngram
    table = ngram.ngram_table(ngram.count_ngrams(transcripts, V=43, order=2))      # (V^(order-1), V) float32 probabilities
    ngram.save_table('phn.2gram.npy', table)
    bonus = ngram.fusion_table(table, weight=0.5, ins_bonus=0.0)                    # what the kernel adds per extension

The layout is the reference's NgramPrior (src/lm.py:233-290): a plain `.npy` of shape (V^(n-1), V); the row of the context
(c_0, ..., c_{n-2}), oldest symbol first, is sum_i c_i V^(n-2-i); a sequence starts in the context (0, ..., 0, bos) -- zeros, then the
start id, 1 there and by default here.  A table written for the reference loads here and the reverse.
"""
import math
import os

import numpy as np

MAX_ORDER, MAX_TABLE = 4, 1 << 26             # st_ctc_beam_search_lm's limits
EPS = 1e-10                                   # src/lm.py: EPS, added to the probabilities before the logarithm


def context_row(ctx, V):
    """the table row of a context (the last n-1 ids, oldest first): sum_i ctx[i] V^(n-2-i); 0 for the empty context of a unigram"""
    row = 0
    for c in ctx:
        row = row * V + int(c)
    return row


def _check_shape(V, order):
    V, order = int(V), int(order)
    if V < 2 or not 1 <= order <= MAX_ORDER or V ** order > MAX_TABLE:
        raise ValueError('ngram: V = %d, order = %d outside V >= 2, 1 <= order <= %d, V^order <= 2^26' % (V, order, MAX_ORDER))
    return V, order


def order_of(rows, V):
    """the order n of a (V^(n-1), V) table with `rows` rows; None when rows is no power of V within 1 .. MAX_ORDER"""
    for n in range(1, MAX_ORDER + 1):
        if rows == V ** (n - 1):
            return n
    return None


def table_order(shape):
    """the order n of a table of shape (V^(n-1), V); ValueError when the shape is none"""
    n = order_of(shape[0], shape[1]) if len(shape) == 2 and shape[1] >= 2 else None
    if n is not None:
        return n
    raise ValueError('ngram: shape %s is no (V^(order-1), V) table with V >= 2, 1 <= order <= %d' % (tuple(shape), MAX_ORDER))


def count_ngrams(transcripts, V, order, bos=1):
    """transcripts: sequences of ids in [0, V) -> (V^(order-1), V) int64 counts; every sequence starts in the context (0, ..., 0, bos)"""
    V, order = _check_shape(V, order)
    bos = int(bos)
    if not 0 <= bos < V:
        raise ValueError('ngram: bos %d outside [0, %d)' % (bos, V))
    rows = V ** (order - 1)
    counts = np.zeros((rows, V), np.int64)
    for k, seq in enumerate(transcripts):
        ctx = bos if order > 1 else 0
        for c in seq:
            c = int(c)
            if not 0 <= c < V:
                raise ValueError('ngram: id %d of transcript %d outside [0, %d)' % (c, k, V))
            counts[ctx, c] += 1
            ctx = (ctx * V + c) % rows
    return counts


def ngram_table(counts, smooth=1.0, blank=0):
    """counts (V^(order-1), V) -> float32 probabilities: add-`smooth` over the non-blank columns, the blank column 0, every row summing
    to 1; a context never seen (with smooth == 0 too) is uniform over the non-blank columns"""
    counts = np.asarray(counts)
    table_order(counts.shape)
    V, blank, smooth = counts.shape[1], int(blank), float(smooth)
    if not 0 <= blank < V:
        raise ValueError('ngram: blank %d outside [0, %d)' % (blank, V))
    if not (math.isfinite(smooth) and smooth >= 0.0) or (counts < 0).any():
        raise ValueError('ngram: counts and smooth must be >= 0 (smooth %r)' % (smooth,))
    c = counts.astype(np.float64) + smooth
    c[:, blank] = 0.0
    tot = c.sum(1, keepdims=True)
    uniform = np.full(V, 1.0 / (V - 1))
    uniform[blank] = 0.0
    p = np.where(tot > 0.0, c / np.where(tot > 0.0, tot, 1.0), uniform[None, :])
    return p.astype(np.float32)


def save_table(path, table):
    """write a (V^(order-1), V) table as a plain float32 .npy (NgramPrior's np.load(path)), exactly at `path`"""
    table = np.ascontiguousarray(table, dtype=np.float32)
    table_order(table.shape)
    with open(path, 'wb') as f:
        np.save(f, table, allow_pickle=False)


def load_table(path):
    """-> the (V^(order-1), V) float32 table of a .npy file; ValueError naming the file when it holds none"""
    try:
        table = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise ValueError('%s: cannot read the n-gram table (%s)' % (path, e))
    if not isinstance(table, np.ndarray) or table.dtype.kind not in 'fiu':
        raise ValueError('%s: not a numeric array' % (path,))
    if table.ndim == 1:
        table = table[None, :]                 # NgramPrior stores a unigram as a vector
    try:
        table_order(table.shape)
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))
    return np.ascontiguousarray(table, dtype=np.float32)


def fusion_table(table, weight, ins_bonus, eps=EPS):
    """the bonus the fused search adds for an extension: float32(weight * log(float64(table) + eps) + ins_bonus), computed in float64 and
    cast once.  table: probabilities (V^(order-1), V); NaN, negative or infinite entries and a non-finite weight / ins_bonus / eps are
    refused."""
    table = np.asarray(table)
    table_order(table.shape)
    weight, ins_bonus, eps = float(weight), float(ins_bonus), float(eps)
    if not (math.isfinite(weight) and math.isfinite(ins_bonus)):
        raise ValueError('ngram: weight and ins_bonus must be finite (got %r, %r)' % (weight, ins_bonus))
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError('ngram: eps must be finite and >= 0 (got %r)' % (eps,))
    t = table.astype(np.float64)
    if not np.isfinite(t).all() or (t < 0.0).any():
        raise ValueError('ngram: the table must hold finite probabilities >= 0 (NaN, negative or infinite entries found)')
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.log(t + eps)
        out = np.where(np.isneginf(lg), -np.inf if weight > 0 else (0.0 if weight == 0 else np.inf), weight * lg) + ins_bonus
        out = np.ascontiguousarray(out.astype(np.float32))
    if np.isposinf(out).any() or np.isnan(out).any():              # (-inf is legal: a forbidden transition)
        raise ValueError('ngram: weight %r, ins_bonus %r give +inf or NaN bonuses (a zero probability with eps = 0 needs weight >= 0)'
                         % (weight, ins_bonus))
    return out


def build_lm_from_phn_dir(phn_dir, out, order, V=43, smooth=1.0, vocab=None, bos=1):
    """main.py --build-lm-phn-dir: every .phn of phn_dir (sorted by name; ctc_align.read_phn: the first line's tokens, ids or symbols
    of `vocab`) with id 0 -- the blank -- skipped -> counts of `order` over V classes (43: <pad>, <space>, <eos> and 40 phones) -> add-
    `smooth` probabilities written to `out` (save_table).  Nothing is written when a transcript is unreadable or holds an id >= V.
    -> dict(files, tokens, seen_contexts, contexts, order, V, table, summary: the one line main.py prints)"""
    from .ctc_align import read_phn
    V, order = _check_shape(V, order)
    files = sorted(f for f in os.listdir(phn_dir) if f.lower().endswith('.phn'))
    if not files:
        raise ValueError('--build-lm-phn-dir %s: no .phn files' % (phn_dir,))
    transcripts = []
    for f in files:
        ids = [i for i in read_phn(os.path.join(phn_dir, f), vocab) if i != 0]
        if any(i >= V for i in ids):
            raise ValueError('%s: id %d outside the %d classes of the table (--lm-classes; unit transcripts of K centroids need 3 + K)'
                             % (os.path.join(phn_dir, f), max(ids), V))
        transcripts.append(ids)
    counts = count_ngrams(transcripts, V, order, bos)
    table = ngram_table(counts, smooth, 0)
    save_table(out, table)
    res = dict(files=len(files), tokens=int(counts.sum()), seen_contexts=int((counts.sum(1) > 0).sum()), contexts=counts.shape[0],
               order=order, V=V, table=table)
    res['summary'] = ('[INFO] %d-gram table over %d classes from %d .phn files (%d tokens, %d of %d contexts seen, add-%g) -> %s'
                      % (order, V, res['files'], res['tokens'], res['seen_contexts'], res['contexts'], smooth, out))
    return res
