"""The model-free ops over the C ABI: scoring (edit distances, CTC beam search and forced alignment, DTW, ABX, attention end points) and
signal processing (vocoder, features, resampling, pitch, silence, loudness, STOI, delay, SI-SDR), each as thin as the bindings of
ops.py -- device tensors in, raw pointers to libsemitts_hip.so, device tensors out, no CPU fallback -- behind one set of argument
checks: whatever an entry point would refuse raises ValueError here, before the device is touched.

ops.py imports every name of this module, so ops.X stays valid; the modules of this package call it directly."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ngram import MAX_ORDER as CB_MAX_ORDER, MAX_TABLE as CB_MAX_TABLE, order_of as _ngram_order_of   # (st_ctc_beam_search_lm's limits)


# --------------------------------------------------------------------------------------------- the argument checks every op shares
def _got(t):
    """the '(got ...)' tail of a refusal: shape, dtype and device of a tensor, the type name of anything else"""
    return '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _lengths(what, name, v, shape, lo, hi, of, dev, symbol=None, optional=True):
    """a lengths argument of the op `what`: None (with optional: all of it), or integers of `shape` -- a host tensor / sequence is checked
    against [lo, hi] here, a device tensor is taken as it is (the kernel clamps it) -> int32 tensor on dev, the device of the tensor
    named `of`, or None.  symbol: how a (B,) shape is written ('(B,)' for a device tensor, B itself for a host one); None: the tuple."""
    if v is None and optional:
        return None
    if torch.is_tensor(v) and v.is_cuda:
        if v.device != dev or tuple(v.shape) != shape or v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError('%s: %s must be %s integers on the device of %s (got %s)' % (what, name, symbol or shape, of, _got(v)))
    else:
        host = np.asarray(v.cpu() if torch.is_tensor(v) else v)
        if host.shape != shape or host.dtype.kind not in 'iu' or (host < lo).any() or (host > hi).any():
            raise ValueError('%s: %s must be %s integers in [%d, %d] (got %s)' % (what, name, shape[0] if symbol else shape, lo, hi, host.tolist()))
    return torch.as_tensor(v).to(dev, torch.int32).contiguous()


_IGNORE_DEV = {}


def _ignore_dev(ignore, dev):
    """the tuple of ignored ids as an int32 tensor on dev ([0] for none: the kernels take a pointer), made once per device and tuple"""
    ign = _IGNORE_DEV.get((dev, ignore))
    if ign is None:
        ign = _IGNORE_DEV[(dev, ignore)] = torch.tensor(ignore if ignore else [0], dtype=torch.int32).to(dev)
    return ign


# --------------------------------------------------------------------------------------------- scoring
GED_MAX_T, GED_MAX_V, GED_MAX_L, GED_MAX_IGNORE = 4096, 10240, 1024, 64      # st_ctc_greedy_edit_distance's limits


def ctc_greedy_edit_distance(prob, text, ignore, want_hyp=False):
    """greedy CTC transcript of `prob` and its edit distance to `text`, per utterance (see st_ctc_greedy_edit_distance):
    prob (B, T, V) fp32 posteriors / log-posteriors, or (B, T) int64 ids already argmaxed (st_ids_edit_distance); text (B, L) int64;
    ignore: the ids dropped from both sides.  -> (dist, ref_len) int32 (B,) device tensors [+ (hyp (B, T) int64, hyp_len (B,) int32)
    with want_hyp].  One launch, no host read.  Anything the kernel would refuse raises ValueError before the launch."""
    if not (torch.is_tensor(prob) and torch.is_tensor(text)):
        raise ValueError('ctc_greedy_edit_distance: prob and text must be tensors')
    if not (prob.is_cuda and text.is_cuda and prob.device == text.device):
        raise ValueError('ctc_greedy_edit_distance: prob and text must be on one GPU (got %s, %s)' % (prob.device, text.device))
    ids = prob.dim() == 2
    if ids and prob.dtype != torch.int64 or not ids and (prob.dim() != 3 or prob.dtype != torch.float32):
        raise ValueError('ctc_greedy_edit_distance: prob must be (B, T, V) float32 or (B, T) int64 (got %s %s)'
                         % (tuple(prob.shape), prob.dtype))
    if text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('ctc_greedy_edit_distance: text must be (B, L) int64 (got %s %s)' % (tuple(text.shape), text.dtype))
    B, T = prob.shape[:2]
    V = 0 if ids else prob.shape[2]
    L = text.shape[1]
    ignore = tuple(int(i) for i in ignore)
    if text.shape[0] != B or B < 1:
        raise ValueError('ctc_greedy_edit_distance: %d utterances of prob, %d of text (at least one)' % (B, text.shape[0]))
    if not (1 <= T <= GED_MAX_T and (ids or 1 <= V <= GED_MAX_V) and 1 <= L <= GED_MAX_L and len(ignore) <= GED_MAX_IGNORE):
        raise ValueError('ctc_greedy_edit_distance: T=%d, V=%d, L=%d, %d ignored ids outside 1 <= T <= %d, 1 <= V <= %d, 1 <= L <= %d, '
                         '<= %d ignored ids' % (T, V, L, len(ignore), GED_MAX_T, GED_MAX_V, GED_MAX_L, GED_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('ctc_greedy_edit_distance: ignored ids must fit int32')
    dev = prob.device
    ign = _ignore_dev(ignore, dev)
    prob, text = prob.contiguous(), text.contiguous()
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    ref_len = torch.empty(B, device=dev, dtype=torch.int32)
    hyp = torch.empty(B, T, device=dev, dtype=torch.int64) if want_hyp else None
    hyp_len = torch.empty(B, device=dev, dtype=torch.int32) if want_hyp else None
    lib = _lib.load()
    if ids:
        check(lib.st_ids_edit_distance(_p(prob, torch.int64), B, T, _p(text, torch.int64), L, _p(ign, torch.int32), len(ignore),
                                       _p(dist, torch.int32), _p(ref_len, torch.int32), _p(hyp, torch.int64), _p(hyp_len, torch.int32),
                                       stream_handle()), 'st_ids_edit_distance')
    else:
        check(lib.st_ctc_greedy_edit_distance(_p(prob), B, T, V, _p(text, torch.int64), L, _p(ign, torch.int32), len(ignore),
                                              _p(dist, torch.int32), _p(ref_len, torch.int32), _p(hyp, torch.int64), _p(hyp_len, torch.int32),
                                              stream_handle()), 'st_ctc_greedy_edit_distance')
    return (dist, ref_len, hyp, hyp_len) if want_hyp else (dist, ref_len)


CB_MAX_T, CB_MIN_V, CB_MAX_V, CB_MAX_W = 4096, 2, 1024, 128          # st_ctc_beam_search's limits


def ctc_beam_search(prob, lengths=None, beam_width=16, top_paths=1, blank=0, log_input=False, eps=1e-10, bonus=None, order=None, bos=1):
    """CTC prefix beam search of prob (B, T, V) fp32 on one GPU (see st_ctc_beam_search).  lengths: None (all T frames), or (B,) integer
    frame counts -- a host tensor / sequence is checked against [0, T] here, a device tensor is taken as it is (the kernel clamps it).
    -> (hyp (B, top_paths, T) int64 0-padded, hyp_len (B, top_paths) int32, score (B, top_paths) float32) device tensors; one launch,
    no host read.  bonus: None (st_ctc_beam_search, the acoustic search), or the fused n-gram table of st_ctc_beam_search_lm: a contiguous
    (V^(order-1), V) float32 tensor on the device of prob (order: None = from the shape; bos: the start id of the empty prefix's
    context); its values are not read here.  Anything the kernel would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(prob) or not prob.is_cuda or prob.dim() != 3 or prob.dtype != torch.float32:
        raise ValueError('ctc_beam_search: prob must be a (B, T, V) float32 GPU tensor (got %s)' % _got(prob))
    B, T, V = prob.shape
    W, N, blank = int(beam_width), int(top_paths), int(blank)
    if B < 1 or not (1 <= T <= CB_MAX_T and CB_MIN_V <= V <= CB_MAX_V):
        raise ValueError('ctc_beam_search: B=%d, T=%d, V=%d outside B >= 1, 1 <= T <= %d, %d <= V <= %d' % (B, T, V, CB_MAX_T, CB_MIN_V, CB_MAX_V))
    if not (1 <= W <= CB_MAX_W and 1 <= N <= W):
        raise ValueError('ctc_beam_search: need 1 <= top_paths <= beam_width <= %d (beam_width %d, top_paths %d)' % (CB_MAX_W, W, N))
    if not 0 <= blank < V:
        raise ValueError('ctc_beam_search: blank %d outside [0, %d)' % (blank, V))
    if not eps >= 0.0:
        raise ValueError('ctc_beam_search: eps must be >= 0 (got %r)' % (eps,))
    dev = prob.device
    if bonus is not None:
        if not torch.is_tensor(bonus) or not bonus.is_cuda or bonus.device != dev or bonus.dim() != 2 or bonus.dtype != torch.float32 \
                or not bonus.is_contiguous():
            raise ValueError('ctc_beam_search: bonus must be a contiguous (V^(order-1), V) float32 tensor on the device of prob (got %s)' % _got(bonus))
        found = _ngram_order_of(bonus.shape[0], V) if bonus.shape[1] == V else None
        if found is None:
            raise ValueError('ctc_beam_search: a bonus table of shape %s is no (V^(order-1), V) table for V = %d, 1 <= order <= %d'
                             % (tuple(bonus.shape), V, CB_MAX_ORDER))
        if order is not None and int(order) != found:
            raise ValueError('ctc_beam_search: order %r, but the bonus table of shape %s has order %d' % (order, tuple(bonus.shape), found))
        order, bos = found, int(bos)
        if V ** order > CB_MAX_TABLE:
            raise ValueError('ctc_beam_search: V^order = %d^%d table elements, at most 2^26' % (V, order))
        if not 0 <= bos < V:
            raise ValueError('ctc_beam_search: bos %d outside [0, %d)' % (bos, V))
    elif order is not None:
        raise ValueError('ctc_beam_search: order %r without a bonus table' % (order,))
    lengths = _lengths('ctc_beam_search', 'lengths', lengths, (B,), 0, T, 'prob', dev, '(B,)')
    lib = _lib.load()
    prob = prob.contiguous()
    hyp = torch.empty(B, N, T, device=dev, dtype=torch.int64)
    hyp_len = torch.empty(B, N, device=dev, dtype=torch.int32)
    score = torch.empty(B, N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_ctc_beam_workspace_bytes(B, T, W)), device=dev, dtype=torch.uint8)
    if bonus is None:
        check(lib.st_ctc_beam_search(_p(prob), B, T, V, _p(lengths, torch.int32), W, N, blank, 1 if log_input else 0, float(eps),
                                     _p(hyp, torch.int64), _p(hyp_len, torch.int32), _p(score), _p(ws, torch.uint8), stream_handle()),
              'st_ctc_beam_search')
    else:
        check(lib.st_ctc_beam_search_lm(_p(prob), B, T, V, _p(lengths, torch.int32), W, N, blank, 1 if log_input else 0, float(eps),
                                        _p(bonus), order, bos, _p(hyp, torch.int64), _p(hyp_len, torch.int32), _p(score),
                                        _p(ws, torch.uint8), stream_handle()), 'st_ctc_beam_search_lm')
    return hyp, hyp_len, score


CA_MAX_T, CA_MIN_V, CA_MAX_V, CA_MAX_L = 4096, 2, 10240, 1024          # st_ctc_forced_align's limits


def ctc_forced_align(prob, text, lengths=None, text_lengths=None, blank=0, log_input=False, eps=1e-10):
    """CTC forced alignment (Viterbi) of text (B, L) int64 to prob (B, T, V) fp32 on one GPU (see st_ctc_forced_align).  lengths /
    text_lengths: None (all T frames / all L entries), or (B,) integers -- a host tensor / sequence is checked against [0, T] / [0, L]
    here, a device tensor is taken as it is (the kernel clamps it).  The targets are the non-blank entries of each row of text.
    -> (score (B,) float32, path (B, T) int32, tok_start (B, L) int32, tok_end (B, L) int32) device tensors; one launch, no host read.
    Anything the kernel would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(prob) or not prob.is_cuda or prob.dim() != 3 or prob.dtype != torch.float32:
        raise ValueError('ctc_forced_align: prob must be a (B, T, V) float32 GPU tensor (got %s)' % _got(prob))
    dev = prob.device
    if not torch.is_tensor(text) or not text.is_cuda or text.device != dev or text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('ctc_forced_align: text must be a (B, L) int64 tensor on the device of prob (got %s)' % _got(text))
    B, T, V = prob.shape
    L, blank = text.shape[1], int(blank)
    if text.shape[0] != B:
        raise ValueError('ctc_forced_align: %d utterances of prob, %d of text' % (B, text.shape[0]))
    if B < 1 or not (1 <= T <= CA_MAX_T and CA_MIN_V <= V <= CA_MAX_V and 1 <= L <= CA_MAX_L):
        raise ValueError('ctc_forced_align: B=%d, T=%d, V=%d, L=%d outside B >= 1, 1 <= T <= %d, %d <= V <= %d, 1 <= L <= %d'
                         % (B, T, V, L, CA_MAX_T, CA_MIN_V, CA_MAX_V, CA_MAX_L))
    if not 0 <= blank < V:
        raise ValueError('ctc_forced_align: blank %d outside [0, %d)' % (blank, V))
    if not eps >= 0.0:
        raise ValueError('ctc_forced_align: eps must be >= 0 (got %r)' % (eps,))
    lengths = _lengths('ctc_forced_align', 'lengths', lengths, (B,), 0, T, 'prob', dev, '(B,)')
    text_lengths = _lengths('ctc_forced_align', 'text_lengths', text_lengths, (B,), 0, L, 'prob', dev, '(B,)')
    lib = _lib.load()
    prob, text = prob.contiguous(), text.contiguous()
    score = torch.empty(B, device=dev, dtype=torch.float32)
    path = torch.empty(B, T, device=dev, dtype=torch.int32)
    tok_start = torch.empty(B, L, device=dev, dtype=torch.int32)
    tok_end = torch.empty(B, L, device=dev, dtype=torch.int32)
    nbytes = int(lib.st_ctc_align_workspace_bytes(B, T, L))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_ctc_forced_align(_p(prob), B, T, V, _p(lengths, torch.int32), _p(text, torch.int64), L, _p(text_lengths, torch.int32),
                                  blank, 1 if log_input else 0, float(eps), _p(score), _p(path, torch.int32), _p(tok_start, torch.int32),
                                  _p(tok_end, torch.int32), _p(ws, torch.uint8), stream_handle()), 'st_ctc_forced_align')
    return score, path, tok_start, tok_end


DTW_MAX_T, DTW_MAX_D = 4096, 64          # st_dtw_batch's limits


def _dtw_side(name, t):
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError('dtw: %s must be a (B, T, D) float32 GPU tensor (got %s)' % (name, _got(t)))


def dtw(x, y, x_len=None, y_len=None, cols=None, scale=1.0, want_path=True):
    """Dynamic time warping of x (B, Tx, D) against y (B, Ty, D), fp32 on one GPU, pair by pair (see st_dtw_batch): Euclidean frame
    distance over the columns cols = (d0, d1) (None: all D) times `scale`, unweighted symmetric steps, ties to the diagonal, then
    (i-1, j).  Any batch / row strides (the last dimension has stride 1: a column window of a wider tensor is passed as cols, not as
    a slice).  x_len / y_len: None (all rows), or (B,) integers -- a host tensor / sequence is checked against [0, Tx] / [0, Ty] here,
    a device tensor is taken as it is (the kernel clamps it).
    -> (total (B,) float32, path_len (B,) int32, path (B, Tx + Ty - 1, 2) int32 or None when want_path is false) device tensors;
    one launch, no host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    _dtw_side('x', x)
    _dtw_side('y', y)
    dev = x.device
    if y.device != dev:
        raise ValueError('dtw: x on %s, y on %s' % (x.device, y.device))
    B, Tx, D = x.shape
    Ty = y.shape[1]
    if y.shape[0] != B or y.shape[2] != D:
        raise ValueError('dtw: x is %s, y is %s: the pairs and the columns must match' % (tuple(x.shape), tuple(y.shape)))
    if B < 1 or not (1 <= Tx <= DTW_MAX_T and 1 <= Ty <= DTW_MAX_T) or D < 1:
        raise ValueError('dtw: B=%d, Tx=%d, Ty=%d, D=%d outside B >= 1, 1 <= Tx, Ty <= %d, D >= 1' % (B, Tx, Ty, D, DTW_MAX_T))
    if cols is None:
        cols = (0, D)
    try:
        d0, d1 = (int(c) for c in cols)
    except (TypeError, ValueError):
        raise ValueError('dtw: cols must be a pair (d0, d1) (got %r)' % (cols,))
    if not (0 <= d0 < d1 <= D and d1 - d0 <= DTW_MAX_D):
        raise ValueError('dtw: cols [%d, %d) outside 0 <= d0 < d1 <= D = %d, at most %d columns' % (d0, d1, D, DTW_MAX_D))
    scale = float(scale)
    if not 0.0 < scale < float('inf'):
        raise ValueError('dtw: scale must be finite and positive (got %r)' % (scale,))
    strides = []
    for name, t in (('x', x), ('y', y)):
        sb, st = (t.stride(0) if B > 1 else 0), (t.stride(1) if t.shape[1] > 1 else max(t.stride(1), d1))     # (a 1-long dimension's stride is free)
        if (t.stride(2) != 1 and D > 1) or st < d1 or sb < 0:
            raise ValueError('dtw: %s has strides %s: the last dimension needs stride 1 and rows at least d1 = %d floats apart'
                             % (name, tuple(t.stride()), d1))
        strides.append((sb, st))
    x_len = _lengths('dtw', 'x_len', x_len, (B,), 0, Tx, 'x', dev, '(B,)')
    y_len = _lengths('dtw', 'y_len', y_len, (B,), 0, Ty, 'x', dev, '(B,)')
    lib = _lib.load()
    total = torch.empty(B, device=dev, dtype=torch.float32)
    path_len = torch.empty(B, device=dev, dtype=torch.int32)
    path = torch.empty(B, Tx + Ty - 1, 2, device=dev, dtype=torch.int32) if want_path else None
    nbytes = int(lib.st_dtw_workspace_bytes(B, Tx, Ty))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_dtw_batch(_p(x), strides[0][0], strides[0][1], _p(x_len, torch.int32), Tx, _p(y), strides[1][0], strides[1][1],
                           _p(y_len, torch.int32), Ty, B, d0, d1, scale, _p(total), _p(path_len, torch.int32), _p(path, torch.int32),
                           _p(ws, torch.uint8), stream_handle()), 'st_dtw_batch')
    return total, path_len, path


ABX_MAX_LEN, ABX_MAX_D = 64, 512         # st_dtw_pairs' limits
ABX_METRICS = {'euclid': 0, 'angular': 1, 'kl': 2}


def _abx_ints(what, name, t, dev, dtype=torch.int32, dim=1):
    if (not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dim() != dim or t.dtype != dtype or not t.is_contiguous()):
        raise ValueError('%s: %s must be a contiguous %d-d %s tensor on the device of the features (got %s)'
                         % (what, name, dim, str(dtype).replace('torch.', ''),
                            _got(t)))


def dtw_pairs(feat, item_start, item_len, pair_a, pair_b, metric='angular', max_len=ABX_MAX_LEN, want_cost=False):
    """Path-normalised DTW distance of P pairs of items of one packed feature buffer, one wave a pair (see st_dtw_pairs): feat (n_rows, D)
    float32 on one GPU with unit column stride (a column slice of a wider tensor keeps its row stride); item q is the rows
    [item_start[q], item_start[q] + item_len[q]); pair p is item pair_a[p] against item pair_b[p] -- four contiguous int32 device tensors.
    metric: 'euclid', 'angular' or 'kl' (or its number).  max_len: the longest item the launch takes (it sizes LDS; at most 64).
    -> dist (P,) float32, or (dist, cost (P,) float32, path_len (P,) int32) with want_cost; NaN / 0 for a pair the kernel refuses (a bad
    index, a length outside [1, max_len], rows outside feat, a NaN among its rows).  One launch, no host read.  Anything the C entry
    point would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(feat) or not feat.is_cuda or feat.dim() != 2 or feat.dtype != torch.float32:
        raise ValueError('dtw_pairs: feat must be a (n_rows, D) float32 GPU tensor (got %s)' % _got(feat))
    dev = feat.device
    n_rows, D = feat.shape
    if n_rows < 1 or not 1 <= D <= ABX_MAX_D:
        raise ValueError('dtw_pairs: feat is %s: n_rows >= 1 and 1 <= D <= %d' % (tuple(feat.shape), ABX_MAX_D))
    st = feat.stride(0) if n_rows > 1 else max(feat.stride(0), D)          # (a 1-long dimension's stride is free)
    if (feat.stride(1) != 1 and D > 1) or st < D:
        raise ValueError('dtw_pairs: feat has strides %s: the columns need stride 1 and the rows at least D = %d floats apart'
                         % (tuple(feat.stride()), D))
    if isinstance(metric, str):
        if metric not in ABX_METRICS:
            raise ValueError('dtw_pairs: metric %r is none of %s' % (metric, sorted(ABX_METRICS)))
        metric = ABX_METRICS[metric]
    if not _is_int(metric) or int(metric) not in ABX_METRICS.values():
        raise ValueError('dtw_pairs: metric %r is none of %s' % (metric, sorted(ABX_METRICS)))
    if not _is_int(max_len) or not 1 <= int(max_len) <= ABX_MAX_LEN:
        raise ValueError('dtw_pairs: max_len must be an integer in [1, %d] (got %r)' % (ABX_MAX_LEN, max_len))
    for name, t in (('item_start', item_start), ('item_len', item_len), ('pair_a', pair_a), ('pair_b', pair_b)):
        _abx_ints('dtw_pairs', name, t, dev)
    n_items, P = item_start.shape[0], pair_a.shape[0]
    if n_items < 1 or item_len.shape[0] != n_items:
        raise ValueError('dtw_pairs: %d item starts, %d item lengths: at least one item, as many of each'
                         % (n_items, item_len.shape[0]))
    if P < 1 or pair_b.shape[0] != P or P >= 2 ** 31:
        raise ValueError('dtw_pairs: %d first items, %d second items: at least one pair, below 2^31, as many of each' % (P, pair_b.shape[0]))
    lib = _lib.load()
    dist = torch.empty(P, device=dev, dtype=torch.float32)
    cost = torch.empty(P, device=dev, dtype=torch.float32) if want_cost else None
    path_len = torch.empty(P, device=dev, dtype=torch.int32) if want_cost else None
    check(lib.st_dtw_pairs(_p(feat), n_rows, D, st, _p(item_start, torch.int32), _p(item_len, torch.int32), n_items, _p(pair_a, torch.int32),
                           _p(pair_b, torch.int32), P, int(metric), int(max_len), _p(dist), _p(cost), _p(path_len, torch.int32),
                           stream_handle()), 'st_dtw_pairs')
    return (dist, cost, path_len) if want_cost else dist


def abx_count(dmat, blk):
    """ABX triple counts from finished distances (see st_abx_count): dmat, a contiguous 1-d float32 GPU tensor holding the dense symmetric
    matrices of the cells end to end; blk (NB, 6) int64 on the same device, rows (mat_off, n_c, a_lo, a_hi, b_lo, b_hi).
    -> count (NB, 4) int64 = (wrong, tied, nan, triples) per block, a device tensor; one launch, exact, no host read.  Bad arguments
    raise ValueError before the device is touched."""
    if not torch.is_tensor(dmat) or not dmat.is_cuda or dmat.dim() != 1 or dmat.dtype != torch.float32 or not dmat.is_contiguous():
        raise ValueError('abx_count: dmat must be a contiguous 1-d float32 GPU tensor (got %s)' % _got(dmat))
    _abx_ints('abx_count', 'blk', blk, dmat.device, torch.int64, 2)
    NB = blk.shape[0]
    if blk.shape[1] != 6 or NB < 1 or NB >= 2 ** 31 or dmat.shape[0] < 1:
        raise ValueError('abx_count: blk is %s over %d distances: (NB, 6) with NB >= 1, at least one distance' % (tuple(blk.shape), dmat.shape[0]))
    lib = _lib.load()
    count = torch.empty(NB, 4, device=dmat.device, dtype=torch.int64)
    check(lib.st_abx_count(_p(dmat), dmat.shape[0], _p(blk, torch.int64), NB, _p(count, torch.int64), stream_handle()), 'st_abx_count')
    return count


def abx_across(dmat, grp, xr):
    """Across-speaker ABX group errors and counts from finished distances (see st_abx_across): dmat, a contiguous 1-d float32 GPU tensor
    holding the dense matrices of the contexts end to end; grp (NG, 8) int64 on the same device, rows (mat_off, n_c, a_lo, a_hi, b_lo,
    b_hi, xr_lo, xr_hi); xr (NX, 2) int64, the X index ranges the groups' slices name.
    -> (err (NG,) float64, count (NG, 5) int64 = (wrong, tied, nan, triples, x_speakers)), device tensors; one launch, exact, no host
    read.  Bad arguments raise ValueError before the device is touched."""
    if not torch.is_tensor(dmat) or not dmat.is_cuda or dmat.dim() != 1 or dmat.dtype != torch.float32 or not dmat.is_contiguous():
        raise ValueError('abx_across: dmat must be a contiguous 1-d float32 GPU tensor (got %s)' % _got(dmat))
    _abx_ints('abx_across', 'grp', grp, dmat.device, torch.int64, 2)
    _abx_ints('abx_across', 'xr', xr, dmat.device, torch.int64, 2)
    NG, NX = grp.shape[0], xr.shape[0]
    if grp.shape[1] != 8 or NG < 1 or NG >= 2 ** 31 or dmat.shape[0] < 1:
        raise ValueError('abx_across: grp is %s over %d distances: (NG, 8) with NG >= 1, at least one distance' % (tuple(grp.shape), dmat.shape[0]))
    if xr.shape[1] != 2 or NX < 1:
        raise ValueError('abx_across: xr is %s: (NX, 2) with NX >= 1' % (tuple(xr.shape),))
    lib = _lib.load()
    err = torch.empty(NG, device=dmat.device, dtype=torch.float64)
    count = torch.empty(NG, 5, device=dmat.device, dtype=torch.int64)
    check(lib.st_abx_across(_p(dmat), dmat.shape[0], _p(grp, torch.int64), NG, _p(xr, torch.int64), NX, _p(err, torch.float64), _p(count, torch.int64),
                            stream_handle()), 'st_abx_across')
    return err, count


KM_MAX_D, KM_MAX_K, KM_MAX_FLOATS = 256, 4096, 2 ** 40        # the k-means entry points' limits
KM_CHUNK = 1024                      # points of a histogram chunk of st_kmeans_update and of a seeding chunk: the tests straddle it
KM_SLAB = 256                        # members of a summation slab of st_kmeans_update


def _km_data(what, x):
    """the (N, D) float32 GPU matrix every k-means op clusters (unit column stride; a column slice keeps its row stride) -> st_kmeans_data"""
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError('%s: x must be a (N, D) float32 GPU tensor (got %s)' % (what, _got(x)))
    N, D = x.shape
    if N < 1 or N >= 2 ** 31 or not 1 <= D <= KM_MAX_D:
        raise ValueError('%s: x is %s: 1 <= N < 2^31 and 1 <= D <= %d' % (what, tuple(x.shape), KM_MAX_D))
    ld = x.stride(0) if N > 1 else max(x.stride(0), D)            # (a 1-long dimension's stride is free)
    if (x.stride(1) != 1 and D > 1) or ld < D or N * ld >= KM_MAX_FLOATS:
        raise ValueError('%s: x has strides %s: the columns need stride 1, the rows at least D = %d floats apart, N * stride below 2^40'
                         % (what, tuple(x.stride()), D))
    return _lib.StKmeansData(None, ld, N, D)


def _km_tensor(what, name, t, x, shape, dtype, symbol):
    """an operand of a k-means op: a contiguous tensor of `shape` and `dtype` on the device of x"""
    if not torch.is_tensor(t) or not t.is_cuda or t.device != x.device or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
        raise ValueError('%s: %s must be a contiguous %s %s tensor on the device of x (got %s)'
                         % (what, name, symbol, str(dtype).replace('torch.', ''), _got(t)))


def _km_cent(what, name, cent, x):
    """a (K, D) table of centroids for x -> K"""
    if not torch.is_tensor(cent) or cent.dim() != 2 or not 1 <= cent.shape[0] <= KM_MAX_K:
        raise ValueError('%s: %s must be a (K, D) tensor with 1 <= K <= %d (got %s)' % (what, name, KM_MAX_K, _got(cent)))
    _km_tensor(what, name, cent, x, (cent.shape[0], x.shape[1]), torch.float32, '(K, D = %d)' % x.shape[1])
    return cent.shape[0]


def _km_fill(d, x):
    d.x = _p(x)
    return C.byref(d)


def kmeans_assign(x, cent):
    """the nearest centroid of every row (see st_kmeans_assign): x (N, D) float32 on one GPU, cent (K, D) float32 contiguous on the same
    device -> (idx (N,) int32, the smallest k at the least squared distance, -1 for a row holding a NaN or an infinity; dist (N,) float32, that
    distance, NaN for such a row).  One launch, no host read.  Bad arguments raise ValueError before the device is touched."""
    d = _km_data('kmeans_assign', x)
    K = _km_cent('kmeans_assign', 'cent', cent, x)
    lib = _lib.load()
    idx = torch.empty(d.N, device=x.device, dtype=torch.int32)
    dist = torch.empty(d.N, device=x.device, dtype=torch.float32)
    check(lib.st_kmeans_assign(_km_fill(d, x), _p(cent), K, _p(idx, torch.int32), _p(dist), stream_handle()), 'st_kmeans_assign')
    return idx, dist


def kmeans_update(x, idx, dist, cent_in):
    """the centroids of an assignment (see st_kmeans_update): idx (N,) int32 and dist (N,) float32 as kmeans_assign gives them, cent_in
    (K, D) float32 -> (cent_out (K, D) float32: the float64 mean of a cluster's members, cent_in's row for an empty cluster; count (K,)
    int32; stats (4,) float64 = (inertia, the squared shift of the table, empty clusters, rows that are no member)).  Bitwise repeatable;
    seven launches, no host read.  Bad arguments raise ValueError before the device is touched."""
    d = _km_data('kmeans_update', x)
    _km_tensor('kmeans_update', 'idx', idx, x, (d.N,), torch.int32, '(N = %d,)' % d.N)
    _km_tensor('kmeans_update', 'dist', dist, x, (d.N,), torch.float32, '(N = %d,)' % d.N)
    K = _km_cent('kmeans_update', 'cent_in', cent_in, x)
    lib = _lib.load()
    dev = x.device
    cent_out = torch.empty(K, d.D, device=dev, dtype=torch.float32)
    count = torch.empty(K, device=dev, dtype=torch.int32)
    stats = torch.empty(4, device=dev, dtype=torch.float64)
    ws = torch.empty(int(lib.st_kmeans_update_workspace_bytes(d.N, d.D, K)) // 8 + 2, device=dev, dtype=torch.float64)
    check(lib.st_kmeans_update(_km_fill(d, x), _p(idx, torch.int32), _p(dist), _p(cent_in), K, _p(cent_out), _p(count, torch.int32),
                               _p(stats, torch.float64), _p(ws, torch.float64), stream_handle()), 'st_kmeans_update')
    return cent_out, count, stats


def kmeans_relocate(x, idx, dist, count, cent):
    """move the empty clusters (see st_kmeans_relocate): the e-th cluster with count 0 takes the row of the e-th point in the order (dist
    descending, index ascending); cent (K, D) float32 is changed in place -> cent.  One launch.  Bad arguments raise ValueError before
    the device is touched."""
    d = _km_data('kmeans_relocate', x)
    _km_tensor('kmeans_relocate', 'idx', idx, x, (d.N,), torch.int32, '(N = %d,)' % d.N)
    _km_tensor('kmeans_relocate', 'dist', dist, x, (d.N,), torch.float32, '(N = %d,)' % d.N)
    K = _km_cent('kmeans_relocate', 'cent', cent, x)
    _km_tensor('kmeans_relocate', 'count', count, x, (K,), torch.int32, '(K = %d,)' % K)
    lib = _lib.load()
    check(lib.st_kmeans_relocate(_km_fill(d, x), _p(idx, torch.int32), _p(dist), _p(count, torch.int32), K, _p(cent), stream_handle()),
          'st_kmeans_relocate')
    return cent


def kmeans_pp_init(x, K, u):
    """k-means++ seeding (see st_kmeans_pp_step): K rows of x, the first at floor(u[0] N), the j-th drawn with probability proportional
    to the squared distance to the nearest of the rows before it by u[j]; u: K numbers in [0, 1) (a host sequence, or a (K,) float64
    tensor on the device of x).  -> (cent (K, D) float32, picks (K,) int32, mind (N,) float32: the squared distance of every row to the
    nearest pick).  2 K launches and one host read, of the flag that fewer than K distinct rows exist: that raises ValueError, as bad
    arguments do before the device is touched."""
    d = _km_data('kmeans_pp_init', x)
    if not _is_int(K) or not 1 <= int(K) <= KM_MAX_K:
        raise ValueError('kmeans_pp_init: K must be an integer in [1, %d] (got %r)' % (KM_MAX_K, K))
    K = int(K)
    if torch.is_tensor(u) and u.is_cuda:
        _km_tensor('kmeans_pp_init', 'u', u, x, (K,), torch.float64, '(K = %d,)' % K)
    else:
        host = np.asarray(u.cpu() if torch.is_tensor(u) else u, dtype=np.float64)
        if host.shape != (K,) or not ((host >= 0.0) & (host < 1.0)).all():
            raise ValueError('kmeans_pp_init: u must be K = %d numbers in [0, 1) (got %s)' % (K, host.tolist() if host.size <= 8 else host.shape))
        u = host
    lib = _lib.load()
    dev = x.device
    if not torch.is_tensor(u) or not u.is_cuda:
        u = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
    cent = torch.empty(K, d.D, device=dev, dtype=torch.float32)
    picks = torch.zeros(K, device=dev, dtype=torch.int32)
    mind = torch.full((d.N,), float('inf'), device=dev, dtype=torch.float32)
    part = torch.zeros(int(lib.st_kmeans_chunks(d.N)), device=dev, dtype=torch.float64)
    totals = torch.zeros(K, device=dev, dtype=torch.float64)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    px, s = _km_fill(d, x), stream_handle()
    for j in range(K):
        check(lib.st_kmeans_pp_pick(px, _p(mind), _p(part, torch.float64), _p(u, torch.float64), j, K, _p(picks, torch.int32),
                                    _p(totals, torch.float64), _p(flag, torch.int32), s), 'st_kmeans_pp_pick')
        check(lib.st_kmeans_pp_step(px, _p(picks, torch.int32), j, K, _p(mind), _p(part, torch.float64), _p(cent), s), 'st_kmeans_pp_step')
    if int(flag.item()):                                           # (the one host read)
        raise ValueError('kmeans_pp_init: x holds fewer than K = %d distinct rows' % K)
    return cent, picks, mind


AE_MAX_S, AE_MAX_L = 4096, 2048         # st_attn_endpoint's limits


def attn_endpoint(align, enc_len, patience=3, max_jump=4):
    """End of speech and alignment diagnostics of align (B, S, L), fp32 on one GPU, utterance by utterance (see st_attn_endpoint).
    Any batch / row strides with unit stride in L (a sliced view is read where it lies).  enc_len: (B,) real phones per utterance -- a
    host sequence / tensor is checked against [1, L] here, a device tensor is taken as it is (the kernel clamps it).
    -> (stats (B, 6) int32 = (end, reached, n_back, n_skip, covered, nonfinite), focus (B,) float32, peak (B, S) int32,
    dur (B, L) int32) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError before the
    device is touched."""
    if not torch.is_tensor(align) or not align.is_cuda or align.dim() != 3 or align.dtype != torch.float32:
        raise ValueError('attn_endpoint: align must be a (B, S, L) float32 GPU tensor (got %s)' % _got(align))
    dev = align.device
    B, S, L = align.shape
    if B < 1 or not (1 <= S <= AE_MAX_S and 1 <= L <= AE_MAX_L):
        raise ValueError('attn_endpoint: B=%d, S=%d, L=%d outside B >= 1, 1 <= S <= %d, 1 <= L <= %d' % (B, S, L, AE_MAX_S, AE_MAX_L))
    for name, v in (('patience', patience), ('max_jump', max_jump)):
        if not _is_int(v) or not 1 <= int(v) <= 2 ** 31 - 1:
            raise ValueError('attn_endpoint: %s must be an integer >= 1 (got %r)' % (name, v))
    sb, st = (align.stride(0) if B > 1 else 0), (align.stride(1) if S > 1 else max(align.stride(1), L))     # (a 1-long dimension's stride is free)
    if (align.stride(2) != 1 and L > 1) or st < L or sb < 0:
        raise ValueError('attn_endpoint: align has strides %s: the last dimension needs stride 1 and rows at least L = %d floats apart'
                         % (tuple(align.stride()), L))
    enc_len = _lengths('attn_endpoint', 'enc_len', enc_len, (B,), 1, L, 'align', dev, '(B,)', optional=False)
    lib = _lib.load()
    # one allocation, carved into the four contiguous outputs (the call is latency-bound: three more torch.empty cost as much as the kernel)
    flat = torch.empty(B * (7 + S + L), device=dev, dtype=torch.int32)
    stats, focus = flat[:6 * B].view(B, 6), flat[6 * B:7 * B].view(torch.float32)
    peak, dur = flat[7 * B:(7 + S) * B].view(B, S), flat[(7 + S) * B:].view(B, L)
    check(lib.st_attn_endpoint(_p(align), sb, st, _p(enc_len, torch.int32), B, S, L, int(patience), int(max_jump), _p(stats, torch.int32),
                               _p(focus), _p(peak, torch.int32), _p(dur, torch.int32), stream_handle()), 'st_attn_endpoint')
    return stats, focus, peak, dur


def hyp_edit_distance(hyp, hyp_len, text, ignore):
    """edit distance of transcripts that are already collapsed (a beam search's) to `text`, per utterance (see st_hyp_edit_distance):
    hyp (B, Lh) int64 with hyp_len (B,) int32 tokens each, text (B, L) int64, ignore: the ids dropped from both sides.  -> (dist,
    ref_len) int32 (B,) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError first."""
    if not all(torch.is_tensor(x) for x in (hyp, hyp_len, text)):
        raise ValueError('hyp_edit_distance: hyp, hyp_len and text must be tensors')
    if not (hyp.is_cuda and hyp.device == hyp_len.device == text.device):
        raise ValueError('hyp_edit_distance: hyp, hyp_len and text must be on one GPU (got %s, %s, %s)' % (hyp.device, hyp_len.device, text.device))
    if hyp.dim() != 2 or hyp.dtype != torch.int64 or text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('hyp_edit_distance: hyp and text must be 2-D int64 (got %s %s, %s %s)'
                         % (tuple(hyp.shape), hyp.dtype, tuple(text.shape), text.dtype))
    B, Lh = hyp.shape
    L = text.shape[1]
    if hyp_len.shape != (B,) or hyp_len.dtype != torch.int32:
        raise ValueError('hyp_edit_distance: hyp_len must be (%d,) int32 (got %s %s)' % (B, tuple(hyp_len.shape), hyp_len.dtype))
    ignore = tuple(int(i) for i in ignore)
    if text.shape[0] != B or B < 1:
        raise ValueError('hyp_edit_distance: %d hypotheses, %d transcripts (at least one)' % (B, text.shape[0]))
    if not (1 <= Lh <= GED_MAX_T and 1 <= L <= GED_MAX_L and len(ignore) <= GED_MAX_IGNORE):
        raise ValueError('hyp_edit_distance: Lh=%d, L=%d, %d ignored ids outside 1 <= Lh <= %d, 1 <= L <= %d, <= %d ignored ids'
                         % (Lh, L, len(ignore), GED_MAX_T, GED_MAX_L, GED_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('hyp_edit_distance: ignored ids must fit int32')
    dev = hyp.device
    ign = _ignore_dev(ignore, dev)
    hyp, hyp_len, text = hyp.contiguous(), hyp_len.contiguous(), text.contiguous()
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    ref_len = torch.empty(B, device=dev, dtype=torch.int32)
    check(_lib.load().st_hyp_edit_distance(_p(hyp, torch.int64), _p(hyp_len, torch.int32), B, Lh, _p(text, torch.int64), L,
                                           _p(ign, torch.int32), len(ignore), _p(dist, torch.int32), _p(ref_len, torch.int32),
                                           stream_handle()), 'st_hyp_edit_distance')
    return dist, ref_len


EA_MAX_L, EA_MAX_V, EA_MAX_IGNORE = 1024, 1024, 64          # st_edit_align's limits


def edit_align(hyp, hyp_len, ref, ref_len=None, ignore=(), n_classes=1, confusion=None, want_ali=True):
    """Levenshtein alignment with its trace-back, pair by pair on one GPU (see st_edit_align): hyp (B, N, Lh) int64 transcripts of
    hyp_len (B, N) tokens, N paths per utterance, against ref (B, Lr) int64 of ref_len (B,) tokens (None: all Lr); a host sequence of
    lengths is checked against [0, L] here, a device tensor is taken as it is (the kernel clamps it).  ignore: the ids dropped from
    both sides.  confusion: None, a (n_classes + 1, n_classes + 1) int32 device tensor that path 0 of every utterance is added into, or
    True for a zeroed one made here.
    -> (counts (B, N, 4) int32 = correct, substitutions, deletions, insertions; ali_len (B, N) int32; ali (B, N, Lr + Lh, 2) int32 or
    None when want_ali is false; the confusion tensor or None) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError before
    the device is touched."""
    for name, t in (('hyp', hyp), ('ref', ref)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int64:
            raise ValueError('edit_align: %s must be an int64 GPU tensor (got %s)' % (name, _got(t)))
    dev = hyp.device
    if ref.device != dev:
        raise ValueError('edit_align: hyp on %s, ref on %s' % (hyp.device, ref.device))
    if hyp.dim() != 3 or ref.dim() != 2:
        raise ValueError('edit_align: hyp must be (B, N, Lh) and ref (B, Lr) (got %s, %s)' % (tuple(hyp.shape), tuple(ref.shape)))
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    if ref.shape[0] != B:
        raise ValueError('edit_align: %d utterances of hypotheses, %d references: they must match' % (B, ref.shape[0]))
    if B < 1 or N < 1 or B * N > 2 ** 24:
        raise ValueError('edit_align: B=%d, N=%d outside B >= 1, N >= 1, B N <= 2^24' % (B, N))
    if not (1 <= Lh <= EA_MAX_L and 1 <= Lr <= EA_MAX_L):
        raise ValueError('edit_align: Lh=%d, Lr=%d outside 1 <= Lh, Lr <= %d' % (Lh, Lr, EA_MAX_L))
    V = n_classes
    if not _is_int(V) or not 1 <= int(V) <= EA_MAX_V:
        raise ValueError('edit_align: n_classes must be an integer in [1, %d] (got %r)' % (EA_MAX_V, V))
    V = int(V)
    try:
        ignore = tuple(int(i) for i in ignore)
    except (TypeError, ValueError):
        raise ValueError('edit_align: ignore must be a sequence of integer ids (got %r)' % (ignore,))
    if len(ignore) > EA_MAX_IGNORE:
        raise ValueError('edit_align: %d ignored ids, at most %d' % (len(ignore), EA_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('edit_align: ignored ids must fit int32')
    if confusion is not None and confusion is not True:
        if (not torch.is_tensor(confusion) or not confusion.is_cuda or confusion.device != dev or confusion.dtype != torch.int32
                or tuple(confusion.shape) != (V + 1, V + 1) or not confusion.is_contiguous()):
            raise ValueError('edit_align: confusion must be a contiguous (%d, %d) int32 tensor on the device of hyp (got %s)'
                             % (V + 1, V + 1, _got(confusion)))
    hyp_len = _lengths('edit_align', 'hyp_len', hyp_len, (B, N), 0, Lh, 'hyp', dev, optional=False)
    ref_len = _lengths('edit_align', 'ref_len', ref_len, (B,), 0, Lr, 'hyp', dev)
    lib = _lib.load()
    ign = _ignore_dev(ignore, dev)
    hyp, ref = hyp.contiguous(), ref.contiguous()
    if confusion is True:
        confusion = torch.zeros(V + 1, V + 1, device=dev, dtype=torch.int32)
    # one allocation, carved into the outputs (the call is latency-bound)
    AL = Lr + Lh
    flat = torch.empty(B * N * (5 + (2 * AL if want_ali else 0)), device=dev, dtype=torch.int32)
    counts, ali_len = flat[:4 * B * N].view(B, N, 4), flat[4 * B * N:5 * B * N].view(B, N)
    ali = flat[5 * B * N:].view(B, N, AL, 2) if want_ali else None
    nbytes = int(lib.st_edit_align_workspace_bytes(B * N, Lr, Lh))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_edit_align(_p(hyp, torch.int64), _p(hyp_len, torch.int32), B, N, Lh, _p(ref, torch.int64), _p(ref_len, torch.int32), Lr,
                            _p(ign, torch.int32), len(ignore), V, _p(counts, torch.int32), _p(ali_len, torch.int32), _p(ali, torch.int32),
                            _p(confusion, torch.int32), _p(ws, torch.uint8), stream_handle()), 'st_edit_align')
    return counts, ali_len, ali, confusion


# --------------------------------------------------------------------------------------------- Griffin-Lim vocoder (src/audio.py)
def _audio_ws(fn, B, T, n_fft, hop, win, device):
    n = fn(B, T, n_fft, hop, win)
    if n == 0:
        raise RuntimeError('semi_tts_amd: bad STFT dimensions B=%d T=%d n_fft=%d hop=%d win=%d' % (B, T, n_fft, hop, win))
    return torch.empty(n, device=device, dtype=torch.float32)


def stft_fwd(x, n_fft, hop, win):
    """torch.stft(x (B, L), n_fft, hop, win, hann_window(win), center=True, pad_mode='reflect', onesided) on the HIP kernel:
    -> (B, T, n_fft // 2 + 1, 2) float32, frame-major (re, im), T = 1 + L // hop."""
    assert x.dim() == 2 and x.is_contiguous()
    B, L = x.shape
    spec = torch.empty(B, 1 + L // hop, n_fft // 2 + 1, 2, device=x.device, dtype=torch.float32)
    check(_lib.load().st_stft_fwd(_p(x), _p(spec), B, L, n_fft, hop, win, stream_handle()), 'st_stft_fwd')
    return spec


def istft(spec, n_fft, hop, win):
    """inverse of stft_fwd (lib/istft.py semantics, no `length`): spec (B, T, n_fft // 2 + 1, 2) -> (B, hop * (T - 1))"""
    assert spec.dim() == 4 and spec.shape[2] == n_fft // 2 + 1 and spec.shape[3] == 2 and spec.is_contiguous()
    B, T = spec.shape[:2]
    lib = _lib.load()
    ws = _audio_ws(lib.st_istft_workspace_floats, B, T, n_fft, hop, win, spec.device)
    x = torch.empty(B, hop * (T - 1), device=spec.device, dtype=torch.float32)
    check(lib.st_istft(_p(spec), _p(x), B, T, n_fft, hop, win, _p(ws), stream_handle()), 'st_istft')
    return x


GL_INV_PREEMPHASIS, GL_CLIP = 1, 2


def griffin_lim(feat, phases, n_fft, hop, win, n_iter=30, normalized=False, power=1.0, post=0):
    """griffin_lim_batch() on a linear spectrogram with one frame count: feat (B, T, F) in any strides (the decoder's (B, T, F) output
    or a transposed (B, F, T) magnitude), phases (B, F, T) contiguous -> waveform (B, hop * (T - 1)).  post: GL_INV_PREEMPHASIS | GL_CLIP."""
    return griffin_lim_batch(feat, phases, n_fft, hop, win, n_iter=n_iter, normalized=normalized, power=power, post=post)


MEL_TO_LINEAR_TILE = 16          # frames per workgroup of st_mel_to_linear (MEL_TILE in audio.hip): the tests straddle it
MEL_MAX = 256                    # most mel bins st_mel_to_linear takes (MEL_MAX in audio.hip)


def mel_to_linear(mel, basis, normalized=True, take_abs=False):
    """st_mel_to_linear: mel (B, T, n_mels) in any strides, basis (n_mels, F) contiguous (the transposed pseudo-inverse of the mel
    filterbank) -> (B, T, F) = sum_m basis[m, k] a[b, t, m], a the denormalised amplitude of mel (normalized) or mel itself;
    take_abs stores the magnitude Griffin-Lim takes."""
    assert mel.dim() == 3 and basis.dim() == 2 and basis.is_contiguous() and basis.shape[0] == mel.shape[2]
    B, T, n_mels = mel.shape
    F = basis.shape[1]
    lin = torch.empty(B, T, F, device=mel.device, dtype=torch.float32)
    sb, st, sm = mel.stride()
    check(_lib.load().st_mel_to_linear(_p(mel), sb, st, sm, _p(basis), _p(lin), B, T, n_mels, F, int(bool(normalized)),
                                       int(bool(take_abs)), stream_handle()), 'st_mel_to_linear')
    return lin


def griffin_lim_batch(feat, phases, n_fft, hop, win, n_iter=30, normalized=False, power=1.0, post=0, basis=None, frames=None):
    """st_griffin_lim_batch, the one vocoder entry: utterances of one length or of their own, linear or mel input.  feat (B, T, F)
    linear in any strides, or (B, T, n_mels) with basis (n_mels, F) as mel_to_linear() takes it; phases (B, F, T) contiguous; frames:
    device int32 (B,) frame counts (None: T for all).  -> waveform (B, hop * (T - 1)), row b filled on [0, hop * (frames[b] - 1))
    and zero after.  feat rows and phase columns beyond an utterance's frames are never read."""
    F = n_fft // 2 + 1
    assert feat.dim() == 3 and feat.shape[2] == (F if basis is None else basis.shape[0])
    B, T, n_in = feat.shape
    assert phases.shape == (B, F, T) and phases.is_contiguous()
    assert basis is None or (basis.shape == (n_in, F) and basis.is_contiguous())
    assert frames is None or (frames.shape == (B,) and frames.dtype == torch.int32 and frames.is_contiguous() and frames.is_cuda)
    lib = _lib.load()
    ws = _audio_ws(lib.st_gl_batch_workspace_floats, B, T, n_fft, hop, win, feat.device)
    wav = torch.empty(B, hop * (T - 1), device=feat.device, dtype=torch.float32)
    sb, st, sf = feat.stride()
    job = _lib.StGlJob(feat=_p(feat), sb=sb, st=st, sf=sf, n_in=n_in, basis=_p(basis), normalized=int(bool(normalized)), power=float(power),
                       phases=_p(phases), frames=_p(frames, torch.int32), wav=_p(wav), B=B, T=T, n_iter=int(n_iter), post=int(post))
    check(lib.st_griffin_lim_batch(C.byref(job), C.byref(_lib.StFraming(n_fft, win, hop)), _p(ws), stream_handle()), 'st_griffin_lim_batch')
    return wav


# --------------------------------------------------------------------------------------------- feature extraction (src/audio.py)
FEATURES_MAX_BATCH = 64          # utterances per st_audio_features call (its per-utterance metadata travels by value)


def _chunks(B):
    """(first utterance, count) of every call a batch of B utterances is issued in"""
    return [(b0, min(FEATURES_MAX_BATCH, B - b0)) for b0 in range(0, B, FEATURES_MAX_BATCH)]


def _host_ptr(a, b0):
    """address of row b0 of a contiguous host array (None stays None)"""
    return None if a is None else a.ctypes.data + b0 * a.itemsize


def _host_off_lens(off, lens):
    return np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int32)


def _wave_batch(x):
    """StWaveBatch of the packed buffer x, without its per-call off / len / B (_wave_chunk sets them)"""
    return _lib.StWaveBatch(x=_p(x), n_samples=x.numel())


def _wave_args(what, x, off, lens):
    """the packed buffer and the utterances in it as the op `what` takes them -> (off int64, lens int32) contiguous host arrays"""
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('%s: x must be a packed 1-D contiguous float32 GPU tensor (got %s)' % (what, _got(x)))
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    if off.shape != (B,) or (off < 0).any() or (off + lens > x.numel()).any():
        raise ValueError('%s: an utterance lies outside the %d packed samples (off %s, lens %s)' % (what, x.numel(), off.tolist(), lens.tolist()))
    return off, lens


def _lens_check(what, lens):
    """the lengths of a ragged batch that is issued in chunks: B >= 1 integers in [1, 2^31)"""
    lens = np.asarray(lens)
    if lens.ndim != 1 or lens.shape[0] < 1 or lens.dtype.kind not in 'iu' or (lens < 1).any() or (lens >= 2 ** 31).any():
        raise ValueError('%s: lens must be B >= 1 integers in [1, 2^31) (got %s)' % (what, lens.tolist(),))


def _pair_lens(what, lens, subject, each, max_batch, max_len):
    """the lengths of one call's signals of a batch of pairs: 0 .. max_batch integers in [1, max_len] -> the array"""
    v = np.asarray(lens)
    if v.ndim != 1 or not 0 <= v.shape[0] <= max_batch or (v.shape[0] and v.dtype.kind not in 'iu'):
        raise ValueError('%s: %s must be 0 .. %d integers, one call takes no more pairs (got %s)'
                         % (what, subject, max_batch, 'shape %s, %s' % (v.shape, v.dtype)))
    if v.shape[0] and ((v < 1).any() or (v > max_len).any()):
        raise ValueError('%s: every %s must lie in [1, %d] (got %s)' % (what, each, max_len, v.tolist()))
    return v


def _wave_operands(x, n_fft, win, hop, fb):
    """the operands st_audio_features and st_audio_mfcc share: (StWaveBatch without its per-call off / len / B, StFraming, StMelBank)"""
    assert x.dim() == 1 and x.is_contiguous()
    fs, fc, fo, fw = fb
    return (_wave_batch(x), _lib.StFraming(n_fft, win, hop),
            _lib.StMelBank(start=_p(fs, torch.int32), cnt=_p(fc, torch.int32), off=_p(fo, torch.int32), w=_p(fw), n_mels=fs.shape[0]))


def _wave_chunk(w, off, lens, b0, nb):
    """points the StWaveBatch `w` (modified in place) at utterances [b0, b0 + nb) and returns a reference to it"""
    w.off, w.len, w.B = _host_ptr(off, b0), _host_ptr(lens, b0), nb
    return C.byref(w)


def audio_features(x, off, lens, n_fft, win, hop, preemph, fb, T_pad, with_linear=True, aug_win=None, aug_hop=None, Ta_pad=None,
                   snr_db=None, noise=None, seed=0):
    """st_audio_features on a ragged batch: x the packed float32 waveforms (device), utterance b = x[off[b]:off[b] + lens[b]];
    fb = (start, count, offset, weights) device tensors of the banded mel filterbank.  -> (mel (B, T_pad, n_mels),
    linear (B, T_pad, n_fft // 2 + 1) or None, aug (B, Ta_pad, n_mels) or None); the augmented mel when aug_win / aug_hop (per
    utterance) are given, with noise at snr_db[b] (NaN: none) from `noise` (packed like x) or the built-in generator of `seed`.
    Batches above FEATURES_MAX_BATCH are issued in chunks of it; the generator is keyed on the position in the whole batch
    (feature_noise(n, b, seed) is utterance b's noise whatever B is)."""
    assert noise is None or (noise.shape == x.shape and noise.is_contiguous())
    w, fr, bank = _wave_operands(x, n_fft, win, hop, fb)
    n_mels, F = bank.n_mels, n_fft // 2 + 1
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    use_aug = aug_win is not None
    dev = x.device
    mel = torch.empty(B, T_pad, n_mels, device=dev, dtype=torch.float32)
    lin = torch.empty(B, T_pad, F, device=dev, dtype=torch.float32) if with_linear else None
    aug = torch.empty(B, Ta_pad, n_mels, device=dev, dtype=torch.float32) if use_aug else None
    if use_aug:
        aug_win = np.ascontiguousarray(aug_win, dtype=np.int32)
        aug_hop = np.ascontiguousarray(aug_hop, dtype=np.int32)
    if snr_db is not None:
        snr_db = np.ascontiguousarray(snr_db, dtype=np.float32)
    lib = _lib.load()
    ws = torch.empty(lib.st_features_workspace_floats(min(B, FEATURES_MAX_BATCH)), device=dev, dtype=torch.float32)
    a = _lib.StFeatAug(noise=_p(noise), seed=int(seed) & (2 ** 64 - 1), Ta_pad=Ta_pad or 0)
    for b0, nb in _chunks(B):
        a.win, a.hop, a.snr_db, a.utt0, a.out = _host_ptr(aug_win, b0), _host_ptr(aug_hop, b0), _host_ptr(snr_db, b0), b0, _p(aug[b0:]) if use_aug else None
        check(lib.st_audio_features(_wave_chunk(w, off, lens, b0, nb), C.byref(fr), float(preemph), C.byref(bank), C.byref(a), _p(mel[b0:]),
                                    _p(lin[b0:]) if with_linear else None, T_pad, _p(ws), stream_handle()), 'st_audio_features')
    return mel, lin, aug


def feature_noise(n, utt, seed, device):
    """the built-in noise generator of st_audio_features: (n,) standard normals of (seed, utterance utt, sample index)"""
    out = torch.empty(n, device=device, dtype=torch.float32)
    check(_lib.load().st_feature_noise(_p(out), n, utt, int(seed) & (2 ** 64 - 1), stream_handle()), 'st_feature_noise')
    return out


MFCC_MIN_FRAMES = 9              # fewest frames per utterance st_audio_mfcc takes: the width of the derivative filters


def audio_mfcc(x, off, lens, n_fft, win, hop, preemph, fb, dct, T_pad, with_mel=False):
    """st_audio_mfcc on a ragged batch packed as for audio_features: dct (n_mfcc, n_mels) float32 on the device (audio.mfcc_dct);
    win / hop: the MFCC framing.  -> (mfcc (B, T_pad, 3 * n_mfcc): cepstra, first and second derivatives; mel (B, T_pad, n_mels) at
    that framing, or None without with_mel).  Batches above FEATURES_MAX_BATCH are issued in chunks of it."""
    w, fr, bank = _wave_operands(x, n_fft, win, hop, fb)
    n_mels = bank.n_mels
    assert dct.dim() == 2 and dct.shape[1] == n_mels and dct.is_contiguous()
    n_mfcc = dct.shape[0]
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    out = torch.empty(B, T_pad, 3 * n_mfcc, device=x.device, dtype=torch.float32)
    mel = torch.empty(B, T_pad, n_mels, device=x.device, dtype=torch.float32) if with_mel else None
    lib = _lib.load()
    for b0, nb in _chunks(B):
        check(lib.st_audio_mfcc(_wave_chunk(w, off, lens, b0, nb), C.byref(fr), float(preemph), C.byref(bank), _p(dct), n_mfcc, _p(out[b0:]),
                                _p(mel[b0:]) if with_mel else None, T_pad, stream_handle()), 'st_audio_mfcc')
    return out, mel


def segment_gather(feat, seg_utt, seg_start, seg_len, max_len):
    """st_segment_gather: feat (B, T_pad, D) float32 on the device, rows contiguous; seg_utt / seg_start / seg_len: device int32 (S,).
    -> (S, max_len, D): row i < seg_len[s] of segment s = feat[seg_utt[s], seg_start[s] + i], every other row 0."""
    assert feat.dim() == 3 and feat.stride(2) == 1
    B, T_pad, D = feat.shape
    S = seg_utt.shape[0]
    for a in (seg_utt, seg_start, seg_len):
        assert a.shape == (S,) and a.dtype == torch.int32 and a.is_contiguous() and a.device == feat.device
    out = torch.empty(S, max_len, D, device=feat.device, dtype=torch.float32)
    check(_lib.load().st_segment_gather(_p(feat), feat.stride(0), feat.stride(1), B, T_pad, D, _p(seg_utt, torch.int32),
                                        _p(seg_start, torch.int32), _p(seg_len, torch.int32), S, int(max_len), _p(out), stream_handle()),
          'st_segment_gather')
    return out


# --------------------------------------------------------------------------------------------- sample-rate conversion
RESAMPLE_TILE = 1024                 # outputs per workgroup of st_resample_batch (RS_TILE in resample.hip): the tests straddle it
RESAMPLE_MAX_TABLE_FLOATS = 9216     # LDS floats of the staged table: min(n, RESAMPLE_TILE) rows of (taps | 1) + 1 (RS_MAX_TABLE)
RESAMPLE_MAX_STAGE_FLOATS = 6912     # LDS floats of a tile's input span (RS_MAX_STAGE)


def resample_lds_floats(o, n, taps, first_min, first_max):
    """(staged table floats, staged input floats) of one st_resample_batch workgroup at the ratio o / n: what the two limits bound"""
    return min(n, RESAMPLE_TILE) * ((taps | 1) + 1), ((RESAMPLE_TILE - 1) * o + n - 1) // n + first_max - first_min + taps


def resample_batch(x, off, lens, o, n, first, table, first_min, first_max, out=None):
    """st_resample_batch on a ragged batch: x the packed waveforms on the device, float32 or int16 PCM (scaled by 1 / 32768 in the
    kernel); utterance b = x[off[b]:off[b] + lens[b]].  first (n,) int32 and table (n, taps) float32: the device copies of
    audio.resample_table(); first_min / first_max the bounds of first.  -> (y, out_off, out_lens): the packed float32 output
    (`out`, a contiguous 1-D float32 device tensor of exactly the summed output lengths, or a new one), utterance b =
    y[out_off[b]:out_off[b] + out_lens[b]], out_lens[b] = ceil(n lens[b] / o).  Batches above FEATURES_MAX_BATCH are issued in
    chunks of it."""
    assert x.dim() == 1 and x.is_contiguous() and x.dtype in (torch.float32, torch.int16)
    assert table.dim() == 2 and table.shape[0] == n and table.is_contiguous() and table.dtype == torch.float32
    assert first.shape == (n,) and first.dtype == torch.int32 and first.is_contiguous()
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    out_lens = (lens.astype(np.int64) * n + o - 1) // o
    out_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(out_lens)[:-1]]), dtype=np.int64)
    total = int(out_lens.sum())
    if out is None:
        out = torch.empty(total, device=x.device, dtype=torch.float32)
    assert out.dim() == 1 and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == total and out.device == x.device
    lib = _lib.load()
    for b0, nb in _chunks(B):
        check(lib.st_resample_batch(_p(x, x.dtype), int(x.dtype == torch.int16), x.numel(), _host_ptr(off, b0), _host_ptr(lens, b0), nb,
                                    int(o), int(n), table.shape[1], int(first_min), int(first_max), _p(first, torch.int32), _p(table),
                                    _p(out), total, _host_ptr(out_off, b0), stream_handle()), 'st_resample_batch')
    return out, out_off, out_lens


# --------------------------------------------------------------------------------------------- pitch (st_f0_yin, st_f0_path_scores)
F0_MAX_TAU, F0_MAX_W = 1024, 2048    # st_f0_yin's limits
F0_RUN, F0_MAX_SPAN = 8, 10240       # frames a workgroup takes from one staged span, and the samples such a span may hold (f0.hip)


def f0_run_length(hop, W, tau_max):
    """the consecutive frames one st_f0_yin workgroup takes at this framing (st_f0_run_length): the tests straddle it"""
    r = F0_RUN
    while r > 1 and (r - 1) * int(hop) + int(W) + int(tau_max) > F0_MAX_SPAN:
        r -= 1
    return r


def _f0_check(lens, hop, W, tau_min, tau_max, sample_rate, threshold):
    """every refusal of st_f0_yin that does not need the buffers, raised before any device is touched"""
    for name, v in (('hop', hop), ('W', W), ('tau_min', tau_min), ('tau_max', tau_max)):
        if not _is_int(v):
            raise ValueError('f0_yin: %s must be an integer (got %r)' % (name, v))
    if hop < 1:
        raise ValueError('f0_yin: hop %d below 1' % hop)
    if not 2 <= tau_min < tau_max <= F0_MAX_TAU:
        raise ValueError('f0_yin: lags [%d, %d] outside 2 <= tau_min < tau_max <= %d' % (tau_min, tau_max, F0_MAX_TAU))
    if not 1 <= W <= F0_MAX_W:
        raise ValueError('f0_yin: window W = %d outside [1, %d]' % (W, F0_MAX_W))
    threshold, sample_rate = float(threshold), float(sample_rate)
    if not 0.0 < threshold <= 1.0:
        raise ValueError('f0_yin: threshold must lie in (0, 1] (got %r)' % (threshold,))
    if not 0.0 < sample_rate < float('inf'):
        raise ValueError('f0_yin: sample_rate must be finite and positive (got %r)' % (sample_rate,))
    _lens_check('f0_yin', lens)


def f0_yin(x, off, lens, hop, W, tau_min, tau_max, sample_rate, threshold, T_pad, with_aper=False):
    """st_f0_yin on a ragged batch packed as for audio_features: x the packed float32 waveforms on the device, utterance b =
    x[off[b]:off[b] + lens[b]].  -> (f0 (B, T_pad) in Hz, 0 on unvoiced frames and on the rows past 1 + lens[b] // hop; aper (B, T_pad),
    the normalised difference at the chosen lag, or None without with_aper).  Batches above FEATURES_MAX_BATCH are issued in chunks
    of it.  Anything the kernel would refuse raises ValueError before the device is touched."""
    _f0_check(lens, hop, W, tau_min, tau_max, sample_rate, threshold)
    off, lens = _wave_args('f0_yin', x, off, lens)
    B = len(lens)
    T_pad = int(T_pad)
    if T_pad < 1 + int(lens.max()) // hop:
        raise ValueError('f0_yin: T_pad %d below the %d frames of the longest utterance' % (T_pad, 1 + int(lens.max()) // hop))
    lib = _lib.load()
    f0 = torch.empty(B, T_pad, device=x.device, dtype=torch.float32)
    aper = torch.empty(B, T_pad, device=x.device, dtype=torch.float32) if with_aper else None
    w = _wave_batch(x)
    for b0, nb in _chunks(B):
        check(lib.st_f0_yin(_wave_chunk(w, off, lens, b0, nb), int(hop), int(W), int(tau_min), int(tau_max), float(sample_rate), float(threshold),
                            _p(f0[b0:]), _p(aper[b0:]) if with_aper else None, T_pad, stream_handle()), 'st_f0_yin')
    return f0, aper


def f0_path_scores(f0_x, f0_y, path, path_len):
    """st_f0_path_scores: f0_x (B, Tx) and f0_y (B, Ty) float32 tracks on one GPU (unit stride along a row, any row stride), path
    (B, P, 2) int32 and path_len (B,) int32 on the same device.  THE PATH MUST COME FROM metrics.dtw / metrics.mcd over sequences of
    Tx and Ty rows (P = Tx + Ty - 1): the kernel reads its first path_len entries as indices without checking them.
    -> (counts (B, 4) int32 = (n_pairs, n_both, n_vuv, n_gross), sums (B, 2) float32 = (sum c^2, sum c) in cents over the both-voiced
    pairs) device tensors; one launch, no host read.  Anything else raises ValueError before the device is touched."""
    for name, t in (('f0_x', f0_x), ('f0_y', f0_y)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError('f0_path_scores: %s must be a (B, T) float32 GPU tensor (got %s)' % (name, _got(t)))
    dev = f0_x.device
    B, Tx = f0_x.shape
    Ty = f0_y.shape[1]
    if f0_y.device != dev or f0_y.shape[0] != B or B < 1 or Tx < 1 or Ty < 1:
        raise ValueError('f0_path_scores: f0_x is %s on %s, f0_y is %s on %s: B >= 1 pairs of at least one frame on one device'
                         % (tuple(f0_x.shape), f0_x.device, tuple(f0_y.shape), f0_y.device))
    strides = []
    for name, t in (('f0_x', f0_x), ('f0_y', f0_y)):
        sb = t.stride(0) if B > 1 else 0
        if (t.stride(1) != 1 and t.shape[1] > 1) or sb < 0:
            raise ValueError('f0_path_scores: %s has strides %s: a row needs unit stride' % (name, tuple(t.stride())))
        strides.append(sb)
    if (not torch.is_tensor(path) or not path.is_cuda or path.device != dev or path.dtype != torch.int32
            or tuple(path.shape) != (B, Tx + Ty - 1, 2) or not path.is_contiguous()):
        raise ValueError('f0_path_scores: path must be the contiguous (B, Tx + Ty - 1, 2) = (%d, %d, 2) int32 tensor of metrics.dtw on the device '
                         'of the tracks (got %s)' % (B, Tx + Ty - 1, _got(path)))
    if (not torch.is_tensor(path_len) or not path_len.is_cuda or path_len.device != dev or path_len.dtype != torch.int32
            or tuple(path_len.shape) != (B,) or not path_len.is_contiguous()):
        raise ValueError('f0_path_scores: path_len must be the (B,) int32 tensor of metrics.dtw on the device of the tracks (got %s)' % _got(path_len))
    lib = _lib.load()
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    sums = torch.empty(B, 2, device=dev, dtype=torch.float32)
    check(lib.st_f0_path_scores(_p(f0_x), strides[0], Tx, _p(f0_y), strides[1], Ty, _p(path, torch.int32), _p(path_len, torch.int32), B,
                                Tx + Ty - 1, _p(counts, torch.int32), _p(sums), stream_handle()), 'st_f0_path_scores')
    return counts, sums


# --------------------------------------------------------------------------------------------- silence trimming (st_trim_silence)
TRIM_MAX_FRAME_LENGTH = 8192         # st_trim_silence's limit
TRIM_RUN, TRIM_MAX_SPAN = 16, 12288  # frames a workgroup takes from one staged span, and the samples such a span may hold (trim.hip)
TRIM_CHUNK = 256                     # frames per step of the decision launch: the tests straddle it


def trim_run_length(frame_length, hop):
    """the consecutive frames one st_trim_silence workgroup takes at this framing (st_trim_run_length): the tests straddle it"""
    r = TRIM_RUN
    while r > 1 and (r - 1) * int(hop) + int(frame_length) > TRIM_MAX_SPAN:
        r -= 1
    return r


def trim_ratio(top_db):
    """the threshold ratio of st_trim_silence: 10^(-top_db / 10) in double, rounded once to float32"""
    return float(np.float32(10.0 ** (-float(top_db) / 10.0)))


def _trim_check(lens, frame_length, hop, top_db, pad=0, max_iv=0):
    """every refusal of st_trim_silence that does not need the buffers, raised before any device is touched"""
    for name, v in (('frame_length', frame_length), ('hop', hop), ('pad', pad), ('max_iv', max_iv)):
        if not _is_int(v):
            raise ValueError('trim_silence: %s must be an integer (got %r)' % (name, v))
    if not 1 <= hop <= frame_length <= TRIM_MAX_FRAME_LENGTH:
        raise ValueError('trim_silence: needs 1 <= hop <= frame_length <= %d (hop %d, frame_length %d)' % (TRIM_MAX_FRAME_LENGTH, hop, frame_length))
    if not _is_number(top_db) or not np.isfinite(top_db):
        raise ValueError('trim_silence: top_db must be a finite number (got %r)' % (top_db,))
    if not 0.0 < trim_ratio(top_db) < 1.0:
        raise ValueError('trim_silence: top_db %r gives the ratio %r; it must lie strictly inside (0, 1) in float32'
                         % (top_db, trim_ratio(top_db)))
    if not 0 <= pad < 2 ** 31:
        raise ValueError('trim_silence: pad %d outside [0, 2^31)' % pad)
    if not 0 <= max_iv < 2 ** 30:
        raise ValueError('trim_silence: max_iv %d outside [0, 2^30)' % max_iv)
    _lens_check('trim_silence', lens)


def trim_silence(x, off, lens, frame_length, hop, top_db, pad=0, max_iv=0, T_pad=None, energy=None):
    """st_trim_silence on a ragged batch packed as for audio_features: x the packed float32 waveforms on the device, utterance b =
    x[off[b]:off[b] + lens[b]] (the offsets need not be cumulative).  -> device tensors (energy (B, T_pad) float32, 0 on the rows past
    1 + lens[b] // hop; bounds (B, 4) int32 = (start, end, non-silent frames, flags); intervals (B, max_iv, 2) int32 and n_iv (B,)
    int32, or None, None with max_iv = 0).  T_pad None: the longest utterance's frames.  Batches above FEATURES_MAX_BATCH are
    issued in chunks of it.  energy: a contiguous (B, T_pad) float32 tensor on x's device to write the energies into (default: a new one).
    Anything the kernel would refuse raises ValueError before the device is touched."""
    _trim_check(lens, frame_length, hop, top_db, pad, max_iv)
    off, lens = _wave_args('trim_silence', x, off, lens)
    B = len(lens)
    frames = 1 + int(lens.max()) // hop
    T_pad = frames if T_pad is None else int(T_pad)
    if T_pad < frames:
        raise ValueError('trim_silence: T_pad %d below the %d frames of the longest utterance' % (T_pad, frames))
    lib = _lib.load()
    dev = x.device
    if energy is None:
        energy = torch.empty(B, T_pad, device=dev, dtype=torch.float32)
    elif not (torch.is_tensor(energy) and energy.shape == (B, T_pad) and energy.dtype == torch.float32 and energy.is_contiguous() and energy.device == dev):
        raise ValueError('trim_silence: energy must be a contiguous (%d, %d) float32 tensor on %s' % (B, T_pad, dev))
    bounds = torch.empty(B, 4, device=dev, dtype=torch.int32)
    iv = torch.empty(B, max_iv, 2, device=dev, dtype=torch.int32) if max_iv else None
    n_iv = torch.empty(B, device=dev, dtype=torch.int32) if max_iv else None
    ratio = trim_ratio(top_db)
    w = _wave_batch(x)
    for b0, nb in _chunks(B):
        check(lib.st_trim_silence(_wave_chunk(w, off, lens, b0, nb), int(frame_length), int(hop), ratio, int(pad), int(max_iv), _p(energy[b0:]),
                                  T_pad, _p(bounds[b0:], torch.int32), _p(iv[b0:], torch.int32) if max_iv else None,
                                  _p(n_iv[b0:], torch.int32) if max_iv else None, stream_handle()), 'st_trim_silence')
    return energy, bounds, iv, n_iv


# --------------------------------------------------------------------------------------------- loudness (st_loudness_batch, st_wave_gain)
LOUDNESS_MIN_SR, LOUDNESS_MAX_SR = 8000, 48000     # st_loudness_batch's limits
LOUDNESS_THREADS = 256                             # runs a hop is cut into (loudness.hip)
LOUDNESS_TABLE_DOUBLES = 152 + 256 * 16            # ST_LOUDNESS_TABLE_DOUBLES
LOUDNESS_FLAGS = {'nonfinite': 1, 'short': 2, 'silent': 4, 'peak_limited': 8, 'gain_limited': 16}


def loudness_hop(sr):
    """samples of a 100 ms hop at this rate: (sr + 5) // 10"""
    return (int(sr) + 5) // 10


def loudness_run_length(sr):
    """the samples one st_loudness_batch thread owns at this rate (st_loudness_run_length): the tests straddle it"""
    return (loudness_hop(sr) + LOUDNESS_THREADS - 1) // LOUDNESS_THREADS


def _loudness_check(lens, sr, target=None, peak_db=-1.0, max_gain_db=30.0, H_pad=None):
    """every refusal of st_loudness_batch that does not need the buffers, raised before any device is touched -> (hop, H_pad)"""
    if not _is_int(sr) or not LOUDNESS_MIN_SR <= sr <= LOUDNESS_MAX_SR:
        raise ValueError('loudness: the sample rate must be an integer in [%d, %d] (got %r)' % (LOUDNESS_MIN_SR, LOUDNESS_MAX_SR, sr))
    for name, v in (('peak_db', peak_db), ('max_gain_db', max_gain_db)):
        if not _is_number(v) or not np.isfinite(v):
            raise ValueError('loudness: %s must be a finite number (got %r)' % (name, v))
    if target is not None and (not _is_number(target) or np.isinf(target)):
        raise ValueError('loudness: target must be a finite number, or None / NaN to measure only (got %r)' % (target,))
    lens = np.asarray(lens)
    if lens.ndim != 1 or not 1 <= lens.shape[0] <= FEATURES_MAX_BATCH or lens.dtype.kind not in 'iu':
        raise ValueError('loudness: lens must be 1 .. %d integers, one call takes no more utterances (got %s)'
                         % (FEATURES_MAX_BATCH, 'shape %s, %s' % (lens.shape, lens.dtype)))
    if (lens < 1).any() or (lens >= 2 ** 31).any():
        raise ValueError('loudness: every length must lie in [1, 2^31) (got %s)' % (lens.tolist(),))
    hop = loudness_hop(sr)
    hops = int(lens.max()) // hop
    if H_pad is None:
        H_pad = max(1, hops)
    if not _is_int(H_pad) or H_pad < hops or H_pad >= 2 ** 31:
        raise ValueError('loudness: H_pad %r below the %d hops of the longest utterance' % (H_pad, hops))
    return hop, int(H_pad)


def loudness(x, off, lens, sr, target=None, peak_db=-1.0, max_gain_db=30.0, H_pad=None):
    """st_loudness_batch (ITU-R BS.1770-4 integrated loudness; the definition is in include/semitts.h) on a ragged batch packed as for
    audio_features: x the packed float32 waveforms on the device, utterance b = x[off[b]:off[b] + lens[b]], at most FEATURES_MAX_BATCH
    of them (the callers above split).  -> device tensors (hop_energy (B, H_pad) float32, stats (B, 8) float32 = (L_I, momentary
    maximum, relative gate, sample peak, ungated, gain, 0, 0), counts (B, 4) int32 = (blocks, above the absolute gate, above the
    relative gate, flags)).  target None (or NaN): measure only, gain 1.  H_pad None: the longest utterance's hops (at least 1).
    Four launches, no host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    hop, H_pad = _loudness_check(lens, sr, target, peak_db, max_gain_db, H_pad)
    off, lens = _wave_args('loudness', x, off, lens)
    from .audio import kweight_tables                          # (here: audio imports this module)
    lib = _lib.load()
    dev = x.device
    tab = kweight_tables(sr, dev)
    B = len(lens)
    hop_energy = torch.empty(B, H_pad, device=dev, dtype=torch.float32)
    stats = torch.empty(B, 8, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = torch.empty(B * (H_pad + 1) * 9, device=dev, dtype=torch.float64)
    w = _wave_batch(x)
    check(lib.st_loudness_batch(_wave_chunk(w, off, lens, 0, B), int(sr), _p(tab, torch.float64), float('nan') if target is None else float(target),
                                float(peak_db), float(max_gain_db), _p(hop_energy), H_pad, _p(stats), _p(counts, torch.int32),
                                _p(ws, torch.float64), stream_handle()), 'st_loudness_batch')
    return hop_energy, stats, counts


def wave_gain(x, off, lens, stats, out=None, pcm16=False):
    """st_wave_gain: utterance b of the packed batch times the gain stats[b, 5] of `loudness`, read on the device (no host read).
    pcm16 False -> float32, one product a sample, written into `out` (a packed buffer like x; x itself is allowed: in place; default a
    new buffer of zeros).  pcm16 True -> int16, rint(clip(x g, -1, 1) * 32767) as audio.write_wav, into `out` (int16, x's size) or a
    new buffer of zeros.  Samples outside the utterances are not written.  At most FEATURES_MAX_BATCH utterances a call."""
    lens_a = np.asarray(lens)
    if lens_a.ndim != 1 or not 1 <= lens_a.shape[0] <= FEATURES_MAX_BATCH or lens_a.dtype.kind not in 'iu' or (lens_a < 1).any() or (lens_a >= 2 ** 31).any():
        raise ValueError('wave_gain: lens must be 1 .. %d integers in [1, 2^31) (got %s)' % (FEATURES_MAX_BATCH, lens_a.tolist()))
    off, lens = _wave_args('wave_gain', x, off, lens)
    B = len(lens)
    dt = torch.int16 if pcm16 else torch.float32
    if not (torch.is_tensor(stats) and stats.is_cuda and stats.device == x.device and stats.dtype == torch.float32 and tuple(stats.shape) == (B, 8)
            and stats.is_contiguous()):
        raise ValueError('wave_gain: stats must be the contiguous (%d, 8) float32 tensor of loudness() on %s' % (B, x.device))
    if out is None:
        out = torch.zeros(x.numel(), device=x.device, dtype=dt)
    elif not (torch.is_tensor(out) and out.device == x.device and out.dtype == dt and out.dim() == 1 and out.numel() == x.numel() and out.is_contiguous()):
        raise ValueError('wave_gain: out must be a contiguous 1-D %s tensor of %d samples on %s' % (dt, x.numel(), x.device))
    lib = _lib.load()
    w = _wave_batch(x)
    check(lib.st_wave_gain(_wave_chunk(w, off, lens, 0, B), _p(stats), None if pcm16 else _p(out), _p(out, torch.int16) if pcm16 else None,
                           stream_handle()), 'st_wave_gain')
    return out


# --------------------------------------------------------------------------------------------- intelligibility (st_stoi_batch)
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT = 10000, 256, 128, 512
STOI_BANDS, STOI_SEG = 15, 30
STOI_MAX_BATCH = 64                  # st_stoi_batch's limits: pairs a call ...
STOI_MAX_LEN = 1 << 22               # ... and samples of the longest signal (7 minutes at 10 kHz)
STOI_CHUNK = 256                     # frames per step of the selection launch's scan: the tests straddle it
STOI_SENTINEL = 1e-5                 # both scores of a pair with fewer than 30 band frames (pystoi's convention)
STOI_BAND_EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
                   (109, 138), (138, 174), (174, 219))


def stoi_frames(L):
    """F of an L-sample signal at 10 kHz: the frames i with 128 i < L - 256 (strict, as the authors' code); 0 when L <= 256"""
    L = int(L)
    return (L - STOI_FRAME + STOI_HOP - 1) // STOI_HOP if L > STOI_FRAME else 0


def _stoi_check(lens, F_pad=None):
    """every refusal of st_stoi_batch that does not need the buffers, raised before any device is touched -> F_pad"""
    lens = _pair_lens('stoi_batch', lens, 'lens', 'length', STOI_MAX_BATCH, STOI_MAX_LEN)
    frames = max([1] + [stoi_frames(v) for v in lens])
    if F_pad is None:
        F_pad = frames
    if not _is_int(F_pad) or F_pad < frames or F_pad >= 2 ** 24:
        raise ValueError('stoi_batch: F_pad %r below the %d frames of the longest signal (at least 1)' % (F_pad, frames))
    return int(F_pad)


def stoi_batch(x, y, off, lens, F_pad=None, want_parts=False):
    """st_stoi_batch (STOI and ESTOI; the definition is in include/semitts.h) on a ragged batch of pairs at 10 kHz: x the packed float32
    clean signals on the device, y the processed ones packed the same way (x's size), pair b = x / y[off[b]:off[b] + lens[b]], at most
    STOI_MAX_BATCH of them (metrics.stoi splits).  -> device tensors (score (B, 2) float32 = (STOI, ESTOI), counts (B, 4) int32 =
    (frames F, kept K, band frames M, segments S), and with want_parts energy (B, F_pad) float32, kept (B, F_pad) int32 with -1 past K,
    bands (B, 2, 15, F_pad) float32 with 0 past M; None, None, None without).  F_pad None: the longest signal's frames (at least 1).
    B = 0 launches nothing.  No host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    F_pad = _stoi_check(lens, F_pad)
    if not torch.is_tensor(y) or not torch.is_tensor(x) or y.shape != x.shape or y.device != x.device or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError('stoi_batch: y must be a packed 1-D contiguous float32 tensor of x\'s size on x\'s device (got %s)' % _got(y))
    off, lens = _wave_args('stoi_batch', x, off, lens)
    lib = _lib.load()
    dev = x.device
    B = len(lens)
    score = torch.empty(B, 2, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    energy = torch.empty(B, F_pad, device=dev, dtype=torch.float32) if want_parts else None
    kept = torch.empty(B, F_pad, device=dev, dtype=torch.int32) if want_parts else None
    bands = torch.empty(B, 2, STOI_BANDS, F_pad, device=dev, dtype=torch.float32) if want_parts else None
    if B == 0:
        return score, counts, energy, kept, bands
    ws = torch.empty(int(lib.st_stoi_workspace_floats(B, F_pad)), device=dev, dtype=torch.float32)
    w = _wave_batch(x)
    check(lib.st_stoi_batch(_wave_chunk(w, off, lens, 0, B), _p(y), _p(score), _p(counts, torch.int32), F_pad, _p(energy), _p(kept, torch.int32),
                            _p(bands), _p(ws), stream_handle()), 'st_stoi_batch')
    return score, counts, energy, kept, bands


# --------------------------------------------------------------------------------------------- alignment (st_xcorr_delay, st_sisdr_batch, st_wave_gather)
XCORR_MAX_BATCH = 64                 # st_xcorr_delay's limits: pairs a call ...
XCORR_MAX_LEN = 1 << 22              # ... samples of the longest signal of either side ...
XCORR_MAX_LAG = 16384                # ... and the search bound D (+-0.34 s at 48 kHz)
XCORR_CHUNK = 1024                   # samples of a staged piece, the smallest chunk of x: the tests straddle it
XCORR_LAG_TILE = 2048                # lags a workgroup owns: the tests straddle it
XCORR_MAX_CHUNKS = 32                # chunks of the longest signal: past 32 * 1024 samples the chunk grows
SISDR_CHUNK = 8192                   # samples a workgroup of st_sisdr_batch's first launch sums


def xcorr_chunk_len(L):
    """samples of one chunk of an L-sample reference: XCORR_CHUNK times the smallest factor that leaves at most XCORR_MAX_CHUNKS chunks"""
    return XCORR_CHUNK * ((int(L) + XCORR_CHUNK * XCORR_MAX_CHUNKS - 1) // (XCORR_CHUNK * XCORR_MAX_CHUNKS))


def _pair_check(what, xlens, ylens, max_lag=0):
    """every refusal of st_xcorr_delay / st_sisdr_batch that does not need the buffers, raised before any device is touched"""
    xl, yl = (_pair_lens(what, v, 'the lengths of ' + name, 'length of ' + name, XCORR_MAX_BATCH, XCORR_MAX_LEN)
              for name, v in (('x', xlens), ('y', ylens)))
    if xl.shape[0] != yl.shape[0]:
        raise ValueError('%s: %d references and %d processed signals: one of each per pair' % (what, xl.shape[0], yl.shape[0]))
    if not _is_int(max_lag) or not 0 <= max_lag <= XCORR_MAX_LAG:
        raise ValueError('%s: max_lag must be an integer in [0, %d] (got %r)' % (what, XCORR_MAX_LAG, max_lag))


def _pair_args(what, x, xoff, xlens, y, yoff, ylens):
    xoff, xlens = _wave_args(what, x, xoff, xlens)
    if not torch.is_tensor(y) or y.device != x.device:
        raise ValueError('%s: y must be a packed 1-D contiguous float32 tensor on x\'s device' % what)
    yoff, ylens = _wave_args(what, y, yoff, ylens)
    wx, wy = _wave_batch(x), _wave_batch(y)
    B = len(xlens)
    return _wave_chunk(wx, xoff, xlens, 0, B), _wave_chunk(wy, yoff, ylens, 0, B), (wx, wy, xoff, xlens, yoff, ylens)


def xcorr_delay(x, xoff, xlens, y, yoff, ylens, max_lag, want_corr=False):
    """st_xcorr_delay (the definition is in include/semitts.h): the integer delay of B pairs by direct float64 cross-correlation over
    the lags [-max_lag, max_lag].  x, y: two packed float32 device buffers, pair b = x[xoff[b]:xoff[b] + xlens[b]] against
    y[yoff[b]:yoff[b] + ylens[b]] (the lengths may differ, the offsets need not be cumulative), at most XCORR_MAX_BATCH pairs
    (metrics.delay splits).  -> device tensors (delay (B,) int32, positive: y is late; coef (B,) float32; corr (B, 2 max_lag + 1)
    float64 with want_corr, else None).  B = 0 launches nothing.  No host read.  Anything the kernel would refuse raises ValueError
    before the device is touched."""
    _pair_check('xcorr_delay', xlens, ylens, max_lag)
    px, py, keep = _pair_args('xcorr_delay', x, xoff, xlens, y, yoff, ylens)
    lib = _lib.load()
    dev, B, D = x.device, len(keep[3]), int(max_lag)
    delay = torch.empty(B, device=dev, dtype=torch.int32)
    coef = torch.empty(B, device=dev, dtype=torch.float32)
    corr = torch.empty(B, 2 * D + 1, device=dev, dtype=torch.float64) if want_corr else None
    if B == 0:
        return delay, coef, corr
    max_len = int(max(keep[3].max(), keep[5].max()))
    ws = torch.empty(int(lib.st_xcorr_workspace_bytes(B, max_len, D)) // 8, device=dev, dtype=torch.float64)
    check(lib.st_xcorr_delay(px, py, D, _p(delay, torch.int32), _p(coef), _p(corr, torch.float64), _p(ws, torch.float64), stream_handle()),
          'st_xcorr_delay')
    return delay, coef, corr


def sisdr_batch(x, xoff, xlens, y, yoff, ylens, delay=None, zero_mean=True):
    """st_sisdr_batch (the definition is in include/semitts.h): SI-SDR, SNR and gain of B pairs on the overlap a delay leaves.  x, y as
    for xcorr_delay.  delay: None (0) or a DEVICE int32 tensor (B,), read on the device only: the caller checks its values where they
    come from the host.  -> device tensors (score (B, 3) float32 = (SI-SDR dB, SNR dB, gain dB), sums (B, 6) float64 = (n, sum x, sum y,
    sum x^2, sum y^2, sum x y)).  B = 0 launches nothing.  No host read."""
    _pair_check('sisdr_batch', xlens, ylens)
    B = len(xlens)
    if delay is not None and not (torch.is_tensor(delay) and delay.is_cuda and delay.dtype == torch.int32 and tuple(delay.shape) == (B,)
                                  and delay.is_contiguous() and torch.is_tensor(x) and delay.device == x.device):
        raise ValueError('sisdr_batch: delay must be None or a contiguous (%d,) int32 tensor on x\'s device (got %s)' % (B, _got(delay)))
    px, py, keep = _pair_args('sisdr_batch', x, xoff, xlens, y, yoff, ylens)
    lib = _lib.load()
    dev = x.device
    score = torch.empty(B, 3, device=dev, dtype=torch.float32)
    sums = torch.empty(B, 6, device=dev, dtype=torch.float64)
    if B == 0:
        return score, sums
    max_len = int(max(keep[3].max(), keep[5].max()))
    ws = torch.empty(int(lib.st_sisdr_workspace_bytes(B, max_len)) // 8, device=dev, dtype=torch.float64)
    check(lib.st_sisdr_batch(px, py, _p(delay, torch.int32), int(bool(zero_mean)), _p(sums, torch.float64), _p(score), _p(ws, torch.float64),
                             stream_handle()), 'st_sisdr_batch')
    return score, sums


def wave_gather(src, src_off, dst, dst_off, lens):
    """st_wave_gather: dst[dst_off[b]:dst_off[b] + lens[b]] = src[src_off[b]:src_off[b] + lens[b]] for at most XCORR_MAX_BATCH spans in one
    launch; src, dst: two different contiguous 1-D float32 buffers on one device; nothing else of dst is written.  -> dst"""
    la = np.asarray(lens)
    if la.ndim != 1 or not 0 <= la.shape[0] <= XCORR_MAX_BATCH or (la.shape[0] and (la.dtype.kind not in 'iu' or (la < 1).any() or (la > XCORR_MAX_LEN).any())):
        raise ValueError('wave_gather: lens must be 0 .. %d integers in [1, %d] (got %s)' % (XCORR_MAX_BATCH, XCORR_MAX_LEN, la.tolist()))
    B = la.shape[0]
    so, do = np.asarray(src_off), np.asarray(dst_off)
    if so.shape != (B,) or do.shape != (B,) or (B and (so.dtype.kind not in 'iu' or do.dtype.kind not in 'iu')):
        raise ValueError('wave_gather: src_off and dst_off must hold %d integers each' % B)
    for name, t in (('src', src), ('dst', dst)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('wave_gather: %s must be a contiguous 1-D float32 GPU tensor (got %s)' % (name, _got(t)))
    if src.device != dst.device or src.data_ptr() == dst.data_ptr():
        raise ValueError('wave_gather: src and dst must be two different buffers on one device')
    if B == 0:
        return dst
    so, do = np.ascontiguousarray(so, dtype=np.int64), np.ascontiguousarray(do, dtype=np.int64)
    la = np.ascontiguousarray(la, dtype=np.int32)
    if (so < 0).any() or (so + la > src.numel()).any() or (do < 0).any() or (do + la > dst.numel()).any():
        raise ValueError('wave_gather: a span lies outside its buffer (src %d samples, dst %d; src_off %s, dst_off %s, lens %s)'
                         % (src.numel(), dst.numel(), so.tolist(), do.tolist(), la.tolist()))
    lib = _lib.load()
    check(lib.st_wave_gather(_p(src), src.numel(), so.ctypes.data, _p(dst), dst.numel(), do.ctypes.data, la.ctypes.data, B, stream_handle()),
          'st_wave_gather')
    return dst


# (last: ops.py imports this module at its own end, and either of the two may be the first to be imported)
from .ops import _p, stream_handle  # noqa: E402
