"""Phone error rate of greedy CTC transcripts on the device (ref: src/util.py:169-181, cal_per).

The reference copies the argmax to the host and runs a Python loop and the C `editdistance` package per
utterance.  Here one HIP launch per batch (st_ctc_greedy_edit_distance) gives every utterance's edit distance
and reference length as device tensors; nothing is read back until somebody asks for a Python number.

    from semi_tts_amd.metrics import cal_per        # replaces `from src.util import cal_per` (bin/train_vqvae.py:11)

Mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW), the objective distance between a synthesised utterance and the
recording it imitates (the reference has no such measure): `dtw` warps two feature sequences of differing lengths onto each other in
one HIP launch per batch (st_dtw_batch, semi_tts_amd/csrc/dtw.hip), `mcd` is the metric on the project's MFCC.

    from semi_tts_amd.metrics import mcd
    mcd_db, path_len, path = mcd(conv.extract_mfcc_batch(syn), syn_frames, conv.extract_mfcc_batch(ref), ref_frames)

Where a synthesised utterance ends, read off the decoder's attention (the model has no trained stop gate), with the alignment diagnostics
of the same pass: `attention_endpoints`, one HIP launch per batch (st_attn_endpoint, semi_tts_amd/csrc/attn_stats.hip).

    from semi_tts_amd.metrics import attention_endpoints
    mel, linear, align, enc_len = model.synthesise(transcripts, sid)
    ep = attention_endpoints(align, enc_len)        # ep.end[b] decoder steps = r * ep.end[b] frames

Pitch along the same warp: F0 RMSE in cents, voicing error and gross pitch error of two F0 tracks (AudioConverter.extract_f0_batch, the
YIN tracker st_f0_yin) over the frame pairs of the path `mcd` returned: `f0_scores`, one HIP launch per batch (st_f0_path_scores,
semi_tts_amd/csrc/f0.hip).

    from semi_tts_amd.metrics import f0_scores
    s = f0_scores(conv.extract_f0_batch(syn), conv.extract_f0_batch(ref), path, path_len)     # s['f0_rmse_cents'][b], s['vuv_error'][b]

Intelligibility of a waveform against the time-aligned recording it was made from (a vocoder's output, a resampled or gain-changed
file): `stoi`, STOI and ESTOI from short-time third-octave envelopes (st_stoi_batch, semi_tts_amd/csrc/stoi.hip).  Not for
free-running synthesis, whose timing is the model's own: `mcd` along the warp is the measure there.

    from semi_tts_amd.metrics import stoi
    r = stoi(recordings, vocoded, 22050)            # r.score[b] = (STOI, ESTOI), r.counts[b] = (frames, kept, band frames, segments)

Pairs that are shifted against each other (a codec, another vocoder, a file cut elsewhere): `delay`, the integer delay by an exact float64
cross-correlation (st_xcorr_delay, semi_tts_amd/csrc/xcorr.hip); `align_pairs`, both sides cut to the overlap in the layout `stoi` takes;
`si_sdr`, SI-SDR / SNR / gain on the overlap (st_sisdr_batch).

    from semi_tts_amd.metrics import align_pairs, si_sdr, stoi
    ref, deg, d, coef = align_pairs(recordings, decoded, max_lag=1102)      # +-50 ms at 22050 Hz; d[b] > 0: decoded[b] is late
    r = stoi(ref, deg, 22050)
    s = si_sdr(recordings, decoded, d)              # s.score[b] = (SI-SDR dB, SNR dB, gain dB)
"""
import collections
import math

import torch

from . import toolops

# <pad>, <space>, <eos> and id 42, exactly as src/util.py:16.  Id 42 is the last phoneme of the reference's 43-entry vocabulary
# (data/cmu_phn.vocab), not a special token: the reference drops it from both transcripts all the same, and so does this module,
# so that the numbers agree with the reference's.
IGNORE_INDICES = (0, 1, 2, 42)

# dB of mel-cepstral distortion per unit of Euclidean distance between two rows of the project's MFCC (columns 1 .. n_cep - 1): see mcd
MCD_SCALE = 50.0 * math.sqrt(2.0)


def _on_device(pred, truth):
    """both on one GPU: a host tensor (what the reference's loop passes after .cpu()) goes to the other one's device, or the current one"""
    dev = pred.device if pred.is_cuda else truth.device if truth.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return pred.to(dev), truth.to(dev)


def edit_distances(pred, truth, ignore=IGNORE_INDICES):
    """-> (dist, ref_len): int32 (B,) device tensors, no host read.  pred: (B, T, V) float32 posteriors or log-posteriors (the greedy
    transcript is their argmax over V), or (B, T) int64 ids already argmaxed -- cal_per accepts both (`len(pred.shape) >= 3`).
    truth: (B, L) int64 transcripts.  dist[b] = edit distance between the collapsed, filtered argmax and truth[b] without the
    ignored ids; ref_len[b] = the length of the latter."""
    pred, truth = _on_device(pred, truth)
    return toolops.ctc_greedy_edit_distance(pred, truth, ignore)


def per_sum(pred, truth, ignore=IGNORE_INDICES):
    """sum over the batch of dist / ref_len as a float64 device scalar (no host read).  An utterance whose transcript is empty once the
    ignored ids are gone (ref_len == 0) makes the sum NaN -- the reference raises ZeroDivisionError there."""
    return _rate_sum(*edit_distances(pred, truth, ignore))


def _rate_sum(dist, ref_len):
    d, n = dist.to(torch.float64), ref_len.to(torch.float64)
    rate = torch.where(ref_len > 0, d / n.clamp_min(1.0), torch.full_like(d, math.nan))
    return rate.sum()


def beam_per_sum(prob, truth, beam_width, lengths=None, ignore=IGNORE_INDICES, log_input=False, lm=None, lm_weight=0.5, ins_bonus=0.0):
    """per_sum of the top-1 CTC prefix beam search transcripts (ctc_decode.beam_search, blank 0) instead of the greedy ones: prob
    (B, T, V) float32 posteriors (log-posteriors with log_input), truth (B, L) int64, lengths the valid frames per utterance (None: all).
    The hypotheses are already collapsed, so the distance does not merge runs (st_hyp_edit_distance).  lm, lm_weight, ins_bonus: the
    n-gram fusion of ctc_decode.beam_search (None: the acoustic search).  cal_per and the trainer's validation stay greedy, as the
    reference's are."""
    from .ctc_decode import beam_search
    prob, truth = _on_device(prob, truth)
    hyp, hyp_len, _ = beam_search(prob, lengths, beam_width, 1, log_input=log_input, lm=lm, lm_weight=lm_weight, ins_bonus=ins_bonus)
    return _rate_sum(*toolops.hyp_edit_distance(hyp[:, 0], hyp_len[:, 0], truth, ignore))


def cal_per(pred, truth):
    """drop-in for src/util.py:cal_per: the mean phone error rate of the batch as a Python float (one host read); None gives nan"""
    if pred is None:
        return math.nan
    return float(per_sum(pred, truth)) / pred.shape[0]


def dtw(x, y, x_len=None, y_len=None, cols=None, scale=1.0, want_path=True):
    """Dynamic time warping of B pairs of feature sequences on one GPU: x (B, Tx, D) against y (B, Ty, D), float32, of x_len / y_len
    valid rows each (None: all; a host sequence is checked, a device tensor is clamped by the kernel).  The frame distance is
    d(i, j) = scale * ||x[i, d0:d1] - y[j, d0:d1]||_2 with cols = (d0, d1) (None: all D columns, at most 64); the accumulated cost is
    D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) with D(0, 0) = d(0, 0) -- the unweighted symmetric step pattern, the
    default of librosa.sequence.dtw -- and a tie goes to the diagonal, then to (i-1, j), then to (i, j-1).
    -> (total (B,) float32 = D(n-1, m-1), path_len (B,) int32, path (B, Tx + Ty - 1, 2) int32: the cells (i, j) of the optimal path
    from (0, 0) to (n-1, m-1), -1 past path_len; None when want_path is false), device tensors.  An empty side or a NaN among the
    compared values gives total NaN, path_len 0 and a path of -1.  A pair's result depends on that pair alone and is bitwise
    repeatable.  One launch, no host read; bad arguments raise ValueError before the device is touched."""
    return toolops.dtw(x, y, x_len, y_len, cols, scale, want_path)


def mcd(mfcc_x, x_len, mfcc_y, y_len, n_cep=13):
    """Mel-cepstral distortion along the DTW path, in dB per aligned frame pair: mfcc_x (B, Tx, >= n_cep) and mfcc_y (B, Ty, >= n_cep)
    as AudioConverter.extract_mfcc_batch gives them (cepstra in the first 13 columns), x_len / y_len their frame counts (as in dtw).
    -> (mcd_db (B,) float32 = total / path_len of dtw over the columns [1, n_cep) at scale MCD_SCALE, path_len (B,) int32, path).

    Why 50 sqrt(2).  The usual definition is MCD = (10 / ln 10) sqrt(2 sum_{k >= 1} (c_k - c'_k)^2) on cepstra of the natural-log
    spectrum.  The project's MFCC is the orthonormal DCT of the normalised mel n = (20 log10 a + 80) / 100 of the mel amplitude a, so
    ln a = 5 ln 10 * n + const, and the constant falls out of every coefficient k >= 1 (the DCT rows past the first sum to zero).  The
    DCT is linear: a difference of natural-log cepstra is 5 ln 10 times the difference of the project's, and
    (10 / ln 10) sqrt(2 sum_{k >= 1} dc_ln^2) = (10 / ln 10) * sqrt(2) * 5 ln 10 * ||dc_n|| = 50 sqrt(2) ||dc_n||.

    Two caveats.  Where the normalisation clamps n into [0, 1] (mel levels below -80 dB or above +20 dB) the clamped value is what is
    compared.  And the orthonormal scaling of the DCT makes the figure comparable within this project -- between checkpoints, vocoder
    settings, Griffin-Lim iteration counts -- not with MCD tables computed from SPTK mel-cepstra.
    An empty utterance or a NaN among the cepstra gives NaN."""
    n_cep = int(n_cep)
    toolops._dtw_side('mfcc_x', mfcc_x)
    toolops._dtw_side('mfcc_y', mfcc_y)
    width = min(mfcc_x.shape[2], mfcc_y.shape[2])
    if not 2 <= n_cep <= width:
        raise ValueError('mcd: n_cep = %d: at least 2 (the 0th coefficient is left out) and at most the %d columns given' % (n_cep, width))
    total, path_len, path = toolops.dtw(mfcc_x, mfcc_y, x_len, y_len, (1, n_cep), MCD_SCALE, True)
    return total / path_len.to(torch.float32), path_len, path


AttentionEndpoints = collections.namedtuple('AttentionEndpoints', 'end reached n_back n_skip covered nonfinite focus peak dur')


def attention_endpoints(align, enc_len, patience=3, max_jump=4):
    """End of speech and alignment diagnostics from the attention of a free-running decode: align (B, S, L) float32 on one GPU (a
    sliced view with unit stride in L is read where it lies, as VQVAE.text_to_speech returns one), enc_len the real phones n of every
    utterance (a list, an array or a device tensor; the appended index 0 at position n and the batch padding are not counted).
    The peak of step t is the lowest column among the maxima of align[b, t, :] over all L columns (NaN never wins; 0 for a row of
    NaN).  The utterance ends after the first `patience` consecutive steps whose peak is at or past the last phone n - 1:
    end = t0 + patience, reached = 1; without such a run end = S, reached = 0.  Over the steps [0, end): focus = the mean peak weight,
    n_back = steps whose peak lies before the previous one, n_skip = steps whose peak lies more than max_jump phones past it,
    dur[j] = steps whose peak is column j, covered = real phones with dur > 0.  nonfinite = 1 when align holds a NaN or an infinity.
    -> AttentionEndpoints(end, reached, n_back, n_skip, covered, nonfinite: (B,) int32; focus (B,) float32; peak (B, S) int32;
    dur (B, L) int32), device tensors.  An utterance's result depends on it alone and is bitwise repeatable.  One launch, no host
    read; bad arguments raise ValueError before the device is touched."""
    stats, focus, peak, dur = toolops.attn_endpoint(align, enc_len, patience, max_jump)
    return AttentionEndpoints(*stats.unbind(1), focus, peak, dur)


def f0_scores(f0_x, f0_y, path, path_len):
    """Pitch figures of B pairs of F0 tracks along a warp: f0_x (B, Tx), f0_y (B, Ty) float32 in Hz as AudioConverter.extract_f0_batch
    gives them (0 or NaN: unvoiced), path (B, Tx + Ty - 1, 2) and path_len (B,) as `dtw` / `mcd` return them for sequences of Tx and Ty
    frames -- the path MUST come from there: its entries index the tracks unchecked.  Over the path_len frame pairs (i, j) of a pair:
      n_pairs, n_both (both frames voiced), n_vuv (one voiced, one not), n_gross (both voiced and |fx - fy| > 0.2 fy): int32;
      f0_rmse_cents = sqrt(sum c^2 / n_both), mean_cents = sum c / n_both with c = 1200 log2(fx / fy), NaN where n_both = 0;
      vuv_error = n_vuv / n_pairs, gross_error = n_gross / n_both (NaN where the denominator is 0).
    -> a dict of (B,) device tensors (the four counts, the four figures, and sum_sq_cents / sum_cents as the kernel summed them).
    One launch and a few element-wise divisions on the device; no host read.  Bitwise repeatable."""
    counts, sums = toolops.f0_path_scores(f0_x, f0_y, path, path_len)
    n_pairs, n_both, n_vuv, n_gross = counts.unbind(1)
    nan = torch.full_like(sums[:, 0], math.nan)
    both, pairs = n_both.to(torch.float32), n_pairs.to(torch.float32)
    some, any_pair = n_both > 0, n_pairs > 0
    return {'n_pairs': n_pairs, 'n_both': n_both, 'n_vuv': n_vuv, 'n_gross': n_gross, 'sum_sq_cents': sums[:, 0], 'sum_cents': sums[:, 1],
            'f0_rmse_cents': torch.where(some, torch.sqrt(sums[:, 0] / both.clamp_min(1.0)), nan),
            'mean_cents': torch.where(some, sums[:, 1] / both.clamp_min(1.0), nan),
            'vuv_error': torch.where(any_pair, n_vuv.to(torch.float32) / pairs.clamp_min(1.0), nan),
            'gross_error': torch.where(some, n_gross.to(torch.float32) / both.clamp_min(1.0), nan)}


TranscriptAlignment = collections.namedtuple('TranscriptAlignment', 'correct sub dele ins dist ref_len hyp_len ali_len ali confusion')


def align_transcripts(hyp, hyp_len, ref, ref_len=None, ignore=IGNORE_INDICES, n_classes=None, confusion=None, want_ali=True):
    """Phone-error breakdown of transcripts on one GPU: hyp (B, Lh) int64, or (B, N, Lh) for N paths per utterance (already collapsed,
    as ctc_decode.beam_search gives them), of hyp_len (B,) / (B, N) tokens, against ref (B, Lr) int64 of ref_len (B,) tokens (None: all
    Lr).  A host sequence of lengths is checked against [0, L], a device tensor is clamped by the kernel.  The ids in `ignore` are
    dropped from both sides wherever they sit (cal_per's filter by default); r[0 .. n) is the filtered reference and h[0 .. m) the
    filtered hypothesis.

    Definition.  D(i, 0) = i, D(0, j) = j, D(i, j) = min(D(i-1, j-1) + [r_i != h_j], D(i-1, j) + 1, D(i, j-1) + 1).  The alignment is
    the trace-back from (n, m): at (i, j) with i, j > 0 the diagonal if D(i-1, j-1) + [r_i != h_j] = D(i, j), otherwise the deletion
    (i-1, j) if D(i-1, j) + 1 = D(i, j), otherwise the insertion (i, j-1); on the border only one move exists.  This is the tie order
    of `dtw` -- diagonal, then (i-1, j), then (i, j-1) -- and fixes one alignment among the optimal ones.

    -> TranscriptAlignment of device tensors, (B,) or (B, N) like hyp_len: correct, sub, dele, ins (int32; dist = sub + dele + ins,
    ref_len = correct + sub + dele = n, hyp_len = correct + sub + ins = m, ali_len = their sum); ali (..., Lr + Lh, 2) int32, the
    aligned pairs in forward order as (reference token, hypothesis token) with -1 for a gap and (-1, -1) past ali_len (None when
    want_ali is false); confusion (V + 1, V + 1) int32 or None.
    The confusion matrix counts path 0 of every utterance: [r, h] a correct or substituted pair, [r, V] a deletion, [V, h] an
    insertion; a pair with a token outside [0, V) is counted in correct / sub / dele / ins but touches no cell.  With `confusion`
    given, that tensor is added into and returned (V = its size - 1), so a corpus keeps one matrix on the device and reads it once;
    with n_classes = V alone a zeroed matrix is made; with neither, none is kept.
    One launch (st_edit_align), no host read; integers only, bitwise repeatable; bad arguments raise ValueError before the device is
    touched."""
    if not torch.is_tensor(hyp) or hyp.dim() not in (2, 3):
        raise ValueError('align_transcripts: hyp must be a (B, Lh) or (B, N, Lh) tensor (got %s)'
                         % (tuple(hyp.shape) if torch.is_tensor(hyp) else type(hyp).__name__))
    single = hyp.dim() == 2
    if single:
        hyp = hyp.unsqueeze(1)
        if torch.is_tensor(hyp_len):
            hyp_len = hyp_len.unsqueeze(1) if hyp_len.dim() == 1 else hyp_len
        else:
            hyp_len = [[v] for v in hyp_len]
    if confusion is not None and n_classes is None and torch.is_tensor(confusion) and confusion.dim() == 2:
        n_classes = confusion.shape[0] - 1
    if confusion is None and n_classes is not None:
        confusion = True            # (a zeroed matrix, made once the arguments have passed their checks)
    counts, ali_len, ali, confusion = toolops.edit_align(hyp, hyp_len, ref, ref_len, ignore, 1 if n_classes is None else n_classes, confusion,
                                                         want_ali)
    if single:
        counts, ali_len = counts[:, 0], ali_len[:, 0]
        ali = None if ali is None else ali[:, 0]
    c, s, d, i = counts.unbind(-1)
    return TranscriptAlignment(c, s, d, i, s + d + i, c + s + d, c + s + i, ali_len, ali, confusion)


NBest = collections.namedtuple('NBest', 'dist path')


def nbest_per(dist):
    """The n-best "oracle" of align_transcripts(...).dist (B, N): per utterance the lowest distance over the N paths and the lowest
    path index k that attains it -> NBest(dist (B,) int32, path (B,) int64), device tensors, no host read."""
    if not torch.is_tensor(dist) or dist.dim() != 2 or dist.shape[1] < 1:
        raise ValueError('nbest_per: dist must be a (B, N) tensor with N >= 1')
    best = dist.min(dim=1).values
    N = dist.shape[1]
    k = torch.arange(N, device=dist.device).expand_as(dist)
    path = torch.where(dist == best.unsqueeze(1), k, torch.full_like(k, N)).min(dim=1).values
    return NBest(best, path)


def _abx_table(what, name, v, dev):
    """an item / pair table as a contiguous int32 tensor on dev: a device tensor is taken as it is, host integers are copied over"""
    if torch.is_tensor(v) and v.is_cuda:
        return v
    import numpy as np
    host = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    if host.ndim != 1 or host.dtype.kind not in 'iu' or (host.size and (host.min() < -2 ** 31 or host.max() >= 2 ** 31)):
        raise ValueError('%s: %s must be a 1-d sequence of int32 integers (got %s %s)' % (what, name, host.shape, host.dtype))
    return torch.from_numpy(host.astype(np.int32)).to(dev)


def dtw_pairs(feat, item_start, item_len, pair_a, pair_b, metric='angular', want_cost=False, max_len=None):
    """Path-normalised DTW distances of many pairs of short items of one packed feature buffer, one launch (st_dtw_pairs,
    semi_tts_amd/csrc/abx.hip): feat (n_rows, D) float32 on one GPU; item q is the rows [item_start[q], item_start[q] + item_len[q]),
    1 .. 64 of them; pair p compares item pair_a[p] with item pair_b[p].  The tables are int32 device tensors, or host integer
    sequences (copied over).  metric: 'angular' (the angle between the frames over pi, formed as 2 atan2(|u - v|, |u + v|) / pi of the
    unit vectors, in [0, 1]), 'kl' (the symmetrised KL divergence of probability rows) or 'euclid'; the recurrence and the tie rule are dtw's, the path
    length is carried beside the cost and dist = cost / path_len, the DTW of ABXpy and Libri-light's ABX evaluation.
    max_len sizes the kernel's LDS: None takes the longest item of a host item_len and 64 for a device tensor.
    -> dist (P,) float32, or (dist, cost, path_len) with want_cost: device tensors.  A pair with a bad index, an item outside
    [1, max_len] rows or outside feat, or a NaN among its rows gets NaN (path_len 0).  Bad arguments raise ValueError before the
    device is touched."""
    if not torch.is_tensor(feat) or not feat.is_cuda:
        raise ValueError('dtw_pairs: feat must be a (n_rows, D) float32 GPU tensor (got %s)' % (type(feat).__name__ if not torch.is_tensor(feat) else feat.device))
    if max_len is None:
        max_len = toolops.ABX_MAX_LEN
        if not (torch.is_tensor(item_len) and item_len.is_cuda) and len(item_len):
            max_len = min(max(int(max(int(v) for v in item_len)), 1), toolops.ABX_MAX_LEN)
    tabs = [_abx_table('dtw_pairs', n, v, feat.device) for n, v in (('item_start', item_start), ('item_len', item_len), ('pair_a', pair_a), ('pair_b', pair_b))]
    return toolops.dtw_pairs(feat, tabs[0], tabs[1], tabs[2], tabs[3], metric, max_len, want_cost)


AbxResult = collections.namedtuple('AbxResult', 'blocks block_cell block_a block_b counts table score pairs keep')


def abx(feat, item_start, item_len, label, cell, metric='angular', max_items=50, seed=0):
    """ABX phone-discrimination error of the items of a packed feature buffer (see semi_tts_amd.abx for the terms): feat (n_rows, D)
    float32 on one GPU; item_start / item_len / label / cell host integer sequences, one entry per item (label: the phone, cell: the
    context within which items are compared).  A (cell, label) group above max_items is subsampled (abx.subsample, seeded).  Every
    unordered pair of a cell goes through dtw_pairs once (sorted by the first item), is mirrored into the cell's dense matrix by one
    indexed store, and st_abx_count counts, per ordered (a, b) of a cell, the triples X, A in a, B in b with d(A, X) > d(B, X) (wrong)
    and == (tied).  The counts are read once and aggregated on the host in float64 (abx.aggregate: block error
    (wrong + tied / 2) / (triples - nan), mean over cells, then over the ordered phone pairs).
    -> AbxResult(blocks (NB, 6), block_cell, block_a, block_b, counts (NB, 4) int64 numpy, table [(a, b, cells, triples, error)],
    score, pairs = the DTW pairs computed, keep = the items used).  Without a block: empty tables and score NaN."""
    import numpy as np
    from . import abx as A
    if not torch.is_tensor(feat) or not feat.is_cuda or feat.dim() != 2 or feat.dtype != torch.float32:
        raise ValueError('abx: feat must be a (n_rows, D) float32 GPU tensor')
    start, length = np.asarray(item_start, np.int64).reshape(-1), np.asarray(item_len, np.int64).reshape(-1)
    if not (len(start) == len(length) == len(label) == len(cell)):
        raise ValueError('abx: %d starts, %d lengths, %d labels, %d cells: one of each per item' % (len(start), len(length), len(label), len(cell)))
    pl = A.plan(label, cell, max_items, seed)
    if len(pl.blocks) == 0:
        return AbxResult(pl.blocks, pl.block_cell, pl.block_a, pl.block_b, np.zeros((0, 4), np.int64), [], float('nan'), 0, pl.keep)
    dev = feat.device
    max_len = int(min(max(length[pl.keep].max(), 1), toolops.ABX_MAX_LEN))
    tabs = torch.from_numpy(np.concatenate([start, length]).astype(np.int32)).to(dev)
    pairs = torch.from_numpy(np.concatenate([pl.pair_a, pl.pair_b])).to(dev)
    n, P = len(start), len(pl.pair_a)
    dist = toolops.dtw_pairs(feat, tabs[:n], tabs[n:], pairs[:P], pairs[P:], metric, max_len)
    dmat = torch.zeros(pl.dmat_len, device=dev, dtype=torch.float32)
    dmat[torch.from_numpy(np.concatenate([pl.pos_ab, pl.pos_ba])).to(dev)] = torch.cat([dist, dist])        # (the one mirrored store)
    counts = toolops.abx_count(dmat, torch.from_numpy(pl.blocks).to(dev)).cpu().numpy()                          # (the one host read)
    agg = A.aggregate(pl.block_a, pl.block_b, counts)
    return AbxResult(pl.blocks, pl.block_cell, pl.block_a, pl.block_b, counts, agg.table, agg.score, P, pl.keep)


AbxAcrossResult = collections.namedtuple('AbxAcrossResult', 'grp xr grp_context grp_speaker grp_a grp_b err counts table score speakers pairs keep')


def _abx_across_dmat(dist, pl, dev):
    """the contexts' matrices with the distances stored and mirrored by one indexed store; entries between items of one speaker (and the
    diagonal) are never written and never read"""
    import numpy as np
    dmat = torch.zeros(pl.dmat_len, device=dev, dtype=torch.float32)
    dmat[torch.from_numpy(np.concatenate([pl.pos_ab, pl.pos_ba])).to(dev)] = torch.cat([dist, dist])
    return dmat


def abx_across(feat, item_start, item_len, label, context, speaker, metric='angular', max_items=50, seed=0, max_bytes=8 << 30):
    """Across-speaker ABX phone-discrimination error (see semi_tts_amd.abx): as abx, but A and B are tokens of one speaker and X a
    token of phone a from ANOTHER speaker of the same context -- the figure that tells whether a representation still carries the
    speaker.  feat (n_rows, D) float32 on one GPU; item_start / item_len / label / context / speaker host integer sequences, one entry
    per item.  A (context, speaker, label) group above max_items is subsampled as abx does.  Every cross-speaker pair of a context
    goes through dtw_pairs once and is mirrored into the context's matrix by one indexed store; st_abx_across then forms, per group
    (context, speaker, a, b), the pair score (wrong + tied / 2) / (triples - nan) against every other speaker and their float64 mean in
    ascending speaker order.  err and counts are read once; abx.aggregate_across averages over (context, speaker), then over the ordered
    phone pairs: Libri-light's order.
    -> AbxAcrossResult(grp (NG, 8), xr (NX, 2), grp_context, grp_speaker, grp_a, grp_b, err (NG,) float64 numpy, counts (NG, 5) int64
    numpy, table [(a, b, groups, triples, error)], score, speakers [(speaker, groups, error)], pairs, keep).  Without a group: empty
    tables and score NaN.  ValueError before the device is touched for tables of different lengths, fewer than two speakers, and
    matrices and pair tables above max_bytes."""
    import numpy as np
    from . import abx as A
    if not torch.is_tensor(feat) or not feat.is_cuda or feat.dim() != 2 or feat.dtype != torch.float32:
        raise ValueError('abx_across: feat must be a (n_rows, D) float32 GPU tensor')
    start, length = np.asarray(item_start, np.int64).reshape(-1), np.asarray(item_len, np.int64).reshape(-1)
    if not (len(start) == len(length) == len(label) == len(context) == len(speaker)):
        raise ValueError('abx_across: %d starts, %d lengths, %d labels, %d contexts, %d speakers: one of each per item'
                         % (len(start), len(length), len(label), len(context), len(speaker)))
    if len(set(np.asarray(speaker).reshape(-1).tolist())) < 2:
        raise ValueError('abx_across: the items have fewer than two speakers: X has no other speaker to come from')
    pl = A.plan_across(label, context, speaker, max_items, seed, max_bytes)
    if len(pl.grp) == 0:
        return AbxAcrossResult(pl.grp, pl.xr, pl.grp_context, pl.grp_speaker, pl.grp_a, pl.grp_b, np.zeros(0), np.zeros((0, 5), np.int64), [],
                               float('nan'), [], 0, pl.keep)
    dev = feat.device
    max_len = int(min(max(length[pl.keep].max(), 1), toolops.ABX_MAX_LEN))
    tabs = torch.from_numpy(np.concatenate([start, length]).astype(np.int32)).to(dev)
    pairs = torch.from_numpy(np.concatenate([pl.pair_a, pl.pair_b])).to(dev)
    n, P = len(start), len(pl.pair_a)
    dist = toolops.dtw_pairs(feat, tabs[:n], tabs[n:], pairs[:P], pairs[P:], metric, max_len)
    dmat = _abx_across_dmat(dist, pl, dev)                                                                      # (the one mirrored store)
    err, counts = toolops.abx_across(dmat, torch.from_numpy(pl.grp).to(dev), torch.from_numpy(pl.xr).to(dev))
    both = torch.cat([err.view(torch.int64).unsqueeze(1), counts], 1).cpu().numpy()                             # (the one host read)
    err, counts = both[:, 0].copy().view(np.float64), np.ascontiguousarray(both[:, 1:])
    agg = A.aggregate_across(pl.grp_a, pl.grp_b, pl.grp_speaker, err, counts)
    return AbxAcrossResult(pl.grp, pl.xr, pl.grp_context, pl.grp_speaker, pl.grp_a, pl.grp_b, err, counts, agg.table, agg.score, agg.speakers, P,
                           pl.keep)


StoiResult = collections.namedtuple('StoiResult', 'score counts energy kept bands')


def _stoi_side(what, wavs, who='stoi'):
    """one side of metrics.stoi (or of `who`, the function the messages name) as a WaveBatch (nothing is uploaded here)"""
    from .audio import WaveBatch
    if isinstance(wavs, WaveBatch):
        return wavs
    if torch.is_tensor(wavs) and wavs.dim() == 1:
        wavs = [wavs]
    try:
        n = len(wavs)
    except TypeError:
        raise ValueError('%s: %s must be a list of 1-D waveforms or a WaveBatch (got %s)' % (who, what, type(wavs).__name__))
    if n == 0:
        raise ValueError('%s: %s is an empty batch' % (who, what))
    wavs = [torch.as_tensor(w) for w in wavs]
    for i, w in enumerate(wavs):
        if w.dim() != 1 or w.numel() < 1 or not (w.dtype.is_floating_point or w.dtype == torch.int16):
            raise ValueError('%s: %s[%d] must be a non-empty 1-D floating point or int16 waveform (got %s %s)' % (who, what, i, tuple(w.shape), w.dtype))
    return WaveBatch([w.to(torch.float32) / 32768.0 if w.dtype == torch.int16 else w for w in wavs])


def stoi(clean, degraded, sample_rate, want_parts=False):
    """Short-time objective intelligibility of B (clean, processed) waveform pairs on one GPU: STOI (Taal, Hendriks, Heusdens, Jensen
    2011) and ESTOI (Jensen, Taal 2016); the definition is in include/semitts.h (st_stoi_batch, semi_tts_amd/csrc/stoi.hip).  clean,
    degraded: lists of 1-D waveforms (tensors or arrays; int16 PCM counts as x / 32768) or WaveBatches, pairwise of EQUAL length and
    time-aligned -- the measure correlates short-time envelopes frame by frame and searches no delay itself: `align_pairs` finds a
    constant shift and returns the two overlaps in the form this function takes.  sample_rate: the rate
    of both sides; anything but 10000 Hz goes through audio.resample first (the project's Hann-windowed sinc, so the values differ
    slightly from pystoi's, which emulates Octave's resample).  More than toolops.STOI_MAX_BATCH pairs are issued in chunks of it.
    -> StoiResult of device tensors in the caller's order: score (B, 2) float32 = (STOI, ESTOI); counts (B, 4) int32 = (frames, kept
    frames, band frames M, segments S); with want_parts energy (B, F_pad), kept (B, F_pad) int32 (-1 past the kept ones) and bands
    (B, 2, 15, F_pad) (0 past M), else None.  A pair with S = 0 (shorter than 30 band frames) scores toolops.STOI_SENTINEL twice; a
    non-finite clean signal scores NaN.  A pair's figures depend on that pair alone and are bitwise repeatable.  No host read.
    Unequal lengths, an empty input, a rate the resampler refuses or a signal past toolops.STOI_MAX_LEN samples at 10 kHz raise ValueError
    before the device is touched."""
    import numpy as np
    from . import audio
    xb, yb = _stoi_side('clean', clean), _stoi_side('degraded', degraded)
    if len(xb.lens) != len(yb.lens):
        raise ValueError('stoi: %d clean and %d processed signals: one of each per pair' % (len(xb.lens), len(yb.lens)))
    ox, oy = np.asarray(xb.order), np.asarray(yb.order)
    lx, ly = np.empty_like(xb.lens), np.empty_like(yb.lens)
    lx[ox], ly[oy] = xb.lens, yb.lens                                   # (lengths in the caller's order)
    if (lx != ly).any():
        i = int(np.nonzero(lx != ly)[0][0])
        raise ValueError('stoi: pair %d has %d clean and %d processed samples: the two sides must be equally long' % (i, lx[i], ly[i]))
    if not np.array_equal(ox, oy):
        raise ValueError('stoi: the two WaveBatches are ordered differently')
    audio.resample_table(sample_rate, toolops.STOI_FS)                       # (the resampler's refusals, raised here)
    longest = audio.resampled_len(int(lx.max()), sample_rate, toolops.STOI_FS)
    if longest > toolops.STOI_MAX_LEN:
        raise ValueError('stoi: the longest signal has %d samples at %d Hz, above the limit of %d' % (longest, toolops.STOI_FS, toolops.STOI_MAX_LEN))
    if int(sample_rate) != toolops.STOI_FS:
        xb, yb = audio.resample(xb, int(sample_rate), toolops.STOI_FS), audio.resample(yb, int(sample_rate), toolops.STOI_FS)
    order, lens, off = np.asarray(xb.order), xb.lens, xb.offsets         # (equal lengths sort alike: yb's are the same)
    dev = xb.device or yb.device or audio._device()
    x, y = xb.packed(dev), yb.packed(dev)
    if not np.array_equal(off, yb.offsets) or x.numel() != y.numel():    # (two windows of differently laid out buffers)
        raise ValueError('stoi: the two WaveBatches are laid out differently')
    B = len(lens)
    F_pad = max(1, max(toolops.stoi_frames(v) for v in lens))             # one width for every chunk: the parts concatenate
    outs = [toolops.stoi_batch(x, y, off[b0:b0 + toolops.STOI_MAX_BATCH], lens[b0:b0 + toolops.STOI_MAX_BATCH], F_pad, want_parts)
            for b0 in range(0, B, toolops.STOI_MAX_BATCH)]
    inv = torch.from_numpy(xb.inverse()).to(dev)                         # row i of the result is the caller's pair i
    return StoiResult(*[torch.cat(parts).index_select(0, inv) if parts[0] is not None else None for parts in zip(*outs)])


DelayResult = collections.namedtuple('DelayResult', 'delay coef corr')
SiSdrResult = collections.namedtuple('SiSdrResult', 'score sums')


def _pair_sides(what, clean, degraded):
    """both sides of a batch of pairs whose lengths may differ -> (x buffer, y buffer, and in the CALLER's order the int64 arrays
    x offsets, x lengths, y offsets, y lengths).  Every refusal is raised before anything is uploaded."""
    import numpy as np
    xb, yb = _stoi_side('clean', clean, what), _stoi_side('degraded', degraded, what)
    if len(xb.lens) != len(yb.lens):
        raise ValueError('%s: %d clean and %d processed signals: one of each per pair' % (what, len(xb.lens), len(yb.lens)))
    longest = int(max(xb.lens.max(), yb.lens.max()))
    if longest > toolops.XCORR_MAX_LEN:
        raise ValueError('%s: the longest signal has %d samples, above the limit of %d' % (what, longest, toolops.XCORR_MAX_LEN))
    ix, iy = xb.inverse(), yb.inverse()
    return xb, yb, xb.offsets[ix], xb.lens[ix], yb.offsets[iy], yb.lens[iy]


def _check_lag(what, max_lag):
    import numpy as np
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= toolops.XCORR_MAX_LAG:
        raise ValueError('%s: max_lag must be an integer in [0, %d] (got %r)' % (what, toolops.XCORR_MAX_LAG, max_lag))
    return int(max_lag)


def delay(clean, degraded, max_lag, want_corr=False):
    """The integer delay of each of B (clean, processed) waveform pairs on one GPU: the lag in [-max_lag, max_lag] samples at which the
    plain cross-correlation r[d] = sum_n x[n] y[n + d] is largest (st_xcorr_delay, semi_tts_amd/csrc/xcorr.hip; the definition is in
    include/semitts.h).  A positive delay: the processed signal is late.  clean, degraded: lists of 1-D waveforms (tensors or arrays;
    int16 PCM counts as x / 32768) or WaveBatches; the two lengths of a pair may differ.  The search is in float64 and exact on 16-bit
    PCM input, so the decision has no tolerance there; ties go to the smallest |d|, then to the non-negative lag.  More than
    toolops.XCORR_MAX_BATCH pairs are issued in chunks of it.
    -> DelayResult of device tensors in the caller's order: delay (B,) int32; coef (B,) float32 = r[d*] / sqrt(sum x^2 sum y^2); corr
    (B, 2 max_lag + 1) float64 with want_corr (column d + max_lag), else None.  A NaN anywhere in r: delay 0, coef NaN.  A pair's
    figures depend on that pair alone and are bitwise repeatable.  No host read.  Every refusal raises ValueError before the device is
    touched."""
    D = _check_lag('delay', max_lag)
    from . import audio
    xb, yb, xo, xl, yo, yl = _pair_sides('delay', clean, degraded)
    dev = xb.device or yb.device or audio._device()
    x, y = xb.packed(dev), yb.packed(dev)
    M = toolops.XCORR_MAX_BATCH
    outs = [toolops.xcorr_delay(x, xo[b0:b0 + M], xl[b0:b0 + M], y, yo[b0:b0 + M], yl[b0:b0 + M], D, want_corr) for b0 in range(0, len(xl), M)]
    return DelayResult(*[torch.cat(parts) if parts[0] is not None else None for parts in zip(*outs)])


def si_sdr(clean, degraded, delay=None, zero_mean=True):
    """Scale-invariant signal-to-distortion ratio (Le Roux, Wisdom, Erdogan, Hershey 2019), SNR and gain of B waveform pairs on the
    overlap a delay leaves (st_sisdr_batch; the definition is in include/semitts.h).  clean, degraded as for `delay`.  delay: None (0),
    one int for every pair, or the device int32 tensor `delay(...)` returned (it stays on the device).  With d >= 0 the clean signal is
    scored from 0 and the processed one from d; with d < 0 the clean one from -d and the processed one from 0; n = the shorter remainder.
    zero_mean: the means over the overlap are removed first (the usual definition).
    -> SiSdrResult of device tensors in the caller's order: score (B, 3) float32 = (SI-SDR dB, SNR dB, gain dB); sums (B, 6) float64 =
    (n, sum x, sum y, sum x^2, sum y^2, sum x y), exact on 16-bit PCM input.  IEEE semantics: a scaled copy scores +inf without
    zero_mean, a silent reference NaN (SNR -inf), a delay longer than a side NaN with n = 0.  No host read.  Every refusal raises ValueError
    before the device is touched."""
    import numpy as np
    from . import audio
    xb, yb, xo, xl, yo, yl = _pair_sides('si_sdr', clean, degraded)
    B = len(xl)
    if delay is not None and not torch.is_tensor(delay):
        if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or not -2 ** 31 < delay < 2 ** 31:
            raise ValueError('si_sdr: delay must be None, an int or the device tensor metrics.delay returned (got %r)' % (delay,))
    elif delay is not None and not (delay.is_cuda and delay.dtype == torch.int32 and tuple(delay.shape) == (B,)):
        raise ValueError('si_sdr: a delay tensor must be int32 of shape (%d,) on the device (got %s %s on %s)'
                         % (B, tuple(delay.shape), delay.dtype, delay.device))
    dev = xb.device or yb.device or (delay.device if torch.is_tensor(delay) else None) or audio._device()
    x, y = xb.packed(dev), yb.packed(dev)
    if delay is not None:
        delay = delay.contiguous() if torch.is_tensor(delay) else torch.full((B,), int(delay), device=dev, dtype=torch.int32)
    M = toolops.XCORR_MAX_BATCH
    outs = [toolops.sisdr_batch(x, xo[b0:b0 + M], xl[b0:b0 + M], y, yo[b0:b0 + M], yl[b0:b0 + M], None if delay is None else delay[b0:b0 + M], zero_mean)
            for b0 in range(0, B, M)]
    return SiSdrResult(*[torch.cat(parts) for parts in zip(*outs)])


def overlap(lx, ly, d):
    """the span a delay d leaves of a pair of lx and ly samples -> (first clean sample, first processed sample, samples; <= 0: none)"""
    x0, y0 = max(0, -int(d)), max(0, int(d))
    return x0, y0, min(int(lx) - x0, int(ly) - y0)


def align_pairs(clean, degraded, max_lag):
    """Searches each pair's delay (`delay`) and cuts both sides to the overlap it leaves.  -> (clean', degraded', delay, coef): the two
    sides as WaveBatches over two NEW packed device buffers with one common layout and equal lengths -- what `stoi` accepts as it
    stands -- and the device tensors of `delay`, in the caller's order.  The cut lengths reorder the batch (a WaveBatch is sorted longest
    first); the order travels in the WaveBatches, so `stoi(clean', degraded', sr)` returns its rows in the caller's order.  One host
    read: the B delays.  The spans are copied by one st_wave_gather launch per side and 64 pairs.  A pair whose best lag leaves no
    overlap (possible only when max_lag reaches a signal's length) raises ValueError."""
    import numpy as np
    from . import audio
    D = _check_lag('align_pairs', max_lag)
    xb, yb, xo, xl, yo, yl = _pair_sides('align_pairs', clean, degraded)
    dev = xb.device or yb.device or audio._device()
    x, y = xb.packed(dev), yb.packed(dev)
    M, B = toolops.XCORR_MAX_BATCH, len(xl)
    outs = [toolops.xcorr_delay(x, xo[b0:b0 + M], xl[b0:b0 + M], y, yo[b0:b0 + M], yl[b0:b0 + M], D) for b0 in range(0, B, M)]
    dl, coef = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    d_host = dl.cpu().numpy()                                            # (the one host read)
    spans = [overlap(xl[i], yl[i], d_host[i]) for i in range(B)]
    for i, (_, _, n) in enumerate(spans):
        if n < 1:
            raise ValueError('align_pairs: pair %d: the best lag %d leaves no overlap of its %d and %d samples' % (i, d_host[i], xl[i], yl[i]))
    n = np.array([s[2] for s in spans], np.int64)
    order = np.argsort(-n, kind='stable')                                # longest overlap first; WaveBatch.from_packed is told this order
    off = np.empty(B, np.int64)
    off[order] = np.concatenate([[0], np.cumsum(n[order])[:-1]])         # (offsets in the caller's order)
    sides = []
    for buf, so in ((x, xo + np.array([s[0] for s in spans], np.int64)), (y, yo + np.array([s[1] for s in spans], np.int64))):
        out = torch.empty(int(n.sum()), device=dev, dtype=torch.float32)
        for b0 in range(0, B, M):
            toolops.wave_gather(buf, so[b0:b0 + M], out, off[b0:b0 + M], n[b0:b0 + M])
        sides.append(audio.WaveBatch.from_packed(out, n, order))
    return sides[0], sides[1], dl, coef


# k-means units (semi_tts_amd/kmeans.py): the baseline representation the measures above are compared on
from .kmeans import KMeansFit, fit as kmeans_fit, quantise  # noqa: E402,F401
