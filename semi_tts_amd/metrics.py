"""Phone error rate of greedy CTC transcripts on the device (ref: src/util.py:169-181, cal_per).

The reference copies the argmax to the host and runs a Python loop and the C `editdistance` package per
utterance.  Here one HIP launch per batch (st_ctc_greedy_edit_distance) gives every utterance's edit distance
and reference length as device tensors; nothing is read back until somebody asks for a Python number.

    from semi_tts_amd.metrics import cal_per        # replaces `from src.util import cal_per` (bin/train_vqvae.py:11)
"""
import math

import torch

from . import ops

# <pad>, <space>, <eos> and id 42, exactly as src/util.py:16.  Id 42 is the last phoneme of the reference's 43-entry vocabulary
# (data/cmu_phn.vocab), not a special token: the reference drops it from both transcripts all the same, and so does this module,
# so that the numbers agree with the reference's.
IGNORE_INDICES = (0, 1, 2, 42)


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
    return ops.ctc_greedy_edit_distance(pred, truth, ignore)


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
    return _rate_sum(*ops.hyp_edit_distance(hyp[:, 0], hyp_len[:, 0], truth, ignore))


def cal_per(pred, truth):
    """drop-in for src/util.py:cal_per: the mean phone error rate of the batch as a Python float (one host read); None gives nan"""
    if pred is None:
        return math.nan
    return float(per_sum(pred, truth)) / pred.shape[0]
