"""Transcripts from CTC posteriors: prefix beam search on the device (st_ctc_beam_search, semi_tts_amd/csrc/ctc_decode.hip).

    from semi_tts_amd.ctc_decode import beam_search
    hyp, hyp_len, score = beam_search(p_code, lengths, beam_width=16, top_paths=4)      # VQVAE.speech_to_text's posteriors
    hyp, hyp_len, score = beam_search(post, lengths, log_input=True)                      # ASRPostnet's log-posteriors
    hyp, hyp_len, score = beam_search(p_code, lengths, lm='phn.2gram.npy', lm_weight=0.5, ins_bonus=0.2)   # with a phone n-gram

Blank = 0 and eps = 1e-10 are the conventions of the trainer's CTC loss (compute_ctcloss, bin/train_vqvae.py:430-444): the search scores
log(prob + eps).  The reference names this mode (main.py --asr-decode) but its bin/asr_decode.py is absent.  With `lm`, a dense n-gram
table in the reference's NgramPrior layout (semi_tts_amd/ngram.py), every extension of a prefix by symbol c also scores
lm_weight * log(P(c | context) + 1e-10) + ins_bonus inside the kernel's candidate scoring (st_ctc_beam_search_lm), so the table decides
which candidates survive each frame; neural, word-level and back-off models are not part of it.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import ngram, toolops

_BONUS_CACHE = OrderedDict()        # (table identity, weight, ins_bonus, device) -> (the table object, its fused device tensor)
_BONUS_CACHE_SIZE = 8


def fused_bonus(lm, lm_weight=0.5, ins_bonus=0.0, device=None, V=None):
    """the device tensor st_ctc_beam_search_lm adds from: ngram.fusion_table(lm, lm_weight, ins_bonus) on `device`, built once per distinct
    (lm, lm_weight, ins_bonus, device) and kept.  lm: a probability table (V^(order-1), V) as a numpy array, a torch tensor, or the path
    of a .npy file (ngram.load_table; a file is read again when its modification time changes).  An array is identified by the object: one
    changed in place after its first use must be passed as a new object.  V: the width the table must have (None: any)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(lm, (str, os.PathLike)):
        path = os.path.abspath(os.fspath(lm))
        try:
            ident = ('file', path, os.stat(path).st_mtime_ns)
        except OSError as e:
            raise ValueError('%s: cannot read the n-gram table (%s)' % (path, e))
    elif isinstance(lm, np.ndarray) or torch.is_tensor(lm):
        ident = ('object', id(lm))
    else:
        raise ValueError('beam_search: lm must be a numpy array, a torch tensor or a path (got %s)' % type(lm).__name__)
    key = (ident, float(lm_weight), float(ins_bonus), str(device))
    hit = _BONUS_CACHE.get(key)
    if hit is None:
        table = ngram.load_table(lm) if ident[0] == 'file' else (lm.detach().cpu().numpy() if torch.is_tensor(lm) else lm)
        host = ngram.fusion_table(table, lm_weight, ins_bonus)
        if V is not None and host.shape[1] != V:
            raise ValueError('beam_search: the n-gram table has %d classes, the posteriors %d' % (host.shape[1], V))
        hit = (lm, torch.from_numpy(host).to(device))              # (lm is kept so that its id stays its own)
        _BONUS_CACHE[key] = hit
        while len(_BONUS_CACHE) > _BONUS_CACHE_SIZE:
            _BONUS_CACHE.popitem(last=False)
    else:
        _BONUS_CACHE.move_to_end(key)
    if V is not None and hit[1].shape[1] != V:
        raise ValueError('beam_search: the n-gram table has %d classes, the posteriors %d' % (hit[1].shape[1], V))
    return hit[1]


def beam_search(prob, lengths=None, beam_width=16, top_paths=1, blank=0, log_input=False, eps=1e-10, lm=None, lm_weight=0.5,
                ins_bonus=0.0, bos=1, bonus=None):
    """prob (B, T, V) float32 posteriors (log-posteriors with log_input) on one GPU; lengths: valid frames per utterance (None: all T).
    -> (hyp (B, top_paths, T) int64 label ids 0-padded, hyp_len (B, top_paths) int32, score (B, top_paths) float32 natural-log prefix
    probabilities), device tensors, best first.  One launch, no host read; bad arguments raise ValueError before the device is touched.
    lm: None (the acoustic search), or an n-gram probability table (fused_bonus: array, tensor or .npy path) fused with lm_weight and
    ins_bonus; bos: the start id of the empty prefix's context.  bonus: instead of lm, a fused table already on the device
    (toolops.ctc_beam_search).  With either, score is the fused score: the log prefix probability plus the bonuses of the prefix's symbols."""
    if lm is not None and bonus is not None:
        raise ValueError('beam_search: lm and bonus are two ways to give one table; pass one of them')
    if lm is not None:
        if not torch.is_tensor(prob) or not prob.is_cuda or prob.dim() != 3:
            raise ValueError('beam_search: prob must be a (B, T, V) float32 GPU tensor')
        bonus = fused_bonus(lm, lm_weight, ins_bonus, prob.device, prob.shape[2])
    if bonus is None:
        return toolops.ctc_beam_search(prob, lengths, beam_width, top_paths, blank, log_input, eps)
    return toolops.ctc_beam_search(prob, lengths, beam_width, top_paths, blank, log_input, eps, bonus=bonus, bos=bos)
