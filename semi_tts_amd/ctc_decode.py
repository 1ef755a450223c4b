"""Transcripts from CTC posteriors: prefix beam search on the device (st_ctc_beam_search, semi_tts_amd/csrc/ctc_decode.hip).

    from semi_tts_amd.ctc_decode import beam_search
    hyp, hyp_len, score = beam_search(p_code, lengths, beam_width=16, top_paths=4)      # VQVAE.speech_to_text's posteriors
    hyp, hyp_len, score = beam_search(post, lengths, log_input=True)                      # ASRPostnet's log-posteriors

Blank = 0 and eps = 1e-10 are the conventions of the trainer's CTC loss (compute_ctcloss, bin/train_vqvae.py:430-444): the search scores
log(prob + eps).  The reference names this mode (main.py --asr-decode) but its bin/asr_decode.py is absent; LM fusion is not part of it.
"""
from . import ops


def beam_search(prob, lengths=None, beam_width=16, top_paths=1, blank=0, log_input=False, eps=1e-10):
    """prob (B, T, V) float32 posteriors (log-posteriors with log_input) on one GPU; lengths: valid frames per utterance (None: all T).
    -> (hyp (B, top_paths, T) int64 label ids 0-padded, hyp_len (B, top_paths) int32, score (B, top_paths) float32 natural-log prefix
    probabilities), device tensors, best first.  One launch, no host read; bad arguments raise ValueError before the device is touched."""
    return ops.ctc_beam_search(prob, lengths, beam_width, top_paths, blank, log_input, eps)
