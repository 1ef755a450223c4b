"""When was each phone spoken: CTC forced alignment on the device (st_ctc_forced_align, semi_tts_amd/csrc/ctc_align.hip), and the file
formats of main.py --align-wav-dir.

    from semi_tts_amd.ctc_align import forced_align
    score, path, tok_start, tok_end = forced_align(p_code, text, lengths)                 # VQVAE.speech_to_text's posteriors
    score, path, tok_start, tok_end = forced_align(post, text, lengths, log_input=True)   # ASRPostnet's log-posteriors

Blank = 0 and eps = 1e-10 are the conventions of the trainer's CTC loss (compute_ctcloss, bin/train_vqvae.py:430-444): the aligner scores
log(prob + eps) over the targets that loss trains on (the non-blank entries of each row of text).  The reference has no aligner: its
AudioConverter reads phone boundaries "found by MFA" from a segment_file (src/audio.py:310-327); segment_row writes that layout.
"""
import os

from . import toolops

MAX_TOKENS = toolops.CA_MAX_L


def forced_align(prob, text, lengths=None, text_lengths=None, blank=0, log_input=False, eps=1e-10):
    """prob (B, T, V) float32 posteriors (log-posteriors with log_input) and text (B, L) int64 on one GPU; lengths / text_lengths: valid
    frames / transcript entries per utterance (None: all).  The most probable CTC alignment of each row's non-blank entries:
    -> (score (B,) float32 its natural-log probability, path (B, T) int32 the label of every frame (-1 past the length), tok_start,
    tok_end (B, L) int32 the frames [start, end) of every target token (-1 past the targets)), device tensors.  An utterance too short
    for its transcript scores -inf, one with a NaN posterior or a target outside [0, V) scores NaN; their path and spans are -1.
    One launch, no host read; bad arguments raise ValueError before the device is touched."""
    return toolops.ctc_forced_align(prob, text, lengths, text_lengths, blank, log_input, eps)


def read_phn(path, vocab=None):
    """the transcript of a .phn file as a list of ids: the tokens of its first non-empty line -- what follows the last TAB when the line
    holds one (the `score<TAB>tokens` lines of --transcribe-wav-dir), separated by blanks, each a symbol of `vocab` (a list indexed by id,
    solver.read_vocab) or a decimal id.  No tokens (or no such line) is a valid, empty transcript.  A file that cannot be read, an
    unknown symbol or more than 1024 tokens raises ValueError naming the file."""
    try:
        with open(path) as f:
            lines = f.read().splitlines()
    except (OSError, UnicodeDecodeError) as e:
        raise ValueError('%s: cannot read the transcript (%s)' % (path, e))
    line = next((ln for ln in lines if ln.strip(' \r\n') != ''), '')
    if '\t' in line:
        line = line.rsplit('\t', 1)[1]
    index = {s: i for i, s in reversed(list(enumerate(vocab)))} if vocab is not None else {}
    ids = []
    for tok in line.split():
        if tok in index:
            ids.append(index[tok])
        elif tok.isascii() and tok.isdigit():
            ids.append(int(tok))
        else:
            raise ValueError('%s: unknown symbol %r (not in the vocabulary, not a decimal id)' % (path, tok))
    if len(ids) > MAX_TOKENS:
        raise ValueError('%s: %d tokens, the aligner takes at most %d' % (path, len(ids), MAX_TOKENS))
    return ids


def read_phn_paths(path, vocab=None):
    """every transcript of a .phn file, in order, as a list of lists of ids: one per non-empty line, read as read_phn reads the first
    (line k is path k of --transcribe-wav-dir --top-paths N).  A line that holds a score and no tokens is an empty transcript; a file
    without a non-empty line gives one empty transcript.  The errors of read_phn, naming the file."""
    try:
        with open(path) as f:
            lines = f.read().splitlines()
    except (OSError, UnicodeDecodeError) as e:
        raise ValueError('%s: cannot read the transcript (%s)' % (path, e))
    index = {s: i for i, s in reversed(list(enumerate(vocab)))} if vocab is not None else {}
    paths = []
    for line in lines:
        if line.strip(' \r\n') == '':
            continue
        if '\t' in line:
            line = line.rsplit('\t', 1)[1]
        ids = []
        for tok in line.split():
            if tok in index:
                ids.append(index[tok])
            elif tok.isascii() and tok.isdigit():
                ids.append(int(tok))
            else:
                raise ValueError('%s: unknown symbol %r (not in the vocabulary, not a decimal id)' % (path, tok))
        if len(ids) > MAX_TOKENS:
            raise ValueError('%s: %d tokens, at most %d are read' % (path, len(ids), MAX_TOKENS))
        paths.append(ids)
    return paths or [[]]


def _symbol(i, vocab):
    return vocab[i] if vocab is not None and 0 <= i < len(vocab) else str(i)


def format_ali(score, frames, frame_s, tokens, starts, ends, vocab=None):
    """the text of one utterance's .ali file: `# score=<%.6f> frames=<T_enc> frame_s=<%.6f>`, then one line per target token
    `symbol<TAB>start_frame<TAB>end_frame<TAB>start_s<TAB>end_s` (x_s = x_frame * frame_s, %.6f).  An utterance without an alignment
    (score -inf or NaN) gets the header alone."""
    lines = ['# score=%.6f frames=%d frame_s=%.6f' % (score, frames, frame_s)]
    if score == score and score != float('-inf'):
        for tok, a, b in zip(tokens, starts, ends):
            lines.append('%s\t%d\t%d\t%.6f\t%.6f' % (_symbol(int(tok), vocab), a, b, a * frame_s, b * frame_s))
    return '\n'.join(lines) + '\n'


def segment_key(filename):
    """the key of a file in the reference's segment table: its name up to the first '.'"""
    return os.path.basename(filename).split('.')[0]


def segment_row(filename, starts, frames, frame_s):
    """one row `key,seg` of segments.csv in the reference's segment_file layout (pd.read_csv(index_col=0), column `seg` = boundary times
    joined by '_', the last one the total length; src/audio.py:326-327, 425-432): the start times of tokens 1 .. S-1, then the duration
    frames * frame_s (%.4f).  The blank frames after a token belong to it and the leading ones to the first token, so the S segments
    tile the utterance.  None for an utterance without tokens (nothing to segment)."""
    if len(starts) == 0:
        return None
    times = [a * frame_s for a in list(starts)[1:]] + [frames * frame_s]
    return '%s,%s' % (segment_key(filename), '_'.join('%.4f' % t for t in times))


SEGMENTS_HEADER = 'file,seg'
