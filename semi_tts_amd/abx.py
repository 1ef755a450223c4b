"""Host side of the ABX phone-discrimination error (standard library + numpy; nothing here touches a device).

The measure (Schatz et al. 2013; ZeroSpeech, Libri-light): take three phone tokens A, B and X of one context, A and X of one phone and B
of another; the error is how often X lies closer to B than to A, distances being path-normalised DTW over frame distances.  The
distances and the triple counts are the kernels' (st_dtw_pairs, st_abx_count through semi_tts_amd.metrics.abx); this module reads the
phone boundaries (.ali files as ctc_align.format_ali writes them), cuts them into items, keys them into cells, lays out the pair list
and the block table a launch works through, aggregates the counts and writes the tables.

    items   one phone token each: a run of rows of the packed feature buffer, a label (the phone) and a cell (the context)
    cell    the items that may be compared: same speaker and, with context 'triphone', same previous and next symbol
    block   an ordered pair of labels (a, b) of one cell with n_a >= 2 and n_b >= 1: the triples X, A in a (A != X), B in b

The across-speaker measure (plan_across, aggregate_across; st_abx_across through metrics.abx_across) takes A and B from one speaker and
X from another speaker of the same context:

    context the cell without its speaker: previous and next symbol with 'triphone', one for all with 'none'
    group   (context, speaker s, a, b): A in (s, a), B in (s, b), X in (s', a) for every other speaker s' of the context that has a
"""
import collections
import math
import os
import re

import numpy as np

MAX_ITEM_ROWS = 64                  # st_dtw_pairs' longest item
EDGE_LEFT, EDGE_RIGHT = '<s>', '</s>'       # the utterance's edge as a context symbol
ABX_HEADER = 'phone_a,phone_b,cells,triples,error'
PHONES_HEADER = 'phone,tokens,items,too_short,too_long'
CONTEXTS = ('triphone', 'none')

Ali = collections.namedtuple('Ali', 'frames frame_s symbols starts ends')
Plan = collections.namedtuple('Plan', 'keep pair_a pair_b pos_ab pos_ba dmat_len blocks block_cell block_a block_b')
Aggregate = collections.namedtuple('Aggregate', 'table score block_error')
ACROSS_HEADER = 'phone_a,phone_b,groups,triples,error'
ACROSS_SPEAKERS_HEADER = 'speaker,groups,error'
AcrossPlan = collections.namedtuple('AcrossPlan', 'keep pair_a pair_b pos_ab pos_ba dmat_len grp xr grp_context grp_speaker grp_a grp_b')
AggregateAcross = collections.namedtuple('AggregateAcross', 'table score speakers')


def read_ali(path):
    """one .ali file -> Ali(frames, frame_s, symbols, starts, ends).  ValueError naming the file for a missing or malformed header, a
    malformed line, frames out of order or outside [0, frames], or a file without tokens."""
    try:
        with open(path) as f:
            lines = [ln.rstrip('\n') for ln in f]
    except (OSError, UnicodeDecodeError) as e:
        raise ValueError('%s is not a readable .ali file (%s)' % (path, e))
    lines = [ln for ln in lines if ln.strip()]
    if not lines or not lines[0].startswith('#'):
        raise ValueError('%s: no `# ... frames=N frame_s=S` header' % path)
    fr, fs = re.search(r'\bframes=(\d+)\b', lines[0]), re.search(r'\bframe_s=([0-9.eE+-]+)', lines[0])
    try:
        frames, frame_s = int(fr.group(1)), float(fs.group(1))
    except (AttributeError, ValueError):
        raise ValueError('%s: the header needs frames=<integer> and frame_s=<seconds> (got %r)' % (path, lines[0]))
    if not (frames >= 1 and 0.0 < frame_s < float('inf')):
        raise ValueError('%s: frames=%d frame_s=%r: both must be positive' % (path, frames, frame_s))
    symbols, starts, ends = [], [], []
    for ln in lines[1:]:
        if ln.startswith('#'):
            continue
        p = ln.split('\t') if '\t' in ln else ln.split()
        try:
            sym, a, b = p[0].strip(), int(p[1]), int(p[2])
        except (IndexError, ValueError):
            raise ValueError('%s: malformed line %r (symbol, start_frame, end_frame, ...)' % (path, ln))
        if not sym or not 0 <= a <= b <= frames or (starts and a < starts[-1]):
            raise ValueError('%s: line %r: frames must satisfy 0 <= start <= end <= %d and starts must not decrease' % (path, ln, frames))
        symbols.append(sym)
        starts.append(a)
        ends.append(b)
    if not symbols:
        raise ValueError('%s has no tokens' % path)
    return Ali(frames, frame_s, symbols, starts, ends)


def frame_to_row(t, ali_frame_s, feat_frame_s, n_rows):
    """alignment frame t -> feature row: round(t ali_frame_s / feat_frame_s) (halves up), clipped into [0, n_rows]"""
    return min(max(int(math.floor(t * ali_frame_s / feat_frame_s + 0.5)), 0), int(n_rows))


def utterance_items(ali, feat_frame_s, n_rows, ignore=(), min_frames=1):
    """the items of one utterance.  Token k spans from its start_frame to the next token's start_frame, the last one to the utterance's
    frames (the token and its trailing blank frames, the tiling of segments.csv; leading blanks belong to no item); the span becomes the
    feature rows [frame_to_row(start), frame_to_row(end)).  A symbol of `ignore` is never an item but is still its neighbours' context.
    -> (items [(symbol, row, rows, previous symbol, next symbol)], stats {symbol: [tokens, items, too_short, too_long]})"""
    S = len(ali.symbols)
    items, stats = [], collections.OrderedDict()
    min_frames = max(int(min_frames), 1)
    for k, sym in enumerate(ali.symbols):
        if sym in ignore:
            continue
        st = stats.setdefault(sym, [0, 0, 0, 0])
        st[0] += 1
        end = ali.starts[k + 1] if k + 1 < S else ali.frames
        r0, r1 = (frame_to_row(t, ali.frame_s, feat_frame_s, n_rows) for t in (ali.starts[k], end))
        if r1 - r0 < min_frames:
            st[2] += 1
        elif r1 - r0 > MAX_ITEM_ROWS:
            st[3] += 1
        else:
            st[1] += 1
            items.append((sym, r0, r1 - r0, ali.symbols[k - 1] if k > 0 else EDGE_LEFT, ali.symbols[k + 1] if k + 1 < S else EDGE_RIGHT))
    return items, stats


def cell_key(speaker, prev, nxt, context='triphone'):
    """what two items must share to be compared: the speaker and, with context 'triphone', the previous and the next symbol"""
    if context not in CONTEXTS:
        raise ValueError('context %r is none of %s' % (context, CONTEXTS))
    return (speaker, prev, nxt) if context == 'triphone' else (speaker,)


def read_spk_map(path):
    """a `key,speaker` CSV (no header needed: a first line `key,speaker` or `file,speaker` is skipped) -> {key: speaker}"""
    out = {}
    with open(path) as f:
        for n, ln in enumerate(f):
            ln = ln.strip()
            if not ln or ln.startswith('#'):
                continue
            p = [c.strip() for c in ln.split(',')]
            if len(p) != 2 or not p[0] or not p[1]:
                raise ValueError('%s: line %d %r is not `key,speaker`' % (path, n + 1, ln))
            if n == 0 and p[1] == 'speaker':
                continue
            out[p[0]] = p[1]
    return out


def subsample(label, cell, max_items, seed):
    """the items kept, in plan order: sorted by cell, then by label, then by index; a (cell, label) group above max_items is cut to
    max_items of its members (in index order) drawn with numpy.random.RandomState(seed), the groups visited in that sorted order"""
    label, cell = np.asarray(label, np.int64).reshape(-1), np.asarray(cell, np.int64).reshape(-1)
    if label.shape != cell.shape:
        raise ValueError('abx: %d labels, %d cells: one of each per item' % (len(label), len(cell)))
    if isinstance(max_items, bool) or not isinstance(max_items, (int, np.integer)) or max_items < 1:
        raise ValueError('abx: max_items must be a positive integer (got %r)' % (max_items,))
    order = np.lexsort((np.arange(len(label)), label, cell))
    rs = np.random.RandomState(seed)
    keep, lo = [], 0
    key = np.stack([cell[order], label[order]], 1)
    while lo < len(order):
        hi = lo + 1
        while hi < len(order) and key[hi, 0] == key[lo, 0] and key[hi, 1] == key[lo, 1]:
            hi += 1
        g = order[lo:hi]
        if len(g) > max_items:
            g = g[np.sort(rs.choice(len(g), int(max_items), replace=False))]
        keep.append(g)
        lo = hi
    return np.concatenate(keep) if keep else np.zeros(0, np.int64)


def plan(label, cell, max_items=50, seed=0):
    """the work of one metrics.abx call.  keep: subsample().  A cell with at least one block gets a dense (n_c, n_c) matrix at
    mat_off in one flat buffer of dmat_len floats; every unordered pair i < j of its items (local indices, row-major: sorted by the
    first item) becomes one DTW pair, pair_a / pair_b indexing the caller's item tables, written to pos_ab = mat_off + i n_c + j and
    mirrored to pos_ba.  blocks (NB, 6) int64 = (mat_off, n_c, a_lo, a_hi, b_lo, b_hi) for every ordered (a, b), a != b, n_a >= 2,
    n_b >= 1, of every cell; block_cell / block_a / block_b name them."""
    label, cell = np.asarray(label, np.int64).reshape(-1), np.asarray(cell, np.int64).reshape(-1)
    keep = subsample(label, cell, max_items, seed)
    pa, pb, ab, ba, blocks, bc, bla, blb = [], [], [], [], [], [], [], []
    off, lo = 0, 0
    kc, kl = cell[keep], label[keep]
    while lo < len(keep):
        hi = lo + 1
        while hi < len(keep) and kc[hi] == kc[lo]:
            hi += 1
        labs, first, cnt = np.unique(kl[lo:hi], return_index=True, return_counts=True)
        if len(labs) >= 2 and cnt.max() >= 2:
            nc = hi - lo
            i, j = np.triu_indices(nc, 1)
            pa.append(keep[lo + i])
            pb.append(keep[lo + j])
            ab.append(off + i.astype(np.int64) * nc + j)
            ba.append(off + j.astype(np.int64) * nc + i)
            for x in range(len(labs)):
                if cnt[x] < 2:
                    continue
                for y in range(len(labs)):
                    if y != x:
                        blocks.append((off, nc, first[x], first[x] + cnt[x], first[y], first[y] + cnt[y]))
                        bc.append(kc[lo])
                        bla.append(labs[x])
                        blb.append(labs[y])
            off += nc * nc
        lo = hi
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)       # noqa: E731
    return Plan(keep, cat(pa).astype(np.int32), cat(pb).astype(np.int32), cat(ab), cat(ba), off,
                np.asarray(blocks, np.int64).reshape(-1, 6), np.asarray(bc, np.int64), np.asarray(bla, np.int64), np.asarray(blb, np.int64))


def aggregate(block_a, block_b, counts):
    """the ZeroSpeech aggregation, float64: block error = (wrong + tied / 2) / (triples - nan) (a block with no triple left has none);
    error(a, b) = the mean over the cells that have the block; score = the mean over the ordered (a, b) with at least one block.
    -> Aggregate(table [(a, b, cells, triples, error)] sorted by (a, b), score (nan without a block), block_error (NB,))"""
    counts = np.asarray(counts, np.int64).reshape(-1, 4)
    wrong, tied, nan, triples = (counts[:, k].astype(np.float64) for k in range(4))
    valid = triples - nan
    with np.errstate(all='ignore'):
        err = np.where(valid > 0, (wrong + 0.5 * tied) / np.where(valid > 0, valid, 1.0), np.nan)
    groups = collections.OrderedDict()
    for q in np.lexsort((np.asarray(block_b), np.asarray(block_a))):
        if err[q] == err[q]:
            groups.setdefault((int(block_a[q]), int(block_b[q])), []).append(q)
    table = [(a, b, len(qs), int(valid[qs].sum()), float(np.mean(err[qs]))) for (a, b), qs in groups.items()]
    score = float(np.mean([r[4] for r in table])) if table else float('nan')
    return Aggregate(table, score, err)


def plan_across(label, context, speaker, max_items=50, seed=0, max_bytes=None):
    """the work of one metrics.abx_across call.  keep: subsample(label, cell) with cell the dense id of (context, speaker) in sorted
    order, i.e. the items in (context, speaker, label, index) order -- what the within-speaker plan of the same cells keeps.  A context
    with at least one group gets a dense (n_c, n_c) matrix at mat_off; its DTW pairs are the unordered pairs i < j (context order,
    row-major) whose speakers differ, written to pos_ab and mirrored to pos_ba -- entries between items of one speaker stay unwritten.
    A group is (context, speaker s, a, b): s has both labels, a != b, and another speaker of the context has a.  grp (NG, 8) int64 =
    (mat_off, n_c, a_lo, a_hi, b_lo, b_hi, xr_lo, xr_hi), ordered by (context, speaker, a, b); xr (NX, 2) int64 holds, per (context,
    a), the (x_lo, x_hi) of every speaker that has a in ascending speaker order (the group's own among them), shared by its groups.
    max_bytes: ValueError as soon as the matrices (4 bytes an entry) and the pair tables (28 bytes a pair) pass it, before either is
    laid out."""
    label, context, speaker = (np.asarray(v, np.int64).reshape(-1) for v in (label, context, speaker))
    if not len(label) == len(context) == len(speaker):
        raise ValueError('abx: %d labels, %d contexts, %d speakers: one of each per item' % (len(label), len(context), len(speaker)))
    cell = np.unique(np.stack([context, speaker], 1), axis=0, return_inverse=True)[1].reshape(-1) if len(label) else context
    keep = subsample(label, cell, max_items, seed)
    kc, ks, kl = context[keep], speaker[keep], label[keep]
    pa, pb, ab, ba, grp, xr, gc, gs, ga, gb = [], [], [], [], [], [], [], [], [], []
    off = xoff = nbytes = 0
    bounds = np.concatenate([[0], np.flatnonzero(np.diff(kc)) + 1, [len(keep)]]) if len(keep) else np.zeros(1, np.int64)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        nc, s, lab = int(hi - lo), ks[lo:hi], kl[lo:hi]
        start = np.flatnonzero(np.concatenate([[True], (s[1:] != s[:-1]) | (lab[1:] != lab[:-1])]))      # the (speaker, label) runs
        end = np.concatenate([start[1:], [nc]])
        rs, rl = s[start], lab[start]
        o = np.lexsort((rs, rl))                                    # the runs by (label, speaker): one label's X ranges lie together
        labs, xfirst, xcnt = np.unique(rl[o], return_index=True, return_counts=True)
        ia, ib = np.nonzero((rs[:, None] == rs[None, :]) & (rl[:, None] != rl[None, :]))         # runs (s, a), (s, b): sorted by (s, a, b)
        li = np.searchsorted(labs, rl[ia])
        ok = xcnt[li] >= 2                                          # another speaker has a
        ia, ib, li = ia[ok], ib[ok], li[ok]
        if len(ia) == 0:
            continue
        n_pairs = (nc * nc - int((np.unique(s, return_counts=True)[1].astype(np.int64) ** 2).sum())) // 2
        nbytes += 4 * nc * nc + 28 * n_pairs
        if max_bytes is not None and nbytes > max_bytes:
            raise ValueError('abx: the distance matrices and pair tables of the contexts need more than %d bytes (%d bytes with the context of %d '
                             'items); lower --abx-max-items or use --abx-context triphone' % (max_bytes, nbytes, nc))
        i, j = np.triu_indices(nc, 1)
        cross = s[i] != s[j]
        i, j = i[cross].astype(np.int64), j[cross].astype(np.int64)
        pa.append(keep[lo + i])
        pb.append(keep[lo + j])
        ab.append(off + i * nc + j)
        ba.append(off + j * nc + i)
        full = lambda v: np.full(len(ia), v, np.int64)              # noqa: E731
        grp.append(np.stack([full(off), full(nc), start[ia], end[ia], start[ib], end[ib], xoff + xfirst[li], xoff + xfirst[li] + xcnt[li]], 1))
        xr.append(np.stack([start[o], end[o]], 1))
        gc.append(full(kc[lo]))
        gs.append(rs[ia])
        ga.append(rl[ia])
        gb.append(rl[ib])
        off += nc * nc
        xoff += len(o)
    cat = lambda v, w=None: np.concatenate(v).astype(np.int64) if v else np.zeros((0,) if w is None else (0, w), np.int64)     # noqa: E731
    return AcrossPlan(keep, cat(pa).astype(np.int32), cat(pb).astype(np.int32), cat(ab), cat(ba), off, cat(grp, 8), cat(xr, 2),
                      cat(gc), cat(gs), cat(ga), cat(gb))


def _group_means(keys, err):
    """err (already in the order the means are to be summed in) by the rows of keys -> (the distinct rows sorted, members, float64 means:
    a sequential sum in the given order and one division)"""
    uniq, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    return uniq, cnt, np.bincount(inv.reshape(-1), weights=err, minlength=len(uniq)) / cnt


def aggregate_across(grp_a, grp_b, grp_speaker, err, count):
    """Libri-light's order of means, float64: the kernel has averaged a group's pair scores over the X speakers (err, NaN without one);
    error(a, b) = the mean of err over the groups (context, speaker) of the pair that have one; score = the mean over the ordered (a, b)
    with at least one group.  -> AggregateAcross(table [(a, b, groups, triples, error)] sorted by (a, b) -- triples: those left after
    the NaN ones --, score (nan without a group), speakers [(speaker, groups, error)]: the same group errors averaged per speaker of
    A and B).  Vectorised: nothing here walks the groups."""
    a, b, spk, err = (np.asarray(v).reshape(-1) for v in (grp_a, grp_b, grp_speaker, err))
    count = np.asarray(count, np.int64).reshape(-1, 5)
    if not len(a) == len(b) == len(spk) == len(err) == len(count):
        raise ValueError('abx: %d, %d, %d group names, %d errors, %d counts: one of each per group' % (len(a), len(b), len(spk), len(err), len(count)))
    has = (err == err) & (count[:, 4] > 0)
    if not has.any():
        return AggregateAcross([], float('nan'), [])
    a, b, spk, err, left = a[has], b[has], spk[has], err[has].astype(np.float64), (count[has, 3] - count[has, 2])
    pairs, n, e = _group_means(np.stack([a, b], 1), err)
    tri = np.bincount(np.unique(np.stack([a, b], 1), axis=0, return_inverse=True)[1].reshape(-1), weights=left.astype(np.float64))
    table = [(int(p[0]), int(p[1]), int(g), int(t), float(v)) for p, g, t, v in zip(pairs, n, tri, e)]
    who, n, v = _group_means(spk.reshape(-1, 1), err)
    return AggregateAcross(table, float(np.mean(e)), [(int(w[0]), int(g), float(x)) for w, g, x in zip(who, n, v)])


def format_abx_across_csv(table, names=None):
    """abx_across.csv: ACROSS_HEADER, one row per ordered phone pair"""
    name = (lambda v: str(v)) if names is None else (lambda v: names[v])
    return '\n'.join([ACROSS_HEADER] + ['%s,%s,%d,%d,%.6f' % (name(a), name(b), g, t, e) for a, b, g, t, e in table]) + '\n'


def format_abx_across_speakers_csv(speakers, names=None):
    """abx_across_speakers.csv: ACROSS_SPEAKERS_HEADER, one row per speaker of A and B"""
    name = (lambda v: str(v)) if names is None else (lambda v: names[v])
    return '\n'.join([ACROSS_SPEAKERS_HEADER] + ['%s,%d,%.6f' % (name(s), g, e) for s, g, e in speakers]) + '\n'


def format_abx_csv(table, names=None):
    """abx.csv: ABX_HEADER, one row per ordered phone pair"""
    name = (lambda v: str(v)) if names is None else (lambda v: names[v])
    return '\n'.join([ABX_HEADER] + ['%s,%s,%d,%d,%.6f' % (name(a), name(b), c, t, e) for a, b, c, t, e in table]) + '\n'


def format_phones_csv(stats):
    """abx_phones.csv: PHONES_HEADER, one row per phone sorted by name: its tokens, the items made of them, those dropped as too short / too long"""
    return '\n'.join([PHONES_HEADER] + ['%s,%d,%d,%d,%d' % ((s,) + tuple(stats[s])) for s in sorted(stats)]) + '\n'


def ali_pairs(ali_dir, wav_dir):
    """the .ali files of ali_dir sorted by name, each with <stem>.wav of wav_dir -> [(ali file, stem, wav file)] (names, not paths).
    ValueError naming the file when there is none or a partner is missing."""
    files = sorted(f for f in os.listdir(ali_dir) if f.lower().endswith('.ali'))
    if not files:
        raise ValueError('--abx-ali-dir %s: no .ali files' % ali_dir)
    out = []
    for f in files:
        stem = os.path.splitext(f)[0]
        if not os.path.isfile(os.path.join(wav_dir, stem + '.wav')):
            raise ValueError('--abx-ali-dir: %s has no waveform %s' % (f, os.path.join(wav_dir, stem + '.wav')))
        out.append((f, stem, stem + '.wav'))
    return out
