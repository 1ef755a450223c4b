"""Float-free oracle of st_edit_align (include/semitts.h): the filter, the full Levenshtein table, the trace-back with its tie order
(diagonal, then the deletion (i-1, j), then the insertion (i, j-1)), the four counts, the aligned pairs and the confusion matrix -- plain
Python integers and numpy int arrays, nothing shared with the kernel.  Also the text of the files PhnScorer writes, formatted
independently of the solver, and generators of adversarial pairs (alphabets of 2 and 3 symbols, where nearly every cell is a tie)."""
import numpy as np


def filt(seq, ignore=()):
    ig = set(int(i) for i in ignore)
    return [int(x) for x in seq if int(x) not in ig]


def table(r, h):
    """the full (n + 1, m + 1) table D"""
    n, m = len(r), len(h)
    D = [list(range(m + 1))]
    for i in range(1, n + 1):
        up, ri = D[-1], r[i - 1]
        cur = [i]
        for j in range(1, m + 1):
            cur.append(min(up[j - 1] + (ri != h[j - 1]), up[j] + 1, cur[j - 1] + 1))
        D.append(cur)
    return np.asarray(D, dtype=np.int64).reshape(n + 1, m + 1)


def align(ref, hyp, ignore=()):
    """-> (counts (C, S, D, I), pairs: the aligned (reference token, hypothesis token) in forward order, -1 for a gap)"""
    r, h = filt(ref, ignore), filt(hyp, ignore)
    D = table(r, h)
    i, j = len(r), len(h)
    rev = []
    c = s = d = ins = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1, j - 1] + (r[i - 1] != h[j - 1]) == D[i, j]:
            rev.append((r[i - 1], h[j - 1]))
            if r[i - 1] == h[j - 1]:
                c += 1
            else:
                s += 1
            i, j = i - 1, j - 1
        elif j == 0 or (i > 0 and D[i - 1, j] + 1 == D[i, j]):
            rev.append((r[i - 1], -1))
            d += 1
            i -= 1
        else:
            rev.append((-1, h[j - 1]))
            ins += 1
            j -= 1
    assert s + d + ins == D[len(r), len(h)]
    return (c, s, d, ins), rev[::-1]


def levenshtein(a, b):
    """the plain two-row distance, written apart from table()"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def brute_force_distance(a, b):
    """the distance by exhaustive recursion over the three moves (tiny strings only)"""
    if not a:
        return len(b)
    if not b:
        return len(a)
    return min(brute_force_distance(a[:-1], b[:-1]) + (a[-1] != b[-1]), brute_force_distance(a[:-1], b) + 1, brute_force_distance(a, b[:-1]) + 1)


def is_cover(pairs, r, h):
    """the pairs, gaps removed, spell r on the left and h on the right, in order, and no row is a double gap"""
    return ([a for a, _ in pairs if a != -1] == list(r) and [b for _, b in pairs if b != -1] == list(h)
            and all(a != -1 or b != -1 for a, b in pairs))


def add_confusion(conf, pairs, V):
    """add one aligned path into conf (V + 1, V + 1): a pair with a token outside [0, V) touches no cell"""
    for a, b in pairs:
        row = V if a == -1 else a
        col = V if b == -1 else b
        if (a != -1 and not 0 <= a < V) or (b != -1 and not 0 <= b < V):
            continue
        conf[row, col] += 1
    return conf


def batch(hyp, hyp_len, ref, ref_len, ignore, V):
    """the kernel's outputs for hyp (B, N, Lh), hyp_len (B, N), ref (B, Lr), ref_len (B,) or None (lengths clamped into [0, L]):
    -> counts (B, N, 4), ali_len (B, N), ali (B, N, Lr + Lh, 2) int32 and confusion (V + 1, V + 1) int64 from path 0"""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    counts = np.zeros((B, N, 4), dtype=np.int32)
    ali_len = np.zeros((B, N), dtype=np.int32)
    ali = np.full((B, N, Lr + Lh, 2), -1, dtype=np.int32)
    conf = np.zeros((V + 1, V + 1), dtype=np.int64)
    for b in range(B):
        n = Lr if ref_len is None else min(max(int(ref_len[b]), 0), Lr)
        for k in range(N):
            m = min(max(int(hyp_len[b][k]), 0), Lh)
            c, pairs = align(ref[b, :n], hyp[b, k, :m], ignore)
            counts[b, k] = c
            ali_len[b, k] = len(pairs)
            if pairs:
                ali[b, k, :len(pairs)] = np.asarray(pairs, dtype=np.int64).astype(np.int32)
            if k == 0:
                add_confusion(conf, pairs, V)
    return counts, ali_len, ali, conf


# ---------------------------------------------------------------- adversarial pairs
def random_pair(rs, n, m, alphabet, first=3):
    """two strings over `alphabet` symbols first, first + 1, ...: with 2 or 3 symbols nearly every cell of the table is a tie"""
    return rs.randint(first, first + alphabet, size=n).tolist(), rs.randint(first, first + alphabet, size=m).tolist()


def edited_pair(rs, n, alphabet, rate=0.15, first=3):
    """a reference of n symbols and a hypothesis made from it by about `rate` substitutions, deletions and insertions"""
    ref = rs.randint(first, first + alphabet, size=n).tolist()
    hyp = []
    for x in ref:
        u = rs.rand()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            hyp.append(int(rs.randint(first, first + alphabet)))
            continue
        hyp.append(x)
        if u > 1 - rate / 3:
            hyp.append(int(rs.randint(first, first + alphabet)))
    return ref, hyp


def pad(seqs, L, fill=0):
    out = np.full((len(seqs), L), fill, dtype=np.int64)
    for k, s in enumerate(seqs):
        out[k, :len(s)] = s
    return out


# ---------------------------------------------------------------- the files of PhnScorer
def sym(vocab, t):
    return vocab[t] if vocab is not None and 0 <= t < len(vocab) else str(t)


def per_text(rows, nbest=False):
    """rows: (file, (C, S, D, I)[, nbest_dist, nbest_path])"""
    out = ['file,ref_tokens,hyp_tokens,correct,sub,del,ins,per' + (',nbest_per,nbest_path' if nbest else '')]
    for row in rows:
        f, (c, s, d, i) = row[0], row[1]
        n = c + s + d
        line = '%s,%d,%d,%d,%d,%d,%d,%s' % (f, n, c + s + i, c, s, d, i, '%.6f' % ((s + d + i) / n) if n else 'nan')
        if nbest:
            line += ',%s,%d' % ('%.6f' % (row[2] / n) if n else 'nan', row[3])
        out.append(line)
    return '\n'.join(out) + '\n'


def confusions_text(conf, vocab=None):
    V = conf.shape[0] - 1
    cells = []
    for a in range(V + 1):
        for b in range(V + 1):
            if a != b and conf[a, b]:
                cells.append((-int(conf[a, b]), a, b))
    out = ['ref,hyp,count']
    for negc, a, b in sorted(cells):
        out.append('%s,%s,%d' % ('<ins>' if a == V else sym(vocab, a), '<del>' if b == V else sym(vocab, b), -negc))
    return '\n'.join(out) + '\n'


def phones_text(conf, vocab=None):
    V = conf.shape[0] - 1
    out = ['phone,ref_count,correct,sub,del,ins_as_hyp']
    for a in range(V):
        ref_count = int(conf[a, :].sum())
        if ref_count == 0 and int(conf[:, a].sum()) == 0:
            continue
        out.append('%s,%d,%d,%d,%d,%d' % (sym(vocab, a), ref_count, conf[a, a], conf[a, :V].sum() - conf[a, a], conf[a, V], conf[V, a]))
    return '\n'.join(out) + '\n'


def ops_text(pairs, vocab=None):
    ref, hyp, op = [], [], []
    for a, b in pairs:
        x, y = ('*' if a == -1 else sym(vocab, a)), ('*' if b == -1 else sym(vocab, b))
        o = 'D' if b == -1 else 'I' if a == -1 else 'C' if a == b else 'S'
        w = max(len(x), len(y))
        ref.append(x.ljust(w))
        hyp.append(y.ljust(w))
        op.append(o.ljust(w))
    return ''.join((tag + ' '.join(cols)).rstrip() + '\n' for tag, cols in (('REF: ', ref), ('HYP: ', hyp), ('OP:  ', op)))
