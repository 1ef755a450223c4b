"""numpy oracle of the across-speaker ABX measure (st_abx_across, abx.plan_across / aggregate_across, metrics.abx_across): brute-force
triple enumeration over Python loops, the float64 pair scores, the group error as their sequential sum in ascending X-speaker order and
one division, and the aggregation in Libri-light's order (X speakers, then context and speaker, then phone pairs).  Distances and DTW
are tests/abx_oracle.py's.

    triple   A in (c, s, a), B in (c, s, b), b != a, X in (c, s', a), s' != s;  wrong: d(A, X) > d(B, X), tied: ==, nan: either is NaN
    pair     (wrong + tied / 2) / (triples - nan) for one (c, s, s', a, b); absent when nothing is left
    group    the mean of the present pair scores over s' for one (c, s, a, b)
"""
import numpy as np

import abx_oracle as O  # noqa: F401  (re-exported: the distances and the DTW the callers pair this oracle with)


def clamp_range(lo, hi, nc):
    """an index range clamped into [0, nc] -> the list of its indices (an inverted range is empty)"""
    lo, hi = min(max(int(lo), 0), nc), min(max(int(hi), 0), nc)
    return lo, hi, list(range(lo, hi))


def pair_counts(dm, ia, ib, ix):
    """(wrong, tied, nan, triples) over A in ia, B in ib, X in ix; d(., X) is read from row X"""
    wrong = tied = nan = 0
    for x in ix:
        for a in ia:
            ax = dm[x, a]
            for b in ib:
                bx = dm[x, b]
                if np.isnan(ax) or np.isnan(bx):
                    nan += 1
                elif ax > bx:
                    wrong += 1
                elif ax == bx:
                    tied += 1
    return wrong, tied, nan, len(ia) * len(ib) * len(ix)


def group(dm, a_rng, b_rng, x_rngs):
    """one group by brute force.  dm: the (n_c, n_c) matrix; a_rng, b_rng: (lo, hi); x_rngs: [(lo, hi)] in ascending speaker order, the
    group's own among them (it is the one equal to a_rng after clamping) -> (err float64 or nan, (wrong, tied, nan, triples, x_speakers))"""
    dm = np.asarray(dm)
    nc = len(dm)
    a_lo, a_hi, ia = clamp_range(*a_rng, nc)
    _, _, ib = clamp_range(*b_rng, nc)
    tot, scores = [0, 0, 0, 0], []
    for lo, hi in x_rngs:
        x_lo, x_hi, ix = clamp_range(lo, hi, nc)
        if (x_lo, x_hi) == (a_lo, a_hi):
            continue
        c = pair_counts(dm, ia, ib, ix)
        tot = [t + v for t, v in zip(tot, c)]
        if c[3] - c[2] > 0:
            scores.append((np.float64(c[0]) + np.float64(0.5) * np.float64(c[1])) / np.float64(c[3] - c[2]))
    s = np.float64(0.0)
    for v in scores:                    # sequentially, in the order of the list
        s = s + v
    return (float(s / np.float64(len(scores))) if scores else float('nan')), tuple(tot) + (len(scores),)


def seq_mean(vals):
    s = 0.0
    for v in vals:
        s = s + float(v)
    return s / len(vals)


def aggregate(groups):
    """{(context, speaker, a, b): (err, counts)} -> (table {(a, b): (groups, triples left, error)}, score, speakers {s: (groups, error)}):
    means over the groups that have an error, visited in sorted key order"""
    per, spk = {}, {}
    for (c, s, a, b) in sorted(groups):
        err, cnt = groups[(c, s, a, b)]
        if err == err:
            per.setdefault((a, b), []).append((err, cnt[3] - cnt[2]))
            spk.setdefault(s, []).append(err)
    table = {k: (len(v), sum(t for _, t in v), seq_mean([e for e, _ in v])) for k, v in per.items()}
    score = float(np.mean([table[k][2] for k in sorted(table)])) if table else float('nan')
    return table, score, {s: (len(v), seq_mean(v)) for s, v in spk.items()}


def abx_across(dist, label, context, speaker, items=None):
    """the whole measure by brute force.  dist(p, q): the distance of items p and q, asked for cross-speaker pairs only (p before q in
    the order below); items: the item indices that take part (None: all), ordered by (context, speaker, label, index).
    -> (groups {(context, speaker, a, b): (err, (wrong, tied, nan, triples, x_speakers))}, table, score, speakers)"""
    label, context, speaker = np.asarray(label), np.asarray(context), np.asarray(speaker)
    items = np.arange(len(label)) if items is None else np.asarray(items)
    items = np.array(sorted(items.tolist(), key=lambda q: (context[q], speaker[q], label[q], q)), np.int64)
    groups = {}
    for c in sorted(set(context[items].tolist())):
        mem = items[context[items] == c]
        n = len(mem)
        dm = np.full((n, n), np.nan)        # same-speaker entries stay NaN: reading one would show up in the nan count
        for i in range(n):
            for j in range(i + 1, n):
                if speaker[mem[i]] != speaker[mem[j]]:
                    dm[i, j] = dm[j, i] = dist(int(mem[i]), int(mem[j]))
        where = {}
        for i, q in enumerate(mem):
            where.setdefault((int(speaker[q]), int(label[q])), []).append(i)
        rng = {k: (v[0], v[-1] + 1) for k, v in where.items()}
        for (s, a) in sorted(rng):
            xs = [rng[(t, l)] for (t, l) in sorted(rng) if l == a]
            if len(xs) < 2:
                continue
            for (t, b) in sorted(rng):
                if t == s and b != a:
                    groups[(int(c), s, a, b)] = group(dm, rng[(s, a)], rng[(t, b)], xs)
    return (groups,) + aggregate(groups)
