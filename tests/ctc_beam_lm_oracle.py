"""float64 oracle of the LM-fused CTC prefix beam search (st_ctc_beam_search_lm): ctc_beam_oracle.search restated with the context row of
every prefix and the bonus of every extension.  The bonus table is the kernel's fp32 table cast up: the same numbers the kernel adds."""
import numpy as np

import ctc_beam_oracle as O

NEG_INF = -np.inf
_lae = O._lae


def start_row(V, order, bos=1):
    """the row of the empty prefix's context (0, ..., 0, bos); 0 for a unigram"""
    return 0 if order == 1 else bos


def next_row(row, c, V, order):
    return (row * V + c) % V ** (order - 1) if order > 1 else 0


def table_order(bonus):
    rows, V = bonus.shape
    for n in range(1, 5):
        if rows == V ** (n - 1):
            return n
    raise ValueError('no (V^(n-1), V) table: %s' % (bonus.shape,))


def prefix_bonus(label, bonus, bos=1):
    """the sum of the extension bonuses along `label` from the start context (float64)"""
    bonus = np.asarray(bonus, np.float64)
    V, order = bonus.shape[1], table_order(bonus)
    row, tot = start_row(V, order, bos), 0.0
    for c in label:
        tot += bonus[row, c]
        row = next_row(row, c, V, order)
    return tot


def search(lp, W, bonus, blank=0, bos=1):
    """ctc_beam_oracle.search with the table: -> (final beam prefixes best first, their fused scores, the smallest W-th / (W+1)-th
    candidate gap over the frames); (None, None, inf) when lp holds a NaN"""
    T, V = lp.shape
    bonus = np.asarray(bonus, np.float64)
    order = table_order(bonus)
    assert bonus.shape[1] == V
    if np.isnan(lp).any():
        return None, None, np.inf
    beam = [((), 0.0, NEG_INF, start_row(V, order, bos))]       # (prefix, log p_blank, log p_nonblank, context row), in slot order
    margin = np.inf
    for t in range(T):
        nb = len(beam)
        slot = {p: s for s, (p, _, _, _) in enumerate(beam)}
        stays = []
        for p, pb, pnb, row in beam:
            spnb = pnb + lp[t, p[-1]] if p else NEG_INF
            stays.append([p, _lae(pb, pnb) + lp[t, blank], spnb, row])
        exts = []
        for s, (p, pb, pnb, row) in enumerate(beam):
            tot = _lae(pb, pnb)
            r = 0
            for c in range(V):
                if c == blank:
                    continue
                e = ((pb if p and c == p[-1] else tot) + lp[t, c]) + bonus[row, c]
                q = p + (c,)
                if q in slot:
                    stays[slot[q]][2] = _lae(stays[slot[q]][2], e)
                else:
                    exts.append((nb + s * (V - 1) + r, q, NEG_INF, e, next_row(row, c, V, order)))
                r += 1
        cands = [(i, p, a, b, row) for i, (p, a, b, row) in enumerate(stays)] + exts
        cands.sort(key=lambda x: (-_lae(x[2], x[3]), x[0]))
        sc = [_lae(x[2], x[3]) for x in cands]
        if len(cands) > W:
            margin = min(margin, O._gap(sc[W - 1], sc[W]))
        beam = [(p, a, b, row) for _, p, a, b, row in cands[:W]]
    return [p for p, _, _, _ in beam], [_lae(a, b) for _, a, b, _ in beam], margin


def beam_search(lp, W, N, bonus, blank=0, bos=1):
    """-> (hyps, scores, margin) as ctc_beam_oracle.beam_search, with the fused scores"""
    return O.finish(*search(lp, W, bonus, blank, bos), N)


def batch_beam_search(prob, lengths, W, N, bonus, blank=0, log_input=False, eps=1e-10, bos=1):
    lp = O.log_probs(prob, log_input, eps)
    B, T, _ = lp.shape
    lengths = [T] * B if lengths is None else [int(x) for x in lengths]
    out = [beam_search(lp[b, :lengths[b]], W, N, bonus, blank, bos) for b in range(B)]
    return [o[0] for o in out], np.array([o[1] for o in out]), np.array([o[2] for o in out])
