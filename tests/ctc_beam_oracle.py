"""float64 oracles of the CTC prefix beam search (st_ctc_beam_search): a plain numpy search over exact prefixes (tuples) with the kernel's
candidate order and tie-break, and a brute-force scorer (the CTC forward recursion for every labelling)."""
import itertools

import numpy as np

NEG_INF = -np.inf


def _lae(a, b):
    return np.logaddexp(a, b)


def log_probs(prob, log_input=False, eps=1e-10):
    p = np.asarray(prob, np.float64)
    return p if log_input else np.log(p + eps)


def beam_search(lp, W, N, blank=0):
    """lp (T, V) float64 log-probabilities of one utterance -> (hyps: list of N tuples, scores (N,), margin).  margin: the smallest gap
    between the W-th and (W+1)-th candidate over all frames, and between neighbours among the first N + 1 prefixes after the last frame
    (inf if there is no such pair): a search in lower precision gives these results wherever the margin is well above its error.
    NaN anywhere: empty hypotheses of score NaN."""
    beam, sc, margin = search(lp, W, blank)
    return finish(beam, sc, margin, N)


def finish(beam, sc, margin, N):
    """search()'s final beam -> beam_search()'s (hyps, scores, margin) for N paths"""
    if sc is None:
        return [()] * N, np.full(N, np.nan), np.inf
    for k in range(min(N + 1, len(sc)) - 1):
        margin = min(margin, _gap(sc[k], sc[k + 1]))
    hyps = list(beam[:N]) + [()] * max(0, N - len(beam))
    return hyps, np.array(list(sc[:N]) + [NEG_INF] * max(0, N - len(beam))), margin


def search(lp, W, blank=0):
    """-> (final beam prefixes best first, their scores, the smallest W-th / (W+1)-th candidate gap over the frames); (None, None, inf)
    when lp holds a NaN"""
    T, V = lp.shape
    if np.isnan(lp).any():
        return None, None, np.inf
    beam = [((), 0.0, NEG_INF)]                                  # (prefix, log p_blank, log p_nonblank), in slot order
    margin = np.inf
    for t in range(T):
        nb = len(beam)
        slot = {p: s for s, (p, _, _) in enumerate(beam)}
        stays = []
        for p, pb, pnb in beam:
            spnb = pnb + lp[t, p[-1]] if p else NEG_INF
            stays.append([p, _lae(pb, pnb) + lp[t, blank], spnb])
        exts = []
        for s, (p, pb, pnb) in enumerate(beam):
            tot = _lae(pb, pnb)
            r = 0
            for c in range(V):
                if c == blank:
                    continue
                e = (pb if p and c == p[-1] else tot) + lp[t, c]
                q = p + (c,)
                if q in slot:
                    stays[slot[q]][2] = _lae(stays[slot[q]][2], e)
                else:
                    exts.append((nb + s * (V - 1) + r, q, NEG_INF, e))
                r += 1
        cands = [(i, p, a, b) for i, (p, a, b) in enumerate(stays)] + exts
        cands.sort(key=lambda x: (-_lae(x[2], x[3]), x[0]))
        sc = [_lae(x[2], x[3]) for x in cands]
        if len(cands) > W:
            margin = min(margin, _gap(sc[W - 1], sc[W]))
        beam = [(p, a, b) for _, p, a, b in cands[:W]]
    return [p for p, _, _ in beam], [_lae(a, b) for _, a, b in beam], margin


def _gap(a, b):
    if a == b == NEG_INF:
        return np.inf                         # structurally impossible candidates: -inf in any precision, ordered by index
    return a - b


def batch_beam_search(prob, lengths, W, N, blank=0, log_input=False, eps=1e-10):
    """prob (B, T, V) -> (hyps [B][N] tuples, scores (B, N), margins (B,)); utterance b uses frames [0, lengths[b])"""
    lp = log_probs(prob, log_input, eps)
    B, T, _ = lp.shape
    lengths = [T] * B if lengths is None else [int(x) for x in lengths]
    out = [beam_search(lp[b, :lengths[b]], W, N, blank) for b in range(B)]
    return [o[0] for o in out], np.array([o[1] for o in out]), np.array([o[2] for o in out])


def ctc_log_prob(lp, label, blank=0):
    """exact log P(label | lp) by the CTC forward recursion (float64)"""
    T = lp.shape[0]
    ext = [blank]
    for c in label:
        ext += [c, blank]
    S = len(ext)
    a = np.full(S, NEG_INF)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        n = np.full(S, NEG_INF)
        for s in range(S):
            v = a[s]
            if s >= 1:
                v = _lae(v, a[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = _lae(v, a[s - 2])
            n[s] = v + lp[t, ext[s]]
        a = n
    return _lae(a[S - 1], a[S - 2]) if S > 1 else a[0]


def brute_force(lp, blank=0):
    """every labelling of at most T non-blank symbols with its exact log probability, best first: list of (label tuple, score)"""
    T, V = lp.shape
    syms = [c for c in range(V) if c != blank]
    out = []
    for n in range(T + 1):
        for lab in itertools.product(syms, repeat=n):
            out.append((lab, ctc_log_prob(lp, lab, blank)))
    out.sort(key=lambda x: -x[1])
    return out


def n_prefixes(T, V):
    """prefixes a search over T frames of V classes can reach (all labellings of at most T symbols)"""
    return sum((V - 1) ** n for n in range(T + 1))


def levenshtein(a, b):
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, y in enumerate(b, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (x != y))
    return d[len(b)]
