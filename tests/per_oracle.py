"""Plain-Python restatement of the reference's cal_per (src/util.py:169-181), written from its definition: greedy CTC transcript
(argmax, runs collapsed FIRST, then the ignored ids dropped), the transcript without the ignored ids, and the Levenshtein distance
with unit costs (what editdistance.eval computes) by the O(|hyp| |ref|) table."""

IGNORE = (0, 1, 2, 42)


def argmax_rows(prob):
    """torch.argmax(dim=-1) as a list of lists, via torch on the CPU (first maximal index; the first NaN wins)"""
    return prob.detach().cpu().argmax(dim=-1).tolist()


def collapse_filter(p, ignore=IGNORE):
    return [v for i, v in enumerate(p) if (i == 0 or v != p[i - 1]) and v not in ignore]


def strip(t, ignore=IGNORE):
    return [v for v in t if v not in ignore]


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def utterance(p, t, ignore=IGNORE):
    """(dist, ref_len, hyp) of one utterance: p = frame ids, t = transcript ids"""
    hyp, ref = collapse_filter(list(p), ignore), strip(list(t), ignore)
    return levenshtein(hyp, ref), len(ref), hyp


def batch(pred_ids, text, ignore=IGNORE):
    """-> lists (dist, ref_len, hyp) over the batch; pred_ids / text: nested lists"""
    out = [utterance(p, t, ignore) for p, t in zip(pred_ids, text)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def cal_per(pred_ids, text, ignore=IGNORE):
    """the batch mean of dist / ref_len (raises ZeroDivisionError on an empty transcript, as the reference does)"""
    d, n, _ = batch(pred_ids, text, ignore)
    er = [float(a) / b for a, b in zip(d, n)]
    return sum(er) / len(er)
