"""Greedy CTC transcript + edit distance on the MI355X (st_ctc_greedy_edit_distance / st_ids_edit_distance, semi_tts_amd.metrics)
against the plain-Python restatement of the reference's cal_per (tests/per_oracle.py): exact equality of dist, ref_len, hyp, hyp_len."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_oracle as O   # noqa: E402
from semi_tts_amd import ops   # noqa: E402
from semi_tts_amd import metrics   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ids(rs, B, T, V):
    """frame ids with frequent runs and ignored ids: a small alphabet, run lengths 1..4"""
    alpha = [a for a in (0, 1, 2, 42, 3, 4, 5, 6) if a < V]
    out = np.zeros((B, T), np.int64)
    for b in range(B):
        seq = []
        while len(seq) < T:
            seq += [int(rs.choice(alpha))] * int(rs.randint(1, 5))
        out[b] = seq[:T]
    return out


def _batch(seed, B, T, V, L, ties=0.1, nans=0.03):
    """posteriors whose argmax is _ids (plus exact ties and NaNs), and transcripts over a small alphabet with ignored ids anywhere"""
    rs = np.random.RandomState(seed)
    ids = _ids(rs, B, T, V)
    prob = (rs.uniform(0, 0.5, (B, T, V))).astype(np.float32)
    np.put_along_axis(prob, ids[..., None], 1.0, axis=-1)
    if V > 1:
        tie = rs.uniform(size=(B, T)) < ties                 # a second index with exactly the maximum: the first one wins
        j = rs.randint(0, V, (B, T))
        prob[tie, j[tie]] = 1.0
        nan = rs.uniform(size=(B, T)) < nans                 # NaN is the maximum, the first NaN wins
        k1, k2 = rs.randint(0, V, (B, T)), rs.randint(0, V, (B, T))
        prob[nan, k1[nan]] = np.nan
        both = nan & (rs.uniform(size=(B, T)) < 0.5)
        prob[both, k2[both]] = np.nan
    talpha = [a for a in (0, 1, 2, 42, 3, 4, 5, 6, 7) if a < max(V, 8)]
    text = rs.choice(talpha, (B, L)).astype(np.int64)
    return torch.from_numpy(prob), torch.from_numpy(text)


def _check(dev, prob, text):
    dist, ref_len, hyp, hyp_len = ops.ctc_greedy_edit_distance(prob.to(dev), text.to(dev), O.IGNORE, want_hyp=True)
    od, on, oh = O.batch(O.argmax_rows(prob), text.tolist())
    assert dist.cpu().tolist() == od
    assert ref_len.cpu().tolist() == on
    assert hyp_len.cpu().tolist() == [len(h) for h in oh]
    H = hyp.cpu()
    for b, h in enumerate(oh):
        assert H[b, :len(h)].tolist() == h and not H[b, len(h):].any()
    return dist, ref_len, hyp, hyp_len


SHAPES = [(1, 1, 1, 1), (5, 2, 43, 43), (32, 129, 43, 43), (5, 533, 43, 171), (1, 4096, 43, 1024), (5, 4096, 43, 171),
          (5, 129, 512, 171), (1, 2, 10240, 1), (5, 533, 10240, 43), (32, 129, 1, 43), (5, 533, 512, 1024)]


@pytest.mark.parametrize('B, T, V, L', SHAPES)
def test_kernel_equals_oracle(dev, B, T, V, L):
    prob, text = _batch(B * 7919 + T * 31 + V + L, B, T, V, L)
    _check(dev, prob, text)


def test_ties_and_nans_take_the_first_index(dev):
    V = 43
    prob = torch.zeros(1, 6, V)
    prob[0, 0, [5, 9]] = 1.0                    # tie -> 5
    prob[0, 1, [9, 5]] = 1.0                    # same ids, tie -> 5 (runs collapse)
    prob[0, 2, 30] = float('nan')               # NaN beats everything -> 30
    prob[0, 2, 31] = 2.0
    prob[0, 3, [12, 7]] = float('nan')          # first NaN -> 7
    prob[0, 4, :] = -float('inf')               # all equal -> 0 (blank, dropped)
    prob[0, 5, [3, 40]] = -0.0                  # +-0 ties with the zeros before index 3 -> 0
    assert torch.argmax(prob, -1).tolist() == [[5, 5, 30, 7, 0, 0]]
    text = torch.tensor([[5, 30, 7, 0]])
    dist, ref_len, hyp, hyp_len = _check(dev, prob, text)
    assert hyp[0, :3].tolist() == [5, 30, 7] and dist.item() == 0 and ref_len.item() == 3


def test_ids_path_equals_posterior_path(dev):
    prob, text = _batch(11, 32, 533, 43, 171)
    ids = torch.argmax(prob, -1).to(dev)
    a = ops.ctc_greedy_edit_distance(prob.to(dev), text.to(dev), O.IGNORE, want_hyp=True)
    b = ops.ctc_greedy_edit_distance(ids, text.to(dev), O.IGNORE, want_hyp=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ed = metrics.edit_distances(ids, text.to(dev))
    assert torch.equal(ed[0], a[0]) and torch.equal(ed[1], a[1])


def test_two_launches_are_bitwise_equal(dev):
    prob, text = _batch(12, 32, 533, 512, 171)
    prob, text = prob.to(dev), text.to(dev)
    a = ops.ctc_greedy_edit_distance(prob, text, O.IGNORE, want_hyp=True)
    b = ops.ctc_greedy_edit_distance(prob, text, O.IGNORE, want_hyp=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_all_ignored_transcript(dev):
    prob, text = _batch(13, 5, 129, 43, 43)
    text[2] = torch.tensor([0, 1, 2, 42] * 10 + [0, 0, 42])
    dist, ref_len, _, hyp_len = _check(dev, prob, text)
    assert ref_len[2].item() == 0 and dist[2].item() == hyp_len[2].item()
    assert math.isnan(float(metrics.per_sum(prob.to(dev), text.to(dev))))
    assert math.isnan(metrics.cal_per(prob.to(dev), text.to(dev)))


def test_cal_per_equals_oracle_mean(dev):
    for seed, (B, T, V, L) in enumerate([(32, 129, 43, 43), (64, 533, 43, 171), (1, 2, 43, 1)]):
        prob, text = _batch(100 + seed, B, T, V, L, nans=0.0)
        text[:, 0] = 3                              # every transcript non-empty
        want = O.cal_per(O.argmax_rows(prob), text.tolist())
        got = metrics.cal_per(prob.to(dev), text.to(dev))
        assert abs(got - want) <= 1e-12
        s = metrics.per_sum(prob.to(dev), text.to(dev))
        assert s.is_cuda and s.dtype == torch.float64
        assert metrics.cal_per(torch.argmax(prob, -1).to(dev), text.to(dev)) == got
        assert metrics.cal_per(prob.to(dev), text) == got             # a host transcript goes to the device


def test_out_of_limit_shapes_raise_before_launch(dev):
    f = lambda *s: torch.zeros(*s, device=dev)
    i64 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int64)
    bad = [(f(1, 4097, 1), i64(1, 4)), (f(1, 1, 10241), i64(1, 4)), (f(1, 1, 43), i64(1, 1025)), (f(2, 3, 43), i64(3, 4)),
           (f(0, 3, 43), i64(0, 4)), (f(1, 0, 43), i64(1, 4)), (f(1, 3, 0), i64(1, 4)), (f(1, 3, 43), i64(1, 0)),
           (f(1, 3, 43), torch.zeros(1, 4, device=dev, dtype=torch.int32)), (f(1, 3, 43).double(), i64(1, 4)),
           (torch.zeros(1, 3, dtype=torch.int32, device=dev), i64(1, 4)), (f(1, 3, 43), i64(1, 4).cpu()), (f(3, 43), i64(3, 4))]
    for prob, text in bad:
        with pytest.raises(ValueError):
            ops.ctc_greedy_edit_distance(prob, text, O.IGNORE)
    with pytest.raises(ValueError):
        ops.ctc_greedy_edit_distance(f(1, 3, 43), i64(1, 4), list(range(65)))
    ops.ctc_greedy_edit_distance(f(1, 4096, 1), i64(1, 1024), list(range(64)))     # the limits themselves are accepted
    ops.ctc_greedy_edit_distance(f(1, 1, 10240), i64(1, 1), ())
