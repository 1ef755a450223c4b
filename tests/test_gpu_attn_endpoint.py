"""st_attn_endpoint on the device against the float64 numpy oracle of tests/attn_endpoint_oracle.py: every integer output, peak and dur
bit for bit; focus within end * 2**-23 absolute.  That bound is derived, not measured: the peak weights lie in [0, 1], so every
partial sum is at most `end` and each of the end - 1 fp32 additions, in whatever order, errs by at most end * 2**-24; the sum is off by
less than end**2 * 2**-24, the mean by less than end * 2**-24, and the one division adds at most 2**-24 to a mean of at most 1:
(end + 1) * 2**-24 <= end * 2**-23.

The kernel gives a row to a wave (4 waves) and strides 64 lanes over L; the run search gives thread i the steps [i seg, (i + 1) seg),
seg = ceil(S / 256).  The shapes below cross L = 64 and 128, S = 4 (waves), S = 256 (seg 1 -> 2) and reach the limits S = 4096, L = 2048."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import attn_endpoint_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT_FIELDS = ('end', 'reached', 'n_back', 'n_skip', 'covered', 'nonfinite')


def _run(align, enc_len, patience=3, max_jump=4):
    """align (B, S, L) array or device tensor -> O.Result of numpy arrays"""
    from semi_tts_amd.metrics import attention_endpoints
    a = align if torch.is_tensor(align) else torch.from_numpy(np.ascontiguousarray(align, np.float32)).to(DEV)
    ep = attention_endpoints(a, enc_len, patience, max_jump)
    torch.cuda.synchronize()
    B, S, L = a.shape
    out = O.Result(*(getattr(ep, k).cpu().numpy() for k in O.Result._fields))
    for k in INT_FIELDS:
        assert getattr(out, k).dtype == np.int32 and getattr(out, k).shape == (B,), k
    assert out.focus.dtype == np.float32 and out.focus.shape == (B,)
    assert out.peak.dtype == np.int32 and out.peak.shape == (B, S) and out.dur.dtype == np.int32 and out.dur.shape == (B, L)
    return out


def _check(got, align, enc_len, patience=3, max_jump=4, what=''):
    """device outputs against the oracle on the same fp32 values; -> the oracle's Result"""
    want = O.endpoint_batch(np.asarray(align, np.float32), enc_len, patience, max_jump)
    for k in INT_FIELDS + ('peak', 'dur'):
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k, getattr(got, k), getattr(want, k))
    for b, (g, w, end) in enumerate(zip(got.focus.tolist(), want.focus.tolist(), want.end.tolist())):
        print('%s utt %d: focus %.9g oracle %.9g diff %.3g bound %.3g' % (what, b, g, w, abs(g - w), end * 2.0 ** -23))
        if np.isfinite(w):
            assert abs(g - w) <= end * 2.0 ** -23, (what, b, g, w)
        else:
            assert (np.isnan(w) and np.isnan(g)) or g == w, (what, b, g, w)
    return want


def _lens(L):
    return sorted({min(max(n, 1), L) for n in (1, 2, L - 1, L)})


def _steps(K, big):
    return sorted({s for s in (1, K - 1, K, K + 1, 3, 4, 5, 255, 256, 257) + ((4096,) if big else ()) if s >= 1})


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('L', [1, 2, 63, 64, 65, 129, 2048])
def test_random_walks_at_every_shape(L, K):
    """every S of the list at this (L, K), one launch each: a ragged batch with n in {1, 2, L - 1, L}, peaks from a random walk with
    skips, falls and visits to the last phone.  (S = 4096 stays with L <= 129: the oracle, not the kernel, would take seconds beyond)"""
    rs = np.random.RandomState(1000 * L + K)
    for S in _steps(K, L <= 129):
        ns = _lens(L)
        a = np.stack([O.from_peaks(O.random_peaks(rs, S, L, n), L, rs, peak_w=0.5 + 0.4 * rs.rand()) for n in ns])
        _check(_run(a, ns, K, 1 + L % 5), a, ns, K, 1 + L % 5, 'L=%d S=%d K=%d' % (L, S, K))


@pytest.mark.parametrize('S', [5, 257, 4096])
def test_where_the_run_starts(S):
    """the first full run placed at the ends of the step range and on either side of the boundaries between the threads' segments
    (seg = ceil(S / 256) steps each) and between the waves, behind broken runs of K - 1 flags; the last one starts one step too late"""
    L, n, K = 65, 40, 3
    seg = (S + 255) // 256
    starts = sorted({t for t in (0, 1, seg - 1, seg, 2 * seg - 1, 63 * seg, 64 * seg - 1, 64 * seg, 64 * seg + 1, 255 * seg - 2, S - K - 1, S - K,
                                 S - K + 1) if 0 <= t <= S - K + 1})
    batch = []
    for t0 in starts:
        cols = [min(t // 2, n - 2) for t in range(S)]               # a slow staircase that stops short of the last phone
        for t in range(2, t0 - 1, 7):                               # broken runs: K - 1 flagged steps, then back
            cols[t:t + K - 1] = [n - 1 + (t % 3)] * len(cols[t:t + K - 1])
        if t0 > 0:
            cols[t0 - 1] = n - 2
        cols[t0:] = [n - 1] * (S - t0)
        batch.append(O.from_peaks(cols, L))
    a = np.stack(batch)
    want = _check(_run(a, [n] * len(starts), K), a, [n] * len(starts), K, what='S=%d' % S)
    assert want.end.tolist() == [t0 + K if t0 + K <= S else S for t0 in starts]
    assert want.reached.tolist() == [int(t0 + K <= S) for t0 in starts] and want.reached[-1] == 0


def test_ties_go_to_the_lower_column():
    L, S = 129, 6
    a = O.from_peaks([100] * S, L)
    a[0, [6, 70]] = 0.9                     # c and c + 64: the same lane, two chunks
    a[1, [70, 6]] = 0.9
    a[2, [10, 20]] = 0.9                    # within one chunk: two lanes
    a[3, [67, 128]] = 0.9                   # chunks 1 and 2
    a[4, :] = 0.25                          # every column
    a[5, [63, 64]] = 0.9                    # the last lane of a chunk and the first of the next
    got = _run(a[None], [L], 1)
    assert got.peak[0].tolist() == [6, 6, 10, 67, 0, 63]
    _check(got, a[None], [L], 1)


def test_short_run_at_the_last_step_is_no_detection():
    L, n = 8, 6
    for K in (2, 3, 5):
        S = 12
        cols = [0, 1, 2, 3, 4, 3, 3, 3, 3, 3, 3, 3]
        cols[S - (K - 1):] = [n - 1] * (K - 1)
        a = O.from_peaks(cols, L)[None]
        got = _run(a, [n], K)
        assert (got.end[0], got.reached[0]) == (S, 0)
        _check(got, a, [n], K)
        cols[S - K] = n - 1                                          # one more flagged step in front: K of them, end = S
        a = O.from_peaks(cols, L)[None]
        got = _run(a, [n], K)
        assert (got.end[0], got.reached[0]) == (S, 1)
        _check(got, a, [n], K)


def test_broken_run_then_a_full_one():
    L, n, K = 70, 66, 3
    cols = [0, 10, 65, 65, 20, 69, 65, 30, 65, 66, 67, 0, 65]
    a = O.from_peaks(cols, L)[None]
    got = _run(a, [n], K, 4)
    assert (got.end[0], got.reached[0], got.n_back[0], got.n_skip[0]) == (11, 1, 3, 4)
    _check(got, a, [n], K, 4)


@pytest.mark.parametrize('K', [1, 3])
def test_single_phone_ends_after_patience_steps(K):
    rs = np.random.RandomState(5)
    a = rs.rand(2, 9, 4).astype(np.float32)
    got = _run(a, [1, 1], K)
    assert got.end.tolist() == [K, K] and got.reached.tolist() == [1, 1]
    _check(got, a, [1, 1], K)


def test_non_finite_entries_are_flagged_and_peaks_stay_defined():
    rs = np.random.RandomState(6)
    L, S = 70, 9
    base = O.from_peaks(O.random_peaks(rs, S, L, 60), L, rs)
    some, allnan, inf, ninf, clean = (base.copy() for _ in range(5))
    some[2, ::3] = np.nan
    some[4, int(np.argmax(some[4]))] = np.nan                       # the peak itself: the runner-up wins
    allnan[3, :] = np.nan
    inf[1, 66] = np.inf
    ninf[5, :] = -np.inf
    a = np.stack([some, allnan, inf, ninf, clean])
    got = _run(a, [60] * 5, 2)
    assert got.nonfinite.tolist() == [1, 1, 1, 1, 0]
    assert got.peak[1, 3] == 0 and got.peak[2, 1] == 66 and got.peak[3, 5] == 0
    _check(got, a, [60] * 5, 2)


def test_sliced_view_is_read_in_place():
    """what text_to_speech returns: a slice of a larger tensor (row stride > L, batch stride > S * row stride); what lies around the
    slice -- larger values and NaN -- is not read"""
    rs = np.random.RandomState(8)
    B, S, L = 3, 11, 37
    a = np.stack([O.from_peaks(O.random_peaks(rs, S, L, n), L, rs) for n in (5, 20, 37)])
    big = np.full((B, S + 3, L + 5), 9.0, np.float32)
    big[:, 0] = np.nan
    big[:, 1:1 + S, 2:2 + L] = a
    t = torch.from_numpy(big).to(DEV)
    view = t[:, 1:1 + S, 2:2 + L]
    assert view.stride(1) > L and view.stride(0) > S * view.stride(1) and not view.is_contiguous()
    got = _run(view, [5, 20, 37])
    assert got.nonfinite.tolist() == [0, 0, 0]
    _check(got, a, [5, 20, 37])


def test_device_enc_len_is_clamped():
    rs = np.random.RandomState(9)
    S, L = 20, 12
    a = np.stack([O.from_peaks(O.random_peaks(rs, S, L, n), L, rs) for n in (1, 12, 7)])
    got = _run(a, torch.tensor([-4, 500, 7], device=DEV))
    _check(got, a, [1, 12, 7])
    _check(_run(a, torch.tensor([1, 12, 7], dtype=torch.int64, device=DEV)), a, [1, 12, 7])


def test_alone_and_inside_a_batch_are_bitwise_equal():
    rs = np.random.RandomState(10)
    S, L = 300, 90
    ns = [1, 30, 89, 90, 45]
    a = np.stack([O.from_peaks(O.random_peaks(rs, S, L, n), L, rs, peak_w=0.37 + 0.1 * i) for i, n in enumerate(ns)])
    for b in range(5):
        alone = _run(a[b:b + 1], ns[b:b + 1])
        batch = a.copy()
        batch[(b + 1) % 5] = np.nan                                  # a neighbour full of NaN
        inside = _run(batch, ns)
        for k in O.Result._fields:
            x, y = getattr(alone, k)[0], getattr(inside, k)[b]
            assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), (b, k)
        assert inside.nonfinite[(b + 1) % 5] == 1 and inside.nonfinite[b] == 0


def test_limit_violations_raise_before_the_launch():
    from semi_tts_amd.metrics import attention_endpoints
    a = torch.rand(2, 5, 4, device=DEV)
    for kw in (dict(align=a[:0], enc_len=[]), dict(align=a[:, :0], enc_len=[1, 1]), dict(align=a[:, :, :0], enc_len=[1, 1]),
               dict(align=torch.empty(1, 4097, 2, device=DEV), enc_len=[1]), dict(align=torch.empty(1, 2, 2049, device=DEV), enc_len=[1]),
               dict(align=a.transpose(1, 2), enc_len=[1, 1]), dict(align=a[:, :1].expand(2, 5, 4), enc_len=[1, 1]),
               dict(align=a.double(), enc_len=[1, 1]), dict(align=a.cpu(), enc_len=[1, 1]),
               dict(align=a, enc_len=[0, 1]), dict(align=a, enc_len=[1, 5]), dict(align=a, enc_len=[1]),
               dict(align=a, enc_len=torch.tensor([1.0, 1.0], device=DEV)),
               dict(align=a, enc_len=[1, 1], patience=0), dict(align=a, enc_len=[1, 1], max_jump=0)):
        with pytest.raises(ValueError):
            attention_endpoints(**kw)
