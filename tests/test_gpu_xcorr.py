"""st_xcorr_delay, st_sisdr_batch and st_wave_gather on the MI355X against the numpy oracle (tests/xcorr_oracle.py) on the guarded case
table (tests/xcorr_cases.py; tests/test_xcorr_host.py checks its guards on the CPU), and the layers above: metrics.delay / si_sdr /
align_pairs and main.py --stoi-align --stoi-sdr.

PCM input (multiples of 2^-15 up to 1): every product is a multiple of 2^-30 and every sum stays below 2^53 units, so corr and the six
sums must equal the int64 oracle BIT FOR BIT, the delay has no tolerance, and coef (one sqrt, one divide, one rounding on exact sums)
lies within 2 float32 ulps.  Float input: |corr - oracle| <= n 2^-53 sum |x_n y_{n+d}| per lag, the first-order bound of n exact
products added in any order (the oracle sums in longdouble, so its own error is 2^-11 of that); the host guard keeps every float
case's decision a factor 10^8 clear of it.  Scores on PCM: both sides evaluate the same float64 expression on identical sums,
what remains is log10 and one rounding: 4 * 2^-23 * max(1, |v|) dB."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_cases as SC        # noqa: E402
import xcorr_cases as XC       # noqa: E402
import xcorr_oracle as XO      # noqa: E402
from helpers import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
D_BATCH = XC.T + 1             # the bound of the batched runs: three lag tiles
SCORE_TOL = 4 * 2.0 ** -23


def _pack(sigs, gap=0, fill=0.0, reverse=False):
    """signals into one buffer with `gap` samples of `fill` around each, optionally laid out in reverse -> (device buffer, offsets)"""
    lens = [len(s) for s in sigs]
    order = list(range(len(sigs)))[::-1] if reverse else list(range(len(sigs)))
    off, pos = [0] * len(sigs), gap
    for i in order:
        off[i] = pos
        pos += lens[i] + gap
    buf = np.full(pos, fill, np.float32)
    for i, s in enumerate(sigs):
        buf[off[i]:off[i] + lens[i]] = s
    return torch.from_numpy(buf).to(DEV), np.array(off, np.int64)


def _run(cases, D, want_corr=True, **kw):
    from semi_tts_amd import ops
    x, xo = _pack([c['x'] for c in cases], **kw)
    y, yo = _pack([c['y'] for c in cases], **kw)
    return ops.xcorr_delay(x, xo, np.array([len(c['x']) for c in cases]), y, yo, np.array([len(c['y']) for c in cases]), D, want_corr)


_ALONE = {}


def alone(c, D=None):
    """(delay, coef, corr) of a case from a call of its own, computed once per bound"""
    D = c['D'] if D is None else D
    if (c['name'], D) not in _ALONE:
        _ALONE[(c['name'], D)] = _run([c], D)
    return _ALONE[(c['name'], D)]


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _ulps32(got, want):
    if np.isnan(want):
        return 0.0 if np.isnan(got) else np.inf
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))


# ---------------------------------------------------------------- the kernel against the oracle
@pytest.mark.parametrize('name', [c['name'] for c in XC.CASES if c['pcm']])
def test_pcm_case_is_bitwise_the_int64_oracle(name):
    c = XC.by_name(name)
    want = XC.oracle(c)
    delay, coef, corr = alone(c)
    got = corr[0].cpu().numpy()
    assert got.shape == (2 * c['D'] + 1,) and np.array_equal(_bits64(got), _bits64(want['corr'])), (name, np.abs(got - want['corr']).max())
    assert int(delay[0]) == want['delay'] and (c['shift'] is None or int(delay[0]) == c['shift']), (name, int(delay[0]), want['delay'])
    u = _ulps32(float(coef[0]), want['coef'])
    print('%s: delay %d coef %.7f (%.2f ulp)' % (name, int(delay[0]), float(coef[0]), u))
    assert u <= 2.0, (name, float(coef[0]), want['coef'])


@pytest.mark.parametrize('name', [c['name'] for c in XC.CASES if not c['pcm'] and not c['nan']])
def test_float_case_within_the_float64_bound(name):
    c = XC.by_name(name)
    want = XC.oracle(c)
    delay, coef, corr = alone(c)
    s, k = XO.corr_abs(c['x'], c['y'], c['D'])
    bound = k * 2.0 ** -53 * s
    err = np.abs(corr[0].cpu().numpy() - want['corr'])
    live = bound > 0
    print('%s: worst |corr - oracle| / bound %.3f, worst absolute %.3e' % (name, float((err[live] / bound[live]).max()), float(err.max())))
    assert (err <= bound).all(), (name, float((err[live] / bound[live]).max()))
    assert int(delay[0]) == want['delay'] == c['shift']


def test_limits_are_refused_before_a_launch_and_an_empty_batch_launches_nothing():
    import ctypes
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    assert lib.st_xcorr_workspace_bytes(0, 100, 1) == 0 and lib.st_xcorr_workspace_bytes(1, 100, ops.XCORR_MAX_LAG + 1) == 0
    assert lib.st_xcorr_workspace_bytes(1, 1, 0) >= 8 and lib.st_sisdr_workspace_bytes(1, 1) >= 40 and lib.st_sisdr_workspace_bytes(65, 1) == 0
    assert lib.st_xcorr_workspace_bytes(64, ops.XCORR_MAX_LEN, ops.XCORR_MAX_LAG) < 600e6          # modest at the limits
    x = torch.zeros(1000, device=DEV)
    p = x.data_ptr()
    keep = []

    def wave(lens, n=1000, B=None):
        off = (ctypes.c_long * len(lens))(*([0] * len(lens)))
        ln = (ctypes.c_int * len(lens))(*lens)
        keep.extend([off, ln])
        return _lib.StWaveBatch(x=p, n_samples=n, off=ctypes.cast(off, ctypes.c_void_p).value, len=ctypes.cast(ln, ctypes.c_void_p).value,
                                B=len(lens) if B is None else B)

    def call(lx, ly, D=1, **kw):
        return lib.st_xcorr_delay(ctypes.byref(wave(lx, **kw)), ctypes.byref(wave(ly, **kw)), D, p, p, None, p, None)
    assert call([10] * 65, [10] * 65) == -22 and b'batch 65' in lib.st_last_error()
    assert call([10, 10], [10]) == -22 and b'2 references and 1 processed' in lib.st_last_error()
    assert call([0], [10]) == -22 and call([10], [1001]) == -22 and b'processed signal 0' in lib.st_last_error()
    assert call([ops.XCORR_MAX_LEN + 1], [10], n=ops.XCORR_MAX_LEN + 1) == -22 and b'outside [1, 4194304]' in lib.st_last_error()
    assert call([10], [10], D=-1) == -22 and call([10], [10], D=ops.XCORR_MAX_LAG + 1) == -22 and b'max_lag 16385' in lib.st_last_error()
    assert lib.st_sisdr_batch(ctypes.byref(wave([10] * 65)), ctypes.byref(wave([10] * 65)), None, 1, p, p, p, None) == -22
    assert lib.st_sisdr_batch(ctypes.byref(wave([10])), ctypes.byref(wave([1001])), None, 1, p, p, p, None) == -22
    assert call([10], [10], B=0) == 0                               # nothing is launched, nothing written
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
    e = np.zeros(0, np.int64)
    delay, coef, corr = ops.xcorr_delay(x, e, e, x, e, e, 3, want_corr=True)
    assert delay.shape == (0,) and coef.shape == (0,) and corr.shape == (0, 7)
    assert ops.sisdr_batch(x, e, e, x, e, e)[1].shape == (0, 6)


# ---------------------------------------------------------------- batching
@pytest.mark.parametrize('reverse', [False, True])
def test_a_batch_of_all_cases_is_bitwise_what_each_gives_alone(reverse):
    cases = XC.CASES[::-1] if reverse else XC.CASES
    delay, coef, corr = _run(cases, D_BATCH)
    d2, c2, none = _run(cases, D_BATCH, want_corr=False)
    assert none is None and torch.equal(delay, d2) and same_bits(coef, c2)
    for b, c in enumerate(cases):
        d, k, r = alone(c, D_BATCH)
        assert int(delay[b]) == int(d[0]) and same_bits(coef[b], k[0]) and same_bits(corr[b], r[0]), c['name']
        # a lag's sum does not depend on the bound either: the columns of the case's own run are the middle of these
        own = alone(c)[2][0]
        assert same_bits(corr[b, D_BATCH - c['D']:D_BATCH + c['D'] + 1], own), c['name']


@pytest.mark.parametrize('B', [64, 65])
def test_metrics_delay_chunks_past_64_pairs(B):
    from semi_tts_amd.metrics import delay
    cases = [XC.CASES[(5 * i) % len(XC.CASES)] for i in range(B)]
    res = delay([torch.from_numpy(c['x']) for c in cases], [c['y'] for c in cases], 37, want_corr=(B == 65))
    assert res.delay.shape == (B,) and res.delay.dtype == torch.int32 and res.coef.is_cuda and (res.corr is None) == (B == 64)
    for b, c in enumerate(cases):                                   # the caller's order, whatever the two sorts by length did
        d, k, r = alone(c, 37)
        assert int(res.delay[b]) == int(d[0]) and same_bits(res.coef[b], k[0]), (b, c['name'])
        if B == 65:
            assert same_bits(res.corr[b], r[0]), (b, c['name'])


def test_metrics_delay_and_si_sdr_do_no_host_read(monkeypatch):
    from semi_tts_amd import metrics
    c = XC.by_name('Lx>Ly/+D')
    x, y = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['y']).to(DEV)

    def read(*a, **k):
        raise AssertionError('a host read')
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__int__', '__float__'):
        monkeypatch.setattr(torch.Tensor, name, read)
    res = metrics.delay([x, x], [y, x], 40)
    sd = metrics.si_sdr([x, x], [y, x], res.delay)
    monkeypatch.undo()
    assert res.delay.tolist() == [37, 0] and sd.sums[:, 0].tolist() == [float(len(c['y']) - 37), float(len(c['x']))]
    assert float(res.coef[1]) == 1.0


def test_int16_counts_as_pcm():
    from semi_tts_amd.metrics import delay
    c = XC.by_name('Lx<Ly/-D')
    i16 = lambda v: torch.from_numpy(np.rint(v.astype(np.float64) * 32768.0).astype(np.int16))      # noqa: E731
    res = delay([i16(c['x'])], [i16(c['y'])], c['D'], want_corr=True)
    d, k, r = alone(c)
    assert int(res.delay[0]) == -37 and same_bits(res.coef, k) and same_bits(res.corr, r)


# ---------------------------------------------------------------- buffers and NaN
def test_nan_neighbours_and_windows_change_no_bit():
    from semi_tts_amd import ops
    for c in (XC.by_name('Lx>Ly/+D'), XC.by_name('C+1/D=T+1/0'), XC.by_name('f/MC+1/D=3')):
        d, k, r = alone(c)
        nan = dict(x=np.full(700, np.nan, np.float32), y=np.full(900, np.nan, np.float32))
        trio = [nan, c, nan]
        # packed between two NaN neighbours, with NaN gaps around every signal, laid out in reverse (non-cumulative offsets)
        for kw in (dict(), dict(gap=777, fill=np.nan), dict(gap=13, fill=np.nan, reverse=True)):
            x, xo = _pack([t['x'] for t in trio], **kw)
            y, yo = _pack([t['y'] for t in trio], **kw)
            delay, coef, corr = ops.xcorr_delay(x, xo, [len(t['x']) for t in trio], y, yo, [len(t['y']) for t in trio], c['D'], True)
            assert int(delay[1]) == int(d[0]) and same_bits(coef[1], k[0]) and same_bits(corr[1], r[0]), (c['name'], kw)
            assert delay[[0, 2]].tolist() == [0, 0] and bool(torch.isnan(coef[[0, 2]]).all())


def test_a_nan_case_gives_delay_0_and_coef_nan_and_leaves_the_others():
    n = XC.by_name('nan-x')
    a, b = XC.by_name('2C+1/D=1/+D'), XC.by_name('Lx<Ly/-D')
    delay, coef, corr = _run([a, n, b], 40)
    assert int(delay[1]) == 0 and bool(torch.isnan(coef[1]))
    want = XC.oracle(n, 40)['corr']
    got = corr[1].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any() and not np.isnan(want).all()
    ok = ~np.isnan(want)
    s, k = XO.corr_abs(np.nan_to_num(n['x']), n['y'], 40)
    assert (np.abs(got[ok] - want[ok]) <= (k * 2.0 ** -53 * s)[ok]).all()
    for row, c in ((0, a), (2, b)):
        d, k, r = alone(c, 40)
        assert int(delay[row]) == int(d[0]) and same_bits(coef[row], k[0]) and same_bits(corr[row], r[0]), c['name']
    # an infinity where no lag's range reaches it (past Ly + D) spoils coef through sum x^2 but no r
    c = XC.by_name('Lx>Ly/+D')
    x = c['x'].copy()
    x[len(c['y']) + 60] = np.inf
    delay, coef, corr = _run([dict(c, x=x)], 37)
    assert same_bits(corr, alone(c)[2]) and int(delay[0]) == 37 and float(coef[0]) == 0.0


# ---------------------------------------------------------------- SI-SDR
def _sisdr(cases, delay, zero_mean):
    from semi_tts_amd import ops
    x, xo = _pack([c['x'] for c in cases])
    y, yo = _pack([c['y'] for c in cases])
    d = None if delay is None else torch.tensor(delay, dtype=torch.int32, device=DEV)
    return ops.sisdr_batch(x, xo, [len(c['x']) for c in cases], y, yo, [len(c['y']) for c in cases], d, zero_mean)


def _score_ok(got, want, name):
    for g, w in zip(got, want):
        if np.isfinite(w):
            assert abs(float(g) - w) <= SCORE_TOL * max(1.0, abs(w)), (name, got, want)
        else:
            assert (np.isnan(w) and np.isnan(g)) or float(g) == w, (name, got, want)


@pytest.mark.parametrize('zero_mean', [False, True])
def test_sisdr_on_the_case_table(zero_mean):
    cases = [c for c in XC.CASES if not c['nan'] and (c['zero_mean'] or not zero_mean)]
    delays = [XC.oracle(c)['delay'] for c in cases]
    score, sums = _sisdr(cases, delays, zero_mean)
    score, sums = score.cpu().numpy(), sums.cpu().numpy()
    worst = 0.0
    for b, c in enumerate(cases):
        want = XO.sums(c['x'], c['y'], delays[b])
        if c['pcm']:
            assert np.array_equal(_bits64(sums[b]), _bits64(want)), (c['name'], sums[b], want)
            _score_ok(score[b], XO.scores(want, zero_mean), c['name'])
            fin = np.isfinite(XO.scores(want, zero_mean))
            worst = max([worst] + list(np.abs(score[b][fin] - XO.scores(want, zero_mean)[fin])))
        else:
            bound = XO.sums_bound(c['x'], c['y'], delays[b])
            assert sums[b, 0] == want[0] and (np.abs(sums[b, 1:] - want[1:]) <= bound).all(), (c['name'], sums[b] - want, bound)
    print('zero_mean %s: worst PCM score deviation %.3e dB' % (zero_mean, worst))
    one = _sisdr([XC.by_name('dc')], [delays[[c['name'] for c in cases].index('dc')]], zero_mean)          # a pair alone: the same bits
    b = [c['name'] for c in cases].index('dc')
    assert np.array_equal(_bits64(one[1][0].cpu().numpy()), _bits64(sums[b])) and np.array_equal(one[0][0].cpu().numpy().view(np.int32), score[b].view(np.int32))


def test_sisdr_special_values():
    c = XC.by_name('Lx>Ly/+D')
    x = c['x']
    half = dict(x=x, y=(0.5 * x).astype(np.float32))
    silent = dict(x=np.zeros(500, np.float32), y=x[:500])
    score, sums = _sisdr([half, silent, c, c], [0, 0, len(c['y']), -len(c['x']) - 7], False)
    s = score.cpu().numpy()
    assert s[0, 0] == np.inf and abs(s[0, 1] - 6.0206) < 1e-4 and abs(s[0, 2] + 6.0206) < 1e-4
    assert np.isnan(s[1, 0]) and s[1, 1] == -np.inf and np.isnan(s[1, 2])             # a silent reference
    assert np.isnan(s[2:]).all() and (sums[2:].cpu().numpy() == 0).all()              # a delay longer than a side: n = 0
    assert np.isnan(_sisdr([silent], None, True)[0][0, 0].item())


def test_a_device_delay_and_a_host_int_give_the_same_bits():
    from semi_tts_amd import metrics
    cases = [XC.by_name('Lx>Ly/+D'), XC.by_name('f/Lx>Ly/+D'), XC.by_name('dc')]
    xs, ys = [c['x'] for c in cases], [c['y'] for c in cases]
    for d in (37, 0, -5, 5000):
        a = metrics.si_sdr(xs, ys, d)
        b = metrics.si_sdr(xs, ys, torch.full((3,), d, dtype=torch.int32, device=DEV))
        assert same_bits(a.score, b.score) and same_bits(a.sums, b.sums), d
        if d == 0:
            n = metrics.si_sdr(xs, ys)
            assert same_bits(a.score, n.score) and same_bits(a.sums, n.sums)
    for i, c in enumerate(cases):                                   # the caller's order, against the oracle's sums
        assert a.sums[i, 0].item() == max(0, XO.overlap(len(c['x']), len(c['y']), 5000)[2])
    found = metrics.delay(xs, ys, 40)
    got = metrics.si_sdr(xs, ys, found.delay)
    for i, c in enumerate(cases):
        want = XO.sums(c['x'], c['y'], int(found.delay[i]))
        if c['pcm']:
            assert np.array_equal(_bits64(got.sums[i].cpu().numpy()), _bits64(want)), c['name']


# ---------------------------------------------------------------- wave_gather and align_pairs
def test_wave_gather_copies_the_spans_and_nothing_else():
    from semi_tts_amd import ops
    rs = np.random.RandomState(3)
    src = torch.from_numpy(rs.randn(40000).astype(np.float32)).to(DEV)
    lens = np.array([1, 2, 1023, 1024, 1025, 4097, 20000, 7], np.int64)
    so = np.array([39999, 5, 100, 2000, 3100, 5000, 10000, 0], np.int64)
    do = np.array([3, 10, 20, 1100, 2200, 3300, 7500, 27600], np.int64)
    dst = torch.full((27700,), -12345.0, device=DEV)
    out = ops.wave_gather(src, so, dst, do, lens)
    assert out is dst
    written = torch.zeros(27700, dtype=torch.bool, device=DEV)
    for a, b, n in zip(so, do, lens):
        assert same_bits(dst[b:b + n], src[a:a + n])
        written[b:b + n] = True
    assert bool((dst[~written] == -12345.0).all()) and int((~written).sum()) == 27700 - int(lens.sum())
    assert ops.wave_gather(src, [], dst, [], []) is dst


def test_align_pairs_returns_the_callers_order_though_the_cuts_reorder():
    from semi_tts_amd import metrics
    a, b, c = XC.by_name('Lx>Ly/+D'), XC.by_name('2C+1/D=1/+D'), XC.by_name('Lx<Ly/-D')
    # before the cut the x sort longest first as (a, b, c); the overlaps are 1087, 2048 and 986 samples: (b, a, c)
    cx, cy, delay, coef = metrics.align_pairs([a['x'], b['x'], c['x']], [a['y'], b['y'], c['y']], 37)
    assert delay.tolist() == [37, 1, -37]
    assert cx.order.tolist() == [1, 0, 2] == cy.order.tolist() and cx.lens.tolist() == [2048, 1087, 986] == cy.lens.tolist()
    assert np.array_equal(cx.offsets, cy.offsets) and cx.offsets.tolist() == [0, 2048, 3135]
    px, py = cx.packed(torch.device(DEV)), cy.packed(torch.device(DEV))
    assert px.numel() == py.numel() == 2048 + 1087 + 986
    for row, (case, d) in zip((1, 0, 2), ((a, 37), (b, 1), (c, -37))):
        x0, y0, n = XO.overlap(len(case['x']), len(case['y']), d)
        o = int(cx.offsets[row])
        assert same_bits(px[o:o + n], torch.from_numpy(case['x'][x0:x0 + n])) and same_bits(py[o:o + n], torch.from_numpy(case['y'][y0:y0 + n]))
    sd = metrics.si_sdr(cx, cy)                                     # the cut batches score in the caller's order too
    full = metrics.si_sdr([a['x'], b['x'], c['x']], [a['y'], b['y'], c['y']], delay)
    assert same_bits(sd.sums, full.sums) and same_bits(sd.score, full.score)
    # two pairs with EQUAL overlaps, either way round: ties keep the caller's order, and every row still comes back in its place
    a2 = dict(a, x=(0.5 * a['x']).astype(np.float32), y=(0.25 * a['y']).astype(np.float32))
    for quad, want_order in (([a, b, a2, c], [1, 0, 2, 3]), ([a2, c, a, b], [3, 0, 2, 1])):
        xs, ys = [q['x'] for q in quad], [q['y'] for q in quad]
        cx, cy, delay, coef = metrics.align_pairs(xs, ys, 37)
        assert cx.order.tolist() == want_order == cy.order.tolist() and np.array_equal(cx.offsets, cy.offsets)
        sd, full = metrics.si_sdr(cx, cy, zero_mean=False), metrics.si_sdr(xs, ys, delay, zero_mean=False)
        assert same_bits(sd.sums, full.sums) and same_bits(sd.score, full.score)
        ia, ia2 = (next(i for i, q in enumerate(quad) if q is t) for t in (a, a2))
        assert float(full.sums[ia, 3]) == 4.0 * float(full.sums[ia2, 3]) and full.sums[ia, 0] == full.sums[ia2, 0] == 1087
        px = cx.packed(torch.device(DEV))
        for row, i in enumerate(want_order):                        # the buffer holds the overlaps in the order the batch states
            d = int(delay[i])
            x0, _, n = XO.overlap(len(quad[i]['x']), len(quad[i]['y']), d)
            o = int(cx.offsets[row])
            assert same_bits(px[o:o + n], torch.from_numpy(quad[i]['x'][x0:x0 + n])), (row, i)
    with pytest.raises(ValueError, match='pair 0: the best lag .* leaves no overlap'):
        metrics.align_pairs([np.full(4, 0.5, np.float32)], [np.full(4, -0.5, np.float32)], 8)      # every overlapping lag is negative: +4 wins


# ---------------------------------------------------------------- end to end: shifted STOI pairs
def _shift(y, s):
    out = np.zeros_like(y)
    if s >= 0:
        out[s:] = y[:len(y) - s]
    else:
        out[:s] = y[-s:]
    return out


def test_stoi_of_aligned_pairs_is_bitwise_stoi_of_the_host_cut_and_the_unaligned_score_is_lower():
    import test_gpu_stoi as TS
    from semi_tts_amd import metrics
    names = ('L7000/snr5', 'L30000/snr20', 'L37000/burst')
    shifts = (-37, 0, 64)
    xs, ys, cut_x, cut_y = [], [], [], []
    for name in names:
        c = SC.by_name(name)
        for s in shifts:
            y = _shift(c['y'], s)
            x0, y0, n = XO.overlap(c['L'], c['L'], s)
            xs.append(c['x']), ys.append(y), cut_x.append(c['x'][x0:x0 + n].copy()), cut_y.append(y[y0:y0 + n].copy())
    cx, cy, delay, coef = metrics.align_pairs(xs, ys, 100)
    assert delay.tolist() == list(shifts) * 3
    got = metrics.stoi(cx, cy, 10000)
    want = metrics.stoi(cut_x, cut_y, 10000)
    assert same_bits(got.score, want.score) and torch.equal(got.counts, want.counts)
    raw = metrics.stoi(xs, ys, 10000)
    _, es = TS.e32()
    for i in (2, 5, 8):                                             # the s = 64 pairs
        a, u = got.score[i].tolist(), raw.score[i].tolist()
        print('%s shifted by 64: aligned STOI %.6f ESTOI %.6f, unaligned %.6f %.6f (bound %.3e)' % (names[i // 3], a[0], a[1], u[0], u[1], TS.FACTOR * es))
        assert a[0] - u[0] > TS.FACTOR * es and a[1] - u[1] > TS.FACTOR * es
    for i in (1, 4, 7):                                             # s = 0: nothing is cut, the scores are those of before
        assert same_bits(got.score[i], raw.score[i])


# ---------------------------------------------------------------- CLI
def test_main_stoi_align_sdr_writes_the_three_tables_and_changes_nothing_without_the_flags(tmp_path):
    from semi_tts_amd.audio import write_wav
    from semi_tts_amd.solver import StoiScorer
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    planted = {'a-pred.wav': 64, 'b.wav': -37, 'c.wav': 0}
    pcm = lambda v: np.rint(np.clip(v.astype(np.float64), -1.0, 1.0) * 32767.0) / 32768.0      # noqa: E731
    want = {}
    for (fname, s), case, cut in zip(planted.items(), ('L7000/snr5', 'L4225/snr5', 'L4097/snr20'), (0, 30, 0)):
        c = SC.by_name(case)
        y = _shift(c['y'], s)[:c['L'] - cut]
        write_wav(str(syn / fname), y, 10000)
        write_wav(str(ref / fname.replace('-pred', '')), c['x'], 10000)
        x0, y0, n = XO.overlap(c['L'], len(y), s)
        want[fname] = (n, XO.scores(XO.sums(pcm(c['x']), pcm(y), s), True))

    def run(name, *flags):
        r = subprocess.run([sys.executable, os.path.join(REPO, 'main.py'), '--stoi-wav-dir', str(syn), '--stoi-ref-dir', str(ref), '--logdir',
                            str(tmp_path / 'log'), '--name', name] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                           cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout
        return r.stdout, tmp_path / 'log' / name
    out, d = run('aligned', '--stoi-align', '--stoi-sdr', '--stoi-max-delay', '0.0064')
    assert 'mean |delay| %.6f s' % ((64 + 37) / 3 / 10000.0) in out and 'mean SI-SDR' in out, out
    assert '[WARNING]' in out and 'the best lag of a-pred.wav, 64 samples, sits on the search bound of +-64 samples' in out, out
    delay = open(str(d / 'delay.csv')).read().split('\n')
    assert delay[0] == 'file,delay_samples,delay_s,coef' and len(delay) == 5 and delay[4] == ''
    sdr = open(str(d / 'sdr.csv')).read().split('\n')
    assert sdr[0] == 'file,samples,si_sdr,snr,gain_db' and len(sdr) == 5
    stoi = open(str(d / 'stoi.csv')).read().split('\n')
    assert stoi[0] == 'file,samples,frames,kept,segments,stoi,estoi' and len(stoi) == 5
    for i, (fname, s) in enumerate(planted.items()):
        f = delay[1 + i].split(',')
        assert f[0] == fname and int(f[1]) == s and float(f[2]) == s / 10000.0 and 0.5 < float(f[3]) <= 1.0, delay[1 + i]
        n, sc = want[fname]
        g = sdr[1 + i].split(',')
        assert g[0] == fname and int(g[1]) == n and all(abs(float(v) - w) <= 1e-4 for v, w in zip(g[2:], sc)), (sdr[1 + i], sc)
        assert stoi[1 + i].split(',')[:2] == [fname, str(n)]
    _, plain = run('plain')                                         # without the flags: byte for byte the unchanged path
    assert sorted(os.listdir(str(plain))) == ['stoi.csv']
    paras = types.SimpleNamespace(stoi_wav_dir=str(syn), stoi_ref_dir=str(ref), stoi_max_len_diff=0.05, batch_size=32, name='direct',
                                  logdir=str(tmp_path / 'log'), verbose=False)
    assert StoiScorer(None, paras, 'test').load_data().set_model().exec() == 3
    assert open(str(plain / 'stoi.csv'), 'rb').read() == open(str(tmp_path / 'log' / 'direct' / 'stoi.csv'), 'rb').read()
    assert open(str(plain / 'stoi.csv')).read() != open(str(d / 'stoi.csv')).read()
