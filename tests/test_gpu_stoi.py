"""st_stoi_batch on the MI355X against the float64 oracle (tests/stoi_oracle.py) on the guarded case table (tests/stoi_cases.py:
tests/test_stoi_host.py checks on the CPU that every case keeps 0.01 dB from the silent-frame threshold), and the layers above it:
metrics.stoi (chunks, rates) and main.py --stoi-wav-dir.

Frame norms: an fp32 sum of n non-negative terms in any order lies within (n - 1) u of the exact one to first order, the products and
the squares add a rounding each and the root halves it all: |got - want| <= (256 + 8) 2^-24 want, the bound of tests/test_gpu_trim.py.

Bands and scores: no closed form leads through the FFT and the two normalisations, so the bound is measured against the oracle's own
float32 form.  e32 = the largest deviation of stoi_oracle.stoi(dtype=float32) from the float64 form over the case table (bands:
relative to the pair's largest band value; scores: absolute, both measures together); the GPU may deviate by FACTOR = 8 times that, the
factor tests/test_gpu_audio_edges.py grants a different summation order of the same float32 steps.  The test computes e32 itself, so the
bound follows the cases; DESIGN.md 3.24 records the values."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as RO   # noqa: E402
import stoi_cases as SC        # noqa: E402
import stoi_oracle as SO       # noqa: E402
from helpers import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
FACTOR = 8.0
NORM_TOL = (SO.N_FRAME + 8) * 2.0 ** -24


def _band_dev(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / want.max()) if want.size else 0.0


def _score_dev(got, want):
    return float(max(abs(float(a) - b) for a, b in zip(got, want)))


_E32 = {}


def e32():
    """(bands, scores): the float32 numpy form's largest deviation from the float64 form over the case table"""
    if not _E32:
        pairs = [(SC.oracle(c, np.float32), SC.oracle(c)) for c in SC.CASES]
        _E32['bands'] = max(_band_dev(a['bands'], b['bands']) for a, b in pairs)
        _E32['score'] = max(_score_dev(a['score'], b['score']) for a, b in pairs if b['counts'][3] > 0)
        print('stoi e32: bands %.3e scores %.3e' % (_E32['bands'], _E32['score']))
    return _E32['bands'], _E32['score']


def _run(cases, F_pad=None):
    """one ops.stoi_batch call on `cases` packed back to back -> host (score, counts, energy, kept, bands) and the device scores"""
    from semi_tts_amd import ops
    lens = np.array([c['L'] for c in cases], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    x = torch.from_numpy(np.concatenate([c['x'] for c in cases])).to(DEV)
    y = torch.from_numpy(np.concatenate([c['y'] for c in cases])).to(DEV)
    return ops.stoi_batch(x, y, off, lens, F_pad, want_parts=True)


_ALONE = {}


def alone(c):
    """a case's five device outputs from a call of its own, computed once"""
    if c['name'] not in _ALONE:
        _ALONE[c['name']] = _run([c])
    return _ALONE[c['name']]


def _check(name, want, score, counts, energy, kept, bands, eb, es, worst):
    """one pair's rows against a float64 result: norms within NORM_TOL, integers equal, bands and scores within FACTOR * e32"""
    F, K, M, S = want['counts']
    assert counts.tolist() == [F, K, M, S], (name, counts.tolist(), want['counts'])
    e = energy.double().cpu().numpy()
    assert (np.abs(e[:F] - want['norms']) <= NORM_TOL * want['norms']).all(), (name, float(np.abs(e[:F] - want['norms']).max()))
    assert (e[F:] == 0).all(), name
    k = kept.cpu().numpy()
    assert k[:K].tolist() == want['kept'].tolist() and (k[K:] == -1).all(), name
    b = bands.cpu().numpy()
    assert (b[:, :, M:] == 0).all(), name
    db = _band_dev(b[:, :, :M], want['bands'])
    worst['bands'] = max(worst.get('bands', 0.0), db)
    print('%s: counts %s bands %.3e of %.3e' % (name, want['counts'], db, FACTOR * eb), end='')
    assert db <= FACTOR * eb, (name, db, FACTOR * eb)
    s = score.cpu().numpy()
    if S == 0:
        assert s.tolist() == [np.float32(SO.SENTINEL)] * 2, (name, s.tolist())
        print()
    else:
        ds = _score_dev(s, want['score'])
        worst['score'] = max(worst.get('score', 0.0), ds)
        print(' scores %.6f %.6f dev %.3e of %.3e' % (s[0], s[1], ds, FACTOR * es))
        assert ds <= FACTOR * es, (name, ds, FACTOR * es, s.tolist(), want['score'])


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize('L', [L for L, _, _ in SC.LENGTHS])
def test_every_case_alone_against_float64(L):
    """F = 0; F = 1 with M = 0; M = 29 (the sentinel); exactly one segment; two; gaps; kept frames across the scan chunk -- each
    undegraded, under noise at 20, 5 and -5 dB and under a burst (cases that clip in rule 7 and cases that do not)"""
    eb, es = e32()
    worst = {}
    for c in [c for c in SC.CASES if c['L'] == L]:
        _check(c['name'], SC.oracle(c), *[t[0] for t in alone(c)], eb, es, worst)
    print('L%d worst: %s' % (L, worst))


def test_limits_are_refused_before_a_launch_and_an_empty_batch_launches_nothing():
    import ctypes
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    assert [lib.st_stoi_frames(L) for L in (0, 1, 256, 257, 4096, 4097, ops.STOI_MAX_LEN, ops.STOI_MAX_LEN + 1)] == [-1, 0, 0, 1, 30, 31, 32766, -1]
    assert lib.st_stoi_workspace_floats(0, 4) == 0 and lib.st_stoi_workspace_floats(1, 1) >= 36
    x = torch.zeros(1000, device=DEV)
    p = x.data_ptr()

    def call(lens, B=None, F_pad=8, n=1000):
        off = (ctypes.c_long * len(lens))(*([0] * len(lens)))
        ln = (ctypes.c_int * len(lens))(*lens)
        w = _lib.StWaveBatch(x=p, n_samples=n, off=ctypes.cast(off, ctypes.c_void_p).value, len=ctypes.cast(ln, ctypes.c_void_p).value,
                             B=len(lens) if B is None else B)
        return lib.st_stoi_batch(ctypes.byref(w), p, p, p, F_pad, None, None, None, p, None)
    assert call([100] * 65) == -22 and b'batch 65' in lib.st_last_error()
    assert call([1001]) == -22 and call([0]) == -22
    assert call([ops.STOI_MAX_LEN + 1], n=ops.STOI_MAX_LEN + 1) == -22 and b'above the limit' in lib.st_last_error()
    assert call([1000], F_pad=5) == -22 and b'F_pad 5 below the 6 frames' in lib.st_last_error()
    assert call([1000], F_pad=0) == -22
    assert call([100], B=0) == 0                                    # nothing is launched, nothing written
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
    score, counts, energy, kept, bands = ops.stoi_batch(x, x.clone(), [], [], want_parts=True)
    assert score.shape == (0, 2) and counts.shape == (0, 4) and bands.shape == (0, 2, 15, 1)


# ---------------------------------------------------------------- raggedness
def test_the_whole_table_in_one_call_in_a_permuted_order_is_bitwise_what_each_pair_gives_alone():
    order = np.random.RandomState(5).permutation(len(SC.CASES))
    cases = [SC.CASES[i] for i in order]
    assert len(cases) <= 64
    outs = _run(cases, F_pad=301)                                   # (a wider padding than any pair's own call has)
    for b, c in enumerate(cases):
        F, K, M, _ = SC.oracle(c)['counts']
        s, n, e, k, bd = alone(c)
        assert same_bits(outs[0][b], s[0]) and torch.equal(outs[1][b], n[0]), c['name']
        assert same_bits(outs[2][b, :F], e[0, :F]) and torch.equal(outs[3][b, :K], k[0, :K]) and same_bits(outs[4][b, :, :, :M], bd[0, :, :, :M]), c['name']
        assert bool((outs[2][b, F:] == 0).all()) and bool((outs[3][b, K:] == -1).all()) and bool((outs[4][b, :, :, M:] == 0).all()), c['name']


@pytest.mark.parametrize('B', [64, 65])
def test_metrics_stoi_chunks_past_64_pairs(B):
    from semi_tts_amd.metrics import stoi
    cases = [SC.CASES[(7 * i) % len(SC.CASES)] for i in range(B)]
    res = stoi([torch.from_numpy(c['x']) for c in cases], [c['y'] for c in cases], 10000, want_parts=(B == 65))
    assert res.score.shape == (B, 2) and res.counts.shape == (B, 4) and res.score.is_cuda
    for b, c in enumerate(cases):                                   # the caller's order, whatever the sort by length did
        s, n, e, k, bd = alone(c)
        assert same_bits(res.score[b], s[0]) and torch.equal(res.counts[b], n[0]), (b, c['name'])
        if B == 65:
            F, K, M, _ = SC.oracle(c)['counts']
            assert same_bits(res.bands[b, :, :, :M], bd[0, :, :, :M]) and torch.equal(res.kept[b, :K], k[0, :K]), (b, c['name'])
    assert (res.energy is None) == (B == 64)


def test_metrics_stoi_does_no_host_read(monkeypatch):
    from semi_tts_amd.metrics import stoi
    c = SC.by_name('L30000/snr5')
    x, y = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['y']).to(DEV)
    stoi([x], [y], 16000)                                           # (tables uploaded, caches warm)

    def read(*a, **k):
        raise AssertionError('a host read')
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__int__', '__float__'):
        monkeypatch.setattr(torch.Tensor, name, read)
    res = stoi([x, x], [y, x], 16000, want_parts=True)
    monkeypatch.undo()
    assert res.score.is_cuda and abs(float(res.score[1, 0]) - 1.0) < 1e-5


# ---------------------------------------------------------------- rates
def _resample32(x, sr):
    """the float32 form of the resampler: the float32 table, float32 products, one float32 chain over ascending taps"""
    o, n, taps, first, tab, _ = RO.table64(sr, SO.FS)
    tab = tab.astype(np.float32)
    L, M = len(x), RO.out_len(len(x), sr, SO.FS)
    m = np.arange(M, dtype=np.int64)
    p = m % n
    idx = (m * o // n + first[p])[:, None] + np.arange(taps)[None, :]
    xv = np.where((idx >= 0) & (idx < L), x[np.clip(idx, 0, L - 1)], np.float32(0))
    out = np.zeros(M, np.float32)
    for k in range(taps):
        out += tab[p, k] * xv[:, k]
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize('sr, name', [(16000, 'L37000/snr5'), (16000, 'L30000/burst'), (22050, 'L30000/snr5'), (22050, 'L37000/snr20')])
def test_other_rates_go_through_the_resampler(sr, name):
    """the case's samples taken as a recording at 16000 / 22050 Hz: metrics.stoi against the float64 resampling oracle composed with the
    float64 STOI oracle.  e32 here is the deviation of the composed float32 forms (the resampler's float32 form above, then
    stoi_oracle's) from the composed float64 forms on this very pair, or the case table's e32 where that is larger: one pair is a
    single draw of the float32 error of the STOI steps, which the table sizes over forty.  The bound is FACTOR times it, as above."""
    from semi_tts_amd.metrics import stoi
    c = SC.by_name(name)
    x64, y64 = RO.resample_compact(c['x'], sr, SO.FS), RO.resample_compact(c['y'], sr, SO.FS)
    assert SO.margin_db(x64) >= SC.MARGIN_DB                        # the guard, on the resampled signal
    want = SO.stoi(x64, y64)
    want32 = SO.stoi(_resample32(c['x'], sr), _resample32(c['y'], sr), np.float32)
    assert want32['counts'] == want['counts'] and want['counts'][3] >= 1
    assert 0.0 < want['clipped'] < 1.0 or c['deg'] == 'snr20'
    eb, es = (max(t, p) for t, p in zip(e32(), (_band_dev(want32['bands'], want['bands']), _score_dev(want32['score'], want['score']))))
    res = stoi([c['x']], [c['y']], sr, want_parts=True)
    F, K, M, S = want['counts']
    assert res.counts[0].tolist() == [F, K, M, S]
    assert res.kept[0, :K].tolist() == want['kept'].tolist()
    db, ds = _band_dev(res.bands[0, :, :, :M].cpu().numpy(), want['bands']), _score_dev(res.score[0].cpu().numpy(), want['score'])
    print('%d Hz %s: counts %s bands %.3e of %.3e scores dev %.3e of %.3e' % (sr, name, want['counts'], db, FACTOR * eb, ds, FACTOR * es))
    assert db <= FACTOR * eb and ds <= FACTOR * es, (db, FACTOR * eb, ds, FACTOR * es)


# ---------------------------------------------------------------- non-finite input and silence
def test_nan_gives_nan_and_leaves_the_neighbours_untouched():
    a, b, c = SC.by_name('L7000/snr20'), SC.by_name('L30000/snr5'), SC.by_name('L4225/burst')
    bad_x = dict(b, x=b['x'].copy())
    bad_x['x'][12345] = np.nan                                      # NaN in the clean signal
    kept = SC.oracle(a)['kept']
    bad_y = dict(a, y=a['y'].copy())
    bad_y['y'][128 * int(kept[7]) + 200] = np.nan                   # NaN in a kept frame of the processed one
    inf_x = dict(c, x=c['x'].copy())
    inf_x['x'][1000] = np.inf
    score, counts, energy, kept_d, bands = _run([a, bad_x, c, bad_y, b, inf_x])
    torch.cuda.synchronize()
    assert bool(torch.isnan(score[1]).all()) and counts[1].tolist() == [233, 0, 0, 0] and bool((kept_d[1] == -1).all())
    assert bool(torch.isnan(score[5]).all()) and counts[5].tolist() == [32, 0, 0, 0]
    assert bool(torch.isnan(score[3]).all()) and counts[3].tolist() == list(SC.oracle(a)['counts'])
    for row, case in ((0, a), (2, c), (4, b)):
        s, n, _, _, bd = alone(case)
        M = SC.oracle(case)['counts'][2]
        assert same_bits(score[row], s[0]) and torch.equal(counts[row], n[0]) and same_bits(bands[row, :, :, :M], bd[0, :, :, :M]), case['name']


def test_digital_silence_scores_zero():
    c = SC.by_name('L7000/snr5')
    z = np.zeros_like(c['x'])
    score, counts, _, _, _ = _run([dict(c, y=z), dict(c, x=z), dict(c, x=z, y=z), c])
    assert score[:3].tolist() == [[0.0, 0.0]] * 3
    assert counts[0].tolist() == list(SC.oracle(c)['counts']) and counts[1].tolist() == [53, 53, 52, 23] == counts[2].tolist()
    assert same_bits(score[3], alone(c)[0][0])


# ---------------------------------------------------------------- end to end
def test_main_stoi_wav_dir_writes_the_oracles_rows(tmp_path):
    from semi_tts_amd.audio import write_wav
    syn, ref = tmp_path / 'syn', tmp_path / 'ref'
    syn.mkdir()
    ref.mkdir()
    want = {}
    pcm = lambda v: np.rint(np.clip(v.astype(np.float64), -1.0, 1.0) * 32767.0) / 32768.0      # noqa: E731
    for fname, case, sr, cut in (('a-pred.wav', 'L7000/snr5', 10000, 0), ('b.wav', 'L4096/snr20', 10000, 0), ('c.wav', 'L30000/burst', 16000, 40)):
        c = SC.by_name(case)
        write_wav(str(syn / fname), c['y'][:c['L'] - cut], sr)
        write_wav(str(ref / (fname.replace('-pred', ''))), c['x'], sr)
        n = c['L'] - cut
        x, y = pcm(c['x'])[:n], pcm(c['y'])[:n]
        if sr != SO.FS:
            x, y = RO.resample_compact(x, sr, SO.FS), RO.resample_compact(y, sr, SO.FS)
        assert SO.margin_db(x) >= SC.MARGIN_DB
        want[fname] = (n, SO.stoi(x, y))
    r = subprocess.run([sys.executable, os.path.join(REPO, 'main.py'), '--stoi-wav-dir', str(syn), '--stoi-ref-dir', str(ref), '--logdir', str(tmp_path / 'log'),
                        '--name', 'e2e'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout
    assert '[WARNING]' in r.stdout and 'b.wav has 29 band frames' in r.stdout and 'STOI of 3 pairs (2 scored)' in r.stdout, r.stdout
    lines = open(str(tmp_path / 'log' / 'e2e' / 'stoi.csv')).read().split('\n')
    assert lines[0] == 'file,samples,frames,kept,segments,stoi,estoi' and len(lines) == 5 and lines[4] == ''
    _, es = e32()
    for line, fname in zip(lines[1:4], ('a-pred.wav', 'b.wav', 'c.wav')):
        n, w = want[fname]
        f = line.split(',')
        F, K, M, S = w['counts']
        assert f[0] == fname and [int(v) for v in f[1:5]] == [n, F, K, S], (line, w['counts'])
        # (the rows carry six decimals; the 16 kHz pair adds the resampler's float32 error, far under the rounding of the row)
        assert abs(float(f[5]) - w['score'][0]) <= FACTOR * es + 1e-6 and abs(float(f[6]) - w['score'][1]) <= FACTOR * es + 1e-6, (line, w['score'])
    assert lines[2] == 'b.wav,4096,30,30,0,0.000010,0.000010'
