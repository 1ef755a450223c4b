"""st_f0_yin and st_f0_path_scores on the device against the float64 oracle of tests/f0_oracle.py, and the two command-line paths.

On the oracle's robust frames (every comparison of the definition clear by 2 eps, eps = (2 W + tau_max + 8) 2^-24 the derived bound of
an fp32 d') the device must take the oracle's decisions: the same voicing, the same integer lag, f0 inside the oracle's interval, aper
within 2 eps.  The remaining frames are left out; their share is capped at 5 % per signal, from the oracle alone.  The edge shapes
walk the kernel's boundaries: lags at the wave and pass boundaries of the lag ownership and of the prefix sum, windows around the
8-step unrolling, frame counts around the run a workgroup takes, utterances shorter than a hop, and a batch above 32."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import f0_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
THR = 0.15


def _run(xs, sr, hop, W, tau_min, tau_max, thr=THR, T_pad=None, gap=0):
    """the utterances xs in one st_f0_yin batch, in the given order, `gap` NaN samples written behind each -> (f0, aper) (B, T_pad)"""
    from semi_tts_amd import ops
    lens = [len(x) for x in xs]
    parts, off, pos = [], [], 0
    for x in xs:
        off.append(pos)
        parts += [np.asarray(x, np.float32), np.full(gap, np.nan, np.float32)]
        pos += len(x) + gap
    packed = torch.from_numpy(np.concatenate(parts)).to(DEV)
    T_pad = T_pad or max(O.frame_count(n, hop) for n in lens)
    f0, aper = ops.f0_yin(packed, off, lens, hop, W, tau_min, tau_max, float(sr), thr, T_pad, with_aper=True)
    torch.cuda.synchronize()
    f0, aper = f0.cpu().numpy(), aper.cpu().numpy()
    assert f0.dtype == aper.dtype == np.float32 and f0.shape == aper.shape == (len(xs), T_pad)
    return f0, aper


def _check(x, f0, aper, sr, hop, W, tau_min, tau_max, thr=THR, what=''):
    """one utterance's device rows against the oracle -> (robust frames, frames)"""
    o = O.yin(x, sr, hop, W, tau_min, tau_max, thr)
    T, e = len(o['f0']), O.eps(W, tau_max)
    assert T == O.frame_count(len(x), hop) and T <= len(f0)
    assert (f0[T:] == 0).all() and (aper[T:] == 0).all(), what                      # the rows past T
    assert np.isfinite(f0[:T]).all() and np.isfinite(aper[:T]).all(), what
    r = o['robust']
    voiced = f0[:T] > 0
    assert np.array_equal(voiced[r], o['tau'][r] > 0), (what, np.nonzero(r & (voiced != (o['tau'] > 0)))[0])
    rv = r & (o['tau'] > 0)
    with np.errstate(divide='ignore'):
        tau_dev = np.where(voiced, np.round(sr / np.where(voiced, f0[:T], 1.0)), 0).astype(np.int64)
    assert np.array_equal(tau_dev[rv], o['tau'][rv]), (what, np.nonzero(rv & (tau_dev != o['tau']))[0])
    inside = (f0[:T] >= o['f0_lo']) & (f0[:T] <= o['f0_hi'])
    assert inside[rv].all(), (what, np.nonzero(rv & ~inside)[0])
    err = np.abs(aper[:T] - o['aper'])
    assert (err[r] <= 2 * e * o['aper'][r]).all(), (what, (err[r] / np.maximum(o['aper'][r], 1e-300)).max() / e)
    return int(r.sum()), T


def _tone(n, period, seed, noise=0.03):
    """n samples of a 3-harmonic tone of the given period (in samples) with a little noise"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) * (2 * np.pi / period) + rs.uniform(0, 6.28)
    return (0.4 * np.sin(t) + 0.2 * np.sin(2 * t + 1.0) + 0.1 * np.sin(3 * t + 2.0) + noise * rs.randn(n)).astype(np.float32)


# ---------------------------------------------------------------- the signals
@pytest.mark.parametrize('framing', sorted(O.FRAMINGS))
@pytest.mark.parametrize('name', O.SIGNALS)
def test_signals(name, framing):
    sr, hop, tau_min, tau_max, W, n = O.FRAMINGS[framing]
    x = O.signal(name, framing)
    f0, aper = _run([x], sr, hop, W, tau_min, tau_max, T_pad=O.frame_count(n, hop) + 3)
    robust, T = _check(x, f0[0], aper[0], sr, hop, W, tau_min, tau_max, what=(name, framing))
    print('%s / %s: %d of %d frames outside the robust set' % (name, framing, T - robust, T))
    assert T - robust <= 0.05 * T
    if name == 'silence':
        assert (f0[0] == 0).all() and (aper[0, :T] == 1).all()
    if name in ('tone', 'vib', 'hi'):
        assert (f0[0, :T] > 0).mean() > 0.9


# ---------------------------------------------------------------- shapes that can break the kernel
SMALL = [(2000, 20, 80, 5, 40), (2000, 7, 63, 3, 65)]               # (sr, hop, W, tau_min, tau_max)


@pytest.mark.parametrize('sr,hop,W,tau_min,tau_max', SMALL)
def test_edge_lengths_alone_and_in_a_ragged_batch(sr, hop, W, tau_min, tau_max):
    lens = sorted({1, hop - 1, hop, hop + 1, W // 2, W, W + tau_max, 2 * (W + tau_max) + 1})
    xs = [_tone(L, 0.45 * (tau_min + tau_max), 10 + i) for i, L in enumerate(lens)]
    f0b, apb = _run(xs, sr, hop, W, tau_min, tau_max, gap=5)        # NaN behind every utterance: never read for its value
    robust = frames = 0
    for i, x in enumerate(xs):
        f0, ap = _run([x], sr, hop, W, tau_min, tau_max)
        T = O.frame_count(len(x), hop)
        assert f0.shape[1] == T
        assert np.array_equal(f0[0].view(np.uint32), f0b[i, :T].view(np.uint32)) and np.array_equal(ap[0].view(np.uint32), apb[i, :T].view(np.uint32))
        r, t = _check(x, f0b[i], apb[i], sr, hop, W, tau_min, tau_max, what=('L', len(x)))
        robust, frames = robust + r, frames + t
    assert robust >= 0.8 * frames


@pytest.mark.parametrize('tau_max', [63, 64, 65, 255, 256, 257, 1024])
@pytest.mark.parametrize('low', [True, False])
def test_lag_boundaries(tau_max, low):
    """wave and pass boundaries of the lag ownership (64 TL lags a pass, TL = 4, 6 or 8 by tau_max) and of the prefix sum"""
    tau_min = 2 if low else tau_max - 1
    sr, hop, W = 8000, 90, 100
    xs = [_tone(1400, 0.8 * tau_max, tau_max), _tone(700, 0.31 * tau_max, tau_max + 1), np.zeros(300, np.float32)]
    f0, ap = _run(xs, sr, hop, W, tau_min, tau_max)
    robust = frames = 0
    for i, x in enumerate(xs):
        r, t = _check(x, f0[i], ap[i], sr, hop, W, tau_min, tau_max, what=(tau_min, tau_max, i))
        robust, frames = robust + r, frames + t
    assert robust >= 0.8 * frames
    if low:
        assert (f0[0] > 0).sum() >= 5                               # the search did find the tone


@pytest.mark.parametrize('W', [1, 2, 63, 64, 65, 2048])
def test_windows(W):
    sr, hop, tau_min, tau_max = 2000, 50, 5, 40
    xs = [_tone(2600, 17.3, W), _tone(333, 29.0, W + 1)]
    f0, ap = _run(xs, sr, hop, W, tau_min, tau_max)
    robust = frames = 0
    for i, x in enumerate(xs):
        r, t = _check(x, f0[i], ap[i], sr, hop, W, tau_min, tau_max, what=(W, i))
        robust, frames = robust + r, frames + t
    assert robust >= (0.8 if W > 2 else 0.3) * frames              # (one or two terms a lag: many near-ties, still no wrong decision)


@pytest.mark.parametrize('sr,hop,W,tau_min,tau_max', [(2000, 20, 80, 5, 40), (2000, 150, 80, 5, 40), (2000, 2000, 80, 5, 40), (2000, 1500, 2048, 5, 1024)])
def test_frame_counts_around_the_run_length(sr, hop, W, tau_min, tau_max):
    """T one below, at and one above the run of frames a workgroup takes, and three runs + 1; hop > W + tau_max: frames that share no
    samples; at the last two framings the staged span caps the run below 8"""
    from semi_tts_amd import ops
    R = ops.f0_run_length(hop, W, tau_max)
    assert R == {20: 8, 150: 8, 2000: 6, 1500: 5}[hop]
    counts = [R - 1, R, R + 1, 3 * R + 1]
    xs = [_tone((T - 1) * hop + (hop // 3), 23.0, T) for T in counts]
    assert [O.frame_count(len(x), hop) for x in xs] == counts
    f0, ap = _run(xs, sr, hop, W, tau_min, tau_max, gap=3)
    robust = frames = 0
    for i, x in enumerate(xs):
        r, t = _check(x, f0[i], ap[i], sr, hop, W, tau_min, tau_max, what=(hop, counts[i]))
        robust, frames = robust + r, frames + t
        alone = _run([x], sr, hop, W, tau_min, tau_max)[0]
        assert np.array_equal(alone[0].view(np.uint32), f0[i, :counts[i]].view(np.uint32))
    assert robust >= 0.8 * frames


def test_batch_of_33_equals_every_utterance_alone():
    sr, hop, W, tau_min, tau_max = 2000, 20, 80, 5, 40
    rs = np.random.RandomState(5)
    xs = [_tone(int(L), rs.uniform(8, 30), 100 + i) for i, L in enumerate(rs.randint(1, 700, 33))]
    f0, ap = _run(xs, sr, hop, W, tau_min, tau_max, gap=2)
    f0r, apr = _run(xs[::-1], sr, hop, W, tau_min, tau_max)         # another position in the batch, other neighbours
    for i, x in enumerate(xs):
        T = O.frame_count(len(x), hop)
        a0, a1 = _run([x], sr, hop, W, tau_min, tau_max)
        for got in ((f0[i], ap[i]), (f0r[32 - i], apr[32 - i])):
            assert np.array_equal(a0[0].view(np.uint32), got[0][:T].view(np.uint32)) and np.array_equal(a1[0].view(np.uint32), got[1][:T].view(np.uint32))
            assert (got[0][T:] == 0).all() and (got[1][T:] == 0).all()
    for i in (0, 7, 32):
        _check(xs[i], f0[i], ap[i], sr, hop, W, tau_min, tau_max, what=i)
    again = _run(xs, sr, hop, W, tau_min, tau_max, gap=2)[0]
    assert np.array_equal(again.view(np.uint32), f0.view(np.uint32))                # bitwise repeatable


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('sr,hop,W,tau_min,tau_max', SMALL + [(2000, 150, 80, 5, 40)])
def test_one_non_finite_sample_spoils_exactly_the_frames_that_read_it(sr, hop, W, tau_min, tau_max, bad):
    x = _tone(1203, 19.0, 3)
    T = O.frame_count(len(x), hop)
    clean_f0, clean_ap = _run([x], sr, hop, W, tau_min, tau_max)
    for p in (0, 1, W // 2, 601, len(x) - 1):
        y = x.copy()
        y[p] = bad
        f0, ap = _run([y], sr, hop, W, tau_min, tau_max)
        s0 = np.arange(T) * hop - W // 2
        hit = (s0 <= p) & (p < s0 + W + tau_max)                    # the frames whose slice [s0, s0 + W + tau_max) holds p
        assert hit.any() and np.isnan(f0[0, hit]).all() and np.isnan(ap[0, hit]).all(), p
        assert np.array_equal(f0[0, ~hit].view(np.uint32), clean_f0[0, ~hit].view(np.uint32)), p
        assert np.array_equal(ap[0, ~hit].view(np.uint32), clean_ap[0, ~hit].view(np.uint32)), p


# ---------------------------------------------------------------- st_f0_path_scores
def _track(rs, T, kind):
    f = rs.uniform(80, 400, T).astype(np.float32)
    if kind == 'unvoiced':
        f[:] = 0
    elif kind == 'mixed':
        f[rs.rand(T) < 0.3] = 0
        f[rs.rand(T) < 0.1] = np.nan
    return f


def _scores_ok(fx, fy, path, plen, got_counts, got_sums, what):
    counts, s2, s1, sa = O.path_scores(fx, fy, path, plen)
    assert tuple(int(v) for v in got_counts) == counts, (what, got_counts, counts)
    bound = (counts[1] + 8) * 2.0 ** -24
    assert abs(float(got_sums[0]) - s2) <= bound * s2, (what, (float(got_sums[0]) - s2) / max(s2, 1e-300) * 2.0 ** 24)
    assert abs(float(got_sums[1]) - s1) <= bound * sa, (what, (float(got_sums[1]) - s1) / max(sa, 1e-300) * 2.0 ** 24)


@pytest.mark.parametrize('n,m', [(1, 1), (1, 5), (5, 1), (64, 66), (257, 130)])
def test_path_scores_on_dtw_paths(n, m):
    from semi_tts_amd import metrics, ops
    rs = np.random.RandomState(n + m)
    kinds = ['mixed', 'voiced', 'unvoiced', 'mixed']
    B = len(kinds)
    x = torch.from_numpy(rs.randn(B, n, 3).astype(np.float32)).to(DEV)
    y = torch.from_numpy(rs.randn(B, m, 3).astype(np.float32)).to(DEV)
    x_len = [n, n, n, 0]                                            # the last pair is empty: path_len 0, a path of -1
    _, plen, path = metrics.dtw(x, y, x_len, [m] * B)
    fx = np.stack([_track(rs, n, k) for k in kinds])
    fy = np.stack([_track(rs, m, 'voiced' if k == 'unvoiced' else k) for k in kinds])
    dx, dy = torch.from_numpy(fx).to(DEV), torch.from_numpy(fy).to(DEV)
    counts, sums = ops.f0_path_scores(dx, dy, path, plen)
    counts2, sums2 = ops.f0_path_scores(dx, dy, path, plen)
    torch.cuda.synchronize()
    assert torch.equal(counts, counts2) and torch.equal(sums.view(torch.int32), sums2.view(torch.int32))
    hp, hl, hc, hs = path.cpu().numpy(), plen.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy()
    assert hl.tolist()[:3] == hc[:3, 0].tolist() and hl[3] == 0 and hc[3].tolist() == [0, 0, 0, 0] and hs[3].tolist() == [0.0, 0.0]
    for b in range(B):
        _scores_ok(fx[b], fy[b], hp[b], hl[b], hc[b], hs[b], (n, m, kinds[b]))
    assert hc[2, 1] == 0 and hc[2, 2] == hl[2] and hc[1, 1] == hl[1] and hc[1, 2] == 0       # all-unvoiced against voiced; all voiced
    # the figures of metrics.f0_scores: divisions on the device, NaN where there is no both-voiced pair
    s = metrics.f0_scores(dx, dy, path, plen)
    both = hc[:, 1].astype(np.float64)
    with np.errstate(all='ignore'):
        want = {'f0_rmse_cents': np.sqrt(hs[:, 0] / both), 'mean_cents': hs[:, 1] / both, 'gross_error': hc[:, 3] / both,
                'vuv_error': hc[:, 2] / hc[:, 0].astype(np.float64)}
    for k, w in want.items():
        g = s[k].cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(w)) and np.allclose(g, w, rtol=1e-6, atol=0, equal_nan=True), k
    assert np.isnan(want['f0_rmse_cents'][2]) and np.isnan(want['vuv_error'][3])
    # a strided view of a wider tensor is read where it lies
    wide = torch.zeros(B, n + 7, device=DEV)
    wide[:, 3:3 + n] = dx
    c3, s3 = ops.f0_path_scores(wide[:, 3:3 + n], dy, path, plen)
    assert torch.equal(c3, counts) and torch.equal(s3.view(torch.int32), sums.view(torch.int32))


def test_path_scores_on_the_longest_path():
    from semi_tts_amd import ops
    rs = np.random.RandomState(8191)
    T = 4096
    steps = np.arange(2 * T - 1)
    path = np.stack([(steps + 1) // 2, steps // 2], axis=1).astype(np.int32)[None]         # (0,0), (1,0), (1,1), (2,1), ...: 8191 cells
    assert path.shape == (1, 8191, 2) and path[0, -1].tolist() == [T - 1, T - 1]
    for kind in ('voiced', 'mixed'):
        fx, fy = _track(rs, T, kind), _track(rs, T, kind)
        for plen in (8191, 8190, 257, 0):
            args = [torch.from_numpy(a).to(DEV) for a in (fx[None], fy[None], path, np.array([plen], np.int32))]
            counts, sums = ops.f0_path_scores(*args)
            counts2, sums2 = ops.f0_path_scores(*args)
            assert torch.equal(counts, counts2) and torch.equal(sums.view(torch.int32), sums2.view(torch.int32))
            _scores_ok(fx, fy, path[0], plen, counts[0].cpu().numpy(), sums[0].cpu().numpy(), (kind, plen))


# ---------------------------------------------------------------- the converter and the command line
def _config():
    import yaml
    return yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)


def _voice(n, sr, f_hz, stretch=1.0, seed=0):
    """a harmonic sum at f_hz under a syllable-like envelope and a slowly moving spectral tilt, both stretched in time by `stretch`"""
    t = np.arange(n) / sr / stretch
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + 0.5) ** 2
    tilt = 0.5 + 0.4 * np.sin(2 * np.pi * 2.0 * t)
    ph = 2 * np.pi * f_hz * np.arange(n) / sr
    y = sum(np.sin(k * ph) * tilt ** (k - 1) / k for k in range(1, 9))
    return 0.2 * env * y + 1e-3 * np.random.RandomState(seed).randn(n)


def test_extract_f0_matches_the_oracle_and_the_mfcc_rows():
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(**dict(_config()['data']['audio']))
    sr, hop = conv.sr, conv.hop_length_mfcc
    tau_min, tau_max, W = conv.f0_lags()
    xs = [_voice(7000, sr, 120.0), _voice(9000, sr, 210.0, seed=1)]
    f0, aper = conv.extract_f0_batch([torch.from_numpy(x) for x in xs], with_aper=True)
    mfcc = conv.extract_mfcc_batch([torch.from_numpy(x) for x in xs])
    assert f0.shape == aper.shape == mfcc.shape[:2] and f0.is_cuda                  # the rows of the MFCC: a DTW path indexes both
    f0, aper = f0.cpu().numpy(), aper.cpu().numpy()
    for row, x in enumerate(xs[::-1]):                                              # sorted longest first
        _check(x.astype(np.float32), f0[row], aper[row], sr, hop, W, tau_min, tau_max, what=row)
    inner = f0[0, 3:-4]
    assert (np.abs(inner - 210.0) < 2.0).all()
    one = conv.extract_f0_from_waveform(torch.from_numpy(np.stack([0.0 * xs[1], xs[1]])), channel=1)
    assert one.shape == (1 + 9000 // hop,) and not one.is_cuda and np.array_equal(one.numpy().view(np.uint32), f0[0].view(np.uint32))


def test_mcd_f0_end_to_end(tmp_path, capsys):
    import main
    from semi_tts_amd.audio import write_wav
    sr = _config()['data']['audio']['sample_rate']
    n = sr // 2
    ref = _voice(n, sr, 150.0)
    syn = _voice(int(1.05 * n), sr, 150.0 * 2.0 ** (100.0 / 1200.0), stretch=1.05)  # 5 % slower, 100 cents up
    dirs = {k: tmp_path / k for k in ('up_syn', 'up_ref')}
    for d in dirs.values():
        d.mkdir()
    write_wav(dirs['up_syn'] / 'a-pred.wav', syn, sr)
    write_wav(dirs['up_ref'] / 'a.wav', ref, sr)
    log = tmp_path / 'log'
    base = ['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--logdir', str(log), '--no-msg']
    up = ['--mcd-wav-dir', str(dirs['up_syn']), '--mcd-ref-dir', str(dirs['up_ref'])]
    main.main(base + up + ['--name', 'plain'])
    main.main(base + up + ['--name', 'f0', '--mcd-f0'])
    main.main(base + up + ['--name', 'f0path', '--mcd-f0', '--mcd-path'])
    main.main(base + up + ['--name', 'path', '--mcd-path'])
    out = capsys.readouterr().out
    assert sorted(os.listdir(log / 'plain')) == ['mcd.csv'] and sorted(os.listdir(log / 'f0')) == ['f0.csv', 'mcd.csv']
    assert (log / 'f0' / 'mcd.csv').read_bytes() == (log / 'plain' / 'mcd.csv').read_bytes() == (log / 'f0path' / 'mcd.csv').read_bytes()
    assert (log / 'f0path' / 'a.dtw.npy').read_bytes() == (log / 'path' / 'a.dtw.npy').read_bytes()
    rows = (log / 'f0' / 'f0.csv').read_text().splitlines()
    assert rows[0] == 'file,path_len,voiced_pairs,f0_rmse_cents,vuv_error,gross_error,mean_cents' and len(rows) == 2
    assert (log / 'f0path' / 'f0.csv').read_text().splitlines() == rows
    f, plen, both, rmse, vuv, gross, mean = rows[1].split(',')
    assert f == 'a-pred.wav' and int(plen) == int((log / 'plain' / 'mcd.csv').read_text().splitlines()[1].split(',')[3])
    assert 0 < int(both) <= int(plen)
    assert abs(float(mean) - 100.0) < 5.0 and float(vuv) < 0.1 and float(gross) == 0.0 and float(rmse) < 110.0
    assert out.count('F0 along the warp: mean RMSE') == 2
    # the other side: the recording scored against the synthesised file is 100 cents down
    down_syn, down_ref = tmp_path / 'down_syn', tmp_path / 'down_ref'
    down_syn.mkdir()
    down_ref.mkdir()
    write_wav(down_syn / 'a.wav', ref, sr)
    write_wav(down_ref / 'a.wav', syn, sr)
    main.main(base + ['--mcd-wav-dir', str(down_syn), '--mcd-ref-dir', str(down_ref), '--name', 'down', '--mcd-f0', '--f0-min', '70', '--f0-max', '400'])
    mean, vuv = (float(v) for v in np.array((log / 'down' / 'f0.csv').read_text().splitlines()[1].split(','))[[6, 4]])
    assert abs(mean + 100.0) < 5.0 and vuv < 0.1


def test_feat_f0_end_to_end(tmp_path):
    import main
    from semi_tts_amd.audio import load_audio_transform, write_wav
    config = _config()
    sr = config['data']['audio']['sample_rate']
    wavs, log = tmp_path / 'wav', tmp_path / 'log'
    wavs.mkdir()
    write_wav(wavs / 'b.wav', _voice(6000, sr, 180.0), sr)
    write_wav(wavs / 'a.wav', _voice(9100, sr, 95.0, seed=2), sr)
    main.main(['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--feat-wav-dir', str(wavs), '--feat', 'f0', '--logdir', str(log),
               '--name', 'f', '--no-msg', '--f0-threshold', '0.2'])
    assert sorted(os.listdir(log / 'f')) == ['a-f0.npy', 'b-f0.npy']
    conv = load_audio_transform(**dict(config['data']['audio']))
    for stem, L in (('a', 9100), ('b', 6000)):
        got = np.load(log / 'f' / (stem + '-f0.npy'))
        want = conv.extract_f0_batch([conv.load(wavs / (stem + '.wav'))[0]], threshold=0.2)[0].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (1 + L // conv.hop_length_mfcc,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got > 0).mean() > 0.8
    with pytest.raises(ValueError, match='--feat f0 does not combine with --segment-file'):
        main.main(['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--feat-wav-dir', str(wavs), '--feat', 'f0', '--logdir', str(log),
                   '--name', 'seg', '--segment-file', str(tmp_path / 'none.csv')])
    assert not (log / 'seg').exists()
