"""st_dtw_batch on the device against the numpy oracle of tests/dtw_oracle.py (bit for bit where every intermediate is exact in fp32,
within the derived bound eps on Gaussian inputs), metrics.mcd on device cepstra, and the --mcd-wav-dir path end to end.

The kernel has four forms: the rows of x and y staged in LDS or read through L2, the back-pointers in LDS or in the workspace.  Which
one runs follows from (Tx, Ty, D): up to about 550 x 550 frames the back-pointers stay in LDS; the rows join them while (Tx + Ty) (D | 1)
floats still fit.  The shapes below reach all four."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import dtw_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = [(n, m) for n in (1, 2, 3, 63, 64, 65) for m in (1, 2, 5, 64, 66)]
LARGE = [(257, 130), (130, 257), (300, 300)]            # more cells on a diagonal than the workgroup has threads


def _pad(seqs, T, D, fill):
    out = np.full((len(seqs), T, D), fill, np.float32)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out


def _run(x, y, x_len=None, y_len=None, **kw):
    """x, y: (B, T, D) arrays or device tensors -> (total, path_len, path) as numpy arrays (path None without want_path)"""
    from semi_tts_amd.metrics import dtw
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    y = y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(DEV)
    out = dtw(x, y, x_len, y_len, **kw)
    torch.cuda.synchronize()
    total, plen = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert total.dtype == np.float32 and plen.dtype == np.int32 and total.shape == plen.shape == (x.shape[0],)
    path = None
    if out[2] is not None:
        path = out[2].cpu().numpy()
        assert path.dtype == np.int32 and path.shape == (x.shape[0], x.shape[1] + y.shape[1] - 1, 2)
    return total, plen, path


def _assert_exact(total, plen, path, want_total, want_path, what):
    """one pair's device outputs equal the float32 oracle bit for bit, the whole path, -1 beyond it"""
    assert np.float32(total).view(np.uint32) == np.float32(want_total).view(np.uint32), (what, total, want_total)
    assert plen == len(want_path), (what, plen, len(want_path))
    assert np.array_equal(path[:plen], want_path), what
    assert (path[plen:] == -1).all(), what


@pytest.fixture(scope='module')
def exact_cases():
    """[(x, y, D, oracle total, oracle path)]: every (n, m) of SMALL + LARGE at D = 1 and at D = 3; computed once"""
    rs = np.random.RandomState(7)
    cases = []
    for n, m in SMALL + LARGE:
        for D in (1, 3):
            x, y = O.integer_pair(rs, n, m, D)
            total, path = O.dtw(x, y, 1.0, np.float32)
            assert total == np.round(total) and O.is_path(path, n, m)
            cases.append((x, y, D, total, path))
    assert len(cases) == 2 * (len(SMALL) + len(LARGE)) == 66
    return cases


def test_exact_every_pair_alone(exact_cases):
    for x, y, D, want_total, want_path in exact_cases:
        total, plen, path = _run(x[None], y[None])
        _assert_exact(total[0], plen[0], path[0], want_total, want_path, (len(x), len(y), D))


@pytest.mark.parametrize('D', [1, 3])
def test_exact_ragged_batch_equals_the_pairs_alone(exact_cases, D):
    """all pairs of one width in one padded batch (NaN beyond every length): bitwise the oracle, which the pairs alone equal too;
    lengths as host lists and as device tensors"""
    cases = [c for c in exact_cases if c[2] == D]
    xs, ys = [c[0] for c in cases], [c[1] for c in cases]
    xl, yl = [len(s) for s in xs], [len(s) for s in ys]
    X, Y = _pad(xs, max(xl) + 3, D, np.nan), _pad(ys, max(yl) + 1, D, np.nan)
    for lens in ((xl, yl), (torch.tensor(xl, device=DEV), torch.tensor(yl, dtype=torch.int64, device=DEV))):
        total, plen, path = _run(X, Y, *lens)
        for b, c in enumerate(cases):
            _assert_exact(total[b], plen[b], path[b], c[3], c[4], (xl[b], yl[b], D))
    # the same pairs in another order and batch size
    total2, plen2, path2 = _run(X[::-1][:5].copy(), Y[::-1][:5].copy(), xl[::-1][:5], yl[::-1][:5])
    assert np.array_equal(total2.view(np.uint32), total[::-1][:5].view(np.uint32)) and np.array_equal(path2, path[::-1][:5])


@pytest.mark.parametrize('n,m,D', [(600, 610, 1), (610, 600, 3)])
def test_exact_with_the_back_pointers_in_the_workspace(n, m, D):
    """past about 550 x 550 the 2-bit table leaves LDS for the workspace (the rows stay staged at these widths); two pairs, so the second
    one's table starts at an offset"""
    from semi_tts_amd import _lib
    assert int(_lib.load().st_dtw_workspace_bytes(2, n, m)) > 0
    rs = np.random.RandomState(n + D)
    pairs = [O.integer_pair(rs, n, m, D), O.integer_pair(rs, n - 77, m - 300, D)]
    X, Y = _pad([p[0] for p in pairs], n, D, np.nan), _pad([p[1] for p in pairs], m, D, np.nan)
    total, plen, path = _run(X, Y, [n, n - 77], [m, m - 300])
    for b, (x, y) in enumerate(pairs):
        want_total, want_path = O.dtw(x, y, 1.0, np.float32)
        _assert_exact(total[b], plen[b], path[b], want_total, want_path, (b, n, m, D))


def test_exact_at_the_largest_grid():
    """4096 x 4096, the limit: the longest diagonals, the largest table offsets; the second pair is short"""
    T = 4096
    rs = np.random.RandomState(4096)
    pairs = [O.integer_pair(rs, T, T, 1), O.integer_pair(rs, 70, 50, 1)]
    X, Y = _pad([p[0] for p in pairs], T, 1, np.nan), _pad([p[1] for p in pairs], T, 1, np.nan)
    total, plen, path = _run(X, Y, [T, 70], [T, 50])
    for b, (x, y) in enumerate(pairs):
        want_total, want_path = O.dtw(x, y, 1.0, np.float32)
        _assert_exact(total[b], plen[b], path[b], want_total, want_path, b)


def _check_close(x, y, total, plen, path, scale, D, what):
    """the four properties of a pair on Gaussian inputs, against float64, at the derived bound"""
    n, m = len(x), len(y)
    total64, _ = O.dtw(x, y, scale, np.float64)
    e = O.eps(n, m, D)
    own = O.path_cost(x, y, path[:plen], scale)
    print('%s: total %.6f, float64 optimum %.6f (rel %.2e), own path %.6f (excess rel %.2e, total vs own rel %.2e), eps %.2e'
          % (what, total, total64, abs(total - total64) / total64, own, (own - total64) / total64, abs(total - own) / own, e))
    assert abs(float(total) - total64) <= e * total64, what
    assert O.is_path(path[:plen], n, m) and (path[plen:] == -1).all(), what
    assert own - total64 <= e * total64, what
    assert abs(float(total) - own) <= e * own, what


@pytest.mark.parametrize('D', [1, 12, 13, 39, 64])
def test_close_to_float64(D):
    """Gaussian inputs in a column window d0 > 0 of wider rows, a batch stride that is not the tensor's size; (300, 333) at D = 64 reads
    its rows through L2, everything else from LDS"""
    rs = np.random.RandomState(D)
    shapes = [(50, 70), (129, 128), (300, 333)]
    d0, W = 2, D + 5                                       # the columns [2, 2 + D) of rows W floats apart
    Tx, Ty = 300, 333
    bufx = torch.full((len(shapes) * 2, Tx + 1, W), float('nan'), device=DEV)
    bufy = torch.full((len(shapes), Ty, W), float('nan'), device=DEV)
    X, Y = bufx[::2, :Tx], bufy                            # x: every other slab of a larger buffer
    pairs = []
    for b, (n, m) in enumerate(shapes):
        x, y = rs.randn(n, D).astype(np.float32), (rs.randn(m, D) * 1.3 + 0.2).astype(np.float32)
        X[b, :n, d0:d0 + D] = torch.from_numpy(x).to(DEV)
        Y[b, :m, d0:d0 + D] = torch.from_numpy(y).to(DEV)
        pairs.append((x, y))
    assert X.stride(0) == 2 * (Tx + 1) * W and X.stride(1) == W
    scale = 2.5
    total, plen, path = _run(X, Y, [s[0] for s in shapes], [s[1] for s in shapes], cols=(d0, d0 + D), scale=scale)
    for b, (x, y) in enumerate(pairs):
        _check_close(x, y, total[b], plen[b], path[b], scale, D, 'D=%d %s' % (D, shapes[b]))


def test_close_with_rows_and_back_pointers_outside_lds():
    """600 x 610 at D = 64: neither the rows nor the table fit LDS"""
    rs = np.random.RandomState(64)
    x, y = rs.randn(600, 64).astype(np.float32), rs.randn(610, 64).astype(np.float32)
    total, plen, path = _run(x[None], y[None])
    _check_close(x, y, total[0], plen[0], path[0], 1.0, 64, 'D=64 (600, 610)')


def test_edges():
    rs = np.random.RandomState(3)
    D, Tx, Ty = 4, 20, 24
    base_x, base_y = rs.randn(6, Tx, D).astype(np.float32), rs.randn(6, Ty, D).astype(np.float32)
    x, y = base_x.copy(), base_y.copy()
    xl, yl = [0, 9, 12, 12, 12, 20], [5, 0, 10, 10, 10, 24]
    x[2, 7, 2] = np.nan                 # pair 2: a NaN inside the valid region and the columns
    x[3, 12:] = np.nan                  # pair 3: NaN only beyond the lengths
    y[3, 10:] = np.nan
    x[4, 3, 0] = np.nan                 # pair 4: NaN inside [0, len) but outside the columns [1, 4)
    y[4, 5, 0] = np.nan
    total, plen, path = _run(x, y, xl, yl, cols=(1, 4))
    for b in (0, 1, 2):                 # a length-0 side (either), the NaN that counts
        assert np.isnan(total[b]) and plen[b] == 0 and (path[b] == -1).all(), b
    clean_t, clean_l, clean_p = _run(base_x, base_y, xl, yl, cols=(1, 4))
    for b in (3, 4, 5):                 # NaN where nothing is read: bitwise the clean result
        assert np.isfinite(total[b]) and total[b].view(np.uint32) == clean_t[b].view(np.uint32), b
        assert plen[b] == clean_l[b] and np.array_equal(path[b], clean_p[b]), b
        want_total, want_path = O.dtw(base_x[b, :xl[b], 1:4], base_y[b, :yl[b], 1:4], 1.0, np.float64)
        assert abs(total[b] - want_total) <= O.eps(xl[b], yl[b], 3) * want_total and O.is_path(path[b, :plen[b]], xl[b], yl[b])
    # lengths above Tx / Ty on the device are clamped; negative ones count as 0
    dl = _run(base_x, base_y, torch.tensor([99, 21, -3, 20, 20, 20], device=DEV, dtype=torch.int32),
              torch.tensor([24, 10 ** 6, 24, -1, 24, 25], device=DEV, dtype=torch.int32))
    full = _run(base_x, base_y)
    for b in (0, 1, 4, 5):
        assert dl[0][b].view(np.uint32) == full[0][b].view(np.uint32) and np.array_equal(dl[2][b], full[2][b]), b
    for b in (2, 3):
        assert np.isnan(dl[0][b]) and dl[1][b] == 0 and (dl[2][b] == -1).all(), b
    # want_path=False: the same total and path_len; two runs are bitwise equal
    t2, l2, p2 = _run(x, y, xl, yl, cols=(1, 4), want_path=False)
    assert p2 is None and np.array_equal(t2.view(np.uint32), total.view(np.uint32)) and np.array_equal(l2, plen)
    t3, l3, p3 = _run(x, y, xl, yl, cols=(1, 4))
    assert np.array_equal(t3.view(np.uint32), total.view(np.uint32)) and np.array_equal(l3, plen) and np.array_equal(p3, path)


@pytest.mark.parametrize('n,D', [(1, 1), (37, 12), (300, 13)])
def test_identical_sequences_give_zero_and_the_diagonal(n, D):
    x = np.random.RandomState(n).randn(2, n, D).astype(np.float32)
    total, plen, path = _run(x, x.copy(), scale=7.0)
    for b in range(2):
        assert total[b] == 0.0 and not np.signbit(total[b]) and plen[b] == n
        assert np.array_equal(path[b, :n], np.stack([np.arange(n)] * 2, 1)) and (path[b, n:] == -1).all()


# ---------------------------------------------------------------- the metric
SR, HOP = 22050, 220
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=SR,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


def _speech(L, seed):
    """harmonic tone with a moving pitch and gated silences"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / SR
    f0 = 110 + 120 * rs.rand() + 30 * np.sin(2 * np.pi * 1.5 * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(0.4 / (h + 1) * np.sin((h + 1) * ph + rs.rand()) for h in range(6))
    gate = (np.sin(2 * np.pi * 2 * t + 6 * rs.rand()) > -0.4)
    return (0.7 * x * gate + 0.002 * rs.randn(L)).astype(np.float32)


def _warp(x, ratio, seed):
    """x played `ratio` times slower (np.interp), plus faint noise"""
    L = int(len(x) * ratio)
    y = np.interp(np.arange(L) / ratio, np.arange(len(x)), x)
    return (y + 0.001 * np.random.RandomState(seed).randn(L)).astype(np.float32)


def test_mcd_on_device_cepstra():
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.metrics import mcd, MCD_SCALE
    conv = load_audio_transform(**AUDIO_CFG)
    a, b = _speech(SR + 4000, 11), _speech(SR, 12)                      # the second pair: a 1-second signal and its warp
    syn, ref = [_warp(a, 1.1, 21), _warp(b, 1.1, 22)], [a, b]           # both lists longest first, as the batches sort them
    cs = conv.extract_mfcc_batch([torch.from_numpy(w) for w in syn])
    cr = conv.extract_mfcc_batch([torch.from_numpy(w) for w in ref])
    fs_rows, fr = [1 + len(w) // HOP for w in syn], [1 + len(w) // HOP for w in ref]
    assert fs_rows[0] > fs_rows[1] and fr[0] > fr[1] and fr[1] == 1 + SR // HOP
    db, plen, path = mcd(cs, fs_rows, cr, fr)
    torch.cuda.synchronize()
    db, plen, path = db.cpu().numpy(), plen.cpu().numpy(), path.cpu().numpy()
    hs, hr = cs.cpu().numpy(), cr.cpu().numpy()
    for k in range(2):
        n, m = fs_rows[k], fr[k]
        x, y = hs[k, :n, 1:13], hr[k, :m, 1:13]
        total64, _ = O.dtw(x, y, 1.0, np.float64)
        want = MCD_SCALE * total64 / plen[k]
        print('pair %d: %d x %d frames, path %d, mcd %.6f dB, float64 %.6f dB (rel %.2e, eps %.2e)'
              % (k, n, m, plen[k], db[k], want, abs(db[k] - want) / want, O.eps(n, m, 12)))
        assert db.dtype == np.float32 and abs(db[k] - want) <= O.eps(n, m, 12) * want
        assert O.is_path(path[k, :plen[k]], n, m) and max(n, m) <= plen[k] <= n + m - 1
        assert 0.5 < db[k] < 40.0                                           # a warped copy: some distortion, far from unrelated signals
    # a signal with itself
    db0, plen0, _ = mcd(cr, fr, cr.clone(), fr)
    assert db0.cpu().tolist() == [0.0, 0.0] and plen0.cpu().tolist() == fr


# ---------------------------------------------------------------- end to end
def test_mcd_wav_dir_end_to_end(tmp_path, capsys):
    import main
    from semi_tts_amd.audio import load_audio_transform, write_wav
    from semi_tts_amd.metrics import mcd
    syn_dir, ref_dir, log = tmp_path / 'syn', tmp_path / 'ref', tmp_path / 'log'
    syn_dir.mkdir()
    ref_dir.mkdir()
    lens = {'b_utt': 9000, 'a_utt': 6100, 'c_utt': 12345}
    names = {'b_utt': 'b_utt.wav', 'a_utt': 'a_utt-pred.wav', 'c_utt': 'c_utt.x.wav'}
    for i, (key, L) in enumerate(lens.items()):
        ref = _speech(L, 40 + i)
        write_wav(ref_dir / (key + '.wav'), ref, SR)
        # a_utt and b_utt share a batch: a_utt is the longer synthesised file (1.6 x 6100) and the shorter recording, so the two
        # sides sort differently and the scorer has to bring the recordings' rows into the order of the synthesised ones
        write_wav(syn_dir / names[key], _warp(ref, (0.6, 1.6, 1.0)[i], 50 + i), SR)
    argv = ['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--mcd-wav-dir', str(syn_dir), '--mcd-ref-dir', str(ref_dir),
            '--logdir', str(log), '--batch-size', '2']
    main.main(argv + ['--name', 'with', '--mcd-path'])
    main.main(argv + ['--name', 'plain', '--no-msg'])
    out = capsys.readouterr().out
    rows = (log / 'with' / 'mcd.csv').read_text().splitlines()
    assert rows[0] == 'file,frames,ref_frames,path_len,mcd_db' and len(rows) == 4
    assert (log / 'plain' / 'mcd.csv').read_text().splitlines() == rows and sorted(os.listdir(log / 'plain')) == ['mcd.csv']
    assert sorted(os.listdir(log / 'with')) == ['a_utt.dtw.npy', 'b_utt.dtw.npy', 'c_utt.dtw.npy', 'mcd.csv']
    conv = load_audio_transform(**AUDIO_CFG)
    vals = []
    for row, key in zip(rows[1:], ('a_utt', 'b_utt', 'c_utt')):           # sorted by file name
        f, n, m, P, db = row.split(',')
        assert f == names[key]
        x, y = conv.load(syn_dir / f)[0], conv.load(ref_dir / (key + '.wav'))[0]
        assert (int(n), int(m)) == (1 + len(x) // HOP, 1 + len(y) // HOP) and int(m) == 1 + lens[key] // HOP
        want_db, want_P, want_path = mcd(conv.extract_mfcc_batch([x]), [int(n)], conv.extract_mfcc_batch([y]), [int(m)])
        assert db == '%.4f' % float(want_db[0]) and int(P) == int(want_P[0])
        path = np.load(log / 'with' / (key + '.dtw.npy'))
        assert path.dtype == np.int32 and path.shape == (int(P), 2) and O.is_path(path, int(n), int(m))
        assert np.array_equal(path, want_path[0, :int(P)].cpu().numpy())
        vals.append(float(want_db[0]))
    assert out.count('MCD-DTW of 3 pairs: mean %.4f dB' % np.mean(vals)) == 2
    # a missing partner raises before anything is written
    os.remove(ref_dir / 'b_utt.wav')
    with pytest.raises(ValueError, match=r'b_utt\.wav has no recording'):
        main.main(argv + ['--name', 'missing'])
    assert not (log / 'missing').exists()
