"""k-means without a device: the float64 oracle of tests/kmeans_oracle.py against brute-force loops on tiny cases, every refusal of the
toolops bindings and of the C entry points before a device is touched, the size refusal of --kmeans-max-gb, the unit transcripts of
--units-wav-dir read back by the n-gram counter and by --score-phn-dir's reader, the merge of repeats, and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import kmeans_oracle as O  # noqa: E402
from semi_tts_amd import kmeans as KM  # noqa: E402,F401  (the feature under test: without it nothing here runs)


# ---------------------------------------------------------------- the oracle against brute force
def _tiny(seed, N=23, D=3, K=5):
    rs = np.random.RandomState(seed)
    return rs.randint(-4, 5, (N, D)).astype(np.float32), rs.randint(-4, 5, (K, D)).astype(np.float32)


@pytest.mark.parametrize('seed', range(4))
def test_oracle_assign_and_update_equal_a_loop(seed):
    x, c = _tiny(seed)
    x[7] = np.nan
    c[4] = c[1]                                                     # a duplicated centroid: the lower k wins
    idx, dist = O.assign(x, c)
    sums, count, inertia = np.zeros((5, 3)), np.zeros(5, int), 0.0
    for n in range(len(x)):
        if np.isnan(x[n]).any():
            assert idx[n] == -1 and np.isnan(dist[n])
            continue
        best, bk = None, -1
        for k in range(len(c)):
            d = sum((float(x[n, j]) - float(c[k, j])) ** 2 for j in range(3))
            if best is None or d < best:
                best, bk = d, k
        assert idx[n] == bk and dist[n] == best and bk != 4
        sums[bk] += x[n]
        count[bk] += 1
        inertia += best
    out, cnt, stats, c64 = O.update(x, idx, dist, c)
    assert np.array_equal(cnt, count) and stats[0] == inertia and stats[2] == (count == 0).sum() and stats[3] == 1
    for k in range(5):
        want = (sums[k] / count[k]).astype(np.float32) if count[k] else c[k]
        assert np.array_equal(out[k], want)
    assert stats[1] == pytest.approx(((out.astype(np.float64) - c) ** 2).sum(), rel=1e-15)


def test_oracle_tree_sum_is_the_documented_order():
    v = np.random.RandomState(0).rand(37)
    part = [0.0] * 4
    for i, e in enumerate(v):
        part[i % 4] += e
    assert O.tree_sum(v, 4) == (part[0] + part[2]) + (part[1] + part[3])
    assert np.array_equal(O.tree_sum(np.stack([v, 2 * v]), 4), [O.tree_sum(v, 4), O.tree_sum(2 * v, 4)])


def test_oracle_relocate_orders_by_distance_then_index():
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    idx, dist = np.array([0, 0, -1, 0, 0, 0], np.int32), np.array([1.0, 5.0, 9.0, 5.0, np.nan, 2.0])
    cent = np.full((4, 2), -1.0, np.float32)
    out, taken = O.relocate(x, idx, dist, np.array([5, 0, 0, 0]), cent)
    assert taken.tolist() == [1, 3, 5] and np.array_equal(out, [[-1, -1], x[1], x[3], x[5]])
    out, taken = O.relocate(x[:1], idx[:1], dist[:1], np.array([1, 0, 0, 0]), cent)
    assert taken.tolist() == [0] and np.array_equal(out, [[-1, -1], x[0], [-1, -1], [-1, -1]])


@pytest.mark.parametrize('seed', range(3))
def test_oracle_seeding_equals_a_loop_and_refuses_too_few_rows(seed):
    x, _ = _tiny(seed, N=17)
    x[5] = x[2]
    u = np.random.default_rng(seed).random(6)
    picks, mind = O.pp_init(x, 6, u)
    chosen = [int(u[0] * 17)]
    for j in range(1, 6):
        w = [min(sum((float(a) - float(b)) ** 2 for a, b in zip(x[n], x[p])) for p in chosen) for n in range(17)]
        total, run, pick = sum(w), 0.0, None
        for n in range(17):
            run += w[n]
            if w[n] > 0 and run > u[j] * total:
                pick = n
                break
        chosen.append(pick)
    assert picks.tolist() == chosen and len(set(map(tuple, x[picks].tolist()))) == 6
    assert np.array_equal(mind, O.sqdist(x, x[picks]).min(1))
    with pytest.raises(ValueError):
        O.pp_init(x[np.arange(12) % 3], 4, u[:4])


def test_oracle_lloyd_separates_two_blobs():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.randn(40, 2), rs.randn(40, 2) + 30]).astype(np.float32)
    cent, idx, dist, history, converged = O.lloyd(x, x[[0, 1]])
    assert converged and len(set(idx[:40])) == 1 and len(set(idx[40:])) == 1 and idx[0] != idx[40]
    assert all(b[1] <= a[1] for a, b in zip(history, history[1:]))


# ---------------------------------------------------------------- the library and the bindings
def test_exports_and_source_lists():
    from semi_tts_amd import _lib, build
    assert build.KMEANS_SOURCES == ['kmeans.hip'] and 'kmeans.hip' not in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'kmeans.hip'))
    declared = _lib.check_header_symbols()
    for name in ('st_kmeans_assign', 'st_kmeans_update', 'st_kmeans_relocate', 'st_kmeans_pp_step', 'st_kmeans_pp_pick'):
        assert name in declared
    lib = _lib.load()
    assert lib.st_kmeans_chunks(1) == 1 and lib.st_kmeans_chunks(1024) == 1 and lib.st_kmeans_chunks(1025) == 2
    assert lib.st_kmeans_update_workspace_bytes(1000, 39, 50) > 0 and lib.st_kmeans_update_workspace_bytes(1000, 257, 50) == 0
    assert lib.st_kmeans_update_workspace_bytes(1000, 39, 4097) == 0 and lib.st_kmeans_update_workspace_bytes(0, 39, 50) == 0


def test_c_entries_refuse_each_limit_without_a_device():
    from semi_tts_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def data(x=p, ld=4, N=8, D=4):
        return ctypes.byref(_lib.StKmeansData(x, ld, N, D))
    bad_data = (dict(x=None), dict(N=0), dict(D=0), dict(D=257, ld=257), dict(ld=3), dict(N=2 ** 31 - 1, ld=2 ** 9 + 1))
    for kw in bad_data:
        assert lib.st_kmeans_assign(data(**kw), p, 2, p, p, None) == -22 and b'st_kmeans_assign' in lib.st_last_error()
        assert lib.st_kmeans_update(data(**kw), p, p, p, 2, p, p, p, p, None) == -22 and b'st_kmeans_update' in lib.st_last_error()
        assert lib.st_kmeans_relocate(data(**kw), p, p, p, 2, p, None) == -22 and b'st_kmeans_relocate' in lib.st_last_error()
        assert lib.st_kmeans_pp_step(data(**kw), p, 0, 2, p, p, p, None) == -22 and b'st_kmeans_pp_step' in lib.st_last_error()
        assert lib.st_kmeans_pp_pick(data(**kw), p, p, p, 0, 2, p, p, p, None) == -22 and b'st_kmeans_pp_pick' in lib.st_last_error()
    for K in (0, -1, 4097):
        assert lib.st_kmeans_assign(data(), p, K, p, p, None) == -22
        assert lib.st_kmeans_update(data(), p, p, p, K, p, p, p, p, None) == -22
        assert lib.st_kmeans_relocate(data(), p, p, p, K, p, None) == -22
    assert lib.st_kmeans_assign(data(), None, 2, p, p, None) == -22 and lib.st_kmeans_assign(data(), p, 2, None, p, None) == -22
    assert lib.st_kmeans_update(data(), p, p, p, 2, p, p, p, None, None) == -22 and lib.st_kmeans_update(data(), p, p, p, 2, p, p, p, p + 4, None) == -22
    assert lib.st_kmeans_relocate(data(), p, p, None, 2, p, None) == -22
    assert lib.st_kmeans_pp_step(data(), p, 2, 2, p, p, p, None) == -22 and lib.st_kmeans_pp_step(data(), p, -1, 2, p, p, p, None) == -22
    assert lib.st_kmeans_pp_pick(data(), p, p, p, 2, 2, p, p, p, None) == -22 and lib.st_kmeans_pp_pick(data(), p, p, None, 0, 2, p, p, p, None) == -22


def test_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import _lib, kmeans, ops, toolops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)
    host = torch.rand(10, 4)
    for x in (host, [[1.0]], None):
        for call in (lambda: ops.kmeans_assign(x, host), lambda: ops.kmeans_update(x, host, host, host), lambda: ops.kmeans_relocate(x, host, host, host, host),
                     lambda: ops.kmeans_pp_init(x, 2, [0.1, 0.2]), lambda: kmeans.fit(x, 2), lambda: kmeans.quantise(x, host)):
            with pytest.raises(ValueError, match='x must be a \\(N, D\\) float32 GPU tensor'):
                call()
    # a meta tensor stands in for a device tensor: the checks read .is_cuda / .device / .shape / .dtype / .stride() only
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    M = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device='meta')          # noqa: E731
    x, c, idx, dist, cnt = M(10, 4), M(3, 4), M(10, dtype=torch.int32), M(10), M(3, dtype=torch.int32)
    for bad, msg in ((M(10, 4, dtype=torch.float64), 'x must be'), (M(10), 'x must be'), (M(0, 4), '1 <= N'), (M(10, 0), 'D <= 256'), (M(10, 257), 'D <= 256'),
                     (M(4, 10).t(), 'strides'), (M(10, 8)[:, ::2], 'strides'), (M(1, 4).expand(10, 4), 'strides')):
        with pytest.raises(ValueError, match=msg):
            ops.kmeans_assign(bad, c)
        with pytest.raises(ValueError, match=msg):
            ops.kmeans_update(bad, idx, dist, c)
        with pytest.raises(ValueError, match=msg):
            ops.kmeans_relocate(bad, idx, dist, cnt, c)
        with pytest.raises(ValueError, match=msg):
            ops.kmeans_pp_init(bad, 2, [0.1, 0.2])
        with pytest.raises(ValueError, match=msg):
            kmeans.fit(bad, 2)
    assert toolops._km_data('t', M(10, 8)[:, 2:6]).ld == 8                              # a column slice of a wider buffer is taken as it is
    for bad in (M(3, 5), M(3, 4, dtype=torch.float64), M(4097, 4), M(0, 4), M(12), M(4, 3).t(), torch.zeros(3, 4), None):
        with pytest.raises(ValueError, match='kmeans_assign: cent must be'):
            ops.kmeans_assign(x, bad)
        with pytest.raises(ValueError, match='kmeans_update: cent_in must be'):
            ops.kmeans_update(x, idx, dist, bad)
        with pytest.raises(ValueError, match='kmeans_relocate: cent must be'):
            ops.kmeans_relocate(x, idx, dist, cnt, bad)
    for bad in (M(10, dtype=torch.int64), M(9, dtype=torch.int32), M(10, 1, dtype=torch.int32), torch.zeros(10, dtype=torch.int32), None):
        with pytest.raises(ValueError, match='kmeans_update: idx must be'):
            ops.kmeans_update(x, bad, dist, c)
        with pytest.raises(ValueError, match='kmeans_relocate: idx must be'):
            ops.kmeans_relocate(x, bad, dist, cnt, c)
    for bad in (M(10, dtype=torch.float64), M(11), M(20)[::2], None):
        with pytest.raises(ValueError, match='kmeans_update: dist must be'):
            ops.kmeans_update(x, idx, bad, c)
        with pytest.raises(ValueError, match='kmeans_relocate: dist must be'):
            ops.kmeans_relocate(x, idx, bad, cnt, c)
    for bad in (M(3, dtype=torch.int64), M(4, dtype=torch.int32), None):
        with pytest.raises(ValueError, match='kmeans_relocate: count must be'):
            ops.kmeans_relocate(x, idx, dist, bad, c)
    for K in (0, 4097, 2.0, True, None):
        with pytest.raises(ValueError, match='K must be an integer in \\[1, 4096\\]'):
            ops.kmeans_pp_init(x, K, [0.5])
        with pytest.raises(ValueError, match='K must be an integer in \\[1, 4096\\]'):
            kmeans.fit(x, K)
    for u in ([0.5], [0.5, 1.0], [0.5, -0.1], [0.5, float('nan')], M(2), M(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match='kmeans_pp_init: u must be'):
            ops.kmeans_pp_init(x, 2, u)
    for kw, msg in ((dict(K=11), 'K = 11 clusters of N = 10 rows'), (dict(init='random'), 'init'), (dict(iters=0), 'iters >= 1'), (dict(restarts=0), 'iters >= 1'),
                    (dict(tol=-1.0), 'tol >= 0'), (dict(tol=float('nan')), 'tol >= 0')):
        with pytest.raises(ValueError, match=msg):
            kmeans.fit(x, **dict(dict(K=2), **kw))
    for call in (lambda: ops.kmeans_assign(x, c), lambda: ops.kmeans_update(x, idx, dist, c), lambda: ops.kmeans_relocate(x, idx, dist, cnt, c),
                 lambda: ops.kmeans_pp_init(x, 2, [0.1, 0.2]), lambda: kmeans.quantise(x, c)):
        with pytest.raises(AssertionError, match='reached the device'):          # a good call gets as far as the library
            call()


def test_metrics_reexports_fit_and_quantise():
    from semi_tts_amd import kmeans, metrics
    assert metrics.kmeans_fit is kmeans.fit and metrics.quantise is kmeans.quantise and metrics.KMeansFit is kmeans.KMeansFit
    assert kmeans.KMeansFit._fields == ('centroids', 'idx', 'dist', 'inertia', 'n_iter', 'converged', 'history')


# ---------------------------------------------------------------- the tools
def _config():
    import yaml
    return yaml.load(open(os.path.join(REPO, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)


def test_kmeans_max_gb_refuses_before_the_device(tmp_path, monkeypatch):
    from semi_tts_amd import _lib, audio, solver
    from semi_tts_amd.audio import write_wav
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    monkeypatch.setattr(_lib, 'load', lambda *a, **k: (_ for _ in ()).throw(AssertionError('reached the device')))
    config = _config()
    sr = config['data']['audio']['sample_rate']
    wav = tmp_path / 'wav'
    wav.mkdir()

    class P:
        kmeans_wav_dir, kmeans_out, name, logdir, batch_size, resample = str(wav), str(tmp_path / 'book.npy'), 'km', str(tmp_path / 'log'), 4, False
        kmeans_max_gb, kmeans_k = None, 4
    with pytest.raises(ValueError, match='--kmeans-wav-dir .*: no .wav files'):
        solver.KMeansTrainer(config, P(), 'test').load_data()
    rs = np.random.RandomState(0)
    for k in range(3):
        write_wav(str(wav / ('u%d.wav' % k)), 0.1 * rs.randn(sr), sr)         # 1 s each: 101 MFCC frames
    tool = solver.KMeansTrainer(config, P(), 'test').load_data()
    hop = tool.audio_converter.hop_length_mfcc
    assert (tool.feat, tool.K, tool.iters, tool.tol, tool.init, tool.restarts) == ('mfcc', 4, 100, 1e-4, '++', 1)
    assert tool.max_rows == 3 * (1 + sr // hop) and tool.feature_dim() == 39 and tool.set_model().model is None
    P.kmeans_max_gb = (tool.max_rows * 39 * 4 - 1) / float(1 << 30)           # one byte short
    with pytest.raises(ValueError, match=r'3 files give up to %d rows of 39 columns, .* GiB of features; --kmeans-max-gb allows' % tool.max_rows):
        solver.KMeansTrainer(config, P(), 'test').load_data()
    P.kmeans_max_gb = (tool.max_rows * 39 * 4) / float(1 << 30)
    solver.KMeansTrainer(config, P(), 'test').load_data()
    P.kmeans_feat = 'mel'                                                      # wider rows at the mel hop: refused again
    with pytest.raises(ValueError, match='--kmeans-max-gb allows'):
        solver.KMeansTrainer(config, P(), 'test').load_data()
    P.kmeans_feat, P.kmeans_k = 'mfcc', tool.max_rows + 1
    with pytest.raises(ValueError, match='at most %d rows for --kmeans-k %d' % (tool.max_rows, tool.max_rows + 1)):
        solver.KMeansTrainer(config, P(), 'test').load_data()
    write_wav(str(wav / 'u3.wav'), 0.1 * rs.randn(sr // 2), sr // 2)
    P.kmeans_k = 4
    with pytest.raises(ValueError, match=r'--kmeans-wav-dir: sample rate mismatch. Expected %d but get %d .*u3\.wav' % (sr, sr // 2)):
        solver.KMeansTrainer(config, P(), 'test').load_data()
    assert not os.path.exists(P.logdir) and not os.path.exists(P.kmeans_out)


def test_unit_writer_refuses_a_foreign_codebook_in_load_data(tmp_path, monkeypatch):
    from semi_tts_amd import _lib, audio, solver
    from semi_tts_amd.audio import write_wav
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('reached the device')))
    monkeypatch.setattr(_lib, 'load', lambda *a, **k: (_ for _ in ()).throw(AssertionError('reached the device')))
    config = _config()
    sr = config['data']['audio']['sample_rate']
    wav = tmp_path / 'wav'
    wav.mkdir()
    write_wav(str(wav / 'u.wav'), 0.1 * np.random.RandomState(0).randn(sr // 2), sr)
    book = tmp_path / 'book.npy'

    class P:
        units_wav_dir, units_codebook, name, logdir, batch_size, resample = str(wav), str(book), 'units', str(tmp_path / 'log'), 4, False
    with pytest.raises(ValueError, match='--units-codebook .*not a readable .npy file'):
        solver.UnitWriter(config, P(), 'test').load_data()
    for table, msg in ((np.zeros((5, 40), np.float32), 'D = 40 columns, the features have 39'), (np.zeros((5, 39), np.float64), 'float32 array'),
                       (np.zeros(39, np.float32), 'float32 array'), (np.full((2, 39), np.nan, np.float32), 'non-finite')):
        np.save(str(book), table)
        with pytest.raises(ValueError, match=msg):
            solver.UnitWriter(config, P(), 'test').load_data()
    np.save(str(book), np.zeros((5, 39), np.float32))
    assert solver.UnitWriter(config, P(), 'test').load_data().codebook.shape == (5, 39)
    P.kmeans_feat = 'mel'
    with pytest.raises(ValueError, match='D = 39 columns, the features have %d' % config['data']['audio']['num_mels']):
        solver.UnitWriter(config, P(), 'test').load_data()


def test_merge_of_repeats():
    from semi_tts_amd.solver import merge_repeats
    assert merge_repeats([]) == [] and merge_repeats([4]) == [4] and merge_repeats([2, 2, 2]) == [2]
    assert merge_repeats([1, 1, 0, 0, 0, 1, 2, 2, 1]) == [1, 0, 1, 2, 1] and merge_repeats(np.array([7, 7, 8], np.int32)) == [7, 8]


def test_unit_transcripts_are_read_back_with_their_ids(tmp_path):
    from semi_tts_amd import ngram, solver
    from semi_tts_amd.ctc_align import read_phn, read_phn_paths
    units = [49, 49, 0, 0, 0, 17, -1, 17, 49, 1, 1]
    dist = [1.0, 3.0, 2.0, 2.0, 2.0, 0.5, float('nan'), 1.5, 4.0, 0.0, 0.0]
    text = solver.format_units(units, dist)
    want = [52, 3, 20, 52, 4]                                       # 3 + unit, repeats merged, the NaN frame left out
    assert text == '%.6f\t%s\n' % (-1.6, ' '.join(str(i) for i in want)) == solver.format_phn([-1.6], [want], None)
    path = tmp_path / 'u.phn'
    path.write_text(text)
    assert read_phn(str(path)) == want and read_phn_paths(str(path), None) == [want]
    assert min(want) >= 3                                           # the special ids 0 .. 2 stay free
    counts = ngram.count_ngrams([read_phn(str(path))], 3 + 50, 2)
    assert counts.sum() == 5 and counts[1, 52] == 1 and counts[52, 3] == 1 and counts[3, 20] == 1 and counts[20, 52] == 1 and counts[52, 4] == 1
    assert solver.format_units([-1, -1], [float('nan')] * 2) == '0.000000\t\n' and read_phn(str(path)) == want
    # --score-phn-dir pairs and reads the files as they are
    hyp, ref = tmp_path / 'hyp', tmp_path / 'ref'
    hyp.mkdir()
    ref.mkdir()
    (hyp / 'u.phn').write_text(text)
    (ref / 'u.phn').write_text(solver.format_units([49, 0, 17, 17, 2], [1.0] * 5))

    class P:
        score_phn_dir, score_ref_dir, name, logdir, batch_size, vocab = str(hyp), str(ref), 'per', str(tmp_path / 'log'), 4, None
    sc = solver.PhnScorer(None, P(), 'test').load_data()
    assert sc.hyps == [[want]] and sc.refs == [[52, 3, 20, 5]] and sc.n_classes == 53


def test_build_lm_takes_the_unit_transcripts_of_the_default_codebook(tmp_path, capsys):
    """--units-wav-dir under the default K = 50 writes ids up to 52: --build-lm-phn-dir --lm-classes 53 counts them, 43 classes refuse them"""
    import main
    from semi_tts_amd import ngram, solver
    phn = tmp_path / 'units'
    phn.mkdir()
    (phn / 'a.phn').write_text(solver.format_units([49, 49, 0, 17, 17, 49], [1.0] * 6))
    (phn / 'b.phn').write_text(solver.format_units([0, 0, 49, 3], [2.0] * 4))
    out = str(tmp_path / 'units.2gram.npy')
    main.main(['--build-lm-phn-dir', str(phn), '--lm', out, '--lm-order', '2', '--lm-classes', '53'])
    assert '2-gram table over 53 classes from 2 .phn files (7 tokens' in capsys.readouterr().out
    table = np.load(out)
    assert table.shape == (53, 53) and table[52, 3] > table[52, 4] and table[3, 20] > table[3, 21]          # 49 -> 0 and 0 -> 17 were seen
    with pytest.raises(ValueError, match='id 52 outside the 43 classes of the table .*--lm-classes'):
        ngram.build_lm_from_phn_dir(str(phn), str(tmp_path / 'no.npy'), 2)
    assert not os.path.exists(str(tmp_path / 'no.npy'))
    for argv in (['--lm-classes', '53'], ['--build-lm-phn-dir', str(phn), '--lm', out, '--lm-order', '4', '--lm-classes', '100'],
                 ['--build-lm-phn-dir', str(phn), '--lm', out, '--lm-order', '2', '--lm-classes', '1']):
        with pytest.raises(SystemExit):
            main.parse_args(argv + ['--no-msg'])


def test_help_lists_the_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'main.py'), '--help'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout
    for flag in ('--kmeans-wav-dir', '--kmeans-out', '--kmeans-feat', '--kmeans-k', '--kmeans-iters', '--kmeans-tol', '--kmeans-init', '--kmeans-restarts',
                 '--kmeans-max-gb', '--units-wav-dir', '--units-codebook', '--units-frames', '--abx-codebook', '--lm-classes'):
        assert flag in out, flag


def test_parser_pairs_the_flags():
    import main
    cfg = os.path.join(REPO, 'config', 'supervised.yaml')
    p = main.parse_args(['--config', cfg, '--kmeans-wav-dir', 'w', '--kmeans-out', 'b.npy', '--no-msg'])
    assert (p.kmeans_k, p.kmeans_iters, p.kmeans_tol, p.kmeans_restarts, p.kmeans_max_gb, p.kmeans_feat, p.kmeans_init) == (50, 100, 1e-4, 1, 8.0, None, None)
    assert next(name for flag, name in main.TOOLS if getattr(p, flag) not in (None, False)) == 'KMeansTrainer'
    p = main.parse_args(['--config', cfg, '--units-wav-dir', 'w', '--units-codebook', 'b.npy', '--units-frames', '--kmeans-feat', 'mel', '--no-msg'])
    assert next(name for flag, name in main.TOOLS if getattr(p, flag) not in (None, False)) == 'UnitWriter' and p.units_frames
    for argv in (['--kmeans-k', '8'], ['--kmeans-out', 'b.npy'], ['--units-codebook', 'b.npy'], ['--units-frames'], ['--kmeans-feat', 'mel'],
                 ['--abx-codebook', 'b.npy'], ['--config', cfg, '--kmeans-wav-dir', 'w'], ['--config', cfg, '--units-wav-dir', 'w'],
                 ['--kmeans-wav-dir', 'w', '--kmeans-out', 'b.npy'], ['--config', cfg, '--kmeans-wav-dir', 'w', '--kmeans-out', 'b.npy', '--kmeans-k', '4097'],
                 ['--config', cfg, '--kmeans-wav-dir', 'w', '--kmeans-out', 'b.npy', '--units-wav-dir', 'w', '--units-codebook', 'b.npy'],
                 ['--config', cfg, '--kmeans-wav-dir', 'w', '--kmeans-out', 'b.npy', '--feat-wav-dir', 'w'],
                 ['--config', cfg, '--abx-ali-dir', 'a', '--abx-wav-dir', 'w', '--abx-feat', 'code', '--abx-codebook', 'b.npy']):
        with pytest.raises(SystemExit):
            main.parse_args(argv + ['--no-msg'])
