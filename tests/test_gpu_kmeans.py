"""The k-means kernels on the device against the float64 oracle of tests/kmeans_oracle.py: st_kmeans_assign exactly on integer data and
within the first-order bound on float data, st_kmeans_update bit for bit on integer data (its sums in the documented order) and within
the float64 bound on float data, st_kmeans_relocate, the k-means++ seeding, kmeans.fit step by step, and the three command-line paths.

What varies inside the kernels: D <= 40 keeps a lane's rows in registers, a wider row is re-read in chunks of 40 columns; a lane owns two
points and a workgroup 512; the centroids pass in tiles of 16 rows, at most 8192 floats a tile (D = 256: 32 rows, so K = 4096 takes 128
tiles); the update cuts the points into chunks of 1024 and a cluster's members into slabs of 256.  The shapes below straddle each."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import kmeans_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 1, 1), (63, 3, 2), (64, 4, 7), (65, 13, 50), (1000, 39, 64), (1000, 39, 65), (4099, 80, 512), (257, 129, 1000), (300, 256, 4096)]
FLOAT_SHAPES = [(4096, 39, 50), (5000, 80, 512), (3000, 64, 256)]
_CACHE = {}


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _int_case(N, D, K):
    """integer coordinates in [-8, 8]: every fp32 intermediate of either distance form is exact.  Computed once per shape."""
    key = ('int', N, D, K)
    if key not in _CACHE:
        rs = np.random.RandomState(N + 7 * D + 13 * K)
        x = rs.randint(-8, 9, (N, D)).astype(np.float32)
        c = rs.randint(-8, 9, (K, D)).astype(np.float32)
        idx, dist = O.assign(x, c)
        _CACHE[key] = (x, c, idx, dist)
    return _CACHE[key]


def _float_case(N, D, K, mean):
    """standard normal rows around `mean`, the centroids one Lloyd step from K of the rows -> (x, c, d64 (N, K))"""
    key = ('float', N, D, K, mean)
    if key not in _CACHE:
        rs = np.random.RandomState(N + D + K + int(mean))
        x = (rs.randn(N, D) + mean).astype(np.float32)
        c0 = x[rs.choice(N, K, replace=False)]
        idx0, dist0 = O.assign(x, c0)
        c = O.update(x, idx0, dist0, c0)[0]
        _CACHE[key] = (x, c, O.sqdist(x, c))
    return _CACHE[key]


def _eps(x, c):
    """the first-order bound of either fp32 distance form: (D + 3) 2^-24 (||x_n|| + max_k ||c_k||)^2 per point"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (x.shape[1] + 3) * 2.0 ** -24 * (np.sqrt((x * x).sum(1)) + np.sqrt((c * c).sum(1)).max()) ** 2


def _margin(d64):
    if d64.shape[1] == 1:
        return np.full(d64.shape[0], np.inf)
    part = np.partition(d64, 1, axis=1)
    return part[:, 1] - part[:, 0]


def _check_assign(x, c, d64, idx, dist=None, cap=0.01):
    """the fp32 step check of the assignment: the share of close calls on the oracle alone, then the device's result"""
    eps, margin, best = _eps(x, c), _margin(d64), d64.argmin(1)
    share = float((margin <= 2 * eps).mean())
    print('share of points within 2 eps of a tie: %.4f %%' % (100 * share))
    assert share <= cap
    idx = np.asarray(idx)
    assert idx.min() >= 0 and idx.max() < c.shape[0]
    own = d64[np.arange(len(idx)), idx]
    if dist is not None:
        err = np.abs(np.asarray(dist, np.float64) - own)
        print('max |dist - d64[idx]| / eps: %.4f' % float((err / eps).max()))
        assert (err <= eps).all()
    assert (own - d64.min(1) <= 2 * eps).all()
    clear = margin > 2 * eps
    assert np.array_equal(idx[clear], best[clear])


def _check_update(x, idx, cent_in, cent_out, count=None):
    """the fp32 step check of the update: |cent_out - c64| <= 2^-24 |c64| + 2^-52 sum_n |x[n, d]| over the members, per entry"""
    ref, cnt, _, c64 = O.update(x, idx, np.zeros(len(idx)), cent_in)
    x64, idx = np.asarray(x, np.float64), np.asarray(idx)
    mass = np.zeros_like(c64)
    np.add.at(mass, idx[idx >= 0], np.abs(x64[idx >= 0]))
    bound = 2.0 ** -24 * np.abs(c64) + 2.0 ** -52 * mass
    err = np.abs(np.asarray(cent_out, np.float64) - c64)
    assert (err[cnt > 0] <= bound[cnt > 0]).all()
    assert np.array_equal(_bits32(np.asarray(cent_out)[cnt == 0]), _bits32(np.asarray(cent_in)[cnt == 0]))
    if count is not None:
        assert np.array_equal(np.asarray(count), cnt)


# ---------------------------------------------------------------- 1. assign, exact
def _assign_exact(x, c, xd=None):
    from semi_tts_amd import toolops
    idx_o, dist_o = O.assign(x, c)
    idx, dist = toolops.kmeans_assign(_dev(x) if xd is None else xd, _dev(c))
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), idx_o)
    assert np.array_equal(_bits32(dist.cpu().numpy()), _bits32(dist_o))
    return idx_o, dist_o


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_assign_integer_data_is_the_oracle_bit_for_bit(N, D, K):
    from semi_tts_amd import toolops
    x, c, idx_o, dist_o = _int_case(N, D, K)
    idx, dist = toolops.kmeans_assign(_dev(x), _dev(c))
    assert np.array_equal(idx.cpu().numpy(), idx_o)
    assert np.array_equal(_bits32(dist.cpu().numpy()), _bits32(dist_o))


def test_assign_duplicated_centroids_lowest_k_wins():
    x, c = _int_case(1000, 39, 64)[:2]
    c = c.copy()
    c[40], c[41], c[63] = c[3], c[3], c[17]
    idx_o, _ = _assign_exact(x, c)
    assert not np.isin(idx_o, [40, 41, 63]).any() and (idx_o == 3).any() and (idx_o == 17).any()
    c[:] = c[0]                                  # every centroid the same: all points go to 0
    assert (_assign_exact(x, c)[0] == 0).all()


def test_assign_more_centroids_than_points():
    rs = np.random.RandomState(5)
    _assign_exact(rs.randint(-8, 9, (5, 3)).astype(np.float32), rs.randint(-8, 9, (40, 3)).astype(np.float32))


def test_assign_rows_of_a_wider_buffer():
    rs = np.random.RandomState(6)
    wide = rs.randint(-8, 9, (700, 64)).astype(np.float32)
    c = rs.randint(-8, 9, (33, 41)).astype(np.float32)
    xd = _dev(wide)[:, 5:46]
    assert xd.stride(0) == 64 and not xd.is_contiguous()
    _assign_exact(wide[:, 5:46], c, xd)


def test_assign_nan_rows_get_minus_one():
    from semi_tts_amd import toolops
    x, c = _int_case(1000, 39, 65)[:2]
    x = x.copy()
    x[0, 38], x[511, 0], x[999, 20] = np.nan, np.nan, np.nan
    idx_o, dist_o = O.assign(x, c)
    idx, dist = toolops.kmeans_assign(_dev(x), _dev(c))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(idx, idx_o) and (idx == -1).sum() == 3 and np.isnan(dist[[0, 511, 999]]).all()
    keep = idx >= 0
    assert np.array_equal(_bits32(dist[keep]), _bits32(dist_o[keep]))


def test_assign_infinite_rows_are_no_members():
    from semi_tts_amd import toolops
    x, c = _int_case(1000, 39, 65)[:2]
    x = x.copy()
    x[5, 0], x[700, 38] = np.inf, -np.inf
    idx_o, dist_o = O.assign(x, c)
    idx, dist = toolops.kmeans_assign(_dev(x), _dev(c))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(idx, idx_o) and idx[5] == -1 and idx[700] == -1 and (idx == -1).sum() == 2 and np.isnan(dist[[5, 700]]).all()
    out, count, stats = toolops.kmeans_update(_dev(x), _dev(idx), _dev(dist), _dev(c))
    assert stats.cpu().numpy()[3] == 2 and np.isfinite(out.cpu().numpy()).all() and int(count.sum()) == 998


# ---------------------------------------------------------------- 2. assign, fp32
@pytest.mark.parametrize('mean', [0.0, 3.0])
@pytest.mark.parametrize('N,D,K', FLOAT_SHAPES)
def test_assign_float_data_within_the_first_order_bound(N, D, K, mean):
    from semi_tts_amd import toolops
    x, c, d64 = _float_case(N, D, K, mean)
    eps, margin = _eps(x, c), _margin(d64)
    assert float((margin <= 2 * eps).mean()) <= 0.01         # (on the oracle alone, before the device is asked)
    idx, dist = toolops.kmeans_assign(_dev(x), _dev(c))
    _check_assign(x, c, d64, idx.cpu().numpy(), dist.cpu().numpy())


# ---------------------------------------------------------------- 3. update
def _update(x, idx, dist, cent_in):
    from semi_tts_amd import toolops
    out, count, stats = toolops.kmeans_update(_dev(x), _dev(idx, torch.int32), _dev(dist, torch.float32), _dev(cent_in))
    return out.cpu().numpy(), count.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_update_integer_data_is_the_oracle_bit_for_bit(N, D, K):
    x, c, idx_o, dist_o = _int_case(N, D, K)
    ref_out, ref_count, ref_stats, _ = O.update(x, idx_o, dist_o, c)
    out, count, stats = _update(x, idx_o, dist_o, c)
    assert np.array_equal(count, ref_count) and count.dtype == np.int32
    assert np.array_equal(_bits32(out), _bits32(ref_out))
    assert np.array_equal(_bits64(stats), _bits64(ref_stats))
    assert stats[2] == (ref_count == 0).sum() and stats[3] == 0


@pytest.mark.parametrize('N,D,K', FLOAT_SHAPES)
def test_update_float_data_within_the_float64_bound_and_repeatable(N, D, K):
    x, c, d64 = _float_case(N, D, K, 3.0)
    idx = d64.argmin(1).astype(np.int32)
    dist = d64.min(1).astype(np.float32)
    out, count, stats = _update(x, idx, dist, c)
    _check_update(x, idx, c, out, count)
    ref = float(np.sum(dist.astype(np.float64)))
    assert abs(stats[0] - ref) <= N * 2.0 ** -52 * ref
    out2, count2, stats2 = _update(x, idx, dist, c)
    assert np.array_equal(_bits32(out), _bits32(out2)) and np.array_equal(count, count2) and np.array_equal(_bits64(stats), _bits64(stats2))


def test_update_empty_clusters_keep_their_rows_and_nan_rows_are_left_out():
    x, c, idx_o, dist_o = _int_case(1000, 39, 65)
    idx, dist = idx_o.copy(), dist_o.copy()
    idx[idx == 7] = 8                               # cluster 7 loses its members
    idx[[3, 600, 999]] = -1
    dist[[3, 600, 999]] = np.nan
    ref_out, ref_count, ref_stats, _ = O.update(x, idx, dist, c)
    out, count, stats = _update(x, idx, dist, c)
    assert count[7] == 0 and np.array_equal(_bits32(out[7]), _bits32(c[7])) and stats[2] >= 1 and stats[3] == 3
    assert np.array_equal(count, ref_count) and np.array_equal(_bits32(out), _bits32(ref_out)) and np.array_equal(_bits64(stats), _bits64(ref_stats))


@pytest.mark.parametrize('K', [1, 5])
def test_update_one_cluster_holds_every_point(K):
    x, c = _int_case(4099, 80, 512)[:2]
    c = c[:K]
    idx = np.full(4099, K - 1, np.int32)
    dist = O.sqdist(x, c[K - 1:K])[:, 0]
    ref_out, ref_count, ref_stats, _ = O.update(x, idx, dist, c)
    out, count, stats = _update(x, idx, dist, c)
    assert count[K - 1] == 4099 and stats[2] == K - 1
    assert np.array_equal(count, ref_count) and np.array_equal(_bits32(out), _bits32(ref_out)) and np.array_equal(_bits64(stats), _bits64(ref_stats))


# ---------------------------------------------------------------- 4. relocate
def _relocate(x, idx, dist, count, cent):
    from semi_tts_amd import toolops
    return toolops.kmeans_relocate(_dev(x), _dev(idx, torch.int32), _dev(dist, torch.float32), _dev(count, torch.int32), _dev(cent)).cpu().numpy()


def test_relocate_takes_the_farthest_points_lower_index_first():
    rs = np.random.RandomState(11)
    x = rs.randint(-8, 9, (200, 6)).astype(np.float32)
    x[150] = x[20]                                  # a tie in dist: the lower index goes first
    c = np.stack([x[:100].mean(0).round(), np.full(6, 500.0), x[100:].mean(0).round(), np.full(6, -500.0)]).astype(np.float32)
    idx, dist = O.assign(x, c)
    dist[20] = dist[150] = dist.max() + 1.0         # the tied pair is the farthest
    out, count, stats, _ = O.update(x, idx, dist, c)
    assert count[1] == 0 and count[3] == 0 and stats[2] == 2
    ref, taken = O.relocate(x, idx, dist, count, out)
    assert taken.tolist() == [20, 150]
    got = _relocate(x, idx, dist, count, out)
    assert np.array_equal(_bits32(got), _bits32(ref))
    assert np.array_equal(got[1], x[20]) and np.array_equal(got[3], x[150]) and np.array_equal(got[[0, 2]], out[[0, 2]])


def test_relocate_more_empty_clusters_than_points():
    x = np.array([[1, 2, 3], [4, 5, 6], [np.nan, 0, 0]], np.float32)
    c = np.array([[2, 3, 4]] + [[100 * k, 0, 0] for k in range(1, 6)], np.float32)
    idx, dist = O.assign(x, c)
    assert idx.tolist() == [0, 0, -1]
    out, count, stats, _ = O.update(x, idx, dist, c)
    ref, taken = O.relocate(x, idx, dist, count, out)
    assert stats[2] == 5 and taken.tolist() == [1, 0]           # (dist 12 before dist 3)
    got = _relocate(x, idx, dist, count, out)
    assert np.array_equal(_bits32(got), _bits32(ref))
    assert np.array_equal(got[1], x[1]) and np.array_equal(got[2], x[0]) and np.array_equal(got[3:], c[3:])


# ---------------------------------------------------------------- 5. seeding
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_seeding_integer_data_picks_the_oracles_rows(seed):
    from semi_tts_amd import toolops
    rs = np.random.RandomState(40 + seed)
    x = rs.randint(-8, 9, (300, 5)).astype(np.float32)
    x[rs.choice(300, 20, replace=False)] = x[rs.choice(300, 20)]          # 20 duplicated rows
    u = np.random.default_rng(seed).random(17)
    picks_o, mind_o = O.pp_init(x, 17, u)
    cent, picks, mind = toolops.kmeans_pp_init(_dev(x), 17, u)
    assert picks.cpu().numpy().tolist() == picks_o.tolist()
    assert np.array_equal(cent.cpu().numpy(), x[picks_o])
    assert np.array_equal(_bits32(mind.cpu().numpy()), _bits32(mind_o))


@pytest.mark.parametrize('N,D,K', [(5000, 39, 50), (1500, 80, 64)])
def test_seeding_float_data_never_picks_a_chosen_row(N, D, K):
    from semi_tts_amd import toolops
    x = _float_case(5000, 80, 512, 3.0)[0][:N, :D].copy()
    u = np.random.default_rng(3).random(K)
    cent, picks, mind = toolops.kmeans_pp_init(_dev(x), K, u)
    picks = picks.cpu().numpy()
    assert picks[0] == int(np.floor(u[0] * N)) and len(set(picks.tolist())) == K      # distinct rows: no pick had mind == 0
    d64 = O.sqdist(x, x[picks])
    for j in range(1, K):
        assert d64[picks[j], :j].min() > 0
    assert np.array_equal(cent.cpu().numpy(), x[picks])
    assert (np.abs(mind.cpu().numpy().astype(np.float64) - d64.min(1)) <= _eps(x, x[picks])).all()


def test_seeding_as_many_centres_as_rows_picks_every_row_once():
    from semi_tts_amd import toolops
    rs = np.random.RandomState(9)
    x = rs.permutation(33 * 4).reshape(33, 4).astype(np.float32)
    u = np.random.default_rng(9).random(33)
    cent, picks, mind = toolops.kmeans_pp_init(_dev(x), 33, u)
    assert sorted(picks.cpu().numpy().tolist()) == list(range(33)) and (mind.cpu().numpy() == 0).all()
    assert picks.cpu().numpy().tolist() == O.pp_init(x, 33, u)[0].tolist()


def test_seeding_fewer_distinct_rows_than_centres_raises():
    from semi_tts_amd import toolops
    from semi_tts_amd.kmeans import fit
    rs = np.random.RandomState(10)
    x = rs.randint(-8, 9, (5, 4)).astype(np.float32)[np.arange(40) % 5]
    with pytest.raises(ValueError, match='fewer than K = 6 distinct rows'):
        toolops.kmeans_pp_init(_dev(x), 6, np.random.default_rng(0).random(6))
    with pytest.raises(ValueError, match='distinct rows'):
        fit(_dev(x), 6)
    assert toolops.kmeans_pp_init(_dev(x), 5, np.random.default_rng(0).random(5))[1].cpu().numpy().tolist() == O.pp_init(x, 5, np.random.default_rng(0).random(5))[0].tolist()


# ---------------------------------------------------------------- 6. fit
FIT_SEED = 2        # found on the CPU: the oracle's lloyd from its own k-means++ recovers the planted partition (two of its eight picks
#                     fall into one blob, so Lloyd has work to do: 4 iterations); seeds 0 .. 11 all do except 8, which ends in a local optimum


def _blobs():
    rs = np.random.RandomState(7)
    label = np.arange(2048) % 8
    centres = np.zeros((8, 13), np.float32)
    centres[np.arange(8), np.arange(8)] = 20.0      # 20 sqrt(2) sigma apart
    return (centres[label] + rs.randn(2048, 13)).astype(np.float32), label


def test_fit_recovers_planted_blobs_step_by_step():
    from semi_tts_amd.kmeans import fit, quantise
    x, label = _blobs()
    picks_o, _ = O.pp_init(x, 8, np.random.default_rng(FIT_SEED).random(8))
    _, idx_o, _, hist_o, conv_o = O.lloyd(x, x[picks_o])
    assert conv_o and len(set(zip(idx_o.tolist(), label.tolist()))) == 8
    steps = []

    def on_step(it, cent_in, idx, cent_out):
        cin, ids, cout = cent_in.cpu().numpy(), idx.cpu().numpy(), cent_out.cpu().numpy()
        _check_assign(x, cin, O.sqdist(x, cin), ids)
        _check_update(x, ids, cin, cout)
        steps.append(it)

    xd = _dev(x)
    km = fit(xd, 8, seed=FIT_SEED, on_step=on_step)
    assert steps == list(range(km.n_iter)) and km.converged and 1 <= km.n_iter <= 10
    assert [h[0] for h in km.history] == steps and all(h[3] == 0 for h in km.history)
    inertia = [h[1] for h in km.history] + [km.inertia]
    assert all(b <= a * (1 + 1e-6) for a, b in zip(inertia, inertia[1:]))
    idx = km.idx.cpu().numpy()
    assert len(set(zip(idx.tolist(), label.tolist()))) == 8 and (np.bincount(idx) == 256).all()
    q_idx, q_dist = quantise(xd, km.centroids)
    assert torch.equal(q_idx, km.idx) and torch.equal(q_dist, km.dist)
    # the same partition, so the same means: the two inertias differ by the fp32 error of the device's distances, eps_n a point
    assert abs(km.inertia - hist_o[-1][1]) <= _eps(x, km.centroids.cpu().numpy()).sum() + 1e-9 * km.inertia
    assert km.centroids.shape == (8, 13) and km.centroids.dtype == torch.float32


def test_fit_restarts_keep_the_lowest_inertia():
    from semi_tts_amd.kmeans import fit
    xd = _dev(_blobs()[0])
    single = [fit(xd, 8, seed=s) for s in (8, 9, 10)]
    best = min(single, key=lambda r: r.inertia)
    km = fit(xd, 8, seed=8, restarts=3)
    assert km.inertia == best.inertia and torch.equal(km.centroids, best.centroids) and torch.equal(km.idx, best.idx)
    sample = fit(xd, 8, init='sample', seed=1, iters=3)
    assert sample.n_iter <= 3 and sample.centroids.shape == (8, 13)


# ---------------------------------------------------------------- 7. the command line
SR = 22050
ALI = {     # symbol, start frame, end frame at frame_s = 0.05: 12 frames = 0.6 s
    'k1': [('sil', 0, 2), ('a', 2, 4), ('sil', 4, 6), ('b', 6, 9), ('sil', 9, 12)],
    'k2': [('sil', 1, 2), ('b', 2, 5), ('sil', 5, 7), ('a', 7, 9), ('sil', 9, 11)],
    'k3': [('sil', 0, 3), ('a', 3, 6), ('c', 6, 9), ('sil', 9, 12)],
    'k4': [('c', 0, 3), ('sil', 3, 5), ('b', 5, 8), ('a', 8, 12)],
    'k5': [('a', 0, 4), ('b', 4, 7), ('sil', 7, 9), ('c', 9, 12)],
    'k6': [('sil', 0, 1), ('c', 1, 5), ('a', 5, 8), ('b', 8, 12)],
}
ABX_ARGS = ['--abx-context', 'none', '--abx-ignore', 'sil', '--batch-size', '4']
CFG = os.path.join(REPO, 'config', 'supervised.yaml')
# abx.csv of make_dirs' files as the Python sources of commit 0702108 (the parent of --abx-codebook) wrote it on an MI355X for
# main.py --config config/supervised.yaml --abx-ali-dir ALI --abx-wav-dir WAVS + ABX_ARGS
PARENT_ABX = os.path.join(REPO, 'tests', 'golden', 'kmeans_abx_parent.csv')


def _wave(L, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / SR
    f0 = 110 + 90 * rs.rand() + 30 * np.sin(2 * np.pi * 2.5 * t + rs.rand())
    ph = 2 * np.pi * np.cumsum(f0) / SR
    return (0.5 * sum(np.sin((h + 1) * ph + rs.rand()) / (h + 1) for h in range(6)) * (0.3 + 0.7 * rs.rand(L // 2205 + 1).repeat(2205)[:L])
            + 0.01 * rs.randn(L)).astype(np.float32)


def make_dirs(root):
    """six short synthetic recordings and their alignments under `root` -> (ali_dir, wav_dir)"""
    from semi_tts_amd.audio import write_wav
    ali_dir, wav_dir = os.path.join(root, 'ali'), os.path.join(root, 'wav')
    os.makedirs(ali_dir)
    os.makedirs(wav_dir)
    for k, (stem, toks) in enumerate(ALI.items()):
        write_wav(os.path.join(wav_dir, stem + '.wav'), _wave(13230 + 441 * k, 160 + k), SR)
        with open(os.path.join(ali_dir, stem + '.ali'), 'w') as f:
            f.write('# score=-1.000000 frames=12 frame_s=0.050000\n' + ''.join(
                '%s\t%d\t%d\t%.6f\t%.6f\n' % (s, a, b, a * 0.05, b * 0.05) for s, a, b in toks))
    return ali_dir, wav_dir


@pytest.fixture(scope='module')
def unit_dirs(tmp_path_factory):
    """the directories, and the codebook --kmeans-wav-dir fits to them (K = 8 over the MFCC of the six files)"""
    import main
    root = tmp_path_factory.mktemp('kmeans')
    ali_dir, wav_dir = make_dirs(str(root))
    log, book = str(root / 'log'), str(root / 'book' / 'units8.npy')
    main.main(['--config', CFG, '--kmeans-wav-dir', wav_dir, '--kmeans-out', book, '--kmeans-k', '8', '--kmeans-restarts', '2', '--logdir', log,
               '--name', 'fit', '--batch-size', '4', '--seed', '3'])
    return ali_dir, wav_dir, log, book


def _features(wav_dir):
    """the MFCC of the six files, file by file -> (packed (rows, 39) device buffer, rows per file)"""
    import yaml
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(**yaml.load(open(CFG), Loader=yaml.FullLoader)['data']['audio'])
    parts, rows = [], []
    for stem in sorted(ALI):
        x = conv.load(os.path.join(wav_dir, stem + '.wav'))[0]
        n = 1 + len(x) // conv.hop_length_mfcc
        parts.append(conv.extract_mfcc_batch([x])[0, :n])
        rows.append(n)
    return torch.cat(parts, 0).contiguous(), rows, conv


def test_kmeans_wav_dir_writes_codebook_and_tables(unit_dirs):
    from semi_tts_amd.kmeans import quantise
    _, wav_dir, log, book = unit_dirs
    table = np.load(book)
    assert table.shape == (8, 39) and table.dtype == np.float32 and np.isfinite(table).all()
    fit_rows = open(os.path.join(log, 'fit', 'kmeans.csv')).read().splitlines()
    assert fit_rows[0] == 'restart,iter,inertia,shift,empty' and {r.split(',')[0] for r in fit_rows[1:]} == {'0', '1'}
    assert all(len(r.split(',')) == 5 for r in fit_rows[1:])
    unit_rows = open(os.path.join(log, 'fit', 'kmeans_units.csv')).read().splitlines()
    feat, rows, _ = _features(wav_dir)
    idx, _ = quantise(feat, _dev(table))
    assert unit_rows == ['unit,frames'] + ['%d,%d' % (u, n) for u, n in enumerate(np.bincount(idx.cpu().numpy(), minlength=8).tolist())]
    assert sum(int(r.split(',')[1]) for r in unit_rows[1:]) == sum(rows)


def test_units_wav_dir_writes_the_quantised_sequences(unit_dirs):
    import main
    from semi_tts_amd.ctc_align import read_phn
    from semi_tts_amd.kmeans import quantise
    from semi_tts_amd.solver import merge_repeats
    _, wav_dir, log, book = unit_dirs
    main.main(['--config', CFG, '--units-wav-dir', wav_dir, '--units-codebook', book, '--units-frames', '--logdir', log, '--name', 'units',
               '--batch-size', '4', '--no-msg'])
    out = os.path.join(log, 'units')
    assert sorted(os.listdir(out)) == sorted([s + '.phn' for s in ALI] + [s + '-units.npy' for s in ALI])
    feat, rows, _ = _features(wav_dir)
    idx, dist = quantise(feat, _dev(np.load(book)))
    idx, dist, r0 = idx.cpu().numpy(), dist.cpu().numpy().astype(np.float64), 0
    for stem, n in zip(sorted(ALI), rows):
        units = np.load(os.path.join(out, stem + '-units.npy'))
        assert units.dtype == np.int32 and np.array_equal(units, idx[r0:r0 + n])
        assert read_phn(os.path.join(out, stem + '.phn')) == [3 + u for u in merge_repeats(units)]
        score = float(open(os.path.join(out, stem + '.phn')).read().split('\t')[0])
        assert abs(score + dist[r0:r0 + n].mean()) <= 1e-6 * max(1.0, dist[r0:r0 + n].mean())
        r0 += n


def _items(ali_dir, rows, conv):
    from semi_tts_amd import abx as A
    out, first = [], 0
    for stem, n in zip(sorted(ALI), rows):
        its, _ = A.utterance_items(A.read_ali(os.path.join(ali_dir, stem + '.ali')), conv.hop_length_mfcc / float(SR), n, ('sil',), 1)
        out += [(s, first + r0, ln, A.cell_key('spk', p, q, 'none')) for s, r0, ln, p, q in its]
        first += n
    return out


def test_abx_codebook_scores_the_quantised_rows_and_leaves_the_plain_run_alone(unit_dirs):
    import main
    from semi_tts_amd import abx as A
    from semi_tts_amd.kmeans import quantise
    from semi_tts_amd.metrics import abx
    ali_dir, wav_dir, log, book = unit_dirs
    base = ['--config', CFG, '--abx-ali-dir', ali_dir, '--abx-wav-dir', wav_dir, '--logdir', log, '--no-msg'] + ABX_ARGS
    main.main(base + ['--name', 'plain'])
    main.main(base + ['--name', 'discrete', '--abx-codebook', book])
    assert open(os.path.join(log, 'plain', 'abx.csv')).read() == open(PARENT_ABX).read()
    feat, rows, conv = _features(wav_dir)
    table = _dev(np.load(book))
    idx, _ = quantise(feat, table)
    quantised = table.index_select(0, idx.long()).contiguous()
    items = _items(ali_dir, rows, conv)
    names = sorted({r[0] for r in items})
    res = abx(quantised, [r[1] for r in items], [r[2] for r in items], [names.index(r[0]) for r in items], [0] * len(items), 'angular', 50, 0)
    assert names == ['a', 'b', 'c'] and open(os.path.join(log, 'discrete', 'abx.csv')).read() == A.format_abx_csv(res.table, names)
    assert open(os.path.join(log, 'discrete', 'abx.csv')).read() != open(os.path.join(log, 'plain', 'abx.csv')).read()
