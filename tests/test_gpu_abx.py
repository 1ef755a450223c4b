"""st_dtw_pairs and st_abx_count on the device against the numpy oracle of tests/abx_oracle.py (bit for bit where every intermediate is
exact in fp32, within the derived bound eps on Gaussian / Dirichlet rows), metrics.abx against the brute-force measure, and the
--abx-ali-dir path end to end.

The DTW kernel has one form per metric; what varies with the shape is the number of lanes a sweep uses (n up to 64: one lane a row),
the cells a lane takes in the distance phase (n m over 64), the 16-byte loads and the scalar tail of a row (D mod 4), and the waves of
a workgroup that have a pair (P mod 4).  The sizes below reach each of them."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import abx_oracle as O  # noqa: E402
import dtw_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_SIZES = (1, 2, 3, 31, 32, 33, 63, 64)
F64_SIZES = (1, 2, 5, 33, 64)


def _pack(items, stride=None, fill=0.0, gap=0):
    """a list of (n_i, D) arrays -> (device (rows, D) buffer -- a column slice of a (rows, stride) one with stride given --, starts, lens);
    `gap` rows of `fill` lie before every item"""
    D = items[0].shape[1]
    rows = sum(len(x) + gap for x in items) + gap
    buf = np.full((rows, stride or D), fill, np.float32)
    starts, r = [], 0
    for x in items:
        r += gap
        starts.append(r)
        buf[r:r + len(x), :D] = x
        r += len(x)
    t = torch.from_numpy(buf).to(DEV)
    return (t[:, :D] if stride else t), np.array(starts, np.int32), np.array([len(x) for x in items], np.int32)


def _run(feat, starts, lens, pa, pb, metric, max_len=None):
    """-> (dist, cost, path_len) numpy arrays"""
    from semi_tts_amd.metrics import dtw_pairs
    out = dtw_pairs(feat, starts, lens, np.asarray(pa, np.int32), np.asarray(pb, np.int32), metric, want_cost=True, max_len=max_len)
    torch.cuda.synchronize()
    dist, cost, plen = (o.cpu().numpy() for o in out)
    assert dist.dtype == cost.dtype == np.float32 and plen.dtype == np.int32 and dist.shape == cost.shape == plen.shape == (len(pa),)
    return dist, cost, plen


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _assert_dist_is_quotient(dist, cost, plen):
    ok = plen > 0
    assert np.array_equal(_bits(dist[ok]), _bits(cost[ok] / plen[ok].astype(np.float32)))
    assert np.isnan(dist[~ok]).all() and np.isnan(cost[~ok]).all()


# ---------------------------------------------------------------- 1. euclid, exact
@pytest.mark.parametrize('D', [1, 3])
def test_euclid_is_bitwise_the_float32_oracle_and_st_dtw_batch(D):
    from semi_tts_amd.metrics import dtw
    rs = np.random.RandomState(11 + D)
    items, pa, pb, want = [], [], [], []
    for n in EXACT_SIZES:
        for m in EXACT_SIZES:
            x, y = dtw_oracle.integer_pair(rs, n, m, D)
            pa.append(len(items))
            pb.append(len(items) + 1)
            items += [x, y]
            c, L = O.dtw_len(O.distances(x, y, 'euclid', np.float32))
            assert c == np.round(c) and max(n, m) <= L <= n + m - 1
            want.append((c, L))
    assert len(pa) == 64
    feat, starts, lens = _pack(items)
    dist, cost, plen = _run(feat, starts, lens, pa, pb, 'euclid')          # all pairs in one launch over one packed buffer
    assert np.array_equal(_bits(cost), _bits([c for c, _ in want])) and np.array_equal(plen, [L for _, L in want])
    _assert_dist_is_quotient(dist, cost, plen)
    # the same pairs through the workgroup-per-pair kernel: the two check each other
    x = np.zeros((64, 64, D), np.float32)
    y = np.zeros((64, 64, D), np.float32)
    for p in range(64):
        x[p, :len(items[2 * p])], y[p, :len(items[2 * p + 1])] = items[2 * p], items[2 * p + 1]
    total, path_len, _ = dtw(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), [len(items[2 * p]) for p in range(64)],
                             [len(items[2 * p + 1]) for p in range(64)], want_path=False)
    assert np.array_equal(_bits(total.cpu().numpy()), _bits(cost)) and np.array_equal(path_len.cpu().numpy(), plen)


# ---------------------------------------------------------------- 2. angular and kl against float64
def _rows(rs, metric, n, D):
    if metric == 'kl':
        return rs.dirichlet(np.full(D, 0.7), n).astype(np.float32)
    return rs.randn(n, D).astype(np.float32)


@pytest.mark.parametrize('metric,D', [('angular', D) for D in (1, 2, 13, 39, 64, 65, 512)] + [('kl', D) for D in (2, 40, 75)])
def test_angular_and_kl_within_the_derived_bound_of_float64(metric, D):
    rs = np.random.RandomState(1000 + D)
    items, pa, pb = [], [], []
    for n in F64_SIZES:
        for m in F64_SIZES:
            pa.append(len(items))
            pb.append(len(items) + 1)
            items += [_rows(rs, metric, n, D), _rows(rs, metric, m, D)]
    feat, starts, lens = _pack(items)
    dist, cost, plen = _run(feat, starts, lens, pa, pb, metric)
    _assert_dist_is_quotient(dist, cost, plen)
    worst = 0.0
    for p in range(len(pa)):
        x, y = items[pa[p]], items[pb[p]]
        n, m = len(x), len(y)
        d64 = O.distances(x, y, metric, np.float64)
        opt, _ = O.dtw_len(d64)
        e, c, L = O.eps(n, m, D, metric), float(cost[p]), int(plen[p])
        assert max(n, m) <= L <= n + m - 1, (n, m, L)
        worst = max(worst, abs(c - opt) / (e * opt + e * (n + m)))
        assert abs(c - opt) <= e * opt + e * (n + m), (n, m, c, opt, e)
        assert O.min_cost_with_len(d64, L) <= opt * (1 + 2 * e) + e * (n + m), (n, m, L)
    print('%s D=%d: worst |c - opt| / bound = %.4f' % (metric, D, worst))


# ---------------------------------------------------------------- 3. edges
def test_zero_rows_under_angular():
    rs = np.random.RandomState(3)
    z, x = np.zeros((4, 5), np.float32), rs.randn(4, 5).astype(np.float32)
    feat, starts, lens = _pack([z, x, z.copy()])
    dist, cost, plen = _run(feat, starts, lens, [0, 0, 1], [1, 2, 0], 'angular')
    assert dist[0] == 0.5 and dist[2] == 0.5 and cost[0] == 0.5 * plen[0] and plen[0] == 4         # every cell 0.5: the diagonal
    assert dist[1] == 0.0 and cost[1] == 0.0 and plen[1] == 4


@pytest.mark.parametrize('metric', ['euclid', 'angular'])
def test_an_item_against_itself(metric):
    rs = np.random.RandomState(4)
    items = [rs.randn(n, 13).astype(np.float32) for n in (1, 2, 7, 33, 64)]
    feat, starts, lens = _pack(items)
    dist, cost, plen = _run(feat, starts, lens, range(5), range(5), metric)
    assert (dist == 0).all() and (cost == 0).all() and plen.tolist() == [1, 2, 7, 33, 64]


@pytest.mark.parametrize('metric', ['euclid', 'angular', 'kl'])
def test_nan_inside_an_item_and_outside_all_items(metric):
    rs = np.random.RandomState(5)
    items = [_rows(rs, metric, n, 6) for n in (3, 5, 4, 6)]
    pa, pb = [0, 0, 0, 1, 1, 2, 2], [1, 2, 3, 2, 3, 3, 2]
    feat, starts, lens = _pack(items, gap=2, fill=1.0)
    clean = _run(feat, starts, lens, pa, pb, metric)
    assert np.isfinite(clean[0]).all()
    bad = feat.clone()
    bad[int(starts[2]) + 3, 4] = float('nan')                                  # the last row of item 2
    dist, cost, plen = _run(bad, starts, lens, pa, pb, metric)
    hit = np.array([2 in (a, b) for a, b in zip(pa, pb)])
    assert np.isnan(dist[hit]).all() and np.isnan(cost[hit]).all() and (plen[hit] == 0).all()
    for got, want in zip((dist, cost, plen), clean):
        assert np.array_equal(got[~hit].view(np.uint32), want[~hit].view(np.uint32))
    # NaN in the rows that belong to no item changes nothing, bitwise
    gaps = np.ones(feat.shape[0], bool)
    for s, n in zip(starts, lens):
        gaps[s:s + n] = False
    holes = feat.clone()
    holes[torch.from_numpy(gaps).to(DEV)] = float('nan')
    for got, want in zip(_run(holes, starts, lens, pa, pb, metric), clean):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_refused_pairs_are_nan_with_path_len_zero():
    from semi_tts_amd import ops
    rs = np.random.RandomState(6)
    items = [rs.randn(n, 3).astype(np.float32) for n in (4, 5, 9, 2)]
    feat, starts, lens = _pack(items)
    n_rows = feat.shape[0]
    # item 4: len 0; item 5: len max_len + 1 = 9 (item 2 itself has 9 rows); item 6: reaches past n_rows; item 7: starts before row 0
    starts = np.concatenate([starts, [0, 0, n_rows - 2, -1]]).astype(np.int32)
    lens = np.concatenate([lens, [0, 9, 3, 2]]).astype(np.int32)
    pa, pb = [0, -1, 0, 8, 4, 0, 2, 0, 6, 0, 7, 3], [1, 0, 8, 0, 0, 4, 0, 5, 0, 6, 0, 0]
    t = lambda v: torch.from_numpy(np.asarray(v, np.int32)).to(DEV)       # noqa: E731
    dist, cost, plen = (o.cpu().numpy() for o in ops.dtw_pairs(feat, t(starts), t(lens), t(pa), t(pb), 'euclid', 8, True))
    good = np.array([True] + [False] * 10 + [True])
    assert np.isfinite(dist[good]).all() and (plen[good] > 0).all()
    assert np.isnan(dist[~good]).all() and np.isnan(cost[~good]).all() and (plen[~good] == 0).all()


def test_negative_probability_under_kl():
    rs = np.random.RandomState(7)
    items = [_rows(rs, 'kl', 4, 5) for _ in range(3)]
    items[1][2, 3] = -0.25
    feat, starts, lens = _pack(items)
    dist, cost, plen = _run(feat, starts, lens, [0, 0, 1], [1, 2, 2], 'kl')
    assert np.isnan(dist[[0, 2]]).all() and (plen[[0, 2]] == 0).all() and np.isfinite(dist[1]) and plen[1] >= 4


# ---------------------------------------------------------------- 4. independence
@pytest.mark.parametrize('metric', ['angular', 'euclid'])
def test_a_pair_depends_on_its_two_items_alone(metric):
    rs = np.random.RandomState(8)
    lens_ = [1, 2, 5, 9, 17, 20, 33, 40]
    items = [rs.randn(n, 13).astype(np.float32) for n in lens_]
    feat, starts, lens = _pack(items)
    pa, pb = np.array([0, 1, 2, 3, 4, 5, 6, 7, 3]), np.array([7, 6, 5, 4, 3, 2, 1, 0, 3])
    alone = _run(feat, starts, lens, pa, pb, metric)
    # embedded at shuffled positions of a list of 1000
    where = rs.permutation(1000)[:len(pa)]
    big_a, big_b = rs.randint(0, 8, 1000), rs.randint(0, 8, 1000)
    big_a[where], big_b[where] = pa, pb
    for got, want in zip(_run(feat, starts, lens, big_a, big_b, metric), alone):
        assert np.array_equal(got[where].view(np.uint32), want.view(np.uint32))
    # row stride above D, and other rows around the items
    wide, s2, l2 = _pack(items, stride=17, fill=3.0, gap=1)
    assert wide.stride(0) == 17
    for got, want in zip(_run(wide, s2, l2, pa, pb, metric), alone):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # P not a multiple of the waves of a workgroup
    for P in (1, 3, 5, 257):
        qa, qb = np.resize(pa, P), np.resize(pb, P)
        for got, want in zip(_run(feat, starts, lens, qa, qb, metric), alone):
            assert np.array_equal(got.view(np.uint32), np.resize(want, P).view(np.uint32))
    # max_len 64 against the largest item, and twice the same call
    for got, same, want in zip(_run(feat, starts, lens, pa, pb, metric, max_len=64), _run(feat, starts, lens, pa, pb, metric, max_len=40), alone):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(same.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- 5. st_abx_count
@pytest.mark.parametrize('NB', [1, 300])
def test_abx_count_equals_brute_force(NB):
    from semi_tts_amd import ops
    rs = np.random.RandomState(9 + NB)
    mats, offs, off = [], [], 0
    for nc in (5, 40, 200):
        d = rs.randint(0, 6, (nc, nc)).astype(np.float32)            # small integers: ties abound
        d = np.triu(d, 1) + np.triu(d, 1).T
        nan = rs.rand(nc, nc) < 0.02
        d[nan | nan.T] = np.nan
        d[np.arange(nc), np.arange(nc)] = 12345.0                     # the diagonal is never read
        mats.append(d)
        offs.append(off)
        off += nc * nc
    blocks, want = [], []
    sizes = [(na, nb) for na in (1, 2, 3, 17, 70) for nb in (0, 1, 2, 64, 130)]
    for q in range(NB):
        na, nb = sizes[q % len(sizes)] if NB > 1 else (70, 130)
        c = 2 if na + nb > 40 else (1 if na + nb > 5 or q % 2 else 0)   # several blocks share one cell matrix
        nc = len(mats[c])
        a_lo = int(rs.randint(0, nc - na + 1))
        b_lo = int(rs.randint(0, nc - nb + 1))                         # (the classes may overlap: the kernel compares indices of a only)
        if c == 0:
            na, nb = min(na, nc), min(nb, nc)
            a_lo, b_lo = 0, nc - nb
        blocks.append((offs[c], nc, a_lo, a_lo + na, b_lo, b_lo + nb))
        want.append(O.triple_counts_fast(mats[c], np.arange(a_lo, a_lo + na), np.arange(b_lo, b_lo + nb)))
    assert O.triple_counts(mats[0], [0, 1, 2], [3, 4]) == O.triple_counts_fast(mats[0], [0, 1, 2], [3, 4])
    dmat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(DEV)
    got = ops.abx_count(dmat, torch.from_numpy(np.asarray(blocks, np.int64)).to(DEV)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, np.asarray(want, np.int64))
    assert NB == 1 or ((got[:, 1] > 0).sum() > 50 and (got[:, 2] > 0).sum() > 50 and (got[:, 3] == 0).sum() >= 60)
    # ranges are clamped into [0, n_c]; a matrix outside dmat reads nothing
    odd = np.asarray([(offs[0], 5, -3, 9, 3, 99), (off - 10, 200, 0, 2, 2, 3), (-1, 5, 0, 2, 2, 3)], np.int64)
    got = ops.abx_count(dmat, torch.from_numpy(odd).to(DEV)).cpu().numpy()
    assert got[0].tolist() == list(O.triple_counts(mats[0], range(5), [3, 4])) and (got[1:] == -1).all()


# ---------------------------------------------------------------- 6. metrics.abx
def _abx_both(items, label, cell, metric, dtype, **kw):
    """metrics.abx on the device and the brute-force oracle with distances in `dtype` -> (device result, {(cell, a, b): device counts},
    oracle blocks, oracle table, oracle score)"""
    from semi_tts_amd.metrics import abx
    feat, starts, lens = _pack(items)
    res = abx(feat, starts, lens, label, cell, metric, **kw)
    dist = lambda p, q: float(O.pair(items[p], items[q], metric, dtype)[0])       # noqa: E731
    blocks, table, score = O.abx(dist, label, cell, items=res.keep)
    got = {(int(c), int(a), int(b)): tuple(int(v) for v in row) for c, a, b, row in zip(res.block_cell, res.block_a, res.block_b, res.counts)}
    return res, got, blocks, table, score


def _integer_items(rs, n_items):
    return [rs.randint(-8, 9, (rs.randint(1, 9), 1)).astype(np.float32) * np.array([1, 2, 2], np.float32) for _ in range(n_items)]


def test_abx_integer_items_equal_the_oracle():
    rs = np.random.RandomState(21)
    label = np.array([0] * 4 + [1] * 3 + [2] * 1 + [0] * 2 + [1] * 5 + [2] * 2 + [1] * 3)
    cell = np.array([7] * 8 + [3] * 9 + [5] * 3)                          # cell 5 has one label: no block, no distance
    perm = rs.permutation(len(label))
    label, cell = label[perm], cell[perm]
    res, got, blocks, table, score = _abx_both(_integer_items(rs, len(label)), label, cell, 'euclid', np.float32)
    assert got == blocks and len(blocks) == 4 + 6 and res.pairs == 8 * 7 // 2 + 9 * 8 // 2
    assert {(a, b): (c, t) for a, b, c, t, _ in res.table} == {k: v[:2] for k, v in table.items()}
    assert all(abs(e - table[(a, b)][2]) <= 1e-15 for a, b, _, _, e in res.table) and abs(res.score - score) <= 1e-15
    assert sum(v[1] for v in blocks.values()) > 0                           # ties occur


def test_abx_of_two_well_separated_labels_is_zero():
    rs = np.random.RandomState(22)
    label = np.array([0, 1] * 6)
    items = [(np.eye(8, dtype=np.float32)[lab] * 5 + 0.1 * rs.randn(rs.randint(2, 9), 8)).astype(np.float32) for lab in label]
    res, got, blocks, table, score = _abx_both(items, label, np.zeros(12, int), 'angular', np.float64)
    assert res.score == 0.0 and score == 0.0 and got == blocks and [r[:4] for r in res.table] == [(0, 1, 1, 180), (1, 0, 1, 180)]


ABX_F64_SEED = 31


def test_abx_of_overlapping_labels_differs_from_float64_only_within_the_margin():
    """device (fp32) and float64 counts may differ only on the triples whose float64 margin |d(A, X) - d(B, X)| is below
    2 eps max(d(A, X), d(B, X)); ABX_F64_SEED was chosen on the CPU so that fewer than 1 % of the triples are that close"""
    rs = np.random.RandomState(ABX_F64_SEED)
    label = np.repeat(np.arange(3), 6)
    D = 8
    items = [(0.6 * np.eye(D)[lab] + rs.randn(rs.randint(3, 9), D)).astype(np.float32) for lab in label]
    res, got, blocks, table, score = _abx_both(items, label, np.zeros(len(label), int), 'angular', np.float64)
    e = O.eps(8, 8, D, 'angular')
    dm = np.zeros((18, 18))
    for i in range(18):
        for j in range(i + 1, 18):
            dm[i, j] = dm[j, i] = float(O.pair(items[i], items[j], 'angular', np.float64)[0])
    total = close_total = 0
    for (c, a, b), want in blocks.items():
        ia, ib = np.nonzero(label == a)[0], np.nonzero(label == b)[0]
        close = sum(1 for x in ia for A in ia if A != x for B in ib if abs(dm[A, x] - dm[B, x]) < 2 * e * max(dm[A, x], dm[B, x]))
        dev = got[(c, a, b)]
        print('block', (a, b), 'device', dev, 'float64', want, 'within the margin', close)
        assert dev[3] == want[3] == 180 and dev[2] == want[2] == 0
        assert abs(dev[0] - want[0]) <= close and abs(dev[1] - want[1]) <= close
        total, close_total = total + want[3], close_total + close
    assert total == 6 * 180 and close_total < 0.01 * total
    assert 0.05 < score < 0.5 and abs(res.score - score) <= 1.5 * close_total / 180.0 / 6 + 1e-12


def test_abx_subsampling_equals_the_oracle_on_the_same_subsample():
    rs = np.random.RandomState(23)
    label = np.array([0] * 7 + [1] * 5 + [2] * 2 + [0] * 6 + [1] * 1)
    cell = np.array([0] * 14 + [1] * 7)
    items = _integer_items(rs, len(label))
    res, got, blocks, table, score = _abx_both(items, label, cell, 'euclid', np.float32, max_items=3, seed=5)
    assert got == blocks and abs(res.score - score) <= 1e-15
    kept = sorted(zip(cell[res.keep].tolist(), label[res.keep].tolist()))
    assert [kept.count(k) for k in sorted(set(kept))] == [3, 3, 2, 3, 1] and len(set(res.keep.tolist())) == 12
    again = _abx_both(items, label, cell, 'euclid', np.float32, max_items=3, seed=5)[0]
    other = _abx_both(items, label, cell, 'euclid', np.float32, max_items=3, seed=6)[0]
    assert np.array_equal(again.keep, res.keep) and np.array_equal(again.counts, res.counts) and not np.array_equal(other.keep, res.keep)


# ---------------------------------------------------------------- 7. the command line
SR = 22050
ALI = {     # symbol, start frame, end frame at frame_s = 0.05: 12 frames = 0.6 s
    'u1': [('sil', 0, 2), ('a', 2, 4), ('sil', 4, 6), ('b', 6, 9), ('sil', 9, 12)],
    'u2': [('sil', 1, 2), ('b', 2, 5), ('sil', 5, 7), ('a', 7, 9), ('sil', 9, 11)],
    'u3': [('sil', 0, 3), ('a', 3, 6), ('c', 6, 9), ('sil', 9, 12)],
    'u4': [('c', 0, 3), ('sil', 3, 5), ('b', 5, 8), ('a', 8, 12)],
}           # without sil: a x 4, b x 3, c x 2; only the context (sil, sil) holds two phones (a x 2, b x 2)


def _wave(L, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / SR
    f0 = 120 + 80 * rs.rand() + 40 * np.sin(2 * np.pi * 3 * t + rs.rand())
    ph = 2 * np.pi * np.cumsum(f0) / SR
    return (0.5 * sum(np.sin((h + 1) * ph + rs.rand()) / (h + 1) for h in range(5)) * (0.3 + 0.7 * rs.rand(L // 2205 + 1).repeat(2205)[:L])
            + 0.01 * rs.randn(L)).astype(np.float32)


@pytest.fixture()
def abx_dirs(tmp_path):
    from semi_tts_amd.audio import write_wav
    ali_dir, wav_dir = tmp_path / 'ali', tmp_path / 'wav'
    ali_dir.mkdir()
    wav_dir.mkdir()
    for k, (stem, toks) in enumerate(ALI.items()):
        write_wav(wav_dir / (stem + '.wav'), _wave(13230 + 441 * k, 60 + k), SR)
        (ali_dir / (stem + '.ali')).write_text('# score=-1.000000 frames=12 frame_s=0.050000\n' + ''.join(
            '%s\t%d\t%d\t%.6f\t%.6f\n' % (s, a, b, a * 0.05, b * 0.05) for s, a, b in toks))
    return ali_dir, wav_dir, tmp_path / 'log'


@pytest.mark.parametrize('context', ['triphone', 'none'])
def test_abx_ali_dir_mfcc_end_to_end(abx_dirs, context, capsys):
    import main
    from semi_tts_amd import abx as A
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.metrics import abx
    import yaml
    ali_dir, wav_dir, log = abx_dirs
    cfg = os.path.join(REPO, 'config', 'supervised.yaml')
    main.main(['--config', cfg, '--abx-ali-dir', str(ali_dir), '--abx-wav-dir', str(wav_dir), '--abx-context', context, '--abx-ignore', 'sil',
               '--logdir', str(log), '--name', context, '--batch-size', '3'])
    out = capsys.readouterr().out
    assert sorted(os.listdir(log / context)) == ['abx.csv', 'abx_phones.csv']
    # the same features, file by file, and the items by hand
    conv = load_audio_transform(**yaml.load(open(cfg), Loader=yaml.FullLoader)['data']['audio'])
    hop = conv.hop_length_mfcc
    parts, rows, stats, first = [], [], {}, 0
    for stem in sorted(ALI):
        x = conv.load(wav_dir / (stem + '.wav'))[0]
        n = 1 + len(x) // hop
        parts.append(conv.extract_mfcc_batch([x])[0, :n])
        its, st = A.utterance_items(A.read_ali(str(ali_dir / (stem + '.ali'))), hop / float(SR), n, ('sil',), 1)
        rows += [(s, first + r0, ln, A.cell_key('spk', p, q, context)) for s, r0, ln, p, q in its]
        for s, v in st.items():
            stats[s] = [u + w for u, w in zip(stats.get(s, [0, 0, 0, 0]), v)]
        first += n
    names = sorted({r[0] for r in rows})
    cells = sorted({r[3] for r in rows})
    assert names == ['a', 'b', 'c'] and len(rows) == 9 and len(cells) == (1 if context == 'none' else 6)
    res = abx(torch.cat(parts, 0).contiguous(), [r[1] for r in rows], [r[2] for r in rows], [names.index(r[0]) for r in rows],
              [cells.index(r[3]) for r in rows], 'angular', 50, 0)
    assert (log / context / 'abx.csv').read_text() == A.format_abx_csv(res.table, names)
    assert (log / context / 'abx_phones.csv').read_text() == A.format_phones_csv(stats) == 'phone,tokens,items,too_short,too_long\na,4,4,0,0\nb,3,3,0,0\nc,2,2,0,0\n'
    assert len(res.table) == (6 if context == 'none' else 2) and np.isfinite(res.score)
    assert '%.2f %% over %d phone pairs, %d triples, %d pairs of DTW' % (100 * res.score, len(res.table), sum(r[3] for r in res.table), res.pairs) in out


@pytest.mark.parametrize('feat', ['latent', 'code'])
def test_abx_ali_dir_model_representations_run_and_repeat(abx_dirs, feat):
    import main
    ali_dir, wav_dir, log = abx_dirs
    cfg = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')
    texts = []
    for name in ('one', 'two'):
        main.main(['--config', cfg, '--abx-ali-dir', str(ali_dir), '--abx-wav-dir', str(wav_dir), '--abx-feat', feat, '--abx-context', 'none',
                   '--logdir', str(log), '--name', name, '--no-msg'])
        texts.append(((log / name / 'abx.csv').read_text(), (log / name / 'abx_phones.csv').read_text()))
    assert texts[0] == texts[1]
    rows = texts[0][0].splitlines()
    assert rows[0] == 'phone_a,phone_b,cells,triples,error' and len(rows) == 1 + 12         # a, b, c and sil, every ordered pair
    assert all(0.0 <= float(r.split(',')[4]) <= 1.0 for r in rows[1:])
