#!/usr/bin/env python3
"""Across-speaker ABX at a Libri-light-like context (st_dtw_pairs for the cross-speaker pairs, st_abx_across; semi_tts_amd.metrics
.abx_across): 8 speakers x 40 labels x 6 items of 5 .. 25 frames x 39 columns in ONE context, `angular` -- 1920 items, every
cross-speaker pair in one launch, then the 8 x 40 x 39 groups (speaker, a, b), each against the 7 other speakers' tokens of a.
Before anything is timed the device's counts and group errors are compared with a float64 numpy oracle working on the device's own
distances: counts equal, errors bit for bit.  Device time from events around windows of back-to-back launches after warm-up, median of
the windows, random data.  Beside it the same oracle on up to 16 CPU processes (forked before the GPU is opened; they read the matrix
from a file), wall time of all groups.  Prints one JSON line and writes it to profiles/bench_abx_across.json (--out).

    python tools/bench_abx_across.py [--calls 4] [--windows 5] [--out FILE]
    python tools/bench_abx_across.py --cpu-only      # the numpy timing alone on a random matrix (needs no GPU; the device fields read "not measured")
"""
import argparse
import json
import multiprocessing
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

SPEAKERS, LABELS, PER_RUN, D, LEN_LO, LEN_HI, CPU_PROCS = 8, 40, 6, 39, 5, 25, 16


def inputs(seed=0):
    """items around one direction per label and a smaller shift per speaker, packed -> (feat, starts, lens, label, speaker)"""
    rs = np.random.RandomState(seed)
    speaker = np.repeat(np.arange(SPEAKERS), LABELS * PER_RUN)
    label = np.tile(np.repeat(np.arange(LABELS), PER_RUN), SPEAKERS)
    lens = rs.randint(LEN_LO, LEN_HI + 1, len(label)).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    centre, shift = rs.randn(LABELS, D), 0.5 * rs.randn(SPEAKERS, D)
    rows = np.repeat(np.arange(len(label)), lens)
    feat = (centre[label[rows]] + shift[speaker[rows]] + rs.randn(int(lens.sum()), D)).astype(np.float32)
    return feat, starts, lens, label, speaker


def group_numpy(dm, row, xr):
    """one group in float64 numpy: the measure of include/semitts.h, vectorised over the triples of an X range"""
    off, nc, a_lo, a_hi, b_lo, b_hi, x0, x1 = row
    tot, s, present = np.zeros(4, np.int64), np.float64(0.0), 0
    for x_lo, x_hi in xr[x0:x1]:
        if (x_lo, x_hi) == (a_lo, a_hi):
            continue
        ax = dm[off:off + nc * nc].reshape(nc, nc)[x_lo:x_hi, a_lo:a_hi].astype(np.float64)[:, :, None]
        bx = dm[off:off + nc * nc].reshape(nc, nc)[x_lo:x_hi, b_lo:b_hi].astype(np.float64)[:, None, :]
        nan = np.isnan(ax) | np.isnan(bx)
        with np.errstate(invalid='ignore'):
            c = np.array([((ax > bx) & ~nan).sum(), ((ax == bx) & ~nan).sum(), nan.sum(), nan.size], np.int64)
        tot += c
        if c[3] - c[2] > 0:
            s = s + (np.float64(c[0]) + 0.5 * np.float64(c[1])) / np.float64(c[3] - c[2])
            present += 1
    return (s / present if present else np.nan), tot.tolist() + [present]


def _chunk(args):
    path, grp, xr = args
    dm = np.load(path, mmap_mode='r')
    xr = [tuple(r) for r in xr.tolist()]
    out = [group_numpy(dm, row, xr) for row in grp.tolist()]
    return np.array([e for e, _ in out], np.float64), np.array([c for _, c in out], np.int64)


def cpu_ms(pool, path, grp, xr, repeats=3):
    jobs = [(path, g, xr) for g in np.array_split(grp, 16 * CPU_PROCS)]
    pool.map(_chunk, jobs[:CPU_PROCS])
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = pool.map(_chunk, jobs, chunksize=1)
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=4, help='launches per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_abx_across.json'))
    a = ap.parse_args(argv)
    from semi_tts_amd import abx as A
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    pool = multiprocessing.get_context('fork').Pool(procs)        # (before the GPU is opened: the workers never see it)
    feat, starts, lens, label, speaker = inputs()
    pl = A.plan_across(label, np.zeros(len(label), np.int64), speaker, max_items=PER_RUN, seed=0)
    P, NG = len(pl.pair_a), len(pl.grp)
    res = {'shape': dict(items=len(label), speakers=SPEAKERS, labels=LABELS, items_per_run=PER_RUN, frames=[LEN_LO, LEN_HI], columns=D, contexts=1,
                         metric='angular', cross_speaker_pairs=P, groups=NG, x_ranges_per_group=SPEAKERS, matrix_bytes=4 * pl.dmat_len),
           'numpy_processes': procs, 'dtw_pairs_us_per_launch': 'not measured', 'abx_across_us_per_launch': 'not measured',
           'numpy_over_abx_across': 'not measured', 'checked_before_timing': 'not measured'}
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'dmat.npy')
    try:
        if a.cpu_only:
            np.save(path, np.random.RandomState(1).rand(pl.dmat_len).astype(np.float32))
        else:
            import torch
            if not torch.cuda.is_available():
                raise SystemExit('bench_abx_across: no GPU (--cpu-only times the numpy form alone)')
            from semi_tts_amd import ops
            dev = torch.device('cuda:0')
            t = lambda v, dt=np.int32: torch.from_numpy(np.ascontiguousarray(v, dt)).to(dev)       # noqa: E731
            fd, sd, ld, pa, pb = t(feat, np.float32), t(starts), t(lens), t(pl.pair_a), t(pl.pair_b)
            max_len = int(lens.max())
            dist = ops.dtw_pairs(fd, sd, ld, pa, pb, 'angular', max_len)
            dmat = torch.full((pl.dmat_len,), float('nan'), device=dev)      # (NaN where nothing is stored: a read there would be counted)
            dmat[t(np.concatenate([pl.pos_ab, pl.pos_ba]), np.int64)] = torch.cat([dist, dist])
            grp, xr = t(pl.grp, np.int64), t(pl.xr, np.int64)
            err, cnt = ops.abx_across(dmat, grp, xr)
            err, cnt = err.cpu().numpy(), cnt.cpu().numpy()
            np.save(path, dmat.cpu().numpy())
        ms, want_err, want_cnt = cpu_ms(pool, path, pl.grp, pl.xr)
        res['numpy_float64_ms_all_groups'] = round(ms, 2)
        res['numpy_float64_us_per_group'] = round(ms * 1e3 / NG, 2)
        res['triples'] = int(want_cnt[:, 3].sum())
        if not a.cpu_only:
            if not (np.array_equal(cnt, want_cnt) and np.array_equal(err.view(np.uint64), want_err.view(np.uint64))):
                raise SystemExit('bench_abx_across: the device differs from the oracle in %d counts rows, %d errors'
                                 % (int((cnt != want_cnt).any(1).sum()), int((err.view(np.uint64) != want_err.view(np.uint64)).sum())))
            res['checked_before_timing'] = dict(counts_equal=True, errors_bitwise_equal=True, groups=NG, nan_counted=int(cnt[:, 2].sum()))
            agg = A.aggregate_across(pl.grp_a, pl.grp_b, pl.grp_speaker, err, cnt)
            res['abx_across_error_percent'] = round(100 * agg.score, 3)

            def windows(fn, calls):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                out = []
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    e1.synchronize()
                    out.append(round(e0.elapsed_time(e1) / calls * 1e3, 2))
                return dict(median_us=round(float(np.median(out)), 2), min_us=min(out), max_us=max(out), windows=out)
            res['calls_per_window'] = dict(dtw_pairs=a.calls, abx_across=8 * a.calls)
            w = res['dtw_pairs_us_per_launch'] = windows(lambda: ops.dtw_pairs(fd, sd, ld, pa, pb, 'angular', max_len), a.calls)
            x = res['abx_across_us_per_launch'] = windows(lambda: ops.abx_across(dmat, grp, xr), 8 * a.calls)
            one = t(pl.grp[:1], np.int64)
            res['abx_across_one_group_us_per_launch'] = windows(lambda: ops.abx_across(dmat, one, xr), 8 * a.calls)
            res['dtw_pairs_ns_per_pair'] = round(w['median_us'] * 1e3 / P, 2)
            res['abx_across_ns_per_group'] = round(x['median_us'] * 1e3 / NG, 2)
            res['abx_across_ns_per_triple'] = round(x['median_us'] * 1e3 / res['triples'], 4)
            # what a launch reads: a group's row, its list twice, and per foreign range n_x (n_a + n_b) distances
            res['bytes_read_per_launch'] = int(NG * (64 + 2 * 16 * SPEAKERS + (SPEAKERS - 1) * PER_RUN * 2 * PER_RUN * 4))
            res['gbytes_per_s'] = round(res['bytes_read_per_launch'] / x['median_us'] / 1e3, 1)
            res['numpy_over_abx_across'] = round(ms * 1e3 / x['median_us'], 1)
            res['device'] = torch.cuda.get_device_name(0)
    finally:
        pool.close()
        pool.join()
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
