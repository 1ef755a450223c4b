#!/usr/bin/env python3
"""The ABX distance engine at a ZeroSpeech-like cell (st_dtw_pairs, st_abx_count; semi_tts_amd.metrics.dtw_pairs / abx): 2000 items
(40 labels x 50) of 5 .. 25 frames x 39 columns in one cell, all 1 999 000 unordered pairs in one launch, `angular`; then the triple
counts of its 1560 ordered label pairs (50 x 49 x 50 triples each).  Device time from events around windows of back-to-back calls after
warm-up, median of 5 windows, random data.  Beside it, per pair and on a 2048-pair sample of the same pairs: the existing
workgroup-per-pair kernel (metrics.dtw, batches of 64, want_path=False; Euclidean -- it has no other distance) and the float64 numpy
oracle of the tests on up to 16 CPU processes.  The device distances of the sample are compared with the oracle's before anything is
timed.  Bytes: what the distance phase requests per pair (both rows of every cell, 2 n m D floats, plus the n + m rows of the norms)
against the L2 rate, and the rows a pair needs once ((n + m) D floats); the vector instructions of both phases, counted from the
loops, against the issue rate -- the larger share says which resource bounds the kernel.  Prints one JSON line and writes it to
profiles/bench_abx.json (--out).

    python tools/bench_abx.py [--calls 4] [--windows 5] [--out FILE]
    python tools/bench_abx.py --cpu-only          # the numpy timing alone (needs no GPU; the device fields read "not measured")
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np   # noqa: E402

LABELS, PER_LABEL, D, LEN_LO, LEN_HI, SAMPLE, CPU_PROCS = 40, 50, 39, 5, 25, 2048, 16
L2_TBS = 17.0               # rows shared by every workgroup of an XCD, chip-wide (MI355X: 16.8 - 18.8 TB/s measured)
CUS, SIMDS, CLOCK_GHZ, ISSUE_CYCLES = 256, 4, 2.4, 2        # a wave64 vector instruction occupies its SIMD-32 for 2 cycles


def inputs(seed=0):
    """items around one direction per label (so the distances are not all alike), packed -> (feat, starts, lens, label)"""
    rs = np.random.RandomState(seed)
    label = np.repeat(np.arange(LABELS), PER_LABEL)
    lens = rs.randint(LEN_LO, LEN_HI + 1, len(label)).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    centre = rs.randn(LABELS, D)
    feat = (centre[np.repeat(label, lens)] + rs.randn(int(lens.sum()), D)).astype(np.float32)
    return feat, starts, lens, label


def _one(args):
    import abx_oracle as O
    x, y = args
    return float(O.pair(x, y, 'angular', np.float64)[0])


def cpu_ms(jobs, repeats=3):
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, jobs[:64])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, jobs, chunksize=16)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, np.asarray(res)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=4, help='launches per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_abx.json'))
    a = ap.parse_args(argv)
    from semi_tts_amd import abx as A
    feat, starts, lens, label = inputs()
    pl = A.plan(label, np.zeros(len(label), np.int64), max_items=PER_LABEL, seed=0)
    P = len(pl.pair_a)
    n, m = lens[pl.pair_a].astype(np.int64), lens[pl.pair_b].astype(np.int64)
    sample = np.random.RandomState(1).choice(P, SAMPLE, replace=False)
    jobs = [(feat[starts[p]:starts[p] + lens[p]], feat[starts[q]:starts[q] + lens[q]]) for p, q in zip(pl.pair_a[sample], pl.pair_b[sample])]
    ms, procs, want = cpu_ms(jobs)                      # (before the GPU is opened: the workers are forked from a process without one)
    req = float(np.mean(2 * n * m * D + (n + m) * D) * 4)
    uniq = float(np.mean((n + m) * D) * 4)
    # vector instructions a wave issues for a pair, from the loops of abx.hip: per 64 cells D x (2 mul, 2 add / sub, 2 fma) + ~60 of
    # address, root and atan2f; per row of the norms D fma over 64 rows a pass; ~16 per anti-diagonal of the sweep
    valu = float(np.mean(np.ceil(n * m / 64.0) * (6 * D + 60) + np.ceil((n + m) / 64.0) * (D + 20) + (n + m - 1) * 16))
    res = {'shape': dict(items=len(label), labels=LABELS, frames=[LEN_LO, LEN_HI], columns=D, pairs=P, blocks=len(pl.blocks),
                         triples_per_block=PER_LABEL * (PER_LABEL - 1) * PER_LABEL, metric='angular', sample=SAMPLE),
           'numpy_float64_us_per_pair': round(ms * 1e3 / SAMPLE, 2), 'numpy_processes': procs,
           'bytes_requested_per_pair': round(req), 'bytes_needed_once_per_pair': round(uniq), 'vector_instructions_per_pair': round(valu),
           'dtw_pairs_us_per_launch': 'not measured', 'dtw_pairs_ns_per_pair': 'not measured', 'abx_count_us_per_launch': 'not measured',
           'dtw_batch_ns_per_pair': 'not measured', 'dtw_batch_over_dtw_pairs': 'not measured', 'numpy_over_dtw_pairs': 'not measured'}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_abx: no GPU (--cpu-only times the numpy form alone)')
        from semi_tts_amd import ops
        from semi_tts_amd.metrics import dtw
        dev = torch.device('cuda:0')
        t = lambda v, dt=np.int32: torch.from_numpy(np.ascontiguousarray(v, dt)).to(dev)       # noqa: E731
        fd, sd, ld, pa, pb = t(feat, np.float32), t(starts), t(lens), t(pl.pair_a), t(pl.pair_b)
        max_len = int(lens.max())
        dist = ops.dtw_pairs(fd, sd, ld, pa, pb, 'angular', max_len)
        got = dist[t(sample, np.int64)].cpu().numpy().astype(np.float64)
        rel = float(np.max(np.abs(got - want) / want))
        if not rel < 1e-4:
            raise SystemExit('bench_abx: the device distances differ from the float64 ones by %.2e' % rel)
        res['max_rel_difference_from_float64'] = float('%.2e' % rel)
        dmat = torch.zeros(pl.dmat_len, device=dev)
        dmat[t(np.concatenate([pl.pos_ab, pl.pos_ba]), np.int64)] = torch.cat([dist, dist])
        blk = t(pl.blocks, np.int64)
        counts = ops.abx_count(dmat, blk).cpu().numpy()
        res['abx_error_percent'] = round(100 * A.aggregate(pl.block_a, pl.block_b, counts).score, 3)
        # the sample through the workgroup-per-pair kernel: batches of 64, rows padded to the longest item
        xs = np.zeros((SAMPLE, LEN_HI, D), np.float32)
        ys = np.zeros((SAMPLE, LEN_HI, D), np.float32)
        for k, (x, y) in enumerate(jobs):
            xs[k, :len(x)], ys[k, :len(y)] = x, y
        xd, yd = t(xs, np.float32), t(ys, np.float32)
        xl, yl = t(lens[pl.pair_a[sample]]), t(lens[pl.pair_b[sample]])

        def old():
            for b in range(0, SAMPLE, 64):
                dtw(xd[b:b + 64], yd[b:b + 64], xl[b:b + 64], yl[b:b + 64], want_path=False)

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
        res['calls_per_window'] = a.calls
        w = res['dtw_pairs_us_per_launch'] = windows(lambda: ops.dtw_pairs(fd, sd, ld, pa, pb, 'angular', max_len), a.calls)
        res['dtw_pairs_us_per_launch_max_len_64'] = windows(lambda: ops.dtw_pairs(fd, sd, ld, pa, pb, 'angular', 64), a.calls)
        res['dtw_pairs_euclid_us_per_launch'] = windows(lambda: ops.dtw_pairs(fd, sd, ld, pa, pb, 'euclid', max_len), a.calls)
        res['abx_count_us_per_launch'] = windows(lambda: ops.abx_count(dmat, blk), a.calls)
        o = res['dtw_batch_us_per_sample'] = windows(old, a.calls)
        ns = w['median_us'] * 1e3 / P
        res['dtw_pairs_ns_per_pair'] = round(ns, 2)
        res['dtw_pairs_euclid_ns_per_pair'] = round(res['dtw_pairs_euclid_us_per_launch']['median_us'] * 1e3 / P, 2)
        res['dtw_batch_ns_per_pair'] = round(o['median_us'] * 1e3 / SAMPLE, 1)
        res['dtw_batch_over_dtw_pairs'] = round(res['dtw_batch_ns_per_pair'] / res['dtw_pairs_euclid_ns_per_pair'], 1)
        res['dtw_batch_euclid_over_dtw_pairs_angular'] = round(res['dtw_batch_ns_per_pair'] / ns, 1)
        res['numpy_over_dtw_pairs'] = round(ms * 1e6 / SAMPLE / ns, 1)
        res['share_of_l2_rate'] = round(req / ns / (L2_TBS * 1e3), 3)                      # bytes per ns over TB/s x 1000
        res['share_of_vector_issue'] = round(valu * ISSUE_CYCLES / (ns * CLOCK_GHZ * CUS * SIMDS), 3)
        res['bound_by'] = 'vector issue' if res['share_of_vector_issue'] > res['share_of_l2_rate'] else 'L2 / L1 reads'
        res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
