#!/usr/bin/env python3
"""DTW of a corpus-like batch (st_dtw_batch, semi_tts_amd.metrics.dtw): 32 pairs of about 300 x 330 frames -- 3 s at the 10 ms hop of
the MFCC, the second side a tenth longer -- over the 12 columns [1, 13) of 39-wide rows, what metrics.mcd compares.  Device time per
batch from events around windows of back-to-back calls (with and without the path), beside the vectorised anti-diagonal numpy form of
the tests (tests/dtw_oracle.py, float32) over the same 32 pairs on up to 16 CPU processes, and the barriers a pair costs (one per
anti-diagonal plus four).  The device results are compared with the numpy ones before anything is timed.  Prints one JSON line and
writes it to profiles/bench_dtw.json (--out).

    python tools/bench_dtw.py [--calls 200] [--windows 5] [--out FILE]
    python tools/bench_dtw.py --cpu-only          # the numpy timing alone (needs no GPU; the device fields read "not measured")
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

B, WIDTH, COLS, SCALE = 32, 39, (1, 13), 1.0
CPU_PROCS = 16
FIXED_BARRIERS = 4          # set-up, staging, end of the sweep, trace-back -> path


def inputs(seed=0):
    """x (B, 300, 39), y (B, 330, 39) float32 and the lengths: 270 .. 300 frames against 1.1 times as many; y is x resampled along time
    plus noise, so the optimal path wanders about the diagonal as a real warp does"""
    rs = np.random.RandomState(seed)
    xl = rs.randint(270, 301, B)
    xl[0] = 300
    yl = np.round(1.1 * xl).astype(np.int64)
    x, y = np.zeros((B, 300, WIDTH), np.float32), np.zeros((B, 330, WIDTH), np.float32)
    for b in range(B):
        s = np.cumsum(rs.randn(xl[b], WIDTH), axis=0).astype(np.float32) * 0.1
        x[b, :xl[b]] = s
        t = np.linspace(0, xl[b] - 1, yl[b])
        y[b, :yl[b]] = np.stack([np.interp(t, np.arange(xl[b]), s[:, k]) for k in range(WIDTH)], 1) + 0.05 * rs.randn(yl[b], WIDTH)
    return x, y, xl.astype(np.int32), yl.astype(np.int32)


def _one(args):
    import dtw_oracle as O
    x, y = args
    total, path = O.dtw(x, y, SCALE, np.float32)
    return float(total), len(path)


def cpu_ms(x, y, xl, yl, repeats=3):
    """wall time of the numpy form over the B pairs on CPU_PROCS processes (the pool is up before the clock starts) -> (ms, results)"""
    jobs = [(x[b, :xl[b], COLS[0]:COLS[1]], y[b, :yl[b], COLS[0]:COLS[1]]) for b in range(B)]
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, jobs)
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, jobs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_dtw.json'))
    a = ap.parse_args(argv)
    x, y, xl, yl = inputs()
    ms, procs, cpu = cpu_ms(x, y, xl, yl)             # (before the GPU is opened: the workers are forked from a process without one)
    res = {'shape': dict(B=B, x_frames=[int(xl.min()), int(xl.max())], y_frames=[int(yl.min()), int(yl.max())], columns=COLS[1] - COLS[0],
                         row_width=WIDTH),
           'barriers_per_pair_mean': round(float(np.mean(xl + yl - 1)) + FIXED_BARRIERS, 1),
           'numpy_float32_ms_per_batch': round(ms, 1), 'numpy_processes': procs,
           'device_us_per_batch': 'not measured', 'device_us_per_batch_no_path': 'not measured', 'numpy_over_device': 'not measured'}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_dtw: no GPU (--cpu-only times the numpy form alone)')
        from semi_tts_amd.metrics import dtw
        dev = torch.device('cuda:0')
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        xld, yld = torch.from_numpy(xl).to(dev), torch.from_numpy(yl).to(dev)
        total, plen, _ = dtw(xd, yd, xld, yld, cols=COLS, scale=SCALE)
        total, plen = total.cpu().numpy(), plen.cpu().numpy()
        rel = max(abs(total[b] - cpu[b][0]) / cpu[b][0] for b in range(B))
        if rel > 1e-4:
            raise SystemExit('bench_dtw: the device total differs from the numpy one by %.2e' % rel)
        res['max_rel_difference_from_numpy'] = float('%.2e' % rel)
        res['path_len_equal'] = int(sum(int(plen[b]) == cpu[b][1] for b in range(B)))

        def windows(fn):
            for _ in range(20):
                fn()
            out = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                out.append(round(e0.elapsed_time(e1) / a.calls * 1e3, 2))
            return dict(median_us=round(float(np.median(out)), 2), min_us=min(out), max_us=max(out), windows=out)
        res['calls_per_window'] = a.calls
        res['device_us_per_batch'] = windows(lambda: dtw(xd, yd, xld, yld, cols=COLS, scale=SCALE))
        res['device_us_per_batch_no_path'] = windows(lambda: dtw(xd, yd, xld, yld, cols=COLS, scale=SCALE, want_path=False))
        res['numpy_over_device'] = round(ms * 1e3 / res['device_us_per_batch']['median_us'], 1)
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
