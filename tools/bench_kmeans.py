#!/usr/bin/env python3
"""k-means at the size of a small corpus of MFCC frames (st_kmeans_assign, st_kmeans_update, the k-means++ kernels; semi_tts_amd.kmeans):
N = 262144 rows x D = 39 columns drawn around 64 centres, at K = 50 and K = 512.  Before anything is timed the device's assignment is
held against the float64 oracle of tests/kmeans_oracle.py on a sample of the rows (the bound and the margin rule of
tests/test_gpu_kmeans.py) and its update against the oracle's float64 means of the device's own assignment.  Device time from events
around windows of back-to-back calls of at least 200 ms each after warm-up, median of the windows: one assign, one update, one Lloyd iteration (assign + update,
no host read), the same iteration written in torch on the same GPU (torch.cdist(x, c).argmin(1) + index_add_ + divide) alternating with
it in one process, and the k-means++ seeding of K centres (host clock around the 2 K launches, ended by its flag read).  Beside them the
fp32 FMA floor of the assign -- 2 N K D flop at 155 TFLOP/s, the fp32 rate MI355X_MICROARCH measured -- and one iteration of the oracle's
arithmetic in float64 numpy on 16 CPU processes (forked before the GPU is opened).  Prints one JSON line per K and writes them to
profiles/bench_kmeans.json (--out).

    python tools/bench_kmeans.py [--window-ms 200] [--windows 5] [--out FILE]
    python tools/bench_kmeans.py --cpu-only      # the numpy timing alone (needs no GPU; the device fields read "not measured")
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

N, D, KS, CENTRES, CPU_PROCS, SAMPLE = 262144, 39, (50, 512), 64, 16, 4096
FP32_PEAK = 155e12          # FLOP/s, measured (MI355X_MICROARCH, "Peak FP32 (matrix)": the fp32 MFMA runs at the vector FMA rate)
X = None                    # the rows, made before the pool is forked: the workers inherit them


def inputs(seed=0):
    rs = np.random.RandomState(seed)
    centres = 3.0 * rs.randn(CENTRES, D)
    return (centres[rs.randint(0, CENTRES, N)] + rs.randn(N, D)).astype(np.float32)


def _chunk(args):
    """rows [lo, hi) of one float64 iteration: nearest centroid by the expanded form on BLAS, then the sums and counts of the clusters"""
    lo, hi, c = args
    x = X[lo:hi].astype(np.float64)
    d = (x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :]
    idx = d.argmin(1)
    order = np.argsort(idx, kind='stable')
    count = np.bincount(idx, minlength=c.shape[0])
    sums = np.zeros_like(c)
    keep = np.nonzero(count)[0]
    sums[keep] = np.add.reduceat(x[order], np.concatenate([[0], np.cumsum(count[keep])[:-1]]), axis=0)
    return sums, count, float(d[np.arange(hi - lo), idx].sum())


def cpu_ms(pool, c, procs, repeats=3):
    c = c.astype(np.float64)
    edges = np.linspace(0, N, 4 * procs + 1).astype(int)
    jobs = [(int(a), int(b), c) for a, b in zip(edges[:-1], edges[1:])]
    pool.map(_chunk, jobs[:procs])
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = pool.map(_chunk, jobs, chunksize=1)
        count = sum(r[1] for r in res)
        _ = sum(r[0] for r in res) / np.maximum(count, 1)[:, None]
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def check_steps(x, xd, cd, K):
    """the step checks of tests/test_gpu_kmeans.py on this input: the assignment on SAMPLE rows, the update on all -> what was checked"""
    import torch
    import kmeans_oracle as O
    from semi_tts_amd import ops
    idx, dist = ops.kmeans_assign(xd, cd)
    out, count, stats = ops.kmeans_update(xd, idx, dist, cd)
    c = cd.cpu().numpy()
    rows = np.random.RandomState(1).choice(N, SAMPLE, replace=False)
    xs, ids, ds = x[rows], idx.cpu().numpy()[rows], dist.cpu().numpy()[rows].astype(np.float64)
    d64 = O.sqdist(xs, c)
    x64 = xs.astype(np.float64)
    eps = (D + 3) * 2.0 ** -24 * (np.sqrt((x64 * x64).sum(1)) + np.sqrt((c.astype(np.float64) ** 2).sum(1)).max()) ** 2
    part = np.partition(d64, 1, axis=1)
    clear = part[:, 1] - part[:, 0] > 2 * eps
    own = d64[np.arange(SAMPLE), ids]
    ok = (np.abs(ds - own) <= eps).all() and (own - d64.min(1) <= 2 * eps).all() and np.array_equal(ids[clear], d64.argmin(1)[clear])
    ids_all = idx.cpu().numpy()
    _, cnt, _, c64 = O.update(x, ids_all, dist.cpu().numpy(), c)
    mass = np.zeros_like(c64)
    np.add.at(mass, ids_all, np.abs(x.astype(np.float64)))
    got = out.cpu().numpy().astype(np.float64)
    ok_update = np.array_equal(cnt, count.cpu().numpy()) and (np.abs(got - c64)[cnt > 0] <= (2.0 ** -24 * np.abs(c64) + 2.0 ** -52 * mass)[cnt > 0]).all()
    out2, _, stats2 = ops.kmeans_update(xd, idx, dist, cd)
    same = torch.equal(out, out2) and torch.equal(stats.view(torch.int64), stats2.view(torch.int64))
    if not (ok and ok_update and same):
        raise SystemExit('bench_kmeans: K = %d: the step checks fail (assign %s, update %s, repeatable %s): nothing is timed' % (K, ok, ok_update, same))
    return dict(assign_rows=SAMPLE, rows_within_2eps_of_a_tie=int((~clear).sum()), update_rows=N, update_bitwise_repeatable=True)


def main(argv=None):
    global X
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=8, help='calls of the first window, from which the timed windows are sized')
    ap.add_argument('--window-ms', type=float, default=200.0, help='the least length of a timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_kmeans.json'))
    a = ap.parse_args(argv)
    X = x = inputs()
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    pool = multiprocessing.get_context('fork').Pool(procs)        # (before the GPU is opened: the workers never see it)
    lines = []
    try:
        for K in KS:
            res = {'shape': dict(N=N, D=D, K=K, centres=CENTRES), 'numpy_processes': procs,
                   'assign_fma_floor_us': round(2.0 * N * K * D / FP32_PEAK * 1e6, 2)}
            for f in ('assign_us', 'update_us', 'lloyd_iteration_us', 'torch_iteration_us', 'torch_over_lloyd', 'seeding_ms', 'numpy_over_lloyd',
                      'checked_before_timing'):
                res[f] = 'not measured'
            c0 = x[np.random.RandomState(2).choice(N, K, replace=False)]
            res['numpy_float64_ms_per_iteration'] = round(cpu_ms(pool, c0, procs), 2)
            if not a.cpu_only:
                import torch
                if not torch.cuda.is_available():
                    raise SystemExit('bench_kmeans: no GPU (--cpu-only times the numpy form alone)')
                from semi_tts_amd import ops
                dev = torch.device('cuda:0')
                xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(c0).to(dev)
                res['checked_before_timing'] = check_steps(x, xd, cd, K)
                idx, dist = ops.kmeans_assign(xd, cd)

                def lloyd():
                    i, d = ops.kmeans_assign(xd, cd)
                    return ops.kmeans_update(xd, i, d, cd)

                def torch_form():
                    i = torch.cdist(xd, cd).argmin(1)
                    sums = torch.zeros(K, D, device=dev).index_add_(0, i, xd)
                    return sums / torch.bincount(i, minlength=K).clamp(min=1).unsqueeze(1)

                def window(fn, calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    e1.synchronize()
                    return round(e0.elapsed_time(e1) / calls * 1e3, 2)

                def stat(out):
                    return dict(median_us=round(float(np.median(out)), 2), min_us=min(out), max_us=max(out), windows=out)
                fns = dict(assign_us=lambda: ops.kmeans_assign(xd, cd), update_us=lambda: ops.kmeans_update(xd, idx, dist, cd),
                           lloyd_iteration_us=lloyd, torch_iteration_us=torch_form)
                for fn in fns.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                # a window lasts about --window-ms: its calls are sized from a first window of --calls (a window of a millisecond would
                # measure the clock and the scheduler)
                calls = {k: max(a.calls, int(np.ceil(a.window_ms * 1e3 / max(window(fn, a.calls), 1.0)))) for k, fn in fns.items()}
                outs = {k: [] for k in fns}
                for _ in range(a.windows):                      # (the forms alternate inside one process: each window sees the same machine)
                    for k, fn in fns.items():
                        outs[k].append(window(fn, calls[k]))
                for k in fns:
                    res[k] = stat(outs[k])
                res['calls_per_window'] = calls
                res['timed_calls_include'] = 'the allocation of the outputs and of the update workspace (torch.empty from the caching allocator) on every call'
                res['torch_over_lloyd'] = round(res['torch_iteration_us']['median_us'] / res['lloyd_iteration_us']['median_us'], 2)
                res['assign_share_of_fma_floor'] = round(res['assign_fma_floor_us'] / res['assign_us']['median_us'], 3)
                res['numpy_over_lloyd'] = round(res['numpy_float64_ms_per_iteration'] * 1e3 / res['lloyd_iteration_us']['median_us'], 1)
                u = np.random.default_rng(0).random(K)
                ops.kmeans_pp_init(xd, K, u)
                times = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ops.kmeans_pp_init(xd, K, u)
                    times.append(round((time.perf_counter() - t0) * 1e3, 3))
                res['seeding_ms'] = dict(median_ms=float(np.median(times)), runs=times, launches=2 * K)
                res['device'] = torch.cuda.get_device_name(0)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    finally:
        pool.close()
        pool.join()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return lines


if __name__ == '__main__':
    main()
