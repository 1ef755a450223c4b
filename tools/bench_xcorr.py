#!/usr/bin/env python3
"""What the alignment of waveform pairs costs (st_xcorr_delay, st_sisdr_batch, semi_tts_amd.metrics.align_pairs).

  Workload  B = 32 pairs of 2.5 .. 3.5 s at 22050 Hz: an AR(1) sequence (coefficient 0.9) under a syllable envelope, rounded to 16-bit
            PCM, against the same signal shifted by a planted delay within +-40 ms in white noise at 20 dB SNR; the search bound is
            +-50 ms = 1102 lags each way.
  Timed     device time from windows of back-to-back calls between two synchronises (median of --windows): `xcorr` ops.xcorr_delay on
            the packed buffers (both launches and the workspace allocation), `sisdr` ops.sisdr_batch with the device delays,
            `align_stoi` metrics.align_pairs + metrics.stoi on the cut batches (one host read of the delays inside), `stoi` metrics.stoi
            alone on the same pairs, `conv1d_fp32` torch.nn.functional.conv1d (groups = B, the pairs zero-padded to one length) for the
            same lags in float32 on the same GPU (--conv-only, a run of its own: its first call builds a solver).
  Kernels   the two launches of st_xcorr_delay apart come from a kernel trace: run `--trace-only` under rocprofv3 --kernel-trace --stats
            and pass the *kernel_stats.csv it wrote with --kernel-stats.
  Beside    the float64 numpy oracle (one numpy.dot per lag) on up to 16 CPU processes, and the fp64 FMA floor: the multiply-adds the
            definition needs (the sum over pairs and lags of the overlap) over 78.6 TFLOP/s, AMD's PUBLISHED fp64 vector peak of the
            MI355X -- the spec sheet's figure, not a measurement.
  Checked   before anything is timed: every delay is the planted one, and corr equals the float64 oracle BIT FOR BIT (PCM input: every
            sum is exact in float64 in any order).

Prints one JSON line and writes it to profiles/bench_xcorr.json (--out).

    python tools/bench_xcorr.py [--calls 50] [--windows 5] [--kernel-stats CSV] [--conv-json FILE] [--out FILE]
    python tools/bench_xcorr.py --trace-only           # 20 calls of the kernels and nothing else (for a kernel trace)
    python tools/bench_xcorr.py --conv-only --out F    # the conv1d timing alone -> F (merged by --conv-json F)
    python tools/bench_xcorr.py --merge F --conv-json G --out H      # add a --conv-only result to an earlier result (no GPU)
    python tools/bench_xcorr.py --cpu-only             # the numpy timing alone (needs no GPU; the device fields read "not measured")
"""
import argparse
import csv
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):     # one BLAS thread a process: the oracle runs on CPU_PROCS processes,
    os.environ[_v] = '1'                                                      # and a pool of threads inside each only makes them fight
import numpy as np   # noqa: E402

B, SR, MAX_DELAY_S, SNR_DB = 32, 22050, 0.05, 20.0
D = int(MAX_DELAY_S * SR)           # 1102
CPU_PROCS = 16
FP64_PEAK_FLOPS = 78.6e12           # AMD's published fp64 vector peak of the MI355X (spec, not measured)


def pcm(v):
    return (np.rint(np.clip(v, -1.0, 1.0) * 32767.0) / 32768.0).astype(np.float32)


def pair(rs):
    from scipy.signal import lfilter
    n = int(rs.randint(int(2.5 * SR), int(3.5 * SR)))
    t = np.arange(n) / SR
    x = lfilter([1.0], [1.0, -0.9], rs.randn(n)) * np.clip(np.sin(2 * np.pi * 2.5 * t + rs.uniform(0, 6)) + 0.8, 0.05, 1)
    x *= 0.5 / np.abs(x).max()
    s = int(rs.randint(-int(0.04 * SR), int(0.04 * SR) + 1))
    y = np.zeros(n)
    if s >= 0:
        y[s:] = x[:n - s]
    else:
        y[:s] = x[-s:]
    noise = rs.randn(n)
    y += noise * np.sqrt((x ** 2).mean() / (noise ** 2).mean()) * 10.0 ** (-SNR_DB / 20.0)
    return pcm(x), pcm(y), s


def inputs(n=B, seed=0):
    rs = np.random.RandomState(seed)
    return [pair(rs) for _ in range(n)]


def corr64(xy):
    """the float64 numpy oracle of one pair: r[d] for d = -D .. D, one dot per lag -> (r, argmax lag)"""
    x, y = xy[0].astype(np.float64), xy[1].astype(np.float64)
    r = np.zeros(2 * D + 1)
    for d in range(-D, D + 1):
        lo, hi = max(0, -d), min(len(x), len(y) - d)
        if hi > lo:
            r[d + D] = np.dot(x[lo:hi], y[lo + d:hi + d])
    return r, int(np.argmax(r)) - D


def fmas(pairs):
    """the multiply-adds of the definition: the sum over pairs and lags of the overlap"""
    total = 0
    for x, y, _ in pairs:
        d = np.arange(-D, D + 1)
        total += int(np.maximum(0, np.minimum(len(x), len(y) - d) - np.maximum(0, -d)).sum())
    return total


def cpu_ms(pairs, repeats=3):
    """wall time of the float64 oracle over the pairs on CPU_PROCS processes (the pool is up before the clock starts)"""
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(corr64, pairs[:procs])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(corr64, pairs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, res


def window(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def alternate(sides, calls, windows, warmup=5):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            out[k].append(round(window(fn, calls), 2))
    return {k: dict(median_us=round(float(np.median(v)), 2), min_us=min(v), max_us=max(v), windows=v) for k, v in out.items()}


def kernel_stats(path):
    """average microseconds per launch of this file's kernels from a rocprofv3 *kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            low = {k.lower(): v for k, v in row.items()}
            name = low.get('name', '')
            for key in ('xcorr_partial_kernel', 'xcorr_finish_kernel', 'sisdr_partial_kernel', 'sisdr_finish_kernel', 'wave_gather_kernel'):
                if key in name:
                    avg_ns = float(low['averagens']) if 'averagens' in low else float(low['avg_us']) * 1e3
                    out[key] = dict(calls=int(low['calls']), avg_us=round(avg_ns / 1e3, 2))
    return out


def device_inputs(pairs):
    import torch
    dev = torch.device('cuda:0')
    lens = np.array([len(x) for x, _, _ in pairs], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    px = torch.from_numpy(np.concatenate([x for x, _, _ in pairs])).to(dev)
    py = torch.from_numpy(np.concatenate([y for _, y, _ in pairs])).to(dev)
    return dev, lens, off, px, py


def conv_only(pairs, calls, out):
    """torch.nn.functional.conv1d, float32, groups = B: input the processed signals zero-padded by D on both sides, weight the references"""
    import torch
    import torch.nn.functional as F
    dev = torch.device('cuda:0')
    L = max(len(x) for x, _, _ in pairs)
    w = torch.zeros(len(pairs), 1, L, device=dev)
    inp = torch.zeros(1, len(pairs), L + 2 * D, device=dev)
    for b, (x, y, _) in enumerate(pairs):
        w[b, 0, :len(x)] = torch.from_numpy(x).to(dev)
        inp[0, b, D:D + len(y)] = torch.from_numpy(y).to(dev)
    fn = lambda: F.conv1d(inp, w, groups=len(pairs))      # noqa: E731
    got = fn()[0].argmax(dim=1).cpu().numpy() - D
    for _ in range(2):
        fn()
    v = [round(window(fn, calls), 2) for _ in range(3)]
    res = dict(median_us=round(float(np.median(v)), 2), windows=v, calls_per_window=calls,
               delays_found=int((got == np.array([s for _, _, s in pairs])).sum()))
    with open(out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps(res))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=B, help=argparse.SUPPRESS)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--trace-only', action='store_true', help='20 calls of each kernel and nothing else (for a kernel trace)')
    ap.add_argument('--conv-only', action='store_true', help='the conv1d float32 timing alone, written to --out')
    ap.add_argument('--kernel-stats', default=None, help='a rocprofv3 *kernel_stats.csv of a --trace-only run: the launches apart')
    ap.add_argument('--conv-json', default=None, help='the file a --conv-only run wrote')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_xcorr.json'))
    ap.add_argument('--merge', default=None, help='a result file of this tool: add --conv-json to it and write --out (no GPU, nothing is timed)')
    a = ap.parse_args(argv)
    if a.merge:
        res, c = json.load(open(a.merge)), json.load(open(a.conv_json))
        res['us_per_call']['conv1d_fp32'] = c
        res['conv1d_fp32_over_xcorr'] = round(c['median_us'] / res['us_per_call']['xcorr']['median_us'], 1)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res) + '\n')
        print(json.dumps(res))
        return res
    pairs = inputs(a.pairs)
    if a.trace_only or a.conv_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_xcorr: no GPU')
        if a.conv_only:
            return conv_only(pairs, 3, a.out)
        from semi_tts_amd import ops
        dev, lens, off, px, py = device_inputs(pairs)
        for _ in range(20):
            dl, _, _ = ops.xcorr_delay(px, off, lens, py, off, lens, D)
            ops.sisdr_batch(px, off, lens, py, off, lens, dl)
        torch.cuda.synchronize()
        return None
    ms, procs, cpu = cpu_ms(pairs)
    n_fma = fmas(pairs)
    nm = 'not measured'
    res = {'shape': dict(B=len(pairs), sample_rate=SR, max_lag=D, lags=2 * D + 1, snr_db=SNR_DB, samples=int(sum(len(x) for x, _, _ in pairs)),
                         seconds=[round(min(len(x) for x, _, _ in pairs) / SR, 2), round(max(len(x) for x, _, _ in pairs) / SR, 2)],
                         fp64_fmas=n_fma),
           'numpy_float64_ms_per_batch': round(ms, 2), 'numpy_processes': procs,
           'fp64_peak_flops_assumed': FP64_PEAK_FLOPS, 'fp64_peak_is': 'the published spec of the MI355X, not a measurement',
           'fma_floor_us': round(2.0 * n_fma / FP64_PEAK_FLOPS * 1e6, 2),
           'us_per_call': nm, 'kernels_us': nm, 'numpy_over_device': nm, 'conv1d_fp32_over_xcorr': nm, 'fraction_of_fp64_floor': nm,
           'align_stoi_over_stoi': nm}
    assert [d for _, d in cpu] == [s for _, _, s in pairs], 'the oracle does not find the planted delays'
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_xcorr: no GPU (--cpu-only times the numpy form alone)')
        from semi_tts_amd import metrics, ops
        dev, lens, off, px, py = device_inputs(pairs)
        dl, coef, corr = ops.xcorr_delay(px, off, lens, py, off, lens, D, want_corr=True)
        want = np.stack([r for r, _ in cpu])
        if dl.tolist() != [s for _, _, s in pairs] or not np.array_equal(corr.cpu().numpy().view(np.int64), want.view(np.int64)):
            raise SystemExit('bench_xcorr: the device correlation is not the oracle\'s')
        res['corr_bitwise_the_float64_oracle'] = True
        res['mean_coef'] = round(float(coef.mean()), 4)
        xs = [px[o:o + n] for o, n in zip(off, lens)]
        ys = [py[o:o + n] for o, n in zip(off, lens)]

        def align_stoi():
            cx, cy, _, _ = metrics.align_pairs(xs, ys, D)
            return metrics.stoi(cx, cy, SR)
        res['calls_per_window'] = a.calls
        t = alternate({'xcorr': lambda: ops.xcorr_delay(px, off, lens, py, off, lens, D), 'sisdr': lambda: ops.sisdr_batch(px, off, lens, py, off, lens, dl),
                       'align_stoi': align_stoi, 'stoi': lambda: metrics.stoi(xs, ys, SR)}, a.calls, a.windows)
        res['us_per_call'] = t
        res['numpy_over_device'] = round(ms * 1e3 / t['xcorr']['median_us'], 1)
        res['align_stoi_over_stoi'] = round(t['align_stoi']['median_us'] / t['stoi']['median_us'], 2)
        res['fraction_of_fp64_floor'] = dict(whole_call=round(res['fma_floor_us'] / t['xcorr']['median_us'], 3))
        if a.kernel_stats:
            k = kernel_stats(a.kernel_stats)
            res['kernels_us'] = k
            if 'xcorr_partial_kernel' in k:
                res['fraction_of_fp64_floor']['partial_launch'] = round(res['fma_floor_us'] / k['xcorr_partial_kernel']['avg_us'], 3)
        if a.conv_json and os.path.exists(a.conv_json):
            c = json.load(open(a.conv_json))
            res['us_per_call']['conv1d_fp32'] = c
            res['conv1d_fp32_over_xcorr'] = round(c['median_us'] / t['xcorr']['median_us'], 1)
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
