#!/usr/bin/env python3
"""What the intelligibility measure costs (st_stoi_batch, semi_tts_amd.metrics.stoi).

  Workload  B = 32 pairs of 2.5 .. 3.5 s at 22050 Hz: tones plus noise under a syllable envelope between stretches of near-silence,
            against the same signal in white noise at 5 dB SNR.
  Timed     metrics.stoi per call, device time from windows of back-to-back calls between two synchronises (median of --windows):
            `at_22050` the whole call on the 22050 Hz waveforms already on the device (both sides through audio.resample, then
            st_stoi_batch), `at_10000` the same pairs already at 10 kHz as WaveBatches (no resampling), and `kernel` ops.stoi_batch
            alone on the packed 10 kHz buffers (the five launches and the workspace allocation).
  Beside    the float64 numpy oracle (tests/stoi_oracle.py) on the 10 kHz pairs on up to 16 CPU processes, and the byte floor of the
            10 kHz call (both sides read once at 4 B per sample, over the 6.29 TB/s a device copy reaches on this card).
  Checked   before anything is timed: the scores of `at_22050` against the float64 resampling oracle composed with the float64 STOI
            oracle, within 8 times the deviation of the composed float32 numpy forms (the bound of tests/test_gpu_stoi.py), and
            the counts equal.

Prints one JSON line and writes it to profiles/bench_stoi.json (--out).

    python tools/bench_stoi.py [--calls 100] [--windows 5] [--out FILE]
    python tools/bench_stoi.py --cpu-only          # the numpy timing alone (needs no GPU; the device fields read "not measured")
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

B, SR, FS, SNR_DB = 32, 22050, 10000, 5.0
CPU_PROCS = 16
COPY_BYTES_PER_S = 6.29e12      # measured device-to-device copy rate of the card (read + write counted once each way)
FACTOR = 8.0


def pair(rs):
    """2.5 .. 3.5 s: tones plus noise under a syllable envelope with 0.2 .. 0.5 s of noise at -80 dB at both ends and one pause inside;
    -> (clean, the same in white noise at SNR_DB)"""
    n = int(rs.randint(int(2.5 * SR), int(3.5 * SR)))
    lead, tail = (int(v) for v in rs.randint(int(0.2 * SR), int(0.5 * SR), 2))
    t = np.arange(n - lead - tail) / SR
    env = np.clip(np.sin(2 * np.pi * 2.5 * t + rs.uniform(0, 6)) + 0.8, 0.05, 1)
    x = env * (0.3 * np.sin(2 * np.pi * rs.uniform(100, 800) * t) + 0.1 * np.sin(2 * np.pi * rs.uniform(800, 3000) * t)) + 0.01 * rs.randn(len(t))
    a = int(rs.uniform(0.3, 0.6) * len(x))
    x[a:a + int(0.15 * SR)] *= 1e-4
    x = np.concatenate([3e-5 * rs.randn(lead), x, 3e-5 * rs.randn(tail)])
    noise = rs.randn(n)
    noise *= np.sqrt((x ** 2).mean() / (noise ** 2).mean()) * 10.0 ** (-SNR_DB / 20.0)
    return x.astype(np.float32), (x + noise).astype(np.float32)


def inputs(n=B, seed=0):
    rs = np.random.RandomState(seed)
    return [pair(rs) for _ in range(n)]


def _resample32(x):
    """the resampler's float32 form (float32 table, products and one chain over ascending taps), as tests/test_gpu_stoi.py"""
    import resample_oracle as RO
    o, n, taps, first, tab, _ = RO.table64(SR, FS)
    tab = tab.astype(np.float32)
    L, M = len(x), RO.out_len(len(x), SR, FS)
    m = np.arange(M, dtype=np.int64)
    p = m % n
    idx = (m * o // n + first[p])[:, None] + np.arange(taps)[None, :]
    xv = np.where((idx >= 0) & (idx < L), x[np.clip(idx, 0, L - 1)], np.float32(0))
    out = np.zeros(M, np.float32)
    for k in range(taps):
        out += tab[p, k] * xv[:, k]
    return out


def _down(xy):
    import resample_oracle as RO
    return RO.resample_compact(xy[0], SR, FS), RO.resample_compact(xy[1], SR, FS)


def _one(xy):
    """the float64 oracle on one 10 kHz pair"""
    import stoi_oracle as SO
    r = SO.stoi(xy[0], xy[1])
    return r['score'], r['counts']


def _one32(xy):
    import stoi_oracle as SO
    return SO.stoi(_resample32(xy[0]), _resample32(xy[1]), np.float32)['score']


def cpu_ms(pairs10, repeats=3):
    """wall time of the float64 oracle over the pairs on CPU_PROCS processes (the pool is up before the clock starts)"""
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, pairs10[:procs])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, pairs10, chunksize=1)
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


def alternate(sides, calls, windows, warmup=10):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            out[k].append(round(window(fn, calls), 2))
    return {k: dict(median_us=round(float(np.median(v)), 2), min_us=min(v), max_us=max(v), windows=v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_stoi.json'))
    a = ap.parse_args(argv)
    pairs = inputs()
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:      # (before the GPU is opened: the workers are forked from a process without one)
        pairs10 = pool.map(_down, pairs, chunksize=1)
        score32 = pool.map(_one32, pairs, chunksize=1)
    ms, procs, cpu = cpu_ms(pairs10)
    samples, samples10 = int(sum(len(x) for x, _ in pairs)), int(sum(len(x) for x, _ in pairs10))
    want = np.array([s for s, _ in cpu], np.float64)
    counts = np.array([c for _, c in cpu], np.int64)
    e32 = float(np.abs(np.array(score32, np.float64) - want).max())
    nm = 'not measured'
    res = {'shape': dict(B=B, sample_rate=SR, snr_db=SNR_DB, samples=samples, samples_at_10k=samples10, frames=int(counts[:, 0].sum()),
                         kept=int(counts[:, 1].sum()), segments=int(counts[:, 3].sum()),
                         seconds=[round(min(len(x) for x, _ in pairs) / SR, 2), round(max(len(x) for x, _ in pairs) / SR, 2)]),
           'oracle_mean_stoi': round(float(want[:, 0].mean()), 6), 'oracle_mean_estoi': round(float(want[:, 1].mean()), 6),
           'numpy_float64_ms_per_batch': round(ms, 2), 'numpy_processes': procs, 'e32_scores': e32,
           'byte_floor_us': round(2 * 4.0 * samples10 / COPY_BYTES_PER_S * 1e6, 3), 'copy_bytes_per_s_assumed': COPY_BYTES_PER_S,
           'stoi_us_per_call': nm, 'numpy_over_device': nm, 'device_over_byte_floor': nm, 'resampling_share': nm}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_stoi: no GPU (--cpu-only times the numpy form alone)')
        from semi_tts_amd import audio, ops
        from semi_tts_amd.metrics import stoi
        dev = torch.device('cuda:0')
        xs = [torch.from_numpy(x).to(dev) for x, _ in pairs]
        ys = [torch.from_numpy(y).to(dev) for _, y in pairs]
        got = stoi(xs, ys, SR)
        dev_score, dev_counts = got.score.double().cpu().numpy(), got.counts.cpu().numpy()
        worst = float(np.abs(dev_score - want).max())
        if not (dev_counts == counts).all() or not worst <= FACTOR * e32:
            raise SystemExit('bench_stoi: the device scores are not the oracle\'s (worst deviation %.3e, bound %.3e)' % (worst, FACTOR * e32))
        res['scores_within_bound_of_float64'] = True
        res['worst_score_deviation'] = worst
        xb, yb = audio.resample(xs, SR, FS), audio.resample(ys, SR, FS)
        px, py = xb.packed(dev), yb.packed(dev)
        res['calls_per_window'] = a.calls
        t = alternate({'at_22050': lambda: stoi(xs, ys, SR), 'at_10000': lambda: stoi(xb, yb, FS),
                       'kernel': lambda: ops.stoi_batch(px, py, xb.offsets, xb.lens)}, a.calls, a.windows)
        res['stoi_us_per_call'] = t
        res['numpy_over_device'] = round(ms * 1e3 / t['at_10000']['median_us'], 1)
        res['device_over_byte_floor'] = round(t['kernel']['median_us'] / res['byte_floor_us'], 1)
        res['resampling_share'] = round(1.0 - t['at_10000']['median_us'] / t['at_22050']['median_us'], 3)
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
