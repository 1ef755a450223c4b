#!/usr/bin/env python3
"""Pitch tracking of a corpus-like batch (st_f0_yin, AudioConverter.extract_f0_batch) and the F0 figures along a warp
(st_f0_path_scores, semi_tts_amd.metrics.f0_scores): 32 utterances of about 3 s at the configuration's framing (22050 Hz, hop 220,
lags 44 .. 368, window 736: about 9500 frames of 2.7e5 multiply-adds each).  Device time per batch from events around windows of
back-to-back calls, beside the vectorised float32 numpy form of the same definition (tests/f0_oracle.py) on up to 16 CPU processes and
beside st_audio_mfcc on the same batch; and what the difference loop reaches of the fp32 FMA peak (CUs x 128 lanes x clock) and of the
LDS read rate (128 B / clk / CU for 4-byte reads).  A direct-form term is a subtraction and an FMA, so half the FMA peak is the loop's
ceiling on the vector ALU; a plain loop of two LDS reads per term is bound at 16 terms / clk / CU.  The device track is compared with
the numpy one before anything is timed.  Prints one JSON line and writes it to profiles/bench_f0.json (--out).

    python tools/bench_f0.py [--calls 100] [--windows 5] [--out FILE]
    python tools/bench_f0.py --cpu-only          # the numpy timing alone (needs no GPU; the device fields read "not measured")
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

B, SR, HOP, TAU_MIN, TAU_MAX, W, THR = 32, 22050, 220, 44, 368, 736, 0.15
CPU_PROCS = 16
CLOCK_HZ = 2.4e9            # MI355X engine clock under load
LANES_PER_CU = 128          # fp32 FMA lanes of a CU (4 SIMDs x 32)
LDS_B32_BYTES_PER_CLK = 128
STEP_J = 8                  # F0_J of f0.hip


def lags_per_lane(tau_max):
    """f0_lags_per_lane of f0.hip"""
    best, cost = 4, 1 << 30
    for tl in (4, 6, 8):
        c = (tau_max + 64 * tl) // (64 * tl) * tl
        if c <= cost:
            best, cost = tl, c
    return best


def inputs(seed=0, stretch=1.0):
    """B voiced / unvoiced utterances of 2.7 .. 3 s (times `stretch`): a harmonic sum on a moving pitch under a syllable envelope"""
    rs = np.random.RandomState(seed)
    out = []
    for b in range(B):
        n = int(rs.randint(int(2.7 * SR), 3 * SR + 1) * stretch) if b else int(3 * SR * stretch)
        t = np.arange(n) / SR / stretch
        f = rs.uniform(90, 260) * (1 + 0.1 * np.sin(2 * np.pi * rs.uniform(0.3, 1.0) * t)) * stretch ** 0.1
        ph = 2 * np.pi * np.cumsum(f) / SR
        env = np.clip(np.sin(2 * np.pi * 2.5 * t + rs.uniform(0, 6)) + 0.6, 0, 1)
        y = sum(np.sin(k * ph) / k for k in range(1, 7))
        out.append((0.2 * env * y + 0.01 * rs.randn(n)).astype(np.float32))
    return out


def _one(x):
    import f0_oracle as O
    f0, _, tau = O.yin_f32(x, SR, HOP, W, TAU_MIN, TAU_MAX, THR)
    return f0, tau


def cpu_ms(xs, repeats=3):
    """wall time of the numpy form over the B utterances on CPU_PROCS processes (the pool is up before the clock starts)"""
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, xs[:procs])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, xs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_f0.json'))
    a = ap.parse_args(argv)
    xs = inputs()
    frames = [1 + len(x) // HOP for x in xs]
    terms = float(sum(frames)) * W * (TAU_MAX + 1)
    tl = lags_per_lane(TAU_MAX)
    ms, procs, cpu = cpu_ms(xs)                        # (before the GPU is opened: the workers are forked from a process without one)
    nm = 'not measured'
    res = {'shape': dict(B=B, sample_rate=SR, hop=HOP, tau_min=TAU_MIN, tau_max=TAU_MAX, W=W, frames=int(sum(frames)),
                         seconds=[round(min(map(len, xs)) / SR, 2), round(max(map(len, xs)) / SR, 2)]),
           'difference_terms_per_batch': terms, 'lags_per_lane': tl, 'lds_reads_per_term': round((2 * STEP_J + tl - 1) / (STEP_J * tl), 4),
           'numpy_float32_ms_per_batch': round(ms, 1), 'numpy_processes': procs,
           'f0_yin_us_per_batch': nm, 'f0_path_scores_us_per_batch': nm, 'numpy_over_device': nm, 'mfcc_us_per_batch': nm,
           'f0_over_mfcc_per_frame': nm, 'fraction_of_fp32_fma_peak': nm, 'fraction_of_lds_read_rate': nm,
           'fraction_of_two_reads_per_term_bound': nm}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_f0: no GPU (--cpu-only times the numpy form alone)')
        import yaml
        from semi_tts_amd import metrics, ops
        from semi_tts_amd.audio import WaveBatch, load_audio_transform
        dev = torch.device('cuda:0')
        config = yaml.load(open(os.path.join(ROOT, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
        conv = load_audio_transform(**dict(config['data']['audio']))
        assert (conv.sr, conv.hop_length_mfcc) + conv.f0_lags() == (SR, HOP, TAU_MIN, TAU_MAX, W)
        wb = WaveBatch([torch.from_numpy(x) for x in xs])
        packed, T_pad = wb.packed(dev), int(1 + wb.lens.max() // HOP)

        def yin():
            return ops.f0_yin(packed, wb.offsets, wb.lens, HOP, W, TAU_MIN, TAU_MAX, float(SR), THR, T_pad)[0]
        f0 = yin().cpu().numpy()
        same = total = 0
        for row, k in enumerate(wb.order):
            want_f0, want_tau = cpu[k]
            got_tau = np.where(f0[row, :frames[k]] > 0, np.round(SR / np.maximum(f0[row, :frames[k]], 1e-9)), 0)
            same += int((got_tau == want_tau).sum())
            total += frames[k]
        if same < 0.995 * total:
            raise SystemExit('bench_f0: the device track takes the numpy decision on %d of %d frames only' % (same, total))
        res['frames_equal_to_numpy'] = [same, total]

        def windows(fn, calls):
            for _ in range(max(20, calls // 2)):         # (the clocks settle within the first few hundred launches)
                fn()
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
        res['f0_yin_us_per_batch'] = y = windows(yin, a.calls)
        res['mfcc_us_per_batch'] = m = windows(lambda: conv.extract_mfcc_batch(wb), a.calls)
        # the figures along the warp of the MCD against a second batch, a tenth slower
        wb2 = WaveBatch([torch.from_numpy(x) for x in inputs(1, 1.1)], order=np.arange(B))
        fr1, fr2 = (1 + wb.lens // HOP).tolist(), (1 + wb2.lens // HOP).tolist()
        _, plen, path = metrics.mcd(conv.extract_mfcc_batch(wb), fr1, conv.extract_mfcc_batch(wb2), fr2)
        f0a, f0b = conv.extract_f0_batch(wb), conv.extract_f0_batch(wb2)
        res['f0_path_scores_us_per_batch'] = windows(lambda: ops.f0_path_scores(f0a, f0b, path, plen), 4 * a.calls)
        res['path_len_mean'] = round(float(plen.float().mean()), 1)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        per_s = terms / (y['median_us'] * 1e-6)
        res['numpy_over_device'] = round(ms * 1e3 / y['median_us'], 1)
        res['f0_over_mfcc_per_frame'] = round(y['median_us'] / m['median_us'], 2)      # (the same frames on both sides)
        res['compute_units'], res['clock_hz_assumed'] = cus, CLOCK_HZ
        res['difference_terms_per_s'] = float('%.4g' % per_s)
        res['fraction_of_fp32_fma_peak'] = round(per_s / (cus * LANES_PER_CU * CLOCK_HZ), 4)
        res['fraction_of_lds_read_rate'] = round(per_s * res['lds_reads_per_term'] * 4 / (cus * LDS_B32_BYTES_PER_CLK * CLOCK_HZ), 4)
        res['fraction_of_two_reads_per_term_bound'] = round(per_s / (cus * (LDS_B32_BYTES_PER_CLK / 8) * CLOCK_HZ), 4)
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
