#!/usr/bin/env python3
"""What loudness normalisation costs (st_loudness_batch, st_wave_gain, corpus.DeviceSplit(loudness=)).

  kernel    ops.loudness on B = 32 utterances of 2.5 .. 3.5 s at 16000 Hz, alone and followed by ops.wave_gain in place: device time
            per call from windows of back-to-back calls between two synchronises (median of --windows), beside the float64
            scipy.signal.lfilter + numpy form of the definition (tests/loudness_oracle.py) on up to 16 CPU processes, beside the byte
            floor (the samples read twice at 4 B, over the 6.29 TB/s a device copy reaches on this card) and beside st_trim_silence on
            the same batch, per sample.  The integrated loudness is compared with the float64 oracle's before anything is timed.
  load      corpus.load_splits on a 64-utterance split (tools/bench_trim.py's, 22050 Hz) written to a temporary directory, without and
            with loudness (the one-off cost, wall time to a synchronise).

Prints one JSON line and writes it to profiles/bench_loudness.json (--out).

    python tools/bench_loudness.py [--calls 300] [--windows 5] [--out FILE]
    python tools/bench_loudness.py --cpu-only      # the lfilter timing alone (needs no GPU; the device fields read "not measured")
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np   # noqa: E402

B, SR = 32, 16000
ARGS = dict(target=-23.0, peak_db=-1.0, max_gain_db=30.0)
TRIM_FL, TRIM_HOP, TRIM_TOP_DB = 2048, 512, 60.0
CPU_PROCS = 16
COPY_BYTES_PER_S = 6.29e12      # measured device-to-device copy rate of the card (read + write counted once each way)
LAUNCHES = dict(meter=4, gain=1)


def utterance(rs):
    """2.5 .. 3.5 s: tones plus noise under a syllable envelope, at a level drawn over 20 dB"""
    n = int(rs.randint(int(2.5 * SR), int(3.5 * SR)))
    t = np.arange(n) / SR
    env = np.clip(np.sin(2 * np.pi * 2.5 * t + rs.uniform(0, 6)) + 0.8, 0.05, 1)
    x = env * (0.3 * np.sin(2 * np.pi * rs.uniform(100, 800) * t) + 0.1 * np.sin(2 * np.pi * rs.uniform(800, 3000) * t)) + 0.01 * rs.randn(n)
    return (10.0 ** rs.uniform(-1.0, 0.0) * x).astype(np.float32)


def inputs(n=B, seed=0):
    rs = np.random.RandomState(seed)
    return [utterance(rs) for _ in range(n)]


def _one(x):
    """the float64 form: lfilter per stage, hop sums, blocks, gates, the gain and the product"""
    import loudness_oracle as O
    m = O.measure(x, SR, **ARGS)
    return m['lufs'], m['flags'], float(np.abs(O.apply_gain(x, m['gain'])).max())


def cpu_ms(xs, repeats=3):
    """wall time of the float64 form over the utterances on CPU_PROCS processes (the pool is up before the clock starts)"""
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, xs[:procs])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, xs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, res


def load_figures(calls, windows):
    """the one-off load cost of a 64-utterance split without / with loudness"""
    import torch
    import yaml
    import bench_trim as BT
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.corpus import load_splits
    config = yaml.load(open(os.path.join(ROOT, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
    conv = load_audio_transform(**dict(config['data']['audio']))
    assert conv.sr == BT.SR
    pcm = [np.rint(np.clip(x, -1, 1) * 32767).astype('<i2') for x in BT.inputs(64, seed=2)]
    out = {}
    with tempfile.TemporaryDirectory() as root:
        cfg = BT.write_corpus(os.path.join(root, 'a'), pcm)

        def load(loudness):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, sets = load_splits(cfg, conv, 3, ['paired'], {'paired': 32}, verbose=lambda m: None, loudness=loudness)
            torch.cuda.synchronize()
            return sets['paired'], (time.perf_counter() - t0) * 1e3
        load(ARGS)                                                  # (first use: library load, table upload)
        loads = {'none': [], 'loudness': []}
        for _ in range(3):
            loads['none'].append(round(load(None)[1], 2))
            ds, ms = load(ARGS)
            loads['loudness'].append(round(ms, 2))
        out['load_splits_ms'] = {k: dict(median_ms=float(np.median(v)), runs=v) for k, v in loads.items()}
        out['load_loudness_cost_ms'] = round(out['load_splits_ms']['loudness']['median_ms'] - out['load_splits_ms']['none']['median_ms'], 2)
        out['loudness_report'] = ds.loudness_report
        out['sample_rate'], out['utterances'], out['samples'] = conv.sr, len(ds.rows), int(ds.lens.sum())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the lfilter timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_loudness.json'))
    a = ap.parse_args(argv)
    xs = inputs()
    samples = int(sum(len(x) for x in xs))
    ms, procs, cpu = cpu_ms(xs)                        # (before the GPU is opened: the workers are forked from a process without one)
    nm = 'not measured'
    res = {'shape': dict(B=B, sample_rate=SR, hop=(SR + 5) // 10, samples=samples, hops=int(sum(len(x) // ((SR + 5) // 10) for x in xs)),
                         seconds=[round(min(map(len, xs)) / SR, 2), round(max(map(len, xs)) / SR, 2)], **ARGS),
           'launches': LAUNCHES, 'lfilter_float64_ms_per_batch': round(ms, 2), 'cpu_processes': procs,
           'byte_floor_us': round(8.0 * samples / COPY_BYTES_PER_S * 1e6, 3), 'copy_bytes_per_s_assumed': COPY_BYTES_PER_S,
           'loudness_us_per_batch': nm, 'loudness_and_gain_us_per_batch': nm, 'cpu_over_device': nm, 'byte_floor_fraction': nm,
           'trim_us_per_batch': nm, 'loudness_over_trim_per_sample': nm, 'load': nm}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_loudness: no GPU (--cpu-only times the lfilter form alone)')
        from bench_trim import alternate
        from semi_tts_amd import ops
        from semi_tts_amd.audio import WaveBatch
        dev = torch.device('cuda:0')
        wb = WaveBatch([torch.from_numpy(x) for x in xs])
        packed = wb.packed(dev)
        scratch = packed.clone()

        def meter():
            return ops.loudness(packed, wb.offsets, wb.lens, SR, **ARGS)

        def meter_gain():
            _, stats, _ = ops.loudness(packed, wb.offsets, wb.lens, SR, **ARGS)
            return ops.wave_gain(packed, wb.offsets, wb.lens, stats, out=scratch)

        _, stats, counts = meter()
        got, flags = stats[:, 0].cpu().numpy(), counts[:, 3].cpu().numpy()
        want = [cpu[k] for k in wb.order]
        if any(abs(float(g) - w[0]) > 0.01 for g, w in zip(got, want)) or flags.tolist() != [w[1] for w in want]:
            raise SystemExit('bench_loudness: the device loudness is not the oracle\'s')
        res['lufs_within_0.01_of_float64'] = True
        res['lufs_range'] = [round(float(got.min()), 2), round(float(got.max()), 2)]
        res['calls_per_window'] = a.calls
        t = alternate({'meter': meter, 'meter_gain': meter_gain,
                       'trim': lambda: ops.trim_silence(packed, wb.offsets, wb.lens, TRIM_FL, TRIM_HOP, TRIM_TOP_DB)}, a.calls, a.windows)
        res['loudness_us_per_batch'], res['loudness_and_gain_us_per_batch'], res['trim_us_per_batch'] = t['meter'], t['meter_gain'], t['trim']
        us = t['meter']['median_us']
        res['cpu_over_device'] = round(ms * 1e3 / us, 1)
        res['byte_floor_fraction'] = round(res['byte_floor_us'] / us, 4)
        res['loudness_over_trim_per_sample'] = round(us / t['trim']['median_us'], 2)      # (the same samples on both sides)
        res['load'] = load_figures(max(100, a.calls // 3), a.windows)
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
