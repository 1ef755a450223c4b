#!/usr/bin/env python3
"""What silence trimming costs (st_trim_silence, AudioConverter.trim_batch, corpus.DeviceSplit(trim=)).

  kernel    ops.trim_silence on B = 32 utterances of 2.5 .. 3.5 s at 22050 Hz (0.2 .. 0.5 s of near-silence at both ends), frames of
            2048 every 512: device time per call from windows of back-to-back calls between two synchronises (median of --windows),
            beside the float32 numpy form of the definition (tests/trim_oracle.py) on up to 16 CPU processes, beside the byte floor
            (4 B per sample read once, over the 6.29 TB/s a device copy reaches on this card) and beside st_audio_mfcc per frame.  The
            bounds are compared with the float64 oracle's before anything is timed.
  load      corpus.load_splits on a 64-utterance split written to a temporary directory, without and with trim (the one-off cost, wall
            time to a synchronise), and one fetch (B = 32) from each -- and from a third split whose files were cut on the host to
            the same bounds and loaded without trim: the fetch "at equal trimmed length" a trimmed split has to match.

Prints one JSON line and writes it to profiles/bench_trim.json (--out).

    python tools/bench_trim.py [--calls 300] [--windows 5] [--out FILE]
    python tools/bench_trim.py --cpu-only          # the numpy timing alone (needs no GPU; the device fields read "not measured")
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
import numpy as np   # noqa: E402

B, SR, FL, HOP, TOP_DB = 32, 22050, 2048, 512, 60.0
TRIM = dict(top_db=TOP_DB, frame_length=FL, hop_length=HOP, pad_ms=0.0)
CPU_PROCS = 16
COPY_BYTES_PER_S = 6.29e12      # measured device-to-device copy rate of the card (read + write counted once each way)


def utterance(rs):
    """2.5 .. 3.5 s: tones plus noise under a syllable envelope between 0.2 .. 0.5 s of noise at -80 dB"""
    n = int(rs.randint(int(2.5 * SR), int(3.5 * SR)))
    lead, tail = (int(v) for v in rs.randint(int(0.2 * SR), int(0.5 * SR), 2))
    t = np.arange(n - lead - tail) / SR
    env = np.clip(np.sin(2 * np.pi * 2.5 * t + rs.uniform(0, 6)) + 0.8, 0.05, 1)
    x = env * (0.3 * np.sin(2 * np.pi * rs.uniform(100, 800) * t) + 0.1 * np.sin(2 * np.pi * rs.uniform(800, 3000) * t)) + 0.01 * rs.randn(len(t))
    return np.concatenate([3e-5 * rs.randn(lead), x, 3e-5 * rs.randn(tail)]).astype(np.float32)


def inputs(n=B, seed=0):
    rs = np.random.RandomState(seed)
    return [utterance(rs) for _ in range(n)]


def _one(x):
    """the float32 numpy form: energies in float32, the decision as the kernel takes it"""
    import trim_oracle as O
    e = np.maximum(O.frame_energy(x, FL, HOP, np.float32), np.float32(1e-10))
    idx = np.flatnonzero(e > e.max() * np.float32(O.ratio_of(TOP_DB)))
    return int(idx[0]) * HOP, min(len(x), (int(idx[-1]) + 1) * HOP)


def cpu_ms(xs, repeats=3):
    """wall time of the numpy form over the utterances on CPU_PROCS processes (the pool is up before the clock starts)"""
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, xs[:procs])
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, xs, chunksize=1)
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


def alternate(sides, calls, windows, warmup=20):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            out[k].append(round(window(fn, calls), 2))
    return {k: dict(median_us=round(float(np.median(v)), 2), min_us=min(v), max_us=max(v), windows=v) for k, v in out.items()}


def write_corpus(root, waves):
    """the utterances `waves` (int16 arrays) as an all-paired data.corpus under root -> its dict"""
    import csv
    import wave
    rs = np.random.RandomState(1)
    vocab = ['P%02d' % i for i in range(40)]
    os.makedirs(os.path.join(root, 'wav', 'spk'), exist_ok=True)
    with open(os.path.join(root, 'partition.csv'), 'w', newline='') as fp, open(os.path.join(root, 'map.tsv'), 'w', newline='') as fm:
        wp, wm = csv.writer(fp), csv.writer(fm, delimiter='\t')
        wp.writerow(['', 'speaker', 'split', 'duration'])
        wm.writerow(['file', 'phn_seq', 'spkr'])
        for k, pcm in enumerate(waves):
            fid = 'u%03d' % k
            with wave.open(os.path.join(root, 'wav', 'spk', fid + '.wav'), 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(SR)
                w.writeframes(np.ascontiguousarray(pcm, dtype='<i2').tobytes())
            wp.writerow([fid, 'spk', 'paired', '%.3f' % (len(pcm) / SR)])
            wm.writerow([fid, ' '.join(vocab[int(i)] for i in rs.randint(0, 40, int(rs.randint(20, 43)))), 'spk'])
    with open(os.path.join(root, 'spkr.json'), 'w') as f:
        json.dump({'spk': 0}, f)
    with open(os.path.join(root, 'phn.vocab'), 'w') as f:
        f.write('\n'.join(vocab) + '\n')
    return dict(name='vctk', path=os.path.join(root, 'wav'), partition_table=os.path.join(root, 'partition.csv'),
                map_table=os.path.join(root, 'map.tsv'), spkr_map=os.path.join(root, 'spkr.json'),
                vocab_file=os.path.join(root, 'phn.vocab'), batch_size=32, bucketing=True)


def load_figures(conv, calls, windows):
    """the one-off load cost without / with trim and a fetch from each and from a host-cut copy of the corpus"""
    import torch
    from semi_tts_amd.corpus import load_splits
    pcm = [np.rint(np.clip(x, -1, 1) * 32767).astype('<i2') for x in inputs(64, seed=2)]
    out = {}
    with tempfile.TemporaryDirectory() as root:
        cfg = write_corpus(os.path.join(root, 'a'), pcm)

        def load(c, trim):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, sets = load_splits(c, conv, 3, ['paired'], {'paired': 32}, verbose=lambda m: None, trim=trim)
            torch.cuda.synchronize()
            return sets['paired'], (time.perf_counter() - t0) * 1e3
        load(cfg, TRIM)                                             # (first use: library load, filterbank upload)
        loads = {'none': [], 'trim': []}
        for _ in range(3):
            plain, ms = load(cfg, None)
            loads['none'].append(round(ms, 2))
            trimmed, ms = load(cfg, TRIM)
            loads['trim'].append(round(ms, 2))
        out['load_splits_ms'] = {k: dict(median_ms=float(np.median(v)), runs=v) for k, v in loads.items()}
        out['load_trim_cost_ms'] = round(out['load_splits_ms']['trim']['median_ms'] - out['load_splits_ms']['none']['median_ms'], 2)
        out['trim_report'] = trimmed.trim_report
        # the same corpus cut on the host to the bounds the device found, loaded without trim
        paths = [u.path for u in plain.rows]
        bounds = conv.load_batch(paths, trim=TRIM).bounds
        by = {os.path.basename(p): (int(a), int(b)) for p, (a, b) in zip(paths, bounds)}
        cut = [pcm[k][by['u%03d.wav' % k][0]:by['u%03d.wav' % k][1]] for k in range(len(pcm))]
        pre, _ = load(write_corpus(os.path.join(root, 'b'), cut), None)
        assert sorted(pre.lens.tolist()) == sorted(trimmed.lens.tolist())
        out['fetch_us'] = alternate({'untrimmed': plain.fetch, 'trimmed': trimmed.fetch, 'cut_on_host': pre.fetch}, calls, windows)
        out['seconds_per_utterance'] = dict(untrimmed=round(float(plain.lens.mean()) / SR, 3), trimmed=round(float(trimmed.lens.mean()) / SR, 3))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_trim.json'))
    a = ap.parse_args(argv)
    xs = inputs()
    frames = [1 + len(x) // HOP for x in xs]
    samples = int(sum(len(x) for x in xs))
    ms, procs, cpu = cpu_ms(xs)                        # (before the GPU is opened: the workers are forked from a process without one)
    nm = 'not measured'
    res = {'shape': dict(B=B, sample_rate=SR, frame_length=FL, hop=HOP, top_db=TOP_DB, frames=int(sum(frames)), samples=samples,
                         seconds=[round(min(map(len, xs)) / SR, 2), round(max(map(len, xs)) / SR, 2)]),
           'numpy_float32_ms_per_batch': round(ms, 2), 'numpy_processes': procs,
           'byte_floor_us': round(4.0 * samples / COPY_BYTES_PER_S * 1e6, 3), 'copy_bytes_per_s_assumed': COPY_BYTES_PER_S,
           'trim_us_per_batch': nm, 'numpy_over_device': nm, 'device_over_byte_floor': nm, 'mfcc_us_per_batch': nm, 'trim_over_mfcc_per_frame': nm,
           'load': nm}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_trim: no GPU (--cpu-only times the numpy form alone)')
        import yaml
        import trim_oracle as O
        from semi_tts_amd import ops
        from semi_tts_amd.audio import WaveBatch, load_audio_transform
        dev = torch.device('cuda:0')
        config = yaml.load(open(os.path.join(ROOT, 'config', 'supervised.yaml')), Loader=yaml.FullLoader)
        conv = load_audio_transform(**dict(config['data']['audio']))
        assert conv.sr == SR
        wb = WaveBatch([torch.from_numpy(x) for x in xs])
        packed = wb.packed(dev)

        def trim():
            return ops.trim_silence(packed, wb.offsets, wb.lens, FL, HOP, TOP_DB)
        got = trim()[1].cpu().numpy()
        want = [O.trim(xs[k], FL, HOP, TOP_DB)['bounds'] for k in wb.order]
        if got.tolist() != want or [list(cpu[k]) for k in wb.order] != [w[:2] for w in want]:
            raise SystemExit('bench_trim: the device bounds are not the oracle\'s')
        res['bounds_equal_to_float64'] = True
        res['kept_fraction'] = round(float((got[:, 1] - got[:, 0]).sum()) / samples, 4)
        res['calls_per_window'] = a.calls
        t = alternate({'trim': trim, 'mfcc': lambda: conv.extract_mfcc_batch(wb)}, a.calls, a.windows)
        res['trim_us_per_batch'], res['mfcc_us_per_batch'] = t['trim'], t['mfcc']
        us = t['trim']['median_us']
        mfcc_frames = int((1 + wb.lens // conv.hop_length_mfcc).sum())
        res['numpy_over_device'] = round(ms * 1e3 / us, 1)
        res['device_over_byte_floor'] = round(us / res['byte_floor_us'], 1)
        res['mfcc_frames'] = mfcc_frames
        res['trim_over_mfcc_per_frame'] = round((us / sum(frames)) / (t['mfcc']['median_us'] / mfcc_frames), 3)
        res['load'] = load_figures(conv, max(100, a.calls // 3), a.windows)
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
