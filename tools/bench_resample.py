#!/usr/bin/env python3
"""Sample-rate conversion (st_resample_batch) on a corpus-like batch: 32 utterances of about 3 s (2.5 .. 3.5 s, ragged) at
48000 -> 22050 Hz and at 16000 -> 22050 Hz, float32 and int16 PCM input.  One JSON line, also written to --out:

  per case   us per launch (device events around a window of launches, after warm-up; median / min / spread over the rounds),
             the algorithmic bytes (input read once, output written once; the table is not counted), those bytes over the time
             as a fraction of the HBM peak and of what a float4 copy reaches, audio seconds per second
  cpu        the same definition as a strided torch conv1d (the full form: n output channels of 2 ceil(W) + o taps, stride o,
             the batch zero-padded to its longest utterance) on 16 CPU threads, and its ratio to the launch
  max_err    the launch against that CPU form, as a sanity check of what was timed

The GPU step runs in a child process under a time limit of its own; if it fails or runs out of time nothing further is started
and the tool exits non-zero.  Without a GPU the tool refuses to run: a CPU run measures nothing.

    python tools/bench_resample.py [--batch-size 32 --seconds 3 --rounds 20 --window 50 --warmup 5 --out profiles/bench_resample.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

HBM_PEAK_BPS = 8.0e12            # HBM3E, specification
HBM_COPY_BPS = 6.3e12            # what a float4 copy reaches
CASES = [(48000, 22050), (16000, 22050)]
GPU_STEP_TIMEOUT_S = 240


def make_batch(B, seconds, sr, seed=0):
    """B utterances of 0.83 .. 1.17 x `seconds`, longest first: a tone under noise, |x| < 1"""
    rs = np.random.RandomState(seed)
    lens = [int(round(v * sr)) for v in np.linspace(seconds * 7 / 6, seconds * 5 / 6, B)]
    return [np.clip(0.3 * np.sin(2 * np.pi * 220 * np.arange(L) / sr + rs.rand()) + 0.1 * rs.randn(L), -1, 1).astype(np.float32) for L in lens]


def full_kernel(orig, new, lpw=6, rolloff=0.99):
    """(kernel (n, 1, 2 width + o) float32, width, o, n): the clamped-window form of the definition, one output channel per phase"""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    j = np.arange(-width, width + o, dtype=np.float64)
    t = np.clip((j[None, :] / o - np.arange(n, dtype=np.float64)[:, None] / n) * base, -lpw, lpw)
    a = t * np.pi
    k = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a)) * np.cos(t * np.pi / lpw / 2.0) ** 2 * (base / o)
    return torch.from_numpy(k.astype(np.float32))[:, None, :], width, o, n


def cpu_conv(waves, orig, new, kern=None):
    """the batch, zero-padded to its longest utterance, through F.conv1d with stride o: -> (B, n * Q) float32 (row b valid on
    ceil(n L_b / o) samples)"""
    k, width, o, n = kern if kern is not None else full_kernel(orig, new)
    Lmax = max(len(w) for w in waves)
    x = torch.zeros(len(waves), 1, Lmax + 2 * width + o)
    for b, w in enumerate(waves):
        x[b, 0, width:width + len(w)] = torch.from_numpy(w)
    y = torch.nn.functional.conv1d(x, k, stride=o)                     # (B, n, Q)
    return y.transpose(1, 2).reshape(len(waves), -1)


def gpu_step(a):
    from semi_tts_amd import audio, ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample: needs a GPU (a CPU run measures nothing)')
    dev = torch.device('cuda:0')
    out = {}
    for orig, new in CASES:
        waves = make_batch(a.batch_size, a.seconds, orig)
        o, n, taps, first, _ = audio.resample_table(orig, new)
        _, _, _, first_d, table_d = audio.resample_table(orig, new, device=dev)
        lens = np.array([len(w) for w in waves])
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
        out_lens = [audio.resampled_len(int(L), orig, new) for L in lens]
        out_off = np.concatenate([[0], np.cumsum(out_lens)[:-1]]).tolist()
        n_out = int(sum(out_lens))
        y = torch.empty(n_out, device=dev)
        for kind in ('float32', 'int16'):
            if kind == 'float32':
                x = torch.cat([torch.from_numpy(w) for w in waves]).to(dev)
            else:
                x = torch.cat([torch.from_numpy(np.rint(w * 32767).astype(np.int16)) for w in waves]).to(dev)
            call = lambda: ops.resample_batch(x, off, lens, o, n, first_d, table_d, int(first.min()), int(first.max()), out=y)    # noqa: E731
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            t = []
            for _ in range(a.rounds):
                ev[0].record()
                for _ in range(a.window):
                    call()
                ev[1].record()
                ev[1].synchronize()
                t.append(ev[0].elapsed_time(ev[1]) * 1e3 / a.window)
            t = np.array(t)
            us = float(np.median(t))
            nbytes = int(x.numel() * x.element_size() + 4 * n_out)
            res = dict(us=round(us, 2), us_min=round(float(t.min()), 2), spread=round(float((t.max() - t.min()) / us), 4), bytes=nbytes,
                       hbm_floor_us=round(nbytes / HBM_PEAK_BPS * 1e6, 3), fraction_of_hbm_peak=round(nbytes / HBM_PEAK_BPS * 1e6 / us, 4),
                       fraction_of_copy_rate=round(nbytes / HBM_COPY_BPS * 1e6 / us, 4),
                       audio_seconds_per_second=round(float(lens.sum()) / orig / (us * 1e-6), 1), taps=taps, phases=n,
                       lds_bytes=4 * sum(ops.resample_lds_floats(o, n, taps, int(first.min()), int(first.max()))),
                       workgroups=int(sum(-(-m // ops.RESAMPLE_TILE) for m in out_lens)))
            if kind == 'float32':                                             # what was timed is the definition
                ref = cpu_conv(waves, orig, new)
                got = y.cpu()
                res['max_err_vs_cpu_conv'] = max(float((got[a0:a0 + m] - ref[b, :m]).abs().max()) for b, (a0, m) in enumerate(zip(out_off, out_lens)))
            out['%d_%d_%s' % (orig, new, kind)] = res
    print('GPU_STEP ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--window', type=int, default=50, help='launches between the two events of a round')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cpu-rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--step', default=None, choices=('gpu',), help='(internal: the child process of the GPU step)')
    a = ap.parse_args()
    if a.step == 'gpu':
        return gpu_step(a)
    cmd = ['timeout', '-k', '10', str(GPU_STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--step', 'gpu', '--batch-size', str(a.batch_size),
           '--seconds', str(a.seconds), '--rounds', str(a.rounds), '--window', str(a.window), '--warmup', str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('GPU_STEP ')]
    if r.returncode != 0 or not line:
        sys.stdout.write(r.stdout)
        raise SystemExit('bench_resample: the GPU step ended with status %d; nothing further was started' % r.returncode)
    res = dict(tool='bench_resample', batch=a.batch_size, seconds=a.seconds, rounds=a.rounds, window=a.window, tile=None,
               assumptions='HBM %.1f TB/s peak, %.1f TB/s float4 copy; time per launch includes the launch; bytes: input once + output once'
               % (HBM_PEAK_BPS / 1e12, HBM_COPY_BPS / 1e12))
    res.update(json.loads(line[0][9:]))
    from semi_tts_amd import ops
    res['tile'] = ops.RESAMPLE_TILE
    torch.set_num_threads(16)
    for orig, new in CASES:
        waves = make_batch(a.batch_size, a.seconds, orig)
        kern = full_kernel(orig, new)
        cpu_conv(waves, orig, new, kern)
        t = []
        for _ in range(a.cpu_rounds):
            t0 = time.perf_counter()
            cpu_conv(waves, orig, new, kern)
            t.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(t))
        res['%d_%d_cpu_conv1d' % (orig, new)] = dict(ms=round(ms, 2), ms_min=round(min(t), 2), threads=torch.get_num_threads(),
                                                    taps_per_phase=int(kern[0].shape[2]))
        for kind in ('float32', 'int16'):
            res['%d_%d_%s' % (orig, new, kind)]['cpu_over_gpu'] = round(ms * 1e3 / res['%d_%d_%s' % (orig, new, kind)]['us'], 1)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
