#!/usr/bin/env python3
"""Feature extraction (semi_tts_amd.audio.extract_batch, st_audio_features) on a C2-sized batch: 32 utterances with ragged
lengths around 258 frames (hop 275 at 22050 Hz), clean mel + linear and the augmented mel (noise from the built-in generator at a
drawn SNR, time-stretched framing).  One JSON line: us per batch, launches, the same clean frames through ops.stft_fwd alone (the
yardstick for the FFT part; its complex output, no epilogue), and the torch fp32 CPU form of the same work at 16 threads
(`cpu_baseline`).

    python tools/bench_features.py [--batch-size 32 --frames 258 --steps 50 --warmup 5 --no-cpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np   # noqa: E402
import torch         # noqa: E402

AUDIO = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
             use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(steps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--frames', type=int, default=258)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    import random
    from semi_tts_amd import ops
    from semi_tts_amd.audio import WaveBatch, load_audio_transform
    import feat_oracle as O
    conv = load_audio_transform(**AUDIO)
    B, hop, win, n_fft = a.batch_size, conv.hop_length, conv.win_length, conv.n_fft
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    lens = [int(hop * (a.frames - 1) * f) for f in rs.uniform(0.8, 1.2, B)]                   # ragged, ~258 frames on average
    wavs = [torch.from_numpy((0.3 * rs.randn(L)).astype(np.float32)).to(dev) for L in lens]
    wb = WaveBatch(wavs)
    random.seed(0)
    draws = [conv._draw() for _ in range(B)]
    snr, stretch = [d[0] for d in draws], [d[1] for d in draws]

    def run():
        return conv.extract_batch(wb, r=5, seed=1, snr=snr, stretch=stretch)
    us, us_min = timed(run, a.steps, a.warmup)
    r1, r2 = run(), run()
    repeatable = all(torch.equal(x, y) for x, y in zip(r1, r2))
    frames = int(sum(1 + L // hop for L in lens))
    aug_frames = int(sum(1 + L // conv.stretch_dims(s)[1] for L, s in zip(lens, stretch)))
    # the yardstick: the same clean frames through st_stft_fwd (one (B, L_max) batch: the padding frames are computed there too)
    Lmax = max(lens)
    xpad = torch.zeros(B, Lmax, device=dev)
    for i, w in enumerate(wavs):
        xpad[i, :w.numel()] = w
    stft_us, _ = timed(lambda: ops.stft_fwd(xpad, n_fft, hop, win), a.steps, a.warmup)
    stft_frames = B * (1 + Lmax // hop)
    res = dict(tool='bench_features', batch=B, mean_frames=round(frames / B, 1), n_fft=n_fft, hop=hop, win=win, n_mels=conv.n_mels,
               us_per_batch=round(us, 1), us_min=round(us_min, 1), launches=2, clean_frames=frames, aug_frames=aug_frames,
               ns_per_frame=round(us * 1e3 / (frames + aug_frames), 2), bitwise_repeatable=repeatable,
               stft_fwd=dict(us=round(stft_us, 1), frames=stft_frames, ns_per_frame=round(stft_us * 1e3 / stft_frames, 2),
                             what='ops.stft_fwd on the clean framing of the zero-padded (B, L_max) batch: complex output, no epilogue'),
               ratio_vs_stft_per_frame=round((us / (frames + aug_frames)) / (stft_us / stft_frames), 3),
               ratio_vs_stft_same_batch=round(us / stft_us, 3))
    if not a.no_cpu:
        torch.set_num_threads(16)
        from semi_tts_amd.audio import mel_filterbank
        fb = mel_filterbank(conv.sr, n_fft, conv.n_mels)
        xs = [w.cpu().numpy() for w in wavs]
        nz = [np.random.RandomState(i).randn(len(x)).astype(np.float32) for i, x in enumerate(xs)]
        t0 = time.perf_counter()
        for x, n, s, r in zip(xs, nz, snr, stretch):
            O.features(x, fb, dtype=torch.float32)
            aw, ah = conv.stretch_dims(r)
            O.features(x, fb, win=aw, hop=ah, noise=n, snr=s, dtype=torch.float32)
        cpu_us = (time.perf_counter() - t0) * 1e6
        res['cpu_baseline'] = dict(kind='torch fp32 CPU (tests/feat_oracle.py, per utterance as the reference loader), 16 threads',
                                   us=round(cpu_us, 1))
        res['speedup_vs_cpu_fp32'] = round(cpu_us / us, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
