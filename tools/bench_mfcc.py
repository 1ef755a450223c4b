#!/usr/bin/env python3
"""MFCC extraction (semi_tts_amd.audio.extract_mfcc_batch, st_audio_mfcc) on a corpus-like batch: 32 utterances of about 3 s
(2.5 .. 3.5 s, ragged) at 22050 Hz, n_fft 2048, the MFCC framing 551 / 220.  One JSON line, also written to --out:

  us_per_batch   device events around a window of calls, after warm-up; median / min / spread over the rounds (two launches a call)
  stft_fwd       the same frames through ops.stft_fwd alone at that framing (the zero-padded (B, L_max) batch: complex output, no
                 epilogue) and the ratio of the two times per frame
  cpu_baseline   the same computation in torch fp32 (tests/feat_oracle.py at the MFCC framing) + scipy (dct, two savgol_filter calls)
                 per utterance on 16 CPU threads, and its ratio to the call
  max_err        the call against that CPU form, as a sanity check of what was timed

Without a GPU the tool refuses to run: a CPU run measures nothing.

    python tools/bench_mfcc.py [--batch-size 32 --seconds 3 --rounds 20 --window 20 --warmup 5 --no-cpu --out profiles/bench_mfcc.json]
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
             use_linear=True, snr_range=[-1, -1], time_stretch_range=[1.0, 1.0])


def timed(fn, rounds, window, warmup):
    """us per call: -> (median, min, (max - min) / median) over `rounds` windows of `window` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = []
    for _ in range(rounds):
        ev[0].record()
        for _ in range(window):
            fn()
        ev[1].record()
        ev[1].synchronize()
        t.append(ev[0].elapsed_time(ev[1]) * 1e3 / window)
    t = np.array(t)
    return float(np.median(t)), float(t.min()), float((t.max() - t.min()) / np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--window', type=int, default=20, help='calls between the two events of a round')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mfcc: needs a GPU (a CPU run measures nothing)')
    from semi_tts_amd import ops
    from semi_tts_amd.audio import WaveBatch, load_audio_transform, mel_filterbank
    conv = load_audio_transform(**AUDIO)
    B, sr, n_fft, win, hop = a.batch_size, conv.sr, conv.n_fft, conv.win_length_mfcc, conv.hop_length_mfcc
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    lens = [int(round(v * sr)) for v in np.linspace(a.seconds * 7 / 6, a.seconds * 5 / 6, B)]
    waves = [np.clip(0.3 * np.sin(2 * np.pi * 220 * np.arange(L) / sr + rs.rand()) + 0.1 * rs.randn(L), -1, 1).astype(np.float32) for L in lens]
    wb = WaveBatch([torch.from_numpy(w).to(dev) for w in waves])

    def run():
        return conv.extract_mfcc_batch(wb)
    us, us_min, spread = timed(run, a.rounds, a.window, a.warmup)
    r1, r2 = run(), run()
    frames = int(sum(1 + L // hop for L in lens))
    Lmax = max(lens)
    xpad = torch.zeros(B, Lmax, device=dev)
    for i, w in enumerate(waves):
        xpad[i, :len(w)] = torch.from_numpy(w)
    stft_us, _, stft_spread = timed(lambda: ops.stft_fwd(xpad, n_fft, hop, win), a.rounds, a.window, a.warmup)
    stft_frames = B * (1 + Lmax // hop)
    res = dict(tool='bench_mfcc', batch=B, seconds=a.seconds, sample_rate=sr, n_fft=n_fft, win=win, hop=hop, n_mels=conv.n_mels, n_mfcc=13,
               rounds=a.rounds, window=a.window, us_per_batch=round(us, 1), us_min=round(us_min, 1), spread=round(spread, 4), launches=2,
               frames=frames, ns_per_frame=round(us * 1e3 / frames, 2), audio_seconds_per_second=round(sum(lens) / sr / (us * 1e-6), 1),
               bitwise_repeatable=bool(torch.equal(r1, r2)),
               stft_fwd=dict(us=round(stft_us, 1), spread=round(stft_spread, 4), frames=stft_frames,
                             ns_per_frame=round(stft_us * 1e3 / stft_frames, 2),
                             what='ops.stft_fwd at the MFCC framing on the zero-padded (B, L_max) batch: complex output, no epilogue'),
               ratio_vs_stft_per_frame=round((us / frames) / (stft_us / stft_frames), 3))
    if not a.no_cpu:
        import scipy.fft
        import scipy.signal
        import feat_oracle as O
        torch.set_num_threads(16)
        fb = mel_filterbank(sr, n_fft, conv.n_mels)

        def cpu_one(x):
            _, mel = O.features(x, fb, n_fft=n_fft, hop=hop, win=win, dtype=torch.float32)
            c = scipy.fft.dct(mel.numpy(), axis=0, type=2, norm='ortho')[:13]
            return np.concatenate([c] + [scipy.signal.savgol_filter(c, 9, deriv=o, polyorder=o, axis=-1, mode='interp') for o in (1, 2)])
        cpu_one(waves[0])
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            refs = [cpu_one(x) for x in waves]
            t.append((time.perf_counter() - t0) * 1e6)
        cpu_us = float(np.median(t))
        got = r1.cpu().numpy()
        res['max_err_vs_cpu'] = max(float(np.abs(got[b, :r.shape[1]] - r.T).max()) for b, r in enumerate(refs))      # (lens are sorted already)
        res['cpu_baseline'] = dict(kind='torch fp32 stft + mel (tests/feat_oracle.py) and scipy dct / savgol_filter, per utterance, 16 threads',
                                   us=round(cpu_us, 1), us_min=round(min(t), 1))
        res['cpu_over_gpu'] = round(cpu_us / us, 1)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
