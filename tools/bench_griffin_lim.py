#!/usr/bin/env python3
"""Griffin-Lim vocoder (semi_tts_amd.audio, st_griffin_lim_batch) on a C2 batch: 32 utterances x 258 frames of a normalised linear
spectrogram (n_fft 2048, hop 275, win 1102), 30 iterations, denormalisation + inverse pre-emphasis + clip included.  One JSON line:
ms per batch, audio seconds per second, launches, the estimated floors (`roofline`) from the kernels' byte counts, and the same
algorithm as torch CPU STFT / iSTFT on the same inputs (`cpu_baseline`, fp32, 16 threads; --cpu-fp64 adds the fp64 oracle).

    python tools/bench_griffin_lim.py [--batch-size 32 --frames 258 --iters 30 --steps 20 --warmup 3 --no-cpu]
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

N_FFT, HOP, WIN, SR = 2048, 275, 1102, 22050
LDS_READ_BPS = 150e12      # ds_read_b64, every CU streaming (MI355X_MICROARCH-style figures: DESIGN.md)
LDS_WRITE_BPS = 45e12      # ds_write_b32 / b64
L2_BPS = 22 * 256 * 2.4e9  # what the compute units take in from L2: ~22 B/clk per CU, 256 CUs at 2.4 GHz


def byte_counts(B, T, n_iter, n_fft=N_FFT, hop=HOP, win=WIN):
    """LDS and L2 bytes of the n_iter gl_iter_kernel launches (audio.hip), counted from what each workgroup reads and writes"""
    M = n_fft // 2
    stages = int(np.log2(M)) // 2 + (int(np.log2(M)) & 1)
    lds_w = 4 * n_fft + 2 * stages * 8 * M + 8 * M              # gather, 2 FFTs, the split / projection / merge pass
    lds_r = 2 * stages * 8 * M + 8 * M + 4 * win               # 2 FFTs, the split pass, the windowed output
    # overlap-add gather: every support sample of a frame reads each frame covering it (up to 5); plus envelope, window (twice),
    # magnitude row, frame written
    s = np.arange(win)[None, :] + (np.arange(T)[:, None] * hop)
    contrib = np.minimum(s // hop, T - 1) - np.maximum(0, -(-(s - win + 1) // hop)) + 1
    l2 = 4 * (contrib.mean() * win + win + 2 * win + (M + 1) + win)
    frames = B * T * n_iter
    return dict(lds_bytes=frames * (lds_w + lds_r), lds_ms=frames * (lds_w / LDS_WRITE_BPS + lds_r / LDS_READ_BPS) * 1e3,
                l2_bytes=frames * l2, l2_ms=frames * l2 / L2_BPS * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--frames', type=int, default=258)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-fp64', action='store_true')
    a = ap.parse_args()
    from semi_tts_amd import ops
    from semi_tts_amd.audio import draw_phases
    import gl_oracle as O
    B, T = a.batch_size, a.frames
    F, L = N_FFT // 2 + 1, HOP * (T - 1)
    dev = torch.device('cuda:0')
    # a normalised linear spectrogram of a harmonic signal (what the decoder's `lin` looks like), (B, T, F)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(L, dtype=torch.float64) / SR
    f0 = 100 + 150 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = sum(0.3 / (h + 1) * torch.sin(2 * np.pi * f0 * (h + 1) * t) for h in range(8)) + 0.01 * torch.randn(B, L, generator=g,
                                                                                                          dtype=torch.float64)
    amp = O.stft(x).abs()
    feat = torch.clamp((20 * torch.log10(torch.clamp(amp, min=1e-5)) - 20 + 100) / 100, 0, 1).float().transpose(1, 2).contiguous()
    np.random.seed(0)
    phases = torch.from_numpy(draw_phases((B, F, T)))
    feat_d, ph_d = feat.to(dev), phases.to(dev)
    post = ops.GL_INV_PREEMPHASIS | ops.GL_CLIP

    def run():
        return ops.griffin_lim(feat_d, ph_d, N_FFT, HOP, WIN, n_iter=a.iters, normalized=True, post=post)
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(a.steps):
        ev[0].record()
        run()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    ms = float(np.median(times))
    a1, a2 = run(), run()
    repeatable = bool(torch.equal(a1, a2))
    bc = byte_counts(B, T, a.iters)
    floor = max(bc['lds_ms'], bc['l2_ms'])
    res = dict(tool='bench_griffin_lim', batch=B, frames=T, n_fft=N_FFT, hop=HOP, win=WIN, iters=a.iters,
               ms_per_batch=round(ms, 4), ms_min=round(float(min(times)), 4), audio_seconds_per_second=round(B * L / SR / (ms / 1e3), 1),
               launches=a.iters + 3, bitwise_repeatable=repeatable,
               roofline=dict(lds_gb=round(bc['lds_bytes'] / 1e9, 2), lds_floor_ms=round(bc['lds_ms'], 3),
                             l2_gb=round(bc['l2_bytes'] / 1e9, 2), l2_floor_ms=round(bc['l2_ms'], 3), floor_ms=round(floor, 3),
                             fraction_of_floor=round(floor / ms, 3),
                             assumptions='LDS %.0f TB/s read, %.0f TB/s write; L2 -> CU %.1f TB/s' % (LDS_READ_BPS / 1e12,
                                                                                                    LDS_WRITE_BPS / 1e12, L2_BPS / 1e12)))
    if not a.no_cpu:
        torch.set_num_threads(16)
        base = {}
        for name, dt in [('fp32', torch.float32)] + ([('fp64', torch.float64)] if a.cpu_fp64 else []):
            mag = O.denormalize_to_amp(feat.to(dt).transpose(1, 2))
            t0 = time.perf_counter()
            wav = O.griffin_lim(mag, phases.to(dt), a.iters)
            np.clip(O.inv_preemphasis(wav.numpy()), -1, 1)
            base[name + '_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        res['cpu_baseline'] = dict(kind='torch CPU restatement of src/audio.py Griffin-Lim (tests/gl_oracle.py), 16 threads', **base)
        res['speedup_vs_cpu_fp32'] = round(base['fp32_ms'] / ms, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
