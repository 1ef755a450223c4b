#!/usr/bin/env python3
"""Mel vocoding and ragged batches (st_mel_to_linear, st_griffin_lim_batch) at the C2 shape: 32 utterances x 258 frames, n_fft 2048 /
hop 275 / win 1102, 80 mels, 30 iterations, denormalisation + inverse pre-emphasis + clip included.  One JSON line:

  mel_to_linear     the product alone: ms, its bytes (mel in, basis once, output out) and the fraction of the HBM floor of those bytes
  gl_from_mel / gl_from_linear     Griffin-Lim through st_griffin_lim_batch from each input kind
  batch_uniform / griffin_lim      ops.griffin_lim_batch(frames=None, basis=None) against ops.griffin_lim.  The two are ONE routine since the
                    uniform entry point st_griffin_lim was removed (ops.griffin_lim calls griffin_lim_batch): the row times one code
                    path twice and is kept so that the figures under profiles/ stay comparable
  ragged / ragged_as_singles / ragged_as_uniform     32 lengths spread evenly over 129 .. 258 frames in one ragged call, as 32
                    single calls of ops.griffin_lim, and as the uniform T = 258 batch (which vocodes the padding too)

Every variant is warmed up, then the variants are timed in turn, round after round (device events around each call), so drift of
the machine falls on all of them alike; per variant: the median, the minimum and the spread (max - min) / median over the rounds.

    python tools/bench_vocode.py [--batch-size 32 --frames 258 --iters 30 --rounds 20 --warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

N_FFT, HOP, WIN, SR, N_MELS = 2048, 275, 1102, 22050, 80
HBM_PEAK_BPS = 8.0e12            # HBM3E, specification
HBM_COPY_BPS = 6.3e12            # what a float4 copy reaches


def ragged_lengths(B, T):
    """B frame counts spread evenly over T // 2 .. T, longest first"""
    return [int(round(v)) for v in np.linspace(T, T // 2, B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--frames', type=int, default=258)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    from semi_tts_amd import ops
    from semi_tts_amd.audio import draw_phases, mel_basis
    if not torch.cuda.is_available():
        raise SystemExit('bench_vocode: needs a GPU (a CPU run measures nothing)')
    B, T = a.batch_size, a.frames
    F = N_FFT // 2 + 1
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    # a smooth normalised mel / linear pair of decoder-like range (the values do not change what the kernels do)
    mel = torch.from_numpy((0.55 + 0.3 * np.sin(np.linspace(0, 6, N_MELS))[None, None] * np.cos(np.linspace(0, 9, T))[None, :, None]
                            + 0.03 * rs.randn(B, T, N_MELS)).astype(np.float32)).to(dev)
    lin = torch.from_numpy((0.5 + 0.3 * np.sin(np.linspace(0, 40, F))[None, None] * np.cos(np.linspace(0, 9, T))[None, :, None]
                            + 0.03 * rs.randn(B, T, F)).astype(np.float32)).to(dev)
    np.random.seed(0)
    ph = torch.from_numpy(draw_phases((B, F, T))).to(dev)
    basis = torch.from_numpy(mel_basis(SR, N_FFT, N_MELS)).to(dev)
    lens = ragged_lengths(B, T)
    frames = torch.tensor(lens, dtype=torch.int32, device=dev)
    singles = [(lin[b:b + 1, :n].contiguous(), ph[b:b + 1, :, :n].contiguous()) for b, n in enumerate(lens)]
    post = ops.GL_INV_PREEMPHASIS | ops.GL_CLIP
    kw = dict(n_iter=a.iters, normalized=True, post=post)
    variants = {
        'mel_to_linear': lambda: ops.mel_to_linear(mel, basis, normalized=True, take_abs=True),
        'gl_from_mel': lambda: ops.griffin_lim_batch(mel, ph, N_FFT, HOP, WIN, basis=basis, **kw),
        'gl_from_linear': lambda: ops.griffin_lim_batch(lin, ph, N_FFT, HOP, WIN, **kw),
        'griffin_lim': lambda: ops.griffin_lim(lin, ph, N_FFT, HOP, WIN, **kw),
        'ragged': lambda: ops.griffin_lim_batch(lin, ph, N_FFT, HOP, WIN, frames=frames, **kw),
        'ragged_from_mel': lambda: ops.griffin_lim_batch(mel, ph, N_FFT, HOP, WIN, basis=basis, frames=frames, **kw),
        'ragged_as_singles': lambda: [ops.griffin_lim(f, p, N_FFT, HOP, WIN, **kw) for f, p in singles],
    }
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))

    def stat(k):
        t = np.array(times[k])
        med = float(np.median(t))
        return dict(ms=round(med, 4), ms_min=round(float(t.min()), 4), spread=round(float((t.max() - t.min()) / med), 4))
    res = dict(tool='bench_vocode', batch=B, frames=T, n_fft=N_FFT, hop=HOP, win=WIN, n_mels=N_MELS, iters=a.iters, rounds=a.rounds,
               ragged_lengths=[lens[0], lens[-1]], ragged_frames_total=int(sum(lens)), uniform_frames_total=B * T)
    res.update({k: stat(k) for k in variants})
    # the uniform T batch is the 'gl_from_linear' call: it vocodes B * T frames where the ragged one vocodes sum(lens)
    res['ragged_as_uniform'] = res['gl_from_linear']
    nbytes = 4 * (B * T * N_MELS + N_MELS * F + B * T * F)
    m = res['mel_to_linear']
    m.update(bytes=nbytes, hbm_floor_ms=round(nbytes / HBM_PEAK_BPS * 1e3, 5), fraction_of_hbm_floor=round(nbytes / HBM_PEAK_BPS * 1e3 / m['ms'], 4),
             fraction_of_copy_rate=round(nbytes / HBM_COPY_BPS * 1e3 / m['ms'], 4), gflop=round(2 * B * T * N_MELS * F / 1e9, 3),
             assumptions='HBM %.1f TB/s peak, %.1f TB/s float4 copy; one launch, time includes the launch' % (HBM_PEAK_BPS / 1e12, HBM_COPY_BPS / 1e12))
    res['mel_minus_linear_ms'] = round(res['gl_from_mel']['ms'] - res['gl_from_linear']['ms'], 4)
    res['batch_uniform_minus_griffin_lim_ms'] = round(res['gl_from_linear']['ms'] - res['griffin_lim']['ms'], 4)
    res['ragged_vs_singles'] = round(res['ragged_as_singles']['ms'] / res['ragged']['ms'], 3)
    res['ragged_vs_uniform'] = round(res['gl_from_linear']['ms'] / res['ragged']['ms'], 3)
    # results must not change: the batch entry point without frames / basis is the uniform vocoder, the ragged rows are the singles
    res['batch_uniform_equals_griffin_lim'] = bool(torch.equal(variants['gl_from_linear'](), variants['griffin_lim']()))
    rag = variants['ragged']()
    res['ragged_rows_equal_singles'] = all(bool(torch.equal(rag[b, :HOP * (n - 1)], w[0]))
                                           for b, (n, w) in enumerate(zip(lens, variants['ragged_as_singles']())))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
