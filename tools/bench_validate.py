#!/usr/bin/env python3
"""Validation (VqvaeTrainer.validate) and its PER kernel (st_ctc_greedy_edit_distance).  One JSON line:

- `kernel`: the greedy CTC transcript + edit distance of one batch at the C2 dev shape (B = 32, T' = 129, V = 43, L = 43) and at the
  long-form shape (B = 64, T' = 533, V = 43, L = 171): us per launch (CUDA events), against the CPU form of the reference's cal_per
  (argmax on the device, .cpu(), the pure-Python collapse and DP of tests/per_oracle.py) with its host read.
- `validate`: one validate() over K C2 dev batches (32 x 258 frames, single-speaker config) in ms, and the same work split into
  speech_to_text, free-running TTS (+ freq_loss), PER and the final host read, each phase synchronised apart.

    python tools/bench_validate.py [--dev-batches 4 --steps 50 --warmup 5 --no-validate]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np   # noqa: E402
import torch         # noqa: E402


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


def wall(fn, steps):
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def bench_kernel(dev, B, T, V, L, steps, warmup):
    import per_oracle as O
    from semi_tts_amd import ops
    from semi_tts_amd.metrics import IGNORE_INDICES
    rs = np.random.RandomState(B + T)
    prob = torch.from_numpy(rs.dirichlet(np.ones(V) * 0.3, (B, T)).astype(np.float32)).to(dev)
    text = torch.from_numpy(rs.randint(3, V, (B, L))).to(dev)
    text[:, -1] = 0
    med, best = timed(lambda: ops.ctc_greedy_edit_distance(prob, text, IGNORE_INDICES), steps, warmup)
    # the reference's form: argmax on the device, to the host, Python per utterance
    cpu = lambda: O.batch(prob.argmax(dim=-1).cpu().tolist(), text.cpu().tolist(), IGNORE_INDICES)
    cpu_us = wall(cpu, max(3, steps // 10))
    d, n = ops.ctc_greedy_edit_distance(prob, text, IGNORE_INDICES)
    od, on, _ = cpu()
    assert d.cpu().tolist() == od and n.cpu().tolist() == on
    return dict(B=B, T=T, V=V, L=L, us=round(med, 2), us_min=round(best, 2), cpu_python_us=round(cpu_us, 1),
                speedup=round(cpu_us / med, 1))


def bench_validate(dev, K, steps):
    import yaml
    from semi_tts_amd.solver import VqvaeTrainer
    from semi_tts_amd.metrics import per_sum
    config = yaml.safe_load(open(os.path.join(ROOT, 'config', 'semi-single-spkr-paired-data.yaml')))
    scratch = tempfile.mkdtemp(prefix='bench_validate_')      # (nothing is written there: see best_per below)
    paras = types.SimpleNamespace(name='bench', logdir=scratch, ckpdir=scratch, load=None,
                                  seed=0, cpu=False, verbose=False, batch_size=32, frames=256, n_batches=1, dev_batches=K,
                                  valid_step=None, max_step=1, store_best_per=True)
    tr = VqvaeTrainer(config, paras, 'train')
    tr.load_data()
    tr.set_model()
    tr.best_per = -1.0                            # (nothing beats it: no checkpoint is written while timing)
    tr.validate()                                 # warm-up: device copies of the dev set, first-call set-up
    total = wall(tr.validate, steps)
    batches = [tr.fetch_data('dev_iter') for _ in range(K)]
    m = tr.model.eval()
    phase = {'speech_to_text': 0.0, 'tts': 0.0, 'per': 0.0, 'host_read': 0.0}
    with torch.no_grad():
        for _ in range(steps):
            pers = []
            for mel, _, linear, text, sid in batches:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pp = m.speech_to_text(paired_mel=mel, unpaired_mel=None)[0]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                pers.append(per_sum(pp, text))
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                mp, lp = m.text_to_speech(text, sid, None, None, None, None, mel.shape[1], None, tf_rate=0.0)[:2]
                loss = tr.freq_loss(mp, mel) + tr.freq_loss(lp, linear)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                phase['speech_to_text'] += t1 - t0
                phase['per'] += t2 - t1
                phase['tts'] += t3 - t2
            t0 = time.perf_counter()
            torch.stack(pers + [loss.double()]).tolist()
            phase['host_read'] += time.perf_counter() - t0
    m.train()
    shutil.rmtree(scratch, ignore_errors=True)
    return dict(dev_batches=K, B=32, frames=258, validate_ms=round(total / 1e3, 2),
                split_ms={k: round(v * 1e3 / steps, 3) for k, v in phase.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dev-batches', type=int, default=4)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--validate-steps', type=int, default=5)
    ap.add_argument('--no-validate', action='store_true', help='the kernel alone')
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    out = dict(kernel=[bench_kernel(dev, 32, 129, 43, 43, a.steps, a.warmup), bench_kernel(dev, 64, 533, 43, 171, a.steps, a.warmup)])
    if not a.no_validate:
        out['validate'] = bench_validate(dev, a.dev_batches, a.validate_steps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
