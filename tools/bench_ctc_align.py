#!/usr/bin/env python3
"""CTC forced alignment (st_ctc_forced_align) at the C2 shape after the stride-2 encoder (B = 32, T = 129, V = 43, up to 43 targets) and
at the long form (B = 64, T = 533, up to 171 targets): time per call of ctc_align.forced_align on probabilities and on log input; at C2
the yardstick ops.ctc_loss(prob, text, 1e-10, want_grad=False) -- the same trellis with a logsumexp per cell, both directions -- on the
same posteriors and targets, the two sides alternated window by window in one process; and the float64 oracle of the tests
(tests/ctc_align_oracle.py) on one CPU core over the same batch.  Prints one JSON line.

    python tools/bench_ctc_align.py [--calls 2000] [--windows 5] [--no-oracle]
    python tools/bench_ctc_align.py --trace-only       # a short run of the kernels alone, for rocprofv3 --kernel-trace --stats
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

SHAPES = {'c2': dict(B=32, T=129, V=43, L=43), 'long': dict(B=64, T=533, V=43, L=171)}


def inputs(name, temp=1.0, seed=0):
    """the tests' generator: posteriors peaked on a random monotone placement of random transcripts"""
    import ctc_align_oracle as O
    s = SHAPES[name]
    return O.peaked(np.random.RandomState(seed), s['B'], s['T'], s['V'], temp, s['L'])


def window(fn, calls):
    """us per call of `calls` back-to-back calls between two synchronises: pipelined time per call, not one call's latency"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def alternate(sides, calls, windows, warmup=20):
    """{name: [us per call of each window]}: every side warmed up, then `windows` rounds with the sides taking turns"""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            out[k].append(round(window(fn, calls), 2))
    return out


def summary(xs):
    return dict(median_us=round(float(np.median(xs)), 2), min_us=min(xs), max_us=max(xs), windows=xs)


def oracle_ms(name, prob, text, tl):
    import ctc_align_oracle as O
    lp = O.log_probs(prob)
    t0 = time.perf_counter()
    O.batch_align(None, text, None, tl, lp=lp)
    return round((time.perf_counter() - t0) * 1e3, 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=2000, help='calls per timed window (>= 200)')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-oracle', action='store_true', help='skip the CPU oracle timing')
    ap.add_argument('--trace-only', action='store_true', help='20 calls of each kernel and nothing else (for a kernel trace)')
    ap.add_argument('--oracle-only', action='store_true', help='the CPU oracle timing alone (needs no GPU)')
    a = ap.parse_args(argv)
    if a.calls < 200 and not (a.trace_only or a.oracle_only):
        ap.error('--calls must be >= 200: a shorter window measures the clock')
    data = {name: inputs(name) for name in SHAPES}
    res = {'shapes': SHAPES, 'calls_per_window': a.calls, 'temperature': 1.0}
    if a.oracle_only:
        res['oracle_float64_1core_ms'] = {name: oracle_ms(name, *data[name]) for name in SHAPES}
        print(json.dumps(res))
        return res
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_ctc_align: no GPU (there is no CPU timing of the kernels)')
    from semi_tts_amd import ops
    from semi_tts_amd.ctc_align import forced_align
    dev = torch.device('cuda:0')
    sides = {}
    for name, (prob, text, tl) in data.items():
        pd, td = torch.from_numpy(prob).to(dev), torch.from_numpy(text).to(dev)
        ld = torch.log(pd.double() + 1e-10).float()
        tld = torch.from_numpy(tl).to(dev)
        sides[name + '_align_prob'] = (lambda pd=pd, td=td, tld=tld: forced_align(pd, td, None, tld))
        sides[name + '_align_log'] = (lambda ld=ld, td=td, tld=tld: forced_align(ld, td, None, tld, log_input=True))
        if name == 'c2':         # st_ctc_loss takes transcripts of up to 127 tokens: the long form has no yardstick
            sides['c2_ctc_loss_nograd'] = (lambda pd=pd, td=td: ops.ctc_loss(pd, td, 1e-10, want_grad=False))
    if a.trace_only:
        for fn in sides.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        return None
    res['us_per_call'] = {k: summary(v) for k, v in alternate(sides, a.calls, a.windows).items()}
    res['c2_align_over_ctc_loss'] = round(res['us_per_call']['c2_align_prob']['median_us'] / res['us_per_call']['c2_ctc_loss_nograd']['median_us'], 3)
    if not a.no_oracle:
        res['oracle_float64_1core_ms'] = {name: oracle_ms(name, *data[name]) for name in SHAPES}
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
