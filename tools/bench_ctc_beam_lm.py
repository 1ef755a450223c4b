#!/usr/bin/env python3
"""What n-gram fusion costs the CTC prefix beam search (st_ctc_beam_search_lm against st_ctc_beam_search) at the C2 shape after the
stride-2 encoder, B = 32, T = 129, V = 43, at W in {1, 16, 128}: the unfused call, order 2 and order 3.  (The kernel reads the table through
L2; a variant that copied the live rows into LDS once a frame was measured with this tool before it was removed:
profiles/bench_ctc_beam_lm_with_lds_staging.json)
The method of tools/bench_ctc_align.py: windows of back-to-back calls between two synchronises -- pipelined time per call, not one
call's latency --, the sides taking turns in one process, medians and the spread over the windows.  A call is ops.ctc_beam_search
as a user calls it: the allocation of its outputs and workspace is inside the window, the same on every side.  Prints one JSON line and writes it
to --out (default profiles/bench_ctc_beam_lm.json).

    python tools/bench_ctc_beam_lm.py [--calls 200] [--windows 5] [--widths 1 16 128]
    python tools/bench_ctc_beam_lm.py --trace-only       # a short run of the kernels alone, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

SHAPE = dict(B=32, T=129, V=43)


def softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def inputs(temp=1.0, seed=7):
    """the tests' generator: half the frames peak on the blank, the rest on a random symbol"""
    rs = np.random.RandomState(seed)
    B, T, V = SHAPE['B'], SHAPE['T'], SHAPE['V']
    tgt = np.where(rs.rand(B, T) < 0.5, 0, rs.randint(1, V, (B, T)))
    return softmax((rs.randn(B, T, V) + 6.0 * np.eye(V)[tgt]) / temp)


def table(order, seed=11):
    """the tests' table: a softmax of seeded noise, fused with weight 0.8 and bonus 0.3"""
    from semi_tts_amd import ngram
    V = SHAPE['V']
    return ngram.fusion_table(softmax(np.random.RandomState(seed).randn(V ** (order - 1), V) * 1.5), 0.8, 0.3)


def window(fn, calls):
    """us per call of `calls` back-to-back calls between two synchronises"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def alternate(sides, calls, windows, warmup=5):
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
    med = float(np.median(xs))
    return dict(median_us=round(med, 2), min_us=min(xs), max_us=max(xs), spread_pct=round((max(xs) - min(xs)) / med * 100.0, 2), windows=xs)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200, help='calls per timed window at W <= 16 (>= 100); a wider beam takes calls * 16 / W, at least 30: a W = 128 call costs about five '
                    'W = 16 calls, so every window stays above 0.15 s')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--widths', type=int, nargs='+', default=[1, 16, 128])
    ap.add_argument('--trace-only', action='store_true', help='10 calls of each side and nothing else (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_ctc_beam_lm.json'))
    a = ap.parse_args(argv)
    if a.calls < 100 and not a.trace_only:
        ap.error('--calls must be >= 100: a window shorter than about 0.1 s measures the clock')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_ctc_beam_lm: no GPU (there is no CPU timing of the kernels)')
    from semi_tts_amd import ops
    dev = torch.device('cuda:0')
    pd = torch.from_numpy(inputs()).to(dev)
    tables = {order: torch.from_numpy(table(order)).to(dev) for order in (2, 3)}

    res = {'shape': SHAPE, 'timed': 'ops.ctc_beam_search per call, output and workspace allocation included (the same on every side)',
           'temperature': 1.0, 'top_paths': 1, 'windows': a.windows, 'us_per_call': {}, 'fused_over_unfused': {}}
    for W in a.widths:
        sides = {
            'unfused': (lambda W=W: ops.ctc_beam_search(pd, None, W, 1)),
            'order2': (lambda W=W: ops.ctc_beam_search(pd, None, W, 1, bonus=tables[2])),
            'order3': (lambda W=W: ops.ctc_beam_search(pd, None, W, 1, bonus=tables[3])),
        }
        if a.trace_only:
            for fn in sides.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            continue
        calls = max(30, a.calls if W <= 16 else a.calls * 16 // W)         # a W = 128 call is about five W = 16 calls
        got = {k: summary(v) for k, v in alternate(sides, calls, a.windows).items()}
        res['us_per_call']['W%d' % W] = dict(got, calls_per_window=calls)
        base = got['unfused']['median_us']
        res['fused_over_unfused']['W%d' % W] = {k: round(v['median_us'] / base, 4) for k, v in got.items() if k != 'unfused'}
    if a.trace_only:
        return None
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
