#!/usr/bin/env python3
"""End-of-speech detection on a batch of decoder alignments (st_attn_endpoint, semi_tts_amd.metrics.attention_endpoints): B = 32
utterances, S = 100 decoder steps, L = 60 phones -- about one C2 batch.  Device time per call from events around windows of
back-to-back calls of the Python function (argument checks and the output allocation included) and of the C entry alone, beside two
ways of doing without the kernel, both checked equal to the kernel's integers first:
  torch + host   max over L on the device (torch.max), one .cpu() of peaks and weights, the run search and the counts in a host loop
                 (host clock around the whole thing: it ends in the copy's synchronise)
  numpy          the float64 oracle of the tests (tests/attn_endpoint_oracle.py) over the 32 utterances on up to 16 CPU processes
and the bytes the kernel has to read against the time HBM would take to deliver them.  The kernel is barrier- and latency-bound: one
workgroup per utterance, a few dependent load -> shuffle chains per wave and six barriers; the byte floor is printed to show how far
from a bandwidth problem it is, not as a target.  Prints one JSON line and writes it to profiles/bench_attn_endpoint.json (--out).

    python tools/bench_attn_endpoint.py [--calls 500] [--windows 5] [--out FILE]
    python tools/bench_attn_endpoint.py --cpu-only      # the numpy timing alone (needs no GPU; the device fields read "not measured")
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np   # noqa: E402

B, S, L, PATIENCE, MAX_JUMP = 32, 100, 60, 3, 4
CPU_PROCS = 16
HBM_PEAK_BPS = 8.0e12            # HBM3E, specification
INT_FIELDS = ('end', 'reached', 'n_back', 'n_skip', 'covered', 'nonfinite')


def inputs(seed=0):
    """align (B, S, L) float32 and the phone counts: 30 .. 59 phones of 1 .. 3 steps each, a softmax-like row around the peak, so most
    utterances end well inside the S steps and a few do not"""
    import attn_endpoint_oracle as O
    rs = np.random.RandomState(seed)
    ns = rs.randint(30, L, B)
    a = np.zeros((B, S, L), np.float32)
    for b in range(B):
        durs = rs.randint(1, 4, ns[b]).tolist()
        cols = [j for j, d in enumerate(durs) for _ in range(d)][:S]
        cols += [ns[b] - 1 + (k % 2) for k in range(S - len(cols))]         # the last phone and the token behind it, in turn
        a[b] = O.from_peaks(cols, L, rs, peak_w=0.6)
    return a, ns.astype(np.int32)


def _one(args):
    import attn_endpoint_oracle as O
    r = O.endpoint(args[0], args[1], PATIENCE, MAX_JUMP)
    return [int(getattr(r, k)) for k in INT_FIELDS]


def cpu_ms(a, ns, repeats=3):
    """wall time of the numpy oracle over the B utterances on CPU_PROCS processes (the pool is up before the clock starts)"""
    jobs = [(a[b], int(ns[b])) for b in range(B)]
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, jobs)
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, jobs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, np.array(res, np.int32)


def torch_host(ad, ns):
    """the composition a caller without the kernel would write -> (B, 6) integers"""
    w, p = ad.max(dim=-1)
    nonfinite = (~np.isfinite(ad.sum(dim=(1, 2)).cpu().numpy())).astype(np.int32)
    peak, w = p.cpu().numpy(), w.cpu().numpy()
    out = np.zeros((B, 6), np.int32)
    for b in range(B):
        flag = peak[b] >= ns[b] - 1
        end, reached, run = S, 0, 0
        for t in range(S):
            run = run + 1 if flag[t] else 0
            if run >= PATIENCE:
                end, reached = t + 1, 1
                break
        d = np.diff(peak[b, :end])
        cov = np.unique(peak[b, :end])
        out[b] = (end, reached, int((d < 0).sum()), int((d > MAX_JUMP).sum()), int((cov < ns[b]).sum()), nonfinite[b])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=500, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the numpy timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_attn_endpoint.json'))
    a = ap.parse_args(argv)
    x, ns = inputs()
    ms, procs, cpu = cpu_ms(x, ns)                    # (before the GPU is opened: the workers are forked from a process without one)
    nbytes = B * S * L * 4 + B * 4 + B * (6 + 1 + S + L) * 4
    res = {'shape': dict(B=B, S=S, L=L, patience=PATIENCE, max_jump=MAX_JUMP, phones=[int(ns.min()), int(ns.max())]),
           'reached': int(cpu[:, 1].sum()), 'end_steps': [int(cpu[:, 0].min()), int(cpu[:, 0].max())],
           'bound': 'barrier- and latency-bound (one workgroup per utterance, six barriers); the byte floor is not a target',
           'bytes_read_and_written': nbytes, 'hbm_floor_us': round(nbytes / HBM_PEAK_BPS * 1e6, 4),
           'numpy_float64_ms_per_batch': round(ms, 2), 'numpy_processes': procs,
           'device_us_per_batch': 'not measured', 'launch_alone_us': 'not measured', 'torch_host_us_per_batch': 'not measured', 'torch_host_over_device': 'not measured',
           'numpy_over_device': 'not measured', 'device_over_hbm_floor': 'not measured'}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_attn_endpoint: no GPU (--cpu-only times the numpy form alone)')
        from semi_tts_amd.metrics import attention_endpoints
        dev = torch.device('cuda:0')
        ad, nd = torch.from_numpy(x).to(dev), torch.from_numpy(ns).to(dev)
        ep = attention_endpoints(ad, nd, PATIENCE, MAX_JUMP)
        got = np.stack([getattr(ep, k).cpu().numpy() for k in INT_FIELDS], 1)
        if not np.array_equal(got, cpu):
            raise SystemExit('bench_attn_endpoint: the device integers differ from the numpy oracle')
        if not np.array_equal(torch_host(ad, ns), got):
            raise SystemExit('bench_attn_endpoint: the torch + host composition differs from the kernel')
        res['integers_equal'] = True
        for _ in range(20):
            attention_endpoints(ad, nd, PATIENCE, MAX_JUMP)
        out = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                attention_endpoints(ad, nd, PATIENCE, MAX_JUMP)
            e1.record()
            e1.synchronize()
            out.append(round(e0.elapsed_time(e1) / a.calls * 1e3, 2))
        res['calls_per_window'] = a.calls
        res['device_us_per_batch'] = dict(median_us=round(float(np.median(out)), 2), min_us=min(out), max_us=max(out), windows=out)
        # the launch alone: the C entry on outputs allocated once (no argument checks, no allocation: what a captured graph would replay)
        from semi_tts_amd import _lib, ops
        lib, stream = _lib.load(), ops.stream_handle()
        st_, fo, pk, du = (t.clone() for t in ops.attn_endpoint(ad, nd, PATIENCE, MAX_JUMP))
        args = (ad.data_ptr(), ad.stride(0), ad.stride(1), nd.data_ptr(), B, S, L, PATIENCE, MAX_JUMP, st_.data_ptr(), fo.data_ptr(),
                pk.data_ptr(), du.data_ptr(), stream)
        raw = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                lib.st_attn_endpoint(*args)
            e1.record()
            e1.synchronize()
            raw.append(round(e0.elapsed_time(e1) / a.calls * 1e3, 2))
        res['launch_alone_us'] = dict(median_us=round(float(np.median(raw)), 2), min_us=min(raw), max_us=max(raw), windows=raw)
        for _ in range(5):
            torch_host(ad, ns)
        th = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                torch_host(ad, ns)
            th.append(round((time.perf_counter() - t0) / 20 * 1e6, 1))
        res['torch_host_us_per_batch'] = dict(median_us=float(np.median(th)), min_us=min(th), max_us=max(th), windows=th)
        med = res['device_us_per_batch']['median_us']
        res['torch_host_over_device'] = round(res['torch_host_us_per_batch']['median_us'] / med, 1)
        res['numpy_over_device'] = round(ms * 1e3 / med, 1)
        res['device_over_hbm_floor'] = round(med / (nbytes / HBM_PEAK_BPS * 1e6), 1)
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
