#!/usr/bin/env python3
"""Transcript scoring of a corpus-like batch (st_edit_align, semi_tts_amd.metrics.align_transcripts): B = 32 utterances of 40 ... 100
phones a side over V = 43 classes, the hypothesis made from the reference by about 15 % substitutions, deletions and insertions, with
N = 1 and N = 8 paths per utterance.  Device time per call from events around windows of back-to-back calls (median / min / max of
the windows) for the Python entry (ops.edit_align with `ali` and the confusion matrix) and for the C entry alone on buffers made once,
beside st_hyp_edit_distance on the same pairs (the distance alone: the ratio is what the trace-back, `ali` and the confusion matrix
cost), beside the integer oracle of the tests (tests/edit_align_oracle.py) over the same pairs on up to 16 CPU processes, and beside
the byte floor (every token read once, every output written once, over the 6.29 TB/s a device copy reaches on this card).  The device
results are compared with the oracle's before anything is timed.  A sweep over the length (1 ... 400 phones, N = 1) separates the fixed
part of a call from the cost per phone.  Prints one JSON line and writes it to
profiles/bench_edit_align.json (--out).

    python tools/bench_edit_align.py [--calls 2000] [--windows 5] [--out FILE]
    python tools/bench_edit_align.py --cpu-only          # the oracle's timing alone (needs no GPU; the device fields read "not measured")
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

B, V, RATE, LO, HI = 32, 43, 0.15, 40, 100
IGNORE = (0, 1, 2)
CPU_PROCS = 16
SWEEP = (1, 25, 50, 100, 200, 400)
COPY_BYTES_PER_S = 6.29e12      # measured device-to-device copy rate of the card


def inputs(N, seed=0):
    """hyp (B, N, Lh), hyp_len (B, N), ref (B, Lr), ref_len (B,): references of LO .. HI phones (ids 3 .. V - 1), every path its own
    edit of the reference"""
    import edit_align_oracle as O
    rs = np.random.RandomState(seed)
    refs, hyps = [], []
    for b in range(B):
        n = HI if b == 0 else int(rs.randint(LO, HI + 1))
        ref = rs.randint(3, V, size=n).tolist()
        paths = []
        for _ in range(N):
            rs2 = np.random.RandomState(rs.randint(1 << 30))
            hyp = []
            for x in ref:
                u = rs2.rand()
                if u < RATE / 3:
                    continue
                hyp.append(int(rs2.randint(3, V)) if u < 2 * RATE / 3 else x)
                if u > 1 - RATE / 3:
                    hyp.append(int(rs2.randint(3, V)))
            paths.append(hyp)
        refs.append(ref)
        hyps.append(paths)
    Lr, Lh = max(len(r) for r in refs), max(len(t) for p in hyps for t in p)
    hyp = np.stack([O.pad(p, Lh) for p in hyps])
    return hyp, np.asarray([[len(t) for t in p] for p in hyps], np.int32), O.pad(refs, Lr), np.asarray([len(r) for r in refs], np.int32)


def _one(args):
    import edit_align_oracle as O
    ref, hyp = args
    counts, pairs = O.align(ref, hyp, IGNORE)
    return counts, len(pairs)


def cpu_ms(hyp, hyp_len, ref, ref_len, repeats=3):
    """wall time of the oracle's table and trace-back over the B N pairs on CPU_PROCS processes (the pool is up before the clock starts)"""
    N = hyp.shape[1]
    jobs = [(ref[b, :ref_len[b]].tolist(), hyp[b, k, :hyp_len[b, k]].tolist()) for b in range(B) for k in range(N)]
    procs = min(CPU_PROCS, os.cpu_count() or 1)
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, jobs)
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = pool.map(_one, jobs, chunksize=1)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), procs, res


def byte_floor_us(N, Lr, Lh):
    read = 8 * B * (N * Lh + Lr) + 4 * B * (N + 1)
    written = 4 * B * N * (5 + 2 * (Lr + Lh))
    return (read + written) / COPY_BYTES_PER_S * 1e6


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=2000, help='calls per timed window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--cpu-only', action='store_true', help='the oracle timing alone (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_edit_align.json'))
    a = ap.parse_args(argv)
    nm = 'not measured'
    data = {N: inputs(N) for N in (1, 8)}
    cpu = {N: cpu_ms(*data[N]) for N in data}             # (before the GPU is opened: the workers are forked from a process without one)
    res = {'shape': dict(B=B, phones=[LO, HI], V=V, edit_rate=RATE, ignore=list(IGNORE)), 'copy_bytes_per_s_assumed': COPY_BYTES_PER_S,
           'calls_per_window': a.calls}
    for N in data:
        hyp, hyp_len, ref, ref_len = data[N]
        res['N%d' % N] = {'Lr': int(ref.shape[1]), 'Lh': int(hyp.shape[2]), 'oracle_ms_per_batch': round(cpu[N][0], 2), 'oracle_processes': cpu[N][1],
                          'byte_floor_us': round(byte_floor_us(N, ref.shape[1], hyp.shape[2]), 3), 'edit_align_us': nm,
                          'edit_align_c_entry_us': nm, 'hyp_edit_distance_c_entry_us': nm, 'edit_align_over_hyp_edit_distance': nm,
                          'oracle_over_device': nm, 'device_over_byte_floor': nm}
    if not a.cpu_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_edit_align: no GPU (--cpu-only times the oracle alone)')
        import edit_align_oracle as O
        from semi_tts_amd import _lib, ops
        lib = _lib.load()
        dev = torch.device('cuda:0')
        stream = ops.stream_handle()

        def windows(fn):
            for _ in range(50):
                fn()
            out = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                out.append(round(e0.elapsed_time(e1) / a.calls * 1e3, 2))
            return dict(median_us=round(float(np.median(out)), 2), min_us=min(out), max_us=max(out), windows=out)
        for N in data:
            hyp, hyp_len, ref, ref_len = data[N]
            Lr, Lh = ref.shape[1], hyp.shape[2]
            hd, hl = torch.from_numpy(hyp).to(dev), torch.from_numpy(hyp_len).to(dev)
            rd, rl = torch.from_numpy(ref).to(dev), torch.from_numpy(ref_len).to(dev)
            conf = torch.zeros(V + 1, V + 1, dtype=torch.int32, device=dev)
            counts, ali_len, _, _ = ops.edit_align(hd, hl, rd, rl, IGNORE, V, conf)
            counts, ali_len = counts.cpu().numpy().reshape(B * N, 4), ali_len.cpu().numpy().reshape(B * N)
            bad = sum(tuple(counts[p]) != tuple(cpu[N][2][p][0]) or int(ali_len[p]) != cpu[N][2][p][1] for p in range(B * N))
            if bad:
                raise SystemExit('bench_edit_align: %d of %d pairs differ from the oracle' % (bad, B * N))
            r = res['N%d' % N]
            r['pairs_equal_to_oracle'] = B * N
            r['edit_align_us'] = windows(lambda: ops.edit_align(hd, hl, rd, rl, IGNORE, V, conf))
            # the C entries alone, on buffers made once (references repeated per path for the distance kernel, which takes one hypothesis a row)
            ign = torch.tensor(IGNORE, dtype=torch.int32).to(dev)
            out = torch.empty(B * N * (5 + 2 * (Lr + Lh)), dtype=torch.int32, device=dev)
            p_counts, p_len, p_ali = out.data_ptr(), out.data_ptr() + 16 * B * N, out.data_ptr() + 20 * B * N
            r['edit_align_c_entry_us'] = windows(lambda: lib.st_edit_align(hd.data_ptr(), hl.data_ptr(), B, N, Lh, rd.data_ptr(), rl.data_ptr(), Lr,
                                                                           ign.data_ptr(), len(IGNORE), V, p_counts, p_len, p_ali, conf.data_ptr(),
                                                                           None, stream))
            r['edit_align_c_entry_no_ali_no_confusion_us'] = windows(lambda: lib.st_edit_align(
                hd.data_ptr(), hl.data_ptr(), B, N, Lh, rd.data_ptr(), rl.data_ptr(), Lr, ign.data_ptr(), len(IGNORE), V, p_counts, p_len, None, None,
                None, stream))
            flat_h, flat_l = hd.reshape(B * N, Lh), hl.reshape(B * N)
            rep = torch.where(torch.arange(Lr, device=dev)[None] < rl[:, None], rd, torch.zeros_like(rd)).repeat_interleave(N, dim=0).contiguous()
            dist = torch.empty(2 * B * N, dtype=torch.int32, device=dev)
            r['hyp_edit_distance_c_entry_us'] = windows(lambda: lib.st_hyp_edit_distance(flat_h.data_ptr(), flat_l.data_ptr(), B * N, Lh, rep.data_ptr(),
                                                                                         Lr, ign.data_ptr(), len(IGNORE), dist.data_ptr(),
                                                                                         dist.data_ptr() + 4 * B * N, stream))
            torch.cuda.synchronize()
            if not np.array_equal(dist[:B * N].cpu().numpy(), counts[:, 1:].sum(axis=1)):
                raise SystemExit('bench_edit_align: the distances differ from st_hyp_edit_distance')
            us = r['edit_align_c_entry_us']['median_us']
            r['edit_align_over_hyp_edit_distance'] = round(us / r['hyp_edit_distance_c_entry_us']['median_us'], 2)
            r['oracle_over_device'] = round(r['oracle_ms_per_batch'] * 1e3 / us, 1)
            r['device_over_byte_floor'] = round(us / r['byte_floor_us'], 1)
        # what a call costs at other lengths (N = 1, every reference exactly L phones): the fixed part and the slope per phone
        sweep = {}
        for L in SWEEP:
            rs = np.random.RandomState(L)
            pairs = [O.edited_pair(rs, L, V - 3, RATE) for _ in range(B)]
            Lh = max(1, max(len(h) for _, h in pairs))
            hd = torch.from_numpy(O.pad([h for _, h in pairs], Lh)).to(dev).view(B, 1, Lh)
            hl = torch.tensor([[len(h)] for _, h in pairs], dtype=torch.int32).to(dev)
            rd = torch.from_numpy(O.pad([r for r, _ in pairs], L)).to(dev)
            conf = torch.zeros(V + 1, V + 1, dtype=torch.int32, device=dev)
            sweep[str(L)] = windows(lambda: ops.edit_align(hd, hl, rd, None, IGNORE, V, conf))['median_us']
        res['N1_us_by_phones'] = sweep
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
