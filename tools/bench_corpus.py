#!/usr/bin/env python3
"""What the corpus loader and the CTC frame counts cost.

  fetch     one paired fetch of a device-resident split (semi_tts_amd.corpus.DeviceSplit) at B = 32 of about 3 s utterances against
            AudioConverter.extract_batch on the same waves packed alone: the difference is the loader's own cost (sampler, window, the
            small text / sid upload).  The corpus is 64 seeded utterances written to a temporary directory.
  ctc       ops.ctc_loss (value and gradient) at B = 32, T = 129, V = 512, L = 43 with in_len=None and with lengths of 60 ... 100 % of T,
            and ops.frame_lengths on the matching (32, 258, 80) mel.
  parent    with --parent-lib FILE (libsemitts_hip.so built from the parent commit): its st_ctc_loss against this build's, same inputs,
            results compared bit for bit first, the two builds alternated window by window; the parent is timed as two sides, whose
            difference is the run-to-run spread the comparison is allowed.

Sides are alternated window by window in one process; a window is `--calls` back-to-back calls between two synchronises.  Prints one
JSON line and, with --out, writes it.

    python tools/bench_corpus.py [--calls 300] [--windows 5] [--parent-lib FILE] [--out profiles/bench_corpus.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

SR = 22050
CTC = dict(B=32, T=129, V=512, L=43)


def window(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def alternate(sides, calls, windows, warmup=10):
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


def write_corpus(root, n=64, seed=0):
    """n utterances of 2.5 ... 3.5 s (tones plus noise), all paired, transcripts of 20 ... 42 phones over 40 symbols -> data.corpus dict"""
    import csv
    from semi_tts_amd.audio import write_wav
    rs = np.random.RandomState(seed)
    vocab = ['P%02d' % i for i in range(40)]
    os.makedirs(os.path.join(root, 'wav', 'spk'), exist_ok=True)
    with open(os.path.join(root, 'partition.csv'), 'w', newline='') as fp, open(os.path.join(root, 'map.tsv'), 'w', newline='') as fm:
        wp, wm = csv.writer(fp), csv.writer(fm, delimiter='\t')
        wp.writerow(['', 'speaker', 'split', 'duration'])
        wm.writerow(['file', 'phn_seq', 'spkr'])
        for k in range(n):
            L = int(rs.randint(int(2.5 * SR), int(3.5 * SR)))
            t = np.arange(L) / SR
            x = 0.3 * np.sin(2 * np.pi * rs.uniform(100, 800) * t) + 0.1 * np.sin(2 * np.pi * rs.uniform(800, 3000) * t) + 0.02 * rs.randn(L)
            fid = 'u%03d' % k
            write_wav(os.path.join(root, 'wav', 'spk', fid + '.wav'), x, SR)
            wp.writerow([fid, 'spk', 'paired', '%.3f' % (L / SR)])
            wm.writerow([fid, ' '.join(vocab[int(i)] for i in rs.randint(0, 40, int(rs.randint(20, 43)))), 'spk'])
    with open(os.path.join(root, 'spkr.json'), 'w') as f:
        json.dump({'spk': 0}, f)
    with open(os.path.join(root, 'phn.vocab'), 'w') as f:
        f.write('\n'.join(vocab) + '\n')
    return dict(name='vctk', path=os.path.join(root, 'wav'), partition_table=os.path.join(root, 'partition.csv'),
                map_table=os.path.join(root, 'map.tsv'), spkr_map=os.path.join(root, 'spkr.json'),
                vocab_file=os.path.join(root, 'phn.vocab'), batch_size=32, bucketing=True)


def fetch_sides(root):
    """{'fetch': a paired fetch, 'extract_alone': extract_batch on one such batch packed alone (its own draws, as the fetch makes them)}"""
    import yaml
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.corpus import load_splits
    conv = load_audio_transform(**yaml.safe_load(open(os.path.join(ROOT, 'config', 'semi-single-spkr-paired-data.yaml')))['data']['audio'])
    _, sets = load_splits(write_corpus(root), conv, 3, ['paired'], {'paired': 32}, verbose=lambda m: None)
    ds = sets['paired']
    ds.fetch()
    by = {u.id: u for u in ds.rows}
    alone = conv.load_batch([by[i].path for i in ds.last_fetch[0]])

    def extract_alone():
        import torch
        draws = [conv._draw() for _ in range(32)]
        return conv.extract_batch(alone, r=3, seed=int(torch.randint(0, 2 ** 62, (1,))), snr=[d[0] for d in draws], stretch=[d[1] for d in draws])
    return {'fetch': ds.fetch, 'extract_alone': extract_alone}, dict(B=32, utterances=len(ds.rows), buffer_mb=round(ds.nbytes / 2 ** 20, 2),
                                                                       seconds_per_utterance=round(float(ds.lens.mean()) / SR, 2))


def ctc_inputs(dev, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    B, T, V, L = (CTC[k] for k in 'BTVL')
    prob = torch.softmax(torch.randn(B, T, V, generator=g) * 1.5, dim=-1).to(dev)
    text = torch.randint(1, V, (B, L), generator=g)
    for b in range(B):
        text[b, int(torch.randint(20, L, (1,), generator=g)):] = 0
    in_len = (T * (0.6 + 0.4 * torch.rand(B, generator=g))).round().to(torch.int32).clamp(max=T)
    mel = torch.rand(B, 2 * T, 80, generator=g)
    for b in range(B):
        mel[b, 2 * int(in_len[b]):] = 0
    return prob, text.to(dev), in_len.to(dev), mel.to(dev)


def parent_side(path, prob, text, eps=1e-10):
    """st_ctc_loss of another build of the library on (prob, text): -> (callable, loss, dprob)"""
    import torch
    from semi_tts_amd import ops
    lib = C.CDLL(path)
    P, I = C.c_void_p, C.c_int
    lib.st_ctc_workspace_floats.argtypes, lib.st_ctc_workspace_floats.restype = [I, I], C.c_size_t
    lib.st_ctc_loss.argtypes, lib.st_ctc_loss.restype = [P, P, C.c_float, P, P, P, I, I, I, I, I, P], I
    B, T, V = prob.shape
    L = text.shape[1]
    loss, dprob = torch.empty((), device=prob.device), torch.empty_like(prob)

    def call():
        ws = torch.empty(int(lib.st_ctc_workspace_floats(B, T)), device=prob.device)
        rc = lib.st_ctc_loss(prob.data_ptr(), text.data_ptr(), eps, loss.data_ptr(), dprob.data_ptr(), ws.data_ptr(), B, T, V, L, 0,
                             ops.stream_handle())
        assert rc == 0, rc
    return call, loss, dprob


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=300, help='calls per timed window (>= 100)')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='libsemitts_hip.so built from the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.calls < 100:
        ap.error('--calls must be >= 100: a shorter window measures the clock')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_corpus: no GPU (nothing here is timed on a CPU)')
    from semi_tts_amd import ops
    dev = torch.device('cuda:0')
    res = {'calls_per_window': a.calls, 'ctc_shape': CTC}
    with tempfile.TemporaryDirectory() as root:
        sides, res['fetch_shape'] = fetch_sides(root)
        t = {k: summary(v) for k, v in alternate(sides, max(100, a.calls // 3), a.windows).items()}
    res['fetch_us'] = t
    res['loader_own_cost_us'] = round(t['fetch']['median_us'] - t['extract_alone']['median_us'], 2)
    prob, text, in_len, mel = ctc_inputs(dev)
    full = torch.full_like(in_len, CTC['T'])
    sides = {'ctc_none': lambda: ops.ctc_loss(prob, text, 1e-10),
             'ctc_len_60_100': lambda: ops.ctc_loss(prob, text, 1e-10, in_len=in_len),
             'ctc_len_full': lambda: ops.ctc_loss(prob, text, 1e-10, in_len=full),
             'frame_lengths': lambda: ops.frame_lengths(mel, 0.0, 2)}
    assert ops.frame_lengths(mel, 0.0, 2).tolist() == in_len.tolist()
    res['ctc_us'] = {k: summary(v) for k, v in alternate(sides, a.calls, a.windows).items()}
    res['mean_in_len_over_T'] = round(float(in_len.float().mean()) / CTC['T'], 3)
    if a.parent_lib:
        call, p_loss, p_grad = parent_side(a.parent_lib, prob, text)
        call()
        loss, grad = ops.ctc_loss(prob, text, 1e-10)
        same = bool(torch.equal(loss.view(torch.int32), p_loss.view(torch.int32)) and torch.equal(grad.view(torch.int32), p_grad.view(torch.int32)))
        res['parent_bitwise_equal'] = same
        t = alternate({'parent_a': call, 'this': sides['ctc_none'], 'parent_b': call}, a.calls, a.windows)
        res['parent_us'] = {k: summary(v) for k, v in t.items()}
        pa, pb, th = (res['parent_us'][k]['median_us'] for k in ('parent_a', 'parent_b', 'this'))
        both = t['parent_a'] + t['parent_b']
        res['parent_spread_us'] = round(max(abs(pa - pb), max(both) - min(both)), 2)       # run-to-run spread measured on the parent itself
        res['this_minus_parent_us'] = round(th - 0.5 * (pa + pb), 2)
        res['no_slower_than_parent'] = bool(res['this_minus_parent_us'] <= res['parent_spread_us'])     # the allowed difference: that spread
    else:
        res['parent_us'] = 'not measured'
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
