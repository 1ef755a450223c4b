#!/usr/bin/env python3
"""CTC prefix beam search (st_ctc_beam_search) at the C2 shapes after the stride-2 encoder: B = 32, T = 129, V = 43, W in {1, 8, 16, 64,
128}, N = 1 and N = W; the whole transcription of one batch (features, eval encoder + codebook, search); and the float64 oracle of the
tests (tests/ctc_beam_oracle.py) over the same batch on 16 CPU processes, for comparison.  Prints one JSON line.

    python tools/bench_ctc_beam.py [--steps 20] [--oracle-widths 16]
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import yaml          # noqa: E402


def timed(fn, steps, warmup=3):
    """ms per call of `steps` back-to-back calls between two synchronises: pipelined time per call, not one call's latency"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _init():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _oracle(args):
    import ctc_beam_oracle as O
    return O.search(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--oracle-widths', type=str, default='16', help='comma-separated beam widths to time the CPU oracle at')
    a = ap.parse_args()
    from semi_tts_amd.ctc_decode import beam_search
    dev = torch.device('cuda:0')
    B, T, V = 32, 129, 43
    rs = np.random.RandomState(0)
    tgt = np.where(rs.rand(B, T) < 0.5, 0, rs.randint(1, V, (B, T)))
    x = rs.randn(B, T, V) + 6.0 * np.eye(V)[tgt]
    prob = np.exp(x - x.max(-1, keepdims=True))
    prob = (prob / prob.sum(-1, keepdims=True)).astype(np.float32)
    pd = torch.from_numpy(prob).to(dev)
    res = {'shape': [B, T, V], 'search_ms': {}}
    for W in (1, 8, 16, 64, 128):
        for N in sorted({1, W}):
            res['search_ms']['W%d_N%d' % (W, N)] = round(timed(lambda: beam_search(pd, None, W, N), a.steps), 4)
    # one batch end to end: 32 waveforms of ~3 s -> clean mel -> eval encoder + codebook -> search (W = 16)
    from semi_tts_amd.audio import load_audio_transform, WaveBatch, SNR_OFF
    from semi_tts_amd.synthetic import load_synthetic
    from semi_tts_amd.vqvae import VQVAE
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config', 'semi-single-spkr-paired-data.yaml')))
    conv = load_audio_transform(**cfg['data']['audio'])
    mcfg = dict(cfg['model'], codebook=dict(cfg['model']['codebook'], phn_attr_pth='', proj_attr=None))    # (no attribute table here)
    model = VQVAE(cfg['data']['audio']['num_mels'], cfg['data']['audio']['num_freq'], 43, 109, **mcfg).to(dev).eval()
    load_synthetic(model, seed=1234)
    hop = conv.hop_length
    waves = [torch.from_numpy((0.1 * rs.randn(hop * (256 - 1 - 8 * (i % 4)))).astype(np.float32)).to(dev) for i in range(B)]
    wb = WaveBatch(waves)
    frames = 1 + wb.lens // hop

    def features():
        return conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)[0]
    mel = features()

    def encoder():
        with torch.no_grad():
            return model.speech_to_text(paired_mel=mel, unpaired_mel=None)[0]

    def whole():
        m = conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)[0]
        return model.transcribe(m, frames, 16, 1)
    res['batch'] = dict(B=B, mel_frames=int(mel.shape[1]), enc_frames=int(encoder().shape[1]))
    res['features_ms'] = round(timed(features, a.steps), 4)
    res['encoder_eval_ms'] = round(timed(encoder, a.steps), 4)
    res['transcribe_batch_ms'] = round(timed(whole, a.steps), 4)
    # the float64 oracle on 16 CPU processes
    lp = np.log(prob.astype(np.float64) + 1e-10)
    res['oracle_cpu16_ms'] = {}
    with ProcessPoolExecutor(16, mp_context=mp.get_context('spawn'), initializer=_init) as ex:
        list(ex.map(_oracle, [(lp[0], 1, 0)] * 16))
        for W in [int(w) for w in a.oracle_widths.split(',') if w]:
            t0 = time.perf_counter()
            list(ex.map(_oracle, [(lp[b], W, 0) for b in range(B)]))
            res['oracle_cpu16_ms']['W%d' % W] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
