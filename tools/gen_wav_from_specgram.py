#!/usr/bin/env python3
"""Offline vocoding of saved linear spectrograms (the reference's util/gen_wav_from_specgram.py): every <name>-spec.npy under
--specgram-dir becomes <name>.wav in --output-dir, by Griffin-Lim on the device (semi_tts_amd.audio).  Files of the same length
are vocoded as one batch.

    python tools/gen_wav_from_specgram.py --config config/supervised.yaml --specgram-dir log/synthetic_0k --output-dir wav/
"""
import argparse
import os
import sys
from collections import defaultdict
from glob import glob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import yaml          # noqa: E402


def run(paras):
    from semi_tts_amd.audio import load_audio_transform, write_wav
    os.makedirs(paras.output_dir, exist_ok=True)
    config = yaml.safe_load(open(paras.config))
    conv = load_audio_transform(**config['data']['audio'])
    np.random.seed(paras.seed)
    groups = defaultdict(list)
    for f in sorted(glob(os.path.join(paras.specgram_dir, '*-spec.npy'))):
        groups[np.load(f, mmap_mode='r').shape].append(f)
    n = 0
    for shape, files in sorted(groups.items()):
        for i in range(0, len(files), paras.batch_size):
            chunk = files[i:i + paras.batch_size]
            wavs, sr = conv.feat_to_wave(torch.from_numpy(np.stack([np.load(f) for f in chunk])))
            for f, w in zip(chunk, wavs):
                write_wav(os.path.join(paras.output_dir, os.path.basename(f).replace('-spec.npy', '.wav')), w, sr)
                n += 1
    print('wrote %d waveforms to %s' % (n, paras.output_dir))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Convert spectrogram into raw waveform.')
    ap.add_argument('--config', type=str, required=True, help='Path to experiment config.')
    ap.add_argument('--specgram-dir', type=str, required=True, help='Path to input spectrogram.')
    ap.add_argument('--output-dir', type=str, required=True, help='Path to output wave.')
    ap.add_argument('--batch-size', type=int, default=32, help='same-length files vocoded together')
    ap.add_argument('--seed', type=int, default=0, help='np.random seed of the initial phases')
    run(ap.parse_args())
