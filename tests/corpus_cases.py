"""The toy corpus of the corpus-loader tests, in the layout of data.corpus: two speakers, 10 paired, 6 unpaired and 4 dev utterances of
0.25 to 0.6 s at 22050 Hz (seeded tones plus noise), transcripts of 2 to 8 phones (some with a double space), a vocabulary of 6 symbols."""
import csv
import json
import os

import numpy as np

SR = 22050
VOCAB = ['AA', 'B', 'CH', 'D', 'EH', 'F']
SPEAKERS = {'lj': 0, 'p225': 1}
N_SPLIT = (('paired', 10), ('unpaired', 6), ('dev', 4))


def toy_rows(seed=0):
    """-> list of dict(id, speaker, split, samples, phn_seq, tokens): tokens the hand encoding of phn_seq (ids 3.., 1 for the empty
    piece of a double space, one trailing 0)"""
    rs = np.random.RandomState(seed)
    rows = []
    for split, n in N_SPLIT:
        for k in range(n):
            spk = 'lj' if (k + len(rows)) % 3 else 'p225'
            n_ph = int(rs.randint(2, 9))
            phones = [VOCAB[int(i)] for i in rs.randint(0, len(VOCAB), n_ph)]
            gap = int(rs.randint(1, n_ph)) if k % 2 == 0 else None        # a double space before phone `gap`
            seq, tokens = '', []
            for j, ph in enumerate(phones):
                if j:
                    seq += ' '
                if gap == j:
                    seq += ' '
                    tokens.append(1)
                seq += ph
                tokens.append(3 + VOCAB.index(ph))
            rows.append(dict(id='%s_%03d' % (split[:2], k), speaker=spk, split=split, samples=int(rs.randint(int(0.25 * SR), int(0.6 * SR))),
                             phn_seq=seq, tokens=tokens + [0]))
    return rows


def toy_wave(row, seed=0):
    rs = np.random.RandomState([seed, sum(map(ord, row['id']))])
    t = np.arange(row['samples']) / SR
    f = rs.uniform(120.0, 900.0, 3)
    x = sum(a * np.sin(2 * np.pi * fi * t + p) for a, fi, p in zip((0.3, 0.2, 0.1), f, rs.uniform(0, 6.28, 3)))
    return x + 0.02 * rs.randn(row['samples'])


def write_tables(root, rows, vocab=VOCAB, speakers=SPEAKERS):
    """the four files; -> the data.corpus dict (batch_size 4, no bucketing)"""
    root = str(root)
    os.makedirs(os.path.join(root, 'wav'), exist_ok=True)
    with open(os.path.join(root, 'partition.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['', 'speaker', 'split', 'duration'])
        for r in rows:
            w.writerow([r['id'], r['speaker'], r['split'], '%.3f' % (r['samples'] / SR)])
    with open(os.path.join(root, 'map.tsv'), 'w', newline='') as f:
        w = csv.writer(f, delimiter='\t')
        w.writerow(['file', 'phn_seq', 'spkr'])
        for r in rows:
            if r.get('phn_seq') is not None:
                w.writerow([r['id'], r['phn_seq'], r['speaker']])
    with open(os.path.join(root, 'spkr.json'), 'w') as f:
        json.dump(speakers, f)
    with open(os.path.join(root, 'phn.vocab'), 'w') as f:
        f.write('\n'.join(vocab) + '\n')
    return dict(name='vctk', path=os.path.join(root, 'wav'), partition_table=os.path.join(root, 'partition.csv'),
                map_table=os.path.join(root, 'map.tsv'), spkr_map=os.path.join(root, 'spkr.json'),
                vocab_file=os.path.join(root, 'phn.vocab'), batch_size=4, bucketing=False)


def write_waves(cfg, rows, sr=SR, seed=0):
    from semi_tts_amd.audio import write_wav
    for r in rows:
        d = os.path.join(cfg['path'], r['speaker'])
        os.makedirs(d, exist_ok=True)
        write_wav(os.path.join(d, r['id'] + '.wav'), toy_wave(r, seed), sr)


def write_toy_corpus(root, seed=0):
    """-> (data.corpus dict, rows)"""
    rows = toy_rows(seed)
    cfg = write_tables(root, rows)
    write_waves(cfg, rows, seed=seed)
    return cfg, rows
