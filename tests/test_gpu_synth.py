"""main.py --synth-phn-dir end to end on the shipped model size with synthetic weights, the trimming of solver.Synthesiser on a hand-made
batch, and the refusals that must leave nothing behind."""
import os
import sys
import types
import wave

import numpy as np
import pytest
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import attn_endpoint_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = os.path.join(REPO, 'config', 'supervised.yaml')


def _wav_samples(path, sr):
    with wave.open(path, 'rb') as w:
        assert w.getframerate() == sr and w.getnchannels() == 1 and w.getsampwidth() == 2
        return w.getnframes()


def _phn_dir(tmp_path):
    """three transcripts of 1, 5 and 12 phones: `score<TAB>tokens` as --transcribe-wav-dir writes it, symbols of the vocabulary, ids"""
    d = tmp_path / 'phn'
    d.mkdir()
    vocab = tmp_path / 'phn.vocab'
    vocab.write_text('\n'.join('P%d' % i for i in range(40)) + '\n')
    (d / 'a.phn').write_text('-1.500000\t7\n-2.000000\t7 8\n')
    (d / 'b.phn').write_text('P0 P4 P9 P2 P39\n')
    (d / 'c.phn').write_text(' '.join(str(3 + (5 * i) % 40) for i in range(12)) + '\n')
    return d, vocab, {'a.phn': 1, 'b.phn': 5, 'c.phn': 12}


def test_synth_phn_dir_end_to_end(tmp_path):
    import main as entry
    from semi_tts_amd.audio import load_audio_transform, min_frames
    from semi_tts_amd.solver import SYNTH_HEADER
    from semi_tts_amd.vqvae import synth_frames
    d, vocab, tokens = _phn_dir(tmp_path)
    entry.main(['--config', CFG, '--synth-phn-dir', str(d), '--vocab', str(vocab), '--gen-wav', '--batch-size', '3', '--max-frames-per-phone', '4',
                '--logdir', str(tmp_path / 'log'), '--name', 'syn', '--no-msg'])
    out = str(tmp_path / 'log' / 'syn')
    assert sorted(os.listdir(out)) == sorted(['synth.csv'] + ['%s-%s' % (k, s) for k in 'abc'
                                                              for s in ('mel.npy', 'spec.npy', 'align.npy', 'dur.npy', 'pred.wav')])
    conv = load_audio_transform(**yaml.safe_load(open(CFG))['data']['audio'])
    r, floor = 3, min_frames(conv.n_fft, conv.hop_length)
    T = synth_frames(12, r, 4.0)
    assert T == 90
    rows = open(os.path.join(out, 'synth.csv')).read().splitlines()
    assert rows[0] == SYNTH_HEADER and [x.split(',')[0] for x in rows[1:]] == ['a.phn', 'b.phn', 'c.phn']
    for row in rows[1:]:
        f, ntok, steps, frames, seconds, reached, focus, back, skips, covered = row.split(',')
        n, steps, frames, stem = tokens[f], int(steps), int(frames), os.path.join(out, f[:-4])
        mel, spec = np.load(stem + '-mel.npy'), np.load(stem + '-spec.npy')
        align, dur = np.load(stem + '-align.npy'), np.load(stem + '-dur.npy')
        assert int(ntok) == n and 1 <= steps <= T // r and frames == max(r * steps, floor)
        assert mel.shape == (frames, 80) and spec.shape == (frames, 1025) and mel.dtype == spec.dtype == np.float32
        assert align.shape == (steps, n) and dur.shape == (n,) and dur.dtype == np.int32 and (dur >= 0).all() and (dur % r == 0).all()
        if frames == r * steps:                                     # (the min-frames floor did not apply)
            assert dur.sum() == frames
        assert _wav_samples(stem + '-pred.wav', conv.sr) == conv.hop_length * (frames - 1)
        assert seconds == '%.4f' % (conv.hop_length * (frames - 1) / conv.sr)
        assert reached in ('0', '1') and (reached == '1' or steps == T // r)
        assert 0 <= int(back) < steps and 0 <= int(skips) < steps and 0 <= int(covered) <= min(n, int((dur > 0).sum()))
        assert 0.0 < float(focus) <= 1.0 and np.isfinite(mel).all() and np.isfinite(spec).all()
        # the focus of the csv is the mean peak weight of the kept steps; the peak may sit past the n columns the file keeps
        assert float(focus) >= float(np.mean(align.max(axis=1))) - 1e-4


def test_trimming_cuts_at_the_detected_end(tmp_path, capsys):
    """The solver's trimming on a hand-made device batch: staircase alignments with S well beyond the end, random mel and linear
    tensors.  Random weights will usually not keep the attention on the last phone, so the end-to-end run above cannot show a
    cut; this one does: files end at r * end, an utterance that never arrives is written whole with a [WARNING], the Griffin-Lim
    floor applies to a one-step utterance, and peaks on the appended token count for the last phone's duration."""
    from semi_tts_amd.audio import min_frames
    from semi_tts_amd.solver import Synthesiser, synth_row
    d, vocab, _ = _phn_dir(tmp_path)
    config = yaml.safe_load(open(CFG))
    paras = types.SimpleNamespace(name='trim', logdir=str(tmp_path / 'log'), load=None, seed=1, cpu=False, verbose=False, batch_size=3,
                                  synth_phn_dir=str(d), vocab=str(vocab), gen_wav=True, gen_wav_feat='linear', synth_sid=0,
                                  end_patience=3, end_max_jump=4, max_frames_per_phone=None)
    s = Synthesiser(config, paras, 'test').load_data()
    s.n_frames_per_step = r = 3                                     # (set_model only builds the network, which this test does not run)
    os.makedirs(s.logdir)
    conv = s.audio_converter
    floor = min_frames(conv.n_fft, conv.hop_length)
    S, L = 40, 6
    good, _ = O.staircase([4, 3, 5, 2], S, L, tail=4)               # phone 3 from step 12, the appended token from step 14: end = 15
    late, _ = O.staircase([4, 3, 5, 2], S, L, tail=2)               # leaves the last phone after 2 steps and never returns
    back = O.from_peaks([0, 1, 0, 1, 2, 3, 3, 3] + [5] * (S - 8), L)  # one backward jump; end = 8
    align = torch.from_numpy(np.stack([good, late, back])).to(DEV)
    g = torch.Generator().manual_seed(3)
    mel, lin = torch.rand(3, r * S, 80, generator=g).to(DEV), torch.rand(3, r * S, 1025, generator=g).to(DEV)
    files, trs = ['good.phn', 'late.phn', 'back.phn'], [[3, 4, 5, 6]] * 3
    rows = s.write_batch(files, trs, mel, lin, align, torch.tensor([4, 4, 4], dtype=torch.int32, device=DEV))
    err = capsys.readouterr().out
    assert '[WARNING] late.phn' in err and 'good.phn' not in err and 'back.phn' not in err
    hop, sr = conv.hop_length, conv.sr
    assert rows == [synth_row('good.phn', 4, 15, 45, hop * 44 / sr, 1, 0.75, 0, 0, 4),
                    synth_row('late.phn', 4, 40, 120, hop * 119 / sr, 0, 0.75, 1, 0, 4),
                    synth_row('back.phn', 4, 8, 24, hop * 23 / sr, 1, 0.75, 1, 0, 4)]
    for i, (k, end) in enumerate((('good', 15), ('late', 40), ('back', 8))):
        stem = os.path.join(s.logdir, k)
        assert np.array_equal(np.load(stem + '-mel.npy'), mel[i, :r * end].cpu().numpy())
        assert np.array_equal(np.load(stem + '-spec.npy'), lin[i, :r * end].cpu().numpy())
        assert np.array_equal(np.load(stem + '-align.npy'), align[i, :end, :4].cpu().numpy())
        assert _wav_samples(stem + '-pred.wav', sr) == hop * (r * end - 1)
        assert np.load(stem + '-dur.npy').sum() == r * end
    assert np.load(os.path.join(s.logdir, 'good-dur.npy')).tolist() == [12, 9, 15, 9]       # 2 steps on the phone + 1 on the token behind it
    assert np.load(os.path.join(s.logdir, 'late-dur.npy')).tolist() == [12, 9, 93, 6]
    assert np.load(os.path.join(s.logdir, 'back-dur.npy')).tolist() == [6, 6, 3, 9]
    # a single phone at patience 1 ends after one step: 3 frames, fewer than Griffin-Lim takes -> the floor
    s.patience = 1
    rows = s.write_batch(['one.phn'], [[9]], mel[:1], lin[:1], align[:1], [1])
    assert r < floor and rows == [synth_row('one.phn', 1, 1, floor, hop * (floor - 1) / sr, 1, 0.75, 0, 0, 1)]
    assert np.load(os.path.join(s.logdir, 'one-mel.npy')).shape == (floor, 80) and np.load(os.path.join(s.logdir, 'one-align.npy')).shape == (1, 1)
    assert _wav_samples(os.path.join(s.logdir, 'one-pred.wav'), sr) == hop * (floor - 1)


@pytest.mark.parametrize('bad,extra,msg', [('3 0 4\n', [], r'z\.phn: token 1 is id 0'), ('\n', [], r'z\.phn: empty transcript'),
                                           ('3 43\n', [], r'z\.phn: token 1 is id 43'), (None, ['--synth-sid', '109'], r'--synth-sid 109')])
def test_a_refused_run_writes_nothing(tmp_path, bad, extra, msg):
    import main as entry
    d, vocab, _ = _phn_dir(tmp_path)
    if bad is not None:
        (d / 'z.phn').write_text(bad)
    with pytest.raises(ValueError, match=msg):
        entry.main(['--config', CFG, '--synth-phn-dir', str(d), '--vocab', str(vocab), '--gen-wav', '--logdir', str(tmp_path / 'log'),
                    '--name', 'syn', '--no-msg'] + extra)
    assert not os.path.exists(str(tmp_path / 'log'))
