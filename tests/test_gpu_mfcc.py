"""MFCC and phone-segment features on the MI355X (st_audio_mfcc, st_segment_gather, semi_tts_amd.audio, solver.FeatureWriter) against
the float64 yardstick of tests/mfcc_oracle.py (tests/feat_oracle.py's mel at the MFCC framing, scipy's DCT and Savitzky-Golay filters).
The reference's own MFCC path needs librosa and torchaudio and cannot run where the fixtures are made, so there is no golden file for it:
scipy -- librosa's implementation of both steps -- is the reference.

Tolerance of all 39 columns: sqrt(n_mels) * MEL_TOL (8.9e-4 at 80 mels), derived, not measured: the rows of the orthonormal DCT have
unit 2-norm, so a cepstrum moves by at most sqrt(n_mels) times the largest mel error (MEL_TOL = 1e-4, the bound of the feature tests),
and the absolute tap sums of the two derivative filters are 1/3 and 140/462, both below 1."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfcc_oracle as MO   # noqa: E402
from semi_tts_amd import ops   # noqa: E402
from semi_tts_amd.audio import load_audio_transform, mel_filterbank, write_wav   # noqa: E402

pytestmark = pytest.mark.gpu

AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])
AUDIO_16K = dict(AUDIO_CFG, num_freq=257, num_mels=40, sample_rate=16000)
MEL_TOL = 1e-4
SR, HOP = 22050, 220
LENS = [8 * HOP + 57, 16 * HOP + 100, 39 * HOP + 219]       # 9 (the fewest the derivatives take), 17 and 40 MFCC frames
FRAMES, T_PAD = [9, 17, 40], 43


def _tol(n_mels):
    return float(np.sqrt(n_mels)) * MEL_TOL


def _speech(L, seed, sr=SR):
    """harmonic tone with gated silences (the 1e-5 clamp is reached): the signal of tests/test_gpu_features.py"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / sr
    f0 = 100 + 150 * rs.rand()
    x = sum(0.4 / (h + 1) * np.sin(2 * np.pi * f0 * (h + 1) * t + rs.rand()) for h in range(6))
    gate = (np.sin(2 * np.pi * 2 * t + 6 * rs.rand()) > -0.2)
    return (0.7 * x * gate + 0.002 * rs.randn(L)).astype(np.float32)


def _maxabs(got, ref):
    return float((torch.as_tensor(got).double().cpu() - torch.as_tensor(ref).double()).abs().max())


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def conv():
    return load_audio_transform(**AUDIO_CFG)


@pytest.fixture(scope='module')
def wavs():
    return [_speech(L, 70 + i) for i, L in enumerate(LENS)]


@pytest.fixture(scope='module')
def ref(wavs):
    """the oracle's (mfcc (39, T), mel (80, T)) of every utterance, computed once"""
    fb = mel_filterbank(SR, 2048, 80)
    return [MO.mfcc(w, fb) for w in wavs]


def _run(conv, dev, waves, T_pad, preemph=None, with_mel=True):
    """st_audio_mfcc on `waves` in the given order (no sorting), padded to T_pad"""
    lens = np.array([len(w) for w in waves])
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    x = torch.from_numpy(np.concatenate(waves)).to(dev)
    return ops.audio_mfcc(x, off, lens, conv.n_fft, conv.win_length_mfcc, conv.hop_length_mfcc,
                          conv.preemphasis_coeff if preemph is None else preemph, conv.filterbank(dev), conv.mfcc_table(dev), T_pad,
                          with_mel=with_mel)


@pytest.fixture(scope='module')
def batch(conv, dev, wavs):
    return _run(conv, dev, wavs, T_PAD)


def _check_blocks(got, ref_mfcc, T, what, n_mels=80):
    """got (T_pad, 39) device rows against the oracle's (39, T), block by block; rows past T exactly 0"""
    tol = _tol(n_mels)
    for k, name in enumerate(('cepstra', 'delta', 'delta2')):
        err = _maxabs(got[:T, 13 * k:13 * (k + 1)], ref_mfcc[13 * k:13 * (k + 1)].T)
        print('%s %s: max-abs %.2e (tolerance %.2e)' % (what, name, err, tol))
        assert err <= tol, (what, name, err)
    assert bool((got[T:] == 0).all()), what


def test_ragged_batch_against_the_oracle(conv, batch, ref):
    mfcc, mel = batch
    assert mfcc.is_cuda and mfcc.shape == (3, T_PAD, 39) and mel.shape == (3, T_PAD, 80)
    for b, T in enumerate(FRAMES):
        assert ref[b][0].shape == (39, T)
        _check_blocks(mfcc[b], ref[b][0], T, 'T_b = %d' % T)
        err = _maxabs(mel[b, :T], ref[b][1].T)
        print('T_b = %d mel at the MFCC framing: max-abs %.2e' % (T, err))
        assert err <= MEL_TOL and bool((mel[b, T:] == 0).all())
    # at T_b = 9 every frame takes its derivatives from the window centred at frame 4
    assert bool((mfcc[0, :9, 13:] == mfcc[0, 4, 13:]).all()) and bool((mfcc[0, :9, 13:] != 0).any())
    # longer utterances: the first and last four frames repeat frames 4 and T_b - 5
    assert bool((mfcc[2, :4, 13:] == mfcc[2, 4, 13:]).all()) and bool((mfcc[2, 36:40, 13:] == mfcc[2, 35, 13:]).all())
    assert not bool((mfcc[2, 5, 13:] == mfcc[2, 4, 13:]).all())


def test_zero_utterance_is_exactly_zero(conv, dev, wavs):
    mfcc, mel = _run(conv, dev, [np.zeros(3000, np.float32), wavs[1]], 20)
    assert bool((mfcc[0] == 0).all()) and bool((mel[0] == 0).all())
    assert bool((mfcc[1, :17] != 0).any())


def test_bitwise_independent_of_batch_and_position(conv, dev, wavs, batch):
    mfcc, mel = batch
    again, _ = _run(conv, dev, wavs, T_PAD)
    assert torch.equal(again, mfcc)                                              # repeatable
    rev, rev_mel = _run(conv, dev, wavs[::-1], 40)                               # other positions, another T_pad
    for b, T in enumerate(FRAMES):
        alone, alone_mel = _run(conv, dev, [wavs[b]], T)
        assert torch.equal(alone[0], mfcc[b, :T]) and torch.equal(alone_mel[0], mel[b, :T])
        assert torch.equal(rev[2 - b, :T], mfcc[b, :T]) and torch.equal(rev_mel[2 - b, :T], mel[b, :T])
    # the public call sorts longest first and pads to the longest
    out = conv.extract_mfcc_batch([torch.from_numpy(w) for w in wavs])
    assert out.is_cuda and out.shape == (3, 40, 39)
    for row, b in enumerate((2, 1, 0)):
        assert torch.equal(out[row, :FRAMES[b]], mfcc[b, :FRAMES[b]]) and bool((out[row, FRAMES[b]:] == 0).all())


def test_preemphasis_off(conv, dev, wavs, batch):
    fb = mel_filterbank(SR, 2048, 80)
    got, _ = _run(conv, dev, [wavs[1]], 17, preemph=0.0)
    _check_blocks(got[0], MO.mfcc(wavs[1], fb, preemph=0.0)[0], 17, 'no pre-emphasis')
    assert not torch.equal(got[0], batch[0][1, :17])
    x = torch.from_numpy(wavs[1])[None]
    assert torch.equal(conv.extract_mfcc_from_waveform(x, preemphasis=False), got[0].t().cpu())


def test_16k_n_fft_512(dev):
    c16 = load_audio_transform(**AUDIO_16K)
    assert (c16.n_fft, c16.win_length_mfcc, c16.hop_length_mfcc) == (512, 400, 160)
    fb = mel_filterbank(16000, 512, 40)
    lens = [8 * 160 + 159, 11 * 160 + 3]                                         # 9 and 12 frames
    waves = [_speech(L, 80 + i, sr=16000) for i, L in enumerate(lens)]
    mfcc, mel = _run(c16, dev, waves, 12)
    for b, T in enumerate((9, 12)):
        r_mfcc, r_mel = MO.mfcc(waves[b], fb, sr=16000, n_fft=512)
        _check_blocks(mfcc[b], r_mfcc, T, '16 kHz T_b = %d' % T, n_mels=40)
        assert _maxabs(mel[b, :T], r_mel.T) <= MEL_TOL


def test_batch_across_the_chunk_boundary(dev):
    """FEATURES_MAX_BATCH + 1 utterances go out as two st_audio_mfcc calls (64 + 1): every utterance's rows are bitwise those of the
    utterance extracted alone (a frame's bits depend on neither the batch nor the position in it), rows past its frames are zero"""
    c16 = load_audio_transform(**AUDIO_16K)
    n_fft, win, hop = 512, 32, 16
    B = ops.FEATURES_MAX_BATCH + 1
    lens = np.array([257 + b for b in range(B)])                                 # 17 .. 21 frames: above n_fft / 2 samples and 9 frames
    frames = 1 + lens // hop
    assert B == 65 and frames.min() == 17 and frames.max() == 21
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    x = torch.from_numpy(_speech(int(lens.sum()), 90, sr=16000)).to(dev)
    fb, dct, T_pad = c16.filterbank(dev), c16.mfcc_table(dev), int(frames.max())

    def run(off, lens):
        return ops.audio_mfcc(x, off, lens, n_fft, win, hop, c16.preemphasis_coeff, fb, dct, T_pad, with_mel=True)

    mfcc, mel = run(off, lens)
    assert mfcc.shape == (B, T_pad, 39) and mel.shape == (B, T_pad, 40)
    for b in range(B):
        T = int(frames[b])
        alone, alone_mel = run(off[b:b + 1], lens[b:b + 1])
        assert torch.equal(mfcc[b], alone[0]) and torch.equal(mel[b], alone_mel[0]), b
        assert bool((mfcc[b, T:] == 0).all()) and bool((mel[b, T:] == 0).all()) and bool((mfcc[b, :T] != 0).any()), b


def test_extract_mfcc_from_waveform(conv, dev, wavs, batch, tmp_path):
    x = torch.from_numpy(wavs[2])
    got = conv.extract_mfcc_from_waveform(x[None])
    assert got.shape == (39, 40) and not got.is_cuda and torch.equal(got, batch[0][2, :40].t().cpu())
    got_d = conv.extract_mfcc_from_waveform(torch.stack([x, -x]).to(dev), channel=1)
    assert got_d.is_cuda and got_d.shape == (39, 40)
    assert torch.equal(got_d[:13].cpu(), got[:13])                               # (|X| does not see the sign)
    write_wav(tmp_path / 'u.wav', wavs[2], SR)
    from_file = conv.extract_mfcc_from_file(tmp_path / 'u.wav')
    assert torch.equal(from_file, conv.extract_mfcc_from_waveform(conv.load(tmp_path / 'u.wav')))
    assert from_file.shape == (39, 40) and not from_file.is_cuda


@pytest.mark.parametrize('D', [39, 80, 1025])
def test_segment_gather(dev, D):
    B, T_pad = 2, 23
    big = torch.randn(B, T_pad, D + 3, device=dev)
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
    table = [(0, 0, 5), (0, 5, 7), (1, 3, 1), (1, 10, 13), (0, 22, 0)]           # (utterance, start, rows); the last one is empty
    for feat in (big[:, :, :D].contiguous(), big[:, :, :D], big[:, ::2, 3:]):     # contiguous, a row stride above D, a frame stride
        for max_len in (13, 14):
            out = ops.segment_gather(feat, ints([r[0] for r in table]), ints([r[1] for r in table]), ints([r[2] for r in table]), max_len)
            assert out.shape == (5, max_len, D)
            for s, (u, lo, n) in enumerate(table if feat.size(1) == T_pad else []):
                assert torch.equal(out[s, :n], feat[u, lo:lo + n]) and bool((out[s, n:] == 0).all())
            if feat.size(1) != T_pad:                                            # 12 frames: the reads past them are clamped, not faults
                assert torch.equal(out[0, :5], feat[0, 0:5]) and torch.equal(out[2, :1], feat[1, 3:4])
    feat = big[:, :, :D].contiguous()
    empty = ops.segment_gather(feat, ints([]), ints([]), ints([]), 7)
    assert empty.shape == (0, 7, D)
    assert ops.segment_gather(feat, ints([0]), ints([0]), ints([0]), 0).shape == (1, 0, D)
    # a wrong table: a start past T_pad, a negative one, utterances outside the batch -- every read is clamped into feat
    out = ops.segment_gather(feat, ints([1, 0, 7, -3]), ints([1000, -5, 21, 0]), ints([3, 2, 4, 99]), 4)
    torch.cuda.synchronize()
    assert torch.equal(out[0, :3], feat[1, 22:23].expand(3, D)) and bool((out[0, 3:] == 0).all())
    assert torch.equal(out[1, :2], feat[0, 0:1].expand(2, D))
    assert torch.equal(out[2, :2], feat[1, 21:23]) and torch.equal(out[2, 2:], feat[1, 22:23].expand(2, D))
    assert torch.equal(out[3], feat[0, :4])


def test_segment_batch_against_the_oracle(dev, wavs, tmp_path):
    seg_file = tmp_path / 'segments.csv'
    bounds = {'u0': '0.0_0.2_0.21_0.7_1.0', 'u1': '0.1_0.45_0.5_0.9', 'u2': '0.02_0.3_0.31_0.32_0.8_1.3_1.3'}
    seg_file.write_text('file,seg\n' + ''.join('%s,%s\n' % kv for kv in bounds.items()))
    for kind in ('mfcc', 'mel', 'linear'):
        conv = load_audio_transform(**AUDIO_CFG, segment_file=str(seg_file), segment_feat=kind, min_segment_len=2)
        tw = [torch.from_numpy(w) for w in wavs[::-1]]                           # longest first: rows u2, u1, u0
        if kind == 'mfcc':
            feats, frames = conv.extract_mfcc_batch(tw), [40, 17, 9]
        else:
            mel, _, lin = conv.extract_batch(tw, snr=float('nan'), stretch=1.0)
            feats, frames = (mel if kind == 'mel' else lin), [1 + len(w) // conv.hop_length for w in wavs[::-1]]
        keys = ['dir/u2.wav', 'u1', 'u0.wav']
        seg, counts = conv.segment_batch(feats, frames, keys)
        refs = [MO.segment(feats[b, :frames[b]].cpu().numpy(), conv.boundary(k), 2) for b, k in enumerate(keys)]
        assert counts == [len(r) for r in refs] and sum(counts) > 6 and seg.is_cuda
        assert seg.shape == (sum(counts), max(r.shape[1] for r in refs), conv.seg_feat_dim)
        first = 0
        for r in refs:
            got = seg[first:first + len(r)].cpu().numpy()
            assert np.array_equal(got[:, :r.shape[1]], r) and not got[:, r.shape[1]:].any()
            first += len(r)
        # one utterance through segment(): the reference's call, on the feature's device
        one = conv.segment(feats[1, :frames[1]].cpu(), conv.boundary('u1'))
        assert not one.is_cuda and np.array_equal(one.numpy(), refs[1])


def test_feature_writer_end_to_end(dev, tmp_path):
    import main
    from semi_tts_amd.solver import FeatureWriter
    wav_dir = tmp_path / 'wavs'
    wav_dir.mkdir()
    lens = {'b_utt': 9000, 'a_utt': 6100}
    for i, (stem, L) in enumerate(lens.items()):
        write_wav(wav_dir / (stem + '.wav'), _speech(L, 90 + i), SR)
    seg_file = tmp_path / 'segments.csv'
    seg_file.write_text('file,seg\na_utt,0.05_0.11_0.12_0.2767\nb_utt,0.1_0.2_0.4082\n')
    config = {'data': {'audio': AUDIO_CFG}}
    for kind, dim in (('mfcc', 39), ('mel', 80), ('linear', 1025)):
        paras = main.parse_args(['--config', 'unused', '--feat-wav-dir', str(wav_dir), '--feat', kind, '--segment-file', str(seg_file),
                                 '--min-segment-len', '3', '--logdir', str(tmp_path / 'log'), '--name', kind, '--batch-size', '2', '--no-msg'])
        assert FeatureWriter(config, paras, 'test').load_data().set_model().exec() == 2
        out = tmp_path / 'log' / kind
        assert sorted(os.listdir(out)) == sorted('%s-%s%s.npy' % (s, kind, e) for s in lens for e in ('', '-seg'))
        conv = load_audio_transform(**AUDIO_CFG, segment_file=str(seg_file), segment_feat=kind, min_segment_len=3)
        for stem, L in lens.items():
            path = wav_dir / (stem + '.wav')
            if kind == 'mfcc':
                want = conv.extract_mfcc_from_file(path).t()
                T = 1 + L // HOP
            else:
                sp, msp = conv.extract_feature_from_waveform(conv.load(path))
                want = (msp if kind == 'mel' else sp).t()
                T = 1 + L // conv.hop_length
            feat = np.load(out / ('%s-%s.npy' % (stem, kind)))
            assert feat.dtype == np.float32 and feat.shape == (T, dim) and np.array_equal(feat, want.numpy())
            seg = np.load(out / ('%s-%s-seg.npy' % (stem, kind)))
            want_seg = conv.segment_features(path).numpy()
            assert seg.shape == want_seg.shape and seg.shape[0] >= 2 and seg.shape[2] == dim and np.array_equal(seg, want_seg)
            assert np.array_equal(seg, MO.segment(feat, conv.boundary(stem), 3))
    # without --segment-file only the features are written; a file without a row stops the run before anything is written
    paras = main.parse_args(['--config', 'unused', '--feat-wav-dir', str(wav_dir), '--feat', 'mfcc', '--logdir', str(tmp_path / 'log'),
                             '--name', 'plain', '--batch-size', '1', '--no-msg'])
    assert FeatureWriter(config, paras, 'test').load_data().set_model().exec() == 2
    assert sorted(os.listdir(tmp_path / 'log' / 'plain')) == ['a_utt-mfcc.npy', 'b_utt-mfcc.npy']
    assert np.array_equal(np.load(tmp_path / 'log' / 'plain' / 'a_utt-mfcc.npy'), np.load(tmp_path / 'log' / 'mfcc' / 'a_utt-mfcc.npy'))
    seg_file.write_text('file,seg\na_utt,0.05_0.2767\n')
    paras = main.parse_args(['--config', 'unused', '--feat-wav-dir', str(wav_dir), '--feat', 'mel', '--segment-file', str(seg_file),
                             '--logdir', str(tmp_path / 'log'), '--name', 'missing', '--no-msg'])
    with pytest.raises(KeyError, match='b_utt.wav'):
        FeatureWriter(config, paras, 'test').load_data()
    assert not (tmp_path / 'log' / 'missing').exists()
