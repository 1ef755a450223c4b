"""CPU side of the MFCC and phone-segment features (semi_tts_amd.audio, st_audio_mfcc / st_segment_gather): the DCT table and the two
clamped 9-tap filters against scipy, the cutting rule, the segment table, every refusal before a device is touched, and the new
main.py flags.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfcc_oracle as MO   # noqa: E402
from semi_tts_amd import audio   # noqa: E402
from semi_tts_amd.ctc_align import SEGMENTS_HEADER, segment_row   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


def test_framing_is_the_references():
    conv = audio.load_audio_transform(**AUDIO_CFG)
    assert (conv.win_length_mfcc, conv.hop_length_mfcc) == (551, 220) == MO.mfcc_dims(22050)
    assert audio.mfcc_dims(16000) == (400, 160)
    assert audio.MFCC_DIM == 39 and not conv.use_segment


def test_dct_table_is_scipys():
    for n_mels in (13, 40, 80, 256):
        ref = scipy.fft.dct(np.eye(n_mels), axis=0, type=2, norm='ortho')[:13]
        assert np.abs(audio.mfcc_dct(13, n_mels) - ref).max() <= 1e-12
    mel = np.random.RandomState(0).rand(80, 17)
    assert np.abs(audio.mfcc_dct(13, 80) @ mel - scipy.fft.dct(mel, axis=0, type=2, norm='ortho')[:13]).max() <= 1e-12


@pytest.mark.parametrize('T', [9, 10, 13, 40])
def test_clamped_filters_are_savgol_interp(T):
    c = np.random.RandomState(T).randn(13, T)
    for order, taps in ((1, audio.MFCC_DELTA_TAPS), (2, audio.MFCC_DELTA2_TAPS)):
        ref = scipy.signal.savgol_filter(c, 9, deriv=order, polyorder=order, axis=-1, mode='interp')
        got = audio.clamped_filter(c, taps)
        assert np.abs(got - ref).max() <= 1e-12, (T, order)
        # the first four and last four frames repeat the value of frames 4 and T - 5
        assert np.array_equal(got[:, :4], np.repeat(got[:, 4:5], 4, 1)) and np.array_equal(got[:, T - 4:], np.repeat(got[:, T - 5:T - 4], 4, 1))
    assert abs(sum(abs(w) for w in audio.MFCC_DELTA_TAPS) - 1 / 3) < 1e-15
    assert abs(sum(abs(w) for w in audio.MFCC_DELTA2_TAPS) - 140 / 462) < 1e-15
    with pytest.raises(ValueError, match='9 taps'):
        audio.clamped_filter(np.zeros((13, 8)), audio.MFCC_DELTA_TAPS)


def test_segment_points():
    sp = audio.segment_points
    assert sp([0.0, 0.5, 1.0], 10, 2) == ([(0, 5), (5, 10)], 5)                     # a first boundary of 0 emits nothing
    assert sp([0.3, 0.4, 0.7, 1.0], 10, 2) == ([(0, 3), (3, 7), (7, 10)], 4)        # [3, 4) is too short: absorbed by the next piece
    assert sp([0.25, 0.35, 1.0], 10, 2) == ([(0, 2), (2, 4), (4, 10)], 6)           # 2.5 -> 2 and 3.5 -> 4: halves to even
    assert sp([0.1, 0.2], 10, 5) == ([], 2)                                         # no piece long enough: S = 0
    assert sp([0.1, 0.2, 1.0], 10, 20) == ([], 10)
    assert sp([1.0], 7, 2) == ([(0, 7)], 7)
    for bd, T, m in (([0.0, 0.5, 1.0], 10, 2), ([0.3, 0.4, 0.7, 1.0], 10, 2), ([0.25, 0.35, 1.0], 10, 2), ([0.1, 0.2], 10, 5),
                     ([0.31, 0.33, 0.9, 1.0], 41, 3)):
        feat = np.arange(T * 3, dtype=np.float32).reshape(T, 3)
        pieces, max_len = sp(bd, T, m)
        ref = MO.segment(feat, bd, m)
        assert ref.shape == (len(pieces), max_len, 3)
        for s, (lo, hi) in enumerate(pieces):
            assert np.array_equal(ref[s, :hi - lo], feat[lo:hi]) and not ref[s, hi - lo:].any()


def test_aligner_rows_tile_the_utterance(tmp_path):
    """a row written by ctc_align.segment_row, read back: its pieces cover [0, T) exactly, at the mel and at the MFCC frame rate"""
    frame_s = 2 * 275 / 22050
    rows = [SEGMENTS_HEADER, segment_row('some/dir/utt1.wav', [0, 3, 7, 12, 30], 37, frame_s), segment_row('utt2.x.wav', [0], 5, frame_s)]
    (tmp_path / 'segments.csv').write_text('\n'.join(rows) + '\n')
    table = audio.read_segment_table(tmp_path / 'segments.csv')
    assert sorted(table) == ['utt1', 'utt2'] and table['utt2'] == [1.0] and len(table['utt1']) == 5 and table['utt1'][-1] == 1.0
    for T in (37, 74, 93, 1000):
        for key, n in (('utt1', 5), ('utt2', 1)):
            pieces, max_len = audio.segment_points(table[key], T, 1)
            assert len(pieces) == n and pieces[0][0] == 0 and pieces[-1][1] == T
            assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and max_len == max(hi - lo for lo, hi in pieces)


def test_segment_file_arguments(tmp_path):
    f = tmp_path / 'seg.csv'
    f.write_text('file,seg\nutt1,0.5_1.0_2.0\nutt2,0.3_1.2\n')
    for kind, dim in (('mfcc', 39), ('MEL', 80), ('linear', 1025)):
        conv = audio.load_audio_transform(**AUDIO_CFG, segment_file=str(f), segment_feat=kind, min_segment_len=3)
        assert conv.use_segment and conv.seg_feat_dim == dim and conv.segment_feat == kind.lower() and conv.min_segment_len == 3
        assert conv.boundary_table == {'utt1': [0.25, 0.5, 1.0], 'utt2': [0.25, 1.0]} == {k: audio.compute_len_ratio(v) for k, v in
                                                                                           (('utt1', '0.5_1.0_2.0'), ('utt2', '0.3_1.2'))}
        assert conv.boundary('a/b/utt2.wav') == [0.25, 1.0] and conv.boundary('utt1') == [0.25, 0.5, 1.0]
        with pytest.raises(KeyError, match='utt3.wav'):
            conv.boundary('corpus/utt3.wav')
        with pytest.raises(KeyError, match='utt3'):
            conv.segment_batch(torch.zeros(1, 10, dim), [10], ['utt3'])
    assert audio.load_audio_transform(**AUDIO_CFG, segment_file=str(f), segment_feat='mel').min_segment_len == 2
    with pytest.raises(NotImplementedError):
        audio.load_audio_transform(**AUDIO_CFG, segment_file=str(f), segment_feat='fbank')
    with pytest.raises(NotImplementedError):
        audio.load_audio_transform(**AUDIO_CFG, segment_file=str(f))
    # without a segment_file the other two are not read, as before
    plain = audio.load_audio_transform(**AUDIO_CFG, segment_feat='fbank', min_segment_len=7)
    assert not plain.use_segment
    with pytest.raises(ValueError, match='without a segment_file'):
        plain.boundary('utt1')
    for text, what in (('key,seg\nutt1,1_2\n', 'header'), ('file,seg\nutt1\n', 'line 2'), ('file,seg\nutt1,1_x\n', 'line 2'),
                       ('file,seg\nutt1,1_0\n', 'line 2'), ('file,seg\nutt1,1_2\nutt1,1_3\n', 'twice'), ('', 'header')):
        f.write_text(text)
        with pytest.raises(ValueError, match=what):
            audio.read_segment_table(f)
    with pytest.raises(OSError):
        audio.load_audio_transform(**AUDIO_CFG, segment_file=str(tmp_path / 'missing.csv'), segment_feat='mel')


def test_refusals_come_before_the_device(monkeypatch):
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('device touched')))
    conv = audio.load_audio_transform(**AUDIO_CFG)
    with pytest.raises(ValueError, match='fewer than 9 MFCC frames'):
        conv.extract_mfcc_batch([torch.zeros(8 * 220 - 1)])                         # 8 frames
    with pytest.raises(ValueError, match='fewer than 9 MFCC frames'):
        conv.extract_mfcc_from_waveform(torch.zeros(1, 30000)[:, :1700])
    with pytest.raises(ValueError, match='fewer than 9 MFCC frames'):
        conv.extract_mfcc_batch([torch.zeros(30000), torch.zeros(1759)])
    with pytest.raises(AssertionError, match='device touched'):                     # 9 frames pass every check
        conv.extract_mfcc_batch([torch.zeros(8 * 220)])
    with pytest.raises(ValueError, match='n_fft // 2'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=2049)).extract_mfcc_batch([torch.zeros(2048)])
    with pytest.raises(ValueError, match='not supported'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=1001)).extract_mfcc_batch([torch.zeros(30000)])
    with pytest.raises(ValueError, match='win <= n_fft'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=257)).extract_mfcc_batch([torch.zeros(30000)])      # win 551 > n_fft 512
    with pytest.raises(ValueError, match='mels outside'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_mels=12)).extract_mfcc_batch([torch.zeros(30000)])
    with pytest.raises(ValueError, match='mels outside'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_mels=257)).extract_mfcc_batch([torch.zeros(30000)])
    with pytest.raises(ValueError, match='empty batch'):
        conv.extract_mfcc_batch([])
    with pytest.raises(ValueError, match=r'expected \(T, D\)'):
        conv.segment(torch.zeros(10), [1.0])
    with pytest.raises(ValueError, match='the batch holds'):
        conv._gather(torch.zeros(1, 10, 4), [11], [[1.0]])


FLAG_CASES = [
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc'], None),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mel', '--segment-file', 's.csv', '--min-segment-len', '3', '--batch-size', '4'], None),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'linear', '--segment-file', 's.csv'], None),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'fbank'], 'invalid choice'),
    (['--config', 'c', '--feat-wav-dir', 'd'], 'needs --config (its data.audio) and --feat'),
    (['--feat-wav-dir', 'd', '--feat', 'mfcc'], 'needs --config (its data.audio) and --feat'),
    (['--config', 'c', '--feat', 'mfcc'], 'they need that flag'),
    (['--config', 'c', '--segment-file', 's.csv'], 'they need that flag'),
    (['--config', 'c', '--min-segment-len', '2'], 'they need that flag'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--min-segment-len', '2'], 'it needs that flag'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--segment-file', 's.csv', '--min-segment-len', '0'], 'must be >= 1'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--gen-specgram'], 'does not combine with --gen-specgram'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--tts-only'], 'does not combine with --tts-only'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--unpair-wav-dir', 'x'], 'does not combine with --unpair-wav-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--transcribe-wav-dir', 'x'], 'does not combine with --transcribe-wav-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--align-wav-dir', 'x'], 'does not combine with --align-wav-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--vocode-dir', 'x'], 'does not combine with --vocode-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--resample-wav-dir', 'x', '--resample-out', 'y'],
     'does not combine with --resample-wav-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--build-lm-phn-dir', 'x', '--lm', 't.npy', '--lm-order', '2'],
     'does not combine with --build-lm-phn-dir'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--dev-batches', '2'], 'does not combine with --dev-batches'),
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--resample'], 'it needs one of them'),       # (that error and its text stay)
    (['--config', 'c', '--feat-wav-dir', 'd', '--feat', 'mfcc', '--gen-gt-specgram'], 'bin/gen_gt_specgram.py'),
    (['--config', 'c'], None),
]


def test_main_flag_validation(tmp_path):
    """every case through main.parse_args in one child process (argparse exits the interpreter on an error)"""
    script = tmp_path / 'flags.py'
    script.write_text(
        'import contextlib, io, json, sys\n'
        'sys.path.insert(0, sys.argv[1])\n'
        'import main\n'
        'out = []\n'
        'for argv, _ in json.loads(sys.argv[2]):\n'
        '    err = io.StringIO()\n'
        '    try:\n'
        '        with contextlib.redirect_stderr(err):\n'
        '            p = main.parse_args(argv)\n'
        '        out.append([0, [p.feat_wav_dir, p.feat, p.segment_file, p.min_segment_len, p.batch_size]])\n'
        '    except SystemExit as e:\n'
        '        out.append([e.code, err.getvalue()])\n'
        'print("RESULT " + json.dumps(out))\n')
    r = subprocess.run([sys.executable, str(script), REPO, json.dumps(FLAG_CASES)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][0][7:])
    assert len(res) == len(FLAG_CASES)
    for (argv, want), (code, text) in zip(FLAG_CASES, res):
        if want is None:
            assert code == 0, (argv, text)
        else:
            assert code == 2 and want in text, (argv, code, text)
    assert res[0][1] == ['d', 'mfcc', None, 2, None]
    assert res[1][1] == ['d', 'mel', 's.csv', 3, 4]
    assert res[-1][1] == [None, None, None, 2, None]
