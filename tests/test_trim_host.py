"""Silence trimming without a GPU: the float64 oracle on hand-computed cases, every refusal of ops._trim_check and of main.py's flags,
the build list, what corpus.apply_bounds makes of a split once its bounds are known, and THE GUARD of the GPU tests' case table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_cases as TC     # noqa: E402
import trim_oracle as TO    # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the oracle on cases worked out by hand
def test_oracle_energy_and_bounds_by_hand():
    # frame_length 4, hop 2, L = 6: T = 4; frame t reads x[2t - 2 .. 2t + 2) with zeros outside
    r = TO.trim([1, 1, 0, 0, 0, 0], 4, 2, 10.0, max_iv=2)
    assert r['energy'].tolist() == [0.5, 0.5, 0.0, 0.0]
    assert r['bounds'] == [0, 4, 2, 0] and r['n_iv'] == 1 and r['intervals'].tolist() == [[0, 4], [-1, -1]]
    # the last frame alone: centred on sample L = 4, it reads x[2 .. 6) -> (0 + 4 + 0 + 0) / 4; its span starts at 2 hop = L: empty
    r = TO.trim([0, 0, 0, 2], 4, 2, 3.0, max_iv=1)
    assert r['energy'].tolist() == [0.0, 1.0, 1.0] and r['bounds'] == [2, 4, 2, 0]
    r = TO.trim([0, 0, 0, 0, 0, 2], 4, 4, 3.0, max_iv=1)      # hop 4: frames at 0 and 4; only frame 1 reads sample 5
    assert r['energy'].tolist() == [0.0, 1.0] and r['bounds'] == [4, 6, 1, 0] and r['intervals'].tolist() == [[4, 6]]
    # pad reaches past both ends; two runs, max_iv below the count keeps the first and still counts both
    x = [3, 0, 0, 0, 0, 0, 0, 0, 3, 0]
    r = TO.trim(x, 2, 2, 20.0, pad=100, max_iv=1)
    assert r['energy'].tolist() == [4.5, 0.0, 0.0, 0.0, 4.5, 0.0]
    assert r['bounds'] == [0, 10, 2, 0] and r['n_iv'] == 2 and r['intervals'].tolist() == [[0, 2]] and r['all_intervals'].tolist() == [[0, 2], [8, 10]]
    assert TO.trim(x, 2, 2, 20.0, pad=1)['bounds'] == [0, 10, 2, 0] and TO.trim(x[1:], 2, 2, 20.0)['bounds'][:2] == [8, 9]     # (frame 4 reads x[7], x[8])


def test_oracle_silence_loud_and_non_finite():
    r = TO.trim(np.zeros(11), 4, 2, 60.0, max_iv=2)               # digital silence: every frame is the loudest, kept whole
    assert r['bounds'] == [0, 11, 6, 0] and r['intervals'].tolist() == [[0, 11], [-1, -1]]
    assert TO.trim(np.ones(11), 4, 2, 60.0)['bounds'] == [0, 11, 6, 0]
    for v in (np.nan, np.inf, -np.inf):
        x = np.ones(12)
        x[5] = v
        r = TO.trim(x, 4, 2, 60.0, max_iv=2)
        assert r['bounds'] == [0, 12, -1, 1] and r['n_iv'] == 0 and r['intervals'].tolist() == [[-1, -1]] * 2
        bad = ~np.isfinite(r['energy'])
        assert bad.tolist() == [False, False, True, True, False, False, False]      # frames 2 and 3 read sample 5
        assert np.isnan(r['energy'][bad]).all() if np.isnan(v) else np.isposinf(r['energy'][bad]).all()


def test_oracle_on_the_exact_tie():
    x, bounds, iv = TC.tie_signal()
    assert TO.ratio_of(TC.TIE_TOP_DB) == 2.0 ** -8
    r = TO.trim(x, TC.TIE_FL, TC.TIE_HOP, TC.TIE_TOP_DB, max_iv=1)
    assert r['energy'][[3, 4, 10]].tolist() == [2.0 ** -8] * 3 and r['energy'].max() == 1.0 and r['energy'][5] == 5.0 / 512
    assert r['bounds'] == bounds and r['intervals'].tolist() == iv
    assert TO.margin_db(x, TC.TIE_FL, TC.TIE_HOP, TC.TIE_TOP_DB) == 0.0


def test_single_frame_cases_have_one_non_silent_frame():
    for c in TC.kernel_cases():
        if c['name'].endswith('/single'):
            assert TO.trim(c['x'], c['fl'], c['hop'], c['top_db'])['bounds'][2] == 1, c['name']


# ---------------------------------------------------------------- THE GUARD
def test_guard_every_integer_case_keeps_its_margin():
    """An fp32 sum of n <= 8192 non-negative terms lies within (n + 8) 2^-24 relative of the exact one: under 0.003 dB, once in the
    frame and once in the reference.  A case whose closest frame is 0.01 dB or more from the threshold therefore decides alike in
    fp32 and in float64.  A condition on the table, not a skip: a seed that fails is replaced in tests/trim_cases.py."""
    assert 2 * 10.0 * np.log10(1.0 + (8192 + 8) * 2.0 ** -24) < 0.005 < TC.MARGIN_DB
    cases = TC.integer_cases()
    assert len(cases) > 200 and len({c['name'] for c in cases}) == len(cases)
    low = [(c['name'], m) for c in cases for m in [TO.margin_db(c['x'], c['fl'], c['hop'], c['top_db'])] if not m >= TC.MARGIN_DB]
    assert not low, low
    for c, _, _ in TC.nonfinite_cases():                            # (their finite twins decide the other utterances of that batch)
        assert not np.isfinite(TO.frame_energy(c['x'], c['fl'], c['hop'])).all()


def test_case_table_straddles_the_kernel_constants():
    from semi_tts_amd import ops
    assert (TC.RUN, TC.CHUNK) == (ops.TRIM_RUN, ops.TRIM_CHUNK)
    for fl, hop in TC.FRAMINGS + (TC.WIDE,):
        assert ops.trim_run_length(fl, hop) == TC.RUN
    assert ops.trim_run_length(8192, 512) == 9 and ops.trim_run_length(8192, 8192) == 1 and ops.trim_run_length(2048, 1024) == 11
    frames = {(c['fl'], c['hop']): set() for c in TC.kernel_cases()}
    for c in TC.kernel_cases():
        frames[(c['fl'], c['hop'])].add(1 + len(c['x']) // c['hop'])
    for f in TC.FRAMINGS:
        assert {TC.RUN - 1, TC.RUN, TC.RUN + 1, TC.CHUNK - 1, TC.CHUNK, TC.CHUNK + 1} <= frames[f]


# ---------------------------------------------------------------- ops._trim_check
def test_trim_check_passes_and_ratio():
    from semi_tts_amd import ops
    ops._trim_check(np.array([1, 5]), 2048, 512, 60.0)
    ops._trim_check(np.array([7]), 8192, 1, 0.5, pad=3, max_iv=4)
    assert ops.trim_ratio(60.0) == float(np.float32(1e-6)) and ops.trim_ratio(TC.TIE_TOP_DB) == 2.0 ** -8


@pytest.mark.parametrize('kw, msg', [
    (dict(frame_length=8193), 'needs 1 <= hop <= frame_length <= 8192'),
    (dict(hop=0), 'needs 1 <= hop <= frame_length <= 8192'),
    (dict(frame_length=256, hop=257), 'needs 1 <= hop <= frame_length <= 8192'),
    (dict(hop=2.0), 'hop must be an integer'),
    (dict(frame_length=True), 'frame_length must be an integer'),
    (dict(top_db=0.0), 'strictly inside'),
    (dict(top_db=-3.0), 'strictly inside'),
    (dict(top_db=1e-9), 'strictly inside'),
    (dict(top_db=1000.0), 'strictly inside'),
    (dict(top_db=float('nan')), 'top_db must be a finite number'),
    (dict(top_db='60'), 'top_db must be a finite number'),
    (dict(pad=-1), 'pad -1 outside'),
    (dict(max_iv=-1), 'max_iv -1 outside'),
    (dict(lens=np.array([4, 0])), 'lens must be B >= 1 integers'),
    (dict(lens=np.array([], np.int64)), 'lens must be B >= 1 integers'),
    (dict(lens=np.array([2.0])), 'lens must be B >= 1 integers'),
    (dict(lens=np.array([2 ** 31])), 'lens must be B >= 1 integers'),
])
def test_trim_check_refusals(kw, msg):
    from semi_tts_amd import ops
    args = dict(lens=np.array([100]), frame_length=2048, hop=512, top_db=60.0, pad=0, max_iv=0)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        ops._trim_check(**args)


def test_trim_silence_refuses_host_tensors_before_a_device():
    import torch
    from semi_tts_amd import ops
    with pytest.raises(ValueError, match='packed 1-D contiguous float32 GPU tensor'):
        ops.trim_silence(torch.zeros(10), [0], [10], 4, 2, 60.0)


def test_converter_check_trim():
    from semi_tts_amd.audio import AudioConverter
    conv = AudioConverter(257, 40, 25, 10, 0.97, 16000)
    assert conv._check_trim() == 0 and conv._check_trim(pad_ms=12.5) == 200
    for kw, msg in ((dict(pad_ms=-1.0), 'pad_ms'), (dict(pad_ms=float('inf')), 'pad_ms'), (dict(hop_length=0), 'needs 1 <= hop'),
                    (dict(top_db=0), 'strictly inside')):
        with pytest.raises(ValueError, match=msg):
            conv._check_trim(**kw)


# ---------------------------------------------------------------- the build list
def test_build_lists():
    from semi_tts_amd import build
    assert build.TRIM_SOURCES == ['trim.hip'] and build.PITCH_SOURCES == ['f0.hip'] and len(build.SOURCES) == 20
    assert os.path.isfile(os.path.join(build.CSRC, 'trim.hip'))
    from semi_tts_amd import _lib
    assert 'st_trim_silence' in _lib.SIGNATURES and 'st_trim_run_length' in _lib.SIGNATURES


# ---------------------------------------------------------------- main.py flags
def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


CFG = ['--config', 'x.yaml']


def test_trim_flags_parse():
    entry = _entry()
    p = entry.parse_args(CFG + ['--corpus', '--trim-silence'])
    assert p.trim_silence is True and (p.trim_top_db, p.trim_frame_length, p.trim_hop, p.trim_pad_ms) == (60.0, 2048, 512, 0.0)
    p = entry.parse_args(CFG + ['--corpus'])
    assert p.trim_silence is False and p.trim_wav_dir is None and (p.trim_top_db, p.trim_frame_length, p.trim_hop, p.trim_pad_ms) == (60.0, 2048, 512, 0.0)
    p = entry.parse_args(CFG + ['--transcribe-wav-dir', 'd', '--trim-silence', '--trim-top-db', '40', '--trim-frame-length', '1024', '--trim-hop', '256',
                                '--trim-pad-ms', '12.5'])
    assert (p.trim_top_db, p.trim_frame_length, p.trim_hop, p.trim_pad_ms) == (40.0, 1024, 256, 12.5)
    for mode in (['--unpair-wav-dir', 'd'], ['--mcd-wav-dir', 'd', '--mcd-ref-dir', 'e'], ['--feat-wav-dir', 'd', '--feat', 'mfcc']):
        assert entry.parse_args(CFG + mode + ['--trim-silence']).trim_silence is True
    p = entry.parse_args(CFG + ['--trim-wav-dir', 'a', '--trim-out', 'b', '--trim-top-db', '35'])
    assert (p.trim_wav_dir, p.trim_out, p.trim_top_db, p.trim_silence) == ('a', 'b', 35.0, False)
    from semi_tts_amd.solver import trim_args
    assert trim_args(p) is None
    assert trim_args(entry.parse_args(CFG + ['--corpus', '--trim-silence', '--trim-hop', '128'])) == dict(top_db=60.0, frame_length=2048, hop_length=128,
                                                                                                       pad_ms=0.0)


@pytest.mark.parametrize('argv, msg', [
    (CFG + ['--align-wav-dir', 'd', '--trim-silence'], '--trim-silence does not combine with --align-wav-dir'),
    (CFG + ['--feat-wav-dir', 'd', '--feat', 'mfcc', '--segment-file', 's.csv', '--trim-silence'], '--trim-silence does not combine with --segment-file'),
    (CFG + ['--trim-silence'], '--trim-silence trims what --corpus'),
    (CFG + ['--gen-specgram', '--trim-silence'], '--trim-silence trims what --corpus'),
    (CFG + ['--corpus', '--trim-top-db', '40'], 'they need one of them'),
    (CFG + ['--trim-frame-length', '1024'], 'they need one of them'),
    (CFG + ['--trim-hop', '256'], 'they need one of them'),
    (CFG + ['--trim-pad-ms', '5'], 'they need one of them'),
    (CFG + ['--corpus', '--trim-silence', '--trim-top-db', '0'], '--trim-top-db must be finite and positive'),
    (CFG + ['--corpus', '--trim-silence', '--trim-frame-length', '8193'], '--trim-frame-length <= 8192'),
    (CFG + ['--corpus', '--trim-silence', '--trim-hop', '4096'], '1 <= --trim-hop <= --trim-frame-length'),
    (CFG + ['--corpus', '--trim-silence', '--trim-pad-ms', '-1'], '--trim-pad-ms finite and >= 0'),
    (CFG + ['--trim-wav-dir', 'a'], '--trim-wav-dir needs --trim-out DIR'),
    (['--trim-wav-dir', 'a', '--trim-out', 'b'], '--trim-wav-dir needs --trim-out DIR (the directory to write) and --config'),
    (CFG + ['--trim-wav-dir', 'a', '--trim-out', './a'], '--trim-out must not be the directory --trim-wav-dir reads'),
    (CFG + ['--trim-out', 'b'], '--trim-out belongs to --trim-wav-dir'),
    (CFG + ['--trim-wav-dir', 'a', '--trim-out', 'b', '--trim-silence'], '--trim-wav-dir does not combine with --trim-silence'),
    (CFG + ['--trim-wav-dir', 'a', '--trim-out', 'b', '--transcribe-wav-dir', 'c'], '--trim-wav-dir does not combine with --transcribe-wav-dir'),
    (CFG + ['--trim-wav-dir', 'a', '--trim-out', 'b', '--corpus'], 'it does not combine with --trim-wav-dir'),
])
def test_trim_flag_refusals(argv, msg, capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(argv)
    assert msg in capsys.readouterr().err


def test_trimmer_refuses_before_writing(tmp_path):
    import types
    from semi_tts_amd.audio import write_wav
    from semi_tts_amd.solver import Trimmer
    audio = dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    paras = types.SimpleNamespace(trim_wav_dir=str(src), trim_out=str(dst), trim_top_db=60.0, trim_frame_length=2048, trim_hop=512, trim_pad_ms=0.0,
                                  batch_size=4, verbose=False)
    with pytest.raises(ValueError, match='no .wav files'):
        Trimmer(dict(data=dict(audio=audio)), paras, 'test').load_data()
    write_wav(str(src / 'a.wav'), np.zeros(100), 22050)
    with pytest.raises(ValueError, match='Sample rate mismatch. Expected 16000 but get 22050'):
        Trimmer(dict(data=dict(audio=audio)), paras, 'test').load_data()
    paras.trim_out = str(src)
    with pytest.raises(ValueError, match='is the directory --trim-wav-dir reads'):
        Trimmer(dict(data=dict(audio=audio)), paras, 'test').load_data()
    assert not dst.exists()


# ---------------------------------------------------------------- corpus: re-selection and re-sampling on fake bounds
def _rows(samples):
    from semi_tts_amd.corpus import Utterance
    rows = []
    for k, n in enumerate(samples):
        u = Utterance('u%02d' % k, 's', 0, 'u%02d.wav' % k, n / 100.0, [3, 0])
        u.samples = n
        rows.append(u)
    return rows


def test_sampler_sharded_argument_leaves_the_default_alone():
    from semi_tts_amd.corpus import Sampler
    lengths = [50, 90, 70, 90, 10, 30, 60]
    for rank in (0, 1):
        s = Sampler(lengths, 2, seed=3, rank=rank, world=2)
        assert s.rows.tolist() == np.argsort(-np.asarray(lengths), kind='stable')[rank::2].tolist()
        perm = np.random.RandomState([3, rank, 0]).permutation(len(s.rows))
        assert [b.tolist() for b in s.epoch(0)] == [s.rows[perm[i:i + 2]].tolist() for i in range(0, len(s.rows) - 1, 2)]
    mine = [90, 70, 10, 60]                                        # one rank's rows, already sharded
    s = Sampler(mine, 2, seed=3, rank=1, world=2, sharded=True)
    assert s.rows.tolist() == [0, 1, 3, 2]                        # every row, longest first
    perm = np.random.RandomState([3, 1, 5]).permutation(4)        # still seeded by [seed, rank, epoch]
    assert [b.tolist() for b in s.epoch(5)] == [s.rows[perm[0:2]].tolist(), s.rows[perm[2:4]].tolist()]
    with pytest.raises(ValueError, match='rank 2 of 2'):
        Sampler(mine, 2, rank=2, world=2, sharded=True)


def test_apply_bounds_moves_offsets_drops_and_resamples():
    from semi_tts_amd.corpus import Sampler, apply_bounds, trim_report
    samples = [5000, 9000, 7000, 9000, 1000, 3000, 6000, 8000]
    rows = _rows(samples)
    sampler = Sampler(samples, 2, bucketing=True, train=True, seed=7, rank=1, world=2)
    assert sampler.rows.tolist() == [3, 2, 0, 4]                   # rank 1 of the sort 1, 3, 7, 2, 6, 0, 5, 4
    mine = np.array(sorted(sampler.rows.tolist()))                 # 0, 2, 3, 4
    lens = np.array(samples, np.int64)
    offsets = np.full(8, -1, np.int64)
    offsets[mine] = np.concatenate([[0], np.cumsum(lens[mine])[:-1]])
    #       row 0: [100, 4100)  row 2: [0, 7000) whole  row 3: [500, 700): too short for n_fft 512  row 4: [10, 990)
    start, end = np.array([100, 0, 500, 10]), np.array([4100, 7000, 700, 990])
    new_rows, off, ln, smp, counts = apply_bounds(rows, mine, offsets, lens, start, end, sampler, n_fft=512, hop=128, max_frames=40)
    # row 2 keeps 7000 samples = 55 frames > 40: dropped under the frame limit; row 3 keeps 200 <= 256: short
    assert counts == dict(short=1, tokens=0, frames=1)
    assert [u.id for u in new_rows] == ['u00', 'u04'] and [u.samples for u in new_rows] == [4000, 980]
    assert off.tolist() == [0 + 100, 5000 + 7000 + 9000 + 10] and ln.tolist() == [4000, 980]
    assert rows[0].samples == 5000 and new_rows[0] is not rows[0]  # the corpus' own rows are left as they were
    assert smp.rows.tolist() == [0, 1] and (smp.B, smp.train, smp.bucketing, smp.seed, smp.rank) == (2, True, True, 7, 1)
    assert [b.tolist() for b in smp.epoch(2)] == [[0, 1], [0, 1]]
    without = apply_bounds(rows, mine, offsets, lens, start, end, sampler, n_fft=512, hop=128)
    assert without[4] == dict(short=1, tokens=0, frames=0) and without[2].tolist() == [4000, 7000, 980] and without[3].rows.tolist() == [1, 0, 2]
    with pytest.raises(ValueError, match='no utterance left after trimming'):
        apply_bounds(rows, mine, offsets, lens, start, start + 5, sampler, n_fft=512, hop=128)
    with pytest.raises(ValueError, match='trim bounds outside'):
        apply_bounds(rows, mine, offsets, lens, start, end + 10000, sampler, n_fft=512, hop=128)
    line = trim_report('paired', 1000, 22000, 4980, 4, counts)
    assert line == 'paired: trimmed 22.0 s -> 5.0 s (77.4% removed) | 2 of 4 utterances kept | dropped after trimming: 1 too short, 1 over the frame limit'
