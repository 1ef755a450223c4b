"""st_trim_silence on the MI355X against the float64 oracle (tests/trim_oracle.py) on the guarded case table (tests/trim_cases.py:
tests/test_trim_host.py checks on the CPU that every case whose integers are compared keeps 0.01 dB from the threshold), and the
layers above it: AudioConverter.trim_batch / load_batch(trim=), corpus.DeviceSplit(trim=), main.py --corpus --trim-silence and
--trim-wav-dir.

Energy bound: an fp32 sum of n non-negative terms in any order lies within (n - 1) u of the exact one to first order, the squares add
one rounding each and the quotient one more: |got - want| <= (frame_length + 8) 2^-24 want."""
import csv
import os
import sys
import types

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_cases as CC   # noqa: E402
import trim_cases as TC     # noqa: E402
import trim_oracle as TO    # noqa: E402
from helpers import same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _run(cases, T_pad=None, energy=None, x=None, off=None):
    """one ops.trim_silence call on `cases` (one framing, one top_db / pad / max_iv) packed back to back -> host (energy, bounds, iv, n_iv)"""
    from semi_tts_amd import ops
    c = cases[0]
    assert all((k['fl'], k['hop'], k['top_db'], k['pad'], k['max_iv']) == (c['fl'], c['hop'], c['top_db'], c['pad'], c['max_iv']) for k in cases)
    lens = np.array([len(k['x']) for k in cases], np.int64)
    if x is None:
        x = torch.from_numpy(np.concatenate([k['x'] for k in cases])).to(DEV)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    e, b, iv, n = ops.trim_silence(x, off, lens, c['fl'], c['hop'], c['top_db'], pad=c['pad'], max_iv=c['max_iv'], T_pad=T_pad, energy=energy)
    return e.cpu(), b.cpu().numpy(), None if iv is None else iv.cpu().numpy(), None if n is None else n.cpu().numpy()


def _check(c, e, b, iv, n):
    """one utterance's row of a call against the oracle: energy within the bound (zero frames and padding rows exactly 0), integers equal"""
    want = TO.trim(c['x'], c['fl'], c['hop'], c['top_db'], c['pad'], c['max_iv'])
    T = len(want['energy'])
    got = e[:T].double().numpy()
    tol = (c['fl'] + 8) * 2.0 ** -24 * want['energy']
    assert (np.abs(got - want['energy']) <= tol).all(), (c['name'], float(np.abs(got - want['energy']).max()))
    assert (got[want['energy'] == 0.0] == 0.0).all() and bool((e[T:] == 0).all()), c['name']
    assert b.tolist() == want['bounds'], (c['name'], b.tolist(), want['bounds'])
    if c['max_iv']:
        assert int(n) == want['n_iv'] and iv.tolist() == want['intervals'].tolist(), (c['name'], int(n), iv.tolist(), want['n_iv'])


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize('framing', TC.FRAMINGS + (TC.WIDE,), ids=lambda f: '%dx%d' % f)
def test_every_case_alone_against_float64(framing):
    """edge lengths, speech at both ends, a single non-silent frame, digital silence, a uniformly loud signal, pad past both ends, several
    bursts with max_iv below / at / above the run count, frame counts around st_trim_run_length and around launch 2's chunk of 256"""
    from semi_tts_amd import _lib, ops
    assert _lib.load().st_trim_run_length(*framing) == ops.trim_run_length(*framing) == TC.RUN
    cases = [c for c in TC.kernel_cases() if (c['fl'], c['hop']) == framing]
    assert len(cases) == (1 if framing == TC.WIDE else len(TC.framing_cases(*framing)))
    for c in cases:
        T = 1 + len(c['x']) // c['hop']
        buf = torch.full((1, T + 5), float('nan'), device=DEV)      # rows past T_b: exactly 0, written into a NaN-filled buffer
        e, b, iv, n = _run([c], T_pad=T + 5, energy=buf)
        assert same_bits(e, buf) and not bool(torch.isnan(buf).any())
        _check(c, e[0], b[0], None if iv is None else iv[0], None if n is None else n[0])
        if 'silence' in c['name']:
            assert b[0].tolist() == [0, len(c['x']), T, 0] and bool((e == 0).all())
        if c['name'].endswith('/single'):
            assert b[0][2] == 1


def test_the_exact_tie():
    """a frame at exactly ref * ratio is silent (the comparison is strict), its neighbour one block louder is not"""
    from semi_tts_amd import ops
    x, bounds, iv = TC.tie_signal()
    assert ops.trim_ratio(TC.TIE_TOP_DB) == 2.0 ** -8
    c = dict(name='tie', fl=TC.TIE_FL, hop=TC.TIE_HOP, top_db=TC.TIE_TOP_DB, pad=0, max_iv=2, x=x)
    e, b, got_iv, n = _run([c])
    want = TO.trim(x, TC.TIE_FL, TC.TIE_HOP, TC.TIE_TOP_DB)['energy']
    assert e[0].double().numpy().tolist() == want.tolist()        # power-of-two blocks: every energy exact in fp32
    assert e[0, 3] == e[0, 4] == e[0, 10] == 2.0 ** -8 and e[0].max() == 1.0
    assert b[0].tolist() == bounds and int(n[0]) == 1 and got_iv[0].tolist() == iv + [[-1, -1]]


@pytest.mark.parametrize('spec', TC.POOLS, ids=lambda s: 'B%d_%dx%d' % s[:3])
def test_batch_independence(spec):
    """every utterance of a ragged batch (B = 65 goes out in two calls) is bitwise what it gives alone, and what the oracle says"""
    cases = TC.pool(*spec)
    T_pad = max(1 + len(c['x']) // c['hop'] for c in cases) + 3
    e, b, iv, n = _run(cases, T_pad=T_pad)
    for k, c in enumerate(cases):
        T = 1 + len(c['x']) // c['hop']
        e1, b1, iv1, n1 = _run([c])
        assert same_bits(e[k, :T], e1[0]) and bool((e[k, T:] == 0).all()), c['name']
        assert b[k].tolist() == b1[0].tolist() and iv[k].tolist() == iv1[0].tolist() and n[k] == n1[0], c['name']
        _check(c, e[k], b[k], iv[k], n[k])


def test_window_with_loud_neighbours_reads_zeros_not_neighbours():
    """non-cumulative, unaligned offsets into a larger buffer where loud samples sit directly before and after a quiet utterance"""
    q = TC.neighbour_case()
    other = TC.pool(3, 64, 16, 21)
    rs = np.random.RandomState(5)
    loud = lambda n: rs.uniform(-0.9, 0.9, n).astype(np.float32)      # noqa: E731
    parts = [loud(1001), other[2]["x"], loud(38), q['x'], loud(2003), other[0]['x'], loud(5)]
    starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    x = torch.from_numpy(np.concatenate(parts)).to(DEV)
    cases = [dict(c, top_db=q['top_db'], pad=q['pad'], max_iv=q['max_iv']) for c in (q, other[0], other[2])]
    off = np.array([starts[3], starts[5], starts[1]])
    assert off[0] % 4 != 0 and (np.diff(off) < 0).any()
    e, b, iv, n = _run(cases, x=x, off=off)
    for k, c in enumerate(cases):
        e1, b1, iv1, n1 = _run([c])
        T = e1.shape[1]
        assert same_bits(e[k, :T], e1[0]) and b[k].tolist() == b1[0].tolist() and iv[k].tolist() == iv1[0].tolist() and n[k] == n1[0], c['name']
    _check(q, e[0], b[0], iv[0], n[0])
    assert 0 < b[0][0] < b[0][1] < len(q['x'])                     # the quiet utterance was trimmed on its own burst


def test_non_finite_samples_mark_their_frames_and_their_utterance_alone():
    others = TC.pool(3, 64, 16, 21)
    for c, i, v in TC.nonfinite_cases():
        batch = [dict(o, top_db=c['top_db'], pad=c['pad'], max_iv=c['max_iv']) for o in others[:2]] + [c] + \
                [dict(others[2], top_db=c['top_db'], pad=c['pad'], max_iv=c['max_iv'])]
        e, b, iv, n = _run(batch)
        L, T = len(c['x']), 1 + len(c['x']) // c['hop']
        want = TO.frame_energy(c['x'], c['fl'], c['hop'])
        got = e[2, :T].double().numpy()
        reads = np.array([t * c['hop'] - c['fl'] // 2 <= i < t * c['hop'] - c['fl'] // 2 + c['fl'] for t in range(T)])
        assert reads.sum() == 4 and (np.isnan(got) == reads).all() if np.isnan(v) else (np.isposinf(got) == reads).all()
        assert (np.isnan(want) == np.isnan(got)).all() and (np.isposinf(want) == np.isposinf(got)).all()
        ok = ~reads
        assert (np.abs(got[ok] - want[ok]) <= (c['fl'] + 8) * 2.0 ** -24 * want[ok]).all()
        assert b[2].tolist() == [0, L, -1, 1] and n[2] == 0 and (iv[2] == -1).all()
        for k in (0, 1, 3):
            e1, b1, iv1, n1 = _run([batch[k]])
            assert same_bits(e[k, :e1.shape[1]], e1[0]) and b[k].tolist() == b1[0].tolist() and b[k][3] == 0 and iv[k].tolist() == iv1[0].tolist()
            _check(batch[k], e[k], b[k], iv[k], n[k])


def test_c_entry_refuses_before_a_launch():
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    assert lib.st_trim_run_length(8193, 1) == 0 and lib.st_trim_run_length(64, 65) == 0 and lib.st_trim_run_length(8192, 512) == 9
    x = torch.zeros(100, device=DEV)
    with pytest.raises(ValueError, match='T_pad 3 below the 7 frames'):
        ops.trim_silence(x, [0], [100], 64, 16, 30.0, T_pad=3)
    with pytest.raises(ValueError, match='outside the 100 packed samples'):
        ops.trim_silence(x, [50], [51], 64, 16, 30.0)


# ---------------------------------------------------------------- the layers above: tiny wavs at 16 kHz, n_fft 512
AUDIO = dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000,
             snr_range=[20, 40], time_stretch_range=[0.9, 1.1])
TRIM = dict(top_db=30.0, frame_length=128, hop_length=32, pad_ms=1.0)
PAD = 16                                                            # 1 ms at 16 kHz
R = 3


def _utterance(seed, lead, speech, tail):
    rs = np.random.RandomState(seed)
    t = np.arange(speech) / 16000.0
    tone = 0.4 * np.sin(2 * np.pi * rs.uniform(150, 600) * t) + 0.1 * rs.randn(speech)
    return np.concatenate([1e-4 * rs.randn(lead), tone, 1e-4 * rs.randn(tail)])


SHAPES = ((700, 3000, 900), (0, 2500, 1300), (1500, 4100, 0), (400, 20, 2000), (1000, 3600, 1000), (350, 2800, 420))     # [3]: too short once trimmed


def _pcm(path):
    from semi_tts_amd.audio import _read_pcm
    return _read_pcm(path)[0][:, 0]


def _oracle_bounds(pcm):
    x = pcm.astype(np.float32) / 32768.0
    assert TO.margin_db(x, TRIM['frame_length'], TRIM['hop_length'], TRIM['top_db']) >= TC.MARGIN_DB
    return TO.trim(x, TRIM['frame_length'], TRIM['hop_length'], TRIM['top_db'], pad=PAD, max_iv=0)['bounds'][:2]


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd.audio import load_audio_transform
    return load_audio_transform(**AUDIO)


@pytest.fixture(scope='module')
def wavs(tmp_path_factory):
    from semi_tts_amd.audio import write_wav
    d = tmp_path_factory.mktemp('wavs')
    paths = []
    for k, s in enumerate(SHAPES):
        paths.append(str(d / ('utt%d.wav' % k)))
        write_wav(paths[-1], _utterance(40 + k, *s), 16000)
    return paths


def test_load_batch_trim_then_features_equal_hand_sliced(conv, wavs):
    from semi_tts_amd.audio import WaveBatch
    use = [p for k, p in enumerate(wavs) if k != 3]
    bounds = [_oracle_bounds(_pcm(p)) for p in use]
    wb = conv.load_batch(use, trim=TRIM)
    assert wb.bounds.tolist() == bounds and all(0 <= a < b <= len(_pcm(p)) for (a, b), p in zip(bounds, use))
    assert sum(b - a for a, b in bounds) < sum(len(_pcm(p)) for p in use) - 3000      # something was cut
    plain = conv.load_batch(use)
    hand = WaveBatch([torch.from_numpy(_pcm(p)[a:b].astype(np.float32) / 32768.0).to(DEV) for p, (a, b) in zip(use, bounds)])
    assert wb.order.tolist() == hand.order.tolist() and wb.lens.tolist() == hand.lens.tolist()
    assert wb.packed(DEV).numel() == plain.packed(DEV).numel()      # the window lives in the untrimmed buffer: nothing copied
    kw = dict(r=R, seed=777, snr=[25.0, None, 30.0, 35.0, None], stretch=[1.0, 0.93, 1.05, 1.0, 1.1])
    got, want = conv.extract_batch(wb, **kw), conv.extract_batch(hand, **kw)
    assert all(g.shape == w.shape and same_bits(g, w) for g, w in zip(got, want))
    # the short rule: utt3 keeps 20 + 2 * 16 + framing slack <= n_fft // 2 samples: returned whole and counted
    out, b, n_short, iv = conv.trim_batch([torch.from_numpy(_pcm(p).astype(np.float32) / 32768.0) for p in wavs], with_intervals=True, **TRIM)
    a3, b3 = _oracle_bounds(_pcm(wavs[3]))
    assert b3 - a3 <= conv.n_fft // 2 and n_short == 1 and b[3].tolist() == [0, len(_pcm(wavs[3]))]
    assert [x.tolist() for k, x in enumerate(b) if k != 3] == bounds
    for k, p in enumerate(wavs):
        x = _pcm(p).astype(np.float32) / 32768.0
        assert iv[k].tolist() == TO.trim(x, TRIM['frame_length'], TRIM['hop_length'], TRIM['top_db'])['all_intervals'].tolist()
        assert conv.nonsilent_intervals(torch.from_numpy(x)[None], TRIM['top_db'], TRIM['frame_length'], TRIM['hop_length']).tolist() == iv[k].tolist()


@pytest.fixture(scope='module')
def toy16(tmp_path_factory, wavs):
    """a corpus of the six utterances above as the paired split (speaker directories, tables) plus two each for unpaired and dev"""
    from semi_tts_amd.audio import write_wav
    root = tmp_path_factory.mktemp('corpus16')
    rows = []
    for k, s in enumerate(SHAPES + ((200, 2600, 300), (900, 3300, 100), (100, 2900, 700), (640, 3100, 0))):
        split = 'paired' if k < 6 else 'unpaired' if k < 8 else 'dev'
        rows.append(dict(id='u%02d' % k, speaker='lj' if k % 2 else 'p225', split=split, samples=sum(s), phn_seq='AA B' if k % 3 else 'CH  D EH',
                         tokens=[3, 4, 0] if k % 3 else [5, 1, 6, 7, 0]))
    cfg = CC.write_tables(root, rows)
    for k, (r, s) in enumerate(zip(rows, SHAPES + ((200, 2600, 300), (900, 3300, 100), (100, 2900, 700), (640, 3100, 0)))):
        d = os.path.join(cfg['path'], r['speaker'])
        os.makedirs(d, exist_ok=True)
        write_wav(os.path.join(d, r['id'] + '.wav'), _utterance(40 + k, *s), 16000)
    return cfg, rows


def _splits16(toy16, conv, **kw):
    from semi_tts_amd.corpus import load_splits
    lines = []
    out = load_splits(dict(toy16[0]), conv, R, ['paired', 'unpaired', 'dev'], dict(paired=3, unpaired=2, dev=2), seed=1, verbose=lines.append, **kw)
    return out[1], lines


def test_device_split_trim_fetch_equals_hand_trimmed(toy16, conv):
    from semi_tts_amd.audio import WaveBatch
    sets, lines = _splits16(toy16, conv, trim=TRIM)
    ds = sets['paired']
    by = {r['id']: os.path.join(toy16[0]['path'], r['speaker'], r['id'] + '.wav') for r in toy16[1]}
    assert ds.trim_counts == dict(short=1, tokens=0, frames=0) and [u.id for u in ds.rows] == ['u00', 'u01', 'u02', 'u04', 'u05']      # u03 dropped
    bounds = {u.id: _oracle_bounds(_pcm(by[u.id])) for u in ds.rows}
    assert ds.lens.tolist() == [bounds[u.id][1] - bounds[u.id][0] for u in ds.rows] == [u.samples for u in ds.rows]
    assert ds.buffer.numel() == sum(r['samples'] for r in toy16[1] if r['split'] == 'paired')       # the trimmed samples stay resident
    assert sorted(ds.sampler.rows.tolist()) == list(range(5)) and (np.diff(ds.lens[ds.sampler.rows]) <= 0).all()
    report = [ln for ln in lines if ln.startswith('paired: trimmed')]
    assert len(report) == 1 and '4 of' not in report[0] and '5 of 6 utterances kept | dropped after trimming: 1 too short, 0 over the frame limit' in report[0]
    assert sum(ln.startswith(('unpaired: trimmed', 'dev: trimmed')) for ln in lines) == 2 and sets['dev'].trim_counts['short'] == 0
    for _ in range(3):
        mel, aug, lin, text, sid = ds.fetch()
        ids, seed, snr, stretch = ds.last_fetch
        hand = WaveBatch([torch.from_numpy(_pcm(by[i])[bounds[i][0]:bounds[i][1]].astype(np.float32) / 32768.0).to(DEV) for i in ids])
        assert hand.order.tolist() == list(range(len(ids)))       # the batch comes longest first by TRIMMED length
        want = conv.extract_batch(hand, r=R, seed=seed, snr=snr, stretch=stretch)
        assert all(g.shape == w.shape and same_bits(g, w) for g, w in zip((mel, aug, lin), want))
        rows = {r['id']: r for r in toy16[1]}
        assert sid.tolist() == [CC.SPEAKERS[rows[i]['speaker']] for i in ids] and text.shape[0] == len(ids)


def test_device_split_without_trim_is_todays_fetch(toy16, conv):
    sets, lines = _splits16(toy16, conv)
    ds = sets['paired']
    assert not any('trimmed' in ln for ln in lines) and ds.trim_report is None and len(ds.rows) == 6
    by = {r['id']: os.path.join(toy16[0]['path'], r['speaker'], r['id'] + '.wav') for r in toy16[1]}
    assert ds.sampler.rows.tolist() == np.argsort(-np.array([r['samples'] for r in toy16[1][:6]]), kind='stable').tolist()
    for _ in range(2):
        mel, aug, lin, text, sid = ds.fetch()
        ids, seed, snr, stretch = ds.last_fetch
        want = conv.extract_batch(conv.load_batch([by[i] for i in ids]), r=R, seed=seed, snr=snr, stretch=stretch)
        assert all(same_bits(g, w) for g, w in zip((mel, aug, lin), want))


def test_drops_after_trimming_are_counted(toy16, conv):
    """the short rule and the frame limit run again on the TRIMMED lengths: a limit the longest trimmed utterance alone exceeds drops it"""
    from semi_tts_amd.corpus import Corpus, DeviceSplit, Sampler
    sets, _ = _splits16(toy16, conv, trim=TRIM)
    keep = sorted(sets['paired'].lens.tolist())
    limit = 1 + keep[-2] // conv.hop_length
    assert 1 + keep[-1] // conv.hop_length > limit
    rows = Corpus(**dict(toy16[0])).measure('paired', conv.sr)
    ds = DeviceSplit(conv, rows, Sampler([u.samples for u in rows], 3, seed=1), R, name='paired', trim=TRIM, max_frames=limit)
    assert ds.trim_counts == dict(short=1, tokens=0, frames=1) and len(ds.rows) == 4 and max(ds.lens.tolist()) == keep[-2]
    assert 'dropped after trimming: 1 too short, 1 over the frame limit' in ds.trim_report
    ds.fetch()
    assert len(ds.last_fetch[0]) == 3 and set(ds.last_fetch[0]) <= {u.id for u in ds.rows}


def test_two_corpus_cycle_steps_with_trim_silence(tmp_path):
    import math
    from semi_tts_amd import solver
    toy = CC.write_toy_corpus(tmp_path / 'corpus')
    config = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    config['data']['corpus'] = dict(toy[0])
    paras = types.SimpleNamespace(name='t', logdir=str(tmp_path), ckpdir=str(tmp_path), load=None, seed=1, cpu=False, verbose=False, batch_size=4,
                                  unpair_batch_size=3, frames=64, n_batches=1, dev_batches=0, valid_step=None, max_step=2, store_best_per=False,
                                  corpus=True, actual_len=False, trim_silence=True, trim_top_db=20.0, trim_frame_length=2048, trim_hop=512, trim_pad_ms=0.0)
    tr = solver.VqvaeTrainer(config, paras, 'train')
    tr.load_data()
    assert all(s.trim_report is not None for s in tr.corpus_sets.values())
    tr.set_model()
    log = tr.exec()
    assert [st['kind'] for st in log] == ['speech_first', 'text_first']
    assert all(math.isfinite(st['loss']) and math.isfinite(st['grad_norm']) for st in log)


def test_trim_wav_dir_end_to_end(tmp_path, wavs):
    import shutil
    sys.path.insert(0, REPO)
    import main as entry
    src, dst, cfg = tmp_path / 'in', tmp_path / 'out', tmp_path / 'c.yaml'
    src.mkdir()
    for p in wavs:
        shutil.copy(p, str(src / os.path.basename(p)))
    cfg.write_text(yaml.safe_dump(dict(data=dict(audio=AUDIO, corpus=dict(batch_size=4)))))
    entry.main(['--config', str(cfg), '--trim-wav-dir', str(src), '--trim-out', str(dst), '--batch-size', '4', '--no-msg', '--trim-top-db', '30',
                '--trim-frame-length', '128', '--trim-hop', '32', '--trim-pad-ms', '1'])
    with open(str(dst / 'trim.csv'), newline='') as f:
        table = list(csv.reader(f))
    assert table[0] == ['file', 'samples', 'start', 'end', 'seconds', 'kept_seconds', 'n_intervals'] and len(table) == 1 + len(wavs)
    for row, p in zip(table[1:], sorted(wavs)):
        pcm = _pcm(p)
        a, b = _oracle_bounds(pcm)
        if b - a <= 256:                                           # (utt3: kept whole, trim_batch's short rule)
            a, b = 0, len(pcm)
        n_iv = TO.trim(pcm.astype(np.float32) / 32768.0, 128, 32, 30.0)['n_iv']
        assert row == [os.path.basename(p), str(len(pcm)), str(a), str(b), '%.6f' % (len(pcm) / 16000.0), '%.6f' % ((b - a) / 16000.0), str(n_iv)]
        out = _pcm(str(dst / os.path.basename(p)))
        assert out.dtype == pcm.dtype and np.array_equal(out, pcm[a:b])       # the exact int16 slice
    assert sorted(os.listdir(str(dst))) == sorted([os.path.basename(p) for p in wavs] + ['trim.csv'])
