"""st_loudness_batch / st_wave_gain on the MI355X against the float64 oracle (tests/loudness_oracle.py) on the guarded case table
(tests/loudness_cases.py: tests/test_loudness_host.py checks on the CPU that every block keeps 0.05 LU from both gates), and the layers
above them: AudioConverter.loudness_batch / load_batch(loudness=), corpus.DeviceSplit(loudness=), main.py --loudness-wav-dir,
--feat-wav-dir --normalize-loudness and --vocode-dir --normalize-loudness.

Bounds.  Hop energies: |got - want| <= 2^-23 want + 1e-15 top, top the utterance's largest hop -- one fp32 rounding of a float64
result, plus about 1000 times the 6e-19 top a CPU emulation of the parallel form measured against lfilter, for another summation
order.  Loudness values: 0.01 LU, a tenth of the +-0.1 LU meter tolerance of EBU Tech 3341.  The gating stage fed its own energies:
1e-4 LU (fp32 storage of a float64 result of magnitude <= 100 is 6e-6)."""
import csv
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_cases as CC     # noqa: E402
import loudness_cases as LC   # noqa: E402
import loudness_oracle as LO  # noqa: E402
from helpers import same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
LU = 0.01
AUDIO = dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, preemphasis_coeff=0.97, sample_rate=16000,
             snr_range=[20, 40], time_stretch_range=[0.9, 1.1])
_ORACLE = {}


def _want(c):
    """the oracle's answer for a case, computed once"""
    if c['name'] not in _ORACLE:
        _ORACLE[c['name']] = LO.measure(c['x'], c['fs'], c['target'], c['peak_db'], c['max_gain_db'])
    return _ORACLE[c['name']]


def _pack(cases, x=None, off=None):
    lens = np.array([len(k['x']) for k in cases], np.int64)
    if x is None:
        x = torch.from_numpy(np.concatenate([k['x'] for k in cases])).to(DEV)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return x, np.asarray(off, np.int64), lens


def _run(cases, H_pad=None, x=None, off=None, target='case'):
    """one ops.loudness call on `cases` (one rate, one set of gain arguments) -> device (hop_energy, stats, counts)"""
    from semi_tts_amd import ops
    c = cases[0]
    assert all((k['fs'], k['target'], k['peak_db'], k['max_gain_db']) == (c['fs'], c['target'], c['peak_db'], c['max_gain_db']) for k in cases)
    x, off, lens = _pack(cases, x, off)
    return ops.loudness(x, off, lens, c['fs'], c['target'] if target == 'case' else target, c['peak_db'], c['max_gain_db'], H_pad=H_pad)


def _close(got, want, tol):
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= tol


def _check(c, e, s, n):
    """one utterance's rows (host arrays) against the oracle"""
    want = _want(c)
    H = len(want['e'])
    got = e[:H].astype(np.float64)
    top = want['e'].max() if H else 0.0
    err = np.abs(got - want['e'])
    print('%-28s hops %3d  max |err| / (2^-23 want + 1e-15 top) = %.3g' % (c['name'], H, (err / np.maximum(2.0 ** -23 * want['e'] + 1e-15 * top, 1e-300)).max() if H else 0.0))
    assert (err <= 2.0 ** -23 * want['e'] + 1e-15 * top).all(), (c['name'], float(err.max()))
    assert (e[H:] == 0.0).all(), c['name']
    assert n.tolist() == [want['n_blocks'], want['n_abs'], want['n_rel'], want['flags']], (c['name'], n.tolist(), want['flags'])
    for slot, key in ((0, 'lufs'), (1, 'momentary_max'), (2, 'rel_gate'), (4, 'ungated')):
        assert _close(float(s[slot]), want[key], LU), (c['name'], key, float(s[slot]), want[key])
    assert float(s[3]) == want['peak'], (c['name'], float(s[3]), want['peak'])
    assert abs(float(s[5]) - want['gain']) <= 2.0 ** -22 * want['gain'] + 1.2e-3 * want['gain'] * (want['flags'] == 0), (c['name'], float(s[5]), want['gain'])
    assert s[6] == 0.0 and s[7] == 0.0


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize('fs', LC.RATES + (48000,))
def test_every_case_alone_against_float64(fs):
    """edge lengths around 4 hops and around the run length, noise, a sine, DC across the carry, impulses at the hop seams, a burst
    before digital silence, a quiet middle between the gates, -80 dBFS, zeros, and both gain limits.  (The unlimited gain follows L_I:
    0.01 LU of it are 1.2e-3 of the gain; a limited gain is one rounding of a float64 value.)"""
    from semi_tts_amd import _lib, ops
    assert _lib.load().st_loudness_run_length(fs) == ops.loudness_run_length(fs) == LC.run_of(fs)
    cases = [c for c in LC.kernel_cases() if c['fs'] == fs]
    assert len(cases) == (2 if fs == 48000 else len(LC.length_cases(fs)) + len(LC.signal_cases(fs)))
    for c in cases:
        H = len(c['x']) // LC.hop_of(fs)
        e, s, n = _run([c], H_pad=H + 3)
        assert e.shape == (1, H + 3)
        _check(c, e[0].cpu().numpy(), s[0].cpu().numpy(), n[0].cpu().numpy())


def test_run_length_limits_and_refusals():
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    assert [lib.st_loudness_run_length(f) for f in (7999, 8000, 16000, 22050, 44100, 48000, 48001)] == [0, 4, 7, 9, 18, 19, 0]
    x = torch.zeros(8000, device=DEV)
    with pytest.raises(ValueError, match='H_pad 1 below the 10 hops'):
        ops.loudness(x, [0], [8000], 8000, H_pad=1)
    with pytest.raises(ValueError, match='outside the 8000 packed samples'):
        ops.loudness(x, [4000], [4001], 8000)
    # the C entry itself: -22 before any launch for 65 utterances
    off, lens = np.zeros(65, np.int64), np.full(65, 100, np.int32)
    w = _lib.StWaveBatch(x=x.data_ptr(), n_samples=8000, off=off.ctypes.data, len=lens.ctypes.data, B=65)
    import ctypes
    assert lib.st_loudness_batch(ctypes.byref(w), 8000, x.data_ptr(), -23.0, -1.0, 30.0, x.data_ptr(), 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), None) == -22
    assert b'batch 65 outside' in lib.st_last_error()
    with pytest.raises(ValueError, match='1 .. 64'):
        ops.loudness(x, off, lens.astype(np.int64), 8000)


def test_the_gating_stage_alone():
    """the oracle's gating fed the kernel's own read-back fp32 energies: equal counts, values within 1e-4 LU"""
    for c in LC.kernel_cases():
        e, s, n = _run([c])
        H = len(c['x']) // LC.hop_of(c['fs'])
        want = LO.measure(c['x'], c['fs'], c['target'], c['peak_db'], c['max_gain_db'], energies=e[0, :H].cpu().numpy())
        s, n = s[0].cpu().numpy(), n[0].cpu().numpy()
        assert n.tolist() == [want['n_blocks'], want['n_abs'], want['n_rel'], want['flags']], c['name']
        for slot, key in ((0, 'lufs'), (1, 'momentary_max'), (2, 'rel_gate'), (4, 'ungated')):
            assert _close(float(s[slot]), want[key], 1e-4), (c['name'], key, float(s[slot]), want[key])


@pytest.mark.parametrize('fs', LC.RATES + (48000,))
def test_batch_independence(fs):
    """each case between two full-scale neighbours in a ragged batch of 5 (non-cumulative offsets, NaN-filled gaps) is bitwise what it
    gives alone; so is a repeat of the call"""
    a, b = LC.neighbours(fs)
    cases = [c for c in LC.kernel_cases() if c['fs'] == fs]
    alone = {c['name']: _run([c]) for c in cases + [a, b]}
    for i in range(0, len(cases), 3):
        mid = (cases[i:i + 3] * 3)[:3]
        batch = [a, mid[0], b, mid[1], mid[2]]
        gap = np.full(3, np.nan, np.float32)
        parts, off, pos = [], [], 0
        for k in batch:
            parts += [gap, k['x']]
            off.append(pos + 3)
            pos += 3 + len(k['x'])
        x = torch.from_numpy(np.concatenate(parts + [gap])).to(DEV)
        H_pad = max(len(k['x']) for k in batch) // LC.hop_of(fs) + 2
        e, s, n = _run(batch, H_pad=H_pad, x=x, off=off)
        e2, s2, n2 = _run(batch, H_pad=H_pad, x=x, off=off)
        assert same_bits(e, e2) and same_bits(s, s2) and torch.equal(n, n2)
        for k, c in enumerate(batch):
            e1, s1, n1 = alone[c['name']]
            H = e1.shape[1]
            assert same_bits(e[k, :H], e1[0]) and bool((e[k, H:] == 0).all()), c['name']
            assert same_bits(s[k], s1[0]) and torch.equal(n[k], n1[0]), c['name']


def test_batch_of_64_and_the_split_at_65():
    """B = 64 in one call is bitwise the utterances alone; 65 is refused by ops and split by AudioConverter.loudness_batch"""
    from semi_tts_amd import ops
    from semi_tts_amd.audio import load_audio_transform
    fs = 8000
    pool = LC.ragged_pool(fs, 65)
    e, s, n = _run(pool[:64])
    for k in range(0, 64, 7):
        e1, s1, n1 = _run([pool[k]])
        H = len(pool[k]['x']) // LC.hop_of(fs)
        assert same_bits(e[k, :H], e1[0, :H]) and same_bits(s[k], s1[0]) and torch.equal(n[k], n1[0])
    sh, nh = s.cpu().numpy(), n.cpu().numpy()
    for k in (0, 13, 63):
        _check(pool[k], e[k].cpu().numpy(), sh[k], nh[k])
    with pytest.raises(ValueError, match='1 .. 64'):
        _run(pool)
    conv = load_audio_transform(**dict(AUDIO, sample_rate=fs))
    info = conv.loudness_batch([torch.from_numpy(c['x']) for c in pool])
    for k in (0, 1, 40, 63, 64):                                   # the caller's order, whatever the sort by length did
        want = _want(dict(pool[k], name=pool[k]['name'] + '/measure', target=None))
        assert _close(float(info['lufs'][k]), want['lufs'], LU) and int(info['flags'][k]) == want['flags'] and int(info['n_rel'][k]) == want['n_rel']
        assert float(info['peak'][k]) == want['peak'] and info['gain_db'][k] == 0.0


def test_a_nan_sample_flags_its_utterance_alone():
    c, i = LC.nonfinite_case()
    a, b = LC.neighbours(c['fs'])
    e, s, n = _run([a, c, b])
    hop = LC.hop_of(c['fs'])
    H = len(c['x']) // hop
    got, want = e[1, :H].cpu().numpy().astype(np.float64), LO.hop_energies(c['x'], c['fs'])
    first = i // hop
    assert np.isnan(got[first:]).all() and np.isnan(want[first:]).all()
    assert (np.abs(got[:first] - want[:first]) <= 2.0 ** -23 * want[:first] + 1e-15 * want[:first].max()).all()
    assert n[1].tolist() == [H - 3, 0, 0, 1]
    st = s[1].cpu().numpy()
    assert np.isnan(st[:5]).all() and st[5] == 1.0
    for k, o in ((0, a), (2, b)):
        e1, s1, n1 = _run([o])
        assert same_bits(e[k, :e1.shape[1]], e1[0]) and same_bits(s[k], s1[0]) and torch.equal(n[k], n1[0]) and int(n[k, 3]) == 0
    for v in (np.inf, -np.inf):                                    # an infinity is a non-finite sample too, also in the unmetered tail
        x = c['x'].copy()
        x[i] = 0.0
        x[-1] = v
        e, s, n = _run([dict(c, x=x)])
        assert n[0].tolist() == [H - 3, 0, 0, 1] and float(s[0, 5]) == 1.0 and bool(torch.isnan(s[0, 0]))


# ---------------------------------------------------------------- the gain
def _gain_batch(fs=8000):
    names = ('noise', 'sine997', 'loud_quiet_loud', 'high_crest', 'very_quiet', 'minus80', 'zeros', 'len%d' % (4 * LC.hop_of(fs) - 1), 'impulse0')
    by = {c['name']: c for c in LC.kernel_cases()}
    return [by['%d/%s' % (fs, nm)] for nm in names]


def test_gain_reaches_the_target_and_respects_the_limits():
    from semi_tts_amd import ops
    fs = 8000
    batch = _gain_batch(fs)
    x, off, lens = _pack(batch)
    x0 = x.clone()
    _, s, n = _run(batch)
    y = ops.wave_gain(x, off, lens, s)
    assert same_bits(x, x0)                                        # out of place: the input is untouched
    pcm = ops.wave_gain(x, off, lens, s, pcm16=True)
    z = ops.wave_gain(x, off, lens, s, out=x)                      # in place
    assert z.data_ptr() == x.data_ptr() and same_bits(z, y)
    _, s2, n2 = _run(batch, x=y, off=off, target=None)
    sh, nh, s2h = s.cpu().numpy(), n.cpu().numpy(), s2.cpu().numpy()
    yh, ph = y.cpu().numpy(), pcm.cpu().numpy()
    seen = set()
    for k, c in enumerate(batch):
        sl = slice(int(off[k]), int(off[k] + lens[k]))
        flags, g = int(nh[k, 3]), np.float32(sh[k, 5])
        seen.add(flags)
        assert flags == _want(c)['flags']
        assert np.array_equal(yh[sl].view(np.int32), LO.apply_gain(c['x'], g).view(np.int32)), c['name']      # one fp32 product
        assert np.array_equal(ph[sl], LO.to_pcm16(LO.apply_gain(c['x'], g))), c['name']                       # the .wav writer's formula
        if flags & 7:
            assert g == 1.0 and np.array_equal(yh[sl].view(np.int32), c['x'].view(np.int32))                  # bit for bit the input
        elif flags == 0:
            assert abs(float(s2h[k, 0]) - c['target']) <= LU, (c['name'], float(s2h[k, 0]))
        elif flags == 8:
            ceiling = np.float32(10.0 ** (c['peak_db'] / 20.0))
            assert abs(np.float32(sh[k, 3]) * g - ceiling) <= np.spacing(ceiling), c['name']
            assert float(s2h[k, 0]) < c['target'] and abs(float(s2h[k, 3]) - ceiling) <= np.spacing(ceiling)
        else:
            assert flags == 16 and abs(float(g) - 10.0 ** 1.5) <= 2.0 ** -23 * 10.0 ** 1.5
            assert abs(float(s2h[k, 0]) - (float(sh[k, 0]) + c['max_gain_db'])) <= LU
    assert seen == {0, 2, 4, 8, 16}


def test_measure_only_leaves_the_gain_at_one():
    batch = _gain_batch()
    _, s, n = _run(batch, target=None)
    _, st, nt = _run(batch)
    assert bool((s[:, 5] == 1.0).all()) and not bool((n[:, 3] & 24).any())
    assert same_bits(s[:, :5], st[:, :5]) and torch.equal(n[:, :3], nt[:, :3])


# ---------------------------------------------------------------- the layers above: tiny wavs at 16 kHz
ARGS = dict(target=-23.0, peak_db=-1.0, max_gain_db=30.0)
SR = 16000


def _tone(seed, n, amp):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / float(SR)
    return amp * (np.sin(2 * np.pi * rs.uniform(150, 600) * t) + 0.25 * rs.randn(n))


# (samples, amplitude): a plain one, a quiet one, a short one (under 400 ms: left alone), one with silence at both ends, a loud one
SHAPES = ((9000, 0.2), (12000, 0.01), (5000, 0.3), (11000, 0.1), (8000, 0.6))


def _pcm(path):
    from semi_tts_amd.audio import _read_pcm
    return _read_pcm(path)[0][:, 0]


def _x(path):
    return _pcm(path).astype(np.float32) / 32768.0


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd.audio import load_audio_transform
    return load_audio_transform(**AUDIO)


@pytest.fixture(scope='module')
def wavs(tmp_path_factory):
    from semi_tts_amd.audio import write_wav
    d = tmp_path_factory.mktemp('wavs')
    paths = []
    for k, (n, amp) in enumerate(SHAPES):
        x = _tone(60 + k, n, amp)
        if k == 3:
            x[:2500] *= 1e-4
            x[-2000:] *= 1e-4
        paths.append(str(d / ('utt%d.wav' % k)))
        write_wav(paths[-1], x, SR)
    return paths


def _expect(x, **kw):
    """oracle: (measurement, normalised float32 waveform)"""
    m = LO.measure(x, SR, **dict(ARGS, **kw))
    return m, LO.apply_gain(x, np.float32(m['gain']))


def test_loudness_batch_keeps_the_callers_order_with_one_host_read(conv, wavs, monkeypatch):
    from semi_tts_amd.audio import WaveBatch
    xs = [_x(p) for p in wavs]
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: (reads.append(tuple(t.shape)), real(t, *a, **k))[1])
    info = conv.loudness_batch([torch.from_numpy(x) for x in xs])                  # a list, not sorted by length
    assert len(reads) == 1
    for k, x in enumerate(xs):
        m = LO.measure(x, SR)
        assert _close(float(info['lufs'][k]), m['lufs'], LU) and int(info['flags'][k]) == m['flags'] and float(info['peak'][k]) == m['peak']
        assert [int(info[key][k]) for key in ('n_blocks', 'n_abs', 'n_rel')] == [m['n_blocks'], m['n_abs'], m['n_rel']] and info['gain_db'][k] == 0.0
    assert int(info['flags'][2]) == 2
    # with a target: (dict, WaveBatch); a WaveBatch is normalised in place with the same offsets and lens, a list is left alone
    given = [torch.from_numpy(x).to(DEV) for x in xs]
    keep = [g.clone() for g in given]
    del reads[:]
    info, out = conv.loudness_batch(given, **ARGS)
    assert len(reads) == 1 and all(same_bits(g, k) for g, k in zip(given, keep))
    wb = WaveBatch([torch.from_numpy(x) for x in xs])
    buf = wb.packed(DEV)
    info2, out2 = conv.loudness_batch(wb, **ARGS)
    assert out2.packed(DEV).data_ptr() == buf.data_ptr() and out2.offsets.tolist() == wb.offsets.tolist() and out2.lens.tolist() == wb.lens.tolist()
    monkeypatch.undo()
    y, y2 = out.packed(DEV).cpu().numpy(), buf.cpu().numpy()
    for row, k in enumerate(out.order):
        m, want = _expect(xs[k])
        sl = slice(int(out.offsets[row]), int(out.offsets[row] + out.lens[row]))
        assert abs(float(info['gain_db'][k]) - 20 * math.log10(m['gain'])) <= 1.1 * LU and int(info['flags'][k]) == m['flags'] == int(info2['flags'][row])
        g = np.float32(10.0 ** (info['gain_db'][k] / 20.0))
        assert np.abs(y[sl] - want).max() <= 1.2e-3 * np.abs(want).max() and np.array_equal(y[sl], y2[sl])
        if m['flags'] == 0:
            assert abs(LO.measure(y[sl], SR)['lufs'] - ARGS['target']) <= LU
        elif m['flags'] & 7:
            assert g == 1.0 and np.array_equal(y[sl], xs[k])


def test_load_batch_meters_the_trimmed_span(conv, wavs):
    trim = dict(top_db=30.0, frame_length=128, hop_length=32, pad_ms=1.0)
    use = [wavs[3], wavs[0], wavs[4]]
    wb = conv.load_batch(use, trim=trim, loudness=ARGS)
    plain = conv.load_batch(use, trim=trim)
    assert wb.bounds.tolist() == plain.bounds.tolist() and wb.order.tolist() == plain.order.tolist() and wb.lens.tolist() == plain.lens.tolist()
    a, b = wb.bounds[0]
    assert a > 2000 and b < SHAPES[3][0] - 1500                    # the silence at both ends of utt3 is cut
    y = wb.packed(DEV).cpu().numpy()
    for row, k in enumerate(wb.order):
        lo, hi = wb.bounds[k]
        x = _x(use[k])
        m, want = _expect(x[lo:hi])
        got = y[int(wb.offsets[row]):int(wb.offsets[row] + wb.lens[row])]
        assert _close(float(wb.loudness['lufs'][k]), m['lufs'], LU) and int(wb.loudness['flags'][k]) == m['flags'] == 0
        assert np.abs(got - want).max() <= 1.2e-3 * np.abs(want).max() and abs(LO.measure(got, SR)['lufs'] - ARGS['target']) <= LU
    whole = LO.measure(_x(use[0]), SR)['lufs']
    assert abs(whole - float(wb.loudness['lufs'][0])) > 10 * LU    # metering the untrimmed file would read differently
    measured = conv.load_batch(use, loudness=dict(target=None))
    assert same_bits(measured.packed(DEV), conv.load_batch(use).packed(DEV)) and _close(float(measured.loudness['lufs'][0]), whole, LU)


def test_device_split_normalises_in_place(tmp_path):
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.corpus import load_splits
    toy = CC.write_toy_corpus(tmp_path / 'corpus')
    conv = load_audio_transform(**yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))['data']['audio'])
    assert conv.sr == CC.SR
    lines, plain_lines = [], []
    kw = dict(seed=1)
    _, sets = load_splits(dict(toy[0]), conv, 3, ['paired', 'dev'], dict(paired=4, dev=2), verbose=lines.append, loudness=ARGS, **kw)
    _, plain = load_splits(dict(toy[0]), conv, 3, ['paired', 'dev'], dict(paired=4, dev=2), verbose=plain_lines.append, **kw)
    assert not any('loudness' in ln for ln in plain_lines) and plain['paired'].loudness_report is None
    for name in ('paired', 'dev'):
        ds, ref = sets[name], plain[name]
        report = [ln for ln in lines if ln.startswith(name + ': loudness of')]
        assert len(report) == 1 and report[0] == ds.loudness_report and 'normalised to -23.0 LUFS' in report[0]
        assert ('loudness of %d utterances' % len(ds.rows)) in report[0]
        assert ds.offsets.tolist() == ref.offsets.tolist() and ds.lens.tolist() == ref.lens.tolist() and ds.buffer.numel() == ref.buffer.numel()
        y, x = ds.buffer.cpu().numpy(), ref.buffer.cpu().numpy()
        info = ds.loudness_info
        assert sorted(info['rows'].tolist()) == list(range(len(ds.rows)))
        flags = []
        for k, i in enumerate(info['rows']):
            sl = slice(int(ds.offsets[i]), int(ds.offsets[i] + ds.lens[i]))
            m, want = _expect_sr(x[sl], CC.SR)
            assert _close(float(info['lufs'][k]), m['lufs'], LU) and int(info['flags'][k]) == m['flags']
            assert np.abs(y[sl] - want).max() <= 1.2e-3 * np.abs(want).max()
            flags.append(m['flags'])
            if m['flags'] == 0:
                assert abs(LO.measure(y[sl], CC.SR)['lufs'] - ARGS['target']) <= LU
            elif m['flags'] & 7:
                assert np.array_equal(y[sl], x[sl])
        assert ('%d peak-limited, %d gain-limited | left alone: 0 non-finite, %d under 400 ms, 0 silent' % (flags.count(8), flags.count(16), flags.count(2))) in report[0]
        assert name != 'paired' or (flags.count(0) >= 1 and flags.count(2) >= 1)     # the toy utterances run 0.25 .. 0.6 s: both kinds occur
    mel, aug, lin, text, sid = sets['paired'].fetch()              # and the split still feeds the trainer
    assert mel.shape[0] == 4 and bool(torch.isfinite(mel).all())


def _expect_sr(x, sr):
    m = LO.measure(x, sr, **ARGS)
    return m, LO.apply_gain(x, np.float32(m['gain']))


def _main(argv):
    sys.path.insert(0, REPO)
    import main as entry
    entry.main(argv)


def test_loudness_wav_dir_end_to_end(tmp_path, wavs):
    import shutil
    src, dst, cfg = tmp_path / 'in', tmp_path / 'out', tmp_path / 'c.yaml'
    src.mkdir()
    use = [wavs[0], wavs[1], wavs[2]]                              # plain, quiet, short (flag 2: copied as it is)
    for p in use:
        shutil.copy(p, str(src / os.path.basename(p)))
    cfg.write_text(yaml.safe_dump(dict(data=dict(audio=AUDIO, corpus=dict(batch_size=4)))))
    _main(['--config', str(cfg), '--loudness-wav-dir', str(src), '--loudness-out', str(dst), '--batch-size', '4', '--no-msg', '--loudness-target', '-26'])
    with open(str(dst / 'loudness.csv'), newline='') as f:
        table = list(csv.reader(f))
    assert table[0] == ['file', 'samples', 'seconds', 'lufs', 'momentary_max', 'rel_gate', 'peak_dbfs', 'n_blocks', 'n_abs', 'n_rel', 'gain_db', 'flags']
    assert len(table) == 4 and sorted(os.listdir(str(dst))) == sorted([os.path.basename(p) for p in use] + ['loudness.csv'])
    for row, p in zip(table[1:], sorted(use)):
        x = _x(p)
        m = LO.measure(x, SR, target=-26.0)
        assert row[:3] == [os.path.basename(p), str(len(x)), '%.6f' % (len(x) / float(SR))]
        assert row[7:10] == [str(m['n_blocks']), str(m['n_abs']), str(m['n_rel'])] and row[11] == str(m['flags'])
        for col, want in ((3, m['lufs']), (4, m['momentary_max']), (5, m['rel_gate']), (10, 20 * math.log10(m['gain']))):
            assert _close(float(row[col]), want, LU + 5e-4), (row, col, want)          # (the table prints three decimals)
        assert abs(float(row[6]) - 20 * math.log10(m['peak'])) <= 1e-3
        out = _pcm(str(dst / os.path.basename(p)))
        if m['flags'] & 7:
            assert np.array_equal(out, _pcm(p))                    # a flagged file: its own samples
        else:
            g = np.float32(10.0 ** (float(row[10]) / 20.0))
            assert np.abs(out.astype(np.int64) - LO.to_pcm16(LO.apply_gain(x, np.float32(m['gain']))).astype(np.int64)).max() <= 1 + 1.2e-3 * 32767 * float(g) * m['peak']
            q = out.astype(np.float32) / 32768.0
            extra = abs(LO.measure(LO.to_pcm16(LO.apply_gain(x, np.float32(m['gain']))).astype(np.float32) / 32768.0, SR)['lufs'] - (-26.0))
            assert abs(LO.measure(q, SR)['lufs'] - (-26.0)) <= LU + extra
    # without --loudness-out: the table alone, into the directory read
    _main(['--config', str(cfg), '--loudness-wav-dir', str(src), '--batch-size', '2', '--no-msg', '--loudness-target', '-26'])
    with open(str(src / 'loudness.csv'), newline='') as f:
        assert list(csv.reader(f)) == table
    assert sorted(os.listdir(str(src))) == sorted([os.path.basename(p) for p in use] + ['loudness.csv'])


def test_feat_wav_dir_normalize_loudness_is_extract_batch_of_the_normalised(tmp_path, conv, wavs):
    import shutil
    from semi_tts_amd.audio import SNR_OFF
    src, cfg = tmp_path / 'in', tmp_path / 'c.yaml'
    src.mkdir()
    use = sorted([wavs[0], wavs[1], wavs[4]])
    for p in use:
        shutil.copy(p, str(src / os.path.basename(p)))
    cfg.write_text(yaml.safe_dump(dict(data=dict(audio=AUDIO, corpus=dict(batch_size=4)))))
    _main(['--config', str(cfg), '--feat-wav-dir', str(src), '--feat', 'mel', '--normalize-loudness', '--batch-size', '4', '--no-msg',
           '--logdir', str(tmp_path / 'log'), '--name', 'f'])
    wb = conv.load_batch(use, loudness=ARGS)
    plain = conv.load_batch(use)
    assert not same_bits(wb.packed(DEV), plain.packed(DEV))
    mel = conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)[0].cpu()
    for row, k in enumerate(wb.order):
        got = np.load(str(tmp_path / 'log' / 'f' / (os.path.splitext(os.path.basename(use[k]))[0] + '-mel.npy')))
        frames = 1 + int(wb.lens[row]) // conv.hop_length
        assert got.shape == (frames, AUDIO['num_mels']) and same_bits(torch.from_numpy(got), mel[row, :frames])
        m, want = _expect(_x(use[k]))
        y = wb.packed(DEV)[int(wb.offsets[row]):int(wb.offsets[row] + wb.lens[row])].cpu().numpy()
        assert m['flags'] == 0 and abs(LO.measure(y, SR)['lufs'] - ARGS['target']) <= LU


def test_vocode_dir_normalize_loudness_writes_the_target_level(tmp_path):
    from semi_tts_amd.audio import load_audio_transform
    config = yaml.safe_load(open(os.path.join(REPO, 'config', 'supervised.yaml')))
    conv = load_audio_transform(**config['data']['audio'])
    D = conv.num_freq
    rs = np.random.RandomState(6)
    feats = {k: rs.uniform(0.3, 0.9, (n, D)).astype(np.float32) for k, n in (('a', 48), ('b', 40))}
    d = tmp_path / 'feats'
    os.makedirs(str(d))
    for k, f in feats.items():
        np.save(str(d / ('%s-spec.npy' % k)), f)
    _main(['--config', os.path.join(REPO, 'config', 'supervised.yaml'), '--vocode-dir', str(d), '--vocode-feat', 'spec', '--batch-size', '8',
           '--logdir', str(tmp_path / 'log'), '--name', 'voc', '--seed', '5', '--normalize-loudness', '--no-msg'])
    np.random.seed(5)                                              # main.py seeds np.random with --seed before the solver runs
    raw = conv.vocode_batch([feats[k] for k in sorted(feats)], 'spec')
    reached = 0
    for k, x in zip(sorted(feats), raw):
        x = x.astype(np.float32)
        m = LO.measure(x, conv.sr, **ARGS)
        assert m['flags'] in (0, 8, 16) and m['n_blocks'] >= 1
        level = m['lufs'] + 20 * math.log10(m['gain'])             # the target where no limit applied
        ideal = LO.to_pcm16(LO.apply_gain(x, np.float32(m['gain']))).astype(np.float32) / 32768.0
        extra = abs(LO.measure(ideal, conv.sr)['lufs'] - level)    # what int16 storage (x 32767, read / 32768, rounding, clipping) moves the level by
        got = LO.measure(_x(str(tmp_path / 'log' / 'voc' / (k + '.wav'))), conv.sr)['lufs']
        print('%s: flags %d, level %.4f, file %.4f, int16 term %.5f' % (k, m['flags'], level, got, extra))
        assert abs(got - level) <= LU + extra
        reached += m['flags'] == 0 and abs(level - ARGS['target']) < 1e-9
    assert reached >= 1
