"""Host side of the sample-rate conversion (semi_tts_amd.audio.resample_table / resampled_len / read_wav / load_batch, the flags
of main.py) and the float64 oracle itself (tests/resample_oracle.py): no GPU."""
import itertools
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import resample_oracle as O  # noqa: E402
from semi_tts_amd import audio, ops  # noqa: E402

RATIOS = [(48000, 22050), (44100, 16000), (16000, 22050), (22050, 32000), (2, 1), (1, 2), (48000, 8000)]
RATES = [8000, 16000, 22050, 24000, 32000, 44100, 48000]
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050)


@pytest.mark.parametrize('orig,new', RATIOS)
def test_compact_equals_full(orig, new):
    """the sum over |i - tau| < W and the clamped-window form of 2 ceil(W) + o taps are the same filter"""
    rs = np.random.RandomState(orig % 1000 + new % 7)
    for L in (1, 5, 700):
        x = rs.uniform(-1, 1, L)
        a, b = O.resample_compact(x, orig, new), O.resample_full(x, orig, new)
        assert a.shape == b.shape == (O.out_len(L, orig, new),)
        err = np.abs(a - b).max()
        print('%d -> %d, L %d: compact vs full %.2e' % (orig, new, L, err))
        assert err <= 1e-12


@pytest.mark.parametrize('orig,new', RATIOS)
def test_table_is_the_float64_table_rounded_once(orig, new):
    o, n, taps, first, table = audio.resample_table(orig, new)
    o64, n64, taps64, first64, table64, W = O.table64(orig, new)
    assert (o, n, taps) == (o64, n64, taps64) and taps <= math.floor(2 * W) + 1
    assert first.dtype == np.int32 and np.array_equal(first, first64)
    assert table.dtype == np.float32 and table.shape == (n, taps)
    assert np.array_equal(table.view(np.uint32), table64.astype(np.float32).view(np.uint32))
    assert audio.resample_table(orig, new)[4] is table                     # cached per ratio
    g = 3
    assert audio.resample_table(orig * g, new * g)[4] is table


@pytest.mark.parametrize('orig,new', RATIOS)
def test_out_of_window_entries_are_exactly_zero(orig, new):
    o, n, taps, first, table = audio.resample_table(orig, new)
    W = O.LPW * o / (min(o, n) * O.ROLLOFF)
    for p in range(n):
        tau = Fraction(p * o, n)
        for k in range(taps):
            d = abs(math.floor(tau) + int(first[p]) + k - tau)                  # |i - tau|, exact
            if d >= W:
                assert table[p, k] == 0.0, (p, k)
        # and nothing inside the window is left out of the row
        assert abs(math.floor(tau) + int(first[p]) - 1 - tau) >= W and abs(math.floor(tau) + int(first[p]) + taps - tau) >= W


def test_table_sizes_of_the_issue():
    sizes = {(48000, 22050): (320, 147, 27), (44100, 16000): (441, 160, 34), (22050, 32000): (441, 640, 13)}
    for (orig, new), want in sizes.items():
        assert audio.resample_table(orig, new)[:3] == want
    assert audio.resample_table(22050, 32000)[4].nbytes == 33280


def test_resampled_len():
    for orig, new in RATIOS + [(22050, 22050), (7, 3)]:
        o, n = O.ratio(orig, new)
        for L in [1, 2, 3, o - 1, o, o + 1, 2 * o - 1, 2 * o, 2 * o + 1, 17 * o, 17 * o + 1, 4000, 66150, 2 ** 31 - 1]:
            if L < 1:
                continue
            assert audio.resampled_len(L, orig, new) == math.ceil(Fraction(L * new, orig)) == O.out_len(L, orig, new), (orig, new, L)


def test_the_definition_resamples_a_sine():
    """a 0.5-amplitude 1 kHz sine, 4000 samples, 48000 -> 22050, against the analytic sine away from 200 samples at each end.
    Measured with the float64 definition: 5.2e-5; the bound is the issue's 2e-4."""
    x = 0.5 * np.sin(2 * np.pi * 1000 * np.arange(4000) / 48000)
    y = O.resample_compact(x, 48000, 22050)
    m = np.arange(len(y))
    err = np.abs(y - 0.5 * np.sin(2 * np.pi * 1000 * m / 22050))[200:-200].max()
    print('sine: max error %.2e' % err)
    assert err <= 2e-4
    _, _, _, first, table = audio.resample_table(48000, 22050)
    y32 = O.resample_compact(x, 48000, 22050, table=table, first=first)          # the table the kernel reads
    assert np.abs(y32 - 0.5 * np.sin(2 * np.pi * 1000 * m / 22050))[200:-200].max() <= 2e-4


def test_dc_gain_and_absolute_sum_of_every_phase():
    lo, hi, amax = 2.0, 0.0, 0.0
    for orig, new in itertools.permutations(RATES, 2):
        table = audio.resample_table(orig, new)[4].astype(np.float64)
        gain = table.sum(1)
        lo, hi, amax = min(lo, gain.min()), max(hi, gain.max()), max(amax, np.abs(table).sum(1).max())
    print('DC gain %.5f .. %.5f, sum |h| <= %.3f' % (lo, hi, amax))
    assert 1 - 2e-3 <= lo and hi <= 1 + 2e-3
    assert amax <= 1.87


def test_all_rate_pairs_are_accepted():
    biggest = 0
    for orig, new in itertools.permutations(RATES, 2):
        o, n, taps, first, table = audio.resample_table(orig, new)
        tab_f, stage_f = ops.resample_lds_floats(o, n, taps, int(first.min()), int(first.max()))
        assert tab_f <= ops.RESAMPLE_MAX_TABLE_FLOATS and stage_f <= ops.RESAMPLE_MAX_STAGE_FLOATS
        assert taps <= 73 and o * n < 2 ** 31
        biggest = max(biggest, table.nbytes)
    assert biggest == 33280
    # two workgroups at the limits fit the 160 KB of a compute unit
    assert 2 * 4 * (ops.RESAMPLE_MAX_TABLE_FLOATS + ops.RESAMPLE_MAX_STAGE_FLOATS) <= 160 * 1024


def test_refusals_raise_before_a_device_is_touched():
    for bad in [(0, 22050), (22050, 0), (-8000, 16000), (22050.0, 16000), (True, 16000), ('48000', 22050)]:
        with pytest.raises(ValueError, match='positive integer'):
            audio.resample_table(*bad)
        with pytest.raises(ValueError):
            audio.resample([np.zeros(10, np.float32)], *bad)
    with pytest.raises(ValueError, match='positive integer'):
        audio.resampled_len(10, 0, 5)
    with pytest.raises(ValueError, match='staged'):
        audio.resample_table(48000, 1000)                 # 48 : 1 -- a tile's input span is beyond the stage
    with pytest.raises(ValueError, match='staged'):
        audio.resample_table(44100, 44101)                # 1024 staged rows of 13 taps are beyond the table
    with pytest.raises(ValueError, match='2\\^31'):
        audio.resample_table(3300001, 657)
    with pytest.raises(ValueError):
        audio.resample_table(48000, 22050, lowpass_filter_width=0)
    with pytest.raises(ValueError):
        audio.resample_table(48000, 22050, rolloff=1.5)
    with pytest.raises(ValueError, match='empty batch'):
        audio.resample([], 48000, 22050)
    with pytest.raises(ValueError, match='samples'):
        audio.resample([np.zeros(0, np.float32)], 48000, 22050)
    with pytest.raises(ValueError, match='int16'):
        audio.resample([np.zeros(8, np.int32)], 48000, 22050)


def test_same_rate_returns_the_values_and_launches_nothing():
    """(no GPU here: a launch would raise)"""
    xs = [np.linspace(-1, 1, 50).astype(np.float32), np.arange(-40, 40, dtype=np.int16)]
    wb = audio.resample(xs, 22050, 22050)
    assert isinstance(wb, audio.WaveBatch) and wb.order.tolist() == [1, 0] and wb.lens.tolist() == [80, 50]
    assert torch.equal(wb._wavs[1], torch.from_numpy(xs[0]))
    assert torch.equal(wb._wavs[0], torch.from_numpy(xs[1].astype(np.float32) / 32768))
    assert audio.resample(wb, 44100, 44100) is wb


def _write(path, L, sr, seed, channels=1):
    rs = np.random.RandomState(seed)
    if channels == 1:
        audio.write_wav(str(path), rs.uniform(-0.9, 0.9, L), sr)
        return
    import wave
    pcm = rs.randint(-30000, 30000, (L, channels)).astype('<i2')
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_read_wav(tmp_path):
    _write(tmp_path / 'a.wav', 300, 16000, 0)
    _write(tmp_path / 'b.wav', 200, 48000, 1, channels=2)
    for name, sr, shape in (('a.wav', 16000, (1, 300)), ('b.wav', 48000, (2, 200))):
        w, got_sr = audio.read_wav(str(tmp_path / name))
        assert got_sr == sr and tuple(w.shape) == shape and w.dtype == torch.float32
        assert torch.equal(w, audio.load_wav(str(tmp_path / name), sr))
        assert torch.equal(w, audio.load_wav(str(tmp_path / name)))


def test_load_batch_groups_by_rate(tmp_path, monkeypatch):
    """the grouping, the order and the error text of load_batch, with the device and the kernel call replaced by the CPU and the oracle"""
    conv = audio.load_audio_transform(**AUDIO_CFG)
    spec = [('u0.wav', 300, 22050, 1), ('u1.wav', 900, 48000, 2), ('u2.wav', 500, 16000, 1), ('u3.wav', 400, 48000, 1), ('u4.wav', 250, 22050, 1)]
    for i, (name, L, sr, ch) in enumerate(spec):
        _write(tmp_path / name, L, sr, i, channels=ch)
    paths = [str(tmp_path / s[0]) for s in spec]
    with pytest.raises(ValueError) as e:
        conv.load_batch(paths)
    with pytest.raises(ValueError) as e_ref:
        conv.load(paths[1])
    assert str(e.value) == str(e_ref.value) == 'Sample rate mismatch. Expected 22050 but get 48000 (%s)' % paths[1]
    calls = []

    def fake(wavs, orig_sr, new_sr):
        calls.append((orig_sr, new_sr, [int(w.numel()) for w in wavs]))
        assert all(w.dtype == torch.int16 for w in wavs)
        return audio.WaveBatch([torch.from_numpy(O.resample_compact(w.numpy() / 32768.0, orig_sr, new_sr).astype(np.float32)) for w in wavs])
    monkeypatch.setattr(audio, '_resample', fake)
    monkeypatch.setattr(audio, '_device', lambda: torch.device('cpu'))
    wb = conv.load_batch(paths, resample=True)
    assert calls == [(16000, 22050, [500]), (48000, 22050, [900, 400])]          # one call per foreign rate, channel 0
    want = [300, audio.resampled_len(900, 48000, 22050), audio.resampled_len(500, 16000, 22050), audio.resampled_len(400, 48000, 22050), 250]
    back = np.empty(5, int)
    back[wb.order] = np.arange(5)
    assert [int(wb.lens[back[i]]) for i in range(5)] == want
    assert wb.lens.tolist() == sorted(want, reverse=True)
    for i in (0, 4):                                                            # the files at the converter's rate are load()'s
        assert torch.equal(wb._wavs[back[i]], conv.load(paths[i])[0])
    ch0 = audio.read_wav(paths[1])[0][0].numpy().astype(np.float64)
    assert np.allclose(wb._wavs[back[1]].numpy(), O.resample_compact(ch0, 48000, 22050), atol=1e-6)
    # all files at the converter's rate: resample=True changes nothing
    monkeypatch.setattr(audio, '_resample', None)
    a, b = conv.load_batch([paths[0], paths[4]], resample=True), conv.load_batch([paths[0], paths[4]])
    assert all(torch.equal(x, y) for x, y in zip(a._wavs, b._wavs)) and a.order.tolist() == b.order.tolist() == [0, 1]
    with pytest.raises(ValueError, match='no files'):
        conv.load_batch([])
    # a rate the kernel refuses raises while the files are read, before the device is asked for
    _write(tmp_path / 'odd.wav', 100, 44101, 9)
    monkeypatch.setattr(audio, '_device', lambda: (_ for _ in ()).throw(AssertionError('device touched')))
    with pytest.raises(ValueError, match='staged'):
        conv.load_batch([paths[0], str(tmp_path / 'odd.wav')], resample=True)


FLAG_CASES = [
    (['--config', 'c', '--resample'], 'it needs one of them'),
    (['--config', 'c', '--resample', '--gen-specgram'], 'it needs one of them'),
    (['--config', 'c', '--resample', '--vocode-dir', 'x'], 'it needs one of them'),
    (['--config', 'c', '--resample', '--transcribe-wav-dir', 'x'], None),
    (['--config', 'c', '--resample', '--align-wav-dir', 'x'], None),
    (['--config', 'c', '--resample', '--unpair-wav-dir', 'x'], None),
    (['--resample-wav-dir', 'x', '--resample-out', 'y', '--resample-rate', '16000'], None),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'y'], None),
    (['--resample-wav-dir', 'x', '--resample-out', 'y'], '--resample-rate N or --config'),
    (['--config', 'c', '--resample-wav-dir', 'x'], 'needs --resample-out'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'x'], 'must not be the directory'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', './x/'], 'must not be the directory'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'y', '--resample-rate', '0'], 'positive'),
    (['--config', 'c', '--resample-out', 'y'], 'they need that flag'),
    (['--config', 'c', '--resample-rate', '16000'], 'they need that flag'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'y', '--transcribe-wav-dir', 'z'], 'does not combine with --transcribe-wav-dir'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'y', '--vocode-dir', 'z'], 'does not combine with --vocode-dir'),
    (['--config', 'c', '--resample-wav-dir', 'x', '--resample-out', 'y', '--resample'], 'it needs one of them'),
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
        '        out.append([0, [p.resample, p.resample_wav_dir, p.resample_out, p.resample_rate]])\n'
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
    assert res[6][1] == [False, 'x', 'y', 16000] and res[3][1][0] is True
    # without the new flags nothing changed: the defaults are off
    assert res[7][1] == [False, 'x', 'y', None]


@pytest.mark.parametrize('orig,new', RATIOS + [(8000, 44100), (44100, 48000)])
def test_kernel_index_arithmetic_stays_inside_the_stage(orig, new):
    """resample_kernel's integer arithmetic, restated in numpy for every output of a few lengths: the staged table row of output t
    holds its phase, and the first tap's index into the staged input span lies in [0, span - taps] without the kernel's clamp --
    so every LDS read is inside the stage the host sized (ops.resample_lds_floats) and reads the sample the definition names"""
    o, n, taps, first, _ = audio.resample_table(orig, new)
    tile = ops.RESAMPLE_TILE
    fmin, fmax = int(first.min()), int(first.max())
    R = min(n, tile)
    tab_f, span = ops.resample_lds_floats(o, n, taps, fmin, fmax)
    assert tab_f == R * ((taps | 1) + 1) and span >= taps
    for L in (1, 7, (tile - 1) * o // n, -(-(tile + 1) * o // n), (3 * tile + 5) * o // n + 1):
        M = audio.resampled_len(L, orig, new)
        m = np.arange(M, dtype=np.int64)
        m0 = m // tile * tile
        t = m - m0
        q0, p0 = m0 // n, m0 % n
        s0 = q0 * o + p0 * o // n + fmin                       # the first staged input sample of the tile
        q, p = m // n, m % n
        r = t % R
        assert np.array_equal((p0 + r) % n, p)                 # the rotated row r is phase p
        fl = q * o + p * o // n
        assert np.array_equal(fl, m * o // n)
        base = fl - s0 + first[p]
        assert base.min() >= 0 and base.max() <= span - taps, (L, int(base.min()), int(base.max()), span, taps)
        assert np.array_equal(s0 + base, m * o // n + first[p])
