"""st_resample_batch / semi_tts_amd.audio.resample on the MI355X against the float64 oracle of tests/resample_oracle.py evaluated on
the float32 table the kernel reads, and the --resample / --resample-wav-dir paths end to end.

The bound of every comparison with the oracle is derived, not measured: an output is one chain of K fused multiply-adds over
the K taps (K roundings, the first of them the rounding of a product), so |got - ref| <= (K + 2) 2^-24 sum_k |h_p[k] x[i_k]| with
the right-hand side evaluated in float64 (at sum |h| <= 1.87 and K <= 73 about 8e-6 max|x| at worst)."""
import functools
import os
import sys
import wave

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
import resample_oracle as O  # noqa: E402
from semi_tts_amd import audio, ops  # noqa: E402
from semi_tts_amd.audio import SNR_OFF  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = ops.RESAMPLE_TILE
RATIOS = [(48000, 22050), (44100, 16000), (16000, 22050), (22050, 32000), (2, 1), (1, 2), (48000, 8000)]
LIN_TOL, MEL_TOL = 5e-4, 1e-4               # the tolerances of tests/test_gpu_features.py
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


def _speech(L, seed, sr):
    """the generator of tests/test_gpu_features.py at a rate of its own: harmonic tone with gated silences, |x| < 1"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / float(max(sr, 8000))
    f0 = 100 + 150 * rs.rand()
    x = sum(0.4 / (h + 1) * np.sin(2 * np.pi * f0 * (h + 1) * t + rs.rand()) for h in range(6))
    gate = (np.sin(2 * np.pi * 2 * t + 6 * rs.rand()) > -0.2)
    return (0.7 * x * gate + 0.002 * rs.randn(L)).astype(np.float32)


def _ramp(L):
    """int16 PCM from -32767 to 32767"""
    return np.rint(np.linspace(-32767, 32767, L)).astype(np.int16)


def _lengths(orig, new):
    """input lengths whose outputs straddle the kernel's tile (L_out = TILE - 1, TILE, TILE + 1, 2 TILE + 3 where the ratio reaches
    them, else the nearest lengths on both sides), a single sample, and an utterance shorter than the filter's half width W"""
    o, n = O.ratio(orig, new)
    W = O.LPW * o / (min(o, n) * O.ROLLOFF)
    Ls = set()
    for target in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        Ls.update((max(1, target * o // n), -(-target * o // n)))
    return sorted(Ls) + [1, max(2, int(W) - 1)]


@functools.lru_cache(maxsize=None)
def _case(orig, new):
    """the ragged batch of one ratio and its oracle, computed once: (float32 waves, oracle outputs, bounds); the last wave is the PCM ramp"""
    Ls = _lengths(orig, new)
    waves = [_speech(L, 7 * i + orig % 13, orig) for i, L in enumerate(Ls)]
    waves.append((_ramp(Ls[-3]).astype(np.float32) / 32768.0))            # the PCM ramp, as the floats it stands for
    _, _, taps, first, table = audio.resample_table(orig, new)
    refs, bounds = [], []
    for w in waves:
        y, s_abs = O.resample_compact(w, orig, new, table=table, first=first, want_abs=True)
        refs.append(y)
        bounds.append((taps + 2) * 2.0 ** -24 * s_abs)
    return waves, refs, bounds


def _rows(wb):
    """a WaveBatch on the device -> its utterances as numpy arrays in the caller's order"""
    y = wb.packed(wb.device).cpu().numpy()
    out = [None] * len(wb.lens)
    for row, k in enumerate(wb.order):
        out[k] = y[wb.offsets[row]:wb.offsets[row] + wb.lens[row]]
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('orig,new', RATIOS)
def test_ragged_batch_against_the_oracle(orig, new):
    """checks 1 and 5: every output within the derived bound of the float64 sum over the float32 table; lengths, offsets and
    the longest-first order are those of resampled_len"""
    waves, refs, bounds = _case(orig, new)
    wb = audio.resample([torch.from_numpy(w) for w in waves], orig, new)
    assert isinstance(wb, audio.WaveBatch) and wb.device is not None and wb.packed(wb.device).is_cuda
    want = [audio.resampled_len(len(w), orig, new) for w in waves]
    assert [len(r) for r in refs] == want
    assert wb.order.tolist() == np.argsort(-np.array(want), kind='stable').tolist()
    assert wb.lens.tolist() == [want[k] for k in wb.order]
    assert wb.offsets.tolist() == np.concatenate([[0], np.cumsum(wb.lens)[:-1]]).tolist()
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE + 3} <= set(want) or new > orig            # (an upsampler skips output lengths)
    assert min(want) <= 2 and max(want) > 2 * TILE
    worst, worst_ratio = 0.0, 0.0
    for got, ref, bound, w in zip(_rows(wb), refs, bounds, waves):
        err = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, err.max())
        worst_ratio = max(worst_ratio, (err / np.maximum(bound, 1e-300)).max())
        assert np.all(err <= bound), (orig, new, len(w), float(err.max()), int(np.argmax(err - bound)))
    print('%d -> %d: max |got - ref| %.3e, at most %.3f of the bound' % (orig, new, worst, worst_ratio))


@pytest.mark.parametrize('orig,new', RATIOS)
def test_alone_equals_in_the_batch_and_repeats(orig, new):
    """checks 2 and 4: an utterance resampled alone has the bits of its row in the ragged batch, whatever its position; a batch of
    three in another order too; two calls give identical bytes"""
    waves, _, _ = _case(orig, new)
    ts = [torch.from_numpy(w).to(DEV) for w in waves]
    batch = _rows(audio.resample(ts, orig, new))
    again = _rows(audio.resample(ts, orig, new))
    for k, t in enumerate(ts):
        alone = _rows(audio.resample([t], orig, new))[0]
        assert _same_bits(alone, batch[k]), (orig, new, k)
        assert _same_bits(again[k], batch[k]), (orig, new, k)
    pick = [4, 0, len(ts) - 1]                                             # unsorted: short, long, the ramp
    three = _rows(audio.resample([ts[k] for k in pick], orig, new))
    for got, k in zip(three, pick):
        assert _same_bits(got, batch[k]), (orig, new, k)


@pytest.mark.parametrize('orig,new', RATIOS)
def test_pcm_input_equals_float_input(orig, new):
    """check 3: int16 PCM, scaled in the kernel, gives the bytes of the same samples passed as float32(x) / 32768 -- speech
    quantised to 16 bits and a ramp that reaches -32767 and 32767"""
    waves, refs, bounds = _case(orig, new)
    pcm = [np.rint(w * 32767.0).astype(np.int16) for w in waves[:-1]] + [_ramp(len(waves[-1]))]
    assert pcm[-1][0] == -32767 and pcm[-1][-1] == 32767
    a = audio.resample([torch.from_numpy(p) for p in pcm], orig, new)
    b = audio.resample([torch.from_numpy(p.astype(np.float32) / 32768.0) for p in pcm], orig, new)
    assert a.order.tolist() == b.order.tolist()
    for x, y in zip(_rows(a), _rows(b)):
        assert _same_bits(x, y)
    # the ramp is the last utterance of the shared case: the PCM path meets the oracle's bound too
    assert np.all(np.abs(_rows(a)[-1].astype(np.float64) - refs[-1]) <= bounds[-1])


@pytest.mark.parametrize('orig,new', [(48000, 22050), (1, 2), (48000, 8000)])
def test_guard_bands_stay_untouched(orig, new):
    """check 6: the packed output sits between two bands of NaNs; the kernel writes every sample of it and nothing else"""
    waves, refs, _ = _case(orig, new)
    o, n, _, first, _ = audio.resample_table(orig, new)
    _, _, _, first_d, table_d = audio.resample_table(orig, new, device=DEV)
    x = torch.cat([torch.from_numpy(w) for w in waves]).to(DEV)
    lens = np.array([len(w) for w in waves])
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total, G = sum(len(r) for r in refs), 4096
    buf = torch.full((total + 2 * G,), float('nan'), device=DEV)
    y, out_off, out_lens = ops.resample_batch(x, off, lens, o, n, first_d, table_d, int(first.min()), int(first.max()), out=buf[G:G + total])
    torch.cuda.synchronize()
    assert out_lens.tolist() == [len(r) for r in refs] and out_off.tolist() == np.concatenate([[0], np.cumsum(out_lens)[:-1]]).tolist()
    host = buf.cpu().numpy()
    assert np.isnan(host[:G]).all() and np.isnan(host[G + total:]).all()
    assert not np.isnan(host[G:G + total]).any()
    assert y.data_ptr() == buf[G:].data_ptr()


def test_more_utterances_than_one_call_takes():
    """FEATURES_MAX_BATCH + 1 very short utterances cross the chunking: every one against the oracle, in the caller's order"""
    orig, new = 48000, 22050
    B = ops.FEATURES_MAX_BATCH + 1
    rs = np.random.RandomState(3)
    waves = [rs.uniform(-1, 1, 1 + (7 * i) % 23).astype(np.float32) for i in range(B)]
    _, _, taps, first, table = audio.resample_table(orig, new)
    wb = audio.resample(waves, orig, new)
    rows = _rows(wb)
    assert len(rows) == B and wb.lens.tolist() == sorted((audio.resampled_len(len(w), orig, new) for w in waves), reverse=True)
    for w, got in zip(waves, rows):
        ref, s_abs = O.resample_compact(w, orig, new, table=table, first=first, want_abs=True)
        assert got.shape == ref.shape and np.all(np.abs(got - ref) <= (taps + 2) * 2.0 ** -24 * s_abs)
    assert _same_bits(rows[B - 1], _rows(audio.resample([waves[B - 1]], orig, new))[0])     # the utterance of the second call


def test_wavebatch_input_and_same_rate():
    waves = [_speech(L, L, 16000) for L in (300, 2000, 700)]
    wb_in = audio.WaveBatch([torch.from_numpy(w).to(DEV) for w in waves])
    out = audio.resample(wb_in, 16000, 22050)
    assert out.order.tolist() == [1, 2, 0]                                  # the caller's indices, longest first
    direct = _rows(audio.resample(waves, 16000, 22050))
    for a, b in zip(_rows(out), direct):
        assert _same_bits(a, b)
    assert audio.resample(wb_in, 22050, 22050) is wb_in
    with pytest.raises(ValueError, match='staged'):
        audio.resample(waves, 48000, 1000)


def test_features_of_resampled_waves():
    """check 7, first half: extract_batch(resample(48 kHz waves)) equals extract_batch of the oracle-resampled waves within the
    feature tests' tolerances (no noise, stretch 1)"""
    conv = audio.load_audio_transform(**AUDIO_CFG)
    waves = [_speech(L, 40 + i, 48000) for i, L in enumerate((30000, 9000, 17001))]
    _, _, _, first, table = audio.resample_table(48000, 22050)
    refs = [O.resample_compact(w, 48000, 22050, table=table, first=first).astype(np.float32) for w in waves]
    wb = audio.resample(waves, 48000, 22050)
    mel, _, lin = conv.extract_batch(wb, r=5, snr=SNR_OFF, stretch=1.0)
    mel_r, _, lin_r = conv.extract_batch([torch.from_numpy(r) for r in refs], r=5, snr=SNR_OFF, stretch=1.0)
    assert mel.shape == mel_r.shape and lin.shape == lin_r.shape and wb.order.tolist() == [0, 2, 1]
    e_mel, e_lin = float((mel - mel_r).abs().max()), float((lin - lin_r).abs().max())
    print('features of resampled waves: mel %.2e, linear %.2e' % (e_mel, e_lin))
    assert e_mel <= MEL_TOL and e_lin <= LIN_TOL


def _write_pcm(path, pcm, sr):
    """pcm (samples,) or (samples, channels) int16"""
    pcm = np.asarray(pcm, '<i2')
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def _header(path):
    with wave.open(str(path), 'rb') as w:
        return w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()


def _loud(L, seed, sr):
    """broadband and loud (white noise under a tone): every mel band stays far above the 16-bit rounding of a conversion"""
    rs = np.random.RandomState(seed)
    return np.clip(0.25 * rs.randn(L) + 0.2 * np.sin(2 * np.pi * 440 * np.arange(L) / sr), -0.99, 0.99)


def test_conversion_mode_and_the_resample_flag(tmp_path):
    """checks 7 (second half) and 8.  --resample-wav-dir writes 16-bit mono files of channel 0 at the asked rate with
    resampled_len samples, within one step of 16 bits of the oracle; --transcribe-wav-dir refuses the 48 kHz files without
    --resample and writes one .phn per file with it.

    What is compared between `--resample` on the 48 kHz files and the plain run on the converted files is the MEL, not the
    .phn lines: a .phn line holds a score printed to 1e-6 that went through the whole encoder, and the conversion's rounding
    to 16 bits (up to 0.5 / 32767 per sample) moves it.  The mel moves too, by a bounded amount: after pre-emphasis a sample is
    off by at most 1.97 * 0.5 / 32767, a frame's spectrum by at most that times sum(window) = 551, a mel amplitude a by at most
    d = that times the largest sum of a band's weights (area-normalised bands: about 1 / (bin width 10.77 Hz) = 0.093), about 1.5e-3, and the normalised mel
    20 log10(a) / 100 by at most -0.2 log10(1 - d / a) -- checked element by element with a from the unrounded side, wherever
    d / a <= 0.5 (nearly everywhere for the loud broadband test signal), on top of the feature kernel's own MEL_TOL on each side."""
    import yaml
    import main as entry
    cfg_path = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')
    config = yaml.load(open(cfg_path), Loader=yaml.FullLoader)
    assert config['data']['audio']['sample_rate'] == 22050
    src, dst = tmp_path / 'wav48', tmp_path / 'wav22'
    src.mkdir()
    pcm = {'a.wav': (np.rint(_loud(14000, 1, 48000) * 32767).astype(np.int16), 48000),
           'b.wav': (np.stack([np.rint(_loud(9000, 2, 48000) * 32767), np.full(9000, 1234)], 1).astype(np.int16), 48000),
           'c.wav': (np.rint(_loud(21000, 3, 48000) * 32767).astype(np.int16), 48000)}
    for name, (p, sr) in pcm.items():
        _write_pcm(src / name, p, sr)
    entry.main(['--resample-wav-dir', str(src), '--resample-out', str(dst), '--resample-rate', '22050', '--batch-size', '2', '--no-msg'])
    assert sorted(os.listdir(str(dst))) == sorted(pcm)
    _, _, _, first, table = audio.resample_table(48000, 22050)
    for name, (p, sr) in pcm.items():
        ch0 = p if p.ndim == 1 else p[:, 0]
        assert _header(dst / name) == (22050, 1, 2, audio.resampled_len(len(ch0), sr, 22050))
        ref = O.resample_compact(ch0 / 32768.0, sr, 22050, table=table, first=first)
        got = audio.read_wav(str(dst / name))[0][0].numpy().astype(np.float64) * 32768.0
        assert np.abs(got - np.clip(ref, -1, 1) * 32767.0).max() <= 0.5 + 32767 * 1e-5, name          # rint of a value the kernel has to 1e-5
    # another rate, and a directory of mixed rates with a file already at the target
    mixed, out16 = tmp_path / 'mixed', tmp_path / 'wav16'
    mixed.mkdir()
    _write_pcm(mixed / 'x.wav', pcm['a.wav'][0][:5000], 48000)
    _write_pcm(mixed / 'y.wav', pcm['c.wav'][0][:3000], 16000)
    _write_pcm(mixed / 'z.wav', pcm['c.wav'][0][:4000], 22050)
    entry.main(['--config', cfg_path, '--resample-wav-dir', str(mixed), '--resample-out', str(out16), '--resample-rate', '16000', '--no-msg'])
    assert [_header(out16 / f) for f in ('x.wav', 'y.wav', 'z.wav')] == [
        (16000, 1, 2, audio.resampled_len(5000, 48000, 16000)), (16000, 1, 2, 3000), (16000, 1, 2, audio.resampled_len(4000, 22050, 16000))]
    with pytest.raises(ValueError, match='is the directory'):
        from semi_tts_amd.solver import Resampler
        paras = entry.parse_args(['--resample-wav-dir', str(src), '--resample-out', str(dst), '--resample-rate', '8000'])
        paras.resample_out = str(src)
        Resampler(None, paras, 'test').load_data()

    # the mel of the two routes to 22050 Hz
    conv = audio.load_audio_transform(**config['data']['audio'])
    names = sorted(pcm)
    with pytest.raises(ValueError, match='Sample rate mismatch. Expected 22050 but get 48000'):
        conv.load_batch([str(src / f) for f in names])
    wb_a = conv.load_batch([str(src / f) for f in names], resample=True)
    wb_b = conv.load_batch([str(dst / f) for f in names])
    assert wb_a.order.tolist() == wb_b.order.tolist() and wb_a.lens.tolist() == wb_b.lens.tolist()
    mel_a, _, _ = conv.extract_batch(wb_a, snr=SNR_OFF, stretch=1.0)
    mel_b, _, _ = conv.extract_batch(wb_b, snr=SNR_OFF, stretch=1.0)
    ma, mb = mel_a.double().cpu().numpy(), mel_b.double().cpu().numpy()
    amp = 10.0 ** ((ma * 100.0 - 80.0) / 20.0)
    fb_sum = float(audio.mel_filterbank(22050, conv.n_fft, conv.n_mels).astype(np.float64).sum(1).max())
    assert conv.win_length == 1102 and 0.09 < fb_sum < 0.12
    d = 1.97 * 0.5 / 32767 * 551.0 * fb_sum
    live = np.zeros_like(ma, bool)
    for row, L in enumerate(wb_a.lens):
        live[row, :1 + L // conv.hop_length] = True
    ok = live & (ma > 0) & (d / amp <= 0.5)
    tol = -0.2 * np.log10(1.0 - np.minimum(d / amp, 0.5)) + 2 * MEL_TOL + 3e-6      # (3e-6: the gain 32767 / 32768 of a written file)
    print('mel, --resample against converted files: max %.2e, %.1f %% of the frames x bands compared, largest tolerance %.2e'
          % (np.abs(ma - mb)[ok].max(), 100.0 * ok.sum() / live.sum(), tol[ok].max()))
    assert ok.sum() >= 0.9 * live.sum()
    assert np.all(np.abs(ma - mb)[ok] <= tol[ok])

    # the flag itself: one Transcriber, refused without --resample, one .phn per file with it
    from semi_tts_amd.solver import Transcriber
    argv = ['--config', cfg_path, '--transcribe-wav-dir', str(src), '--beam-width', '4', '--logdir', str(tmp_path / 'log'), '--name', 'tr',
            '--batch-size', '2', '--no-msg', '--resample']
    paras = entry.parse_args(argv)
    tr = Transcriber(config, paras, 'test')
    tr.load_data()
    tr.set_model()
    paras.resample = False
    with pytest.raises(ValueError, match='Sample rate mismatch. Expected 22050 but get 48000'):
        tr.exec()
    paras.resample = True
    assert tr.exec() == 3
    out = tmp_path / 'log' / 'tr'
    assert sorted(os.listdir(str(out))) == ['a.phn', 'b.phn', 'c.phn']
    for f in os.listdir(str(out)):
        lines = open(str(out / f)).read().splitlines()
        assert len(lines) == 1 and len(lines[0].split('\t')) == 2 and np.isfinite(float(lines[0].split('\t')[0]))
