"""CPU side of feature extraction (semi_tts_amd.audio, st_audio_features): the mel filterbank against the reference's, the fp64
oracle (tests/feat_oracle.py) against the reference's own outputs (tests/golden/audio_features.npz, tools/gen_golden_features.py),
the .wav reader, the batch packing and the argument checks that fire before any device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_oracle as O   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'audio_features.npz')
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN))


def test_mel_filterbank_matches_the_reference_within_one_ulp(gold):
    from semi_tts_amd.audio import mel_filterbank
    fb = mel_filterbank(22050, 2048, 80)
    ref = gold['fb']
    assert fb.shape == ref.shape == (80, 1025) and fb.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(fb), np.abs(ref)).astype(np.float32))
    assert np.all(np.abs(fb.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    assert np.array_equal(fb != 0, ref != 0)


def test_filterbank_bands():
    from semi_tts_amd.audio import band_pack, mel_filterbank
    fb = mel_filterbank(22050, 2048, 80)
    start, cnt, off, w = band_pack(fb)
    assert int((fb != 0).sum()) == 2001 == w.size == int(cnt.sum())
    assert cnt.min() == 7 and cnt.max() == 83
    dense = np.zeros_like(fb)
    for m in range(80):
        dense[m, start[m]:start[m] + cnt[m]] = w[off[m]:off[m] + cnt[m]]
    assert np.array_equal(dense, fb)


@pytest.mark.parametrize('u', [0, 1])
def test_oracle_reproduces_the_reference(gold, u):
    x, fb = gold['wav%d' % u], gold['fb']
    lin, mel = O.features(x, fb)
    assert float((lin - torch.from_numpy(gold['spec%d' % u]).double()).abs().max()) <= 1e-4
    assert float((mel - torch.from_numpy(gold['mel%d' % u]).double()).abs().max()) <= 1e-4
    win, hop = O.stretch_dims(float(gold['stretch%d' % u]))
    _, aug = O.features(x, fb, win=win, hop=hop, noise=gold['noise%d' % u], snr=float(gold['snr%d' % u]))
    assert aug.T.shape == gold['aug%d' % u].shape
    assert float((aug.T - torch.from_numpy(gold['aug%d' % u]).double()).abs().max()) <= 1e-4
    win, hop = O.stretch_dims(float(gold['stretch_clean%d' % u]))
    _, aug = O.features(x, fb, win=win, hop=hop)
    assert float((aug.T - torch.from_numpy(gold['aug_clean%d' % u]).double()).abs().max()) <= 1e-4


def test_wav_round_trip(tmp_path):
    from semi_tts_amd.audio import load_wav, write_wav
    x = np.random.RandomState(0).uniform(-0.9, 0.9, 5000)
    write_wav(tmp_path / 'a.wav', x, 22050)
    y = load_wav(tmp_path / 'a.wav', 22050)
    assert y.shape == (1, 5000) and y.dtype == torch.float32
    np.testing.assert_allclose(y[0].numpy(), np.rint(x * 32767) / 32768, rtol=0, atol=1e-7)
    with pytest.raises(ValueError, match='Sample rate mismatch'):
        load_wav(tmp_path / 'a.wav', 16000)


def test_wave_batch_sorts_longest_first_and_packs():
    from semi_tts_amd.audio import WaveBatch
    wavs = [torch.full((n,), float(i)) for i, n in enumerate([3000, 5000, 3000, 7000])]
    wb = WaveBatch(wavs)
    assert list(wb.order) == [3, 1, 0, 2] and list(wb.lens) == [7000, 5000, 3000, 3000]
    assert list(wb.offsets) == [0, 7000, 12000, 15000]
    x = wb.packed('cpu')
    assert x.shape == (18000,) and float(x[7000]) == 1.0 and float(x[15000]) == 2.0


def test_stretch_dims_follow_the_reference():
    from semi_tts_amd.audio import load_audio_transform
    conv = load_audio_transform(**AUDIO_CFG)
    for rate in (0.9, 0.95, 1.0, 1.07, 1.1):
        assert conv.stretch_dims(rate) == O.stretch_dims(rate)
    assert conv.stretch_dims(1.0) == (1102, 275) and conv.stretch_dims(0.9) == (992, 248)


def test_feature_argument_checks_fire_before_the_device(monkeypatch, tmp_path):
    from semi_tts_amd import audio, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(audio.toolops, 'audio_features', no_device)
    monkeypatch.setattr(audio, '_device', no_device)
    conv = audio.load_audio_transform(**AUDIO_CFG)
    x = torch.rand(30000) - 0.5
    with pytest.raises(ValueError, match='n_fft'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=1000)).extract_batch([x])
    with pytest.raises(ValueError, match='n_fft'):
        audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=1000)).extract_feature_from_waveform(x[None])
    with pytest.raises(ValueError, match='too short'):
        conv.extract_batch([x, torch.rand(1024)])                     # L = n_fft // 2
    with pytest.raises(ValueError, match='too short'):
        conv.extract_feature_from_waveform(torch.rand(1, 900))
    long_win = audio.load_audio_transform(**dict(AUDIO_CFG, frame_length_ms=90))      # win 1984 at rate 1, 2182 at 1.1
    with pytest.raises(ValueError, match='augmented'):
        long_win.extract_batch([x], stretch=1.1)
    with pytest.raises(ValueError, match='clean'):
        audio.load_audio_transform(**dict(AUDIO_CFG, frame_shift_ms=30)).extract_batch([x])    # 2 hop > win
    with pytest.raises(ValueError, match='SNRs'):
        conv.extract_batch([x, x], snr=[10.0], stretch=1.0)
    audio.write_wav(tmp_path / 'b.wav', np.zeros(4000), 16000)
    with pytest.raises(ValueError, match='Sample rate mismatch'):
        conv.wave_to_feat(tmp_path / 'b.wav')


def test_extractor_entries_refuse_what_they_cannot_frame():
    """st_audio_features and st_audio_mfcc refuse a bad batch, framing or filterbank with the entry's own name in the message, before
    anything is launched (the checks are host arithmetic on the operand structs: they return here, without a device; the device
    pointers are host memory nobody reads)"""
    import ctypes as C
    from semi_tts_amd import _lib
    lib = _lib.load()
    raw = C.create_string_buffer(1 << 12)
    p = (C.addressof(raw) + 255) & ~255          # 256-byte aligned, like a device allocation

    def call(entry, lens=(4000,), off=None, n_samples=1 << 20, fr=(1024, 1024, 256), T_pad=None, n_mels=40, n_mfcc=13, aug=None, x=p,
             batch=True):
        lens = np.asarray(lens, dtype=np.int32)
        off = np.asarray(np.arange(len(lens)) * 8000 if off is None else off, dtype=np.int64)
        w = _lib.StWaveBatch(x=x, n_samples=n_samples, off=off.ctypes.data, len=lens.ctypes.data, B=len(lens))
        bank = _lib.StMelBank(start=p, cnt=p, off=p, w=p, n_mels=n_mels)
        T_pad = 1 + int(lens.max()) // max(fr[2], 1) if T_pad is None else T_pad
        wp, frp = C.byref(w) if batch else None, C.byref(_lib.StFraming(*fr))
        if entry == 'st_audio_features':
            rc = lib.st_audio_features(wp, frp, 0.97, C.byref(bank), None if aug is None else C.byref(aug), p, p, T_pad, p, None)
        else:
            rc = lib.st_audio_mfcc(wp, frp, 0.97, C.byref(bank), p, n_mfcc, p, None, T_pad, None)
        return rc, lib.st_last_error().decode()

    def refused(entry, why, **kw):
        rc, msg = call(entry, **kw)
        assert rc != 0 and msg.startswith(entry + ': ') and why in msg, (rc, msg)

    for entry in ('st_audio_features', 'st_audio_mfcc'):
        refused(entry, 'not supported', fr=(1536, 1024, 256))
        refused(entry, 'need 0 < 2 * hop <= win <= n_fft', fr=(2048, 1102, 600))
        refused(entry, 'reflect padding', lens=(4000, 512))                       # n_fft / 2 samples
        refused(entry, 'outside the', lens=(4000, 4000), off=(0, 4001), n_samples=8000)
        refused(entry, 'outside [1, 64]', lens=(4000,) * 65)
        refused(entry, 'T_pad', lens=(4000, 4096), T_pad=16)                      # the longest utterance has 17 frames
        refused(entry, 'null pointer', batch=False)
        refused(entry, 'null pointer', x=None)
    aug_win, aug_hop = np.asarray([1102, 1102], dtype=np.int32), np.asarray([275, 600], dtype=np.int32)
    refused('st_audio_features', 'augmented framing needs', aug=_lib.StFeatAug(out=p, Ta_pad=64))
    refused('st_audio_features', 'augmented framing needs 0 <', fr=(2048, 1024, 256), lens=(4000, 4000),
            aug=_lib.StFeatAug(win=aug_win.ctypes.data, hop=aug_hop.ctypes.data, out=p, Ta_pad=64))
    refused('st_audio_features', 'first utterance index', aug=_lib.StFeatAug(utt0=-1))
    refused('st_audio_mfcc', 'derivatives need at least 9', fr=(512, 512, 128), lens=(4000, 8 * 128 - 1))
    refused('st_audio_mfcc', 'n_mfcc', n_mels=12)
