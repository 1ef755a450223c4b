"""CPU side of mel vocoding and ragged batches (semi_tts_amd.audio mel_basis / mel_to_wave / vocode_batch, main.py --vocode-dir):
the pseudo-inverse basis against the reference's torch.pinverse, the rank check, refusals that fire before any device is touched,
the order of the phase draws, and the listing / naming / stop-before-writing behaviour of --vocode-dir."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel_oracle as MO   # noqa: E402

AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=22050,
                 use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])
SR = 22050
# every combination of the supported n_fft with these mel counts at 22050 Hz; (512, 80) is the one rank-deficient bank
FULL_RANK = [(n_fft, n_mels) for n_fft in (512, 1024, 2048, 4096) for n_mels in (8, 20, 40, 80) if (n_fft, n_mels) != (512, 80)]


@pytest.mark.parametrize('n_fft,n_mels', FULL_RANK)
def test_mel_basis_matches_the_reference_pinverse(n_fft, n_mels):
    """src/audio.py:202: torch.pinverse(fb).transpose(0, 1) on the float32 bank.  Bound: 1e-4 of the largest entry (a transposed or
    mis-scaled basis is off by O(1); the float32 pseudo-inverse itself is good to a few 1e-6 on these full-rank banks)."""
    from semi_tts_amd.audio import mel_basis, mel_filterbank
    got = mel_basis(SR, n_fft, n_mels)
    assert got.dtype == np.float32 and got.shape == (n_mels, n_fft // 2 + 1) and got.flags['C_CONTIGUOUS']
    ref = torch.pinverse(torch.from_numpy(mel_filterbank(SR, n_fft, n_mels))).transpose(0, 1).numpy()
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print('mel_basis n_fft %d, %d mels: max-abs %.2e of %.3g' % (n_fft, n_mels, err, scale))
    assert err <= 1e-4 * scale
    # and it is a right inverse of the bank: fb @ pinv(fb) = I for a full-rank bank with fewer mels than bins
    eye = mel_filterbank(SR, n_fft, n_mels).astype(np.float64) @ got.astype(np.float64).T
    assert np.abs(eye - np.eye(n_mels)).max() < 1e-4


def test_rank_deficient_bank_is_refused():
    from semi_tts_amd import audio
    with pytest.raises(ValueError, match='rank deficient'):
        audio.mel_basis(SR, 512, 80)
    sv = np.linalg.svd(audio.mel_filterbank(SR, 512, 80).astype(np.float64), compute_uv=False)
    assert sv[-1] / sv[0] < 1e-12                                   # orders of magnitude below the 1e-6 threshold ...
    for n_fft, n_mels in FULL_RANK:                                  # ... and every full-rank bank orders of magnitude above it
        sv = np.linalg.svd(audio.mel_filterbank(SR, n_fft, n_mels).astype(np.float64), compute_uv=False)
        assert sv[-1] / sv[0] > 0.1


def test_converter_caches_its_basis():
    from semi_tts_amd import audio
    conv = audio.load_audio_transform(**AUDIO_CFG)
    a = conv.mel_basis()
    assert a is conv.mel_basis() and np.array_equal(a, audio.mel_basis(SR, 2048, 80))


def test_oracle_is_the_reference_expression():
    """mel_oracle against the reference's own lines in float64 torch: pinverse(fb).T @ db_to_amp(denormalize(mel) + 20)"""
    rs = np.random.RandomState(0)
    mel = rs.uniform(-0.2, 1.2, (2, 7, 8)).astype(np.float32)
    basis = rs.randn(8, 33).astype(np.float32)
    m = torch.from_numpy(mel).double().transpose(1, 2)                                  # (B, n_mels, T) as the reference holds it
    amp = 10 ** (0.05 * ((-100 + torch.clamp(m, min=0, max=1) * 100) + 20))
    ref = torch.matmul(torch.from_numpy(basis).double().t(), amp).transpose(1, 2).numpy()
    got, mag = MO.mel_to_linear(mel, basis)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    assert np.all(mag >= np.abs(got) * (1 - 1e-12))


def _no_device(monkeypatch):
    from semi_tts_amd import audio, ops

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    for name in ('griffin_lim', 'griffin_lim_batch', 'mel_to_linear'):
        monkeypatch.setattr(audio.toolops, name, no_device)
    monkeypatch.setattr(audio, '_device', no_device)
    return audio


def test_refusals_fire_before_the_device(monkeypatch):
    audio = _no_device(monkeypatch)
    conv = audio.load_audio_transform(**AUDIO_CFG)
    # wrong bin count
    with pytest.raises(ValueError, match='mel bins'):
        conv.mel_to_wave(torch.rand(2, 50, 81))
    with pytest.raises(ValueError, match='mel bins'):
        conv.mel_to_wave(torch.rand(50, 1025))
    with pytest.raises(ValueError, match='mel bins'):
        conv.melspecgram_to_specgram(torch.rand(2, 1025, 50))
    with pytest.raises(ValueError, match='mel bins'):
        conv.gen_wav_device(torch.rand(2, 50, 1025), mel=True)
    with pytest.raises(NotImplementedError, match='linear'):                 # the refusal without the new argument stays
        conv.gen_wav_device(torch.rand(2, 50, 80))
    with pytest.raises(ValueError, match='expected'):
        conv.vocode_batch([np.zeros((50, 80), np.float32)], 'spec')
    with pytest.raises(ValueError, match='expected'):
        conv.vocode_batch([np.zeros((50, 80), np.float32), np.zeros((40, 1025), np.float32)], 'mel')
    with pytest.raises(ValueError, match='kind'):
        conv.vocode_batch([np.zeros((50, 80), np.float32)], 'linear')
    with pytest.raises(ValueError, match='empty'):
        conv.vocode_batch([], 'mel')
    # too few frames, for the batch and per utterance (5 is the minimum at 2048 / 275)
    with pytest.raises(ValueError, match='too few'):
        conv.mel_to_wave(torch.rand(4, 80))
    with pytest.raises(ValueError, match='utterance 1.*too few'):
        conv.vocode_batch([np.zeros((9, 80), np.float32), np.zeros((4, 80), np.float32)], 'mel')
    with pytest.raises(ValueError, match='utterance 0.*too few'):
        conv.vocode_batch([np.zeros((4, 1025), np.float32), np.zeros((9, 1025), np.float32)], 'spec')
    # frames: B integers in [5, T]
    mel, lin = torch.rand(3, 20, 80), torch.rand(3, 20, 1025)
    for feat, kw in ((mel, dict(mel=True)), (lin, {})):
        with pytest.raises(ValueError, match='too few'):
            conv.gen_wav_device(feat, frames=[20, 4, 20], **kw)
        with pytest.raises(ValueError, match='the batch holds'):
            conv.gen_wav_device(feat, frames=[20, 21, 20], **kw)
        with pytest.raises(ValueError, match='integers'):
            conv.gen_wav_device(feat, frames=[20, 20], **kw)
        with pytest.raises(ValueError, match='integers'):
            conv.gen_wav_device(feat, frames=[20, 10.5, 20], **kw)
        with pytest.raises(ValueError, match='integers'):
            conv.gen_wav_device(feat, frames=np.full((3, 1), 20), **kw)
    with pytest.raises(ValueError, match='too few'):
        conv.mel_to_wave(mel, frames=torch.tensor([20, 20, 0]))
    with pytest.raises(ValueError, match='phases'):
        conv.mel_to_wave(mel, phases=np.zeros((3, 1025, 19), np.float32))
    # power != 1 with mel
    with pytest.raises(ValueError, match='power'):
        audio._run(mel, None, 2048, 275, 1102, 1, normalized=True, power=1.5, post=0, basis=conv.mel_basis)
    # a rank-deficient bank
    bad = audio.load_audio_transform(**dict(AUDIO_CFG, num_freq=257))
    with pytest.raises(ValueError, match='rank deficient'):
        bad.mel_to_wave(torch.rand(2, 50, 80))
    with pytest.raises(ValueError, match='rank deficient'):
        bad.vocode_batch([np.zeros((50, 80), np.float32)], 'mel')
    with pytest.raises(ValueError, match='rank deficient'):
        bad.melspecgram_to_specgram(torch.rand(80, 50))
    # legal input does get as far as the device
    for call in (lambda: conv.mel_to_wave(mel, frames=[20, 5, 19]), lambda: conv.melspecgram_to_specgram(torch.rand(80, 1)),
                 lambda: conv.vocode_batch([np.zeros((5, 80), np.float32), np.zeros((9, 80), np.float32)], 'mel')):
        with pytest.raises(AssertionError, match='reached the device'):
            call()


def test_feat_to_wave_still_refuses_mel(monkeypatch):
    audio = _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match='mel'):
        audio.load_audio_transform(**AUDIO_CFG).feat_to_wave(torch.rand(2, 50, 80))


@pytest.mark.parametrize('kind,D', [('spec', 1025), ('mel', 80)])
def test_vocode_batch_draws_phases_as_the_file_loop(monkeypatch, kind, D):
    """the reference script vocodes file after file, each drawing np.random.rand(F, T_i): one batch consumes the generator alike"""
    from semi_tts_amd import audio, ops
    lens = [9, 23, 5, 14]
    seen = {}

    def fake(feat, phases, n_fft, hop, win, **kw):
        seen.update(phases=phases.clone(), frames=kw['frames'].clone(), feat=feat.clone(), kw=kw)
        return torch.zeros(feat.shape[0], hop * (feat.shape[1] - 1))
    monkeypatch.setattr(audio.toolops, 'griffin_lim_batch', fake)
    monkeypatch.setattr(audio, '_device', lambda: torch.device('cpu'))
    conv = audio.load_audio_transform(**AUDIO_CFG)
    monkeypatch.setattr(conv, 'mel_basis', lambda device=None: torch.zeros(80, 1025))
    rs = np.random.RandomState(3)
    feats = [rs.rand(n, D).astype(np.float32) for n in lens]
    np.random.seed(11)
    wavs = conv.vocode_batch(feats, kind)
    after = np.random.rand()
    np.random.seed(11)
    loop = [audio.draw_phases((1025, n)) for n in lens]
    assert after == np.random.rand()                                 # the generator stands where the file loop leaves it
    assert [len(w) for w in wavs] == [275 * (n - 1) for n in lens] and all(w.dtype == np.float64 for w in wavs)
    assert seen['frames'].tolist() == lens and seen['frames'].dtype == torch.int32
    assert tuple(seen['phases'].shape) == (4, 1025, 23) and tuple(seen['feat'].shape) == (4, 23, D)
    for b, n in enumerate(lens):
        assert np.array_equal(seen['phases'][b, :, :n].numpy(), loop[b])
        assert np.array_equal(seen['feat'][b, :n].numpy(), feats[b])
    assert (seen['kw']['basis'] is not None) == (kind == 'mel') and seen['kw']['normalized'] and seen['kw']['power'] == 1.0
    assert seen['kw']['post'] == ops.GL_CLIP | ops.GL_INV_PREEMPHASIS and seen['kw']['n_iter'] == audio.GFL_ITER


# ---------------------------------------------------------------------------------------------- main.py --vocode-dir
def _paras(tmp_path, feat_dir, kind):
    return types.SimpleNamespace(vocode_dir=str(feat_dir), vocode_feat=kind, batch_size=2, logdir=str(tmp_path / 'log'), name='voc',
                                 verbose=False)


def _config():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return yaml.safe_load(open(os.path.join(root, 'config', 'supervised.yaml')))


def _write(feat_dir, names, shapes):
    os.makedirs(feat_dir, exist_ok=True)
    for n, sh in zip(names, shapes):
        np.save(os.path.join(feat_dir, n), np.zeros(sh, np.float32))


def test_vocode_dir_lists_sorts_and_names(tmp_path):
    from semi_tts_amd.solver import Vocoder
    d = tmp_path / 'feats'
    _write(d, ['b-spec.npy', 'a-spec.npy', 'LJ001-0002-spec.npy', 'a-mel.npy', 'c-mel.npy', 'a-align.npy', 'x-spec.npy.bak'],
           [(9, 1025), (5, 1025), (12, 1025), (5, 80), (7, 80), (3, 3), (9, 1025)])
    s = Vocoder(_config(), _paras(tmp_path, d, 'spec'), 'test').load_data()
    assert s.files == [('LJ001-0002-spec.npy', 'LJ001-0002'), ('a-spec.npy', 'a'), ('b-spec.npy', 'b')]
    s = Vocoder(_config(), _paras(tmp_path, d, 'mel'), 'test').load_data()
    assert s.files == [('a-mel.npy', 'a'), ('c-mel.npy', 'c')]
    assert s.logdir == os.path.join(str(tmp_path / 'log'), 'voc')


def test_vocode_dir_writes_stems_in_batches(tmp_path, monkeypatch):
    """exec without a device: vocode_batch replaced; <logdir>/<stem>.wav for every file, batches of --batch-size in sorted order"""
    import wave
    from semi_tts_amd.solver import Vocoder
    d = tmp_path / 'feats'
    _write(d, ['u2-mel.npy', 'u1-mel.npy', 'u3-mel.npy'], [(9, 80), (5, 80), (7, 80)])
    s = Vocoder(_config(), _paras(tmp_path, d, 'mel'), 'test').load_data().set_model()
    calls = []

    def fake(feats, kind):
        calls.append(([f.shape[0] for f in feats], kind))
        return [np.zeros(275 * (f.shape[0] - 1)) for f in feats]
    monkeypatch.setattr(s.audio_converter, 'vocode_batch', fake)
    assert s.exec() == 3
    assert calls == [([5, 9], 'mel'), ([7], 'mel')]
    assert sorted(os.listdir(s.logdir)) == ['u1.wav', 'u2.wav', 'u3.wav']
    with wave.open(os.path.join(s.logdir, 'u2.wav'), 'rb') as w:
        assert (w.getframerate(), w.getnframes()) == (22050, 275 * 8)


@pytest.mark.parametrize('kind,bad,shape,msg', [
    ('spec', 'm-spec.npy', (9, 80), 'm-spec.npy has shape'),            # mel-sized file among the linear ones
    ('spec', 'm-spec.npy', (4, 1025), 'm-spec.npy has 4 frames'),       # too few frames
    ('spec', 'm-spec.npy', (1025,), 'm-spec.npy has shape'),
    ('mel', 'm-mel.npy', (9, 1025), 'm-mel.npy has shape'),
    ('mel', 'm-mel.npy', (2, 80), 'm-mel.npy has 2 frames'),
])
def test_vocode_dir_stops_before_writing_on_a_bad_file(tmp_path, kind, bad, shape, msg):
    from semi_tts_amd.solver import Vocoder
    d = tmp_path / 'feats'
    good = (9, 1025) if kind == 'spec' else (9, 80)
    _write(d, ['a-%s.npy' % kind, bad, 'z-%s.npy' % kind], [good, shape, good])
    s = Vocoder(_config(), _paras(tmp_path, d, kind), 'test')
    with pytest.raises(ValueError, match=msg):
        s.load_data()
    assert not os.path.exists(s.logdir)                              # nothing written, not even the directory


def test_vocode_dir_without_files(tmp_path):
    from semi_tts_amd.solver import Vocoder
    d = tmp_path / 'feats'
    _write(d, ['a-mel.npy'], [(9, 80)])
    with pytest.raises(ValueError, match='no \\*-spec.npy'):
        Vocoder(_config(), _paras(tmp_path, d, 'spec'), 'test').load_data()


def test_vocode_flags(capsys):
    import main
    p = main.parse_args(['--config', 'config/supervised.yaml', '--vocode-dir', 'x'])
    assert (p.vocode_dir, p.vocode_feat, p.gen_wav_feat) == ('x', 'spec', 'linear')
    assert main.parse_args(['--config', 'c', '--vocode-dir', 'x', '--vocode-feat', 'mel']).vocode_feat == 'mel'
    p = main.parse_args(['--config', 'c', '--gen-specgram', '--gen-wav', '--gen-wav-feat', 'mel'])
    assert p.gen_wav and p.gen_wav_feat == 'mel'
    assert main.parse_args(['--config', 'c', '--gen-specgram', '--gen-wav']).gen_wav_feat == 'linear'
    for argv in (['--vocode-feat', 'mel'], ['--vocode-dir', 'x', '--gen-specgram'], ['--vocode-dir', 'x', '--tts-only'],
                 ['--gen-wav-feat', 'mel'], ['--gen-specgram', '--gen-wav-feat', 'mel'], ['--vocode-dir', 'x', '--vocode-feat', 'linear']):
        with pytest.raises(SystemExit):
            main.parse_args(['--config', 'c'] + argv)
    capsys.readouterr()


def test_vocoder_entry_refuses_what_it_cannot_vocode():
    """st_griffin_lim_batch, the one vocoder entry, refuses a bad job before anything is launched (host arithmetic on the job and
    framing structs: it returns here, without a device; the device pointers are host memory nobody reads)"""
    import ctypes as C
    from semi_tts_amd import _lib
    lib = _lib.load()
    raw = C.create_string_buffer(1 << 12)
    p = (C.addressof(raw) + 255) & ~255          # 256-byte aligned, like a device allocation
    fr = _lib.StFraming(n_fft=1024, win=1024, hop=256)

    def refused(why, **kw):
        job = _lib.StGlJob(**dict(dict(feat=p, sb=12 * 513, st=513, sf=1, n_in=513, normalized=1, power=1.0, phases=p, wav=p, B=3, T=12,
                                       n_iter=2, post=3), **kw))
        rc = lib.st_griffin_lim_batch(C.byref(job), C.byref(fr), p, None)
        msg = lib.st_last_error().decode()
        assert rc != 0 and msg.startswith('st_griffin_lim_batch: ') and why in msg, (rc, msg)

    refused('power must be 1', basis=p, n_in=80, sb=12 * 80, st=80, power=1.5)
    refused('bins, expected', n_in=512)
    refused('bad n_iter', post=4)
    refused('bad batch', T=1)
    assert lib.st_griffin_lim_batch(None, C.byref(fr), p, None) != 0 and 'null' in lib.st_last_error().decode()
    assert lib.st_griffin_lim_batch(C.byref(_lib.StGlJob()), None, p, None) != 0 and 'null' in lib.st_last_error().decode()
