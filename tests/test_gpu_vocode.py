"""Mel vocoding and ragged batches on the MI355X (audio.hip: st_mel_to_linear, st_griffin_lim_batch): the mel -> linear product
against the float64 oracle (tests/mel_oracle.py) under the derived dot-product bounds, Griffin-Lim from mel against the linear
path and the float64 Griffin-Lim oracle, ragged batches bitwise against each utterance vocoded alone, and main.py --vocode-dir."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_oracle as O    # noqa: E402
import mel_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 22050
DIMS = (2048, 275, 1102)
AUDIO_CFG = dict(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97, sample_rate=SR,
                 use_linear=True)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd import audio
    return audio.load_audio_transform(**AUDIO_CFG)


_BASIS = {}


def _basis(n_fft, n_mels):
    from semi_tts_amd.audio import mel_basis
    if (n_fft, n_mels) not in _BASIS:
        _BASIS[(n_fft, n_mels)] = mel_basis(SR, n_fft, n_mels)
    return _BASIS[(n_fft, n_mels)]


def _mel(B, T, n_mels, seed):
    """normalised-mel-like values that include exactly 0, exactly 1, values below 0 and above 1"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-0.15, 1.15, (B, T, n_mels)).astype(np.float32)
    flat = x.reshape(-1)
    flat[0::7], flat[3::11] = 0.0, 1.0
    if flat.size > 2:
        flat[1], flat[2] = -0.25, 1.5
    return x


def _phases(shape, seed):
    from semi_tts_amd.audio import draw_phases
    np.random.seed(seed)
    return draw_phases(shape)


# ---------------------------------------------------------------------------------------------- the product
def _tile_frames():
    from semi_tts_amd import ops
    t = ops.MEL_TO_LINEAR_TILE
    return sorted({1, 5, 9, 33, t - 1, t, t + 1})


@pytest.mark.parametrize('layout', ['contiguous', 'transposed'])
@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n_fft,n_mels', [(512, 40), (2048, 80), (2048, 1)])
def test_mel_to_linear_matches_the_oracle(dev, n_fft, n_mels, B, normalized, layout):
    """|got - ref| <= (n_mels + 2) u sum_m |basis| |a| for normalized=0 (the dot-product bound), (n_mels + 128) u sum_m |basis| a_ref
    for normalized=1 (mel_oracle.bound), per element, for every T around and across the frame tile."""
    from semi_tts_amd import ops
    basis = _basis(n_fft, n_mels)
    bd = torch.from_numpy(basis).to(dev)
    for T in _tile_frames():
        mel = _mel(B, T, n_mels, seed=n_fft + 100 * T + B)
        md = torch.from_numpy(mel).to(dev)
        if layout == 'transposed':                                   # a (B, n_mels, T) tensor read as its (B, T, n_mels) view
            md = md.transpose(1, 2).contiguous().transpose(1, 2)
            assert not md.is_contiguous() or T == 1 or n_mels == 1
        ref, mag = MO.mel_to_linear(mel, basis, normalized)
        got = ops.mel_to_linear(md, bd, normalized=normalized, take_abs=False)
        assert got.shape == (B, T, n_fft // 2 + 1)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = MO.bound(mag, n_mels, normalized)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print('mel_to_linear n_fft %d mels %d B %d T %d norm %d %s: worst err / bound %.3f' % (n_fft, n_mels, B, T, normalized, layout, worst))
        assert np.all(err <= bound), (T, worst)
        mag_got = ops.mel_to_linear(md, bd, normalized=normalized, take_abs=True)
        assert torch.equal(mag_got, got.abs())


def test_mel_to_linear_rows_do_not_depend_on_batch_or_tile(dev):
    """each output is one fmaf chain over ascending m: a row alone, in a batch, at any position of a tile, is bitwise the same"""
    from semi_tts_amd import ops
    basis = torch.from_numpy(_basis(2048, 80)).to(dev)
    mel = torch.from_numpy(_mel(3, 37, 80, seed=5)).to(dev)
    full = ops.mel_to_linear(mel, basis)
    for b, t in ((0, 0), (1, 15), (1, 16), (2, 36)):
        assert torch.equal(ops.mel_to_linear(mel[b:b + 1, t:t + 1], basis)[0, 0], full[b, t])
    assert torch.equal(ops.mel_to_linear(mel[:, 3:30], basis), full[:, 3:30])


def test_mel_to_linear_refusals(dev):
    from semi_tts_amd import ops
    with pytest.raises(RuntimeError, match='mels'):
        ops.mel_to_linear(torch.zeros(1, 2, 257, device=dev), torch.zeros(257, 1025, device=dev))
    with pytest.raises(RuntimeError, match='bins'):
        ops.mel_to_linear(torch.zeros(1, 2, 80, device=dev), torch.zeros(80, 1000, device=dev))


# ---------------------------------------------------------------------------------------------- Griffin-Lim from mel
def _close(got, ref, rel_l2, max_abs, what):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    scale = float(ref.abs().max())
    rl2 = float((got - ref).norm() / ref.norm())
    ma = float((got - ref).abs().max())
    print('%s: rel L2 %.2e, max-abs %.2e (scale %.3g)' % (what, rl2, ma, scale))
    assert rl2 <= rel_l2 and ma <= max_abs * scale, (what, rl2, ma, scale)


@pytest.fixture(scope='module')
def mel_case(dev, conv):
    """B = 3, T = 12 at the configs' dimensions: a smooth normalised mel (so the signed product has a speech-like magnitude)"""
    B, T = 3, 12
    rs = np.random.RandomState(21)
    base = 0.55 + 0.25 * np.sin(np.linspace(0, 3, 80))[None, None, :] * np.cos(np.linspace(0, 2, T))[None, :, None]
    mel = (base + 0.05 * rs.randn(B, T, 80)).astype(np.float32)
    return dict(B=B, T=T, mel=torch.from_numpy(mel).to(dev), phases=_phases((B, 1025, T), 8), basis=conv.mel_basis(dev))


@pytest.mark.parametrize('n_iter', [1, 30])
def test_mel_griffin_lim(dev, mel_case, n_iter):
    """with the basis == on |mel_to_linear| as amplitude, bitwise; and against the float64 oracle fed the device's float32
    amplitude, at the tolerances of test_gpu_audio.py for this comparison (rel L2 1e-4, max-abs 1e-3 of scale)"""
    from semi_tts_amd import ops
    c = mel_case
    ph = torch.from_numpy(c['phases']).to(dev)
    got = ops.griffin_lim_batch(c['mel'], ph, *DIMS, n_iter=n_iter, normalized=True, basis=c['basis'])
    amp = ops.mel_to_linear(c['mel'], c['basis'], normalized=True).abs()
    via = ops.griffin_lim_batch(amp, ph, *DIMS, n_iter=n_iter, normalized=False)
    assert torch.equal(got, via)
    ref = O.griffin_lim(amp.cpu().double().transpose(1, 2), torch.from_numpy(c['phases']), n_iter)
    _close(got.cpu(), ref, 1e-4, 1e-3, 'GL from mel, %d iterations' % n_iter)


def test_mel_to_wave_end_to_end(dev, conv, mel_case):
    from semi_tts_amd import ops
    c = mel_case
    ph = torch.from_numpy(c['phases']).to(dev)
    wav, sr = conv.mel_to_wave(c['mel'], phases=c['phases'])
    assert sr == SR and wav.dtype == np.float64 and wav.shape == (c['B'], 275 * (c['T'] - 1))
    dev_wav = conv.gen_wav_device(c['mel'], c['phases'], mel=True)
    assert np.array_equal(wav, dev_wav.cpu().numpy().astype(np.float64))
    amp = ops.mel_to_linear(c['mel'], c['basis'], normalized=True, take_abs=True)
    chain = ops.griffin_lim(amp, ph, *DIMS, n_iter=30, normalized=False, post=ops.GL_CLIP | ops.GL_INV_PREEMPHASIS)
    assert torch.equal(dev_wav, chain)
    one, _ = conv.mel_to_wave(c['mel'][1].cpu(), phases=c['phases'][1])           # (T, n_mels) from the host
    assert np.array_equal(one, wav[1])
    spec = conv.melspecgram_to_specgram(c['mel'].transpose(1, 2))                  # the reference method: (B, n_mels, T) -> (B, F, T), signed
    assert spec.shape == (c['B'], 1025, c['T']) and bool((spec < 0).any())
    assert torch.equal(spec.abs().transpose(1, 2), amp)


def test_mel_input_refuses_power(dev, mel_case):
    from semi_tts_amd import ops
    c = mel_case
    with pytest.raises(RuntimeError, match='power'):
        ops.griffin_lim_batch(c['mel'], torch.from_numpy(c['phases']).to(dev), *DIMS, n_iter=1, normalized=True, power=1.5, basis=c['basis'])


# ---------------------------------------------------------------------------------------------- ragged batches
RAGGED = [((2048, 275, 1102), 23, [23, 22, 6, 5]),                   # 5 is the minimum for these dimensions
          ((512, 64, 400), 15, [15, 6])]


@pytest.mark.parametrize('post', [0, 3])
@pytest.mark.parametrize('kind', ['linear', 'mel'])
@pytest.mark.parametrize('dims,T,frames', RAGGED, ids=['2048', '512'])
def test_ragged_batch_equals_each_utterance_alone(dev, dims, T, frames, kind, post):
    """row b on [0, L_b) is bitwise the existing Griffin-Lim of utterance b alone, trimmed to T_b frames with its phase columns;
    zero beyond L_b; feat rows and phase columns t >= T_b hold NaN and are never read"""
    from semi_tts_amd import ops
    n_fft, hop, win = dims
    F, B = n_fft // 2 + 1, len(frames)
    n_mels = 80 if n_fft == 2048 else 40
    rs = np.random.RandomState(n_fft + post)
    basis = torch.from_numpy(_basis(n_fft, n_mels)).to(dev) if kind == 'mel' else None
    feat = rs.uniform(0.3, 0.9, (B, T, n_mels if kind == 'mel' else F)).astype(np.float32)
    phases = _phases((B, F, T), 9)
    for b, n in enumerate(frames):
        feat[b, n:], phases[b, :, n:] = np.nan, np.nan
    fd, pd = torch.from_numpy(feat).to(dev), torch.from_numpy(phases).to(dev)
    kw = dict(n_iter=2, normalized=True, post=post)
    got = ops.griffin_lim_batch(fd, pd, n_fft, hop, win, basis=basis, frames=torch.tensor(frames, dtype=torch.int32, device=dev), **kw)
    assert got.shape == (B, hop * (T - 1))
    for b, n in enumerate(frames):
        Lb = hop * (n - 1)
        one = fd[b:b + 1, :n]
        if kind == 'mel':                                            # the existing path takes the magnitude
            one = ops.mel_to_linear(one, basis, normalized=True, take_abs=True)
        alone = ops.griffin_lim(one, pd[b:b + 1, :, :n].contiguous(), n_fft, hop, win, n_iter=2, normalized=kind != 'mel', post=post)
        assert bool(torch.isfinite(alone).all())
        assert torch.equal(got[b, :Lb], alone[0]), (b, n)
        assert bool((got[b, Lb:] == 0).all()), (b, n)


@pytest.mark.parametrize('dims,T,frames', RAGGED, ids=['2048', '512'])
def test_ragged_through_the_converter(dev, dims, T, frames):
    """the same property through audio.griffin_lim / specgram_to_waveform (the reference-shaped methods) and vocode_batch"""
    from semi_tts_amd import audio
    n_fft, hop, win = dims
    F = n_fft // 2 + 1
    cv = audio.AudioConverter(F, 40, 1000.0 * win / SR + 1e-6, 1000.0 * hop / SR + 1e-6, 0.97, SR)
    assert (cv.n_fft, cv.hop_length, cv.win_length) == dims
    rs = np.random.RandomState(4)
    feats = [rs.uniform(0.3, 0.9, (n, F)).astype(np.float32) for n in frames]
    np.random.seed(13)
    wavs = cv.vocode_batch(feats, 'spec')
    np.random.seed(13)
    for f, w in zip(feats, wavs):
        ph = audio.draw_phases((F, f.shape[0]))
        alone = cv.specgram_to_waveform(torch.from_numpy(f).t().to(dev), phases=ph)
        assert w.shape == (hop * (f.shape[0] - 1),) and np.array_equal(w, alone)


@pytest.mark.parametrize('kind', ['linear', 'mel'])
def test_frames_none_is_the_uniform_vocoder(dev, mel_case, kind):
    """ops.griffin_lim is ops.griffin_lim_batch without basis / frames since the uniform entry point was removed, so the first linear
    assertion compares one routine with itself; the second of each kind (frames = T everywhere against frames = None) still compares
    the ragged kernels with the uniform ones"""
    from semi_tts_amd import ops
    c = mel_case
    ph = torch.from_numpy(c['phases']).to(dev)
    full = torch.full((c['B'],), c['T'], dtype=torch.int32, device=dev)
    kw = dict(n_iter=2, normalized=True, post=3)
    if kind == 'linear':
        lin = torch.from_numpy(np.random.RandomState(2).uniform(0.2, 0.9, (c['B'], c['T'], 1025)).astype(np.float32)).to(dev)
        want = ops.griffin_lim(lin, ph, *DIMS, **kw)
        assert torch.equal(ops.griffin_lim_batch(lin, ph, *DIMS, **kw), want)
        assert torch.equal(ops.griffin_lim_batch(lin, ph, *DIMS, frames=full, **kw), want)
    else:
        want = ops.griffin_lim_batch(c['mel'], ph, *DIMS, basis=c['basis'], **kw)
        assert torch.equal(ops.griffin_lim_batch(c['mel'], ph, *DIMS, basis=c['basis'], frames=full, **kw), want)


def test_out_of_range_frame_counts_are_clamped(dev, mel_case):
    """the kernels clamp frames[b] into [minimum, T] (the wrapper above them validates): nothing outside the workspace is touched"""
    from semi_tts_amd import ops
    c = mel_case
    ph = torch.from_numpy(c['phases']).to(dev)
    kw = dict(n_iter=1, normalized=True, basis=c['basis'])
    wild = torch.tensor([-7, 0, 10 ** 6], dtype=torch.int32, device=dev)
    tame = torch.tensor([5, 5, c['T']], dtype=torch.int32, device=dev)
    assert torch.equal(ops.griffin_lim_batch(c['mel'], ph, *DIMS, frames=wild, **kw), ops.griffin_lim_batch(c['mel'], ph, *DIMS, frames=tame, **kw))


# ---------------------------------------------------------------------------------------------- main.py --vocode-dir
@pytest.mark.parametrize('kind,D', [('spec', 1025), ('mel', 80)])
def test_vocode_dir_entry_point(dev, conv, tmp_path, kind, D):
    from semi_tts_amd.audio import write_wav
    lens = {'b': 9, 'a': 14, 'c': 5}
    rs = np.random.RandomState(6)
    feats = {k: rs.uniform(0.3, 0.9, (n, D)).astype(np.float32) for k, n in lens.items()}
    d = tmp_path / 'feats'
    os.makedirs(d)
    for k, f in feats.items():
        np.save(d / ('%s-%s.npy' % (k, kind)), f)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'main.py'), '--config', os.path.join(REPO, 'config', 'supervised.yaml'),
                        '--vocode-dir', str(d), '--vocode-feat', kind, '--batch-size', '8', '--logdir', str(tmp_path / 'log'),
                        '--name', 'voc', '--seed', '5'], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = tmp_path / 'log' / 'voc'
    assert sorted(os.listdir(out)) == ['a.wav', 'b.wav', 'c.wav']
    np.random.seed(5)                                                # main.py seeds np.random with --seed before the solver runs
    want = conv.vocode_batch([feats[k] for k in sorted(feats)], kind)
    for k, w in zip(sorted(feats), want):
        with wave.open(str(out / (k + '.wav')), 'rb') as f:
            assert (f.getframerate(), f.getnchannels(), f.getnframes()) == (SR, 1, 275 * (lens[k] - 1))
            pcm = f.readframes(f.getnframes())
        write_wav(str(tmp_path / 'want.wav'), w, SR)
        with wave.open(str(tmp_path / 'want.wav'), 'rb') as f:
            assert pcm == f.readframes(f.getnframes()), k
