"""The synthesis kernels of semi_tts_amd/csrc/audio.hip on the MI355X at every FFT size and framing edge (tests/audio_cases.py)
against the float64 oracle (tests/gl_oracle.py): STFT / iSTFT lengths and window parities, Griffin-Lim at 512 / 1024 / 4096, the
options and strides of specgram_to_waveform / ops.griffin_lim, and the de-emphasis scan of the final overlap-add at its tile edges.

The de-emphasis scan in isolation (test_deemphasis_scan_at_tile_edges): bound 8 x the serial float32 error on the actual input; the
measured ratio got / serial is printed per case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_cases as A   # noqa: E402
import gl_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


def _close(got, ref, tol, what):
    """test_gpu_audio._close: rel-L2 <= tol[0], max-abs <= tol[1] x scale"""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    if got.is_complex() or ref.is_complex():
        got, ref = torch.view_as_real(got.to(torch.complex128)), torch.view_as_real(ref.to(torch.complex128))
    got, ref = got.double(), ref.double()
    scale = float(ref.abs().max())
    rl2 = float((got - ref).norm() / ref.norm())
    ma = float((got - ref).abs().max())
    print('%s: rel L2 %.2e, max-abs %.2e (scale %.3g)' % (what, rl2, ma, scale))
    assert rl2 <= tol[0] and ma <= tol[1] * scale, (what, rl2, ma, scale)


def _to_frames(spec_bft):
    """(B, F, T) complex -> the library's frame-major (B, T, F, 2) float32"""
    return torch.view_as_real(spec_bft.transpose(1, 2).to(torch.complex64).contiguous()).contiguous()


def _from_frames(spec_btf2):
    return torch.view_as_complex(spec_btf2.cpu().double().contiguous()).transpose(1, 2)


# ---------------------------------------------------------------- A. STFT / iSTFT edges
@pytest.mark.parametrize('signal', sorted(A.SIGNALS))
@pytest.mark.parametrize('p', A.with_batches(A.STFT_CASES), ids=A.case_id)
def test_stft_edges(dev, p, signal):
    from semi_tts_amd import ops
    case, B = p
    n_fft, hop, win, L = case
    x = A.stft_input(case, B, signal)
    got = ops.stft_fwd(x.to(dev), n_fft, hop, win)
    assert got.shape == (B, A.n_frames(hop, L), n_fft // 2 + 1, 2)
    _close(_from_frames(got), A.stft_reference(x, case), A.STFT_TOL, 'stft %s %s' % (A.case_id(p), signal))


@pytest.mark.parametrize('signal', sorted(A.SIGNALS))
@pytest.mark.parametrize('p', A.with_batches(A.ISTFT_CASES), ids=A.case_id)
def test_istft_edges(dev, p, signal):
    from semi_tts_amd import ops
    case, B = p
    n_fft, hop, win, L = case
    spec = _to_frames(A.stft_reference(A.stft_input(case, B, signal), case))
    got = ops.istft(spec.to(dev), n_fft, hop, win)
    assert got.shape == (B, hop * (A.n_frames(hop, L) - 1))
    _close(got.cpu(), A.istft_reference(_from_frames(spec), case), A.STFT_TOL, 'istft %s %s' % (A.case_id(p), signal))


@pytest.mark.parametrize('kind,dims,n,words', A.REFUSALS, ids=lambda v: str(v).replace(' ', ''))
def test_documented_refusals(dev, kind, dims, n, words):
    from semi_tts_amd import ops
    n_fft, hop, win = dims
    with pytest.raises(RuntimeError, match=words):
        if kind == 'stft':
            ops.stft_fwd(torch.zeros(1, n, device=dev), n_fft, hop, win)
        else:
            ops.istft(torch.zeros(1, n, n_fft // 2 + 1, 2, device=dev), n_fft, hop, win)


def test_istft_refuses_the_short_stft_cases(dev):
    from semi_tts_amd import audio, ops
    for n_fft, hop, win, L in A.ISTFT_REFUSED:
        T = A.n_frames(hop, L)
        with pytest.raises(RuntimeError, match='reflect'):
            ops.istft(torch.zeros(1, T, n_fft // 2 + 1, 2, device=dev), n_fft, hop, win)
        with pytest.raises(ValueError, match='too few'):
            audio.griffin_lim(torch.ones(1, n_fft // 2 + 1, T, device=dev), n_fft=n_fft, hop=hop, win=win)


# ---------------------------------------------------------------- B. Griffin-Lim at every size and option
_GL = {}


def _gl_case(dims, zero):
    """inputs and the float64 references of one size, computed once for its three iteration counts"""
    key = (dims, zero)
    if key not in _GL:
        amp, ph = A.gl_input(dims, zero_frames=zero)
        _GL[key] = (amp, ph, {n: A.gl_reference(amp, ph, n, dims) for n in A.GL_ITERS})
    return _GL[key]


@pytest.mark.parametrize('n_iter', A.GL_ITERS)
@pytest.mark.parametrize('dims', A.GL_DIMS, ids=str)
def test_griffin_lim_sizes(dev, dims, n_iter):
    from semi_tts_amd import audio
    amp, ph, refs = _gl_case(dims, False)
    got = audio.griffin_lim(amp.to(dev), phases=ph, n_iter=n_iter, n_fft=dims[0], hop=dims[1], win=dims[2])
    assert got.shape == refs[n_iter].shape
    _close(got.cpu(), refs[n_iter], A.GL_TOL, 'GL %s, %d iterations' % (dims, n_iter))


@pytest.mark.parametrize('n_iter', A.GL_ITERS)
def test_griffin_lim_zero_frames_at_1024(dev, n_iter):
    from semi_tts_amd import audio
    dims = A.GL_ZERO_DIMS
    amp, ph, refs = _gl_case(dims, True)
    got = audio.griffin_lim(amp.to(dev), phases=ph, n_iter=n_iter, n_fft=dims[0], hop=dims[1], win=dims[2])
    _close(got.cpu(), refs[n_iter], A.GL_TOL, 'GL %s with zero frames, %d iterations' % (dims, n_iter))


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd.audio import load_audio_transform
    return load_audio_transform(num_freq=1025, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, preemphasis_coeff=0.97,
                                sample_rate=22050)


@pytest.mark.parametrize('name', sorted(A.OPTION_CASES))
def test_specgram_to_waveform_options(dev, conv, name):
    spec, ph, kw = A.option_input(name)
    ref = A.option_reference(spec, ph, kw)
    got = conv.specgram_to_waveform(spec.to(dev), phases=ph, **kw)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert float(np.abs(got).max()) == 1.0                              # the clip is reached and holds
    _close(got, ref, A.GL_TOL, 'specgram_to_waveform %s' % name)
    if name == 'is_amp':                                                # the power is ignored with isAmp
        assert np.array_equal(got, conv.specgram_to_waveform(spec.to(dev), phases=ph, isAmp=True))
    if name == 'two_d':                                                 # and equals its row of the batched call
        spec3, ph3, _ = A.option_input('two_d')
        both = conv.specgram_to_waveform(spec3[None].to(dev), phases=ph3[None])
        assert np.array_equal(both[0], got)


def test_griffin_lim_zero_iterations_through_the_converter(dev, conv):
    spec, ph, kw = A.option_input('power')
    kw['n_iter'] = 0
    got = conv.specgram_to_waveform(spec.to(dev), phases=ph, **kw)
    _close(got, A.option_reference(spec, ph, kw), A.GL_TOL, 'specgram_to_waveform n_iter = 0')


def test_unclipped_deemphasis_exceeds_one(dev):
    """post = GL_INV_PREEMPHASIS alone: the output passes 1 and the carry runs on the unclipped values"""
    from semi_tts_amd import ops
    amp, ph = A.unclipped_input()
    feat = amp.to(dev).transpose(1, 2)
    got = ops.griffin_lim(feat, torch.from_numpy(ph).to(dev), O.N_FFT, O.HOP, O.WIN, post=ops.GL_INV_PREEMPHASIS).cpu()
    ref = A.option_reference(amp, ph, dict(isAmp=True), clip=False)
    assert float(got.abs().max()) > 1.5
    _close(got, ref, A.GL_TOL, 'de-emphasis without clip')
    clipped = ops.griffin_lim(feat, torch.from_numpy(ph).to(dev), O.N_FFT, O.HOP, O.WIN,
                              post=ops.GL_INV_PREEMPHASIS | ops.GL_CLIP).cpu()
    assert torch.equal(clipped, got.clamp(-1, 1))                      # the clip is applied after the scan, not inside it


@pytest.mark.parametrize('layout', ['time_slice', 'transposed', 'channel_slice'])
def test_griffin_lim_reads_any_strides(dev, layout):
    from semi_tts_amd import ops
    spec, ph, _ = A.option_input('power')                               # (B, F, T) normalised
    B, F, T = spec.shape
    feat = spec.transpose(1, 2).contiguous().to(dev)                    # (B, T, F)
    phd = torch.from_numpy(ph).to(dev)
    kw = dict(n_iter=3, normalized=True, power=1.5, post=ops.GL_INV_PREEMPHASIS | ops.GL_CLIP)
    want = ops.griffin_lim(feat, phd, O.N_FFT, O.HOP, O.WIN, **kw)
    if layout == 'time_slice':
        big = torch.full((B, T + 4, F), 7.0, device=dev)
        big[:, 2:T + 2] = feat
        view = big[:, 2:T + 2, :]
    elif layout == 'transposed':
        view = spec.to(dev).contiguous().transpose(1, 2)
    else:
        big = torch.full((B, T, 2 * F), 7.0, device=dev)
        big[..., ::2] = feat
        view = big[..., ::2]
    assert view.shape == feat.shape and view.stride() != feat.stride() and torch.equal(view, feat)
    assert torch.equal(ops.griffin_lim(view, phd, O.N_FFT, O.HOP, O.WIN, **kw), want)


# ---------------------------------------------------------------- C. the de-emphasis scan at its tile edges
@pytest.mark.parametrize('hop,T', A.OLA_CASES)
def test_deemphasis_scan_at_tile_edges(dev, hop, T):
    """n_iter = 0 twice on one input, post = 0 and post = GL_INV_PREEMPHASIS: both launches compute identical pre-scan samples, so
    the first output through scipy's lfilter in float64 is the reference of the second and only the scan is compared"""
    from semi_tts_amd import ops
    amp, ph = A.ola_input(hop, T)
    feat = amp.to(dev).transpose(1, 2)
    phd = torch.from_numpy(ph).to(dev)
    L = hop * (T - 1)
    x = ops.griffin_lim(feat, phd, A.OLA_N_FFT, hop, A.OLA_WIN, n_iter=0, post=0).cpu().numpy()
    got = ops.griffin_lim(feat, phd, A.OLA_N_FFT, hop, A.OLA_WIN, n_iter=0, post=ops.GL_INV_PREEMPHASIS).cpu().numpy()
    assert x.shape == got.shape == (A.OLA_B, L)
    bound, ref = A.deemph_bound(x)
    err = np.abs(got.astype(np.float64) - ref)
    scale = float(np.abs(ref).max())
    print('de-emphasis scan L=%d: max-abs / scale %.2e at sample %d, serial float32 %.2e, ratio %.2f (scale %.3g)'
          % (L, err.max() / scale, int(err.max(axis=0).argmax()), bound / A.DEEMPH_SLACK / scale,
             err.max() * A.DEEMPH_SLACK / bound, scale))
    assert scale > 10 * float(np.abs(x).max())                           # the slowly decaying component is there
    assert err.max() <= bound, (L, float(err.max()), bound)
    # post = 0 is the plain iSTFT of that spectrum
    ref0 = O.griffin_lim(amp.double(), torch.from_numpy(ph), 0, n_fft=A.OLA_N_FFT, hop=hop, win=A.OLA_WIN)
    _close(x, ref0, A.GL_TOL, 'overlap-add L=%d' % L)
