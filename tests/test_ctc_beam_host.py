"""CPU checks of the CTC prefix beam search feature: the float64 oracle against brute force, the argument checks of the ops layer (they
fire before any device is touched), the --transcribe-wav-dir parser rules, and the .phn formatting."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import ctc_beam_oracle as O  # noqa: E402


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@pytest.mark.parametrize('T,V,blank,seed', [(1, 2, 0, 0), (3, 2, 0, 1), (6, 2, 1, 2), (4, 3, 0, 3), (5, 3, 2, 4), (6, 3, 0, 5),
                                            (3, 4, 0, 6), (4, 4, 3, 7)])
def test_unpruned_oracle_equals_brute_force(T, V, blank, seed):
    """with a beam wide enough for every reachable prefix the search is exact: the same labellings, best first, the same scores"""
    lp = np.log(_softmax(np.random.RandomState(seed).randn(T, V) * 2.0))
    W = O.n_prefixes(T, V)
    hyps, scores, _ = O.beam_search(lp, W, W, blank)
    bf = O.brute_force(lp, blank)
    finite = [(h, s) for h, s in zip(hyps, scores) if np.isfinite(s)]
    bf_finite = [(h, s) for h, s in bf if np.isfinite(s)]
    assert [h for h, _ in finite] == [h for h, _ in bf_finite]
    np.testing.assert_allclose([s for _, s in finite], [s for _, s in bf_finite], rtol=0, atol=1e-12)
    assert len(hyps) == len(set(hyps)) == W            # every prefix exactly once: merging is exact


def test_oracle_edge_cases():
    lp = np.log(_softmax(np.random.RandomState(0).randn(4, 3)))
    hyps, scores, _ = O.beam_search(lp[:0], 4, 3)
    assert hyps == [(), (), ()] and scores[0] == 0.0 and np.all(scores[1:] == -np.inf)
    bad = lp.copy()
    bad[2, 1] = np.nan
    hyps, scores, _ = O.beam_search(bad, 4, 2)
    assert hyps == [(), ()] and np.isnan(scores).all()
    h, s, _ = O.batch_beam_search(np.exp(lp)[None], [2], 2, 1)
    assert h[0] == O.beam_search(np.log(np.exp(lp)[:2] + 1e-10), 2, 1)[0]


def test_levenshtein_does_not_collapse():
    assert O.levenshtein((5, 5), (5,)) == 1
    assert O.levenshtein((3, 4, 5), (3, 5)) == 1 and O.levenshtein((), (1, 2)) == 2


def _no_device(monkeypatch):
    from semi_tts_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'load', no_device)


def _cuda_view(t):
    # the ops checks read .is_cuda / .device / .shape / .dtype only: a meta tensor stands in for a device tensor on the CPU
    return t.to('meta')


def test_beam_search_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops
    _no_device(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    good = _cuda_view(torch.rand(2, 5, 4))
    cases = [
        (dict(prob=torch.rand(2, 5, 4)), 'GPU tensor'),                     # a CPU tensor
        (dict(prob=[[0.5]]), 'GPU tensor'),
        (dict(prob=_cuda_view(torch.rand(2, 5, 4, dtype=torch.float64))), 'float32'),
        (dict(prob=_cuda_view(torch.rand(5, 4))), 'float32'),
        (dict(prob=_cuda_view(torch.rand(0, 5, 4))), 'B=0'),
        (dict(prob=_cuda_view(torch.rand(1, 4097, 4))), 'T=4097'),
        (dict(prob=_cuda_view(torch.rand(1, 5, 1))), 'V=1'),
        (dict(prob=_cuda_view(torch.rand(1, 5, 1025))), 'V=1025'),
        (dict(prob=good, beam_width=0), 'beam_width'),
        (dict(prob=good, beam_width=129), 'beam_width'),
        (dict(prob=good, beam_width=4, top_paths=5), 'top_paths'),
        (dict(prob=good, top_paths=0), 'top_paths'),
        (dict(prob=good, blank=4), 'blank'),
        (dict(prob=good, blank=-1), 'blank'),
        (dict(prob=good, eps=-1.0), 'eps'),
        (dict(prob=good, lengths=[1, 6]), 'lengths'),
        (dict(prob=good, lengths=[1, -1]), 'lengths'),
        (dict(prob=good, lengths=[1]), 'lengths'),
        (dict(prob=good, lengths=torch.tensor([1.0, 2.0])), 'lengths'),
        (dict(prob=good, lengths=_cuda_view(torch.tensor([1, 2, 3]))), 'lengths'),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.ctc_beam_search(**kw)
    from semi_tts_amd import ctc_decode
    with pytest.raises(ValueError, match='beam_width'):
        ctc_decode.beam_search(good, beam_width=200)


def test_hyp_edit_distance_argument_checks_fire_before_the_device(monkeypatch):
    from semi_tts_amd import ops
    _no_device(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta')))
    hyp = _cuda_view(torch.zeros(2, 5, dtype=torch.int64))
    hl = _cuda_view(torch.zeros(2, dtype=torch.int32))
    text = _cuda_view(torch.zeros(2, 3, dtype=torch.int64))
    cases = [
        (([[1]], hl, text, ()), 'tensors'),
        ((torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64), ()), 'one GPU'),
        ((hyp.float(), hl, text, ()), 'int64'),
        ((hyp, hl, text.view(-1), ()), 'int64'),
        ((hyp, hl.long(), text, ()), 'int32'),
        ((hyp, _cuda_view(torch.zeros(3, dtype=torch.int32)), text, ()), 'hyp_len'),
        ((hyp, hl, _cuda_view(torch.zeros(3, 3, dtype=torch.int64)), ()), 'hypotheses'),
        ((_cuda_view(torch.zeros(2, 4097, dtype=torch.int64)), hl, text, ()), 'Lh=4097'),
        ((hyp, hl, _cuda_view(torch.zeros(2, 1025, dtype=torch.int64)), ()), 'L=1025'),
        ((hyp, hl, text, tuple(range(65))), 'ignored'),
        ((hyp, hl, text, (2 ** 31,)), 'int32'),
    ]
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.hyp_edit_distance(*args)


def _entry():
    sys.path.insert(0, REPO)
    import main as entry
    return entry


def test_transcribe_flags_parse():
    entry = _entry()
    p = entry.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml', '--transcribe-wav-dir', 'wavs', '--beam-width', '8',
                          '--top-paths', '3', '--vocab', 'phn.vocab', '--asr-output', 'post', '--batch-size', '4'])
    assert (p.transcribe_wav_dir, p.beam_width, p.top_paths, p.vocab, p.asr_output, p.batch_size) == ('wavs', 8, 3, 'phn.vocab', 'post', 4)
    p = entry.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml', '--transcribe-wav-dir', 'wavs'])
    assert (p.beam_width, p.top_paths, p.vocab, p.asr_output) == (16, 1, None, 'code')
    p = entry.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml'])
    assert p.transcribe_wav_dir is None


_NO_COMBINE = '--transcribe-wav-dir does not combine with --'
_BOUNDS = '--transcribe-wav-dir needs 1 <= --top-paths <= --beam-width <= 128'


@pytest.mark.parametrize('extra,msg', [(['--gen-specgram'], _NO_COMBINE + 'gen-specgram'), (['--tts-only'], _NO_COMBINE + 'tts-only'),
                                       (['--dev-batches', '2'], _NO_COMBINE + 'dev-batches'),
                                       (['--unpair-wav-dir', 'u'], _NO_COMBINE + 'unpair-wav-dir'),
                                       (['--beam-width', '0'], _BOUNDS), (['--beam-width', '129'], _BOUNDS),
                                       (['--beam-width', '4', '--top-paths', '5'], _BOUNDS), (['--top-paths', '0'], _BOUNDS),
                                       (['--asr-output', 'logits'], "--asr-output: invalid choice: 'logits'")])
def test_transcribe_flag_refusals(extra, msg, capsys):
    """the refusals name the rule of the new mode (an argparse 'unrecognized arguments' error would echo the flags too)"""
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml', '--transcribe-wav-dir', 'wavs'] + extra)
    assert msg in capsys.readouterr().err


def test_asr_decode_is_still_refused_with_the_new_flag(capsys):
    entry = _entry()
    with pytest.raises(SystemExit):
        entry.parse_args(['--config', 'config/supervised.yaml', '--asr-decode', '--transcribe-wav-dir', 'wavs'])
    assert 'not part of the reference tree' in capsys.readouterr().err


def test_vocab_and_phn_format(tmp_path):
    from semi_tts_amd.solver import read_vocab, format_phn
    v = tmp_path / 'phn.vocab'
    v.write_text('AA\nAE\n\nAH\n')
    vocab = read_vocab(str(v))
    assert vocab == ['<pad>', '<space>', '<eos>', 'AA', 'AE', 'AH']
    txt = format_phn([-1.5, float('-inf')], [[3, 5, 3, 1], []], vocab)
    assert txt == '-1.500000\tAA AH AA <space>\n-inf\t\n'
    assert format_phn([-0.25], [[4, 9]], None) == '-0.250000\t4 9\n'
    assert format_phn([-0.25], [[4, 9]], vocab) == '-0.250000\tAE 9\n'       # an id past the vocabulary: its number


def test_encoder_lengths_follow_the_conv_stack():
    """VQVAE.encoder_lengths is each ConvLayer.out_len in turn (kernel 4 / stride 2 of the shipped configs halves the frames)"""
    from semi_tts_amd.asr import ConvLayer
    layers = [ConvLayer(4, 4, k, s, False, False, 'relu', 0.0) for k, s in zip([3, 4, 3, 3, 3, 1], [1, 2, 1, 1, 1, 1])]

    class Fake:
        pass
    m = Fake()
    m.asr = Fake()
    m.asr.layers = len(layers)
    for i, l in enumerate(layers):
        setattr(m.asr, 'layer%d' % i, l)
    from semi_tts_amd.vqvae import VQVAE
    got = VQVAE.encoder_lengths(m, [0, 1, 2, 256, 257])
    want = []
    for t in [0, 1, 2, 256, 257]:
        for l in layers:
            t = (t + 2 * l.padding - l.conv.kernel_size[0]) // l.stride + 1
        want.append(t)
    assert got.tolist() == want and want[3] == 128
