"""main.py --corpus on the MI355X: batches fetched from the device-resident splits against the same files loaded alone (bitwise), and
the trainers on a toy corpus (tests/corpus_cases.py) at the small size of tests/test_gpu_validate.py (shipped single-speaker
configuration, B = 4)."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_cases as CC   # noqa: E402
from helpers import same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')
R = 3


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    return CC.write_toy_corpus(tmp_path_factory.mktemp('corpus'))


@pytest.fixture(scope='module')
def conv():
    from semi_tts_amd.audio import load_audio_transform
    return load_audio_transform(**yaml.safe_load(open(CONFIG))['data']['audio'])


def _splits(toy, conv, bucketing=False, **kw):
    from semi_tts_amd.corpus import load_splits
    cfg = dict(toy[0], bucketing=bucketing)
    return load_splits(cfg, conv, R, ['paired', 'unpaired', 'dev'], dict(paired=4, unpaired=3, dev=4), seed=1, verbose=lambda m: None, **kw)


def _paths(toy, ids):
    cfg, rows = toy
    by = {r['id']: r for r in rows}
    return [os.path.join(cfg['path'], by[i]['speaker'], i + '.wav') for i in ids], [by[i] for i in ids]


@pytest.mark.parametrize('bucketing', [False, True])
def test_fetched_batch_is_the_files_loaded_alone(toy, conv, bucketing):
    _, sets = _splits(toy, conv, bucketing=bucketing)
    ds = sets['paired']
    for _ in range(3):                                            # three fetches: other windows, an epoch boundary without bucketing
        mel, aug, lin, text, sid = ds.fetch()
        ids, seed, snr, stretch = ds.last_fetch
        paths, rows = _paths(toy, ids)
        wb = conv.load_batch(paths)
        assert list(wb.order) == list(range(len(ids)))            # batch order IS WaveBatch's order: longest first, stable
        assert list(wb.lens) == [r['samples'] for r in rows]
        m2, a2, l2 = conv.extract_batch(wb, r=R, seed=seed, snr=snr, stretch=stretch)
        assert mel.shape == m2.shape and aug.shape == a2.shape and lin.shape == l2.shape
        assert same_bits(mel, m2) and same_bits(aug, a2) and same_bits(lin, l2)
        # text / sid: the hand encoding, in that order, padded with 0 to the batch's longest
        L = max(len(r['tokens']) for r in rows)
        assert text.dtype == torch.int64 and text.is_contiguous() and tuple(text.shape) == (len(ids), L)
        assert text.tolist() == [r['tokens'] + [0] * (L - len(r['tokens'])) for r in rows]
        assert sid.dtype == torch.int64 and sid.tolist() == [CC.SPEAKERS[r['speaker']] for r in rows]
        # padding: mel / linear to a multiple of r with at least one extra frame, zero beyond each utterance; aug_mel to its longest
        T = [1 + r['samples'] // conv.hop_length for r in rows]
        assert mel.shape[1] % R == 0 and max(T) < mel.shape[1] <= max(T) + R
        for b, t in enumerate(T):
            assert bool((mel[b, t:] == 0).all()) and bool((lin[b, t:] == 0).all()) and bool((mel[b, t - 1] != 0).any())
        assert aug.shape[1] == max(1 + r['samples'] // conv.stretch_dims(s)[1] for r, s in zip(rows, stretch))
        assert all(s is not None and 0.9 <= st <= 1.1 for s, st in zip(snr, stretch))
    again = ds.last_fetch
    ds.fetch()
    assert ds.last_fetch[1] != again[1] or ds.last_fetch[2] != again[2]       # fresh draws per fetch


def test_window_from_the_middle_of_the_buffer(toy, conv):
    _, sets = _splits(toy, conv)
    ds = sets['unpaired']
    order = np.argsort(-ds.lens, kind='stable')
    idx = np.array([i for i in order if 0 < i < len(ds.rows) - 1][:3])      # neither the first nor the last utterance of the buffer
    wb, got = ds.window(idx[::-1])                                # any order in: longest first out
    assert list(got) == list(idx) and int(wb.offsets.min()) > 0 and int((wb.offsets + wb.lens).max()) < ds.buffer.numel()
    assert (np.diff(wb.offsets) < 0).any() or len(set(np.diff(wb.offsets + wb.lens))) > 1        # offsets that are not cumulative
    assert wb.packed(ds.buffer.device).data_ptr() == ds.buffer.data_ptr()      # nothing copied
    kw = dict(r=R, seed=12345, snr=[20.0, None, 35.0], stretch=[0.95, 1.0, 1.07])
    a = conv.extract_batch(wb, **kw)
    b = conv.extract_batch(conv.load_batch([ds.rows[i].path for i in idx]), **kw)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match='outside its buffer'):
        from semi_tts_amd.audio import WaveBatch
        WaveBatch.window(ds.buffer, [ds.buffer.numel() - 10], [11])


def test_dev_split_in_order_without_augmentation_and_the_memory_limit(toy, conv):
    _, sets = _splits(toy, conv)
    dev = sets['dev']
    assert dev.n_batches() == 1
    mel, aug, lin, text, sid = dev.fetch()
    ids, seed, snr, stretch = dev.last_fetch
    assert seed == 0 and snr == [None] * 4 and stretch == [1.0] * 4
    lens = sorted((r['samples'] for r in toy[1] if r['split'] == 'dev'), reverse=True)
    assert [r['samples'] for r in _paths(toy, ids)[1]] == lens                  # in order: longest first
    assert aug.shape[1] == 1 + lens[0] // conv.hop_length and bool(torch.isfinite(aug).all())
    first = ids
    dev.fetch()
    assert dev.last_fetch[0] == first
    with pytest.raises(ValueError, match=r'paired split \(10 utterances, \d+ samples\) needs 0\.000 GB \(\d+ bytes\) on the device, the limit is 0\.000 GB \(10737 bytes\)'):
        _splits(toy, conv, max_gb=1e-5)


def _paras(tmp, **kw):
    base = dict(name='t', logdir=str(tmp), ckpdir=str(tmp), load=None, seed=1, cpu=False, verbose=False, batch_size=4, unpair_batch_size=3,
                frames=64, n_batches=1, dev_batches=0, valid_step=None, max_step=1, store_best_per=False, corpus=True, actual_len=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _trainer(tmp, toy, cls='VqvaeTrainer', hparas=None, **kw):
    from semi_tts_amd import solver
    config = yaml.safe_load(open(CONFIG))
    config['data']['corpus'] = dict(toy[0])
    config['hparas'].update(hparas or {})
    tr = getattr(solver, cls)(config, _paras(tmp, **kw), 'train')
    tr.load_data()
    tr.set_model()
    return tr


def _params(tr):
    return {n: p.detach().clone() for n, p in tr.model.named_parameters()}


def _moved(before, tr):
    return sum(not torch.equal(before[n], p.detach()) for n, p in tr.model.named_parameters())


@pytest.fixture(scope='module')
def cycle(tmp_path_factory, toy):
    """a cycle trainer on the toy corpus after four alternating steps (speech-first with the unpaired split from step 2 on)"""
    tr = _trainer(tmp_path_factory.mktemp('cycle'), toy, dev_batches=-1, max_step=4, valid_step=1000)
    before = _params(tr)
    dev_set, tr.dev_set = tr.dev_set, []
    log = tr.exec()
    tr.dev_set = dev_set
    return tr, before, log


def test_four_cycle_steps_on_the_corpus(cycle):
    tr, before, log = cycle
    assert tr.vocab_size == 9 and tr.n_spkr == 2 and tr.model.spkr_embed.weight.shape[0] == 2
    assert [st['kind'] for st in log] == ['speech_first', 'text_first'] * 2
    assert all(math.isfinite(st['loss']) and math.isfinite(st['grad_norm']) for st in log)
    assert 'unpair_text_len' in log[2] and 'unpair_text_len' not in log[0]       # the unpaired split joins after the start step
    assert math.isfinite(log[2].get('unpair_speech_loss', 0.0))                   # (absent when an unpaired utterance decoded to all blank)
    assert _moved(before, tr) > len(before) // 2
    assert tr.unpair_set.last_fetch is not None and tr.pair_set.last_fetch is not None


def test_validate_walks_the_dev_split(cycle):
    tr = cycle[0]
    assert len(tr.dev_set) == tr.corpus_sets['dev'].n_batches() == 1
    tts, per, post = tr.validate()
    assert math.isfinite(tts) and math.isfinite(per) and per >= 0.0 and post is None
    ids = tr.corpus_sets['dev'].last_fetch[0]
    assert sorted(ids) == sorted(r['id'] for r in CC.toy_rows() if r['split'] == 'dev')
    again = tr.validate()
    assert again[1] == per                                         # the same batches from the start, clean mel: the same PER


def test_trainer_ctc_loss_takes_the_frame_counts(cycle):
    from semi_tts_amd import autograd as AG
    from semi_tts_amd import ops
    tr = cycle[0]
    mel, aug, lin, text, sid = tr.pair_set.fetch()
    f = int(tr.model.time_reduce_factor)
    T = aug.shape[1] // f
    prob = torch.softmax(torch.randn(aug.shape[0], T, tr.vocab_size, device=aug.device), dim=-1)
    in_len = ops.frame_lengths(aug, 0.0, f)
    a = aug.cpu()
    assert in_len.tolist() == (torch.sum((a == 0).long().sum(dim=-1) != a.shape[-1], dim=-1) // f).tolist()      # bin/train_vqvae.py:437-438
    by = {u.id: u.samples for u in tr.pair_set.rows}
    ids, _, _, stretch = tr.pair_set.last_fetch
    frames = [1 + by[i] // tr.audio_converter.stretch_dims(s)[1] for i, s in zip(ids, stretch)]
    assert all(n <= m // f for n, m in zip(in_len.tolist(), frames)) and min(in_len.tolist()) < T       # ragged: the lengths matter
    plain = tr.ctc_loss(prob, text, aug)
    assert same_bits(plain, AG.ctc_loss(prob, text, 1e-10))       # without --actual-len: every frame
    tr.paras.actual_len = True
    try:
        got = tr.ctc_loss(prob, text, aug)
        lp = torch.log(prob)
        got_log = tr.ctc_loss(lp, text, aug, apply_log=False)
    finally:
        tr.paras.actual_len = False
    assert same_bits(got, AG.ctc_loss(prob, text, 1e-10, in_len=in_len))
    assert same_bits(got_log, AG.ctc_loss(lp, text, 1e-10, apply_log=False, in_len=in_len))
    assert float(got) != float(plain)


def test_two_steps_with_actual_len(tmp_path, toy):
    """speech-first, then text-first with the unpaired text (its weight raised above the shipped 0): both CTC forms of --actual-len"""
    tr = _trainer(tmp_path, toy, hparas=dict(unpair_text_weight=1.0), actual_len=True, max_step=2)
    before = _params(tr)
    log = tr.exec()
    assert [st['kind'] for st in log] == ['speech_first', 'text_first']
    assert all(math.isfinite(st['loss']) and math.isfinite(st['grad_norm']) and math.isfinite(st['asr_loss']) for st in log)
    assert 'unpair_text_loss' in log[1] and math.isfinite(log[1]['unpair_text_loss'])
    assert _moved(before, tr) > 0


def test_two_tts_only_steps(tmp_path, toy):
    tr = _trainer(tmp_path, toy, cls='TtsTrainer', max_step=2)
    assert tr.vocab_size == 9 and tr.n_spkr == 2 and sorted(tr.corpus_sets) == ['paired']
    before = _params(tr)
    log = tr.exec()
    assert len(log) == 2 and all(math.isfinite(float(st['loss'])) and math.isfinite(float(st['grad_norm'])) for st in log)
    assert _moved(before, tr) > 0


def test_load_of_another_speaker_table_is_refused(tmp_path, toy, cycle):
    tr = cycle[0]
    sd = {k: v for k, v in tr.model.state_dict().items()}
    sd['spkr_embed.weight'] = torch.zeros(109, sd['spkr_embed.weight'].shape[1])
    path = str(tmp_path / 'other.pth')
    torch.save({'model': sd, 'global_step': 0}, path)
    tr.paras.load = path
    try:
        with pytest.raises(ValueError, match=r'disagrees with the corpus \(vocab_size 9, n_spkr 2\): the checkpoint has 109 speakers'):
            tr.load_ckpt()
    finally:
        tr.paras.load = None
