"""VqvaeTrainer.validate (bin/train_vqvae.py:330-428) on the MI355X, on the shipped single-speaker configuration at a small size
(B = 4, 64 frames): no side effects on the training state, PER and TTS loss against direct recomputations, and main.py end to end with
the reference's checkpoint rules."""
import copy
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')


def _trainer(tmp, postnet=False, dev_batches=2):
    from semi_tts_amd.solver import VqvaeTrainer
    config = yaml.safe_load(open(CONFIG))
    if postnet:
        config['model']['asr_postnet_weight'] = 0.5
    paras = types.SimpleNamespace(name='t', logdir=str(tmp), ckpdir=str(tmp), load=None, seed=1, cpu=False, verbose=False, batch_size=4,
                                  frames=64, n_batches=1, dev_batches=dev_batches, valid_step=None, max_step=1, store_best_per=False)
    tr = VqvaeTrainer(config, paras, 'train')
    tr.load_data()
    tr.set_model()
    return tr


def _flat(x, out, key=''):
    if torch.is_tensor(x):
        out[key] = x.detach().clone()
    elif isinstance(x, dict):
        for k in x:
            _flat(x[k], out, '%s/%s' % (key, k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _flat(v, out, '%s/%d' % (key, i))
    else:
        out[key] = copy.deepcopy(x)
    return out


def _state(tr):
    s = {}
    for n, p in tr.model.named_parameters():
        s['p/' + n] = p.detach().clone()
        s['g/' + n] = None if p.grad is None else p.grad.detach().clone()
    for n, b in tr.model.named_buffers():
        s['b/' + n] = b.detach().clone()
    _flat(tr.optimizer.get_opt_state_dict(), s, 'opt')
    return s


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and \
            a.cpu().reshape(-1).view(torch.uint8).equal(b.cpu().reshape(-1).view(torch.uint8))
    return a == b


@pytest.mark.parametrize('postnet', [False, True])
def test_validate_leaves_training_state_and_matches_recomputation(tmp_path, postnet):
    from semi_tts_amd.metrics import per_sum
    tr = _trainer(tmp_path, postnet=postnet)
    dev_set, tr.dev_set = tr.dev_set, []
    tr.exec()                                       # one training step, no validation
    tr.dev_set = dev_set
    assert tr.step == 1 and tr.model.training
    before = _state(tr)
    assert any(k.startswith('g/') and v is not None for k, v in before.items())
    torch.manual_seed(5)
    np.random.seed(5)
    tts, per, post = tr.validate()
    after = _state(tr)
    assert tr.model.training and all(m.training for m in tr.model.modules())
    assert sorted(before) == sorted(after)
    changed = [k for k in before if not _same(before[k], after[k])]
    assert changed == []

    # the PER: speech_to_text on the clean mel of the same dev batches again, transcribed by the plain-Python oracle
    tr.model.eval()
    torch.manual_seed(5)
    np.random.seed(5)
    per_o, post_o, tts_o = [], [], []
    with torch.no_grad():
        for mel, _, linear, text, sid in dev_set:
            mel, linear, text, sid = mel.cuda(), linear.cuda(), text.cuda(), sid.cuda()
            pp, _, _, _, _, ppp, _ = tr.model.speech_to_text(paired_mel=mel, unpaired_mel=None)
            per_o.append(O.cal_per(O.argmax_rows(pp), text.tolist()))
            assert abs(float(per_sum(pp, text)) / text.shape[0] - per_o[-1]) <= 1e-12
            if ppp is not None:
                post_o.append(O.cal_per(O.argmax_rows(ppp), text.tolist()))
            mp, lp, _, _, _, _, _, _ = tr.model.text_to_speech(text, sid, None, None, None, None, mel.shape[1], None, tf_rate=0.0)
            tts_o.append(float(tr.freq_loss(mp, mel)) + float(tr.freq_loss(lp, linear)))
    tr.model.train()
    assert abs(per - sum(per_o) / len(per_o)) <= 1e-12
    if postnet:
        assert post is not None and abs(post - sum(post_o) / len(post_o)) <= 1e-12
    else:
        assert post is None
    want = sum(tts_o) / len(tts_o)
    assert np.isfinite(tts) and abs(tts - want) <= 1e-6 * abs(want)
    from semi_tts_amd.solver import validation_checkpoints
    names, best = validation_checkpoints(1, tts, per, post, (100.0, 2.0), False)
    assert tr.dev_log[-1]['files'] == [n for n, _ in names] and (tr.best_tts_loss, tr.best_per) == best
    assert all(not n.startswith(('tts_', 'asr_')) for n, _ in names)          # step 1 never saves those


def _main(tmp_path, extra):
    cmd = [sys.executable, os.path.join(REPO, 'main.py'), '--config', CONFIG, '--valid-step', '2', '--max-step', '4', '--batch-size', '4',
           '--frames', '64', '--logdir', str(tmp_path / 'log'), '--ckpdir', str(tmp_path / 'ckpt')] + extra
    p = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0
    return p.stdout


def test_main_with_dev_set_validates_and_saves_by_the_references_rules(tmp_path):
    from semi_tts_amd.solver import validation_checkpoints, BEST_TTS_LOSS_INIT, BEST_PER_INIT
    out = _main(tmp_path, ['--dev-batches', '1'])
    rows = re.findall(r'Dv stat \| step (\d+) \| TTS loss - (\S+) \| PER - (\S+) \| post PER - (\S+)', out)
    assert [int(r[0]) for r in rows] == [1, 2, 4]
    assert all(np.isfinite(float(r[1])) and np.isfinite(float(r[2])) and r[3] == 'None' for r in rows)
    ckdir = tmp_path / 'ckpt' / 'synthetic'
    files = sorted(os.listdir(ckdir)) if ckdir.exists() else []
    # step 1 takes any finite MSE on [0, 1] data as the best TTS loss (it beats 100.0) without saving: tts_<step>.pth / asr_<step>.pth
    # exist exactly where the logged value fell below the running best, from step 2 on
    best, want = (BEST_TTS_LOSS_INIT, BEST_PER_INIT), []
    running_tts, running_per = BEST_TTS_LOSS_INIT, BEST_PER_INIT
    for step, t, p, _ in rows:
        step, t, p = int(step), float(t), float(p)
        names, best = validation_checkpoints(step, t, p, None, best, False)
        want += [n for n, _ in names]
        assert (('tts_%d.pth' % step) in files) == (step > 1 and t < running_tts)
        assert (('asr_%d.pth' % step) in files) == (step > 1 and p < running_per)
        running_tts, running_per = min(running_tts, t), min(running_per, p)
    assert best[0] < BEST_TTS_LOSS_INIT
    assert files == sorted(want)
    tr = _trainer(tmp_path / 'fresh', dev_batches=0)
    for f in files:
        ck = torch.load(str(ckdir / f), map_location='cuda')
        assert set(ck) == {'model', 'optimizer', 'global_step'}
        assert ck['global_step'] == int(re.findall(r'\d+', f)[0])
        fresh = tr._build_model()
        fresh.load_state_dict(ck['model'], strict=True)


def test_main_without_dev_set_is_unchanged(tmp_path):
    out = _main(tmp_path, [])
    assert 'Dv stat' not in out
    assert 'Tr stat | step 4' in out
    assert not (tmp_path / 'ckpt').exists() or not any(os.scandir(tmp_path / 'ckpt'))
