"""Host-side parts of validation: the PER oracle (tests/per_oracle.py) on hand cases, the reference's checkpoint rules
(solver.validation_checkpoints, bin/train_vqvae.py:376-403), the new command-line flags and the argument checks of
ops.ctc_greedy_edit_distance that run before any launch."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import per_oracle as O   # noqa: E402
from semi_tts_amd.solver import validation_checkpoints, BEST_TTS_LOSS_INIT, BEST_PER_INIT   # noqa: E402

A, B_, C_ = 10, 11, 12


def test_oracle_classic_distances():
    kitten, sitting = [ord(c) for c in 'kitten'], [ord(c) for c in 'sitting']
    assert O.levenshtein(kitten, sitting) == 3
    assert O.levenshtein([ord(c) for c in 'flaw'], [ord(c) for c in 'lawn']) == 2
    assert O.levenshtein([], []) == 0
    assert O.levenshtein([A, B_, C_], [A, B_, C_]) == 0


def test_oracle_empty_hyp_and_insertions():
    # every frame blank: the hypothesis is empty, every reference token is a deletion
    d, n, hyp = O.utterance([0, 0, 0, 0], [A, B_, C_, 0])
    assert (d, n, hyp) == (3, 3, [])
    # more hypothesis tokens than reference tokens: a rate above 1
    p = [A, B_, C_, A, B_, C_]
    d, n, _ = O.utterance(p, [A, 0, 0])
    assert (d, n) == (5, 1) and d / n > 1
    assert O.cal_per([p], [[A, 0, 0]]) == 5.0


def test_oracle_collapses_before_filtering():
    # a, blank, a: two tokens (the blank separates the runs before it is dropped) -> one insertion against ref "a"
    d, n, hyp = O.utterance([A, 0, A], [A])
    assert hyp == [A, A] and (d, n) == (1, 1)
    d, n, hyp = O.utterance([A, A, 42, A, 1, 1, B_], [A, B_])
    assert hyp == [A, A, B_] and d == 1


def test_oracle_drops_ignored_ids_anywhere_in_the_transcript():
    d, n, hyp = O.utterance([A, B_, C_], [0, A, 1, B_, 42, 2, C_, 0])
    assert (d, n, hyp) == (0, 3, [A, B_, C_])
    assert O.strip([42, 1, 2, 0]) == []
    with pytest.raises(ZeroDivisionError):               # the reference's behaviour on an all-ignored transcript
        O.cal_per([[A]], [[0, 42]])


def _run(seq, store_best_per=False):
    """feed (step, tts, per, post) through the rules like successive validate() calls; -> file names per call, final best"""
    best, out = (BEST_TTS_LOSS_INIT, BEST_PER_INIT), []
    for step, tts, per, post in seq:
        files, best = validation_checkpoints(step, tts, per, post, best, store_best_per)
        out.append([f for f, _ in files])
    return out, best


def test_checkpoint_rules_basic_sequence():
    assert (BEST_TTS_LOSS_INIT, BEST_PER_INIT) == (100.0, 2.0)
    files, best = _run([(1, 5.0, 0.9, None),          # step 1 never saves tts_ / asr_ (but sets the bests)
                        (2, 4.0, 0.95, None),         # TTS improves
                        (4, 4.5, 0.8, None),          # PER improves
                        (6, 4.5, 0.8, None),          # neither (equal is not better)
                        (10000, 3.0, 0.85, None),     # TTS improves + the regular checkpoint
                        (20000, 3.5, 0.9, None)])     # the regular checkpoint alone
    assert files == [[], ['tts_2.pth'], ['asr_4.pth'], [], ['tts_10000.pth', 'step_10000.pth'], ['step_20000.pth']]
    assert best == (3.0, 0.8)


def test_checkpoint_rules_initial_values():
    files, best = _run([(2, 100.0, 2.0, None), (3, 150.0, 2.5, None), (4, float('nan'), float('nan'), float('nan'))])
    assert files == [[], [], []] and best == (100.0, 2.0)
    files, best = _run([(2, 99.9, 1.999, None)])
    assert files == [['tts_2.pth', 'asr_2.pth']] and best == (99.9, 1.999)


def test_checkpoint_rules_post_per_quirk():
    files, best = _run([(1, 5.0, 0.7, 0.6),     # post beats the JUST UPDATED best_per: saved even at step 1
                        (2, 5.0, 0.65, 0.62),   # neither beats 0.6
                        (3, 5.0, 0.5, 0.55),    # PER 0.5 becomes best_per first: the post PER 0.55 (better than 0.6) is not saved
                        (5, 5.0, 0.52, 0.45)])  # post beats best_per 0.5
    assert files == [['best_post_per.pth'], [], ['asr_3.pth'], ['best_post_per.pth']]
    assert best == (5.0, 0.45)
    files, scores = validation_checkpoints(7, 1.0, 0.4, 0.3, (5.0, 0.45), False)
    assert files == [('tts_7.pth', 1.0), ('asr_7.pth', 0.4), ('best_post_per.pth', 0.3)] and scores == (1.0, 0.3)


def test_checkpoint_rules_store_best_per():
    files, best = _run([(1, 5.0, 0.9, 0.95),           # step 1 saves here; post does not beat 0.9
                        (2, 4.0, 0.95, 0.85),          # post beats best_per; TTS improvements never save
                        (10000, 3.0, 0.8, 0.9)],       # no step_10000.pth under --store-best-per
                       store_best_per=True)
    assert files == [['best_per.pth'], ['best_post_per.pth'], ['best_per.pth']]
    assert best == (100.0, 0.8)                        # best_tts_loss is not touched


def test_parse_args_accepts_validation_flags(capsys):
    import main
    p = main.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml', '--dev-batches', '3', '--valid-step', '2',
                         '--store-best-per'])
    assert (p.dev_batches, p.valid_step, p.store_best_per) == (3, 2, True)
    assert 'store-best-per accepted for compatibility' not in capsys.readouterr().out
    p = main.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml'])
    assert (p.dev_batches, p.valid_step) == (0, None)
    main.parse_args(['--config', 'config/semi-single-spkr-paired-data.yaml', '--store-best-per'])
    assert 'store-best-per accepted for compatibility' in capsys.readouterr().out       # no dev set: still without effect
    for bad in (['--dev-batches', '-1'], ['--valid-step', '0'], ['--dev-batches', '1', '--tts-only'],
                ['--dev-batches', '1', '--gen-specgram']):
        with pytest.raises(SystemExit):
            main.parse_args(['--config', 'config/supervised.yaml'] + bad)


def test_metrics_ignore_indices_are_the_references():
    from semi_tts_amd.metrics import IGNORE_INDICES, cal_per
    assert IGNORE_INDICES == (0, 1, 2, 42) == O.IGNORE
    assert math.isnan(cal_per(None, torch.zeros(2, 3, dtype=torch.int64)))


@pytest.mark.parametrize('prob, text', [
    (torch.zeros(2, 5, 43), torch.zeros(2, 4, dtype=torch.int64)),          # host tensors: no CPU fallback
    (torch.zeros(2, 5, 43, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int64)),
])
def test_edit_distance_refuses_before_any_launch(prob, text):
    from semi_tts_amd import ops
    with pytest.raises(ValueError):
        ops.ctc_greedy_edit_distance(prob, text, O.IGNORE)
