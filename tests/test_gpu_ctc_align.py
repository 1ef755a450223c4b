"""st_ctc_forced_align on the device against the numpy oracle of tests/ctc_align_oracle.py (bit for bit on log input, within the
fp32 tolerance on probabilities), and the --align-wav-dir path end to end."""
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, 'tests')
sys.path.insert(0, TESTS)
sys.path.insert(0, REPO)
import ctc_align_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TEMPS = (0.3, 1.0, 1.5, 3.0)


def _tol(s, T):
    # fp32 accumulates T additions of log-probabilities into a score of magnitude |s|: 1e-4 absolute per 129 frames (the tolerance
    # test_gpu_ctc_beam derives for 129 additions) plus a few ulps of |s|
    return math.ceil(T / 129) * 1e-4 + 2e-6 * np.abs(s)


def _dev(x, dtype):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(DEV)


def _run(prob, text, lengths=None, text_lengths=None, blank=0, log_input=False):
    """lengths / text_lengths: None, a host list (checked by ops), or a device tensor (taken as it is)"""
    from semi_tts_amd.ctc_align import forced_align
    out = forced_align(_dev(prob, np.float32), _dev(text, np.int64), lengths, text_lengths, blank=blank, log_input=log_input)
    torch.cuda.synchronize()
    score, path, ts, te = (x.cpu().numpy() for x in out)
    assert score.dtype == np.float32 and path.dtype == ts.dtype == te.dtype == np.int32
    return score, path, ts, te


def _lp32(prob):
    """log(p + 1e-10) computed in float64 and cast to fp32: what the bit-exact tests give the device as log input"""
    return np.log(np.asarray(prob, np.float64) + 1e-10).astype(np.float32)


def _host(x):
    return None if x is None else np.asarray(x.cpu() if torch.is_tensor(x) else x)


def _assert_exact(got, lp32, text, lengths=None, text_lengths=None, blank=0, clean=None):
    """the device's outputs on log input equal the float32 oracle bit for bit: every utterance, every output"""
    want = O.batch_align(None, text, _host(lengths), _host(text_lengths), blank, dtype=np.float32, lp=lp32 if clean is None else clean)
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    fin = ~np.isnan(want[0])
    assert np.array_equal(got[0][fin].view(np.uint32), want[0][fin].astype(np.float32).view(np.uint32)), (got[0], want[0])
    for g, w, name in zip(got[1:], want[1:], ('path', 'tok_start', 'tok_end')):
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, (name, bad.tolist())
    return want


def _assert_close(got, prob, text, text_lengths, blank=0):
    """on probabilities: an alignment of the targets, its score the float64 optimum within the tolerance, and the path found optimal up to
    rounding; and never above the float64 forward log-likelihood"""
    B, T, _ = prob.shape
    lp = O.log_probs(prob)
    worst = 0.0
    for b in range(B):
        tg = O.targets_of(text[b], text_lengths[b], blank)
        want = float(O.align(lp[b], tg, blank)[0])
        tol = _tol(want, T)
        assert O.is_alignment(got[1][b], tg, blank), b
        err, deficit = abs(float(got[0][b]) - want), want - O.path_score(lp[b], got[1][b])
        print('utterance %d: score %.6f oracle %.6f err %.3g deficit %.3g tol %.3g' % (b, got[0][b], want, err, deficit, tol))
        assert err <= tol, (b, got[0][b], want)
        assert deficit <= tol, (b, deficit)
        assert float(got[0][b]) <= O.forward_loglik(lp[b], tg, blank) + tol, b
        for k in range(len(tg)):
            fr = np.nonzero((got[1][b] == tg[k]) & (np.arange(T) >= got[2][b, k]) & (np.arange(T) < got[3][b, k]))[0]
            assert fr.size == got[3][b, k] - got[2][b, k] > 0, (b, k)             # the span is frames of that label
        assert np.all(got[2][b, len(tg):] == -1) and np.all(got[3][b, len(tg):] == -1)
        worst = max(worst, err / tol)
    return worst


# ---------------------------------------------------------------- 1. tiny problems: the brute force
@pytest.mark.parametrize('T,V,blank,seed', [(1, 3, 0, 0), (3, 3, 0, 1), (5, 3, 2, 2), (6, 3, 0, 3), (6, 3, 1, 4), (4, 4, 3, 5)])
def test_tiny_problems_equal_brute_force(T, V, blank, seed):
    rs = np.random.RandomState(seed)
    syms = [v for v in range(V) if v != blank]
    targets = [[]] + [[a] for a in syms] + [[a, b] for a in syms for b in syms] + [[a, b, a] for a in syms for b in syms]
    B = len(targets)
    prob = O.softmax(rs.randn(B, T, V) * 2.0)
    text = np.full((B, 3), blank, np.int64)
    for b, tg in enumerate(targets):
        text[b, :len(tg)] = tg
    score, path, ts, te = _run(prob, text, blank=blank)
    for b, tg in enumerate(targets):
        bf = O.brute_force(O.log_probs(prob[b]), tg, blank)
        if not bf:
            assert score[b] == -np.inf and np.all(path[b] == -1) and np.all(ts[b] == -1) and np.all(te[b] == -1), b
            continue
        assert abs(score[b] - bf[0][1]) <= 1e-5, (b, score[b], bf[0][1])
        if len(bf) == 1 or bf[0][1] - bf[1][1] > 1e-4:
            assert tuple(path[b].tolist()) == bf[0][0], (b, tg)
        assert O.is_alignment(path[b], tg, blank)


# ---------------------------------------------------------------- 2. - 4. the configuration shapes
@pytest.fixture(scope='module')
def c2_inputs():
    rs = np.random.RandomState(0)
    return {temp: O.peaked(rs, 32, 129, 43, temp, 43) for temp in TEMPS}


@pytest.fixture(scope='module')
def long_inputs():
    rs = np.random.RandomState(0)
    return {temp: O.peaked(rs, 64, 533, 43, temp, 171) for temp in TEMPS}


@pytest.mark.parametrize('temp', TEMPS)
def test_config_shape_log_input_is_bit_exact(c2_inputs, temp):
    prob, text, tl = c2_inputs[temp]
    lp = _lp32(prob)
    got = _run(lp, text, None, tl.tolist(), log_input=True)
    want = _assert_exact(got, lp, text, None, tl)
    assert np.all(np.isfinite(want[0])) and np.all(want[2][:, 0] >= 0)


@pytest.mark.parametrize('temp', TEMPS)
def test_config_shape_probabilities(c2_inputs, temp):
    prob, text, tl = c2_inputs[temp]
    got = _run(prob, text, None, tl.tolist())
    worst = _assert_close(got, prob, text, tl)
    print('temperature %.1f: worst score error %.3f of the tolerance' % (temp, worst))


@pytest.mark.parametrize('temp', TEMPS)
def test_long_form_log_input_is_bit_exact(long_inputs, temp):
    prob, text, tl = long_inputs[temp]
    lp = _lp32(prob)
    got = _run(lp, text, None, tl.tolist(), log_input=True)
    _assert_exact(got, lp, text, None, tl)


@pytest.mark.parametrize('temp', TEMPS)
def test_long_form_probabilities(long_inputs, temp):
    prob, text, tl = long_inputs[temp]
    got = _run(prob, text, None, tl.tolist())
    worst = _assert_close(got, prob, text, tl)
    print('temperature %.1f: worst score error %.3f of the tolerance' % (temp, worst))


# Both shapes above keep their back-pointers in LDS with one or two states per thread.  The other forms of the kernel -- back-pointers in
# the workspace, and 4 or 9 states per thread (chosen from L) -- on log input, exactly: (T, L, target counts, expects a workspace)
FORMS = [(4096, 1024, (1024, 700), True),          # the limits: 9 states per thread, workspace
         (4096, 100, (100, 3), True),              # 1 state per thread, workspace
         (2048, 200, (200, 120), True),            # 2 states per thread, workspace
         (1500, 400, (400, 257), True),            # 4 states per thread, workspace
         (200, 300, (190, 131), False),            # 4 states per thread, LDS
         (160, 600, (140, 120), False)]            # 9 states per thread (L = 600), LDS


@pytest.mark.parametrize('T,L,counts,needs_ws', FORMS)
def test_every_kernel_form_is_bit_exact_on_log_input(T, L, counts, needs_ws):
    from semi_tts_amd import _lib
    assert (int(_lib.load().st_ctc_align_workspace_bytes(2, T, L)) > 0) == needs_ws
    rs = np.random.RandomState(T + L)
    prob, text, tl = O.peaked(rs, 2, T, 43, 1.0, L, counts=counts)
    assert tl.tolist() == list(counts)
    lp = _lp32(prob)
    got = _run(lp, text, None, tl.tolist(), log_input=True)
    want = _assert_exact(got, lp, text, None, tl)
    assert np.all(np.isfinite(want[0]))
    # ragged lengths in the same form: the second utterance stops inside a 16-frame back-pointer word
    lens = [T, T - 7]
    _assert_exact(_run(lp, text, lens, tl.tolist(), log_input=True), lp, text, lens, tl)


# ---------------------------------------------------------------- 5. edges
def test_ragged_lengths_and_garbage_beyond_them():
    rs = np.random.RandomState(1)
    T, V, L = 40, 9, 12
    prob, text, tl = O.peaked(rs, 6, T, V, 1.0, L)
    lengths = np.array([T, 13, 31, 17, 25, 33], np.int32)
    tl = np.minimum(tl, [12, 5, 9, 6, 1, 12]).astype(np.int32)
    lp = _lp32(prob)
    dirty, dtext = lp.copy(), text.copy()
    for b in range(6):
        dirty[b, lengths[b]:] = np.nan if b % 2 else 1e30
        dtext[b, tl[b]:] = 10 ** 6 if b % 2 else -5                        # ids that would make the score NaN if they were read
    for lens, tls in ((lengths.tolist(), tl.tolist()), (torch.from_numpy(lengths).to(DEV), torch.from_numpy(tl).to(DEV)),
                      (torch.from_numpy(lengths.astype(np.int64)).to(DEV), tl.tolist())):
        got = _run(dirty, dtext, lens, tls, log_input=True)
        want = _assert_exact(got, None, text, lengths, tl, clean=lp)
        assert np.all(np.isfinite(want[0]))
    # the same through probabilities (1e30 and NaN past the lengths again)
    dprob = prob.copy()
    for b in range(6):
        dprob[b, lengths[b]:] = np.nan if b % 2 else 1e30
    got = _run(dprob, dtext, lengths.tolist(), tl.tolist())
    for b in range(6):
        tg = O.targets_of(text[b], tl[b])
        sc, _, lab, s0, s1 = O.align(O.log_probs(prob[b, :lengths[b]]), tg)
        assert abs(got[0][b] - sc) <= _tol(sc, T) and np.all(got[1][b, lengths[b]:] == -1)
        assert got[1][b, :lengths[b]].tolist() == lab.tolist() and got[2][b, :len(tg)].tolist() == s0.tolist()
    # device lengths out of range are clamped, not refused
    got = _run(lp, text, torch.tensor([T + 9] * 6, device=DEV), torch.tensor([L + 3] * 6, device=DEV), log_input=True)
    _assert_exact(got, lp, text, None, None)


def test_repeated_tokens_and_the_feasibility_edge():
    rs = np.random.RandomState(2)
    V = 6
    text = np.array([[2, 2, 2, 4, 4, 1], [2, 2, 2, 4, 4, 1], [3, 3, 0, 0, 0, 0], [3, 3, 0, 0, 0, 0], [5, 1, 5, 1, 5, 1]], np.int64)
    need = [9, 9, 3, 3, 6]                                                  # S + adjacent equal targets
    T = 12
    lp = _lp32(O.softmax(rs.randn(5, T, V) * 2.0))
    got = _run(lp, text, [T] * 5, None, log_input=True)
    _assert_exact(got, lp, text, [T] * 5)
    for b in (0, 2):                                                        # a blank separates equal neighbours
        tg = O.targets_of(text[b])
        for k in range(1, len(tg)):
            if tg[k] == tg[k - 1]:
                assert got[3][b, k - 1] < got[2][b, k] and np.all(got[1][b, got[3][b, k - 1]:got[2][b, k]] == 0)
    # length == S + repeats: the one feasible path; one frame fewer: -inf and -1 everywhere
    got = _run(lp, text, need, None, log_input=True)
    want = _assert_exact(got, lp, text, need)
    assert np.all(np.isfinite(want[0]))
    assert got[1][0, :9].tolist() == [2, 0, 2, 0, 2, 4, 0, 4, 1] and got[1][2, :3].tolist() == [3, 0, 3]
    fewer = [n - 1 for n in need]
    got = _run(lp, text, fewer, None, log_input=True)
    _assert_exact(got, lp, text, fewer)
    assert np.all(got[0] == -np.inf) and np.all(got[1] == -1) and np.all(got[2] == -1) and np.all(got[3] == -1)


def test_empty_transcripts_and_empty_utterances():
    rs = np.random.RandomState(3)
    T, V = 10, 5
    lp = _lp32(O.softmax(rs.randn(4, T, V)))
    text = np.array([[0, 0, 0], [1, 2, 0], [0, 0, 0], [3, 0, 0]], np.int64)
    lens = [T, T, 0, 0]
    got = _run(lp, text, lens, None, log_input=True)
    _assert_exact(got, lp, text, lens)
    assert abs(got[0][0] - lp[0, :, 0].astype(np.float64).sum()) < 1e-4 and np.all(got[1][0] == 0)        # S = 0: all blank
    assert got[0][2] == 0.0 and got[0][3] == -np.inf and np.all(got[1][2:] == -1)                        # length 0
    assert np.all(got[2][[0, 2, 3]] == -1) and np.all(got[3][[0, 2, 3]] == -1)
    # text_lengths = 0 empties a transcript that has entries
    got = _run(lp, text, lens, [0, 0, 0, 0], log_input=True)
    _assert_exact(got, lp, text, lens, [0, 0, 0, 0])
    assert got[0][3] == 0.0 and np.all(got[1][1] == 0)


def test_nan_and_targets_out_of_range():
    rs = np.random.RandomState(4)
    T, V = 16, 7
    lp = _lp32(O.softmax(rs.randn(5, T, V)))
    text = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 7, 3], [1, -1, 3]], np.int64)
    lp[0, 5, 2] = np.nan                                                    # a column of ext, inside the length -> NaN
    lp[1, 5, 4] = np.nan                                                    # a column outside ext -> no effect
    lp[2, 12, 2] = np.nan                                                   # past the length (10) -> no effect
    lens = [T, T, 10, T, T]
    got = _run(lp, text, lens, None, log_input=True)
    _assert_exact(got, lp, text, lens)
    assert np.isnan(got[0][[0, 3, 4]]).all() and np.isfinite(got[0][[1, 2]]).all()
    for b in (0, 3, 4):
        assert np.all(got[1][b] == -1) and np.all(got[2][b] == -1) and np.all(got[3][b] == -1)
    # a NaN probability likewise
    prob = O.softmax(rs.randn(2, T, V))
    prob[0, 3, 0] = np.nan
    got = _run(prob, text[:2])
    assert np.isnan(got[0][0]) and np.all(got[1][0] == -1) and np.isfinite(got[0][1])


@pytest.mark.parametrize('blank', [3, 6])
def test_nonzero_blank_and_blank_entries_inside_text(blank):
    rs = np.random.RandomState(5)
    T, V = 30, 7
    prob, text, tl = O.peaked(rs, 4, T, V, 1.0, 8, blank=blank)
    text = np.concatenate([text[:, :3], np.full((4, 2), blank, np.int64), text[:, 3:]], axis=1)      # blanks inside: dropped
    lp = _lp32(prob)
    got = _run(lp, text, None, None, blank=blank, log_input=True)
    _assert_exact(got, lp, text, blank=blank)
    for b in range(4):
        tg = [x for x in text[b].tolist() if x != blank]
        assert O.is_alignment(got[1][b], tg, blank) and np.all(got[2][b, len(tg):] == -1)
    if blank != 0:
        text0 = text.copy()
        text0[0, 0] = 0                                                     # id 0 is an ordinary target when the blank is elsewhere
        got = _run(lp, text0, None, None, blank=blank, log_input=True)
        _assert_exact(got, lp, text0, blank=blank)
        assert got[1][0, got[2][0, 0]] == 0


# ---------------------------------------------------------------- 6. limits
def test_limits_accepted():
    rs = np.random.RandomState(6)
    prob = O.softmax(rs.randn(1, 6, 10240) * 4.0)
    text = np.array([[10239, 5000, 10239]], np.int64)
    lp = _lp32(prob)
    _assert_exact(_run(lp, text, log_input=True), lp, text)
    got = _run(prob, text)
    assert O.is_alignment(got[1][0], text[0]) and abs(got[0][0] - O.align(O.log_probs(prob[0]), text[0])[0]) <= _tol(got[0][0], 6)
    # T = 4096 and L = 1024 together are FORMS[0]


def test_limits_refused():
    from semi_tts_amd import _lib
    lib = _lib.load()
    p = torch.rand(1, 4, 5, device=DEV)
    text = torch.ones(1, 3, dtype=torch.int64, device=DEV)
    score = torch.empty(1, device=DEV)
    path = torch.empty(1, 4, dtype=torch.int32, device=DEV)
    ts = torch.empty(1, 3, dtype=torch.int32, device=DEV)
    te = torch.empty(1, 3, dtype=torch.int32, device=DEV)
    buf = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    args = dict(B=1, T=4, V=5, L=3, blank=0)
    bad = [dict(T=0), dict(T=4097), dict(V=1), dict(V=10241), dict(L=0), dict(L=1025), dict(blank=5), dict(blank=-1), dict(B=0)]
    for kw in bad:
        a = dict(args, **kw)
        rc = lib.st_ctc_forced_align(p.data_ptr(), a['B'], a['T'], a['V'], None, text.data_ptr(), a['L'], None, a['blank'], 0, 1e-10,
                                     score.data_ptr(), path.data_ptr(), ts.data_ptr(), te.data_ptr(), buf.data_ptr(), 0)
        assert rc == -22, kw
    # a shape whose back-pointers need the workspace is refused without one
    assert lib.st_ctc_align_workspace_bytes(1, 4096, 1024) > 0 and lib.st_ctc_align_workspace_bytes(32, 129, 43) == 0
    rc = lib.st_ctc_forced_align(p.data_ptr(), 1, 4096, 5, None, text.data_ptr(), 1024, None, 0, 0, 1e-10, score.data_ptr(),
                                 path.data_ptr(), ts.data_ptr(), te.data_ptr(), None, 0)
    assert rc == -22
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. agreement with the existing kernels
def test_peaked_posteriors_align_to_the_argmax():
    from semi_tts_amd import ops
    rs = np.random.RandomState(7)
    B, T, V = 8, 64, 43
    prob, _, _ = O.peaked(rs, B, T, V, 0.2, 20)
    pd = torch.from_numpy(prob).to(DEV)
    _, _, gh, ghl = ops.ctc_greedy_edit_distance(pd, torch.ones(B, 4, dtype=torch.int64, device=DEV), (0,), want_hyp=True)
    assert int(ghl.max()) >= 1
    score, path, ts, te = _run(prob, gh, None, ghl)                        # the greedy transcript, aligned back
    lp = O.log_probs(prob)
    for b in range(B):
        assert path[b].tolist() == prob[b].argmax(-1).tolist(), b
        want = lp[b].max(-1).sum()
        assert abs(score[b] - want) <= _tol(want, T), (b, score[b], want)


# ---------------------------------------------------------------- 8. determinism
def test_bitwise_repeatable_and_independent_of_the_batch():
    rs = np.random.RandomState(8)
    prob, text, tl = O.peaked(rs, 12, 129, 43, 1.5, 43)
    lengths = np.maximum(rs.randint(1, 130, 12), 2 * tl + 2).clip(0, 129).astype(np.int32)
    lengths[3] = 5                                                          # (an infeasible one among them, unless its transcript is tiny)
    a = _run(prob, text, lengths.tolist(), tl.tolist())
    b = _run(prob, text, lengths.tolist(), tl.tolist())
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    parts = [_run(prob[i:i + 5], text[i:i + 5], lengths[i:i + 5].tolist(), tl[i:i + 5].tolist()) for i in (0, 5, 10)]
    for k in range(4):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), a[k], equal_nan=True)


# ---------------------------------------------------------------- 9. main.py --align-wav-dir end to end
def _write_wav(path, x, sr):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def _posteriors(al, conv, wav_dir, names, source):
    """{file: (posteriors of its own encoder frames, T_enc)} from the aligner's own model on the same mels, in batches of 2"""
    from semi_tts_amd.audio import WaveBatch, SNR_OFF
    out = {}
    for i in range(0, len(names), 2):
        wb = WaveBatch([conv.load(os.path.join(wav_dir, f))[0].to(DEV) for f in names[i:i + 2]])
        mel, _, _ = conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)
        with torch.no_grad():
            outs = al.model.speech_to_text(paired_mel=mel, unpaired_mel=None)
        post = (outs[5] if source == 'post' else outs[0]).cpu().numpy()
        T_enc = al.model.encoder_lengths(1 + wb.lens // conv.hop_length).tolist()
        for j, k in enumerate(wb.order):
            out[names[i + k]] = (post[j, :T_enc[j]], T_enc[j])
    return out


def _check_outputs(out_dir, posts, transcripts, voc, frame_s, source):
    """every .ali line and every segments.csv row against the float64 oracle on `posts`; -> the number of rows in segments.csv"""
    rows = open(os.path.join(out_dir, 'segments.csv')).read().splitlines()
    assert rows[0] == 'file,seg'
    table = dict(r.split(',') for r in rows[1:])
    assert len(table) == len(rows) - 1
    for f, (post, T) in posts.items():
        tg = [x for x in transcripts[f] if x != 0]
        sc, _, _, s0, s1 = O.align(O.log_probs(post, log_input=source == 'post'), tg)
        lines = open(os.path.join(out_dir, f[:-4] + '.ali')).read().splitlines()
        head = dict(kv.split('=') for kv in lines[0][2:].split())
        assert lines[0].startswith('# score=') and int(head['frames']) == T and head['frame_s'] == '%.6f' % frame_s, f
        key = f.split('.')[0]
        if not np.isfinite(sc):
            assert head['score'] == '-inf' and len(lines) == 1 and key not in table, f
            continue
        assert abs(float(head['score']) - sc) <= _tol(sc, T) + 1e-6, (f, head['score'], sc)
        want = ['%s\t%d\t%d\t%.6f\t%.6f' % (voc[x] if x < len(voc) else str(x), a, b, a * frame_s, b * frame_s)
                for x, a, b in zip(tg, s0.tolist(), s1.tolist())]
        assert lines[1:] == want, f
        if tg:
            assert table[key] == '_'.join('%.4f' % (a * frame_s) for a in s0.tolist()[1:] + [T]), f
        else:
            assert key not in table, f
    return len(table)


@pytest.mark.parametrize('source', ['code', 'post'])
def test_align_wav_dir_end_to_end(tmp_path, source):
    """'post' aligns to the ASR postnet's log-posteriors: the shipped configs have no postnet, so a copy of one with
    model.asr_postnet_weight > 0 is written next to the .wav files"""
    import yaml
    import main as entry
    from semi_tts_amd.audio import load_audio_transform
    from semi_tts_amd.solver import Aligner, read_vocab
    from semi_tts_amd.ctc_align import read_phn
    cfg_path = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')
    config = yaml.load(open(cfg_path), Loader=yaml.FullLoader)
    if source == 'post':
        config['model']['asr_postnet_weight'] = 0.5
        cfg_path = str(tmp_path / 'with_postnet.yaml')
        with open(cfg_path, 'w') as f:
            yaml.safe_dump(config, f)
    sr = config['data']['audio']['sample_rate']
    rs = np.random.RandomState(11)
    wav_dir = tmp_path / 'wavs'
    wav_dir.mkdir()
    lens = [9000, 14000, 6000, 11000, 7000]
    for i, n in enumerate(lens):
        t = np.arange(n) / sr
        _write_wav(str(wav_dir / ('u%d.wav' % (4 - i))), 0.3 * np.sin(2 * np.pi * (200 + 50 * i) * t) + 0.05 * rs.randn(n), sr)
    names = sorted(os.listdir(str(wav_dir)))
    vocab = tmp_path / 'phn.vocab'
    vocab.write_text('\n'.join('P%d' % i for i in range(40)) + '\n')
    voc = read_vocab(str(vocab))
    common = ['--config', cfg_path, '--vocab', str(vocab), '--logdir', str(tmp_path / 'log'), '--batch-size', '2', '--no-msg',
              '--asr-output', source]
    # ---- first run: the transcripts --transcribe-wav-dir writes, taken as they are
    entry.main(common + ['--transcribe-wav-dir', str(wav_dir), '--name', 'tr', '--top-paths', '2'])
    argv = common + ['--align-wav-dir', str(wav_dir), '--phn-dir', str(tmp_path / 'log' / 'tr'), '--name', 'al']
    entry.main(argv)
    out = str(tmp_path / 'log' / 'al')
    assert sorted(os.listdir(out)) == ['segments.csv'] + ['u%d.ali' % i for i in range(5)]
    paras = entry.parse_args(argv)
    paras.batch_size = 2
    al = Aligner(config, paras, 'test')
    al.load_data()
    al.set_model()
    conv = load_audio_transform(**config['data']['audio'])
    frame_s = al.model.time_reduce_factor * conv.hop_length / sr
    posts = _posteriors(al, conv, str(wav_dir), names, source)
    transcripts = {f: read_phn(str(tmp_path / 'log' / 'tr' / (f[:-4] + '.phn')), voc) for f in names}
    assert [transcripts[f] for f in names] == al.transcripts
    _check_outputs(out, posts, transcripts, voc, frame_s, source)
    # ---- second run: hand-written id transcripts, one of them longer than its utterance has encoder frames
    V = next(iter(posts.values()))[0].shape[1]
    phn = tmp_path / 'phn'
    phn.mkdir()
    transcripts = {}
    for i, f in enumerate(names):
        ids = rs.randint(1, V, 200 if i == 2 else 5).tolist()
        transcripts[f] = ids
        (phn / (f[:-4] + '.phn')).write_text(' '.join(voc[x] if x < len(voc) and i % 2 else str(x) for x in ids) + '\n')
    assert posts[names[2]][1] < 200 and all(T >= 10 for _, T in posts.values())
    entry.main(common + ['--align-wav-dir', str(wav_dir), '--phn-dir', str(phn), '--name', 'al2'])
    out2 = str(tmp_path / 'log' / 'al2')
    assert _check_outputs(out2, posts, transcripts, voc, frame_s, source) == 4
    assert open(os.path.join(out2, names[2][:-4] + '.ali')).read() == '# score=-inf frames=%d frame_s=%.6f\n' % (posts[names[2]][1], frame_s)
    # ---- third run: one transcript missing -> an error naming it, before anything is written
    os.remove(str(phn / 'u3.phn'))
    with pytest.raises(ValueError, match=r'u3\.phn'):
        entry.main(common + ['--align-wav-dir', str(wav_dir), '--phn-dir', str(phn), '--name', 'al3'])
    assert not os.path.exists(str(tmp_path / 'log' / 'al3'))
