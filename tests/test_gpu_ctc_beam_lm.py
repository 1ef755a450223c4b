"""st_ctc_beam_search_lm on the device against the float64 oracle of tests/ctc_beam_lm_oracle.py, and --transcribe-wav-dir --lm end to end."""
import multiprocessing as mp
import os
import sys
import wave
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, 'tests')
sys.path.insert(0, TESTS)
sys.path.insert(0, REPO)
import ctc_beam_oracle as O  # noqa: E402
import ctc_beam_lm_oracle as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 1e-4
TINY = [(4, 3, 0, 2), (6, 3, 2, 3), (3, 4, 0, 3), (4, 4, 3, 2), (6, 2, 1, 1), (3, 4, 1, 4)]        # (T, V, blank, order)


def _tol(s):
    # test_gpu_ctc_beam's: fp32 accumulates ~T additions of log-probabilities into scores of magnitude |s|; the fusion adds one more
    # fp32 addition per extension, at most T of them, covered by the |s| term
    return 1e-4 + 2e-6 * np.abs(s)


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _peaked(rs, B, T, V, temp):
    """CTC-like posteriors: half the frames peak on the blank, the rest on a random symbol, at softmax temperature `temp`"""
    tgt = np.where(rs.rand(B, T) < 0.5, 0, rs.randint(1, V, (B, T)))
    return _softmax((rs.randn(B, T, V) + 6.0 * np.eye(V)[tgt]) / temp)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(prob, lengths=None, W=16, N=1, blank=0, log_input=False, bonus=None, bos=1, **kw):
    """bonus: None (the unfused entry point) or a host fp32 table, passed to the kernel as it is"""
    from semi_tts_amd.ctc_decode import beam_search
    h, hl, s = beam_search(_dev(prob), lengths, W, N, blank=blank, log_input=log_input, bos=bos,
                           bonus=None if bonus is None else _dev(bonus), **kw)
    torch.cuda.synchronize()
    return h.cpu().numpy(), hl.cpu().numpy(), s.cpu().numpy()


def _hyps(h, hl):
    return [[tuple(h[b, k, :hl[b, k]].tolist()) for k in range(h.shape[1])] for b in range(h.shape[0])]


def _init():
    sys.path.insert(0, TESTS)


def _search_one(args):
    lp, W, bonus, blank = args
    import ctc_beam_lm_oracle as Lc
    return Lc.search(lp, W, bonus, blank)


def _oracle_many(lps, W, bonus, blank=0):
    """search() of every utterance, spread over up to 16 processes (spawned: the parent has the GPU open)"""
    with ProcessPoolExecutor(min(16, len(lps)), mp_context=mp.get_context('spawn'), initializer=_init) as ex:
        return list(ex.map(_search_one, [(lp, W, bonus, blank) for lp in lps]))


def _c2_table(order, V=43):
    """-> (probability table fp32, the fused bonus table fp32): a softmax of seeded noise, fused with weight 0.8 and bonus 0.3"""
    from semi_tts_amd import ngram
    table = _softmax(np.random.RandomState(11).randn(V ** (order - 1), V) * 1.5)
    return table, ngram.fusion_table(table, 0.8, 0.3)


# ---------------------------------------------------------------- tiny problems: the kernel is exact
@pytest.mark.parametrize('T,V,blank,order', TINY)
def test_tiny_exhaustive_equals_brute_force_plus_bonus(T, V, blank, order):
    rs = np.random.RandomState(100 * T + 10 * V + order)
    W = O.n_prefixes(T, V)
    assert W <= 128
    prob = _softmax(rs.randn(3, T, V) * 2.0)
    bonus = (rs.randn(V ** (order - 1), V) * 1.5).astype(np.float32)
    h, hl, s = _run(prob, W=W, N=W, blank=blank, bonus=bonus)
    for b in range(3):
        bf = sorted(((lab, sc + L.prefix_bonus(lab, bonus)) for lab, sc in O.brute_force(O.log_probs(prob[b]), blank) if np.isfinite(sc)),
                    key=lambda x: -x[1])
        got = [(tuple(h[b, k, :hl[b, k]].tolist()), s[b, k]) for k in range(W) if np.isfinite(s[b, k])]
        assert [g[0] for g in got] == [x[0] for x in bf]
        np.testing.assert_allclose([g[1] for g in got], [x[1] for x in bf], rtol=0, atol=1e-5)
        assert len(set(_hyps(h, hl)[b])) == W             # every prefix once: exact merging


# ---------------------------------------------------------------- the C2 shapes
@pytest.fixture(scope='module')
def c2_inputs():
    rs = np.random.RandomState(7)
    return {temp: _peaked(rs, 32, 129, 43, temp) for temp in (1.0, 1.5, 0.35, 0.5)}


@pytest.mark.parametrize('W,N', [(1, 1), (16, 1), (16, 16), (128, 4)])
def test_zero_table_is_bitwise_the_unfused_search(c2_inputs, W, N):
    """adding 0.0f changes no score, so nothing the search decides: hyp, hyp_len and score bit for bit"""
    prob = c2_inputs[1.0]
    want = _run(prob, W=W, N=N)
    for order in (1, 2, 3):
        got = _run(prob, W=W, N=N, bonus=np.zeros((43 ** (order - 1), 43), np.float32))
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (order, W, N)


def c2_class(beam, sc, m, N):
    """test_gpu_ctc_beam's classification: -> ('exact' | 'other', hyps, scores).  'exact': every frame's W-th / (W+1)-th gap and every
    final neighbour gap among the first N + 1 above MARGIN -- the same hypotheses in the same order"""
    hyps, scores, margin = O.finish(beam, sc, m, N)
    return ('exact' if margin > MARGIN else 'other'), hyps, scores


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('W', [1, 4, 16])
@pytest.mark.parametrize('temp', [1.0, 1.5])
def test_config_shapes_match_the_oracle(c2_inputs, order, W, temp):
    """exact utterances: hypothesis for hypothesis, scores within _tol; the others: the top-1 score; at least 0.9 of the 32 must be
    exact (with the float64 oracle alone the shares were 0.906 .. 1.0 in the twelve cells).  The worst score error over _tol is
    printed per cell."""
    prob = c2_inputs[temp]
    _, bonus = _c2_table(order)
    full = _oracle_many(list(O.log_probs(prob)), W, bonus)
    worst = 0.0
    for N in sorted({1, W}):
        h, hl, s = _run(prob, W=W, N=N, bonus=bonus)
        got = _hyps(h, hl)
        n_exact = 0
        for b, (beam, sc, m) in enumerate(full):
            cls, hyps, scores = c2_class(beam, sc, m, N)
            if cls == 'exact':
                n_exact += 1
                assert got[b] == hyps, (b, N)
                worst = max(worst, float(np.max(np.abs(s[b] - scores) / _tol(scores))))
                assert np.all(np.abs(s[b] - scores) <= _tol(scores)), (b, N, s[b] - scores)
            assert abs(s[b, 0] - scores[0]) <= _tol(scores[0]), (b, N, s[b, 0], scores[0])
        print('order %d W %d temp %.1f N %d: exact %d / 32' % (order, W, temp, N, n_exact))
        assert n_exact >= 0.9 * len(full), (order, W, temp, N, n_exact)
    print('order %d W %d temp %.1f: worst score error on exact utterances %.3f of _tol' % (order, W, temp, worst))


@pytest.mark.parametrize('order', [2, 3])
def test_the_table_changes_every_top1(c2_inputs, order):
    """on this fixture the fused best path differs from the acoustic one for all 32 utterances (so does the oracle's): the table is applied"""
    prob = c2_inputs[1.0]
    _, bonus = _c2_table(order)
    a = _hyps(*_run(prob, W=16, N=1)[:2])
    f = _hyps(*_run(prob, W=16, N=1, bonus=bonus)[:2])
    assert sum(x[0] != y[0] for x, y in zip(a, f)) == 32


def test_lm_keyword_builds_the_same_table_once(c2_inputs, tmp_path):
    """beam_search(lm=table | tensor | path) fuses on the host and searches with exactly the table fusion_table gives"""
    from semi_tts_amd import ctc_decode, ngram
    prob = c2_inputs[1.5]
    table, bonus = _c2_table(2)
    want = _run(prob, W=8, N=2, bonus=bonus)
    path = str(tmp_path / 'lm.npy')
    ngram.save_table(path, table)
    for lm in (table, torch.from_numpy(table), path):
        got = _run(prob, W=8, N=2, lm=lm, lm_weight=0.8, ins_bonus=0.3)
        for x, y in zip(got, want):
            assert np.array_equal(x, y)
    d = torch.device(DEV)
    t1 = ctc_decode.fused_bonus(table, 0.8, 0.3, d)
    assert ctc_decode.fused_bonus(table, 0.8, 0.3, d) is t1 and ctc_decode.fused_bonus(path, 0.8, 0.3, d) is \
        ctc_decode.fused_bonus(path, 0.8, 0.3, d)
    assert ctc_decode.fused_bonus(table, 0.7, 0.3, d) is not t1
    assert np.array_equal(t1.cpu().numpy(), bonus)
    # defaults: the acoustic search
    a, b = _run(prob, W=8, N=2), _run(prob, W=8, N=2, lm=None, lm_weight=0.9, ins_bonus=1.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- edge cases
def _check(got, prob, lengths, W, N, bonus, blank=0, bos=1, need=1):
    """(h, hl, s) of the kernel against the oracle, utterance by utterance: the best score always; every hypothesis and score where the
    oracle's margin allows, which must be at least `need` utterances"""
    h, hl, s = got
    paths = _hyps(h, hl)
    lp = O.log_probs(prob)
    exact = 0
    for b in range(len(lp)):
        n = lp.shape[1] if lengths is None else int(lengths[b])
        hyps, scores, margin = L.beam_search(lp[b, :n], W, N, bonus, blank, bos)
        assert abs(s[b, 0] - scores[0]) <= _tol(scores[0]) or s[b, 0] == scores[0], (b, s[b, 0], scores[0])
        if margin > MARGIN:
            exact += 1
            assert paths[b] == hyps, b
            fin = np.isfinite(scores)
            assert np.array_equal(np.isfinite(s[b]), fin) and np.all(np.abs(s[b][fin] - scores[fin]) <= _tol(scores[fin])), b
    assert exact >= need, exact


def test_forbidden_symbol_never_appears():
    rs = np.random.RandomState(12)
    V, bad = 9, 4
    prob = _peaked(rs, 6, 40, V, 1.0)
    for order in (1, 2):
        bonus = (rs.randn(V ** (order - 1), V) * 0.5).astype(np.float32)
        bonus[:, bad] = -np.inf
        h, hl, s = _run(prob, W=8, N=8, bonus=bonus)
        free = _hyps(*_run(prob, W=8, N=1)[:2])
        assert any(bad in p[0] for p in free)                      # the acoustic search does use it
        assert np.all(np.isfinite(s[:, 0]))
        for b, paths in enumerate(_hyps(h, hl)):
            assert all(bad not in p for p, sc in zip(paths, s[b]) if np.isfinite(sc)), b
        _check((h, hl, s), prob, None, 8, 8, bonus, need=3)


def test_ragged_lengths_and_nan_beyond_them():
    rs = np.random.RandomState(13)
    T, V = 40, 9
    prob = _peaked(rs, 6, T, V, 1.0)
    bonus = (rs.randn(V * V, V) * 1.0).astype(np.float32)
    lengths = np.array([0, 1, T, 17, 5, 33], np.int32)
    dirty = prob.copy()
    for b, n in enumerate(lengths):
        dirty[b, n:] = np.nan
    for lens in (lengths.tolist(), torch.from_numpy(lengths).to(DEV)):
        h, hl, s = _run(dirty, lens, W=8, N=3, bonus=bonus)
        _check((h, hl, s), prob, lengths, 8, 3, bonus, need=5)
    assert hl[0].tolist() == [0, 0, 0] and s[0, 0] == 0.0 and np.all(s[0, 1:] == -np.inf)
    assert np.all(h[np.arange(T)[None, None, :] >= hl[:, :, None]] == 0)     # 0-padded


def test_nan_inside_the_length():
    rs = np.random.RandomState(14)
    prob = _peaked(rs, 3, 20, 6, 1.0)
    prob[1, 7, 3] = np.nan
    h, hl, s = _run(prob, [20, 8, 7], W=4, N=2, bonus=(rs.randn(6, 6)).astype(np.float32))
    assert np.all(hl[1] == 0) and np.all(np.isnan(s[1])) and np.all(h[1] == 0)
    assert np.all(np.isfinite(s[0])) and np.all(np.isfinite(s[2]))                     # frame 7 is past utterance 2's length


@pytest.mark.parametrize('blank,bos', [(3, 0), (6, 5)])
def test_nonzero_blank_and_bos(blank, bos):
    rs = np.random.RandomState(15)
    prob = _softmax(rs.randn(4, 25, 7) * 3.0)
    bonus = (rs.randn(49, 7) * 1.0).astype(np.float32)
    h, hl, s = _run(prob, W=6, N=3, blank=blank, bonus=bonus, bos=bos)
    _check((h, hl, s), prob, None, 6, 3, bonus, blank, bos, need=3)
    assert all(blank not in p for paths in _hyps(h, hl) for p in paths)


def test_bitwise_repeatable_and_independent_of_the_batch():
    rs = np.random.RandomState(16)
    prob = _peaked(rs, 12, 129, 43, 1.5)
    lengths = rs.randint(1, 130, 12).astype(np.int32)
    for order, W in ((2, 32), (3, 32), (3, 128)):                 # (order 3 at W = 128: 5504 floats, the LDS form's largest here)
        _, bonus = _c2_table(order)
        a = _run(prob, lengths.tolist(), W=W, N=4, bonus=bonus)
        b = _run(prob, lengths.tolist(), W=W, N=4, bonus=bonus)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
        parts = [_run(prob[i:i + 5], lengths[i:i + 5].tolist(), W=W, N=4, bonus=bonus) for i in (0, 5, 10)]
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), a[k])


def test_limits_accepted():
    rs = np.random.RandomState(17)
    # order 4 at V = 43 (3.4 M elements) at W = 128; V = 1024 at order 1 with W = 128
    prob = _peaked(rs, 2, 12, 43, 1.0)
    bonus = (rs.randn(43 ** 3, 43) * 1.0).astype(np.float32)
    h, hl, s = _run(prob, W=128, N=128, bonus=bonus)
    for b in range(2):
        hyps, scores, margin = L.beam_search(O.log_probs(prob[b]), 128, 128, bonus)
        assert abs(s[b, 0] - scores[0]) <= _tol(scores[0])
        if margin > MARGIN:
            assert _hyps(h, hl)[b] == hyps
            assert np.all(np.abs(s[b] - scores) <= _tol(scores))
    wide = _softmax(rs.randn(1, 3, 1024) * 4.0)
    bonus = (rs.randn(1, 1024) * 1.0).astype(np.float32)
    h, hl, s = _run(wide, W=128, N=128, bonus=bonus)
    hyps, scores, margin = L.beam_search(O.log_probs(wide[0]), 128, 128, bonus)
    assert abs(s[0, 0] - scores[0]) <= _tol(scores[0])
    if margin > MARGIN:
        assert _hyps(h, hl)[0] == hyps
    # V^order = 2^26 exactly: V = 64, order 4 is 2^24; V = 8192 is past V's own limit, so the largest table is V = 406, order 3 (2^25.99)
    prob = _softmax(rs.randn(1, 4, 406) * 3.0)
    bonus = torch.zeros(406 * 406, 406, device=DEV)
    from semi_tts_amd.ctc_decode import beam_search
    hz, hlz, sz = beam_search(_dev(prob), None, 4, 2, bonus=bonus)
    hu, hlu, su = beam_search(_dev(prob), None, 4, 2)
    assert torch.equal(hz, hu) and torch.equal(hlz, hlu) and torch.equal(sz, su)


def test_limits_refused():
    from semi_tts_amd import _lib
    lib = _lib.load()
    p = torch.rand(1, 4, 5, device=DEV)
    table = torch.zeros(5 ** 3, 5, device=DEV)
    buf = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    h = torch.empty(1, 128, 4097, device=DEV, dtype=torch.int64)
    hl = torch.empty(1, 128, device=DEV, dtype=torch.int32)
    s = torch.empty(1, 128, device=DEV, dtype=torch.float32)
    args = dict(B=1, T=4, V=5, W=4, N=1, blank=0, order=2, bos=1, bonus=table.data_ptr())
    bad = [dict(T=0), dict(T=4097), dict(V=1), dict(V=1025), dict(W=0), dict(W=129), dict(N=0), dict(N=5), dict(blank=5), dict(blank=-1),
           dict(B=0), dict(order=0), dict(order=5), dict(bos=-1), dict(bos=5), dict(bonus=None), dict(V=1024, order=3), dict(V=407, order=3),
           dict(V=91, order=4)]
    for kw in bad:
        a = dict(args, **kw)
        rc = lib.st_ctc_beam_search_lm(p.data_ptr(), a['B'], a['T'], a['V'], None, a['W'], a['N'], a['blank'], 0, 1e-10, a['bonus'],
                                       a['order'], a['bos'], h.data_ptr(), hl.data_ptr(), s.data_ptr(), buf.data_ptr(), 0)
        assert rc == -22, kw
    good = [dict(), dict(order=1), dict(order=3), dict(bos=0), dict(bos=4)]
    for kw in good:
        a = dict(args, **kw)
        rc = lib.st_ctc_beam_search_lm(p.data_ptr(), a['B'], a['T'], a['V'], None, a['W'], a['N'], a['blank'], 0, 1e-10, a['bonus'],
                                       a['order'], a['bos'], h.data_ptr(), hl.data_ptr(), s.data_ptr(), buf.data_ptr(), 0)
        assert rc == 0, kw
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the LM helps where it should
LM_V, LM_NOISE, LM_WEIGHT = 16, 2.6, 1.0


def markov_chain(rs, V=LM_V, fanout=2):
    """a sparse chain over the phone ids 3 .. V-1: every phone has `fanout` successors, never itself"""
    phones = np.arange(3, V)
    return {int(p): rs.choice(phones[phones != p], fanout, replace=False).tolist() for p in phones}


def draw_sequences(rs, chain, n, length):
    out = []
    for _ in range(n):
        seq = [int(rs.choice(sorted(chain)))]
        while len(seq) < length:
            seq.append(int(rs.choice(chain[seq[-1]])))
        out.append(seq)
    return out


def noisy_posteriors(rs, seqs, V, noise, peak=4.0):
    """two frames per phone and one blank frame after it; logits = peak on the frame's label + noise * N(0, 1)"""
    T = 3 * len(seqs[0])
    logits = noise * rs.randn(len(seqs), T, V)
    for b, seq in enumerate(seqs):
        for k, c in enumerate(seq):
            logits[b, 3 * k, c] += peak
            logits[b, 3 * k + 1, c] += peak
            logits[b, 3 * k + 2, 0] += peak
    return _softmax(logits)


def lm_problem():
    from semi_tts_amd import ngram
    rs = np.random.RandomState(18)
    chain = markov_chain(rs)
    table = ngram.ngram_table(ngram.count_ngrams(draw_sequences(rs, chain, 400, 12), LM_V, 2), smooth=0.1)
    truth = draw_sequences(rs, chain, 32, 12)
    return truth, noisy_posteriors(rs, truth, LM_V, LM_NOISE), ngram.fusion_table(table, LM_WEIGHT, 0.0)


def test_the_lm_lowers_the_edit_distance():
    """label sequences from a sparse Markov chain, noisy posteriors around them, a bigram counted from other sequences of the chain: the
    fused beam's summed edit distance is strictly below the acoustic beam's -- for the float64 oracle first (the noise level was chosen
    on the CPU so that it is), then for the kernel"""
    truth, prob, bonus = lm_problem()
    W = 8
    o_plain = [O.beam_search(lp, W, 1)[0][0] for lp in O.log_probs(prob)]
    o_fused = [L.beam_search(lp, W, 1, bonus)[0][0] for lp in O.log_probs(prob)]
    d_plain = sum(O.levenshtein(h, t) for h, t in zip(o_plain, truth))
    d_fused = sum(O.levenshtein(h, t) for h, t in zip(o_fused, truth))
    print('oracle: edit distance %d without, %d with the bigram' % (d_plain, d_fused))
    assert d_fused < d_plain
    k_plain = [p[0] for p in _hyps(*_run(prob, W=W, N=1)[:2])]
    k_fused = [p[0] for p in _hyps(*_run(prob, W=W, N=1, bonus=bonus)[:2])]
    g_plain = sum(O.levenshtein(h, t) for h, t in zip(k_plain, truth))
    g_fused = sum(O.levenshtein(h, t) for h, t in zip(k_fused, truth))
    print('kernel: edit distance %d without, %d with the bigram' % (g_plain, g_fused))
    assert g_fused < g_plain


def test_beam_per_sum_with_the_lm():
    from semi_tts_amd.metrics import beam_per_sum
    from semi_tts_amd import ngram
    rs = np.random.RandomState(19)
    prob = _peaked(rs, 4, 40, 43, 0.6)
    table, _ = _c2_table(2)
    bonus = ngram.fusion_table(table, 0.5, 0.0)                     # beam_per_sum's defaults
    text = torch.from_numpy(rs.randint(3, 42, (4, 10)).astype(np.int64))
    got = float(beam_per_sum(_dev(prob), text.to(DEV), 8, lm=table))
    hyps, _, _ = L.batch_beam_search(prob, None, 8, 1, bonus)
    ign = {0, 1, 2, 42}
    want = 0.0
    for b in range(4):
        hh = [x for x in hyps[b][0] if x not in ign]
        rr = [x for x in text[b].tolist() if x not in ign]
        want += O.levenshtein(hh, rr) / len(rr)
    assert abs(got - want) < 1e-12


# ---------------------------------------------------------------- main.py --transcribe-wav-dir --lm end to end
def _write_wav(path, x, sr):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def test_transcribe_wav_dir_with_lm_end_to_end(tmp_path):
    """the .phn scores equal a direct beam_search(..., lm=...) on the same posteriors; a table of another width is refused in load_data,
    before any file is written"""
    import yaml
    import main as entry
    from semi_tts_amd import ngram
    from semi_tts_amd.audio import load_audio_transform, SNR_OFF, WaveBatch
    from semi_tts_amd.ctc_decode import beam_search
    from semi_tts_amd.solver import Transcriber
    cfg_path = os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')
    config = yaml.load(open(cfg_path), Loader=yaml.FullLoader)
    sr = config['data']['audio']['sample_rate']
    rs = np.random.RandomState(20)
    wav_dir = tmp_path / 'wavs'
    wav_dir.mkdir()
    for i, n in enumerate([9000, 14000, 6000]):
        t = np.arange(n) / sr
        _write_wav(str(wav_dir / ('u%d.wav' % i)), 0.3 * np.sin(2 * np.pi * (200 + 50 * i) * t) + 0.05 * rs.randn(n), sr)
    table, _ = _c2_table(2)
    lm = tmp_path / 'phn.2gram.npy'
    ngram.save_table(str(lm), table)
    common = ['--config', cfg_path, '--transcribe-wav-dir', str(wav_dir), '--beam-width', '8', '--top-paths', '2',
              '--logdir', str(tmp_path / 'log'), '--batch-size', '2', '--no-msg']
    argv = common + ['--name', 'fused', '--lm', str(lm), '--lm-weight', '0.8', '--ins-bonus', '0.3']
    entry.main(argv)
    entry.main(common + ['--name', 'plain'])
    out = tmp_path / 'log' / 'fused'
    names = sorted(os.listdir(str(wav_dir)))
    assert sorted(os.listdir(str(out))) == [f[:-4] + '.phn' for f in names]
    paras = entry.parse_args(argv)
    paras.batch_size = 2
    tr = Transcriber(config, paras, 'test')
    tr.load_data()
    tr.set_model()
    conv = load_audio_transform(**config['data']['audio'])
    differ = 0
    for i in range(0, len(names), 2):
        wb = WaveBatch([conv.load(str(wav_dir / f))[0].to(DEV) for f in names[i:i + 2]])
        mel, _, _ = conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)
        with torch.no_grad():
            post = tr.model.speech_to_text(paired_mel=mel, unpaired_mel=None)[0]
        T_enc = tr.model.encoder_lengths(1 + wb.lens // conv.hop_length).clamp(0, post.shape[1])
        h, hl, s = beam_search(post, T_enc, 8, 2, lm=str(lm), lm_weight=0.8, ins_bonus=0.3)
        h, hl, s = h.cpu().numpy(), hl.cpu().numpy(), s.cpu().numpy()
        for j, k in enumerate(wb.order):
            f = names[i + k]
            lines = open(str(out / (f[:-4] + '.phn'))).read().splitlines()
            assert len(lines) == 2
            for n, ln in enumerate(lines):
                s_txt, toks = ln.split('\t')
                assert toks.split() == [str(x) for x in h[j, n, :hl[j, n]].tolist()], f
                assert abs(float(s_txt) - s[j, n]) <= _tol(s[j, n]), (f, s_txt, s[j, n])
            differ += lines != open(str(tmp_path / 'log' / 'plain' / (f[:-4] + '.phn'))).read().splitlines()
    assert differ == len(names)                                     # the table changed every file (scores at least)
    ngram.save_table(str(tmp_path / 'v64.npy'), np.full((1, 64), 1 / 64, np.float32))
    with pytest.raises(ValueError, match=r'v64\.npy.*64 classes'):
        entry.main(common + ['--name', 'refused', '--lm', str(tmp_path / 'v64.npy')])
    assert not (tmp_path / 'log' / 'refused').exists()
