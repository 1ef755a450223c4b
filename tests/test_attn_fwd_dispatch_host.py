"""Which launch a forward attention call takes, and whether the float64 reference and the bounds of attn_fwd_cases.py can be trusted --
host arithmetic only, no GPU: st_attn_fwd_variant looks at shapes and alignment flags and reads no memory.  Every row of the case
table reaches the launch or refusal named in it, together the rows reach every value of every field of the plan and every refusal, the
LDS limits are pinned, a Python restatement of the LDS layout agrees with the library, the reference agrees with the oracle in float64,
the bounds are within the project's present thresholds, and each of a list of plausible defects moves the reference by more than 8
bounds on every Gaussian row -- so the GPU test (test_gpu_attn_fwd.py), which holds the kernels to these bounds, can fail."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fwd_cases as T   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def query(lib, part, c, parts, al=None, **over):
    d = dict(c, **over)
    q = _lib.StAttnFwdQuery(part, d['B'], d['L'], d['A'], d['E'], d['F'], d['K'], parts, T.align_bits(c) if al is None else al)
    out = _lib.StAttnFwdPlan()
    rc = lib.st_attn_fwd_variant(C.byref(q), C.byref(out))
    plan = {n: getattr(out, n) for n, _ in out._fields_}
    plan['part'] = part
    return rc, plan


def row_plans(lib, c):
    """[(want, rc, plan)] of the launches of a row"""
    if c['part'] in ('whole',):
        return [(c['want'], *query(lib, 0, c, 1))]
    if c['part'] == 'cf':
        return [(c['want'], *query(lib, 1, c, c['pre']))]
    if c['part'] == 'prefin':
        return [(c['want'], *query(lib, 1, c, c['pre'])), (c['want_fin'], *query(lib, 2, c, c['fin']))]
    return [(c['want'], *query(lib, 3, c, c['fin']))]


@pytest.mark.parametrize('c', T.ROWS, ids=[c['id'] for c in T.ROWS])
def test_row_reaches_its_variant(lib, c):
    for want, rc, plan in row_plans(lib, c):
        assert T.plan_name(rc, plan) == want, (rc, plan)
        if rc == 0:
            assert plan['workgroups'] == c['B'] * plan['parts']
            if plan['part'] == 1:
                assert plan['parts'] == T.pre_parts_eff(c['pre']) and plan['Lp'] == T.pos_per(c['L'], plan['parts'])
            if plan['part'] == 3:
                assert plan['Lp'] == -(-c['L'] // c['fin']) and plan['parts'] == -(-c['L'] // plan['Lp']) and plan['lds_bytes'] == 0
                assert (plan['parts'] - 1) * plan['Lp'] < c['L'] <= plan['parts'] * plan['Lp']      # no empty range is launched


def test_rows_cover_every_field_value_and_refusal(lib):
    plans = [p for c in T.ROWS for p in row_plans(lib, c)]
    assert {rc for _, rc, _ in plans if rc < 0} == set(T.REFUSALS), 'a refusal code no row reaches'
    ok = [p for _, rc, p in plans if rc == 0]
    for part in (0, 1, 2):
        mine = [p for p in ok if p['part'] == part]
        assert {p['vec'] for p in mine} == {0, 1} and {p['opt_in'] for p in mine} == {0, 1}, part
    for part in (0, 1):
        mine = [p for p in ok if p['part'] == part]
        assert {p['wl_vec'] for p in mine} == {0, 1} and {p['kp32'] for p in mine} == {0, 1}, part
        assert {(p['vec'], p['wl_vec']) for p in mine} >= {(1, 1), (0, 1), (0, 0)}, part      # scalar kernel with vector W_l loads too
        assert {(p['vec'], p['kp32']) for p in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}, part
    pre = [p for p in ok if p['part'] == 1]
    assert {p['s_mfma'] for p in pre} == {0, 1} and {p['parts'] for p in pre} >= {1, 2, 4, 8}
    assert {p['parts'] for p in ok if p['part'] == 2} == {1, 2, 4, 8}
    assert any(p['part'] == 1 and p['vec'] and not p['s_mfma'] and c['F'] == 32 for c in T.ROWS if c['part'] == 'prefin'
               for _, rc, p in row_plans(lib, c)[:1] if rc == 0), 'F = 32 without whole MFMA tiles'
    rng = [(c, p) for c in T.ROWS if c['part'] == 'split' for _, rc, p in row_plans(lib, c) if rc == 0]
    assert any(p['parts'] < c['fin'] for c, p in rng) and {p['Lp'] for _, p in rng} >= {1, 44, 45, 64, 65, 512}


def test_limits_at_the_full_size_attention(lib):
    """the exact L where the opt-in starts and where the launch is refused (A = 256, E = 512, F = 32, K = 31), as the query reports them
    and as the rows on both sides of each see them; the position-range form stops at 512 positions per range"""
    full = dict(T.FULL, B=1, L=43, opts=())
    rc, p = query(lib, 0, full, 1)
    assert rc == 0 and (p['L_64k'], p['L_160k']) == (T.WHOLE_64K_LAST, T.WHOLE_LAST)
    rc, p = query(lib, 1, full, 1)
    assert rc == 0 and (p['L_64k'], p['L_160k']) == (T.PRE1_64K_LAST, T.PRE1_LAST)
    for part, parts, last64, last in ((0, 1, T.WHOLE_64K_LAST, T.WHOLE_LAST), (1, 1, T.PRE1_64K_LAST, T.PRE1_LAST)):
        assert query(lib, part, full, parts, L=last64)[1]['opt_in'] == 0 and query(lib, part, full, parts, L=last64 + 1)[1]['opt_in'] == 1
        assert query(lib, part, full, parts, L=last)[0] == 0 and query(lib, part, full, parts, L=last + 1)[0] == -5
        assert query(lib, part, full, parts, L=last64)[1]['lds_bytes'] <= 64 * 1024 < query(lib, part, full, parts, L=last64 + 1)[1]['lds_bytes']
        assert query(lib, part, full, parts, L=last)[1]['lds_bytes'] <= 160 * 1024 < query(lib, part, full, parts, L=last + 1)[1]['lds_bytes']
    # more pre ranges take longer texts; the fin part has no practical limit; a refused launch still reports the limits
    lasts = [query(lib, 1, full, n)[1]['L_160k'] for n in (1, 2, 4, 8)]
    assert lasts == sorted(lasts) and lasts[1] > T.PRE1_LAST
    assert query(lib, 2, full, 1)[1]['L_160k'] > 30000 and query(lib, 2, full, 8)[1]['L_64k'] == T.FIN_64K_LAST
    rc, p = query(lib, 0, full, 1, L=T.WHOLE_LAST + 1)
    assert rc == -5 and p['L_160k'] == T.WHOLE_LAST
    small = dict(A=32, E=64, F=8, K=7, B=1, opts=())
    assert query(lib, 3, small, 2, L=2 * T.LP_LAST)[0] == 0 and query(lib, 3, small, 2, L=2 * T.LP_LAST + 1)[0] == -8
    assert query(lib, 3, small, 64, L=64 * T.LP_LAST)[0] == 0


def test_what_the_pre_part_does_with_a_part_count(lib):
    """any power of two from 2 to 64 is taken, anything else runs as one range (what include/semitts.h says)"""
    full = dict(T.FULL, B=2, L=100, opts=())
    for parts, eff in ((0, 1), (1, 1), (2, 2), (3, 1), (4, 4), (6, 1), (8, 8), (16, 16), (32, 32), (64, 64), (65, 1), (128, 1), (-2, 1)):
        rc, p = query(lib, 1, full, parts)
        assert rc == 0 and p['parts'] == eff and p['workgroups'] == 2 * eff, parts


def test_alignment_flags(lib):
    full = dict(T.FULL, B=2, L=43, opts=())
    a18 = dict(T.A18, B=2, L=43, opts=())
    for part, bit, rc_full, rc_a18 in ((0, 'mem', -4, -4), (0, 'pm', -4, 0), (0, 'pq', -4, 0), (0, 'v', -4, 0), (0, 'wl', 0, 0), (0, 's', 0, 0),
                                       (1, 'pm', -4, 0), (1, 's', -4, 0), (1, 'pq', 0, 0), (1, 'mem', 0, 0), (1, 'wl', 0, 0),
                                       (2, 's', -4, 0), (2, 'pq', -4, 0), (2, 'mem', -4, -4), (2, 'pm', 0, 0), (2, 'wl', 0, 0)):
        assert query(lib, part, full, 1, al=T.AL_ALL & ~T.AL[bit])[0] == rc_full, (part, bit)
        assert query(lib, part, a18, 1, al=T.AL_ALL & ~T.AL[bit])[0] == rc_a18, (part, bit)
    rc, p = query(lib, 1, full, 1, al=T.AL_ALL & ~T.AL['wl'])       # a misaligned W_l: the scalar kernel, scalar W_l loads, no MFMA
    assert (p['vec'], p['wl_vec'], p['s_mfma']) == (0, 0, 0)
    for bit in ('pq', 's', 'mem', 'v', 'ws'):
        assert query(lib, 3, full, 2, al=T.AL_ALL & ~T.AL[bit])[0] == -4, bit
    assert query(lib, 3, full, 2, al=T.AL_ALL & ~T.AL['pm'] & ~T.AL['wl'])[0] == 0
    assert lib.st_attn_fwd_variant(None, None) == -1 and query(lib, 4, full, 1)[0] == -1 and query(lib, -1, full, 1)[0] == -1


@pytest.mark.parametrize('c', T.ROWS, ids=[c['id'] for c in T.ROWS])
def test_lds_restatement_agrees_with_the_library(lib, c):
    for _, rc, p in row_plans(lib, c):
        if rc in (0, -5) and p['part'] != 3:
            want = T.lds_bytes(p['part'], c['L'], c['A'], 4 if p['part'] == 1 else c['E'], c['F'], c['K'], p['parts'] if p['part'] == 1 else 1,
                               bool(p['s_mfma']))
            assert p['lds_bytes'] == want, p
            assert p['opt_in'] == (1 if want > 64 * 1024 else 0) and (rc == -5) == (want > 160 * 1024)


# ------------------------------------------------------------------------------------------------ the reference and its bounds
def computable(c):
    return c['L'] > 0 and c['E'] % 4 == 0 and c['E'] <= 2048 and c['K'] % 2 == 1


GAUSS = [c for c in T.ROWS if T.is_gaussian(c) and computable(c)]
_cache = {}


def ref_of(c):
    """(inputs, reference): computed once per row and shared"""
    if c['id'] not in _cache:
        x = T.gen_inputs(c)
        _cache[c['id']] = (x, T.reference(x))
    return _cache[c['id']]


def row_bounds(c, x, ref):
    """the loosest bounds the GPU test holds the row's outputs to"""
    if c['part'] == 'cf':
        return T.bounds(x, ref, 'pre')
    if c['part'] == 'split':
        plan_parts = -(-c['L'] // -(-c['L'] // max(c['fin'], 1)))
        return T.bounds(x, ref, 'ranges', ranges=plan_parts)
    b = T.bounds(x, ref, 'whole', E_slices=c['fin'] if c['fin'] in (1, 2, 4, 8) else 1)
    return b


@pytest.mark.parametrize('c', GAUSS, ids=[c['id'] for c in GAUSS])
def test_reference_agrees_with_the_oracle_in_float64(c):
    from oracle import tts_oracle as O
    x, ref = ref_of(c)
    A = c['A']
    W = {'p.query_layer.linear.weight': torch.eye(A, dtype=torch.float64), 'p.loc_conv.conv.weight': x['wc'].double(),
         'p.loc_linear.linear.weight': x['wl'].double(), 'p.v.linear.weight': x['v'].double().view(1, A)}
    ctx, w = O.attention_step(W, x['pq'].double(), x['mem'].double(), x['pm'].double(), x['w_prev'].double(), x['w_cum'].double(), 'p.')
    assert float((w - ref['w']).abs().max()) <= 1e-12 and float((ctx - ref['ctx']).abs().max()) <= 1e-12
    assert float((ref['cum'] - (w + x['w_cum'].double())).abs().max()) <= 1e-12
    # S given == S computed; the conv against a plain loop at a few positions
    again = T.reference(x, S_in=ref['S'])
    assert torch.equal(again['w'], ref['w']) and torch.equal(again['ctx'], ref['ctx'])
    K, L, pad = c['K'], c['L'], (c['K'] - 1) // 2
    hist = torch.stack([x['w_prev'], x['w_cum']], 1).double()
    for l in sorted({0, L // 2, L - 1}):
        acc = torch.zeros(c['B'], c['F'], dtype=torch.float64)
        for k in range(K):
            if 0 <= l + k - pad < L:
                acc += torch.einsum('bc,fc->bf', hist[:, :, l + k - pad], x['wc'][:, :, k].double())
        assert float((acc - ref['cf'][:, l]).abs().max()) <= 1e-13


def test_special_rows_are_what_they_claim():
    for c in T.ROWS:
        if c['special'] in (None, 'plan_only') or not computable(c):
            continue
        x, ref = ref_of(c)
        if c['special'] == 'sat':
            arg = x['pq'].double().unsqueeze(1) + ref['S']
            assert float(arg[..., 0].min()) > 50 and float(arg[..., 1 % c['A']].max()) < -50
        elif c['special'] == 'onehot':
            top = ref['e'].topk(2, -1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 100 and bool((ref['e'].argmax(-1) == c['L'] // 2).all())
            assert float(ref['w'].amax(-1).min()) == 1.0
        elif c['special'] == 'equal':
            assert float(ref['e'].abs().max()) == 0.0 and c['L'] & (c['L'] - 1) == 0
        elif c['special'] == 'zero_hist':
            assert torch.equal(ref['S'], x['pm'].double())


def test_bounds_are_not_slack():
    """at the shapes of test_gpu_parity.test_attention_step the bounds are within that test's thresholds; nowhere more than 4 times them"""
    worst = dict(w=0.0, cum=0.0, ctx=0.0)
    for c in GAUSS:
        if c['part'] == 'cf':
            continue
        x, ref = ref_of(c)
        b = row_bounds(c, x, ref)
        for k in worst:
            worst[k] = max(worst[k], float(b[k].max()))
        assert float(b['w'].max()) <= 4 * 2e-6 and float(b['ctx'].max()) <= 4 * 2e-5, (c['id'], float(b['w'].max()), float(b['ctx'].max()))
        if c['id'] in ('whole_full_L43', 'whole_full_L171'):
            assert float(b['w'].max()) <= 2e-6 and float(b['ctx'].max()) <= 2e-5, (c['id'], float(b['w'].max()), float(b['ctx'].max()))
            assert float(b['S'].max()) <= 2e-6 and float(b['cf'].max()) <= 1e-6
    assert worst['w'] > 0 and worst['ctx'] > 0


@pytest.mark.parametrize('defect', T.DEFECTS)
def test_each_defect_moves_the_reference_by_more_than_8_bounds(defect):
    n = 0
    for c in GAUSS:
        if not T.expressible(defect, c):
            continue
        if c['part'] == 'split' and defect in ('taps_reversed', 'window_plus1', 'window_minus1', 'channels_swapped', 'range_zero_history'):
            continue        # S is an input of the position-range form: the conv is not its business
        x, ref = ref_of(c)
        b = row_bounds(c, x, ref)
        arg = (defect, T.pos_per(c['L'], T.pre_parts_eff(c['pre']))) if defect == 'range_zero_history' else defect
        bad = T.reference(x, defect=arg)
        ratio = max(float(((bad[k] - ref[k]).abs() / b[k]).max()) for k in b)
        assert ratio > 8, (c['id'], defect, ratio)
        n += 1
    assert n >= 4, defect
