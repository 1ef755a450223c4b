"""Host-side half of the step-glue tests (no GPU): the float64 references of step_glue_cases.py agree with float64 torch.autograd of
F.layer_norm, F.batch_norm and an LSTM cell written with torch.sigmoid / torch.tanh, and the case tables reach every cell the kernels
can be run at -- each rule below restates the dispatch in Python and fails when a cell has no case."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_glue_cases as SG   # noqa: E402


# ===================================================================================================== references
@pytest.mark.parametrize('mode', SG.PN_MODES)
def test_prenet_references_against_autograd(mode):
    eps, mom = SG.PN_EPS, SG.PN_MOMENTUM
    for B, b0, P in ((5, 0, 8), (5, 3, 80), (17, 3, 257), (33, 31, 80)):
        y, gamma, beta, rm, rv = SG.prenet_input(mode, B, b0, P, seed=B + P)
        mask = SG.prenet_mask(B, P, seed=3)
        out, new_rm, new_rv = SG.prenet_fwd_ref(y, mode, gamma, beta, rm, rv, eps, mom, mask, b0)
        x = y[b0:].double().requires_grad_()
        g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
        trm, trv = rm.double().clone(), rv.double().clone()
        if mode == 1:
            n = F.layer_norm(x, (P,), g64, b64, eps)
        else:
            n = F.batch_norm(x, trm, trv, g64, b64, training=mode == 3, momentum=mom, eps=eps)
        want = torch.relu(n) * mask[b0:].double()
        assert torch.allclose(out, want.detach(), rtol=1e-12, atol=1e-12)
        if mode == 3:
            assert torch.allclose(new_rm, trm, rtol=1e-13, atol=0) and torch.allclose(new_rv, trv, rtol=1e-13, atol=0)
        else:
            assert new_rm is None and new_rv is None and torch.equal(trm, rm.double()) and torch.equal(trv, rv.double())
        # backward through the norm alone (the kernel gets the gradient at the norm's output)
        dn = torch.randn(B - b0, P, generator=SG.gen(7))
        n.backward(dn.double())
        dx, dg, db = SG.prenet_bwd_ref(dn, y[b0:], mode, gamma, rm, rv, eps)
        scale = float(x.grad.abs().max())
        assert float((dx - x.grad).abs().max()) <= 1e-9 * scale        # (1e4 means at unit spread: float64 itself keeps ~1e-12 here)
        assert torch.allclose(dg, g64.grad, rtol=1e-9, atol=1e-9) and torch.allclose(db, b64.grad, rtol=1e-12, atol=1e-12)


def test_prenet_training_reference_of_one_row():
    """a batch of one row: nn.BatchNorm1d refuses it; the reference normalises with var = 0 and gives no running variance"""
    y, gamma, beta, rm, rv = SG.prenet_input(3, 4, 3, 8, seed=1)
    with pytest.raises(ValueError):
        F.batch_norm(y[3:].double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=True)
    out, new_rm, new_rv = SG.prenet_fwd_ref(y, 3, gamma, beta, rm, rv, SG.PN_EPS, SG.PN_MOMENTUM, None, 3)
    assert torch.equal(out, torch.relu(beta.double())[None]) and new_rv is None
    assert torch.allclose(new_rm, 0.7 * rm.double() + 0.3 * y[3].double(), rtol=1e-14)
    dx, dg, db = SG.prenet_bwd_ref(torch.ones(1, 8), y[3:], 3, gamma, rm, rv, SG.PN_EPS)
    assert float(dx.abs().max()) == 0 and float(dg.abs().max()) == 0 and torch.equal(db, torch.ones(8, dtype=torch.float64))


def test_norm_bounds_hold_for_a_float32_evaluation():
    """the bounds are bounds: plain float32 torch (two passes) stays inside them, a one-pass variance at mean 1e4 does not"""
    x = torch.randn(33, 80, generator=SG.gen(2))
    x[:, 1] += 1e4
    xh, rs, dxh, _ = SG.norm_bounds(x.double(), None, 0, SG.PN_EPS, SG.prenet_k(3, 33, 80))
    xh32 = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + SG.PN_EPS)
    assert bool(((xh32.double() - xh).abs() <= 2 * dxh).all())
    one_pass = (x * x).mean(0) - x.mean(0) ** 2
    bad = (x - x.mean(0)) / torch.sqrt(one_pass.clamp_min(0) + SG.PN_EPS)
    assert not bool(((bad.double() - xh).abs() <= 2 * dxh).all())


@pytest.mark.parametrize('combo', SG.LSTM_PW_COMBOS, ids=lambda c: ''.join(k[0] + k[-1] for k, v in c.items() if v) or 'bare')
def test_lstm_pointwise_reference_against_autograd(combo):
    B, H = 5, 8
    inp = SG.lstm_pw_inputs(B, H, seed=11)
    g = SG.gen(5)
    z = (torch.randn(B, 4, H, generator=g, dtype=torch.float64) * 1.5).requires_grad_()
    cp = inp['c_prev'].double().requires_grad_()
    i, f, gg, o = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])
    c = i * gg + (f * cp if combo['c_prev'] else 0.0)
    h = o * torch.tanh(c)
    pick = lambda k: inp[k] if combo.get(k, True) else None
    dh = inp['dh0'].double()
    if combo['dh1']:
        dh = dh + inp['dh1'].double()
    if combo['dh2']:
        dh = dh + inp['dh2'].double() * (inp['scale2'].double() if combo['scale2'] else 1.0)
    if combo['mask']:
        dh = dh * inp['mask'].double()
    ((h * dh).sum() + (c * inp['dc'].double()).sum()).backward()
    gates = torch.stack([i, f, gg, o], 1).detach()
    dg, dc_out, tg, tc = SG.lstm_pw_ref(inp['dh0'], pick('dh1'), pick('dh2'), pick('scale2'), pick('mask'), gates, c.detach(),
                                        cp.detach() if combo['c_prev'] else None, inp['dc'])
    assert torch.allclose(dg, z.grad.reshape(B, 4 * H), rtol=1e-12, atol=1e-13)
    if combo['c_prev']:
        assert torch.allclose(dc_out, cp.grad, rtol=1e-12, atol=1e-13)
    else:
        assert torch.allclose(dc_out, (inp['dc'].double() + dh * o * (1 - torch.tanh(c) ** 2)).detach() * f.detach(), rtol=1e-12)
    assert bool((tg >= 0).all()) and bool((tc >= 0).all())


def test_lstm_forward_reference_against_torch_cell():
    B, H, K = 5, 8, 12
    g = SG.gen(3)
    x, hp, cp = (torch.randn(B, n, generator=g, dtype=torch.float64) for n in (K, H, H))
    cell = torch.nn.LSTMCell(K, H).double()
    h_t, c_t = cell(x, (hp, cp))
    h, c, _ = SG.sk_cell_ref([x, hp], [cell.weight_ih.detach(), cell.weight_hh.detach()], cell.bias_ih.detach(), cell.bias_hh.detach(),
                             None, cp, None)
    assert torch.allclose(h, h_t.detach(), rtol=1e-12, atol=1e-13) and torch.allclose(c, c_t.detach(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize('act', sorted(SG.ACTS))
def test_act_bwd_reference_against_autograd(act):
    g = SG.gen(act)
    pre = torch.randn(7, 33, generator=g, dtype=torch.float64).requires_grad_()
    fn = {'none': lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[SG.ACTS[act]]
    out = fn(pre)
    dout, mask = torch.randn(7, 33, generator=g), SG.prenet_mask(7, 33, 1)
    (out * mask.double()).backward(dout.double())
    ref, tol = SG.act_bwd_ref(dout, out.detach(), act, mask)
    assert torch.allclose(ref, pre.grad, rtol=1e-13, atol=1e-15) and bool((tol >= 0).all())


def test_pack_unpack_references_are_adjoint_and_state_the_layout():
    for c in SG.PACK_CASES[:6]:
        B, steps, r, M, ld = c['B'], c['steps'], c['r'], c['n_mels'], c['ld']
        g = SG.gen(ld)
        Y = torch.randn(steps, c['Bp'], ld, generator=g)
        mel, stop = SG.unpack_ref(Y, B, steps, r, M)
        for b, t, j in ((0, 0, 0), (B - 1, steps - 1, r - 1)):
            assert torch.equal(mel[b, t * r + j], Y[t, b, j * M:(j + 1) * M]) and stop[b, t * r + j] == Y[t, b, r * M]
        dmel, dstop = torch.randn(B, steps * r, M, generator=g), torch.randn(B, steps * r, generator=g)
        dY = SG.pack_ref(dmel, dstop, B, steps, r, M, ld)
        assert float(dY[:, :, r * M + 1:].abs().sum()) == 0
        # <unpack(Y), (dmel, dstop)> == <Y, pack(dmel, dstop)>: pack is the backward of unpack
        lhs = (mel.double() * dmel.double()).sum() + (stop.double() * dstop.double()).sum()
        rhs = (Y[:, :B].double() * dY.double()).sum()
        assert abs(float(lhs - rhs)) <= 1e-5 * (1 + abs(float(lhs)))      # (dY's stop column was summed in float32)


def test_dteacher_and_adain_references():
    part = torch.randn(4, 3, 5, 12, generator=SG.gen(1))
    d32, d64 = SG.dteacher_ref(part, 3, 3, 5, 7, 3, torch.float32), SG.dteacher_ref(part, 3, 3, 5, 7, 3, torch.float64)
    assert torch.allclose(d64[:, :2], part[1:3, :, :3, :7].double().sum(1).transpose(0, 1), rtol=1e-15, atol=1e-15)
    assert float(d64[:, 2:].abs().max()) == 0 and float((d32.double() - d64).abs().max()) < 1e-6
    g = SG.gen(2)
    hq = torch.randn(9, 5, 10, generator=g, dtype=torch.float64)
    std, mean = (torch.randn(5, 10, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2))
    da = torch.randn(9, 5, 10, generator=g, dtype=torch.float64)
    (std * (hq - mean)).backward(da)
    dstd, dmean, _, _ = SG.adain_ref(da, hq, std.detach(), mean.detach())
    assert torch.allclose(dstd, std.grad, rtol=1e-12, atol=1e-13) and torch.allclose(dmean, mean.grad, rtol=1e-12, atol=1e-13)


def test_scalar_combine_reference():
    W = SG.scalar_weights(8, 4, True, seed=1)
    x = torch.randn(8, generator=SG.gen(2))
    x[4] = float('nan')
    assert float(W[0, 4]) == 0 and bool((W[0, [0, 1, 2, 3, 5, 6, 7]] != 0).all())
    out, _ = SG.scalar_combine_ref(W, x)
    assert bool(torch.isnan(out[0])) and bool(torch.isfinite(out[1:]).all())
    assert bool(torch.isnan((W[0].double() * x.double()).sum()))       # what torch makes of sum(w_i * x_i)


# ===================================================================================================== coverage of the tables
def test_constants_are_the_headers():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'semitts.h')).read()
    assert int(re.search(r'#define ST_SCALAR_MAX (\d+)', hdr).group(1)) == SG.ST_SCALAR_MAX
    codes = {int(v): k.lower() for k, v in re.findall(r'#define ST_ACT_(\w+) (\d+)', hdr)}
    assert codes == SG.ACTS


def test_prenet_tables_reach_every_cell():
    fwd = SG.prenet_fwd_cases()
    for mode in (1, 2, 3):
        for P in (8, 80, 256, 257, 1024, 1040):
            for B in (1, 5, 17, 33):
                for b0 in {0, 3, B - 2}:
                    if 0 <= b0 < B:
                        for mask in (False, True):
                            hit = [c for c in fwd if (c['mode'], c['P'], c['B'], c['b0'], c['mask']) == (mode, P, B, b0, mask)]
                            assert len(hit) == 1, (mode, P, B, b0, mask)
            for rows in (1, 5, 33):
                assert [c for c in SG.prenet_bwd_cases() if (c['mode'], c['P'], c['rows']) == (mode, P, rows)]
    for c in fwd:
        assert c['ldy'] > c['P'] and c['ldmask'] > c['P'] and c['kb0'] == 2 and c['kb_stride'] > c['kb0'] + SG.kb16(c['P'])
    for c in SG.prenet_bwd_cases():
        assert c['ld'] > c['P'] and c['ldy'] > c['P']
    # the paths of norm.hip: a ragged last k-block, a second workgroup of the column-per-thread modes (P > 256), the re-read past the
    # NR_REG = 16 registers of a lane (P > 1024), more than one T16 row tile (B > 16), more than one workgroup of mode 1 (B - b0 > 4)
    Ps, Bs = {c['P'] for c in fwd}, {c['B'] for c in fwd}
    assert any(P % 16 for P in Ps) and any(P > 256 for P in Ps) and any(P > 16 * 64 for P in Ps) and 16 * 64 in Ps
    assert any(B > 16 for B in Bs) and any(B > 32 for B in Bs) and any(c['B'] - c['b0'] > 4 for c in fwd if c['mode'] == 1)
    assert any(c['mode'] == 3 and c['B'] - c['b0'] == 1 for c in fwd)
    for mode in (1, 2, 3):
        assert any(SG.prenet_has_big_mean(mode, c['B'] - c['b0'], c['P']) for c in fwd if c['mode'] == mode)
        assert any(SG.prenet_has_big_mean(mode, c['rows'], c['P']) for c in SG.prenet_bwd_cases() if c['mode'] == mode)
    assert SG.PN_MOMENTUM != 0.1


def test_lstm_pointwise_tables_reach_every_cell():
    want = set()
    for dh1 in (False, True):
        for dh2 in (False, True):
            for scale2 in ((False, True) if dh2 else (False,)):
                for mask in (False, True):
                    for c_prev in (False, True):
                        want.add((dh1, dh2, scale2, mask, c_prev))
    got = {(c['dh1'], c['dh2'], c['scale2'], c['mask'], c['c_prev']) for c in SG.LSTM_PW_COMBOS}
    assert len(want) == 24 and got == want and len(SG.LSTM_PW_COMBOS) == 24
    assert set(SG.LSTM_PW_SHAPES) == {(1, 4), (5, 40), (17, 52), (33, 64)}
    assert any(B * H > 256 for B, H in SG.LSTM_PW_SHAPES)          # more than one workgroup of 256 threads
    assert any(B > 16 for B, H in SG.LSTM_PW_SHAPES) and any(H % 16 for B, H in SG.LSTM_PW_SHAPES)     # T16: row tiles, gates across k-blocks
    assert SG.LSTM_PW_T16[0] is None and SG.LSTM_PW_T16[1]['kb0'] == 1 and SG.LSTM_PW_T16[1]['kb_extra'] > 0


def test_elementwise_tables_reach_every_cell():
    assert set(SG.ACTS) == {0, 1, 2, 3}
    assert {(1, 1), (7, 33), (300, 257)} <= set(SG.ACT_BWD_SHAPES) and any(M * N > SG.GRID_CAP for M, N in SG.ACT_BWD_SHAPES)
    assert all(v > 0 for v in SG.ACT_BWD_PAD.values())
    for r in (1, 2, 5):
        for n_mels in (3, 80):
            assert [c for c in SG.PACK_CASES if (c['r'], c['n_mels']) == (r, n_mels)]
    pads = {c['ld'] - c['r'] * c['n_mels'] for c in SG.PACK_CASES}
    assert pads == {1, 8} and all(c['Bp'] > c['B'] for c in SG.PACK_CASES)
    assert any(c['steps'] * c['B'] * c['ld'] > SG.GRID_CAP and c['steps'] * c['B'] * (c['r'] * c['n_mels'] + c['r']) > SG.GRID_CAP
               for c in SG.PACK_CASES)
    assert set(SG.PACK_PRESENT) == {('dmel', 'dstop'), ('dmel',), ('dstop',)}
    for S in (1, 3):
        kinds = {('one' if c['steps'] == 1 else 'all' if c['steps'] == c['Tt'] else 'fewer') for c in SG.DTEACHER_CASES if c['S'] == S
                 and c['steps'] <= c['Tt']}
        assert kinds == {'one', 'all', 'fewer'}, S
    assert all(c['Bp'] > c['Bt'] and c['XQw'] > c['P'] for c in SG.DTEACHER_CASES)
    for BQ in ((1, 4), (5, 100), (33, 256)):
        for steps in (1, 7, 8, 9, 17):
            hit = [c for c in SG.ADAIN_CASES if (c['B'], c['Q'], c['steps']) == (BQ[0], BQ[1], steps)]
            assert hit and hit[0]['da_ld'] > BQ[1] and hit[0]['hq_ld'] > BQ[1] and hit[0]['da_rows'] > BQ[0] and hit[0]['hq_rows'] > BQ[0]
    assert any((B * Q) % 256 and B * Q > 256 for B, Q in SG.ADAIN_BQ)      # a partial last workgroup behind a full one
    for n in (1, SG.ST_SCALAR_MAX):
        for m in (1, 4):
            assert {c['nan'] for c in SG.SCALAR_CASES if (c['n'], c['m']) == (n, m)} == {False, True}
    assert 1 in SG.SCALE_BY_N and any(n > 4096 * 256 + 3 for n in SG.SCALE_BY_N)


@pytest.mark.parametrize('table,key,sizes', [('SK_LINEAR', 'N', (1, 16, 17, 33)), ('SK_CELL', 'H', (4, 8, 52))])
def test_skinny_single_tables_reach_every_cell(table, key, sizes):
    cases = getattr(SG, table)
    nb = lambda B: 1 if B <= 16 else 2 if B <= 32 else 4
    for B in (3, 16, 17, 32, 33, 70):
        assert SG.sk_nb(B) == nb(B)
    cells = {(nb(c['B']), SG.sk_vec(c['segs'])) for c in cases}
    assert cells == {(n, v) for n in (1, 2, 4) for v in (False, True)}
    assert {c['B'] for c in cases} == {3, 16, 17, 32, 33, 70}
    ways = {SG.sk_way(s) for c in cases for s in c['segs']} - {None}
    assert ways == {'k', 'ldx', 'ptr'}
    assert {c[key] for c in cases} == set(sizes) and {len(c['segs']) for c in cases} == {1, 2, 3}
    assert all(sum(s['k'] for s in c['segs']) <= SG.SK_KMAX for c in cases)
    assert all(s['ldx'] >= s['k'] and s['ldw'] >= s['k'] for c in cases for s in c['segs'])


@pytest.mark.parametrize('table,key,sizes', [('SK_LINEAR_PAIR', 'N', (1, 16, 17, 33)), ('SK_CELL_PAIR', 'H', (4, 8, 52))])
def test_skinny_pair_tables_reach_every_cell(table, key, sizes):
    cases = getattr(SG, table)
    cells = {(SG.sk_nb(c['B']), SG.sk_vec(c['jobs'])) for c in cases}
    assert cells == {(n, v) for n in (1, 2, 4) for v in (False, True)}
    assert {c['B'] for c in cases} == {3, 16, 17, 32, 33, 70} and {c[key] for c in cases} == set(sizes)
    split = {(SG.sk_seg_vec(c['jobs'][0]), SG.sk_seg_vec(c['jobs'][1])) for c in cases}
    assert {(True, False), (False, True), (True, True)} <= split           # job 0 aligned and job 1 not, and the reverse
    assert {SG.sk_way(j) for c in cases for j in c['jobs']} - {None} == {'k', 'ldx', 'ptr'}
    assert all(c['jobs'][0]['k'] != c['jobs'][1]['k'] for c in cases)       # the two jobs never share a shape by accident
    assert {c['opt'] for c in cases} == {False, True}
    # a job on the 16-byte path next to one with k % 4 != 0: the only way in which loading job 1 as job 0 would changes VALUES
    assert any(SG.sk_seg_vec(c['jobs'][0]) and SG.sk_way(c['jobs'][1]) == 'k' for c in cases)
