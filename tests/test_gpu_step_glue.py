"""The small kernels between the products of a decode step and of its backward step -- the per-step prenet normalisation and its
backward, the pointwise half of the LSTM cell backward, st_act_bwd, the decoder's pack / unpack / teacher-gradient / AdaIN kernels, the
scalar arithmetic of the losses -- and every (mode, batch tiles, load path) instantiation of the unpacked skinny products, each called
through its C entry point and compared with the float64 references of step_glue_cases.py (test_step_glue_host.py holds those to
torch.autograd and proves that the tables reach every cell).

Every operand sits in a buffer filled with NaN around its logical region: a read outside the region poisons the result, a write outside
it changes the bit pattern that is checked afterwards.  Kernels that round are held to bounds derived from the float64 reference (u = 2^-24
per rounding, written next to each check or in the reference's docstring); kernels that only move data are held to bit equality."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_glue_cases as SG   # noqa: E402
from helpers import U, bits, gen, guard_ok, guarded, inside, report, same_bits   # noqa: E402
from semi_tts_amd import _lib, ops   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD_ROWS = 4        # guard rows of a 2-D operand: 4 * ld floats keep the view's 16-byte alignment whatever ld is


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ guard-banded operands
def put(t, ld, dev, off=4):
    """(buffer, view): the CPU tensor t (rows, cols) as a view of leading dimension ld inside a NaN-filled buffer"""
    buf, v = guarded(t.shape[0], t.shape[1], ld, dev, pad_rows=PAD_ROWS, off=off, fill=NAN)
    v.copy_(t.to(dev))
    return buf, v


def out2d(rows, cols, ld, dev, off=4):
    return guarded(rows, cols, ld, dev, pad_rows=PAD_ROWS, off=off, fill=NAN)


def ok2d(buf, rows, cols, off=4):
    return guard_ok(buf, inside(rows, cols, pad_rows=PAD_ROWS, off=off), fill=NAN)


class Flat:
    """a contiguous operand of n floats inside a NaN-filled buffer (16 floats before it, 16 after it)"""
    OFF = 16

    def __init__(self, dev, n=None, src=None):
        n = src.numel() if src is not None else n
        self.n = n
        self.buf = torch.full((n + 2 * self.OFF,), NAN, device=dev)
        self.v = self.buf[self.OFF:self.OFF + n]
        if src is not None:
            self.v.copy_(src.reshape(-1).to(dev))

    def cpu(self):
        return self.v.cpu()

    def guard_ok(self):
        b = bits(self.buf)
        nan = bits(torch.tensor([NAN]))[0]
        return bool((b[:self.OFF] == nan).all()) and bool((b[self.OFF + self.n:] == nan).all())


def p(t):
    return ops._p(t)


def within(got, ref, tol):
    """(ok, worst err / tol): every element of got within tol of ref (all on the CPU, float64); an element whose tolerance is 0 must be
    exact"""
    err = (got.double() - ref).abs()
    ok = bool((err <= tol + 1e-300).all()) and bool(torch.isfinite(got).all())
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    return ok, ratio


# ===================================================================================================== st_prenet_norm_fwd
def _pn_out_tol(c, y, gamma, beta, rm, rv, mask, out_ref):
    """bound of the values st_prenet_norm_fwd writes (rows b0.., at least two of them in mode 3).  Modes 1 / 3: norm_bounds gives dxh, the
    affine map and the fma add 3u |pre|, the whole times 2 (test_layer_norm_forward_and_backward); mode 2: x - mean (1 rounding), rstd =
    1 / sqrt(var + eps) (3), the product (1) -> dxh = 6u |xhat|.  ReLU is 1-Lipschitz; the mask multiplies the bound and rounds once"""
    mode, P, b0 = c['mode'], c['P'], c['b0']
    x = y[b0:].double()
    if mode == 2:
        xh = (x - rm.double()) / torch.sqrt(rv.double() + SG.PN_EPS)
        dxh = 6 * U * xh.abs()
    else:
        xh, _, dxh, _ = SG.norm_bounds(x, None, 1 if mode == 1 else 0, SG.PN_EPS, SG.prenet_k(mode, x.shape[0], P))
    pre = xh * gamma.double() + beta.double()
    tol = 2 * (gamma.double().abs() * dxh + 3 * U * pre.abs())
    if mask is not None:
        tol = tol * mask[b0:].double().abs() + U * out_ref.abs()
    return tol


def _pn_stat_tols(x, rm_prev, rv_prev):
    """bounds of one running-statistics update of mode 3 on the nb >= 2 rows x (float64), momentum m, k = nb + 8:
      mean: e_m = k u max|x|;  new mean = (1 - m) rm + m mean: m e_m + 3u (|(1 - m) rm| + |m mean|)
      q = sum d^2, d = x - mean with |error| <= e_m + u |d|: e_q = 2 sum|d| e_m + (nb + 4) u q;  unbiased variance q / (nb - 1)
      new var = (1 - m) rv + m q / (nb - 1): m e_q / (nb - 1) + 3u (|(1 - m) rv| + m q / (nb - 1));   both times 2"""
    m, nb = SG.PN_MOMENTUM, x.shape[0]
    k = nb + 8
    mean = x.mean(0)
    d = x - mean
    e_m = k * U * x.abs().amax(0)
    q = (d * d).sum(0)
    e_q = 2 * d.abs().sum(0) * e_m + (nb + 4) * U * q
    t_rm = 2 * (m * e_m + 3 * U * (((1 - m) * rm_prev).abs() + (m * mean).abs()))
    t_rv = 2 * (m * e_q / (nb - 1) + 3 * U * (((1 - m) * rv_prev).abs() + m * q / (nb - 1)))
    return t_rm, t_rv


@pytest.mark.parametrize('mode', SG.PN_MODES)
def test_prenet_norm_fwd(dev, mode):
    """relu(norm(y)) * mask into a k-block range of a wider T16 buffer, rows b0 .. B - 1: the values, every float of the T16 buffer outside
    those rows' k-blocks (rows below b0, the neighbouring k-blocks, the pad columns of a ragged last k-block, pad rows of the last row
    tile), and the running statistics -- updated with momentum 0.3 and the unbiased variance in mode 3 (after one call and after two),
    bit-unchanged in modes 1 and 2.  A batch of ONE row in mode 3 (nn.BatchNorm1d refuses it, the header says nothing about it) is held to
    what does not depend on a variance of one sample: y - mean = 0, so the output is relu(beta) * mask; the running mean moves towards
    the row; num_batches_tracked counts the call; nothing is asserted about the running variance."""
    lib = _lib.load()
    eps, mom = SG.PN_EPS, SG.PN_MOMENTUM
    worst = dict(out=0.0, rm=0.0, rv=0.0)
    for c in [c for c in SG.prenet_fwd_cases() if c['mode'] == mode]:
        P, B, b0, kbs, kb0 = c['P'], c['B'], c['b0'], c['kb_stride'], c['kb0']
        y, gamma, beta, rm, rv = SG.prenet_input(mode, B, b0, P, seed=7 * B + P + b0)
        mask = SG.prenet_mask(B, P, seed=P + B) if c['mask'] else None
        yb, yv = put(y, c['ldy'], dev)
        mb, mv = put(mask, c['ldmask'], dev, off=2) if c['mask'] else (None, None)
        dst = Flat(dev, SG.t16_floats(B, kbs))
        gam, bet, frm, frv = Flat(dev, src=gamma), Flat(dev, src=beta), Flat(dev, src=rm), Flat(dev, src=rv)
        nbt = torch.tensor([-1, 7, -1], dtype=torch.int64, device=dev)
        view = ops.t16_view(dst.v, kbs, kb0)

        def call():
            _lib.check(lib.st_prenet_norm_fwd(p(yv), c['ldy'], mode, p(gam.v), p(bet.v), p(frm.v), p(frv.v), nbt[1:].data_ptr(), eps, mom,
                                              p(mv), c['ldmask'] if c['mask'] else 0, C.byref(view), b0, B, P, ops.stream_handle()),
                       'st_prenet_norm_fwd')
        call()
        out_ref, rm1, rv1 = SG.prenet_fwd_ref(y, mode, gamma, beta, rm, rv, eps, mom, mask, b0)
        pos = SG.t16_positions(range(b0, B), P, kbs, kb0)
        got_all = dst.cpu()
        got = got_all[pos]
        untouched = torch.ones(dst.n, dtype=torch.bool)
        untouched[pos.reshape(-1)] = False
        assert bool((bits(got_all)[untouched] == bits(torch.tensor([NAN]))[0]).all()), c
        assert dst.guard_ok() and ok2d(yb, B, P) and (mb is None or ok2d(mb, B, P, off=2)), c
        assert gam.guard_ok() and bet.guard_ok() and frm.guard_ok() and frv.guard_ok() and nbt[0] == -1 and nbt[2] == -1, c
        x = y[b0:].double()
        one_row = mode == 3 and B - b0 == 1
        if one_row:
            want = torch.relu(beta)[None] * (mask[b0:] if mask is not None else 1.0)
            assert same_bits(got, want), c
        else:
            ok, r = within(got, out_ref, _pn_out_tol(c, y, gamma, beta, rm, rv, mask, out_ref))
            worst['out'] = max(worst['out'], r)
            assert ok, (c, r)
        if mode != 3:
            assert same_bits(frm.cpu(), rm) and same_bits(frv.cpu(), rv) and int(nbt[1]) == 7, c
            continue
        assert int(nbt[1]) == 8, c
        if one_row:      # new mean = (1 - m) rm + m y: three roundings
            ok, r = within(frm.cpu(), rm1, 2 * 3 * U * (((1 - mom) * rm.double()).abs() + (mom * x[0]).abs()))
            assert ok, (c, r)
            continue
        t_rm, t_rv = _pn_stat_tols(x, rm.double(), rv.double())
        ok_m, r_m = within(frm.cpu(), rm1, t_rm)
        ok_v, r_v = within(frv.cpu(), rv1, t_rv)
        assert ok_m and ok_v, (c, r_m, r_v)
        call()      # a second step on the same rows: the statistics move again from where the first call left them
        rm2 = (1 - mom) * rm1 + mom * x.mean(0)
        rv2 = (1 - mom) * rv1 + mom * x.var(0, unbiased=True)
        t_rm2, t_rv2 = _pn_stat_tols(x, rm1, rv1)
        ok_m, r_m2 = within(frm.cpu(), rm2, t_rm2 + (1 - mom) * t_rm)
        ok_v, r_v2 = within(frv.cpu(), rv2, t_rv2 + (1 - mom) * t_rv)
        worst['rm'], worst['rv'] = max(worst['rm'], r_m, r_m2), max(worst['rv'], r_v, r_v2)
        assert ok_m and ok_v and int(nbt[1]) == 9, (c, r_m2, r_v2)
        assert same_bits(dst.cpu()[pos], got), c       # the same rows and statistics of the batch: the same output
    report('glue_prenet_norm_fwd', mode=mode, err_over_tol_out=worst['out'], err_over_tol_rm=worst['rm'], err_over_tol_rv=worst['rv'])


# ===================================================================================================== st_prenet_norm_bwd
def _pn_bwd_tols(mode, y, dn, gamma, rm, rv):
    """(tdx, t_dgamma, t_dbeta) of ONE call.  dx: norm_bounds' tdx in modes 1 / 3; mode 2: dx = gamma rstd d with rstd's 3 roundings and two
    products -> 6u |dx|, times 2.  dgamma = sum_r d xhat, an fma chain over the rows: (rows + 2) u sum |d xhat| + sum |d| dxh; dbeta = sum_r d:
    rows u sum |d|; both times 2"""
    rows, P = y.shape
    x, d, g = y.double(), dn.double(), gamma.double()[None]
    if mode == 2:
        rs = 1.0 / torch.sqrt(rv.double() + SG.PN_EPS)[None]
        xh = (x - rm.double()[None]) * rs
        dxh, tdx = 6 * U * xh.abs(), 2 * 6 * U * (g * rs * d).abs()
    else:
        xh, _, dxh, tdx = SG.norm_bounds(x, d * g, 1 if mode == 1 else 0, SG.PN_EPS, SG.prenet_k(mode, rows, P))
    t_dg = 2 * ((rows + 2) * U * (d * xh).abs().sum(0) + (d.abs() * dxh).sum(0))
    t_db = 2 * rows * U * d.abs().sum(0)
    return tdx, t_dg, t_db


@pytest.mark.parametrize('mode', SG.PN_MODES)
def test_prenet_norm_bwd(dev, mode):
    """dn -> gradient at the Linear's output, in place, and dgamma / dbeta accumulated over two calls on prefilled sums: after call one
    prefill + sums(1), after call two (prefill + sums(1)) + sums(2) -- each addition one more rounding of the magnitudes involved.
    A single row in mode 3 (autograd has no answer: nn.BatchNorm1d refuses it) is held to the closed form, where xhat = 0: dx = 0,
    dgamma unchanged, dbeta += dn."""
    lib = _lib.load()
    worst = dict(dx=0.0, dg=0.0, db=0.0)
    for c in [c for c in SG.prenet_bwd_cases() if c['mode'] == mode]:
        P, rows, ld, ldy = c['P'], c['rows'], c['ld'], c['ldy']
        g = gen(P + rows)
        pre_g, pre_b = torch.randn(P, generator=g), torch.randn(P, generator=g)
        dgam, dbet = Flat(dev, src=pre_g), Flat(dev, src=pre_b)
        acc_g, acc_b = pre_g.double(), pre_b.double()
        mag_g, mag_b = pre_g.double().abs(), pre_b.double().abs()
        tol_g, tol_b = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
        for call in (0, 1):
            y, gamma, _, rm, rv = SG.prenet_input(mode, rows, 0, P, seed=3 * P + rows + call)
            dn = torch.randn(rows, P, generator=g)
            db_, dv = put(dn, ld, dev)
            yb, yv = put(y, ldy, dev)
            gam, frm, frv = Flat(dev, src=gamma), Flat(dev, src=rm), Flat(dev, src=rv)
            _lib.check(lib.st_prenet_norm_bwd(p(dv), ld, p(yv), ldy, mode, p(gam.v), p(frm.v), p(frv.v), SG.PN_EPS, p(dgam.v), p(dbet.v),
                                              rows, P, ops.stream_handle()), 'st_prenet_norm_bwd')
            dx, dg, db = SG.prenet_bwd_ref(dn, y, mode, gamma, rm, rv, SG.PN_EPS)
            tdx, t_dg, t_db = _pn_bwd_tols(mode, y, dn, gamma, rm, rv)
            assert ok2d(db_, rows, P) and ok2d(yb, rows, P) and same_bits(yv, y), c
            assert same_bits(frm.cpu(), rm) and same_bits(frv.cpu(), rv) and gam.guard_ok() and frm.guard_ok() and frv.guard_ok(), c
            ok, r = within(dv.cpu(), dx, tdx)
            worst['dx'] = max(worst['dx'], r)
            assert ok, (c, call, r)
            if mode == 3 and rows == 1:
                assert float(dv.abs().max()) == 0.0, c
            acc_g, acc_b = acc_g + dg, acc_b + db
            mag_g, mag_b = mag_g + dg.abs(), mag_b + db.abs()
            tol_g, tol_b = tol_g + t_dg + 2 * U * mag_g, tol_b + t_db + 2 * U * mag_b
            ok_g, r_g = within(dgam.cpu(), acc_g, tol_g)
            ok_b, r_b = within(dbet.cpu(), acc_b, tol_b)
            worst['dg'], worst['db'] = max(worst['dg'], r_g), max(worst['db'], r_b)
            assert ok_g and ok_b and dgam.guard_ok() and dbet.guard_ok(), (c, call, r_g, r_b)
            if mode == 3 and rows == 1 and call == 0:
                assert same_bits(dgam.cpu(), pre_g), c
    report('glue_prenet_norm_bwd', mode=mode, err_over_tol_dx=worst['dx'], err_over_tol_dgamma=worst['dg'], err_over_tol_dbeta=worst['db'])


# ===================================================================================================== st_lstm_cell_bwd_pointwise
def _lstm_pw_run(dev, B, H, inp, combo, t16):
    """one call on strided, guard-banded operands -> (dgates (B, 4H), dc (B, H), T16 copy un-tiled or None), all on the CPU"""
    lib = _lib.load()
    c = SG.lstm_pw_c(inp, combo['c_prev'])
    ld0, ld1, ld2, ldc, ldcp, ldg = H + 7, H + 5, H + 6, H + 4, H + 9, 4 * H + 6
    b0, v0 = put(inp['dh0'], ld0, dev)
    b1, v1 = put(inp['dh1'], ld1, dev) if combo['dh1'] else (None, None)
    b2, v2 = put(inp['dh2'], ld2, dev) if combo['dh2'] else (None, None)
    bc, vc = put(c, ldc, dev)
    bcp, vcp = put(inp['c_prev'], ldcp, dev) if combo['c_prev'] else (None, None)
    sc = Flat(dev, src=inp['scale2']) if combo['scale2'] else None
    mk = Flat(dev, src=inp['mask']) if combo['mask'] else None
    gates, dc = Flat(dev, src=inp['gates']), Flat(dev, src=inp['dc'])
    bg, vg = out2d(B, 4 * H, ldg, dev)
    view, tiled, kbs = None, None, 0
    if t16 is not None:
        kbs = SG.kb16(4 * H) + t16['kb0'] + t16['kb_extra']
        tiled = Flat(dev, SG.t16_floats(B, kbs))
        view = C.byref(ops.t16_view(tiled.v, kbs, t16['kb0']))
    _lib.check(lib.st_lstm_cell_bwd_pointwise(p(v0), ld0, p(v1), ld1, p(v2), ld2, p(sc.v) if sc else None, p(mk.v) if mk else None,
                                              p(gates.v), p(vc), ldc, p(vcp), ldcp, p(dc.v), p(vg), ldg, view, B, H, ops.stream_handle()),
               'st_lstm_cell_bwd_pointwise')
    assert ok2d(bg, B, 4 * H) and dc.guard_ok() and gates.guard_ok() and same_bits(gates.cpu(), inp['gates'].reshape(-1))
    for buf, cols in ((b0, H), (b1, H), (b2, H), (bc, H), (bcp, H)):
        assert buf is None or ok2d(buf, B, cols)
    t = None
    if tiled is not None:
        pos = SG.t16_positions(range(B), 4 * H, kbs, t16['kb0'])
        all_ = tiled.cpu()
        untouched = torch.ones(tiled.n, dtype=torch.bool)
        untouched[pos.reshape(-1)] = False
        assert bool((bits(all_)[untouched] == bits(torch.tensor([NAN]))[0]).all()) and tiled.guard_ok()
        t = all_[pos]
    return vg.cpu(), dc.cpu().reshape(B, H), t


@pytest.mark.parametrize('B,H', SG.LSTM_PW_SHAPES)
def test_lstm_cell_bwd_pointwise(dev, B, H):
    """all 24 present / absent combinations of dh1, dh2 (+ scale2), mask and c_prev, every operand strided, with and without the T16
    copy of the gate gradients (a k-block range inside a wider buffer): the values against lstm_pw_ref's rounding count, the carried dc
    updated in place, the T16 copy bit-equal to the natural one and nothing else of its buffer written"""
    inp = SG.lstm_pw_inputs(B, H, seed=B + H)
    worst_g = worst_c = 0.0
    for t16 in SG.LSTM_PW_T16:
        for combo in SG.LSTM_PW_COMBOS:
            dg, dc, tiled = _lstm_pw_run(dev, B, H, inp, combo, t16)
            pick = lambda k: inp[k] if combo[k] else None
            rg, rc, tg, tc = SG.lstm_pw_ref(inp['dh0'], pick('dh1'), pick('dh2'), pick('scale2'), pick('mask'), inp['gates'],
                                            SG.lstm_pw_c(inp, combo['c_prev']), pick('c_prev'), inp['dc'])
            ok_g, r_g = within(dg, rg, tg)
            ok_c, r_c = within(dc, rc, tc)
            worst_g, worst_c = max(worst_g, r_g), max(worst_c, r_c)
            assert ok_g and ok_c, (combo, t16, r_g, r_c)
            assert (tiled is None) == (t16 is None) and (tiled is None or same_bits(tiled, dg)), (combo, t16)
    report('glue_lstm_cell_bwd_pointwise', B=B, H=H, err_over_tol_dgates=worst_g, err_over_tol_dc=worst_c)


def test_lstm_cell_bwd_pointwise_keeps_a_nan_in_its_element(dev):
    """one NaN in dh0: the four gate gradients and dc of that (b, u) are NaN, every other element is bit-equal to the run without it"""
    B, H, b, u = 5, 40, 2, 7
    inp = SG.lstm_pw_inputs(B, H, seed=1)
    combo = dict(dh1=True, dh2=True, scale2=True, mask=True, c_prev=True)
    dg0, dc0, t0 = _lstm_pw_run(dev, B, H, inp, combo, SG.LSTM_PW_T16[1])
    bad = dict(inp, dh0=inp['dh0'].clone())
    bad['dh0'][b, u] = NAN
    dg1, dc1, t1 = _lstm_pw_run(dev, B, H, bad, combo, SG.LSTM_PW_T16[1])
    hit_g = torch.zeros(B, 4 * H, dtype=torch.bool)
    hit_g[b, [u, H + u, 2 * H + u, 3 * H + u]] = True
    hit_c = torch.zeros(B, H, dtype=torch.bool)
    hit_c[b, u] = True
    assert torch.equal(torch.isnan(dg1), hit_g) and torch.equal(torch.isnan(dc1), hit_c) and torch.equal(torch.isnan(t1), hit_g)
    assert torch.equal(bits(dg1)[~hit_g], bits(dg0)[~hit_g]) and torch.equal(bits(dc1)[~hit_c], bits(dc0)[~hit_c])
    assert not bool(torch.isnan(dg0).any()) and not bool(torch.isnan(dc0).any())


# ===================================================================================================== st_act_bwd
@pytest.mark.parametrize('M,N', SG.ACT_BWD_SHAPES)
def test_act_bwd(dev, M, N):
    """dpre = dout * mask * act'(out) on four strided views, every activation code (ST_ACT_NONE without `out`), with and without the
    mask.  No activation and ReLU round only the mask product: bit equality with the float32 product; tanh / sigmoid: act_bwd_ref's bound"""
    lib = _lib.load()
    g = gen(M + N)
    dout = torch.randn(M, N, generator=g)
    pre = torch.randn(M, N, generator=g) * 2
    mask = SG.prenet_mask(M, N, seed=N)
    ldd, ldo, ldm, ldp = (N + 4 + SG.ACT_BWD_PAD[k] for k in ('ldd', 'ldo', 'ldm', 'ldp'))
    bd, vd = put(dout, ldd, dev)
    bm, vm = put(mask, ldm, dev)
    worst = 0.0
    for act, name in SG.ACTS.items():
        out = {'none': None, 'relu': torch.relu(pre), 'tanh': torch.tanh(pre), 'sigmoid': torch.sigmoid(pre)}[name]
        bo, vo = put(out, ldo, dev) if out is not None else (None, None)
        for with_mask in (False, True):
            bp, vp = out2d(M, N, ldp, dev)
            _lib.check(lib.st_act_bwd(p(vd), ldd, p(vo), ldo if out is not None else 0, act, p(vm) if with_mask else None,
                                      ldm if with_mask else 0, p(vp), ldp, M, N, ops.stream_handle()), 'st_act_bwd')
            assert ok2d(bp, M, N) and ok2d(bd, M, N) and ok2d(bm, M, N) and (bo is None or ok2d(bo, M, N)), (name, with_mask)
            got = vp.cpu()
            if name in ('none', 'relu'):
                want = dout * mask if with_mask else dout.clone()
                if name == 'relu':
                    want = want * (out > 0).float()
                assert same_bits(got + 0.0, want + 0.0), (name, with_mask)      # (+ 0.0: -0.0 and 0.0 are the same gradient)
            else:
                ref, tol = SG.act_bwd_ref(dout, out, act, mask if with_mask else None)
                ok, r = within(got, ref, tol)
                worst = max(worst, r)
                assert ok, (name, with_mask, r)
    report('glue_act_bwd', M=M, N=N, err_over_tol=worst)


# ===================================================================================================== pack / unpack
@pytest.mark.parametrize('c', SG.PACK_CASES, ids=lambda c: c['id'])
def test_decoder_pack_and_unpack(dev, c):
    """st_decoder_pack_dout (dmel / dstop present or NULL) and st_decoder_unpack_out against the direct statement of the layout, bit for
    bit: rows b >= B of every step slot and everything around the buffers keep their NaN, pack writes the pad columns as zeros, unpack
    never reads them (they hold NaN on its input); unpack of a packed pair gives dmel back and the r-fold sum of dstop, repeated r times"""
    lib = _lib.load()
    B, Bp, steps, r, M, ld = (c[k] for k in ('B', 'Bp', 'steps', 'r', 'n_mels', 'ld'))
    g = gen(ld + steps)
    dmel, dstop = torch.randn(B, steps * r, M, generator=g), torch.randn(B, steps * r, generator=g)
    fm, fs = Flat(dev, src=dmel), Flat(dev, src=dstop)
    nan_bits = bits(torch.tensor([NAN]))[0]
    packed = None
    for present in SG.PACK_PRESENT:
        dY = Flat(dev, steps * Bp * ld)
        _lib.check(lib.st_decoder_pack_dout(p(fm.v) if 'dmel' in present else None, p(fs.v) if 'dstop' in present else None, p(dY.v), ld,
                                            B, Bp, steps, r, M, ops.stream_handle()), 'st_decoder_pack_dout')
        got = dY.cpu().reshape(steps, Bp, ld)
        want = SG.pack_ref(dmel if 'dmel' in present else None, dstop if 'dstop' in present else None, B, steps, r, M, ld)
        assert same_bits(got[:, :B], want), present
        assert bool((bits(got[:, B:]) == nan_bits).all()) and dY.guard_ok() and fm.guard_ok() and fs.guard_ok(), present
        if len(present) == 2:
            packed = dY
    # unpack: the pad columns and the rows b >= B of its input hold NaN
    Y = torch.randn(steps, Bp, ld, generator=g)
    Y[:, B:] = NAN
    Y[:, :, r * M + 1:] = NAN
    for src, src_cpu in ((Flat(dev, src=Y), Y), (packed, packed.cpu().reshape(steps, Bp, ld))):
        mel, stop = Flat(dev, B * steps * r * M), Flat(dev, B * steps * r)
        _lib.check(lib.st_decoder_unpack_out(p(src.v), p(mel.v), p(stop.v), B, Bp, steps, r, M, ld, ops.stream_handle()), 'st_decoder_unpack_out')
        mel_ref, stop_ref = SG.unpack_ref(src_cpu, B, steps, r, M)
        assert same_bits(mel.cpu(), mel_ref.reshape(-1)) and same_bits(stop.cpu(), stop_ref.reshape(-1))
        assert mel.guard_ok() and stop.guard_ok() and src.guard_ok() and same_bits(src.cpu(), src_cpu.reshape(-1))
    # the packed pair, stated directly: mel is dmel again; the stop value of a step is the sum of its r gradients, r times
    s = torch.zeros(B, steps)
    for j in range(r):
        s = s + dstop.reshape(B, steps, r)[:, :, j]
    assert same_bits(mel.cpu(), dmel.reshape(-1)) and same_bits(stop.cpu().reshape(B, steps, r), s[:, :, None].expand(B, steps, r))


# ===================================================================================================== dteacher sum
@pytest.mark.parametrize('c', SG.DTEACHER_CASES, ids=lambda c: 'S%d_steps%d_Tt%d_B%d' % (c['S'], c['steps'], c['Tt'], c['Bt']))
def test_decoder_dteacher_sum(dev, c):
    """the slabs added in slab order: bit-equal to a float32 sum in that order, and within S roundings of the float64 sum; frames no step
    read are zero.  Rows b >= Bt and columns >= P of the slabs hold NaN: they are not part of the sum"""
    lib = _lib.load()
    S, steps, Tt, Bt, Bp, P, XQw = (c[k] for k in ('S', 'steps', 'Tt', 'Bt', 'Bp', 'P', 'XQw'))
    part = torch.randn(steps + 1, S, Bp, XQw, generator=gen(S + steps + Bt))
    part[:, :, Bt:] = NAN
    part[:, :, :, P:] = NAN
    src, out = Flat(dev, src=part), Flat(dev, Bt * Tt * P)
    _lib.check(lib.st_decoder_dteacher_sum(p(src.v), p(out.v), S, Bp, XQw, Bt, Tt, P, steps, ops.stream_handle()), 'st_decoder_dteacher_sum')
    got = out.cpu().reshape(Bt, Tt, P)
    assert same_bits(got, SG.dteacher_ref(part, S, Bt, Tt, P, steps, torch.float32))
    clean = torch.nan_to_num(part, nan=0.0)
    ref = SG.dteacher_ref(clean, S, Bt, Tt, P, steps, torch.float64)
    mag = SG.dteacher_ref(clean.abs(), S, Bt, Tt, P, steps, torch.float64)
    ok, r = within(got, ref, S * U * mag)            # S additions, each rounding at most the sum of the magnitudes
    assert ok and out.guard_ok() and src.guard_ok(), r
    assert float(got[:, max(steps - 1, 0):].abs().sum()) == 0.0
    report('glue_dteacher_sum', S=S, steps=steps, err_over_tol=r)


# ===================================================================================================== AdaIN backward
@pytest.mark.parametrize('B,Q', SG.ADAIN_BQ)
def test_adain_bwd(dev, B, Q):
    """dstd / dmean over 1 .. 17 steps (either side of the unroll of 8), step strides and leading dimensions beyond the logical sizes
    (everything between the logical rows and columns is NaN)"""
    lib = _lib.load()
    worst_s = worst_m = 0.0
    for c in [c for c in SG.ADAIN_CASES if (c['B'], c['Q']) == (B, Q)]:
        steps = c['steps']
        g = gen(B + Q + steps)
        da, hq = torch.randn(steps, B, Q, generator=g), torch.randn(steps, B, Q, generator=g)
        std, mean = torch.rand(B, Q, generator=g) + 0.5, torch.randn(B, Q, generator=g)
        big_da = torch.full((steps, c['da_rows'], c['da_ld']), NAN)
        big_hq = torch.full((steps, c['hq_rows'], c['hq_ld']), NAN)
        big_da[:, :B, :Q], big_hq[:, :B, :Q] = da, hq
        fda, fhq, fstd, fmean = Flat(dev, src=big_da), Flat(dev, src=big_hq), Flat(dev, src=std), Flat(dev, src=mean)
        dstd, dmean = Flat(dev, B * Q), Flat(dev, B * Q)
        _lib.check(lib.st_adain_bwd(p(fda.v), c['da_rows'] * c['da_ld'], c['da_ld'], p(fhq.v), c['hq_rows'] * c['hq_ld'], c['hq_ld'],
                                    p(fstd.v), p(fmean.v), p(dstd.v), p(dmean.v), B, Q, steps, ops.stream_handle()), 'st_adain_bwd')
        rs, rm_, ts, tm = SG.adain_ref(da, hq, std, mean)
        ok_s, r_s = within(dstd.cpu().reshape(B, Q), rs, ts)
        ok_m, r_m = within(dmean.cpu().reshape(B, Q), rm_, tm)
        worst_s, worst_m = max(worst_s, r_s), max(worst_m, r_m)
        assert ok_s and ok_m and dstd.guard_ok() and dmean.guard_ok(), (c, r_s, r_m)
    report('glue_adain_bwd', B=B, Q=Q, err_over_tol_dstd=worst_s, err_over_tol_dmean=worst_m)


# ===================================================================================================== scalars
@pytest.mark.parametrize('c', SG.SCALAR_CASES, ids=lambda c: 'n%d_m%d%s' % (c['n'], c['m'], '_nan' if c['nan'] else ''))
def test_scalar_combine_and_fanout(dev, c):
    """out[j] = sum_i W[j][i] x_i: a NaN term whose weight is zero makes the total (row 0) NaN, as sum(w_i * x_i) is in torch, and is
    skipped in the subset sums (rows j > 0), as the header says; st_scalar_fanout: out[i] = w_i * dout, one product, bit for bit"""
    lib = _lib.load()
    n, m = c['n'], c['m']
    W = SG.scalar_weights(n, m, c['nan'], seed=n + m)
    x = torch.randn(n, generator=gen(n * m)) * 3
    if c['nan']:
        x[n // 2] = NAN
    xs = [Flat(dev, src=x[i:i + 1]) for i in range(n)]
    outs = [Flat(dev, 1) for _ in range(m)]
    xa = (C.c_void_p * n)(*[p(f.v) for f in xs])
    oa = (C.c_void_p * m)(*[p(f.v) for f in outs])
    wa = (C.c_float * (n * m))(*[float(v) for v in W.reshape(-1)])
    _lib.check(lib.st_scalar_combine(xa, n, wa, m, oa, ops.stream_handle()), 'st_scalar_combine')
    got = torch.cat([f.cpu() for f in outs])
    ref, tol = SG.scalar_combine_ref(W, x)
    assert all(f.guard_ok() for f in outs) and all(f.guard_ok() for f in xs)
    rows = slice(1, m) if c['nan'] else slice(0, m)
    if c['nan']:
        assert bool(torch.isnan(got[0])) and bool(torch.isnan((W[0] * x).sum()))
    ok, r = within(got[rows], ref[rows], tol[rows])
    assert ok, (got, ref, r)
    dout = torch.tensor([1.7])
    fd, fo = Flat(dev, src=dout), Flat(dev, n)
    w0 = (C.c_float * n)(*[float(v) for v in W[0]])
    _lib.check(lib.st_scalar_fanout(p(fd.v), w0, n, p(fo.v), ops.stream_handle()), 'st_scalar_fanout')
    assert same_bits(fo.cpu(), W[0] * dout) and fo.guard_ok()
    report('glue_scalar_combine', n=n, m=m, err_over_tol=r)


@pytest.mark.parametrize('n', SG.SCALE_BY_N)
def test_scale_by(dev, n):
    """y = x * (*scalar): one product per element, bit for bit, up to a length past one full grid (4096 * 256) with a ragged end"""
    lib = _lib.load()
    x = torch.randn(n, generator=gen(n % 1000))
    f = torch.tensor([-0.37])
    fx, ff, fy = Flat(dev, src=x), Flat(dev, src=f), Flat(dev, n)
    _lib.check(lib.st_scale_by(p(fx.v), p(ff.v), p(fy.v), n, ops.stream_handle()), 'st_scale_by')
    assert same_bits(fy.cpu(), x * f) and fy.guard_ok() and fx.guard_ok() and same_bits(fx.cpu(), x)


# ===================================================================================================== unpacked skinny products
class SkOperand:
    """x (B, k) and w (rows, k) of one segment in guard-banded buffers at the segment's strides and offsets from a 16-byte boundary"""

    def __init__(self, dev, B, rows, seg, seed):
        self.x, self.w = SG.sk_operands(B, rows, seg, seed)
        self.xoff, self.woff = 4 + seg['xoff'], 4 + seg['woff']
        self.xb, self.xv = put(self.x, seg['ldx'], dev, off=self.xoff)
        self.wb, self.wv = put(self.w, seg['ldw'], dev, off=self.woff)
        self.seg = ops.seg(self.xv, self.wv, k=seg['k'])
        # the table's alignment is the real one: what sk_dispatch will see
        real = dict(k=seg['k'], ldx=self.seg.ldx, ldw=self.seg.ldw, xoff=(self.xv.data_ptr() % 16) // 4, woff=(self.wv.data_ptr() % 16) // 4)
        assert self.xv.data_ptr() % 4 == 0 and SG.sk_way(real) == SG.sk_way(seg), (real, seg)

    def guards_ok(self):
        return ok2d(self.xb, *self.x.shape, off=self.xoff) and ok2d(self.wb, *self.w.shape, off=self.woff)


def _sk_linear_single(dev, segs, B, N, ldy, seed0):
    """st_skinny_linear_fwd without epilogue on prepared SkOperands -> y on the CPU"""
    yb, yv = out2d(B, N, ldy, dev)
    arr = ops._segs([s.seg for s in segs])
    _lib.check(_lib.load().st_skinny_linear_fwd(arr, len(segs), None, 0, None, 0, p(yv), ldy, 0, None, 0, 0, B, N, ops.stream_handle()),
               'st_skinny_linear_fwd')
    assert ok2d(yb, B, N)
    return yv.cpu()


@pytest.mark.parametrize('c', SG.SK_LINEAR, ids=lambda c: c['id'])
def test_skinny_linear_every_instantiation(dev, c):
    """st_skinny_linear_fwd at every (batch tiles, load path): bias + ReLU + strided mask into a strided output.  2e-5: the bound of
    test_skinny_linear (test_gpu_parity.py) for the same operand distributions at K up to 1536; K here is at most 116"""
    B, N = c['B'], c['N']
    ops_ = [SkOperand(dev, B, N, s, seed=B + N + 10 * i) for i, s in enumerate(c['segs'])]
    g = gen(B * N)
    bias, mask = torch.randn(N, generator=g), (torch.rand(B, N, generator=g) > 0.5).float() * 2
    fb = Flat(dev, src=bias)
    mb, mv = put(mask, N + 7, dev)
    yb, yv = out2d(B, N, N + 9, dev)
    arr = ops._segs([s.seg for s in ops_])
    _lib.check(_lib.load().st_skinny_linear_fwd(arr, len(ops_), p(fb.v), 1, p(mv), N + 7, p(yv), N + 9, 0, None, 0, 0, B, N,
                                                ops.stream_handle()), 'st_skinny_linear_fwd')
    ref = SG.sk_linear_ref([s.x for s in ops_], [s.w for s in ops_], bias, 'relu', mask)
    err = float((yv.cpu().double() - ref).abs().max())
    report('glue_skinny_linear', id=c['id'], nb=SG.sk_nb(B), vec=int(SG.sk_vec(c['segs'])), err=err, tol=SG.SK_TOL_LINEAR)
    assert err < SG.SK_TOL_LINEAR and bool(torch.isfinite(yv).all()), err
    assert ok2d(yb, B, N) and ok2d(mb, B, N) and fb.guard_ok() and all(s.guards_ok() for s in ops_)


def _sk_cell_call(dev, segs, B, H, b_ih, b_hh, pre, c_prev, mask, want_gates):
    """st_lstm_cell_fwd on prepared SkOperands, every other operand strided and guard-banded -> (h, c, gates or None) on the CPU"""
    fbi = Flat(dev, src=b_ih) if b_ih is not None else None
    fbh = Flat(dev, src=b_hh) if b_hh is not None else None
    pb, pv = put(pre, 4 * H + 4, dev) if pre is not None else (None, None)
    cb, cv = put(c_prev, H + 6, dev) if c_prev is not None else (None, None)
    fm = Flat(dev, src=mask) if mask is not None else None
    hb, hv = out2d(B, H, H + 7, dev)
    ob, ov = out2d(B, H, H + 5, dev)
    fg = Flat(dev, B * 4 * H) if want_gates else None
    arr = ops._segs([s.seg for s in segs])
    _lib.check(_lib.load().st_lstm_cell_fwd(arr, len(segs), p(fbi.v) if fbi else None, p(fbh.v) if fbh else None, p(pv), 4 * H + 4, p(cv),
                                            H + 6, p(fm.v) if fm else None, p(hv), H + 7, p(ov), H + 5, p(fg.v) if fg else None, B, H,
                                            ops.stream_handle()), 'st_lstm_cell_fwd')
    assert ok2d(hb, B, H) and ok2d(ob, B, H) and (fg is None or fg.guard_ok()) and (pb is None or ok2d(pb, B, 4 * H))
    assert (cb is None or ok2d(cb, B, H)) and all(s.guards_ok() for s in segs)
    return hv.cpu(), ov.cpu(), fg.cpu().reshape(B, 4, H) if fg else None


def _cell_extras(B, H, seed):
    g = gen(seed)
    return dict(b_ih=torch.randn(4 * H, generator=g) * 0.1, b_hh=torch.randn(4 * H, generator=g) * 0.1,
                pre=torch.randn(B, 4 * H, generator=g) * 0.3, c_prev=torch.randn(B, H, generator=g),
                mask=(torch.rand(B, H, generator=g) > 0.1).float() / 0.9)


@pytest.mark.parametrize('c', SG.SK_CELL, ids=lambda c: c['id'])
def test_lstm_cell_every_instantiation(dev, c):
    """st_lstm_cell_fwd at every (batch tiles, load path), with every optional operand and with none.  1e-5: the bound of test_lstm_cell
    (test_gpu_parity.py) on h, c and the activated gates for the same operand distributions at K up to 1792; K here is at most 116"""
    B, H = c['B'], c['H']
    segs = [SkOperand(dev, B, 4 * H, s, seed=B + H + 10 * i) for i, s in enumerate(c['segs'])]
    ex = _cell_extras(B, H, seed=B * H)
    worst = 0.0
    for full in (True, False):
        e = ex if full else dict.fromkeys(ex)
        h, cc, gates = _sk_cell_call(dev, segs, B, H, e['b_ih'], e['b_hh'], e['pre'], e['c_prev'], e['mask'], full)
        rh, rc, rg = SG.sk_cell_ref([s.x for s in segs], [s.w for s in segs], e['b_ih'], e['b_hh'], e['pre'], e['c_prev'], e['mask'])
        errs = [float((h.double() - rh).abs().max()), float((cc.double() - rc).abs().max())]
        if full:
            errs.append(float((gates.double() - rg).abs().max()))
        worst = max([worst] + errs)
        assert max(errs) < SG.SK_TOL_CELL, (full, errs)
    report('glue_lstm_cell', id=c['id'], nb=SG.sk_nb(B), vec=int(SG.sk_vec(c['segs'])), err=worst, tol=SG.SK_TOL_CELL)


@pytest.mark.parametrize('c', SG.SK_LINEAR_PAIR, ids=lambda c: c['id'])
def test_skinny_linear_pair_every_instantiation(dev, c):
    """st_skinny_linear_pair_fwd: two jobs with their own K, inputs and weights in one launch, at every (batch tiles, load path) -- the load
    path is chosen over BOTH jobs.  Each job bit-equal to st_skinny_linear_fwd on the same operands (the two load paths feed the same
    values to the same MFMA sequence), and within test_skinny_linear's 2e-5 of float64"""
    B, N = c['B'], c['N']
    jobs = [SkOperand(dev, B, N, s, seed=B + N + 100 * j) for j, s in enumerate(c['jobs'])]
    ldy = N + 9
    ys = [out2d(B, N, ldy, dev) for _ in range(2)]
    arr = ops._segs([s.seg for s in jobs])
    ya = (C.c_void_p * 2)(*[p(v) for _, v in ys])
    _lib.check(_lib.load().st_skinny_linear_pair_fwd(arr, ya, ldy, B, N, ops.stream_handle()), 'st_skinny_linear_pair_fwd')
    worst = 0.0
    for j in range(2):
        got = ys[j][1].cpu()
        assert ok2d(ys[j][0], B, N) and jobs[j].guards_ok()
        err = float((got.double() - SG.sk_linear_ref([jobs[j].x], [jobs[j].w], None, None, None)).abs().max())
        worst = max(worst, err)
        assert err < SG.SK_TOL_LINEAR, (j, err)
        assert same_bits(got, _sk_linear_single(dev, [jobs[j]], B, N, ldy, 0)), j
    report('glue_skinny_linear_pair', id=c['id'], nb=SG.sk_nb(B), vec=int(SG.sk_vec(c['jobs'])), err=worst, tol=SG.SK_TOL_LINEAR)


@pytest.mark.parametrize('c', SG.SK_CELL_PAIR, ids=lambda c: c['id'])
def test_lstm_cell_pair_every_instantiation(dev, c):
    """st_lstm_cell_pair_fwd: two cells with their own K, inputs, weights and optional arrays (all present / all absent) in one launch, at
    every (batch tiles, load path).  Each job bit-equal to st_lstm_cell_fwd on the same operands and within test_lstm_cell's 1e-5"""
    B, H, opt = c['B'], c['H'], c['opt']
    jobs = [SkOperand(dev, B, 4 * H, s, seed=B + H + 100 * j) for j, s in enumerate(c['jobs'])]
    ex = [_cell_extras(B, H, seed=B * H + j) for j in range(2)]
    ldpre, ldcp, ldh, ldc = 4 * H + 4, H + 6, H + 7, H + 5
    fbh = [Flat(dev, src=e['b_hh']) for e in ex]
    pre = [put(e['pre'], ldpre, dev) for e in ex]
    cp = [put(e['c_prev'], ldcp, dev) for e in ex]
    hs, cs = [out2d(B, H, ldh, dev) for _ in range(2)], [out2d(B, H, ldc, dev) for _ in range(2)]
    fg = [Flat(dev, B * 4 * H) for _ in range(2)]
    arr2 = lambda ptrs: (C.c_void_p * 2)(*ptrs) if opt else None
    arr = ops._segs([s.seg for s in jobs])
    _lib.check(_lib.load().st_lstm_cell_pair_fwd(arr, arr2([p(f.v) for f in fbh]), arr2([p(v) for _, v in pre]), ldpre,
                                                 arr2([p(v) for _, v in cp]), ldcp, (C.c_void_p * 2)(*[p(v) for _, v in hs]), ldh,
                                                 (C.c_void_p * 2)(*[p(v) for _, v in cs]), ldc, arr2([p(f.v) for f in fg]), B, H,
                                                 ops.stream_handle()), 'st_lstm_cell_pair_fwd')
    worst = 0.0
    nan_bits = bits(torch.tensor([NAN]))[0]
    for j in range(2):
        e = ex[j] if opt else dict.fromkeys(ex[j])
        h, cc = hs[j][1].cpu(), cs[j][1].cpu()
        assert ok2d(hs[j][0], B, H) and ok2d(cs[j][0], B, H) and fg[j].guard_ok() and jobs[j].guards_ok()
        rh, rc, rg = SG.sk_cell_ref([jobs[j].x], [jobs[j].w], None, e['b_hh'], e['pre'], e['c_prev'], None)
        errs = [float((h.double() - rh).abs().max()), float((cc.double() - rc).abs().max())]
        if opt:
            errs.append(float((fg[j].cpu().reshape(B, 4, H).double() - rg).abs().max()))
        else:
            assert bool((bits(fg[j].cpu()) == nan_bits).all())         # no gates_out2: nothing written
        worst = max([worst] + errs)
        assert max(errs) < SG.SK_TOL_CELL, (j, errs)
        h1, c1, g1 = _sk_cell_call(dev, [jobs[j]], B, H, None, e['b_hh'], e['pre'], e['c_prev'], None, opt)
        assert same_bits(h, h1) and same_bits(cc, c1) and (not opt or same_bits(fg[j].cpu(), g1.reshape(-1))), j
    report('glue_lstm_cell_pair', id=c['id'], nb=SG.sk_nb(B), vec=int(SG.sk_vec(c['jobs'])), err=worst, tol=SG.SK_TOL_CELL)
