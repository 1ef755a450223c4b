"""Every forward form of the attention step -- st_attn_step_fwd, st_attn_pre_fwd, st_attn_fin_fwd, st_attn_fin_split_fwd, the location conv
seen through cf_out of the hosted pre part, and the two hand-off forms -- called through the C entry points at the rows of
attn_fwd_cases.py and held to that module's float64 reference within its derived bounds (test_attn_fwd_dispatch_host.py holds the
reference to the oracle and proves that the bounds are tight enough to catch a wrong kernel).

Every operand sits in a NaN-filled buffer: the kernels read clamped addresses and rows past L on purpose, and whatever they read there
must not reach a result; every output's surroundings must keep their bit pattern.  The forms that promise the same arithmetic are held
to bit equality, and NaN in an operand must surface as NaN exactly where the reference has it."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fwd_cases as T   # noqa: E402
import step_glue_cases as SG   # noqa: E402
from helpers import U, bits, guard_ok, guarded, inside, report, same_bits   # noqa: E402
from semi_tts_amd import _lib, ops   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD_ROWS = 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def p(t):
    return ops._p(t)


# ------------------------------------------------------------------------------------------------ guard-banded operands
class Flat:
    """n contiguous floats inside a NaN-filled buffer (16 floats before, 16 after, `off` floats past a 16-byte boundary)"""
    OFF = 16

    def __init__(self, dev, n=None, src=None, off=0):
        n = src.numel() if src is not None else n
        self.n, self.o = n, self.OFF + off
        self.buf = torch.full((n + 2 * self.OFF + off,), NAN, device=dev)
        self.v = self.buf[self.o:self.o + n]
        if src is not None:
            self.v.copy_(src.reshape(-1).to(dev))

    def cpu(self):
        return self.v.cpu()

    def guard_ok(self):
        b, f = bits(self.buf), bits(torch.tensor([NAN]))[0]
        return bool((b[:self.o] == f).all()) and bool((b[self.o + self.n:] == f).all())

    def untouched(self):
        return bool((bits(self.buf) == bits(torch.tensor([NAN]))[0]).all())


class Rows:
    """a (rows, cols) operand of leading dimension ld inside a NaN-filled buffer"""

    def __init__(self, dev, rows, cols, ld, src=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.buf, self.v = guarded(rows, cols, ld, dev, pad_rows=PAD_ROWS, off=4, fill=NAN)
        if src is not None:
            self.v.copy_(src.to(dev))

    def cpu(self):
        return self.v.cpu()

    def guard_ok(self):
        return guard_ok(self.buf, inside(self.rows, self.cols, pad_rows=PAD_ROWS, off=4), fill=NAN)

    def untouched(self):
        return bool((bits(self.buf) == bits(torch.tensor([NAN]))[0]).all())


class T16Out:
    """a T16 destination of (B, K) from k-block kb0 of a buffer wider than it needs, NaN everywhere"""

    def __init__(self, dev, B, K, kb0=0, extra=0):
        self.B, self.K, self.kb0, self.stride = B, K, kb0, kb0 + SG.kb16(K) + extra
        self.buf = torch.full((SG.t16_floats(B, self.stride),), NAN, device=dev)
        self.pos = SG.t16_positions(range(B), K, self.stride, kb0)

    def view(self):
        return ops.t16_view(self.buf, self.stride, self.kb0)

    def cpu(self):
        return self.buf.cpu()[self.pos]

    def guard_ok(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool)
        keep[self.pos.reshape(-1)] = False
        return bool((bits(self.buf)[keep] == bits(torch.tensor([NAN]))[0]).all())

    def untouched(self):
        return bool((bits(self.buf) == bits(torch.tensor([NAN]))[0]).all())


class Inputs:
    """the operands of a row on the device, each in its own guard-banded buffer"""

    def __init__(self, dev, c, x):
        o = c['opts']
        B, L = c['B'], c['L']
        self.pq = Flat(dev, src=x['pq'], off=1 if 'pq_off1' in o else 0)
        self.pm, self.wc, self.v = Flat(dev, src=x['pm']), Flat(dev, src=x['wc']), Flat(dev, src=x['v'])
        self.mem = Flat(dev, src=x['mem'], off=1 if 'mem_off1' in o else 0)
        self.wl = Flat(dev, src=x['wl'], off=1 if 'wl_off1' in o else 0)
        self.w_prev = Rows(dev, B, L, L + 9, src=x['w_prev']) if 'ld' in o else Flat(dev, src=x['w_prev'])
        self.ld_wprev = L + 9 if 'ld' in o else L
        self.w_cum = Flat(dev, src=x['w_cum'])
        self.hq, self.std, self.mean = Flat(dev, src=x['hq']), Flat(dev, src=x['std']), Flat(dev, src=x['mean'])


class Outputs:
    """w_out, w_cum_out and the context destinations the row's options ask for, NaN-filled"""

    def __init__(self, dev, c):
        o = c['opts']
        B, L, E = c['B'], c['L'], c['E']
        self.w = Rows(dev, B, L, L + 7, None) if 'ld' in o else Flat(dev, n=B * L)
        self.ld_w = L + 7 if 'ld' in o else L
        self.cum = Flat(dev, n=B * L)
        self.ctx = None
        if 't16' not in o:
            self.ctx = Rows(dev, B, E, E + 12, None) if 'ld' in o else Flat(dev, n=B * E)
        self.ld_ctx = E + 12 if 'ld' in o else E
        self.t16 = []
        if 't16' in o or 'nat_t16' in o or 'adain_t16' in o:
            self.t16 = [T16Out(dev, B, E)]
        if 't16x3' in o:
            self.t16 = [T16Out(dev, B, E, kb0=k, extra=x) for k, x in ((1, 2), (2, 0), (3, 1))]
        self.hadapt = Flat(dev, n=B * 12) if ('adain' in o or 'adain_t16' in o) else None
        self.B, self.L, self.E = B, L, E

    def fill(self, job):
        job.w_out, job.ld_wout, job.w_cum_out = p(self.w.v), self.ld_w, p(self.cum.v)
        if self.ctx is not None:
            job.ctx, job.ld_ctx = p(self.ctx.v), self.ld_ctx
        for i, t in enumerate(self.t16):
            job.ctx_dst[i] = t.view()
        job.n_ctx_dst = len(self.t16)

    def all(self):
        return [self.w, self.cum] + ([self.ctx] if self.ctx is not None else []) + self.t16 + ([self.hadapt] if self.hadapt is not None else [])

    def guards_ok(self):
        return all(b.guard_ok() for b in self.all())

    def untouched(self):
        return all(b.untouched() for b in self.all())

    def values(self):
        """(w, cum, ctx) on the CPU; every T16 destination must equal the natural context bit for bit"""
        w = self.w.cpu().reshape(self.B, self.L)
        cum = self.cum.cpu().reshape(self.B, self.L)
        ts = [t.cpu() for t in self.t16]
        ctx = self.ctx.cpu().reshape(self.B, self.E) if self.ctx is not None else ts[0]
        for t in ts:
            assert same_bits(t, ctx), 'a T16 destination differs from the natural context'
        return w, cum, ctx


def within(got, ref, tol):
    """(ok, worst err / tol): every element of got finite and within tol of ref"""
    err = (got.double() - ref).abs()
    ok = bool(torch.isfinite(got).all()) and bool((err <= tol).all())
    return ok, float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


def refused(lib, rc, word):
    msg = lib.st_last_error()
    torch.cuda.synchronize()
    return rc != 0 and msg is not None and word in msg.decode()


REFUSAL_WORDS = dict(refused_dims='bad', refused_k_even='odd', refused_e='E=', refused_align='aligned', refused_lds='LDS', refused_parts='parts',
                     refused_range_dims='A=', refused_lp='positions per part')


def check_outputs(name, c, out, ref, b):
    """the outputs of a run against the reference within the bounds b; returns the worst err / bound per output"""
    w, cum, ctx = out.values()
    assert out.guards_ok(), 'an output guard band was written'
    ratios = {}
    for k, got in (('w', w), ('cum', cum), ('ctx', ctx)):
        ok, ratios[k] = within(got, ref[k], b[k])
        print('%s %s %s: worst err / bound %.3f' % (name, c['id'], k, ratios[k]))
    report(name, id=c['id'], **ratios)
    assert all(r <= 1.0 for r in ratios.values()) and bool(torch.isfinite(ctx).all()), ratios
    wsum = w.double().sum(-1)
    assert float((wsum - 1).abs().max()) <= c['L'] * U, float((wsum - 1).abs().max())
    if c['special'] == 'equal':
        assert same_bits(w, torch.full_like(w, 1.0 / c['L']))
    if c['special'] == 'onehot':
        assert bool((w[:, c['L'] // 2] == 1.0).all()) and float(w.sum()) == c['B']
    return w, cum, ctx


# ===================================================================================================== st_attn_step_fwd
def step_job(c, I, out):
    job = _lib.StAttnStepJob()
    job.pq, job.pm, job.memory = p(I.pq.v), p(I.pm.v), p(I.mem.v)
    job.w_prev, job.ld_wprev, job.w_cum_prev = p(I.w_prev.v), I.ld_wprev, p(I.w_cum.v)
    job.loc_conv_w, job.loc_lin_w, job.v = p(I.wc.v), p(I.wl.v), p(I.v.v)
    out.fill(job)
    if out.hadapt is not None:
        job.h_q, job.ld_hq, job.Q = p(I.hq.v), 12, 12
        job.ada_std, job.ada_mean, job.h_adapt = p(I.std.v), p(I.mean.v), p(out.hadapt.v)
    job.L, job.A, job.E, job.F, job.K = c['L'], c['A'], c['E'], c['F'], c['K']
    return job


WHOLE = [c for c in T.ROWS if c['part'] == 'whole' and c['gpu']]


@pytest.mark.parametrize('c', WHOLE, ids=[c['id'] for c in WHOLE])
def test_whole_step(dev, c):
    lib = _lib.load()
    x = T.gen_inputs(c)
    I = Inputs(dev, c, x)
    out = Outputs(dev, c)
    rc = lib.st_attn_step_fwd(C.byref(step_job(c, I, out)), c['B'], ops.stream_handle())
    if c['want'].startswith('refused') or c['id'] in T.REFUSED_BY_ENTRY:
        assert refused(lib, rc, 'AdaIN' if c['id'] in T.REFUSED_BY_ENTRY else REFUSAL_WORDS[c['want']]) and out.untouched()
        return
    ops.check(rc, 'st_attn_step_fwd')
    ref = T.reference(x)
    w, cum, ctx = check_outputs('attn_fwd_whole', c, out, ref, T.bounds(x, ref, 'whole'))
    if out.hadapt is not None:
        h = out.hadapt.cpu().reshape(c['B'], 12)
        tol = 2 * U * (x['std'].double() * (x['hq'].double() - x['mean'].double())).abs() + 2 * U * x['std'].double() * x['hq'].double().abs()
        assert within(h, ref['hadapt'], tol + 1e-300)[0]
    out2 = Outputs(dev, c)
    ops.check(lib.st_attn_step_fwd(C.byref(step_job(c, I, out2)), c['B'], ops.stream_handle()), 'st_attn_step_fwd')
    w2, cum2, ctx2 = out2.values()
    assert same_bits(w, w2) and same_bits(cum, cum2) and same_bits(ctx, ctx2), 'two runs differ'


# ===================================================================================================== st_attn_pre_fwd + st_attn_fin_fwd
def pre_job(c, I, s_buf, parts, cf_out=None):
    return _lib.StAttnPreJob(pm=p(I.pm.v), w_prev=p(I.w_prev.v), ld_wprev=I.ld_wprev, w_cum_prev=p(I.w_cum.v), loc_conv_w=p(I.wc.v),
                             loc_lin_w=p(I.wl.v), s_buf=p(s_buf.v), L=c['L'], A=c['A'], F=c['F'], K=c['K'], parts=parts,
                             cf_out=p(cf_out.v) if cf_out is not None else None)


def fin_job(c, I, s_view, out, parts, status=None):
    job = _lib.StAttnFinJob()
    job.s_buf, job.memory, job.w_cum_prev, job.v = p(s_view), p(I.mem.v), p(I.w_cum.v), p(I.v.v)
    out.fill(job)
    job.parts, job.L, job.A, job.E, job.F, job.K = parts, c['L'], c['A'], c['E'], c['F'], c['K']
    job.status = ops._p(status, torch.int32)
    return job


def run_pre(lib, dev, c, I, parts):
    s = Flat(dev, n=c['B'] * c['L'] * c['A'])
    rc = lib.st_attn_pre_fwd(C.byref(pre_job(c, I, s, parts)), c['B'], ops.stream_handle())
    return rc, s


PREFIN = [c for c in T.ROWS if c['part'] == 'prefin' and c['gpu']]


@pytest.mark.parametrize('c', PREFIN, ids=[c['id'] for c in PREFIN])
def test_pre_then_fin(dev, c):
    lib = _lib.load()
    x = T.gen_inputs(c)
    I = Inputs(dev, c, x)
    B, L, A = c['B'], c['L'], c['A']
    rc, s = run_pre(lib, dev, c, I, c['pre'])
    if c['want'].startswith('refused'):
        assert refused(lib, rc, REFUSAL_WORDS[c['want']]) and s.untouched()
        return
    ops.check(rc, 'st_attn_pre_fwd')
    ref = T.reference(x)
    S = s.cpu().reshape(B, L, A)
    ok, ratio = within(S, ref['S'], T.bounds(x, ref, 'pre', mfma='.mfma' in c['want'])['S'])
    print('attn_fwd_pre %s S: worst err / bound %.3f' % (c['id'], ratio))
    report('attn_fwd_pre', id=c['id'], S=ratio)
    assert ok and s.guard_ok(), ratio        # (the guard band after the buffer: rows past L, dims past A of the last row)
    if c['special'] == 'zero_hist':
        assert same_bits(S, x['pm'])
    for parts in (1, 2, 4, c['pre']):        # any number of position ranges gives the same S bit for bit; so does a second run
        rc, s2 = run_pre(lib, dev, c, I, parts)
        ops.check(rc, 'st_attn_pre_fwd')
        assert same_bits(s2.v, s.v) and s2.guard_ok(), parts
    # ---- the fin part on the S the pre part wrote: the reference takes that S as its input
    out = Outputs(dev, c)
    rc = lib.st_attn_fin_fwd(p(I.pq.v), C.byref(fin_job(c, I, s.v, out, c['fin'])), B, ops.stream_handle())
    if c['want_fin'].startswith('refused'):
        assert refused(lib, rc, REFUSAL_WORDS[c['want_fin']]) and out.untouched()
        return
    ops.check(rc, 'st_attn_fin_fwd')
    ref = T.reference(x, S_in=S)
    w, cum, ctx = check_outputs('attn_fwd_fin', c, out, ref, T.bounds(x, ref, 'fin', E_slices=c['fin']))
    out2 = Outputs(dev, c)
    ops.check(lib.st_attn_fin_fwd(p(I.pq.v), C.byref(fin_job(c, I, s.v, out2, c['fin'])), B, ops.stream_handle()), 'st_attn_fin_fwd')
    w2, cum2, ctx2 = out2.values()
    assert same_bits(w, w2) and same_bits(cum, cum2) and same_bits(ctx, ctx2), 'two runs differ'
    if c['fin'] > 1:        # context slices repeat the energies and the softmax: the weights are those of one workgroup, bit for bit
        out1 = Outputs(dev, c)
        ops.check(lib.st_attn_fin_fwd(p(I.pq.v), C.byref(fin_job(c, I, s.v, out1, 1)), B, ops.stream_handle()), 'st_attn_fin_fwd')
        w1, cum1, ctx1 = check_outputs('attn_fwd_fin', dict(c, id=c['id'] + '/1'), out1, ref, T.bounds(x, ref, 'fin'))
        assert same_bits(w, w1) and same_bits(cum, cum1)


# ===================================================================================================== st_attn_fin_split_fwd
SPLIT = [c for c in T.ROWS if c['part'] == 'split' and c['gpu']]


def run_split(lib, dev, c, I, s, out, parts=None):
    parts = c['fin'] if parts is None else parts
    ws = Flat(dev, n=int(lib.st_attn_fin_split_workspace_floats(c['B'], c['E'], max(parts, 1))))
    rc = lib.st_attn_fin_split_fwd(p(I.pq.v), C.byref(fin_job(c, I, s.v, out, parts)), p(ws.v), c['B'], ops.stream_handle())
    return rc, ws


@pytest.mark.parametrize('c', SPLIT, ids=[c['id'] for c in SPLIT])
def test_fin_over_position_ranges(dev, c):
    lib = _lib.load()
    x = T.gen_inputs(c)
    I = Inputs(dev, c, x)
    S = T.reference(x)['S'].float()          # S is an input of this form: the float64 S, rounded once
    s = Flat(dev, src=S)
    out = Outputs(dev, c)
    rc, ws = run_split(lib, dev, c, I, s, out)
    if c['want'].startswith('refused'):
        assert refused(lib, rc, REFUSAL_WORDS[c['want']]) and out.untouched() and ws.untouched()
        return
    ops.check(rc, 'st_attn_fin_split_fwd')
    ref = T.reference(x, S_in=S)
    Lp = -(-c['L'] // c['fin'])
    ranges = -(-c['L'] // Lp)
    w, cum, ctx = check_outputs('attn_fwd_split', c, out, ref, T.bounds(x, ref, 'ranges', ranges=ranges))
    assert ws.guard_ok() and s.guard_ok()
    out2 = Outputs(dev, c)
    rc, _ = run_split(lib, dev, c, I, s, out2)
    ops.check(rc, 'st_attn_fin_split_fwd')
    w2, cum2, ctx2 = out2.values()
    assert same_bits(w, w2) and same_bits(cum, cum2) and same_bits(ctx, ctx2), 'two runs differ'


# ===================================================================================================== cf_out (the conv alone)
CF = [c for c in T.ROWS if c['part'] == 'cf' and c['gpu']]


@pytest.mark.parametrize('c', CF, ids=[c['id'] for c in CF])
def test_location_conv_through_cf_out(dev, c):
    """st_skinny_linear_packed_attnpre_fwd with a minimal linear (N = 16, K = 16): cf_out is the one direct view of the conv phase"""
    lib = _lib.load()
    x = T.gen_inputs(c)
    I = Inputs(dev, c, x)
    B, L, A, F = c['B'], c['L'], c['A'], c['F']
    g = torch.Generator().manual_seed(5)
    wlin, xin = torch.randn(16, 16, generator=g) * 0.25, torch.randn(B, 16, generator=g)
    packed = ops.pack_weight([wlin.to(dev)], [16], 16)
    x_t = ops.tile_rows(xin.to(dev))
    y = Flat(dev, n=B * 16)
    job = _lib.StPackedLinearJob()
    job.p = _lib.StPackedProduct(packed_w=p(packed), x=ops.t16_view(x_t, K=16), K=16, y=p(y.v), ldy=16, B=B, N=16)
    s, cf = Flat(dev, n=B * L * A), Flat(dev, n=B * L * F)
    ops.check(lib.st_skinny_linear_packed_attnpre_fwd(C.byref(job), C.byref(pre_job(c, I, s, c['pre'], cf_out=cf)), ops.stream_handle()),
              'st_skinny_linear_packed_attnpre_fwd')
    ref = T.reference(x)
    b = T.bounds(x, ref, 'pre')
    ok_cf, r_cf = within(cf.cpu().reshape(B, L, F), ref['cf'], b['cf'])
    ok_s, r_s = within(s.cpu().reshape(B, L, A), ref['S'], b['S'])
    print('attn_fwd_cf %s: worst err / bound cf %.3f S %.3f' % (c['id'], r_cf, r_s))
    report('attn_fwd_cf', id=c['id'], cf=r_cf, S=r_s)
    assert ok_cf and ok_s and cf.guard_ok() and s.guard_ok() and y.guard_ok(), (r_cf, r_s)
    assert float((y.cpu().reshape(B, 16).double() - xin.double() @ wlin.double().t()).abs().max()) < 1e-5
    rc, s1 = run_pre(lib, dev, c, I, 1)      # the hosted pre part is the stand-alone one, bit for bit
    ops.check(rc, 'st_attn_pre_fwd')
    assert same_bits(s1.v, s.v)


# ===================================================================================================== non-finite input
NONFINITE = ('whole_small_L13', 'whole_full_L65', 'whole_scal', 'fin2_full_L43', 'fin2_small_L13', 'split_lp45', 'split_L9_p4')


def _run_form(lib, dev, c, x, S=None):
    """(w, cum, ctx) of the row's form on the operands x (S: the S operand of the fin forms)"""
    I = Inputs(dev, c, x)
    out = Outputs(dev, c)
    if c['part'] == 'whole':
        ops.check(lib.st_attn_step_fwd(C.byref(step_job(c, I, out)), c['B'], ops.stream_handle()), 'st_attn_step_fwd')
    else:
        s = Flat(dev, src=S)
        if c['part'] == 'prefin':
            ops.check(lib.st_attn_fin_fwd(p(I.pq.v), C.byref(fin_job(c, I, s.v, out, c['fin'])), c['B'], ops.stream_handle()), 'st_attn_fin_fwd')
        else:
            ops.check(run_split(lib, dev, c, I, s, out)[0], 'st_attn_fin_split_fwd')
    assert out.guards_ok()
    return out.values()


@pytest.mark.parametrize('cid', NONFINITE)
def test_nan_surfaces_where_the_reference_has_it(dev, cid):
    """NaN in one utterance's pq, or in one element of its S (pm for the whole step), makes that utterance's w, w_cum_out and ctx NaN
    everywhere and leaves every other utterance bit for bit; NaN in memory[b, l, e] makes exactly ctx[b, e] NaN"""
    lib = _lib.load()
    c = [r for r in T.ROWS if r['id'] == cid][0]
    x = T.gen_inputs(c)
    S = T.reference(x)['S'].float()
    clean = _run_form(lib, dev, c, x, S)
    B, L, A, E = c['B'], c['L'], c['A'], c['E']
    bad_b, l0, a0, e0 = B - 1, L // 2, A - 1, E // 2 + 1
    for what in ('pq', 'S', 'mem'):
        x2 = {k: t.clone() for k, t in x.items()}
        S2 = S.clone()
        if what == 'pq':
            x2['pq'][bad_b, 1 % A] = NAN
        elif what == 'S':
            x2['pm'][bad_b, l0, a0] = NAN
            S2[bad_b, l0, a0] = NAN
        else:
            x2['mem'][bad_b, l0, e0] = NAN
        w, cum, ctx = _run_form(lib, dev, c, x2, S2)
        keep = [b for b in range(B) if b != bad_b]
        for got, ref in zip((w, cum, ctx), clean):
            assert same_bits(got[keep], ref[keep]), (what, 'another utterance changed')
        if what == 'mem':
            assert same_bits(w, clean[0]) and same_bits(cum, clean[1])
            nan = torch.isnan(ctx[bad_b])
            assert bool(nan[e0]) and int(nan.sum()) == 1, (what, int(nan.sum()))
            rest = torch.arange(E) != e0
            assert same_bits(ctx[bad_b][rest], clean[2][bad_b][rest])
        else:
            assert bool(torch.isnan(w[bad_b]).all()) and bool(torch.isnan(cum[bad_b]).all()) and bool(torch.isnan(ctx[bad_b]).all()), what


# ===================================================================================================== the hand-off forms
HAND_FIN = [(2, L, 256, 512, parts) for L, parts in ((1, 1), (6, 2), (7, 1), (48, 2), (49, 4), (65, 8))] + [(3, 7, 16, 32, 1), (5, 49, 32, 64, 2)]
HAND_RNG = [(2, 88, 256, 512, 2), (2, 90, 256, 512, 2), (3, 90, 32, 64, 4), (2, 65, 256, 512, 8)]


def _handoff_operands(dev, B, L, A, E, Q=48):
    g = torch.Generator().manual_seed(1000 * L + A)
    r = lambda *s: torch.randn(*s, generator=g)
    wq, hq = r(A, Q) * Q ** -0.5, r(B, Q)
    x = dict(S=r(B, L, A), mem=r(B, L, E), w_cum=torch.softmax(r(B, L), -1) + torch.softmax(r(B, L), -1), v=r(A) * A ** -0.5)
    packed = ops.pack_weight([wq.to(dev)], [Q], A)
    h_t = ops.tile_rows(hq.to(dev))
    pq = torch.empty(B, A, device=dev)
    ops.skinny_linear_packed(packed, ops.t16_view(h_t, K=Q), 16 * ops.kb16(Q), B, A, y=pq)
    c = dict(B=B, L=L, A=A, E=E, F=32, K=31, opts=('t16',))

    class I:
        pass
    I.mem, I.w_cum, I.v, I.s = Flat(dev, src=x['mem']), Flat(dev, src=x['w_cum']), Flat(dev, src=x['v']), Flat(dev, src=x['S'])
    return c, I, packed, h_t, pq, Q


@pytest.mark.parametrize('B,L,A,E,parts', HAND_FIN)
def test_query_projection_and_fin_in_one_launch(dev, B, L, A, E, parts):
    """st_query_attn_fin_fwd == the packed linear + st_attn_fin_fwd on the same operands, bit for bit, over epochs 1, 2, 3 on one granule
    buffer; the status word stays 0"""
    lib = _lib.load()
    c, I, packed, h_t, pq, Q = _handoff_operands(dev, B, L, A, E)
    out1 = Outputs(dev, c)
    ops.check(lib.st_attn_fin_fwd(p(pq), C.byref(fin_job(c, I, I.s.v, out1, parts)), B, ops.stream_handle()), 'st_attn_fin_fwd')
    w1, cum1, ctx1 = out1.values()
    assert bool(torch.isfinite(ctx1).all())
    gran = torch.zeros(B, 2 * A, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hv = ops.t16_view(h_t, K=Q)
    for epoch in (1, 2, 3):
        out = Outputs(dev, c)
        ops.check(lib.st_query_attn_fin_fwd(p(packed), C.byref(hv), 16 * ops.kb16(Q), p(gran), epoch,
                                            C.byref(fin_job(c, I, I.s.v, out, parts, status=status)), B, None, ops.stream_handle()),
                  'st_query_attn_fin_fwd')
        w, cum, ctx = out.values()
        assert int(status.item()) == 0
        assert same_bits(w, w1) and same_bits(cum, cum1) and same_bits(ctx, ctx1) and out.guards_ok(), epoch


def _run_rng(lib, dev, B, L, A, E, parts):
    """(three-launch outputs, [one-launch outputs of epochs 1, 2, 3], operands): the packed linear + st_attn_fin_split_fwd, then
    st_query_attn_rng_fwd on the same operands and one pair of granule buffers; the status word must read 0 after every epoch"""
    assert lib.st_query_attn_rng_fits(B, A, parts) == 1
    c, I, packed, h_t, pq, Q = _handoff_operands(dev, B, L, A, E)
    I.pq = Flat(dev, src=pq)
    out1 = Outputs(dev, c)
    ops.check(run_split(lib, dev, c, I, I.s, out1, parts)[0], 'st_attn_fin_split_fwd')
    three = out1.values()
    gran = torch.zeros(B, 2 * A, device=dev)
    xchg = torch.zeros(2 * int(lib.st_attn_rng_xchg_words(B, E, parts)), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    hv = ops.t16_view(h_t, K=Q)
    one = []
    for epoch in (1, 2, 3):
        out = Outputs(dev, c)
        ops.check(lib.st_query_attn_rng_fwd(p(packed), C.byref(hv), 16 * ops.kb16(Q), p(gran), p(xchg), epoch,
                                            C.byref(fin_job(c, I, I.s.v, out, parts, status=status)), B, ops.stream_handle()),
                  'st_query_attn_rng_fwd')
        one.append(out.values())
        assert int(status.item()) == 0 and out.guards_ok(), epoch
    return three, one, (c, I, pq)


@pytest.mark.parametrize('B,L,A,E,parts', HAND_RNG)
def test_query_projection_and_ranges_in_one_launch_against_float64(dev, B, L, A, E, parts):
    """st_query_attn_rng_fwd over epochs 1, 2, 3 on one pair of granule buffers: every epoch gives the same bits, within the bounds of
    the position-range form of float64 (on the pq the packed linear wrote); the status word stays 0"""
    lib = _lib.load()
    three, one, (c, I, pq) = _run_rng(lib, dev, B, L, A, E, parts)
    for got in one[1:]:
        assert all(same_bits(a, b) for a, b in zip(got, one[0])), 'two epochs differ'
    x = dict(pq=pq.cpu(), pm=I.s.cpu().reshape(B, L, A), mem=I.mem.cpu().reshape(B, L, E), v=I.v.cpu(), w_cum=I.w_cum.cpu().reshape(B, L),
             w_prev=torch.zeros(B, L), wc=torch.zeros(4, 2, 3), wl=torch.zeros(A, 4), hq=torch.zeros(B, 1), std=torch.zeros(B, 1),
             mean=torch.zeros(B, 1))
    ref = T.reference(x, S_in=x['pm'])
    b = T.bounds(x, ref, 'ranges', ranges=parts)
    ratios = {k: within(g, ref[k], b[k])[1] for k, g in zip(('w', 'cum', 'ctx'), one[0])}
    report('attn_fwd_rng', id='B%d_L%d_A%d_p%d' % (B, L, A, parts), **ratios)
    assert all(r <= 1.0 for r in ratios.values()) and bool(torch.isfinite(one[0][2]).all()), ratios


@pytest.mark.parametrize('B,L,A,E,parts', HAND_RNG)
def test_query_projection_and_ranges_in_one_launch_equals_three_launches(dev, B, L, A, E, parts):
    """st_query_attn_rng_fwd == the packed linear + st_attn_fin_split_fwd on the same operands, bit for bit, in every epoch: both combine
    steps add the denominators of up to 8 ranges part by part in the same expression (a tree over the lanes in at_combine_kernel made the
    weights differ by up to 3.7e-9 and the context by up to 1.2e-7)"""
    lib = _lib.load()
    three, one, _ = _run_rng(lib, dev, B, L, A, E, parts)
    for epoch, got in enumerate(one, 1):
        d = {k: float((g.double() - t.double()).abs().max()) for k, g, t in zip(('w', 'cum', 'ctx'), got, three)}
        print('attn_fwd_rng B%d L%d A%d parts%d epoch %d: max |one launch - three launches| %s' % (B, L, A, parts, epoch, d))
        report('attn_fwd_rng_vs_split', B=B, L=L, A=A, parts=parts, epoch=epoch, **d)
        assert all(same_bits(g, t) for g, t in zip(got, three)), (epoch, d)
