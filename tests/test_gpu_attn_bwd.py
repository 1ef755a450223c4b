"""The attention-step backward and the BPTT loop forms against float64.  Needs a real MI355X: pytest -m gpu

Step rows (attn_bwd_cases.STEP): every launch st_attn_bwd_variant names -- plain with and without S, both blocks, both LDS tiers, the
hosted forms (whole step, fallback to two launches, two parts dual / NB2 / generic, four parts, beside the K-split partial product) --
against one location-sensitive attention step in float64 autograd.  Each output element must lie within a bound derived from the lengths
of its sums (u = 2^-24): E terms for dw = dctx . mem, L for the softmax backward, dv and dpq, A for dloc, F K for dhist, plus the 2e-7
absolute error of the kernel's tanh wherever tanh' appears; helpers.report records the measured fraction of each bound.  Outputs land in
sentinel-guarded buffers, strided inputs carry NaN in their gaps, a repeat call is bitwise the first.

Loop forms: the full-size decoder (helpers.full_tacotron, prenet dropout on, masks replayed through the oracle) in every BPTT form --
six launches, fused, overlap, split with 2 / 4 parts, K-split slabs 1 / 2 / 4 of both cells' products -- against ONE float64 reference
per shape; each run first checks (Decoder._last_bwd_forms) that it reached the form it means."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as T   # noqa: E402
from helpers import report   # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TANH_ABS = 2.4e-7          # ab_tanh: |error| <= ~2e-7 absolute (attention_bwd_body.h), with margin
SENT = 7777.0
GUARD = 64
ENV = ('ST_AB_NB2', 'ST_AB_NO_DUAL', 'ST_PART_KW16')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    return torch.device('cuda:0')


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ one step: inputs and reference
def make_step(c, seed=0, n_dctx=3, n_dw=2, dcum_add=True, t0=False):
    """float32 inputs of one step (CPU), the step's attention weights w = softmax(e) of its own forward"""
    B, L, A, E, F, K = c['B'], c['L'], c['A'], c['E'], c['F'], c['K']
    g = _g(1000 + seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc)   # noqa: E731
    x = dict(pq=r(B, A, sc=0.5), pm=r(B, L, A, sc=0.5), memory=r(B, L, E), Wc=r(F, 2, K, sc=1.0 / math.sqrt(2 * K)),
             Wl=r(A, F, sc=1.0 / math.sqrt(F)), v=r(A, sc=1.0 / math.sqrt(A)))
    wp = torch.softmax(r(B, L, sc=2.0), 1)
    x['w_prev'] = None if t0 else wp
    x['cum_prev'] = wp * 3.0 + torch.rand(B, L, generator=g, dtype=torch.float64)
    x['dctx'] = [r(B, E, sc=0.3) for _ in range(n_dctx)]
    x['dw'] = [r(B, L, sc=0.3) for _ in range(n_dw)]
    x['dcum'] = r(B, L, sc=0.3)
    x['dcum_add'] = r(B, L, sc=0.3) if dcum_add else None
    x = {k: (v.float() if torch.is_tensor(v) else ([t.float() for t in v] if isinstance(v, list) else v)) for k, v in x.items()}
    hist = torch.stack([x['w_prev'] if x['w_prev'] is not None else torch.zeros(B, L), x['cum_prev']], 1).double()
    loc = Fn.conv1d(hist, x['Wc'].double(), padding=(K - 1) // 2).transpose(1, 2)
    S = x['pm'].double() + loc @ x['Wl'].double().t()
    e = torch.tanh(x['pq'].double()[:, None, :] + S) @ x['v'].double()
    x['w'] = torch.softmax(e, 1).float()
    x['S'] = S.float()
    return x


def reference(x, c, has_s, split=False):
    """float64 autograd of the step with the kernel's inputs; returns (outputs, per-element bounds)"""
    B, L, A, E, F, K = c['B'], c['L'], c['A'], c['E'], c['F'], c['K']
    d = lambda t: t.double()     # noqa: E731
    w_prev = x['w_prev'] if x['w_prev'] is not None else torch.zeros(B, L)
    hist = torch.stack([d(w_prev), d(x['cum_prev'])], 1).requires_grad_()
    pq = d(x['pq']).requires_grad_()
    v = d(x['v'])[None].repeat(B, 1).requires_grad_()         # one copy per utterance: dv_t is per utterance
    Wc, Wl, mem, w = d(x['Wc']), d(x['Wl']), d(x['memory']), d(x['w'])
    loc = Fn.conv1d(hist, Wc, padding=(K - 1) // 2).transpose(1, 2)
    loc.retain_grad()
    s = pq[:, None, :] + d(x['pm']) + loc @ Wl.t()
    s.retain_grad()
    th = torch.tanh(s)
    e = (th * v[:, None, :]).sum(-1)
    # the kernel's softmax backward with the GIVEN w: de = w (g - w . g), i.e. e's gradient when w = softmax(e)
    G = sum(d(t) for t in x['dw']) if x['dw'] else torch.zeros(B, L, dtype=torch.float64)
    Dctx = sum(d(t) for t in x['dctx']) if x['dctx'] else torch.zeros(B, E, dtype=torch.float64)
    Dcum = d(x['dcum']) + (d(x['dcum_add']) if x['dcum_add'] is not None else 0.0)
    g = G + Dcum + torch.einsum('ble,be->bl', mem, Dctx)
    de = w * (g - (w * g).sum(1, keepdim=True))
    e.backward(de)
    out = dict(dpq=pq.grad, ds=s.grad, dloc=loc.grad, dhist=hist.grad, dv=v.grad, dctx=Dctx, loc=loc.detach(),
               hist_t=hist.detach().transpose(1, 2), dcum=Dcum + (hist.grad[:, 1] if split else 0.0))
    # ---- bounds: magnitudes carried along the same chain
    a = lambda t: d(t).abs()     # noqa: E731
    n_add = len(x['dctx']) + len(x['dw']) + 2
    ctx_mag = sum(a(t) for t in x['dctx']) if x['dctx'] else torch.zeros(B, E, dtype=torch.float64)
    g_mag = torch.einsum('ble,be->bl', mem.abs(), ctx_mag) + a(x['dcum']) + sum(a(t) for t in x['dw'])
    if x['dcum_add'] is not None:
        g_mag = g_mag + a(x['dcum_add'])
    err_g = (E + n_add + 4) * U * g_mag
    wg = (w.abs() * g_mag).sum(1, keepdim=True)
    err_dot = (L + 2) * U * wg + (w.abs() * err_g).sum(1, keepdim=True)
    de_mag = w.abs() * (g_mag + wg)
    err_de = w.abs() * (err_g + err_dot) + 4 * U * de_mag
    hist_mag = hist.detach().abs()
    loc_mag = Fn.conv1d(hist_mag, Wc.abs(), padding=(K - 1) // 2).transpose(1, 2)
    err_loc = (2 * K + 2) * U * loc_mag
    s_mag = d(x['pq']).abs()[:, None, :] + a(x['pm']) + loc_mag @ Wl.abs().t()
    err_s = 3 * U * s_mag + (F + 2) * U * (loc_mag @ Wl.abs().t()) + err_loc @ Wl.abs().t()
    th_v = th.detach()
    err_th = TANH_ABS + err_s
    vm = v.detach().abs()[:, None, :]
    ds_mag = de_mag[:, :, None] * vm * (1 + th_v ** 2)
    err_ds = err_de[:, :, None] * vm * (1 + th_v ** 2) + de_mag[:, :, None] * vm * 2 * th_v.abs() * err_th + 5 * U * ds_mag
    err_dv = (L + 2) * U * (de_mag[:, :, None] * th_v.abs()).sum(1) + (err_de[:, :, None] * th_v.abs() + de_mag[:, :, None] * err_th).sum(1)
    err_dpq = (L + 2) * U * ds_mag.sum(1) + err_ds.sum(1)
    dloc_mag = ds_mag @ Wl.abs()
    err_dloc = (A + 4) * U * dloc_mag + err_ds @ Wl.abs()
    convT = lambda y: torch.nn.grad.conv1d_input((B, 2, L), Wc.abs(), y.transpose(1, 2), padding=(K - 1) // 2)   # noqa: E731
    err_dhist = (F * K + 4) * U * convT(dloc_mag) + convT(err_dloc)
    err_dcum = 2 * U * (a(x['dcum']) + (a(x['dcum_add']) if x['dcum_add'] is not None else 0.0))
    if split:
        err_dcum = err_dcum + err_dhist[:, 1] + U * (a(x['dcum']) + convT(dloc_mag)[:, 1])
    bounds = dict(dpq=err_dpq, ds=err_ds, dloc=err_dloc, dhist=err_dhist, dv=err_dv, dctx=(len(x['dctx']) + 1) * U * ctx_mag + 1e-30,
                  loc=err_loc + 1e-30, hist_t=torch.zeros_like(out['hist_t']), dcum=err_dcum + 1e-30)
    return out, bounds


# ------------------------------------------------------------------------------------------------ device buffers
class Bufs:
    """outputs in sentinel-guarded buffers; strided inputs with NaN in their gaps"""

    def __init__(self, dev):
        self.dev, self.outs = dev, {}

    def out(self, name, *shape):
        n = 1
        for s in shape:
            n *= s
        t = torch.full((n + GUARD,), SENT, device=self.dev)
        self.outs[name] = (t, shape)
        return t

    def view(self, name):
        t, shape = self.outs[name]
        return t[:t.numel() - GUARD].view(*shape)

    def guards_intact(self):
        for k, (t, _) in self.outs.items():
            assert bool((t[-GUARD:] == SENT).all()), 'write past the end of ' + k

    def strided(self, x, extra):
        """(rows, n) with row stride n + extra, NaN in the gaps"""
        if x is None:
            return None, 0
        R, n = x.shape
        t = torch.full((R, n + extra), float('nan'), device=self.dev)
        t[:, :n] = x.to(self.dev)
        return t, n + extra

    def tailed(self, x):
        """contiguous copy with NaN behind its end (a read past the last row shows up)"""
        t = torch.full((x.numel() + GUARD,), float('nan'), device=self.dev)
        t[:x.numel()] = x.reshape(-1).to(self.dev)
        return t


def dev_inputs(x, c, dev, bufs):
    B, L, A, E, F, K = c['B'], c['L'], c['A'], c['E'], c['F'], c['K']
    di = dict(pq=bufs.tailed(x['pq']), pm=bufs.tailed(x['pm']), memory=bufs.tailed(x['memory']), v=x['v'].to(dev),
              Wc=x['Wc'].contiguous().to(dev), S=bufs.tailed(x['S']), cum_prev=bufs.tailed(x['cum_prev']))
    if c['wl'] == 'off1':
        wl = torch.zeros(A * F + 4, device=dev)
        wl[1:1 + A * F] = x['Wl'].reshape(-1).to(dev)
        di['Wl'], di['Wl_p'] = wl, wl.data_ptr() + 4
    else:
        di['Wl'] = x['Wl'].contiguous().to(dev)
        di['Wl_p'] = di['Wl'].data_ptr()
    di['w'], di['ld_w'] = bufs.strided(x['w'], 5)
    di['w_prev'], di['ld_wprev'] = bufs.strided(x['w_prev'], 3)
    di['dctx'] = [bufs.strided(t, 8) for t in x['dctx']]
    di['dw'] = [bufs.strided(t, 3) for t in x['dw']]
    di['dcum_add'], di['ld_dcum_add'] = bufs.strided(x['dcum_add'], 7)
    di['dcum'] = x['dcum'].to(dev).clone()
    return di


def out_bufs(c, bufs, parts=1):
    B, L, A, E, F = c['B'], c['L'], c['A'], c['E'], c['F']
    for n, s in (('dpq', (B, A)), ('dhist', (B, 2, L)), ('ds', (B, L, A)), ('loc', (B, L, F)), ('dloc', (B, L, F)), ('hist_t', (B, L, 2)),
                 ('dctx', (B, E)), ('dv', (B, A))):
        bufs.out(n, *s)
    if parts > 1:
        bufs.out('dloc_part', parts, B, L, F)
    from semi_tts_amd import ops
    t16 = torch.full((ops.t16_floats(B, A) + GUARD,), SENT, device=bufs.dev)
    bufs.outs['dpq_t16'] = (t16, (ops.t16_floats(B, A),))
    return ops.t16_view(t16, K=A)


def P(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def fill_job(c, di, o, t16v=None, s_in=None, loc_t=None):
    """the StAttnBwdJob of one step from the device inputs `di` and the output views `o`: the first three context addends in dctx, the rest
    in dctx_more (the slabs of a K-split product)"""
    from semi_tts_amd import _lib
    j = _lib.StAttnBwdJob()
    j.pq, j.pm, j.memory = P(di['pq']), P(di['pm']), P(di['memory'])
    j.w_prev, j.ld_wprev, j.w_cum_prev, j.w, j.ld_w = P(di['w_prev']), di['ld_wprev'], P(di['cum_prev']), P(di['w']), di['ld_w']
    j.loc_conv_w, j.loc_lin_w, j.v = P(di['Wc']), di['Wl_p'], P(di['v'])
    for q, (t, ld) in enumerate(di['dctx']):
        if q < 3:
            j.dctx[q], j.ld_dctx[q] = P(t), ld
        else:
            j.dctx_more[q - 3], j.ld_dctx_more[q - 3] = P(t), ld
    j.n_dctx, j.n_dctx_more = min(len(di['dctx']), 3), max(len(di['dctx']) - 3, 0)
    for q, (t, ld) in enumerate(di['dw']):
        j.dw_direct[q], j.ld_dw[q] = P(t), ld
    j.n_dw = len(di['dw'])
    j.dcum, j.dcum_add, j.ld_dcum_add = P(di['dcum']), P(di['dcum_add']), di['ld_dcum_add']
    j.dpq, j.dhist, j.ds_t, j.loc_t = P(o['dpq']), P(o['dhist']), P(o['ds']), P(loc_t)
    if t16v is not None:
        j.dpq_t16 = t16v
    j.dloc_t, j.hist_t, j.dctx_t, j.dv_t, j.s_in = P(o['dloc']), P(o['hist_t']), P(o['dctx']), P(o['dv']), P(s_in)
    j.B, j.L, j.A, j.E, j.F, j.K = c['B'], c['L'], c['A'], c['E'], c['F'], c['K']
    return j


def run_plain(c, x, dev, entry='t16'):
    """st_attn_step_bwd with the T16 copy of dpq and S per the row ('t16'), with S given and no T16 copy ('s'), or with neither ('plain':
    S is recomputed); returns outputs (CPU)"""
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    bufs = Bufs(dev)
    di = dev_inputs(x, c, dev, bufs)
    t16v = out_bufs(c, bufs)
    o = {k: bufs.view(k) for k in ('dpq', 'dhist', 'ds', 'loc', 'dloc', 'hist_t', 'dctx', 'dv')}
    s_in = di['S'] if (entry == 's' or (entry == 't16' and c['s'])) else None
    j = fill_job(c, di, o, t16v if entry == 't16' else None, s_in, o['loc'])
    _lib.check(lib.st_attn_step_bwd(C.byref(j), ops.stream_handle()), 'st_attn_step_bwd')
    torch.cuda.synchronize()
    bufs.guards_intact()
    res = {k: v.cpu() for k, v in o.items()}
    res['dcum'] = di['dcum'].cpu()
    if entry == 't16':
        res['dpq_t16'] = ops.untile_rows(bufs.outs['dpq_t16'][0], c['B'], c['A']).cpu()
    return res


def compare(name, got, ref, bounds, keys):
    worst = {}
    for k in keys:
        gk, rk, bk = got[k].double(), ref[k], bounds[k]
        assert gk.shape == rk.shape, (k, gk.shape, rk.shape)
        err = (gk - rk).abs()
        ok = err <= bk
        assert bool(ok.all()), '%s: %s outside its bound at %d elements (worst ratio %.3g, first %s)' % (
            name, k, int((~ok).sum()), float((err / bk.clamp_min(1e-300)).nan_to_num(float('inf')).max()),
            tuple(int(i) for i in (~ok).nonzero()[0]))
        worst[k] = float((err / bk.clamp_min(1e-300)).max())
    report('attn_bwd_step', case=name, **worst)
    return worst


PLAIN = [c for c in T.STEP if c['gpu'] and c['hosted'] == 0]
HOSTED = [c for c in T.STEP if c['gpu'] and c['hosted'] > 0]


def set_env(monkeypatch, c):
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    for e in c['env']:
        monkeypatch.setenv(e, '1')


def variant(c):
    from semi_tts_amd import _lib
    wl = 0x100000 + (4 if c['wl'] == 'off1' else 0)
    return T.step_name(_lib.load().st_attn_bwd_variant(c['L'], c['A'], c['E'], c['F'], c['K'], 1 if c['s'] else 0, c['parts'], c['hosted'],
                                                       c['B'], c['N'], wl))


@pytest.mark.parametrize('c', PLAIN, ids=[c['id'] for c in PLAIN])
def test_step_against_float64(dev, c, monkeypatch):
    set_env(monkeypatch, c)
    assert variant(c) == c['want']
    x = make_step(c, seed=c['L'])
    ref, bnd = reference(x, c, c['s'])
    got = run_plain(c, x, dev, 't16')
    keys = ['dpq', 'ds', 'dloc', 'dhist', 'dv', 'dctx', 'hist_t', 'dcum'] + ([] if c['s'] else ['loc'])
    compare(c['id'], got, ref, bnd, keys)
    assert torch.equal(got['dpq_t16'], got['dpq'])
    again = run_plain(c, x, dev, 't16')
    for k in keys:
        assert torch.equal(got[k], again[k]), k
    if c['s']:       # the entry point without the T16 copy: bitwise the same
        other = run_plain(c, x, dev, 's')
        for k in keys:
            assert torch.equal(got[k], other[k]), k


@pytest.mark.parametrize('L', [17, 49, 97])
def test_given_s_and_recomputed_s_agree(dev, L):
    """st_attn_step_bwd with the forward's S (s_in) and with S recomputed from pm and the location conv: each within its bound of
    the float64 reference, so within the sum of the bounds of each other"""
    c = T.S('x', L, B=3)
    x = make_step(c, seed=7)
    ref, b_s = reference(x, c, True)
    _, b_n = reference(x, c, False)
    gs = run_plain(c, x, dev, 's')
    gn = run_plain(dict(c, s=False), x, dev, 'plain')
    keys = ['dpq', 'ds', 'dloc', 'dhist', 'dv', 'dctx', 'dcum']
    compare('s_L%d' % L, gs, ref, b_s, keys)
    compare('nos_L%d' % L, gn, ref, b_n, keys + ['loc'])
    for k in keys:
        assert bool(((gs[k].double() - gn[k].double()).abs() <= b_s[k] + b_n[k]).all()), k


@pytest.mark.parametrize('n_dctx,n_dw,dcum_add,t0', [(0, 0, False, False), (1, 1, True, False), (3, 2, True, True), (4, 3, False, False),
                                                      (6, 3, True, False)])
def test_context_and_weight_addends(dev, n_dctx, n_dw, dcum_add, t0):
    """0 .. 6 context addends, 0 .. 3 direct weight addends, with and without dcum_add, the first step (w_prev NULL): each against the
    reference of the summed addends, and bitwise what the same addends give as one summed addend where the kernel's order allows it"""
    c = T.S('x', 43, B=4)
    x = make_step(c, seed=31, n_dctx=n_dctx, n_dw=n_dw, dcum_add=dcum_add, t0=t0)
    ref, bnd = reference(x, c, True)
    got = run_plain(c, x, dev, 't16')
    keys = ['dpq', 'ds', 'dloc', 'dhist', 'dv', 'dctx', 'hist_t', 'dcum']
    compare('addends_%d_%d_%d_%d' % (n_dctx, n_dw, dcum_add, t0), got, ref, bnd, keys)
    if n_dctx > 1:   # one addend holding the fp32 sum in the kernel's order (index order, from 0.0): the context gradient is bitwise that sum
        one = dict(x)
        s = torch.zeros_like(x['dctx'][0])
        for t in x['dctx']:
            s = s + t
        one['dctx'] = [s]
        g1 = run_plain(c, one, dev, 't16')
        assert torch.equal(g1['dctx'], got['dctx'])


def test_plain_entry_refuses_parts(dev):
    """the split forms exist only hosted: st_attn_step_bwd with parts = 2 (and a dloc_part buffer) is an argument error before any launch --
    the message names `parts` and every output still holds its sentinel"""
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    c = T.S('x', 43, B=4)
    x = make_step(c, seed=31)
    bufs = Bufs(dev)
    di = dev_inputs(x, c, dev, bufs)
    t16v = out_bufs(c, bufs, parts=2)
    o = {k: bufs.view(k) for k in ('dpq', 'dhist', 'ds', 'loc', 'dloc', 'hist_t', 'dctx', 'dv')}
    j = fill_job(c, di, o, t16v, di['S'], o['loc'])
    j.parts, j.dloc_part = 2, P(bufs.view('dloc_part'))
    dcum0 = di['dcum'].clone()
    with pytest.raises(RuntimeError, match='parts'):
        _lib.check(lib.st_attn_step_bwd(C.byref(j), ops.stream_handle()), 'st_attn_step_bwd')
    torch.cuda.synchronize()
    for k, (t, _) in bufs.outs.items():
        assert bool((t == SENT).all()), k + ' was written'
    assert torch.equal(di['dcum'], dcum0)


# ------------------------------------------------------------------------------------------------ hosted forms
def run_hosted(c, x, dev):
    """the hosted launch (beside a product y = xp W^T of N outputs, or the K-split partial product) and, for parts > 1, the history job in
    st_skinny_linear_packed_attn_hist; returns attention outputs and the products' results (CPU) and their float64 references"""
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    B, L, A, E, F, K = c['B'], c['L'], c['A'], c['E'], c['F'], c['K']
    parts = c['parts']
    N, KP = c['N'], 256
    g = _g(55)
    W = torch.randn(N, KP, generator=g) / 16
    xp = torch.randn(B, KP, generator=g)
    Wd, xd = W.to(dev), xp.to(dev)
    packed = ops.pack_weight([Wd], [KP], N)
    x_t16 = ops.tile_rows(xd)
    xv = ops.t16_view(x_t16, K=KP)
    bufs = Bufs(dev)
    di = dev_inputs(x, c, dev, bufs)
    t16v = out_bufs(c, bufs, parts)
    o = {k: bufs.view(k) for k in ('dpq', 'dhist', 'ds', 'loc', 'dloc', 'hist_t', 'dctx', 'dv')}
    j = fill_job(c, di, o, t16v, di['S'])
    if parts > 1:
        j.parts, j.dloc_part = parts, P(bufs.view('dloc_part'))
    prod = {}
    if c['hosted'] == 1:
        y = bufs.out('y', B, N)
        prd = ops.packed_product(packed, xv, KP, y, N, B, N)
        _lib.check(lib.st_skinny_linear_packed_lstm_bwd_attn_bwd(C.byref(prd), None, C.byref(j), ops.stream_handle()),
                   'st_skinny_linear_packed_lstm_bwd_attn_bwd')
        prod['y'] = (lambda: bufs.view('y'))
    else:
        S_ = 2
        bufs.out('part', S_, B, N)
        _lib.check(lib.st_skinny_partial_attn_bwd(P(packed), C.byref(xv), KP, P(bufs.view('part')), S_, B, N, C.byref(j), ops.stream_handle()),
                   'st_skinny_partial_attn_bwd')
        prod['y'] = (lambda: bufs.view('part').sum(0))
    if parts > 1:
        hj = _lib.StAttnHistJob()
        hj.dloc_part, hj.parts, hj.loc_conv_w = P(bufs.view('dloc_part')), parts, P(di['Wc'])
        hj.w_prev, hj.ld_wprev, hj.w_cum_prev = P(di['w_prev']), di['ld_wprev'], P(di['cum_prev'])
        hj.dloc_t, hj.hist_t, hj.dhist, hj.dcum = P(o['dloc']), P(o['hist_t']), P(o['dhist']), P(di['dcum'])
        hj.B, hj.L, hj.F, hj.K = B, L, F, K
        y2 = bufs.out('y2', B, N)
        prd2 = ops.packed_product(packed, xv, KP, y2, N, B, N)
        _lib.check(lib.st_skinny_linear_packed_attn_hist(C.byref(prd2), C.byref(hj), ops.stream_handle()), 'st_skinny_linear_packed_attn_hist')
        prod['y2'] = (lambda: bufs.view('y2'))
    torch.cuda.synchronize()
    bufs.guards_intact()
    res = {k: v.cpu() for k, v in o.items()}
    res['dcum'] = di['dcum'].cpu()
    res['dpq_t16'] = ops.untile_rows(bufs.outs['dpq_t16'][0], B, A).cpu()
    y64 = xp.double() @ W.double().t()
    yb = (KP + 4) * U * (xp.double().abs() @ W.double().abs().t())
    for k, f in prod.items():
        res[k] = f().cpu()
    return res, y64, yb


@pytest.mark.parametrize('c', HOSTED, ids=[c['id'] for c in HOSTED])
def test_hosted_step_against_float64(dev, c, monkeypatch):
    set_env(monkeypatch, c)
    assert variant(c) == c['want']
    split = c['parts'] > 1
    # the BPTT loop's split form: no dcum_add (dcum holds the total gradient w.r.t. cum_t); the hosted forms see up to 3 + 3 context addends
    x = make_step(c, seed=c['L'] + c['B'], n_dctx=6 if c['hosted'] == 2 else 3, dcum_add=not split)
    ref, bnd = reference(x, c, True, split=split)
    got, y64, yb = run_hosted(c, x, dev)
    keys = ['dpq', 'ds', 'dloc', 'dhist', 'dv', 'dctx', 'hist_t', 'dcum']
    worst = compare(c['id'], got, ref, bnd, keys)
    assert torch.equal(got['dpq_t16'], got['dpq'])
    for k in ('y', 'y2'):
        if k in got:
            err = (got[k].double() - y64).abs()
            assert bool((err <= yb).all()), (k, float((err / yb).max()))
            worst[k] = float((err / yb).max())
    report('attn_bwd_hosted', case=c['id'], **worst)
    again, _, _ = run_hosted(c, x, dev)
    for k in keys + ['y']:
        assert torch.equal(got[k], again[k]), k


# ------------------------------------------------------------------------------------------------ the BPTT loop forms at full size
FORM_KNOBS = {
    'six': dict(fuse=False, overlap=False, parts=1),
    'fused': dict(fuse=True, overlap=False, parts=1),
    'overlap': dict(fuse=True, overlap=True, parts=1),
    'split2': dict(parts=2), 'split4': dict(parts=4),
    'dxd1': dict(parts=2, dsplits=1), 'dxd2': dict(parts=2, dsplits=2), 'dxd4': dict(parts=2, dsplits=4),
    'dxq1': dict(parts=2, qsplits=1), 'dxq2': dict(parts=2, qsplits=2), 'dxq4': dict(parts=2, qsplits=4),
}


def expected_form(form, B, L):
    k = dict(dict(fuse=True, overlap=True, parts=2, dsplits=2, qsplits=4), **FORM_KNOBS[form])
    if not k['fuse']:
        return 'six'
    if not k['overlap']:
        return 'fused'
    if k['parts'] == 1 or L > T.WIDE_HOSTED_LAST:
        return 'overlap'
    if k['parts'] == 4 or B != 32:        # the partial products need 16 < B <= 32 without pad rows (Bp = B)
        return 'split%d' % k['parts']
    return 'split2.d%d.q%d' % (k['dsplits'], k['qsplits'])


def decoder_reference(dev, B, L, steps, seed):
    """the full-size decoder (prenet dropout on) and its float64 reference through the oracle, masks drawn there and replayed"""
    from helpers import full_hp, full_tacotron, masks_to, split_masks
    from oracle import tts_oracle as O
    m = full_tacotron(dev, seed=seed, prenet_dropout=0.5).train()
    dec = m.decoder
    r, n_mels = dec.n_frames_per_step, dec.n_mels
    W = {'decoder.' + k: v.detach().cpu() for k, v in dec.state_dict().items()}
    memory = torch.randn(B, L, 512, generator=_g(1))
    spk = torch.randn(B, 128, generator=_g(2))
    teacher = torch.rand(B, steps * r, n_mels, generator=_g(3))
    hpo = dict(full_hp(0.5), n_mels=n_mels)

    class Drop64(O.DropoutSource):
        def __call__(self, x, p, training):
            if (not training) or p == 0.0:
                return x
            keep = torch.full(x.shape, 1.0 - p, dtype=torch.float32)
            mk = torch.bernoulli(keep, generator=self.gen) / (1.0 - p)
            self.used.append(mk)
            return x * mk.double()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    torch.set_default_dtype(torch.float64)
    try:
        Wd = {k: v.double().requires_grad_() for k, v in W.items() if v.is_floating_point()}
        mem_r, spk_r, tch_r = memory.double().requires_grad_(), spk.double().requires_grad_(), teacher.double().requires_grad_()
        drop = Drop64('rng', generator=_g(11))
        outs = O.decoder_forward(Wd, mem_r, tch_r, spk_r, hpo, 1.0, None, True, drop, lambda: 0.0)
    finally:
        torch.set_default_dtype(torch.float32)
    douts = [torch.randn(*o.shape, generator=_g(20 + i)) for i, o in enumerate(outs[:3])]
    torch.autograd.backward(list(outs[:3]), [d.double() for d in douts])
    masks = masks_to(split_masks(drop.used, hpo, True, 1.0, B, B, steps, list(range(steps)), hpo['prenet_dim']), dev)
    ref = dict(mel=outs[0].detach(), align=outs[1].detach(), stop=outs[2].detach(), dmem=mem_r.grad, dspk=spk_r.grad, dteacher=tch_r.grad,
               **{k[len('decoder.'):]: v.grad for k, v in Wd.items() if v.grad is not None})
    return dec, dict(memory=memory, spk=spk, teacher=teacher, masks=masks, douts=douts), ref


def run_form(dec, data, dev, form):
    k = dict(dict(fuse=True, overlap=True, parts=2, dsplits=2, qsplits=4), **FORM_KNOBS[form])
    dec.bwd_fuse_pointwise, dec.bwd_overlap_attn, dec.bwd_attn_parts = k['fuse'], k['overlap'], k['parts']
    dec.bwd_dxd_splits, dec.bwd_dxq_splits = k['dsplits'], k['qsplits']
    for p in dec.parameters():
        p.grad = None
    dec._last_bwd_forms = None
    mem, spk = data['memory'].to(dev).requires_grad_(), data['spk'].to(dev).requires_grad_()
    tch = data['teacher'].to(dev).requires_grad_()
    mel, align, stop = dec(mem, None, tch, spk, tf_rate=1.0, _masks=data['masks'])
    torch.autograd.backward([mel, align, stop], [d.to(dev) for d in data['douts']])
    got = dict(mel=mel.detach().cpu(), align=align.detach().cpu(), stop=stop.detach().cpu(), dmem=mem.grad.cpu(), dspk=spk.grad.cpu(),
               dteacher=tch.grad.cpu() if tch.grad is not None else None,
               **{n: p.grad.cpu() for n, p in dec.named_parameters() if p.grad is not None})
    return got


def relerr(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


# relative error (max |err| / max |ref|) of every output and gradient: test_decoder_backward_against_oracle allows 1e-4 at its small dims;
# at the full size the worst measured on an MI355X is 2.1e-6 (gate_layer bias, L = 137), so the bound here is 1e-5
DEC_TOL = 1e-5


def check_against_reference(got, ref, name):
    errs = {}
    for k, r in ref.items():
        if r is None:
            continue
        g = got.get(k)
        if k == 'dteacher' and g is None:      # (only where the decoder gives one)
            continue
        assert g is not None, 'missing gradient / output ' + k
        if float(r.abs().max()) < 1e-9:
            assert float(g.abs().max()) < 1e-4, k
            continue
        errs[k] = relerr(g, r)
    report('attn_bwd_forms', case=name, worst=max(errs.values()), worst_key=max(errs, key=errs.get),
           **{k: v for k, v in errs.items() if k in ('mel', 'align', 'stop', 'dmem', 'dspk', 'dteacher')})
    bad = {k: v for k, v in errs.items() if v >= DEC_TOL}
    assert not bad, bad
    assert len(errs) > 20
    return errs


SHAPES = [  # B, L, steps, forms
    (32, 43, 5, ['six', 'fused', 'overlap', 'split2', 'split4', 'dxd1', 'dxd4', 'dxq1', 'dxq2']),
    (32, T.WIDE_HOSTED_LAST, 4, ['overlap', 'split2', 'split4', 'dxd1', 'dxq2']),
    (32, T.WIDE_HOSTED_LAST + 1, 4, ['overlap', 'split2']),
    (16, 48, 4, ['six', 'split2', 'split4']),
    (20, 49, 4, ['fused', 'split2', 'split4']),
    (33, 97, 4, ['overlap', 'split2', 'split4']),
    (1, 43, 6, ['six', 'split2', 'split4']),
]


@pytest.mark.parametrize('B,L,steps,forms', SHAPES, ids=['B%d_L%d' % (s[0], s[1]) for s in SHAPES])
def test_bptt_forms_against_float64(dev, B, L, steps, forms):
    dec, data, ref = decoder_reference(dev, B, L, steps, seed=4000 + B + L)
    for form in forms:
        got = run_form(dec, data, dev, form)
        assert T.forms_name(dec._last_bwd_forms) == expected_form(form, B, L), (form, hex(dec._last_bwd_forms))
        check_against_reference(got, ref, 'B%d_L%d_%s' % (B, L, form))


@pytest.mark.parametrize('form', ['split4', 'dxq2'])
def test_split_forms_read_nothing_unwritten(dev, form):
    """parts = 4 and the partial query-cell form at L = 137 with every buffer the kernels must write first filled with NaN
    (ops.POISON_UNINIT): bitwise the clean run"""
    from semi_tts_amd import ops
    B, L, steps = 32, T.WIDE_HOSTED_LAST, 4
    from helpers import full_tacotron
    dec = full_tacotron(dev, seed=17, prenet_dropout=0.5).train().decoder
    data = dict(memory=torch.randn(B, L, 512, generator=_g(1)), spk=torch.randn(B, 128, generator=_g(2)),
                teacher=torch.rand(B, steps * dec.n_frames_per_step, dec.n_mels, generator=_g(3)))
    res = {}
    for poison in (False, True):
        old = ops.POISON_UNINIT
        ops.POISON_UNINIT = poison
        try:
            torch.manual_seed(9)                # the same dropout masks in both runs
            dec.bwd_fuse_pointwise = dec.bwd_overlap_attn = True
            k = dict(dict(parts=2, dsplits=2, qsplits=4), **FORM_KNOBS[form])
            dec.bwd_attn_parts, dec.bwd_dxd_splits, dec.bwd_dxq_splits = k['parts'], k['dsplits'], k['qsplits']
            for p in dec.parameters():
                p.grad = None
            mem, spk = data['memory'].to(dev).requires_grad_(), data['spk'].to(dev).requires_grad_()
            mel, align, stop = dec(mem, None, data['teacher'].to(dev), spk, tf_rate=1.0)
            douts = [torch.randn(*o.shape, generator=_g(30 + i)).to(dev) for i, o in enumerate((mel, align, stop))]
            torch.autograd.backward([mel, align, stop], douts)
            assert T.forms_name(dec._last_bwd_forms) == expected_form(form, B, L)
            res[poison] = dict(dmem=mem.grad.clone(), **{n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None})
        finally:
            ops.POISON_UNINIT = old
    for k, v in res[False].items():
        assert torch.isfinite(v).all() and torch.equal(v, res[True][k]), k
