"""Every dispatch path of the GEMM family -- st_gemm_fwd / st_gemm_fwd_batch (gemm.hip) and st_gemm_wgrad[_db|_split] /
st_gemm_wgrad_batch (grad.hip) -- on the rows of gemm_cases.py (test_gemm_dispatch_host.py shows which kernel each row reaches), called
through the C entry points.

  * Exact data: small-integer operands, integer bias / residual and a mask in {0, 2}, chosen so that every partial sum stays below 2^24:
    each fp32 sum is then exact in any order, and the result must equal a float64 reference BITWISE -- split-K, every slab sum,
    accumulation into an integer dW, db, both halves of a split, max-pool.  A dropped, duplicated or misplaced term cannot hide in a
    tolerance.  (Only here the float64 reference runs on the GPU: integer arithmetic is exact there as well.)
  * Random data: normal operands and the forward epilogues (bias, act_pre / act_post, BN, highway, residual, mask) on the tile path and
    on the split-K finish, against float64 on the CPU within a derived per-element bound: fp32 MFMA is a k-ordered fp32 fma chain, so
    |y - y64| <= (n + 2) u sum|a w| with u = 2^-24 and n the length of the chain (KT Cin; the slab length + S with split-K), plus each
    epilogue step's own terms (written next to them).  The measured fraction of the bound goes to helpers.report.
  * Guards: outputs inside sentinel-filled buffers (coff > 0, ldc > coff + N, rows above and below); the columns of A past Cin, the
    columns of dC outside [dcoff, dcoff + N) and the rows after the last utterance hold NaN; the weight-gradient workspace has a
    sentinel tail.  A single +inf in one row of A (of dC) reaches only the outputs that read that row; a second call is bitwise the
    first; the batched entry points equal the separate calls bitwise."""
import ctypes as C
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G   # noqa: E402
from helpers import report   # noqa: E402
from semi_tts_amd import _lib, ops   # noqa: E402
from semi_tts_amd._lib import StGemmEpilogue, StGemmJob, StWgradJob, check   # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.6789
NAN = float('nan')
REF_MACS = 1e8          # CPU float64 references above this many multiply-adds run on a subset of the output rows


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).float()


# ---------------------------------------------------------------- operand buffers
def a_buffer(vals, lda, off, dev):
    """(buffer, pointer) of rows `vals` (R, Cin) with row stride lda, starting `off` floats past the 16-byte aligned base; the columns
    past Cin and two rows after the last one hold NaN"""
    R, Cin = vals.shape
    buf = torch.full((off + (R + 2) * lda + 4,), NAN, device=dev)
    buf[off:off + R * lda].view(R, lda)[:, :Cin] = vals.to(dev)
    return buf, buf.data_ptr() + 4 * off


def w_buffer(c, w3, dev):
    """the weight (N, Cin, KT) in the row's layout -> (buffer, pointer)"""
    t = w3.permute(0, 2, 1) if c['w'] == 'tm' else w3
    t = t.contiguous().reshape(-1)
    off = G.w_offset(c)
    buf = torch.full((t.numel() + 4,), NAN, device=dev)
    buf[off:off + t.numel()] = t.to(dev)
    return buf, buf.data_ptr() + 4 * off


def out_buffer(M, N, dev, coff=4, extra=4, pad_rows=2):
    ldc = coff + N + extra
    buf = torch.full((M + 2 * pad_rows, ldc), SENTINEL, device=dev)
    return buf, buf[pad_rows:pad_rows + M, coff:coff + N], ldc, coff


def row0(out, coff):
    """C of st_gemm_fwd for an output view that starts coff columns into its rows (the kernels write C[m * ldc + coff + n])"""
    return out.data_ptr() - 4 * coff


def guard_intact(buf, view_rows, view_cols, pad_rows=2, coff=4):
    keep = torch.zeros(buf.shape, dtype=torch.bool)
    keep[pad_rows:pad_rows + view_rows, coff:coff + view_cols] = True
    return bool((bits(buf)[~keep] == bits(torch.tensor([SENTINEL]))[0]).all())


def pooled(a3):
    """MaxPool1d(2, stride 1, padding 1)[:T] along time of (Bn, T, C)"""
    p = a3.clone()
    p[:, 1:] = torch.maximum(a3[:, 1:], a3[:, :-1])
    return p


def tap_rows(c, k, rows=None):
    """(utterance, input frame) of output rows `rows` (default all) for tap k, and whether the frame lies in [0, Tin)"""
    M = c['Bn'] * c['Tout']
    m = torch.arange(M) if rows is None else rows
    b, t = m // c['Tout'], m % c['Tout']
    ti = t * c['stride'] + k - c['pad']
    ok = (ti >= 0) & (ti < c['Tin'])
    return b, ti.clamp(0, c['Tin'] - 1), ok


def conv_ref(c, a3, w3, rows=None, absval=False):
    """float64 sum_k sum_ci W[n, ci, k] A'[b, t stride + k - pad, ci] (A' = pooled A when the row pools) on the device of a3;
    absval: sum |a w| instead"""
    a3 = a3.double()
    w3 = w3.double().to(a3.device)
    if c['pool']:
        a3 = pooled(a3)
    if absval:
        a3, w3 = a3.abs(), w3.abs()
    out = None
    for k in range(c['KT']):
        b, ti, ok = tap_rows(c, k, rows)
        x = torch.where(ok.to(a3.device).unsqueeze(1), a3[b.to(a3.device), ti.to(a3.device)], torch.zeros((), dtype=torch.float64, device=a3.device))
        y = x @ w3[:, :, k].t()
        out = y if out is None else out + y
    return out


# ---------------------------------------------------------------- forward
def fwd_call(c, a3, w3, dev, ep_t=None, ep_cfg=None, lib=None):
    """run st_gemm_fwd on the row; -> (output view, its sentinel-filled buffer)"""
    lib = lib or _lib.load()
    Bn, Tin, Cin, N, KT, M = c['Bn'], c['Tin'], c['Cin'], c['N'], c['KT'], c['Bn'] * c['Tout']
    abuf, ap = a_buffer(a3.reshape(Bn * Tin, Cin), G.lda_of(c), G.a_offset(c), dev)
    wbuf, wp = w_buffer(c, w3, dev)
    obuf, out, ldc, coff = out_buffer(M, N, dev)
    ep, keep = epilogue(c, ep_t, ep_cfg, dev)
    check(lib.st_gemm_fwd(ap, G.lda_of(c), wp, row0(out, coff), ldc, coff, Bn, Tin, c['Tout'], Cin, N, KT, c['pad'], c['stride'],
                          1 if c['pool'] else 0, C.byref(ep), ops.stream_handle()), 'st_gemm_fwd')
    torch.cuda.synchronize()
    del abuf, wbuf, keep
    return out, obuf


def epilogue(c, t, cfg, dev):
    """st_gemm_epilogue of the row (w_tap_major, split-K workspace) with the operands in t (dict of device tensors) -> (ep, tensors to
    keep alive)"""
    lib = _lib.load()
    ep = StGemmEpilogue()
    ep.w_tap_major = 1 if c['w'] == 'tm' else 0
    keep = []
    M, N = c['Bn'] * c['Tout'], c['N']
    if c['split']:
        S = int(lib.st_gemm_splitk_slabs(c['Bn'], c['Tout'], c['Cin'], N, c['KT']))
        if S > 1:
            ws = torch.full((S * M * N,), NAN, device=dev)
            keep.append(ws)
            ep.splitk_ws, ep.splitk_slabs = ws.data_ptr(), S
    t = t or {}
    cfg = cfg or {}
    ep.bias = ops._p(t.get('bias'))
    if 'bn' in t:
        mean, var, w, b = t['bn']
        ep.bn_mean, ep.bn_var, ep.bn_w, ep.bn_b = ops._p(mean), ops._p(var), ops._p(w), ops._p(b)
    ep.bn_eps = 1e-5
    ep.act_pre, ep.act_post = ops.ACT[cfg.get('act_pre')], ops.ACT[cfg.get('act_post')]
    for name, fld, ld in (('res', 'res', 'ldres'), ('highway_h', 'highway_h', 'ldhw'), ('mask', 'mask', 'ldmask')):
        if name in t:
            setattr(ep, fld, t[name].data_ptr())
            setattr(ep, ld, int(t[name].stride(0)))
    return ep, keep


def slabs_of(c):
    return (fwd_code(c) >> 8) & 0xff


def fwd_code(c):
    import test_gemm_dispatch_host as H
    return _lib.load().st_gemm_fwd_variant(*(lambda j: (j.A, j.lda, j.W, j.C, j.ldc, j.coff, j.Bn, j.Tin, j.Tout, j.Cin, j.N, j.KT,
                                                         j.pad, j.stride, j.pool_prev, C.byref(j.ep)))(H.fwd_job(c)))


@pytest.mark.parametrize('c', G.FWD, ids=[c['id'] for c in G.FWD])
def test_fwd_exact(dev, c):
    """integer data: the result equals the float64 reference bitwise (bias, residual, mask {0, 2} in the epilogue); the guards keep
    their sentinels; NaN in the columns past Cin and the rows after the last utterance changes nothing; +inf in one row of A reaches
    only the outputs whose tap window covers it"""
    g = gen(zlib.crc32(c['id'].encode()))
    Bn, Tin, Cin, N, KT, M = c['Bn'], c['Tin'], c['Cin'], c['N'], c['KT'], c['Bn'] * c['Tout']
    a3, w3 = ints((Bn, Tin, Cin), 4, g), ints((N, Cin, KT), 4, g)
    t = dict(bias=ints((N,), 8, g).to(dev), res=ints((M, N), 8, g).to(dev), mask=(2 * torch.randint(0, 2, (M, N), generator=g)).float().to(dev))
    assert KT * Cin * 16 + 16 < 2 ** 24
    ref = ((conv_ref(c, a3.to(dev), w3) + t['bias'].double()) + t['res'].double()) * t['mask'].double()
    out, obuf = fwd_call(c, a3, w3, dev, t)
    assert torch.equal(out.double(), ref), 'max |diff| %g' % float((out.double() - ref).abs().max())
    assert guard_intact(obuf, M, N)
    out2, _ = fwd_call(c, a3, w3, dev, t)
    assert same_bits(out, out2), 'second call differs'
    # +inf in the last input row of the last utterance (and the last channel: the K tail)
    a_inf = a3.clone()
    a_inf[Bn - 1, Tin - 1, Cin - 1] = float('inf')
    ref_i = ((conv_ref(c, a_inf.to(dev), w3) + t['bias'].double()) + t['res'].double()) * t['mask'].double()
    got_i, _ = fwd_call(c, a_inf, w3, dev, t)
    fin = torch.isfinite(ref_i)
    assert torch.equal(got_i.double()[fin], ref_i[fin]), 'an output that does not read the +inf row changed'
    assert not torch.isfinite(got_i.double()[~fin]).any(), 'an output that reads the +inf row stayed finite'


EPILOGUES = [
    dict(act_pre='relu', res=True, mask=True),
    dict(bn=True, act_post='relu'),
    dict(act_post='sigmoid', highway=True),
    dict(act_pre='tanh', bn=True, bn_affine=False, res=True),
]


def epilogue_ref(cfg, v, e, t):
    """float64 epilogue of gm_epilogue_vals on v (bias included) and the bound e of |v32 - v| carried through it; t on the CPU"""
    def act(x, e, name):
        if name == 'relu':
            return x.clamp_min(0), e
        if name == 'tanh':            # 1-Lipschitz; tanhf's own error: a few ulp
            y = torch.tanh(x)
            return y, e + 8 * U * y.abs() + 2.0 ** -60
        if name == 'sigmoid':         # Lipschitz 1/4
            y = torch.sigmoid(x)
            return y, 0.25 * e + 8 * U * y.abs()
        return x, e
    v, e = act(v, e, cfg.get('act_pre'))
    if 'bn' in t:
        mean, var, w, b = [q.double() for q in t['bn']]
        s = 1.0 / torch.sqrt(var + 1e-5)
        y = (v - mean) * s * w + b
        # the scale carries the error; four roundings (sub, two mul, add) and rsqrt's ~2 ulp on the terms
        e = e * (s * w).abs() + 8 * U * ((v - mean).abs() * (s * w).abs() + b.abs())
        v = y
    v, e = act(v, e, cfg.get('act_post'))
    if 'highway_h' in t:
        H, x = t['highway_h'].double(), t['res'].double()
        y = H * v + x * (1 - v)
        e = e * (H - x).abs() + 4 * U * ((H * v).abs() + x.abs() + (x * v).abs())
        v = y
    elif 'res' in t:
        v = v + t['res'].double()
        e = e + U * v.abs()
    if 'mask' in t:
        v = v * t['mask'].double()
        e = e * t['mask'].double()
    return v, e


@pytest.mark.parametrize('c', G.FWD, ids=[c['id'] for c in G.FWD])
def test_fwd_random_bound(dev, c):
    """normal operands and one of the epilogue combinations: within the derived bound of a float64 reference on the CPU"""
    i = [q['id'] for q in G.FWD].index(c['id'])
    cfg = EPILOGUES[i % len(EPILOGUES)]
    g = gen(1000 + i)
    Bn, Tin, Cin, N, KT, M = c['Bn'], c['Tin'], c['Cin'], c['N'], c['KT'], c['Bn'] * c['Tout']
    a3, w3 = torch.randn((Bn, Tin, Cin), generator=g), torch.randn((N, Cin, KT), generator=g) / math.sqrt(Cin * KT)
    t = dict(bias=torch.randn(N, generator=g))
    if cfg.get('bn'):
        aff = cfg.get('bn_affine', True)
        t['bn'] = (torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5,
                   torch.randn(N, generator=g) if aff else torch.ones(N), torch.randn(N, generator=g) if aff else torch.zeros(N))
    if cfg.get('res') or cfg.get('highway'):
        t['res'] = torch.randn((M, N), generator=g)
    if cfg.get('highway'):
        t['highway_h'] = torch.randn((M, N), generator=g)
    if cfg.get('mask'):
        t['mask'] = (2 * torch.randint(0, 2, (M, N), generator=g)).float()
    td = {k: (tuple(q.to(dev) for q in v) if isinstance(v, tuple) else v.to(dev)) for k, v in t.items()}
    out, obuf = fwd_call(c, a3, w3, dev, td, cfg)
    assert guard_intact(obuf, M, N)
    rows = None
    if M * N * Cin * KT > REF_MACS:
        rows = torch.randperm(M, generator=g)[:max(1, int(REF_MACS // (N * Cin * KT)))].sort().values
    sel = (lambda x: x) if rows is None else (lambda x: x[rows])
    v = conv_ref(c, a3, w3, rows) + t['bias'].double()
    S = slabs_of(c)
    K = Cin * KT
    n = K if S == 1 else math.ceil(K / S) + S + 32          # (a slab is a whole number of 32- or 16-float blocks: at most 32 more)
    e = (n + 2) * U * (conv_ref(c, a3, w3, rows, absval=True) + t['bias'].double().abs())
    tr = {k: (v_ if k in ('bn', 'bias') else sel(v_)) for k, v_ in t.items()}
    ref, bound = epilogue_ref(cfg, v, e, tr)
    got = sel(out.detach().cpu()).double()
    err = (got - ref).abs()
    frac = float((err / (bound + 1e-300)).max())
    report('gemm_fwd_random/' + c['id'], frac_of_bound=frac, S=S, max_err=float(err.max()))
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), 'max err / bound = %g' % frac
    out2, _ = fwd_call(c, a3, w3, dev, td, cfg)
    assert same_bits(out, out2), 'second call differs'


def batch_jobs(cases, dev, g, exact):
    """operands of each forward row -> (StGemmJob array, outputs, tensors to keep alive)"""
    jobs, outs, keep = [], [], []
    for c in cases:
        Bn, Tin, Cin, N, KT, M = c['Bn'], c['Tin'], c['Cin'], c['N'], c['KT'], c['Bn'] * c['Tout']
        if exact:
            a3, w3 = ints((Bn, Tin, Cin), 4, g), ints((N, Cin, KT), 4, g)
            bias = ints((N,), 8, g).to(dev)
        else:
            a3, w3 = torch.randn((Bn, Tin, Cin), generator=g), torch.randn((N, Cin, KT), generator=g) / math.sqrt(Cin * KT)
            bias = torch.randn(N, generator=g).to(dev)
        abuf, ap = a_buffer(a3.reshape(Bn * Tin, Cin), G.lda_of(c), G.a_offset(c), dev)
        wbuf, wp = w_buffer(c, w3, dev)
        obuf, out, ldc, coff = out_buffer(M, N, dev)
        ep, k = epilogue(c, dict(bias=bias), dict(act_pre=None if exact else 'relu'), dev)
        j = StGemmJob()
        j.A, j.lda, j.W, j.C, j.ldc, j.coff = ap, G.lda_of(c), wp, row0(out, coff), ldc, coff
        j.Bn, j.Tin, j.Tout, j.Cin, j.N, j.KT = Bn, Tin, c['Tout'], Cin, N, KT
        j.pad, j.stride, j.pool_prev, j.ep = c['pad'], c['stride'], 1 if c['pool'] else 0, ep
        jobs.append(j)
        outs.append((out, obuf, a3, w3, bias))
        keep += [abuf, wbuf, k]
    return (StGemmJob * len(jobs))(*jobs), outs, keep


@pytest.mark.parametrize('b', G.FWD_BATCH, ids=[b['id'] for b in G.FWD_BATCH])
def test_fwd_batch_equals_separate_calls(dev, b):
    """st_gemm_fwd_batch (random data, bias + relu) is bitwise the separate st_gemm_fwd calls; on integer data both equal float64"""
    lib = _lib.load()
    cases = b['jobs']
    arr, outs, keep = batch_jobs(cases, dev, gen(7), exact=False)
    check(lib.st_gemm_fwd_batch(arr, len(cases), ops.stream_handle()), 'st_gemm_fwd_batch')
    torch.cuda.synchronize()
    first = [o[0].clone() for o in outs]
    for out, *_ in outs:
        out.fill_(NAN)
    for j in arr:
        check(lib.st_gemm_fwd(j.A, j.lda, j.W, j.C, j.ldc, j.coff, j.Bn, j.Tin, j.Tout, j.Cin, j.N, j.KT, j.pad, j.stride, j.pool_prev,
                              C.byref(j.ep), ops.stream_handle()), 'st_gemm_fwd')
    torch.cuda.synchronize()
    for c, f, (out, obuf, *_) in zip(cases, first, outs):
        assert same_bits(f, out), c['id']
        assert guard_intact(obuf, c['Bn'] * c['Tout'], c['N']), c['id']
    arr, outs, keep = batch_jobs(cases, dev, gen(8), exact=True)
    check(lib.st_gemm_fwd_batch(arr, len(cases), ops.stream_handle()), 'st_gemm_fwd_batch')
    torch.cuda.synchronize()
    for c, (out, obuf, a3, w3, bias) in zip(cases, outs):
        assert torch.equal(out.double(), conv_ref(c, a3.to(dev), w3) + bias.double()), c['id']


# ---------------------------------------------------------------- weight gradient
def wg_operands(c, g, exact):
    M, N, Cin = c['Bn'] * c['Tout'], c['N'], c['Cin']
    if exact:
        return ints((M, N), 4, g), ints((c['Bn'], c['Tin'], Cin), 4, g)
    return torch.randn((M, N), generator=g), torch.randn((c['Bn'], c['Tin'], Cin), generator=g)


def wg_ref(c, dc, a3, ns=None, absval=False):
    """float64 dW (N, Cin, KT) = sum_rows dC[row, n] A'[row + k - pad, ci] and db = column sums of dC, on dc's device; ns: a subset
    of the output rows n"""
    dc = dc.double()
    a3 = a3.double().to(dc.device)
    if c['pool']:
        a3 = pooled(a3)
    if ns is not None:
        dc = dc[:, ns.to(dc.device)]
    if absval:
        dc, a3 = dc.abs(), a3.abs()
    cw = dict(c, stride=1)
    dw = []
    for k in range(c['KT']):
        b, ti, ok = tap_rows(cw, k)
        x = torch.where(ok.to(dc.device).unsqueeze(1), a3[b.to(dc.device), ti.to(dc.device)], torch.zeros((), dtype=torch.float64, device=dc.device))
        dw.append(dc.t() @ x)
    return torch.stack(dw, 2), dc.sum(0)


def wg_call(c, dc, a3, dev, dw_init=None, lib=None, ws_tail=64):
    """the row's C entry point (st_gemm_wgrad / _db / _split) on NaN-guarded operands; -> (dW (N, Cin, KT), db or None, workspace
    tail intact)"""
    lib = lib or _lib.load()
    M, N, Cin, KT = c['Bn'] * c['Tout'], c['N'], c['Cin'], c['KT']
    lddc, dcoff = G.dc_layout(c)
    dc_off = 1 if c['dc'] == 'odd' else 0
    cbuf = torch.full((dc_off + (M + 2) * lddc + 4,), NAN, device=dev)
    cbuf[dc_off:dc_off + M * lddc].view(M, lddc)[:, dcoff:dcoff + N] = dc.to(dev)
    dcp = cbuf.data_ptr() + 4 * dc_off
    lda = G.lda_of(c)
    abuf, ap = a_buffer(a3.reshape(-1, Cin), lda, 0, dev)
    nws = int(lib.st_gemm_wgrad_workspace_floats(c['Bn'], c['Tout'], Cin, N, KT))
    ws = torch.full((nws + ws_tail,), NAN, device=dev)
    ws[nws:] = SENTINEL
    dw = torch.full((N, Cin, KT), NAN, device=dev) if dw_init is None else dw_init.to(dev).clone()
    db = torch.full((N,), NAN, device=dev) if c['db'] else None
    acc = 1 if c['acc'] else 0
    st = ops.stream_handle()
    if c['split']:
        sp = c['split']
        d0 = dw[:, :sp, 0].contiguous()
        d1 = dw[:, sp:, 0].contiguous()
        dbd = torch.full((N,), NAN, device=dev) if c['db'] else None
        check(lib.st_gemm_wgrad_split(dcp, lddc, dcoff, ap, lda, d0.data_ptr(), sp, d1.data_ptr(), ops._p(db), ops._p(dbd), ws.data_ptr(),
                                      M, Cin, N, acc, st), 'st_gemm_wgrad_split')
        torch.cuda.synchronize()
        dw = torch.cat([d0, d1], 1).unsqueeze(2)
        if c['db']:
            assert same_bits(db, dbd), 'db_dup differs from db'
    elif c['db']:
        check(lib.st_gemm_wgrad_db(dcp, lddc, dcoff, ap, lda, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), c['Bn'], c['Tin'], c['Tout'],
                                   Cin, N, KT, c['pad'], 1 if c['pool'] else 0, acc, st), 'st_gemm_wgrad_db')
    else:
        check(lib.st_gemm_wgrad(dcp, lddc, dcoff, ap, lda, dw.data_ptr(), ws.data_ptr(), c['Bn'], c['Tin'], c['Tout'], Cin, N, KT,
                                c['pad'], 1 if c['pool'] else 0, acc, st), 'st_gemm_wgrad')
    torch.cuda.synchronize()
    tail_ok = bool((ws[nws:] == SENTINEL).all())
    return dw, db, tail_ok


@pytest.mark.parametrize('c', G.WGRAD, ids=[c['id'] for c in G.WGRAD])
def test_wgrad_exact(dev, c):
    """integer data: dW (accumulated onto an integer dW where the row says so), db and both halves of a split equal float64 bitwise;
    NaN outside the operands' columns / rows changes nothing; the workspace tail keeps its sentinel; +inf in one row of A (of dC)
    reaches only the (n, ci, tap) entries that read it"""
    g = gen(zlib.crc32(c['id'].encode()))
    M, N, Cin, KT = c['Bn'] * c['Tout'], c['N'], c['Cin'], c['KT']
    dc, a3 = wg_operands(c, g, exact=True)
    assert M * 16 < 2 ** 24
    dw0 = ints((N, Cin, KT), 64, g) if c['acc'] else None
    ref, refb = wg_ref(c, dc.to(dev), a3)
    if dw0 is not None:
        ref = ref + dw0.double().to(dev)
    dw, db, tail_ok = wg_call(c, dc, a3, dev, dw0)
    assert tail_ok, 'workspace tail overwritten'
    assert torch.equal(dw.double(), ref), 'max |diff| %g' % float((dw.double() - ref).nan_to_num(1e30).abs().max())
    if c['db']:
        assert torch.equal(db.double(), refb)
    dw2, db2, _ = wg_call(c, dc, a3, dev, dw0)
    assert same_bits(dw, dw2) and (db is None or same_bits(db, db2)), 'second call differs'
    # +inf in the last frame of the FIRST utterance (the next utterance's tap windows must not see it) and in the last row of dC
    for where in ('a', 'dc'):
        dci, ai = dc.clone(), a3.clone()
        if where == 'a':
            ai[0, c['Tin'] - 1, Cin - 1] = float('inf')
        else:
            dci[M - 1, N - 1] = float('inf')
        ref_i, refb_i = wg_ref(c, dci.to(dev), ai)
        if dw0 is not None:
            ref_i = ref_i + dw0.double().to(dev)
        got_i, gotb_i, _ = wg_call(c, dci, ai, dev, dw0)
        fin = torch.isfinite(ref_i)
        assert torch.equal(got_i.double()[fin], ref_i[fin]), '+inf in %s reached an entry that does not read it' % where
        assert not torch.isfinite(got_i.double()[~fin]).any(), '+inf in %s: an entry that reads it stayed finite' % where
        if c['db']:
            finb = torch.isfinite(refb_i)
            assert torch.equal(gotb_i.double()[finb], refb_i[finb])


@pytest.mark.parametrize('c', G.WGRAD, ids=[c['id'] for c in G.WGRAD])
def test_wgrad_random_bound(dev, c):
    """normal data: within (n + 2) u sum|dC A| of float64 on the CPU, n = the rows of a slab + Z (the slab sum; + 1 for accumulate);
    db within (M + 2) u sum|dC|"""
    i = [q['id'] for q in G.WGRAD].index(c['id'])
    g = gen(2000 + i)
    M, N, Cin, KT = c['Bn'] * c['Tout'], c['N'], c['Cin'], c['KT']
    dc, a3 = wg_operands(c, g, exact=False)
    dw0 = torch.randn((N, Cin, KT), generator=g) if c['acc'] else None
    dw, db, tail_ok = wg_call(c, dc, a3, dev, dw0)
    assert tail_ok
    ns = None
    if M * N * Cin * KT > REF_MACS:
        ns = torch.randperm(N, generator=g)[:max(1, int(REF_MACS // (M * Cin * KT)))].sort().values
    ref, refb = wg_ref(c, dc, a3, ns)
    absr, absb = wg_ref(c, dc, a3, ns, absval=True)
    code = _wg_code(c)
    Z = G.wgrad_z(code)
    if G.wgrad_name(code).startswith('convw_small'):      # a slab = whole 64-row blocks of every Z-th (utterance, block) unit
        n = -(-(c['Bn'] * -(-c['Tout'] // 64)) // Z) * 64 + Z
    else:                                               # a slab = rows_per_z rows (whole 32-row chunks)
        n = -(-M // Z) + 32 + Z
    bound = (n + 2) * U * absr
    got = dw.detach().cpu().double()
    if ns is not None:
        got = got[ns]
    if dw0 is not None:
        d0 = dw0.double() if ns is None else dw0.double()[ns]
        ref = ref + d0
        bound = bound + U * (ref.abs() + d0.abs())
    err = (got - ref).abs()
    frac = float((err / (bound + 1e-300)).max())
    report('gemm_wgrad_random/' + c['id'], frac_of_bound=frac, Z=Z, max_err=float(err.max()))
    assert (err <= bound).all(), 'max err / bound = %g' % frac
    if c['db']:
        gb = db.detach().cpu().double()
        if ns is not None:
            gb = gb[ns]
        assert ((gb - refb).abs() <= (n + 2) * U * absb).all()
    dw2, db2, _ = wg_call(c, dc, a3, dev, dw0)
    assert same_bits(dw, dw2) and (db is None or same_bits(db, db2)), 'second call differs'


def _wg_code(c):
    import test_gemm_dispatch_host as H
    return H.wgrad_variant(c)


@pytest.mark.parametrize('b', G.WGRAD_BATCH, ids=[b['id'] for b in G.WGRAD_BATCH])
def test_wgrad_batch_equals_separate_calls(dev, b):
    """st_gemm_wgrad_batch over > 16 mixed jobs (group launches, single calls in between, Z = 1 jobs, a many-slab job, a group of
    one) is bitwise the separate st_gemm_wgrad[_db] calls on random data, as its comment promises"""
    lib = _lib.load()
    jobs = b['jobs']
    g = gen(9)
    arr = (StWgradJob * len(jobs))()
    keep, outs = [], []
    for q, c in zip(arr, jobs):
        M, N, Cin, KT = c['Bn'] * c['Tout'], c['N'], c['Cin'], c['KT']
        dc, a3 = wg_operands(c, g, exact=False)
        lddc, dcoff = G.dc_layout(c)
        off = 1 if c['dc'] == 'odd' else 0
        cbuf = torch.full((off + (M + 2) * lddc + 4,), NAN, device=dev)
        cbuf[off:off + M * lddc].view(M, lddc)[:, dcoff:dcoff + N] = dc.to(dev)
        abuf, ap = a_buffer(a3.reshape(-1, Cin), G.lda_of(c), 0, dev)
        dw = torch.full((N, Cin, KT), NAN, device=dev)
        db = torch.full((N,), NAN, device=dev) if c['db'] else None
        q.dC, q.lddc, q.dcoff, q.A, q.lda, q.dW, q.db = cbuf.data_ptr() + 4 * off, lddc, dcoff, ap, G.lda_of(c), dw.data_ptr(), ops._p(db)
        q.Bn, q.Tin, q.Tout, q.Cin, q.N, q.KT, q.pad = c['Bn'], c['Tin'], c['Tout'], Cin, N, KT, c['pad']
        keep += [cbuf, abuf]
        outs.append((dw, db))
    nws = int(lib.st_gemm_wgrad_batch_workspace_floats(arr, len(jobs)))
    ws = torch.full((nws + 64,), NAN, device=dev)
    ws[nws:] = SENTINEL
    check(lib.st_gemm_wgrad_batch(arr, len(jobs), ws.data_ptr(), ops.stream_handle()), 'st_gemm_wgrad_batch')
    torch.cuda.synchronize()
    assert bool((ws[nws:] == SENTINEL).all())
    first = [(dw.clone(), None if db is None else db.clone()) for dw, db in outs]
    for q, c, (dw, db), (f, fb) in zip(arr, jobs, outs, first):
        dw.fill_(NAN)
        wsj = torch.full((int(lib.st_gemm_wgrad_workspace_floats(c['Bn'], c['Tout'], c['Cin'], c['N'], c['KT'])),), NAN, device=dev)
        if db is not None:
            db.fill_(NAN)
            check(lib.st_gemm_wgrad_db(q.dC, q.lddc, q.dcoff, q.A, q.lda, q.dW, q.db, wsj.data_ptr(), q.Bn, q.Tin, q.Tout, q.Cin, q.N,
                                       q.KT, q.pad, 0, 0, ops.stream_handle()), 'st_gemm_wgrad_db')
        else:
            check(lib.st_gemm_wgrad(q.dC, q.lddc, q.dcoff, q.A, q.lda, q.dW, wsj.data_ptr(), q.Bn, q.Tin, q.Tout, q.Cin, q.N, q.KT,
                                    q.pad, 0, 0, ops.stream_handle()), 'st_gemm_wgrad')
        torch.cuda.synchronize()
        assert torch.isfinite(dw).all(), c['id']
        assert same_bits(f, dw), '%s: batched dW differs from the single call' % c['id']
        if db is not None:
            assert same_bits(fb, db), '%s: batched db differs from the single call' % c['id']
