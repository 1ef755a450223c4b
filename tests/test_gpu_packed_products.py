"""The forward products on pre-packed operands (skinny_packed.hip) on every dispatch path against float64: the layout kernels against the
P16 / T16 index functions of packed_cases.py bit for bit, every row of its LINEAR / CELL / CELL_PAIR / ATTNPRE tables
(test_packed_dispatch_host.py proves that the rows reach every launch) through the C entry points against the float64 references and
their derived bounds, the paths that must agree bit for bit, and the finite-neighbours contract of include/semitts.h.

Operands are built with the index functions, not with the layout kernels, so a product row does not depend on them.  Every natural
output sits in a sentinel-filled buffer with guard rows and columns, every T16 destination is sentinel-filled outside its logical
elements, every natural input is surrounded by NaN: a write outside the ranges changes a bit pattern that is checked, a read outside
poisons the result."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_cases as PC   # noqa: E402
from helpers import SENTINEL, bits, guard_ok, guarded, inside, report, same_bits   # noqa: E402
from semi_tts_amd import _lib, ops   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD_ROWS = 4        # guard rows of a 2-D operand: 4 * ld floats keep the view's 16-byte alignment whatever ld is
BIG = 3e38          # a finite neighbour: BIG * 0 == 0 exactly, BIG * anything else is seen


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def ids(rows):
    return [c['id'] for c in rows]


def p(t):
    return ops._p(t)


def is_sentinel(t):
    return bits(t) == bits(torch.tensor([SENTINEL]))[0]


def within(got, ref, tol, cap):
    """(ok, worst err / tol): every element of got (CPU) within its derived bound AND within the fixed cap the parity tests have always
    used; an element whose bound is 0 must be exact"""
    err = (got.double() - ref).abs()
    ok = bool(torch.isfinite(got).all()) and bool((err <= tol + 1e-300).all()) and bool((err <= cap).all())
    return ok, (float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0)


class Nat:
    """a natural (rows, cols) array inside a guarded buffer.  way: 'vec' -- ld a multiple of 4 and the view 16-byte aligned; 'ld' -- an
    odd ld; 'ptr' -- ld a multiple of 4, the view one float past a 16-byte boundary"""

    def __init__(self, dev, rows, cols, way='vec', fill=SENTINEL, src=None, ld=None):
        self.rows, self.cols, self.fill = rows, cols, fill
        self.off = 1 if way == 'ptr' else 4
        self.ld = ld if ld is not None else (((cols + 8 + 3) & ~3) | (1 if way == 'ld' else 0))
        self.buf, self.v = guarded(rows, cols, self.ld, dev, pad_rows=PAD_ROWS, off=self.off, fill=fill)
        if src is not None:
            self.v.copy_(src.to(dev))

    def cpu(self):
        return self.v.cpu()

    def guard_ok(self):
        return guard_ok(self.buf, inside(self.rows, self.cols, pad_rows=PAD_ROWS, off=self.off), fill=self.fill)


class Flat:
    """n contiguous floats inside a buffer (16 floats before, 16 after, `off` floats past a 16-byte boundary)"""
    OFF = 16

    def __init__(self, dev, n=None, src=None, fill=NAN, off=0):
        n = src.numel() if src is not None else n
        self.n, self.fill, self.o = n, fill, self.OFF + off
        self.buf = torch.full((n + 2 * self.OFF + off,), fill, device=dev)
        self.v = self.buf[self.o:self.o + n]
        if src is not None:
            self.v.copy_(src.reshape(-1).to(dev))

    def guard_ok(self):
        b, f = bits(self.buf), bits(torch.tensor([self.fill]))[0]
        return bool((b[:self.o] == f).all()) and bool((b[self.o + self.n:] == f).all())


class T16Out:
    """a T16 destination of (B, K) from k-block kb0 of a buffer one k-block wider than it needs, sentinel everywhere"""

    def __init__(self, dev, B, K, kb0=0):
        self.B, self.K, self.kb0, self.stride = B, K, kb0, kb0 + PC.kb16(K) + 1
        self.buf = torch.full((PC.t16_floats(B, self.stride),), SENTINEL, device=dev)
        self.pos = PC.t16_positions(range(B), K, self.stride, kb0)

    def view(self):
        return ops.t16_view(self.buf, self.stride, self.kb0)

    def cpu(self):
        return self.buf.cpu()[self.pos]

    def guard_ok(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool)
        keep[self.pos.reshape(-1)] = False
        return bool(is_sentinel(self.buf)[keep].all())


def x_operand(xs, dev, fill=0.0):
    """(buffer, view, 16 * k-blocks): the segments xs, each from its own k-block, as the view that starts X_KB0 k-blocks into a T16 buffer
    X_KB_EXTRA k-blocks wider; the k-block ranges outside the view hold +-fill (alternating), the pads inside it zero"""
    B = xs[0].shape[0]
    KB = sum(PC.kb16(x.shape[1]) for x in xs)
    stride = PC.X_KB0 + KB + PC.X_KB_EXTRA
    img = torch.zeros((B + 15) // 16, stride, 256, device=dev)
    if fill:
        sign = torch.tensor([1.0, -1.0], device=dev).repeat(128)
        img[:, :PC.X_KB0] = fill * sign
        img[:, PC.X_KB0 + KB:] = -fill * sign
    img = img.reshape(-1)
    kb0 = PC.X_KB0
    b = torch.arange(B, dtype=torch.int64, device=dev)[:, None]
    for x in xs:
        k = torch.arange(x.shape[1], dtype=torch.int64, device=dev)[None, :] + 16 * kb0
        img[PC.t16_index(b, k, stride).reshape(-1)] = x.to(dev).reshape(-1)
        kb0 += PC.kb16(x.shape[1])
    return img, ops.t16_view(img, stride, PC.X_KB0), 16 * KB


def w_operand(w, Ks, dev, lstm_H=0):
    """the P16 image of w (N, sum Ks) with every segment from its own k-block, by the index function"""
    wd, off, ws = w.to(dev), 0, []
    for k in Ks:
        ws.append(wd[:, off:off + k])
        off += k
    return PC.p16_image(ws, w.shape[0], lstm_H)


# ===================================================================================================== layout kernels
def _pack_sources(c, dev, seed):
    g = PC.gen(seed)
    srcs, ws = [], []
    for k in c['ks']:
        w = torch.randn(c['N'], k, generator=g)
        ld = k + c['ld_extra']
        f = Flat(dev, n=c['N'] * ld, off=c['off'])
        f.v.view(c['N'], ld)[:, :k].copy_(w.to(dev))
        srcs.append((f, ld))
        ws.append(w)
    return srcs, ws


def _pack_job_args(c, srcs):
    n = len(c['ks'])
    return ((C.c_void_p * n)(*[p(f.v) for f, _ in srcs]), (C.c_int * n)(*[ld for _, ld in srcs]), (C.c_int * n)(*c['ks']), n)


def _pack_single(c, dev, seed=1):
    srcs, ws = _pack_sources(c, dev, seed)
    out = Flat(dev, n=PC.p16_floats(c['ks'], c['N'], c['lstm_H']))
    warr, ldarr, karr, n = _pack_job_args(c, srcs)
    ops.check(_lib.load().st_pack_weight(warr, ldarr, karr, n, c['N'], c['lstm_H'], p(out.v), ops.stream_handle()), 'st_pack_weight')
    return out, ws


@pytest.mark.parametrize('c', PC.PACK_CASES + [PC.PACK_CAP], ids=ids(PC.PACK_CASES + [PC.PACK_CAP]))
def test_pack_weight_is_the_p16_image(dev, c):
    """st_pack_weight == the index function's image bit for bit, pads zero, nothing outside the image written; the last row is just past
    the grid cap of 8192 workgroups (the grid-stride loop's second pass ends ragged)"""
    out, ws = _pack_single(c, dev)
    ref = PC.p16_image([w.to(dev) for w in ws], c['N'], c['lstm_H'])
    assert lib_sizes_agree(c) and same_bits(out.v, ref) and out.guard_ok()


def lib_sizes_agree(c):
    n = len(c['ks'])
    return int(_lib.load().st_packed_weight_floats((C.c_int * n)(*c['ks']), n, c['N'], c['lstm_H'])) == PC.p16_floats(c['ks'], c['N'], c['lstm_H'])


def test_pack_weight_batch_is_the_single_launches(dev):
    """eight jobs of unequal size in one launch (the first just past the batch launch's cap of 4096 workgroups per job) == the index
    function's images == eight st_pack_weight launches"""
    jobs = (_lib.StPackJob * len(PC.PACK_BATCH))()
    outs, keep = [], []
    for i, c in enumerate(PC.PACK_BATCH):
        srcs, ws = _pack_sources(c, dev, seed=10 + i)
        out = Flat(dev, n=PC.p16_floats(c['ks'], c['N'], c['lstm_H']))
        for s, (f, ld) in enumerate(srcs):
            jobs[i].w[s], jobs[i].ldw[s], jobs[i].k[s] = p(f.v), ld, c['ks'][s]
        jobs[i].nseg, jobs[i].N, jobs[i].lstm_H, jobs[i].packed = len(srcs), c['N'], c['lstm_H'], p(out.v)
        outs.append((out, ws))
        keep.append(srcs)
    ops.check(_lib.load().st_pack_weight_batch(jobs, len(PC.PACK_BATCH), ops.stream_handle()), 'st_pack_weight_batch')
    for i, (c, (out, ws)) in enumerate(zip(PC.PACK_BATCH, outs)):
        assert same_bits(out.v, PC.p16_image([w.to(dev) for w in ws], c['N'], c['lstm_H'])) and out.guard_ok(), c['id']
        single, _ = _pack_single(c, dev, seed=10 + i)
        assert same_bits(single.v, out.v), c['id']


@pytest.mark.parametrize('c', PC.PACK_T_CASES + [PC.PACK_T_CAP], ids=ids(PC.PACK_T_CASES + [PC.PACK_T_CAP]))
def test_pack_weight_t_is_the_p16_image_of_the_transpose(dev, c):
    """st_pack_weight_t == the index function's image of cat(ws, 1).t(), both load branches, segment boundaries that cut a 4-row group,
    and one size just past the grid cap"""
    K, cols = c['K'], c['cols']
    big = torch.randn(K, (sum(cols) + 4 + 3) & ~3, generator=PC.gen(5)).to(dev)       # (a row stride that is a multiple of 4)
    ws, off = [], 0
    for n, strided in zip(cols, c['strided']):
        ws.append(big[:, off:off + n] if strided else big[:, off:off + n].contiguous())
        off += n
    vec = all(w.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0 for w in ws) and all(sum(cols[:i]) % 4 == 0 for i in range(len(cols)))
    assert vec == c['id'].startswith(('vec', 'past'))
    n = len(ws)
    out = Flat(dev, n=PC.p16_floats((K,), sum(cols)))
    ops.check(_lib.load().st_pack_weight_t((C.c_void_p * n)(*[p(w) for w in ws]), (C.c_int * n)(*[int(w.stride(0)) for w in ws]),
                                           (C.c_int * n)(*cols), n, K, p(out.v), ops.stream_handle()), 'st_pack_weight_t')
    ref = PC.p16_image([torch.cat(ws, 1).t().contiguous()], sum(cols))
    assert same_bits(out.v, ref) and out.guard_ok()


@pytest.mark.parametrize('c', PC.TILE_CASES + [PC.TILE_CAP], ids=ids(PC.TILE_CASES + [PC.TILE_CAP]))
def test_tile_rows_is_the_t16_image(dev, c):
    """st_tile_rows into a view inside a wider buffer: the logical elements land where the index function says, the pad columns of the
    view's rows are written as zero, everything else (other k-block ranges, rows past B) is untouched"""
    B, K, kb0 = c['B'], c['K'], c['kb0']
    stride = kb0 + PC.kb16(K) + c['kb_extra']
    x = torch.randn(B, K, generator=PC.gen(7))
    src = Nat(dev, B, K, fill=NAN, src=x, ld=K + c['ld_extra'] + 4)
    dst = Flat(dev, n=PC.t16_floats(B, stride), fill=SENTINEL)
    v = ops.t16_view(dst.v, stride, kb0)
    ops.check(_lib.load().st_tile_rows(p(src.v), src.ld, C.byref(v), B, K, ops.stream_handle()), 'st_tile_rows')
    got = dst.v.cpu()
    pos = PC.t16_positions(range(B), K, stride, kb0)
    assert same_bits(got[pos], x) and dst.guard_ok()
    pads = PC.t16_positions(range(B), 16 * PC.kb16(K), stride, kb0)[:, K:].reshape(-1)      # columns K.. of the last k-block, rows < B
    assert bool((bits(got[pads]) == 0).all())
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[pos.reshape(-1)] = False
    keep[pads] = False
    assert bool(is_sentinel(got)[keep].all())


@pytest.mark.parametrize('c', PC.UNTILE_CASES + [PC.UNTILE_VEC_CAP, PC.UNTILE_CAP], ids=ids(PC.UNTILE_CASES + [PC.UNTILE_VEC_CAP, PC.UNTILE_CAP]))
def test_untile_rows_reads_the_t16_image(dev, c):
    """st_untile_rows (both kernels: 16-byte pieces when ld % 4 == 0, element-wise otherwise) from a view inside a wider buffer whose every
    other float is NaN -- pad columns, rows past B and the other k-block ranges; rows past B and columns past K of the destination are
    untouched"""
    B, K, kb0 = c['B'], c['K'], c['kb0']
    stride = kb0 + PC.kb16(K) + c['kb_extra']
    x = torch.randn(B, K, generator=PC.gen(8)).to(dev)
    src = PC.t16_image(x, stride, kb0, fill=NAN)
    ld = K + c['ld_extra']
    assert (ld % 4 == 0) == PC.untile_is_vec(c)
    dst = torch.full((B + 2, ld), NAN, device=dev)
    v = ops.t16_view(src, stride, kb0)
    ops.check(_lib.load().st_untile_rows(C.byref(v), p(dst), ld, B, K, ops.stream_handle()), 'st_untile_rows')
    assert same_bits(dst[:B, :K], x)
    assert bool(torch.isnan(dst[B:]).all()) and bool(torch.isnan(dst[:B, K:]).all())


# ===================================================================================================== linear
def run_linear(c, dev, fill=0.0, seed=0, pre=None, part=None):
    """one row through st_skinny_linear_packed_fwd (pre: through st_skinny_linear_packed_attnpre_fwd with that attention job)
    -> (outputs on the CPU {'y', 't16', 'y2', 'y3'}, all guards intact, the float64 reference)"""
    e, B, N = c['epi'], c['B'], c['N']
    xs, w, bias, mask, mask2 = PC.linear_operands(c, seed)
    ref = PC.linear_ref(c, xs, w, bias, mask, mask2)
    xbuf, xv, Kpad = x_operand(xs, dev, fill)
    packed = w_operand(w, c['Ks'], dev)
    n_split, rep = e['split'] if e['split'] else (0, 0)
    n_split2 = e['third'][0] if e['third'] else 0
    lim = ref['plain'][0].shape[1]
    y = Nat(dev, B, lim, e['y_way']) if e['out'] != 't16' else None
    t16 = T16Out(dev, B, lim, e['ydst_kb0']) if e['out'] != 'y' else None
    y2 = Nat(dev, B, ref['y2'][0].shape[1], 'ld') if n_split else None
    y3 = T16Out(dev, B, N - n_split2, 1) if n_split2 else None
    m1 = Nat(dev, B, N, 'ld', fill=NAN, src=mask) if e['mask'] else None
    m2 = Nat(dev, B, N - n_split2, 'ld', fill=NAN, src=mask2[:, :N - n_split2]) if (n_split2 and e['third'][2]) else None
    bd = Flat(dev, src=bias) if e['bias'] else None
    job = ops.packed_linear_job(packed, xv, Kpad, B, N, y=y.v if y else None, y_dst=t16.view() if t16 else None, bias=bd.v if bd else None,
                                act=None if e['act'] == 'none' else e['act'], mask=m1.v if m1 else None, n_split=n_split,
                                y2=y2.v if y2 else None, rep=rep, n_split2=n_split2, act2=e['third'][1] if n_split2 else None,
                                mask2=m2.v if m2 else None, y3_dst=y3.view() if y3 else None)
    if pre is None:
        ops.check(_lib.load().st_skinny_linear_packed_fwd(C.byref(job), ops.stream_handle()), 'st_skinny_linear_packed_fwd')
    else:
        ops.skinny_linear_packed_attnpre(job, pre, part)
    out = dict(y=y.cpu() if y else None, t16=t16.cpu() if t16 else None, y2=y2.cpu() if y2 else None, y3=y3.cpu() if y3 else None)
    guards = all(o.guard_ok() for o in (y, t16, y2, y3) if o is not None)
    return out, guards, ref


def check_linear(c, out, guards, ref, what):
    worst = 0.0
    for key, rk in (('y', 'plain'), ('t16', 'plain'), ('y2', 'y2'), ('y3', 'y3')):
        if out[key] is None:
            continue
        ok, ratio = within(out[key], ref[rk][0], ref[rk][1], PC.LINEAR_CAP)
        worst = max(worst, ratio)
        assert ok, (c['id'], key, ratio)
    report(what, id=c['id'], worst_err_over_tol=worst)
    if out['y'] is not None and out['t16'] is not None:
        assert same_bits(out['y'], out['t16']), c['id']
    if out['y2'] is not None and c['epi']['split'][1] > 1:       # the `rep` copies of a column are one value
        rep = c['epi']['split'][1]
        copies = out['y2'].view(c['B'], -1, rep)
        assert same_bits(copies, copies[:, :, :1].expand(-1, -1, rep).contiguous()), c['id']
    assert guards, c['id']
    assert worst <= 1.0


@pytest.mark.parametrize('c', PC.LINEAR, ids=ids(PC.LINEAR))
def test_linear_against_float64(dev, c):
    """every LINEAR row: err <= 2 (16 KB + KW + 3) U (sum |x| |w| + |bias|), carried through the activations and masks (packed_cases.py),
    and <= the fixed 2e-5 of test_skinny_linear_packed; y, y_dst, y2 and y3_dst agree; nothing outside the written ranges changes"""
    out, guards, ref = run_linear(c, dev)
    check_linear(c, out, guards, ref, 'packed_linear')


NEIGHBOUR_ROWS = [c for c in PC.LINEAR if c['want'][1] > 1 and sum(PC.kb16(k) for k in c['Ks']) % 16]


@pytest.mark.parametrize('c', NEIGHBOUR_ROWS, ids=ids(NEIGHBOUR_ROWS))
def test_linear_finite_neighbours_do_not_leak(dev, c):
    """more than one batch tile per workgroup and a k-block count that is no multiple of 16: the loads of the last group run on into the
    k-blocks that follow the view (for every batch tile but the last of the span) against weight blocks that read as zero -- the outputs
    are the same bit for bit whether those k-blocks hold zeros or +-3e38"""
    a, ga, _ = run_linear(c, dev, fill=0.0)
    b, gb, _ = run_linear(c, dev, fill=BIG)
    assert ga and gb
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or same_bits(a[k], b[k])), (c['id'], k)


# ===================================================================================================== LSTM cell
def cell_job(c, dev, fill=0.0, seed=0, o=None, part=None, k_lead=None):
    """the StLstmCellPackedJob of a CELL row with every output guarded -> (job, outputs, float64 reference, keep-alive list)"""
    B, H, ab, de = c['B'], c['H'], c['absent'], c['dests']
    o = o or PC.cell_operands(c, seed)
    bi, bh = (None, None) if 'bias' in ab else (o['b_ih'], o['b_hh'])
    cp, mk = (None if 'c_prev' in ab else o['c_prev']), (None if 'mask' in ab else o['mask'])
    ada = 'adain' in de
    ref = PC.cell_ref(o['xs'], o['w'], bi, bh, cp, mk, o['std'] if ada else None, o['mean'] if ada else None)
    xbuf, xv, Kpad = x_operand(o['xs'], dev, fill)
    packed = w_operand(o['w'], c['Ks'], dev, lstm_H=H)
    ex = 5 if c['wide_ld'] else 0
    c_out = Nat(dev, B, H, 'ld' if ex else 'vec')
    cpd = Nat(dev, B, H, fill=NAN, src=cp, ld=H + 4 + ex + 3) if cp is not None else None
    outs = dict(c=c_out, h=T16Out(dev, B, H), h1=T16Out(dev, B, H, 2) if 'h_dst1' in de else None,
                adain=T16Out(dev, B, H, 1) if ada else None, gates=Flat(dev, n=B * 4 * H, fill=SENTINEL) if 'gates' in de else None)
    ins = [Flat(dev, src=t) if t is not None else None for t in (bi, bh, mk, o['std'] if ada else None, o['mean'] if ada else None)]
    v = lambda f: f.v if f is not None else None
    job = ops.lstm_cell_job(packed, xv, Kpad if k_lead is None else k_lead, v(ins[0]), v(ins[1]), cpd.v if cpd else None, outs['h'].view(), c_out.v,
                            B, H, h_dst1=outs['h1'].view() if outs['h1'] else None, mask=v(ins[2]), gates_out=v(outs['gates']),
                            ada_std=v(ins[3]), ada_mean=v(ins[4]), hadapt_dst=outs['adain'].view() if ada else None,
                            part=part, w_kbs=Kpad // 16 if part is not None else 0)
    job.ldc = c_out.ld
    job.ldc_prev = cpd.ld if cpd else H
    return job, outs, ref, [xbuf, packed, cpd, ins]


def cell_outputs(c, outs):
    got = dict(c=outs['c'].cpu(), h=outs['h'].cpu(), h1=outs['h1'].cpu() if outs['h1'] else None,
               adain=outs['adain'].cpu() if outs['adain'] else None,
               gates=outs['gates'].v.cpu().view(c['B'], 4, c['H']) if outs['gates'] else None)
    return got, all(o.guard_ok() for o in outs.values() if o is not None)


def check_cell(c, got, guards, ref, what):
    worst = 0.0
    for key, rk in (('c', 'c'), ('h', 'h'), ('gates', 'gates'), ('adain', 'adain')):
        if got[key] is None:
            continue
        ok, ratio = within(got[key], ref[rk][0], ref[rk][1], PC.CELL_CAP)
        worst = max(worst, ratio)
        assert ok, (c['id'], key, ratio)
    report(what, id=c['id'], worst_err_over_tol=worst)
    if got['h1'] is not None:
        assert same_bits(got['h1'], got['h']), c['id']
    assert guards, c['id']
    assert worst <= 1.0


def run_cell(c, dev, fill=0.0, seed=0):
    job, outs, ref, keep = cell_job(c, dev, fill, seed)
    ops.check(_lib.load().st_lstm_cell_packed_fwd(C.byref(job), ops.stream_handle()), 'st_lstm_cell_packed_fwd')
    got, guards = cell_outputs(c, outs)
    return got, guards, ref


@pytest.mark.parametrize('c', PC.CELL, ids=ids(PC.CELL))
def test_cell_against_float64(dev, c):
    """every CELL row: c, h, the activated gates and the AdaIN output within the bound of cell_ref (the pre-activation bound of the linear
    through the gates, E_FAST for the hardware exp2 / rcp forms) and within the fixed 1e-5 of test_lstm_cell_packed; both h destinations agree; absent operands and destinations; ldc / ldc_prev > H"""
    got, guards, ref = run_cell(c, dev)
    check_cell(c, got, guards, ref, 'packed_cell')


CELL_NEIGHBOUR_ROWS = [c for c in PC.CELL if c['want'][1] > 1 and sum(PC.kb16(k) for k in c['Ks']) % 16 and '_all' in c['id']]


@pytest.mark.parametrize('c', CELL_NEIGHBOUR_ROWS, ids=ids(CELL_NEIGHBOUR_ROWS))
def test_cell_finite_neighbours_do_not_leak(dev, c):
    """the neighbour contract for the cell (pk_body<0, 2..4> and the 2-D tiled cell with two batch tiles per workgroup)"""
    a, ga, _ = run_cell(c, dev, fill=0.0)
    b, gb, _ = run_cell(c, dev, fill=BIG)
    assert ga and gb
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or same_bits(a[k], b[k])), (c['id'], k)


@pytest.mark.parametrize('c', PC.CELL_PAIR, ids=ids(PC.CELL_PAIR))
def test_cell_pair_is_two_single_launches(dev, c):
    """st_lstm_cell_packed_pair_fwd (one launch for two 2-D tiled cells, or its fall-back) == st_lstm_cell_packed_fwd per job, bit for
    bit, and within the bound"""
    lib = _lib.load()
    pair = [cell_job(j, dev, seed=20 + i) for i, j in enumerate(c['jobs'])]
    ops.check(lib.st_lstm_cell_packed_pair_fwd(C.byref(pair[0][0]), C.byref(pair[1][0]), ops.stream_handle()), 'st_lstm_cell_packed_pair_fwd')
    for i, j in enumerate(c['jobs']):
        got, guards = cell_outputs(j, pair[i][1])
        check_cell(dict(j, id=c['id'] + '.' + j['id']), got, guards, pair[i][2], 'packed_cell_pair')
        single, g1, _ = run_cell(j, dev, seed=20 + i)
        assert g1
        for k in got:
            assert (got[k] is None) == (single[k] is None) and (got[k] is None or same_bits(got[k], single[k])), (c['id'], i, k)


def test_fast_gate_functions_error(dev):
    """st_sigmoid_fast / st_tanh_fast through the cell's gates_out: x = 0 and W = 0 make the pre-activations the biases exactly.  Swept
    through [-30, 30] at a spacing below 1e-3 (three interleaved sweeps for the three sigmoid gates), plus +-100, +-inf, +-0 and +-1e-6.
    The measured maxima are reported (DESIGN.md holds them); the bound the cell tests use, E_FAST = 4 x the measured maximum, must hold,
    and the functions saturate to exactly 0, 1 and +-1"""
    H = 1 << 16
    special = torch.tensor([100.0, -100.0, float('inf'), -float('inf'), 0.0, -0.0, 1e-6, -1e-6])
    z = torch.cat([special, torch.linspace(-30, 30, H - special.numel())])
    step = 60.0 / (H - special.numel() - 1)
    bias = torch.stack([z, z, z, z])
    bias[1, special.numel():] += step / 3
    bias[3, special.numel():] += 2 * step / 3
    xbuf = torch.zeros(PC.t16_floats(1, 1), device=dev)
    packed = torch.zeros(PC.p16_floats((16,), 4 * H, H), device=dev)
    bd = bias.reshape(-1).to(dev)
    h, c_out, gates = T16Out(dev, 1, H), torch.empty(1, H, device=dev), torch.empty(1, 4, H, device=dev)
    ops.lstm_cell_packed(packed, ops.t16_view(xbuf, 1, 0), 16, bd, None, None, h.view(), c_out, 1, H, gates_out=gates)
    g = gates[0].cpu()
    assert bool(torch.isfinite(g).all())
    zd = bias.double()
    ref = torch.stack([torch.sigmoid(zd[0]), torch.sigmoid(zd[1]), torch.tanh(zd[2]), torch.sigmoid(zd[3])])
    err = (g.double() - ref).abs()
    e_sig, e_tanh = float(err[[0, 1, 3]].max()), float(err[2].max())
    report('packed_fast_gates', e_sigmoid=e_sig, e_tanh=e_tanh, e_fast=PC.E_FAST, z_sigmoid=float(zd[[0, 1, 3]].reshape(-1)[err[[0, 1, 3]].argmax()]),
           z_tanh=float(zd[2][err[2].argmax()]))
    print('st_sigmoid_fast max |err| %.3e, st_tanh_fast max |err| %.3e' % (e_sig, e_tanh))
    assert max(e_sig, e_tanh) <= PC.E_FAST
    ns = special.numel()
    for row in (0, 1, 3):
        assert g[row, :ns].tolist()[:6] == [1.0, 0.0, 1.0, 0.0, 0.5, 0.5]
    assert g[2, :6].tolist() == [1.0, -1.0, 1.0, -1.0, 0.0, 0.0]       # (the product's +0 plus a bias of -0 is +0)
    # c = i g and h = o tanh(c) of the same launch stay finite and within the same bound
    c_ref = ref[0] * ref[2]
    assert float((c_out[0].cpu().double() - c_ref).abs().max()) <= 2 * PC.E_FAST + 2 * PC.U
    assert float((h.cpu()[0].double() - ref[3] * torch.tanh(c_ref)).abs().max()) <= 4 * PC.E_FAST + 4 * PC.U


# ===================================================================================================== linear + attention pre
def _at_inputs(c, dev, seed=3):
    o = PC.attnpre_operands(c, seed)
    return {k: t.to(dev).contiguous() for k, t in o.items()}


@pytest.mark.parametrize('c', [c for c in PC.ATTNPRE if not c['part']], ids=ids([c for c in PC.ATTNPRE if not c['part']]))
def test_linear_with_attention_pre(dev, c):
    """st_skinny_linear_packed_attnpre_fwd with 1..4 batch tiles per linear workgroup and both attention kernels: S equals ops.attn_pre on
    the same inputs bit for bit, the linear part equals st_skinny_linear_packed_fwd alone bit for bit and is within its bound"""
    d = _at_inputs(c, dev)
    s_buf = torch.full((c['B'], PC.AT_L, c['A']), NAN, device=dev)
    pre = ops.attn_pre_job(d['pm'], d['w_prev'], d['w_cum'], d['loc_conv_w'], d['loc_lin_w'], s_buf, c['parts'])
    out, guards, ref = run_linear(c, dev, pre=pre)
    check_linear(c, out, guards, ref, 'packed_linear_attnpre')
    alone, g1, _ = run_linear(c, dev)
    assert g1 and all(alone[k] is None or same_bits(alone[k], out[k]) for k in alone)
    assert same_bits(s_buf, ops.attn_pre(d['pm'], d['w_prev'], d['w_cum'], d['loc_conv_w'], d['loc_lin_w'], parts=c['parts']))


@pytest.mark.parametrize('c', [c for c in PC.ATTNPRE if c['part']], ids=ids([c for c in PC.ATTNPRE if c['part']]))
def test_linear_with_attention_pre_and_hosted_partial_product(dev, c):
    """... with the partial gate product of a cell behind the attention workgroups: the slab over the cell's k-blocks 1.. and then the
    cell over its leading k-block plus the slab == the whole cell within the cell bound; the slab == st_partial_product_fwd alone"""
    B, H, Ks, k0 = c['B'], PC.PART_H, PC.PART_KS, PC.PART_K0
    cc = dict(id=c['id'] + '.cell', B=B, H=H, Ks=Ks, absent=frozenset(), dests=frozenset(('gates',)), wide_ld=False, saturate=False)
    o = PC.cell_operands(cc, seed=9)
    xbuf, xv, Kpad = x_operand(o['xs'], dev)
    packed = w_operand(o['w'], Ks, dev, lstm_H=H)
    w_kbs = len(Ks)
    slab, slab1 = torch.full((B, 4 * H), NAN, device=dev), torch.full((B, 4 * H), NAN, device=dev)
    xv_part = ops.t16_view(xbuf, xv.kb_stride, xv.kb0 + k0)
    pj = _lib.StPartialProductJob(packed_w=p(packed), w_kbs=w_kbs, kb0=k0, KB=w_kbs - k0, x=xv_part, N=4 * H, part=p(slab))
    d = _at_inputs(c, dev)
    s_buf = torch.full((B, PC.AT_L, c['A']), NAN, device=dev)
    pre = ops.attn_pre_job(d['pm'], d['w_prev'], d['w_cum'], d['loc_conv_w'], d['loc_lin_w'], s_buf, c['parts'])
    out, guards, ref = run_linear(c, dev, pre=pre, part=pj)
    check_linear(c, out, guards, ref, 'packed_linear_attnpre_part')
    alone, g1, _ = run_linear(c, dev)
    assert g1 and all(alone[k] is None or same_bits(alone[k], out[k]) for k in alone)
    assert same_bits(s_buf, ops.attn_pre(d['pm'], d['w_prev'], d['w_cum'], d['loc_conv_w'], d['loc_lin_w'], parts=c['parts']))
    ops.partial_product(packed, w_kbs, k0, w_kbs - k0, xv_part, 4 * H, slab1, B)
    assert same_bits(slab, slab1) and bool(torch.isfinite(slab).all())
    job, outs, cref, keep = cell_job(cc, dev, o=o, part=slab, k_lead=16 * k0)
    ops.check(_lib.load().st_lstm_cell_packed_fwd(C.byref(job), ops.stream_handle()), 'st_lstm_cell_packed_fwd')
    got, gc = cell_outputs(cc, outs)
    check_cell(cc, got, gc, cref, 'packed_cell_hosted_part')


# ===================================================================================================== repeatability
def test_one_row_per_family_twice_is_bitwise_equal(dev):
    for c in (PC.LINEAR[-1], next(c for c in PC.LINEAR if c['id'].startswith('L7') and c['Ks'] != (16,))):
        a, _, _ = run_linear(c, dev)
        b, _, _ = run_linear(c, dev)
        assert all(a[k] is None or same_bits(a[k], b[k]) for k in a), c['id']
    for c in (next(c for c in PC.CELL if c['id'].startswith('C5')), next(c for c in PC.CELL if c['id'].startswith('C7'))):
        a, _, _ = run_cell(c, dev)
        b, _, _ = run_cell(c, dev)
        assert all(a[k] is None or same_bits(a[k], b[k]) for k in a), c['id']
    c = PC.CELL_PAIR[0]
    runs = []
    for _ in range(2):
        pair = [cell_job(j, dev, seed=20 + i) for i, j in enumerate(c['jobs'])]
        ops.check(_lib.load().st_lstm_cell_packed_pair_fwd(C.byref(pair[0][0]), C.byref(pair[1][0]), ops.stream_handle()), 'pair')
        runs.append([cell_outputs(j, pair[i][1])[0] for i, j in enumerate(c['jobs'])])
    for g0, g1 in zip(*runs):
        assert all(g0[k] is None or same_bits(g0[k], g1[k]) for k in g0)
    c = next(c for c in PC.ATTNPRE if c['id'].startswith('A6'))
    d = _at_inputs(c, dev)
    res = []
    for _ in range(2):
        s_buf = torch.full((c['B'], PC.AT_L, c['A']), NAN, device=dev)
        pre = ops.attn_pre_job(d['pm'], d['w_prev'], d['w_cum'], d['loc_conv_w'], d['loc_lin_w'], s_buf, c['parts'])
        out, _, _ = run_linear(c, dev, pre=pre)
        res.append((out, s_buf))
    assert same_bits(res[0][1], res[1][1]) and all(res[0][0][k] is None or same_bits(res[0][0][k], res[1][0][k]) for k in res[0][0])
