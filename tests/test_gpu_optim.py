"""The multi-tensor optimiser kernels (optim.hip: gradient norm, clip scale, Adam, multi-tensor copy) and FusedAdam at every edge, against
float64 with derived bounds (optim_cases.py).  Needs a real MI355X: pytest -m gpu

Operands are views at every alignment inside flat NaN-filled buffers; whatever lies outside the views must still be that NaN, bit for
bit, after every pass.  The same data at another alignment must give the same bits (the 16-byte loops and the float-by-float loops add
and round alike), the table form and the kernel-argument form (a stream capture) must give the same bits, and the error against float64
must stay inside 2 x adam_bound / norm_bound.  Measured error / bound ratios go to parity_report.jsonl."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as OC   # noqa: E402
from helpers import U, bits, report, same_bits   # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float('nan')
NAN_BITS = int(bits(torch.tensor([NAN]))[0])
SCALARS = [(1, 1e-3), (2, 1e-3), (10000, 1e-3), (1, 1.0), (2, 1.0), (10000, 1.0)]      # (step, lr)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ operands and calls
class Placed:
    """tensors as views inside one flat NaN-filled device buffer: view i starts offs[i] floats past a 16-byte boundary, at least four
    NaN floats lie before the first, between two, and after the last"""

    def __init__(self, dev, datas, offs):
        self.spans, cur = [], 0
        for d, off in zip(datas, offs):
            cur = (cur + 3) // 4 * 4 + 4 + off
            self.spans.append((cur, cur + d.numel()))
            cur += d.numel()
        host = torch.full(((cur + 3) // 4 * 4 + 8,), NAN)
        self.outside = torch.ones(host.numel(), dtype=torch.bool)
        for (a, b), d in zip(self.spans, datas):
            host[a:b] = d.reshape(-1)
            self.outside[a:b] = False
        self.init = host.to(dev)
        self.flat = self.init.clone()
        self.views = [self.flat[a:b] for a, b in self.spans]
        assert self.flat.data_ptr() % 16 == 0
        assert all(v.data_ptr() % 16 == 4 * off for v, off, d in zip(self.views, offs, datas) if d.numel())

    def reset(self):
        self.flat.copy_(self.init)

    def guards_ok(self):
        return bool((bits(self.flat)[self.outside] == NAN_BITS).all())

    def cpu(self):
        f = self.flat.cpu()
        return [f[a:b] for a, b in self.spans]


def tabs(ts):
    n = len(ts)
    return (C.c_void_p * n)(*[t.data_ptr() for t in ts]), (C.c_long * n)(*[t.numel() for t in ts])


class MT:
    """the st_mt_* entry points through _lib on torch's current stream (or the capture stream)"""

    def __init__(self, dev):
        from semi_tts_amd import _lib, ops
        self.lib, self._lib, self.ops, self.dev = _lib.load(), _lib, ops, dev

    def misses(self):
        return int(self.lib.st_mt_table_misses())

    def norm_ws(self, gs):
        return (torch.empty(max(1, OC.blocks([g.numel() for g in gs])), device=self.dev), torch.empty((), device=self.dev))

    def norm(self, gs, pre=1.0, ws=None):
        partials, out = ws if ws is not None else self.norm_ws(gs)
        ptrs, sizes = tabs(gs)
        self._lib.check(self.lib.st_mt_grad_norm_scaled(ptrs, sizes, len(gs), partials.data_ptr(), out.data_ptr(), float(pre),
                                                        self.ops.stream_handle()), 'st_mt_grad_norm_scaled')
        return out

    def clip(self, gs, norm, max_norm, pre=1.0):
        ptrs, sizes = tabs(gs)
        self._lib.check(self.lib.st_mt_clip_scale_pre(ptrs, sizes, len(gs), norm.data_ptr(), float(max_norm), float(pre),
                                                      self.ops.stream_handle()), 'st_mt_clip_scale_pre')

    def adam(self, ps, gs, ms, vs, sc, guard=None):
        (pp, sizes), (gp, _), (mp, _), (vp, _) = tabs(ps), tabs(gs), tabs(ms), tabs(vs)
        b1, b2, eps, step_size, bc2 = sc
        if guard is None:
            rc = self.lib.st_mt_adam(pp, gp, mp, vp, sizes, len(ps), b1, b2, eps, step_size, bc2, self.ops.stream_handle())
        else:
            rc = self.lib.st_mt_adam_guarded(pp, gp, mp, vp, sizes, len(ps), b1, b2, eps, step_size, bc2, guard.data_ptr(),
                                             self.ops.stream_handle())
        self._lib.check(rc, 'st_mt_adam')

    def captured(self, fn):
        """fn's launches in their kernel-argument form: recorded into a hipGraph (no table can be made during a capture) and replayed"""
        gr = self.ops.Graph()
        before = self.misses()
        with gr.capture():
            fn()
        assert self.misses() == before                 # (no table during the capture)
        gr.launch()
        torch.cuda.synchronize()


@pytest.fixture(scope='module')
def mt(dev):
    return MT(dev)


def scalar(dev, x):
    return torch.tensor(x, dtype=torch.float32, device=dev)


def grad_data(seed=11, sizes=OC.SIZES):
    """one gradient per size, of scales 1e-3 ... 1e2"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * 10.0 ** (i % 6 - 3) for i, n in enumerate(sizes)]


_ADAM_DATA = {}


def adam_data(seed=31):
    """(p, g, m, v) lists over OC.SIZES, made once"""
    if seed not in _ADAM_DATA:
        _ADAM_DATA[seed] = list(zip(*[OC.adam_operands(n, seed + i) for i, n in enumerate(OC.SIZES)]))
    return _ADAM_DATA[seed]


def within(got, ref, bound):
    """max of |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf)"""
    err = (got.detach().cpu().double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ gradient norm
def test_norm_every_size_at_every_alignment(dev, mt):
    """every size x offset as a one-tensor list: inside norm_bound of float64, the offset copies bitwise the aligned one (the
    float-by-float loop adds in the 16-byte loop's order), twice the same bits, with pre_scale; then ragged lists of all of them.
    The sizes are the table's and the norm's own (OC.NORM_EXTRA_ROWS: every thread through an 8-, a 2- and a 1-piece round and a tail)"""
    sizes = OC.NORM_SIZES
    datas = grad_data(sizes=sizes)
    placed = [Placed(dev, datas, [off] * len(datas)) for off in OC.OFFSETS]
    runs = {}
    for pre in (1.0, 0.25, 1.0 / 3.0):
        for rep in range(2 if pre == 1.0 else 1):
            runs[pre, rep] = torch.stack([torch.stack([mt.norm([v], pre) for v in pl.views]) for pl in placed]).cpu()
    assert same_bits(runs[1.0, 0], runs[1.0, 1])
    worst = 0.0
    for pre in (1.0, 0.25, 1.0 / 3.0):
        got = runs[pre, 0]
        for k in range(1, len(OC.OFFSETS)):
            assert same_bits(got[0], got[k]), (pre, OC.OFFSETS[k], [n for n, a, b in zip(sizes, bits(got[0]), bits(got[k])) if a != b])
        for i, (n, d) in enumerate(zip(sizes, datas)):
            # the fixed order itself: every addition of the kernel restated in numpy float32 gives the device's bits (even pieces of
            # a thread into one running sum, odd into the other, in every loop round alike)
            assert same_bits(got[0, i], torch.tensor(OC.norm_emulate_f32([d], pre))), (n, pre)
            ref = OC.norm_ref([d], pre)
            r = abs(float(got[0, i]) - ref) / (OC.norm_bound(OC.blocks([n]), scaled=pre != 1.0) * ref)
            worst = max(worst, r)
            assert r <= 1.0, (n, pre, r)
    # ragged lists: all sizes at one alignment (the four agree bit for bit), and all 96 views in one list
    ragged = torch.stack([mt.norm(pl.views) for pl in placed]).cpu()
    assert all(same_bits(ragged[0], ragged[k]) for k in range(1, 4))
    assert same_bits(ragged[0], torch.tensor(OC.norm_emulate_f32(datas)))
    nb = OC.blocks(sizes)
    r = abs(float(ragged[0]) - OC.norm_ref(datas)) / (OC.norm_bound(nb) * OC.norm_ref(datas))
    every = [v for pl in placed for v in pl.views]
    for pre in (1.0, 0.25, 1.0 / 3.0):
        a, b = mt.norm(every, pre), mt.norm(every, pre)
        ref = OC.norm_ref(datas * 4, pre)
        r = max(r, abs(float(a) - ref) / (OC.norm_bound(4 * nb, scaled=pre != 1.0) * ref))
        assert same_bits(a, b)
    report('mt_norm_sizes_offsets', norm_ratio_one_tensor=worst, norm_ratio_ragged=r)
    assert r <= 1.0
    assert all(pl.guards_ok() and same_bits(pl.flat, pl.init) for pl in placed)


def test_norm_pieces_join_their_own_running_sum(dev, mt):
    """OC.order_probes at every size, aligned and not: gradients on which a piece that joined the other running sum -- in the eight-piece
    round, the two-piece round, the single piece or the tail -- moves the norm by a whole ulp.  The device gives the bits of the
    restated order, which are 4096 exactly (one ulp more on the tail's probe)."""
    for n in OC.NORM_SIZES:
        probes = OC.order_probes(n)
        if not probes:
            continue
        want = torch.stack([torch.tensor(OC.norm_emulate_f32([x])) for _, x in probes])
        assert all(float(w) == 4096.0 for (lab, _), w in zip(probes, want) if not lab.endswith('tail')), n
        for off in (0, 1):
            pl = Placed(dev, [x for _, x in probes], [off] * len(probes))
            got = torch.stack([mt.norm([v]) for v in pl.views]).cpu()
            bad = [(lab, float(g)) for (lab, _), g, w in zip(probes, got, want) if not same_bits(g, w)]
            assert not bad, (n, off, bad[:6])


def test_norm_of_zero_gradients_is_exactly_zero(dev, mt):
    zeros = [torch.zeros(n) for n in OC.SIZES[::3]]
    zeros[1][0] = -0.0
    for off in (0, 3):
        pl = Placed(dev, zeros, [off] * len(zeros))
        for pre in (1.0, 0.25):
            assert int(bits(mt.norm(pl.views, pre))) == 0
        assert pl.guards_ok()


# ------------------------------------------------------------------------------------------------ clip
@pytest.mark.parametrize('case', ['below', 'equal', 'above', 'norm_zero', 'pre_scale_no_clip', 'pre_scale_and_clip'])
def test_clip_scale(dev, mt, case):
    """g * coef in float64, coef formed in fp32 from the DEVICE norm as the kernel forms it: one rounding, asserted at 2U relative;
    a factor of exactly 1 leaves the gradients bit for bit; the offset copies agree bitwise with the aligned one"""
    datas = grad_data(seed=12)
    true = OC.norm_ref(datas)
    pre = {'pre_scale_no_clip': 0.25, 'pre_scale_and_clip': 1.0 / 3.0}.get(case, 1.0)
    outs, worst = [], 0.0
    for off in OC.OFFSETS:
        pl = Placed(dev, datas, [off] * len(datas))
        norm = scalar(dev, 0.0) if case == 'norm_zero' else mt.norm(pl.views, pre)
        nv = float(norm)
        max_norm = {'below': 0.5 * true, 'equal': nv, 'above': 2.0 * true, 'norm_zero': 5.0, 'pre_scale_no_clip': true,
                    'pre_scale_and_clip': 0.1 * true}[case]
        mt.clip(pl.views, norm, max_norm, pre)
        coef = OC.clip_coef(nv, max_norm, pre)
        assert {'below': coef < 1.0, 'equal': coef <= 1.0, 'above': coef == 1.0, 'norm_zero': coef == 1.0, 'pre_scale_no_clip': coef == 0.25,
                'pre_scale_and_clip': 0.0 < coef < 0.2}[case], coef
        got = pl.cpu()
        for d, x in zip(datas, got):
            if coef == 1.0:
                assert same_bits(x, d)
            else:
                ref = d.double() * coef
                worst = max(worst, within(x, ref, 2 * U * ref.abs()))
        assert float(norm) == nv and pl.guards_ok()
        outs.append(torch.cat(got))
    assert worst <= 1.0, worst
    assert all(same_bits(outs[0], o) for o in outs[1:])
    report('mt_clip', case=case, ratio=worst)


# ------------------------------------------------------------------------------------------------ Adam, one step
def adam_placed(dev, off_p, off_g, off_m, off_v, data=None):
    p, g, m, v = data or adam_data()
    k = len(p)
    return [Placed(dev, t, [o] * k) for t, o in ((p, off_p), (g, off_g), (m, off_m), (v, off_v))]


def run_adam(mt, pls, sc, guard=None):
    mt.adam(pls[0].views, pls[1].views, pls[2].views, pls[3].views, sc, guard)
    assert all(pl.guards_ok() for pl in pls) and same_bits(pls[1].flat, pls[1].init)
    return [torch.cat(pl.cpu()) for pl in (pls[0], pls[2], pls[3])]


@pytest.mark.parametrize('step,lr', SCALARS)
def test_adam_one_step_against_float64(dev, mt, step, lr):
    """st_mt_adam over every size x offset: p, m, v inside 2 x adam_bound per element; all four operands at offsets 1, 2, 3, and only g
    or only v off the 16-byte boundary (the float-by-float loop), give bitwise the all-aligned result"""
    sc = OC.adam_scalars(step, lr)
    data = [torch.cat(t) for t in adam_data()]
    ref = OC.adam_ref(*data, *sc)
    bound = OC.adam_bound(*data, *sc)
    aligned = run_adam(mt, adam_placed(dev, 0, 0, 0, 0), sc)
    ratios = {k: within(x, r, 2 * e) for k, x, r, e in zip('pmv', aligned, ref, bound)}
    report('mt_adam_one_step', step=step, lr=lr, **{k + '_ratio': v for k, v in ratios.items()})
    assert all(bool(torch.isfinite(x).all()) for x in aligned)
    assert max(ratios.values()) <= 1.0, ratios
    for offs in ((1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 0, 0), (0, 0, 0, 3)):
        other = run_adam(mt, adam_placed(dev, *offs), sc)
        assert all(same_bits(a, b) for a, b in zip(aligned, other)), offs


# ------------------------------------------------------------------------------------------------ the guard
def small_adam_data():
    p, g, m, v = adam_data()
    pick = [0, 4, 7, 13, 19, 23]            # 1, 5, 1025, 4097, 32769 and 3 * 32768 + 5 elements
    return [[t[i] for i in pick] for t in (p, g, m, v)]


def test_guarded_adam_skips_on_a_non_finite_norm_only(dev, mt):
    """a guard norm that is NaN, +-inf or above 3.0e38 leaves p, m and v bit for bit; any other, of either sign, is the unguarded step"""
    data = small_adam_data()
    sc = OC.adam_scalars(3, 1e-3)
    want = run_adam(mt, adam_placed(dev, 0, 1, 0, 0, data), sc)
    for gn in (NAN, math.inf, -math.inf, 3.4e38, -3.4e38):
        pls = adam_placed(dev, 0, 1, 0, 0, data)
        run_adam(mt, pls, sc, guard=scalar(dev, gn))
        assert all(same_bits(pl.flat, pl.init) for pl in pls), gn
    for gn in (1e30, 0.0, -1e30, 2.9e38):
        got = run_adam(mt, adam_placed(dev, 0, 1, 0, 0, data), sc, guard=scalar(dev, gn))
        assert all(same_bits(a, b) for a, b in zip(want, got)), gn


# ------------------------------------------------------------------------------------------------ non-finite gradient elements
N_BAD = OC.MT_CHUNK + 1030
BAD_AT = {'first': 0, 'last': N_BAD - 1, 'piece_boundary': 4 * OC.MT_THREADS, 'before_chunk_boundary': OC.MT_CHUNK - 1,
          'chunk_boundary': OC.MT_CHUNK}


def test_non_finite_gradient_elements(dev, mt):
    """one NaN / +inf / -inf in a gradient: the norm is NaN / inf, the unguarded Adam makes exactly that element of p, m, v non-finite
    and every other bitwise the clean run.  The clip's rule: a NaN norm does not clip -- the gradients are only scaled
    by pre_scale; an inf norm clips with coef = 0 -- finite gradients become zeros, the inf element NaN.  Clip, then the guarded Adam
    with that norm: p, m, v bit for bit untouched."""
    cases = [(val, name, at) for val in (NAN, math.inf, -math.inf) for name, at in BAD_AT.items()]
    k = len(cases)
    base = OC.adam_operands(N_BAD, seed=77)
    data = [[t.clone() for _ in range(k)] for t in base]
    sc = OC.adam_scalars(2, 1e-3)
    clean = run_adam(mt, adam_placed(dev, 0, 0, 0, 0, [[t] for t in base]), sc)
    for (val, _, at), g in zip(cases, data[1]):
        g[at] = val
    for off in (0, 1):
        pls = adam_placed(dev, 0, off, 0, 0, data)
        norms = torch.stack([mt.norm([g]) for g in pls[1].views]).cpu()
        got = [x.view(k, N_BAD) for x in run_adam(mt, pls, sc)]
        for i, (val, name, at) in enumerate(cases):
            assert math.isnan(float(norms[i])) if math.isnan(val) else float(norms[i]) == math.inf, (name, val)
            for x, c in zip(got, clean):
                keep = torch.ones(N_BAD, dtype=torch.bool)
                keep[at] = False
                assert not math.isfinite(float(x[i, at])) and same_bits(x[i][keep], c[keep]), (name, val, off)
        # clip with the non-finite norm, then the guarded step
        for pre in (1.0, 0.25):
            pls = adam_placed(dev, 0, off, 0, 0, data)
            for i, (val, name, at) in enumerate(cases):
                g = pls[1].views[i]
                norm = mt.norm([g], pre)
                mt.clip([g], norm, 5.0, pre)
                x, g0 = g.cpu(), data[1][i]
                if math.isnan(val):
                    assert same_bits(x, g0 * pre), (name, pre)                   # (a power of two: exact; NaN * 0.25 keeps its bits)
                else:
                    keep = torch.ones(N_BAD, dtype=torch.bool)
                    keep[at] = False
                    assert math.isnan(float(x[at])) and same_bits(x[keep], g0[keep] * 0.0), (name, val, pre)
                mt.adam([pls[0].views[i]], [g], [pls[2].views[i]], [pls[3].views[i]], sc, guard=norm)
            assert all(pl.guards_ok() for pl in pls)
            assert all(same_bits(pls[j].flat, pls[j].init) for j in (0, 2, 3))


# ------------------------------------------------------------------------------------------------ kernel-argument form
class DeviceList:
    """tensor list made on the device by a seeded generator: tensor i is a view 4 + i % 4 floats into a NaN-filled buffer of its own
    with eight spare floats (the 21 M-element rows would take too long through the host)"""

    def __init__(self, dev, sizes, seed, positive=False):
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.bufs, self.views = [], []
        for i, n in enumerate(sizes):
            buf = torch.full((n + 16,), NAN, device=dev)
            v = buf[4 + i % 4:4 + i % 4 + n]
            v.normal_(generator=gen)
            if positive:
                v.abs_()
            self.bufs.append(buf)
            self.views.append(v)

    def clone(self):
        other = object.__new__(DeviceList)
        other.bufs = [b.clone() for b in self.bufs]
        other.views = [b[4 + i % 4:4 + i % 4 + v.numel()] for i, (b, v) in enumerate(zip(other.bufs, self.views))]
        assert all(a.data_ptr() % 16 == b.data_ptr() % 16 for a, b in zip(self.views, other.views))
        return other

    def guards_ok(self):
        for i, (b, v) in enumerate(zip(self.bufs, self.views)):
            lo = 4 + i % 4
            edge = torch.cat([b[:lo], b[lo + v.numel():]]).view(torch.int32)
            if not bool((edge == NAN_BITS).all()):
                return False
        return True

    def same(self, other):
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(self.bufs, other.bufs))


@pytest.mark.parametrize('c', OC.SPLIT_ROWS, ids=[c['id'] for c in OC.SPLIT_ROWS])
def test_kernel_argument_form_equals_table_form(dev, mt, c):
    """norm, clip and Adam over a list that the kernel-argument form cuts into the launches named in the row (a stream capture: no table),
    against the one-launch table form: same blocks in the same order, so the same bits -- the partial sums of a second launch land
    behind the first's (partial_base), a tensor cut across launches is registered again with its remaining chunks"""
    sizes = c['sizes']
    assert OC.plan(sizes) == c['want']
    lists = [DeviceList(dev, sizes, seed=40 + j, positive=(j == 3)) for j in range(4)]      # p, g, m, v
    ref64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in lists[1].views))
    sc = OC.adam_scalars(2, 1e-3)
    max_norm = 0.5 * ref64

    def passes(ls, ws):
        norm = mt.norm(ls[1].views, ws=ws)
        mt.clip(ls[1].views, norm, max_norm)
        mt.adam(ls[0].views, ls[1].views, ls[2].views, ls[3].views, sc)
        return norm

    tab, arg = lists, [l.clone() for l in lists]
    before = mt.misses()
    n_tab = passes(tab, mt.norm_ws(tab[1].views))
    assert mt.misses() == before + 2                       # (norm and clip share a table, Adam has its own)
    torch.cuda.synchronize()
    ws = mt.norm_ws(arg[1].views)
    ws[0].fill_(NAN)
    mt.captured(lambda: passes(arg, ws))
    nb = OC.blocks(sizes)
    assert not bool(torch.isnan(ws[0][:nb]).any()) and (ws[0].numel() == nb or bool(torch.isnan(ws[0][nb:]).all()))
    r = abs(float(n_tab) - ref64) / (OC.norm_bound(nb) * ref64)
    report('mt_kernel_argument_form', row=c['id'], norm_ratio=r)
    assert same_bits(n_tab, ws[1]) and r <= 1.0
    assert all(a.same(b) for a, b in zip(tab, arg))
    assert all(l.guards_ok() for l in tab + arg)
    assert bool(torch.isfinite(tab[0].views[-1]).all())


# ------------------------------------------------------------------------------------------------ the table cache
class CachedList:
    """p, g, m, v of one list of tiny tensors (1 .. 5 floats at every alignment) in four placed buffers that keep their addresses"""

    def __init__(self, dev, nt, seed, empty_at=()):
        sizes = [0 if j in empty_at else 1 + (j + seed) % 5 for j in range(nt)]
        ops = OC.adam_operands(sum(sizes), seed)
        offs = [(j + seed) % 4 for j in range(nt)]
        self.pls = [Placed(dev, list(t.split(sizes)), offs) for t in ops]
        self.ws = None

    def reset(self, mt):
        for pl in self.pls:
            pl.reset()
        self.ws = self.ws or mt.norm_ws(self.pls[1].views)

    def passes(self, mt, count=None):
        """norm, clip, Adam; count(kind, misses) is called after each to follow the miss counter"""
        p, g, m, v = [pl.views for pl in self.pls]
        for kind in ('norm', 'clip', 'adam'):
            before = mt.misses()
            if kind == 'norm':
                mt.norm(g, ws=self.ws)
            elif kind == 'clip':
                mt.clip(g, self.ws[1], 0.5)
            else:
                mt.adam(p, g, m, v, OC.adam_scalars(2, 1e-3))
            if count:
                count(kind, mt.misses() - before)

    def result(self):
        assert all(pl.guards_ok() for pl in self.pls)
        return torch.cat([bits(self.ws[1]).reshape(1)] + [bits(pl.flat) for pl in self.pls])


def test_table_cache_follows_lru_and_regrows_entries(dev, mt):
    """20 lists, the later ones long enough (1700 .. 3500 tensors: a table of more than 64 KiB, then more than 128 KiB) that the entry
    they take over is regrown, through norm, clip and Adam, twice round, then the first again: every result is bitwise that list's
    kernel-argument result, and the miss counter moves as an LRU over 16 entries predicts (norm and clip share a key).  Then the same
    list on a second stream: the same bits, one more miss per table.  Last, a refreshed old entry outlives the next misses."""
    lengths = list(range(2, 18)) + [1700, 1800, 3400, 3500]
    lists = [CachedList(dev, nt, seed=100 + i) for i, nt in enumerate(lengths)]
    want = []
    for cl in lists:
        cl.reset(mt)
        mt.captured(lambda: cl.passes(mt))
        want.append(cl.result())
    # whatever earlier tests left in the cache: sixteen filler lists make its contents known
    fill = Placed(dev, [torch.ones(3)] * OC.MT_TABS, [0] * OC.MT_TABS)
    for v in fill.views:
        mt.norm([v])
    lru = OC.TableLru(primed=[('fill', j) for j in range(OC.MT_TABS)])
    stream = 0
    seen = []

    def visit(i):
        def count(kind, d):
            seen.append((i, kind, d, int(lru.use(('g' if kind != 'adam' else 'pgmv', i, stream)))))
        lists[i].reset(mt)
        lists[i].passes(mt, count=count)
        assert torch.equal(lists[i].result(), want[i]), i

    for i in list(range(20)) * 2 + [0]:
        visit(i)
    assert all(d == e for _, _, d, e in seen), [s for s in seen if s[2] != s[3]][:5]
    assert sum(d for _, _, d, _ in seen) == 41 * 2 and all(d == 0 for _, kind, d, _ in seen if kind == 'clip')
    visit(0)                                               # (still there: the most recent entry)
    assert [s[2] for s in seen[-3:]] == [0, 0, 0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stream = 1
        visit(0)
        side.synchronize()
    assert [s[2:] for s in seen[-3:]] == [(1, 1), (0, 0), (1, 1)]
    torch.cuda.synchronize()
    stream = 0
    visit(0)                                               # (the first stream's entries were not the ones replaced)
    assert [s[2] for s in seen[-3:]] == [0, 0, 0]
    # the policy itself (a cycle through more keys than entries misses under any policy): use the OLDEST list that is still whole in
    # the cache -- hits that refresh it --, bring in a list that is not there -- two misses --, and the refreshed list is still there:
    # first-in-first-out would have replaced it, least-recently-used replaces the entries behind it
    whole = [k[1] for k in lru.order if k[0] == 'g' and k[2] == 0 and ('pgmv', k[1], 0) in lru.order]
    old = whole[0]
    absent = next(i for i in range(20) if not any(k[0] != 'fill' and k[1] == i for k in lru.order))
    assert {lru.order.index(('g', old, 0)), lru.order.index(('pgmv', old, 0))} & {0, 1}      # (one of the next two to go)
    visit(old)
    assert [s[2] for s in seen[-3:]] == [0, 0, 0]
    visit(absent)
    assert [s[2] for s in seen[-3:]] == [1, 0, 1]
    visit(old)
    assert [s[2] for s in seen[-3:]] == [0, 0, 0]
    assert all(d == e for _, _, d, e in seen), [s for s in seen if s[2] != s[3]][:5]


def test_zero_length_tensors_in_the_list(dev, mt):
    """empty tensors at the front, in the middle and at the end of a list change nothing but the table's key"""
    nt = 9
    full = CachedList(dev, nt, seed=300, empty_at=(0, 1, 4, 8))
    p, g, m, v = [pl.views for pl in full.pls]
    assert [x.numel() for x in g].count(0) == 4 and g[0].numel() == 0 and g[-1].numel() == 0
    keep = [j for j in range(nt) if g[j].numel()]
    sc = OC.adam_scalars(2, 1e-3)
    outs = []
    for idx in (keep, list(range(nt))):
        for pl in full.pls:
            pl.reset()
        sub = [[x[j] for j in idx] for x in (p, g, m, v)]
        norm = mt.norm(sub[1])
        mt.clip(sub[1], norm, 0.5)
        mt.adam(*sub, sc)
        full.ws = (None, norm)
        outs.append(full.result())
    assert torch.equal(outs[0], outs[1])
    for pl in full.pls:
        pl.reset()
    full.ws = mt.norm_ws(g)
    torch.cuda.synchronize()

    def passes():
        mt.norm(g, ws=full.ws)
        mt.clip(g, full.ws[1], 0.5)
        mt.adam(p, g, m, v, sc)
    mt.captured(passes)
    assert torch.equal(full.result(), outs[0])


# ------------------------------------------------------------------------------------------------ st_mt_copy
@pytest.mark.parametrize('c', OC.COPY_SPLIT_ROWS, ids=[c['id'] for c in OC.COPY_SPLIT_ROWS])
def test_mt_copy_split_rows(dev, c):
    """the MC_CHUNK and MC_NB / MC_T edges of st_mt_copy, into slots at every alignment, from sources at another: bitwise, guards intact"""
    from semi_tts_amd import ops
    sizes = c['sizes']
    g = torch.Generator().manual_seed(len(sizes))
    datas = [torch.randn(n, generator=g) for n in sizes]
    for shift in (0, 1):
        src = Placed(dev, datas, [(j + 2 * shift) % 4 for j in range(len(sizes))])
        dst = Placed(dev, [torch.full((n,), NAN) for n in sizes], [(j + shift) % 4 for j in range(len(sizes))])
        ops.mt_copy(dst.views, src.views)
        assert all(same_bits(a, b) for a, b in zip(dst.cpu(), datas))
        assert dst.guards_ok() and same_bits(src.flat, src.init)


# ------------------------------------------------------------------------------------------------ FusedAdam
FA_SHAPES = [(7,), (33, 5), (1,), (1025,), (4097,), (32769,)]
FROZEN = (1, 4)                       # parameters without a gradient on steps 3 .. 5: two step-count buckets from then on


def fa_params(dev, seed=50):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(*s, generator=g) * 10.0 ** (i - 3)).to(dev).requires_grad_() for i, s in enumerate(FA_SHAPES)]


def fa_grads(step, seed=60):
    """the gradients of step `step` (1-based), on the CPU; None for the frozen parameters on steps 3 .. 5"""
    g = torch.Generator().manual_seed(seed + step)
    out = [torch.randn(*s, generator=g) * 10.0 ** ((i + step) % 5 - 3) for i, s in enumerate(FA_SHAPES)]
    return [None if (3 <= step <= 5 and i in FROZEN) else x for i, x in enumerate(out)]


def fa_lr(step):
    return 1e-3 * (1 + step % 4) / (1 + step // 5)


def fa_set(opt, params, step, dev):
    for grp in opt.param_groups:
        grp['lr'] = fa_lr(step)
    for p, g in zip(params, fa_grads(step)):
        p.grad = None if g is None else g.to(dev)


def fa_state_bits(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out += [bits(p).reshape(-1)] + [bits(st[k]).reshape(-1) for k in ('exp_avg', 'exp_avg_sq') if k in st]
    return torch.cat(out)


def fa_copy_state_dict(sd):
    return {'state': {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd['state'].items()},
            'param_groups': [dict(g) for g in sd['param_groups']]}


def fa_one_step_check(opt, params, step, counts, do_step):
    """snapshot p, m, v, step, then every parameter that had a gradient is inside 2 x adam_bound of adam_ref with ITS step count"""
    before = []
    for p in params:
        st = opt.state.get(p, {})
        zero = torch.zeros(p.shape)
        before.append((p.detach().cpu().clone(), st['exp_avg'].cpu().clone() if 'exp_avg' in st else zero,
                       st['exp_avg_sq'].cpu().clone() if 'exp_avg_sq' in st else zero))
    grads = [None if p.grad is None else p.grad.detach().cpu().clone() for p in params]
    do_step()
    worst = 0.0
    for i, (p, g, (p0, m0, v0)) in enumerate(zip(params, grads, before)):
        st = opt.state.get(p, {})
        if g is None:
            assert same_bits(p, p0) and ('exp_avg' not in st or (same_bits(st['exp_avg'], m0) and same_bits(st['exp_avg_sq'], v0)))
            continue
        counts[i] += 1
        sc = OC.adam_scalars(counts[i], fa_lr(step))
        ref = OC.adam_ref(p0, g, m0, v0, *sc)
        bound = OC.adam_bound(p0, g, m0, v0, *sc)
        for x, r, e in zip((p, st['exp_avg'], st['exp_avg_sq']), ref, bound):
            worst = max(worst, within(x, r, 2 * e))
    return worst


def test_fused_adam_every_step_inside_the_one_step_bound(dev):
    """12 steps, another lr each step, two parameters frozen on steps 3 .. 5 (their bias corrections then run three steps behind):
    each step is checked on its own from a snapshot, so nothing compounds.  The state_dict after step 6, loaded into a fresh FusedAdam
    on copies of the parameters, continues bit for bit."""
    from semi_tts_amd.optim import FusedAdam
    params = fa_params(dev)
    opt = FusedAdam(params, lr=1e-3)
    counts, worst, trail = [0] * len(params), 0.0, {}
    for step in range(1, 13):
        fa_set(opt, params, step, dev)
        worst = max(worst, fa_one_step_check(opt, params, step, counts, opt.step))
        trail[step] = fa_state_bits(opt, params)
        if step == 6:
            sd = fa_copy_state_dict(opt.state_dict())
            snap = [p.detach().clone() for p in params]
    report('fused_adam_12_steps', ratio=worst)
    assert worst <= 1.0, worst
    assert counts == [12 - (3 if i in FROZEN else 0) for i in range(len(params))]
    assert [int(float(sd['state'][i]['step'])) for i in range(len(params))] == [6 - (3 if i in FROZEN else 0) for i in range(len(params))]
    again = [s.clone().requires_grad_() for s in snap]
    opt2 = FusedAdam(again, lr=1e-3)
    opt2.load_state_dict(sd)
    for step in range(7, 13):
        fa_set(opt2, again, step, dev)
        opt2.step()
        assert torch.equal(fa_state_bits(opt2, again), trail[step]), step


def test_fused_adam_state_dict_continues_in_torch_adam(dev):
    """the state_dict after step 6 loaded into torch.optim.Adam on CPU copies: each later step, taken from the device's state of that
    moment, inside the same one-step bound (2 x adam_bound around adam_ref).
    This held the kernel to torch's scalars: it used to form 1 - beta as 1.0f - (float)beta (0.00099998713 for beta2 = 0.999) where torch
    rounds the double 1 - beta once (0.001): 1.3e-5 relative on the g^2 term of v, 36 x this bound.  The betas now travel as doubles."""
    from semi_tts_amd.optim import FusedAdam
    params = fa_params(dev)
    opt = FusedAdam(params, lr=1e-3)
    for step in range(1, 7):
        fa_set(opt, params, step, dev)
        opt.step()
    cpu = [p.detach().cpu().clone().requires_grad_() for p in params]
    ref_opt = torch.optim.Adam(cpu, lr=1e-3)
    ref_opt.load_state_dict(fa_copy_state_dict(opt.state_dict()))
    for i, (pc, p) in enumerate(zip(cpu, params)):       # what torch loaded is the device's state: moments bit for bit, own step counts
        st = ref_opt.state[pc]
        assert same_bits(st['exp_avg'], opt.state[p]['exp_avg']) and same_bits(st['exp_avg_sq'], opt.state[p]['exp_avg_sq'])
        assert float(st['step']) == 6 - (3 if i in FROZEN else 0)
    counts = [6 - (3 if i in FROZEN else 0) for i in range(len(params))]
    worst = {}
    for step in range(7, 13):
        fa_set(opt, params, step, dev)
        fa_set(ref_opt, cpu, step, 'cpu')
        with torch.no_grad():                          # torch's step starts from the device's state of this moment (so that each step is
            # bounded on its own: from the loaded state_dict torch keeps its step counts and param_groups, the moments were checked above)
            for pc, p in zip(cpu, params):
                pc.copy_(p.detach().cpu())
                ref_opt.state[pc]['exp_avg'].copy_(opt.state[p]['exp_avg'].cpu())
                ref_opt.state[pc]['exp_avg_sq'].copy_(opt.state[p]['exp_avg_sq'].cpu())
        worst[step] = fa_one_step_check(ref_opt, cpu, step, counts, ref_opt.step)
        opt.step()
    report('fused_adam_state_dict_in_torch_adam', ratio=max(worst.values()))
    assert max(worst.values()) <= 1.0, worst


def test_fused_adam_rollback_of_a_skipped_step(dev):
    """a guarded step with a NaN norm in which only some parameters had gradients, rollback_step(which), three more steps: bitwise the
    run in which that step never happened"""
    from semi_tts_amd.optim import FusedAdam
    runs = []
    for skipped in (False, True):
        params = fa_params(dev)
        opt = FusedAdam(params, lr=1e-3)
        ok = scalar(dev, 1.0)
        for step in (1, 2):
            fa_set(opt, params, step, dev)
            opt.step(guard_norm=ok)
        if skipped:
            fa_set(opt, params, 4, dev)                # (step 4: the frozen parameters have no gradient)
            held = fa_state_bits(opt, params)
            which = opt.guarded_steps
            opt.step(guard_norm=scalar(dev, NAN))
            assert torch.equal(fa_state_bits(opt, params), held)
            assert [opt.state[p]['_step'] for p in params] == [2 if i in FROZEN else 3 for i in range(len(params))]
            opt.rollback_step(which)
            assert [opt.state[p]['_step'] for p in params] == [2] * len(params)
        for step in (6, 7, 8):
            fa_set(opt, params, step, dev)
            opt.step(guard_norm=ok)
        runs.append(fa_state_bits(opt, params))
    assert torch.equal(runs[0], runs[1])


def test_fused_adam_follows_a_parameter_whose_storage_is_replaced(dev):
    """`p.data = ...` after two steps (embed.py loading a pretrained table; module.to()): the third step updates the NEW storage, inside
    the one-step bound, and the old storage keeps its bits (the pointer table cached on the first step went on writing there)"""
    from semi_tts_amd.optim import FusedAdam
    params = fa_params(dev)
    opt = FusedAdam(params, lr=1e-3)
    counts = [0] * len(params)
    for step in (1, 2):
        fa_set(opt, params, step, dev)
        opt.step()
        counts = [c + 1 for c in counts]
    old = params[3].data
    held = bits(old).clone()
    params[3].data = old.clone()
    assert params[3].data_ptr() != old.data_ptr()
    fa_set(opt, params, 6, dev)
    worst = fa_one_step_check(opt, params, 6, counts, opt.step)
    report('fused_adam_storage_swap', ratio=worst)
    assert worst <= 1.0, worst
    assert torch.equal(bits(old), held)
    assert not same_bits(params[3].data, old)
