"""Training-mode BatchNorm kernels at the row counts production runs them at, against float64: the statistics (st_bn_stats: chunk-local
two-pass, merged over up to 128 chunks) over the M x N rows of norm_rnn_cases.py, the normalisation kernels, the two halves of the
backward, the conv bank's kernels (st_bn_bank_*) on the vec and the scalar paths and over unequal segments, the speech encoder's ConvLayer node and the SyncBN
record / merge over ragged shards.  Needs a real MI355X: pytest -m gpu

Tolerances: outputs maxdiff < 1e-5 on O(1) data, gradients relerr < 2e-5 (the suite's conventions); statistics of columns whose mean
is 100 standard deviations: relative variance error < 1e-5 and mean error < 1e-4 std (a one-pass sum / sum of squares is ~1e-2 off)."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_rnn_cases as R   # noqa: E402
from helpers import maxdiff, report   # noqa: E402

pytestmark = pytest.mark.gpu

ACTS = {None: lambda v: v, 'relu': torch.relu, 'tanh': torch.tanh}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def relerr(a, b):
    b = b.detach().cpu().double()
    return float((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-12))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def buffer(M, N, lay, g, scale=1.0, shift=0.5):
    """(M, ld) buffer whose columns [coff, coff + N) are the operand; the other columns hold values nobody may read or write"""
    coff, extra = R.BN_LAYOUTS[lay]
    buf = torch.randn(M, coff + N + extra, generator=g) * scale + shift
    return buf, coff


def bn_ref(x, w, b, eps, act=None):
    """float64 BatchNorm1d in training mode over the rows of x (M, N): -> (act(y), mean, biased var)"""
    mean, var = x.mean(0), x.var(0, unbiased=False)
    y = (x - mean) / torch.sqrt(var + eps)
    if w is not None:
        y = y * w
    if b is not None:
        y = y + b
    return ACTS[act](y), mean, var


# ------------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('M,N,lay', R.bn_stat_rows(), ids=['M%d-N%d-%s' % r for r in R.bn_stat_rows()])
def test_bn_stats_against_float64(dev, M, N, lay):
    """mean, biased variance, running statistics (unbiased variance) and num_batches_tracked over every chunking regime; the last column
    of the window is constant (variance 0); the buffer is only read"""
    from semi_tts_amd import ops
    buf, coff = buffer(M, N, lay, gen(M * 7 + N))
    if N > 1:
        buf[:, coff + N - 1] = 3.7
    xd = buf.to(dev)
    rm, rv = torch.full((N,), 0.25, device=dev), torch.full((N,), 2.0, device=dev)
    tracked = torch.full((1,), 5, dtype=torch.int64, device=dev)
    mean, var = ops.bn_stats(xd, coff, N, rm, rv, 0.1, tracked)
    x = buf[:, coff:coff + N].double()
    mr, vr = x.mean(0), x.var(0, unbiased=False)
    vu = x.var(0, unbiased=True) if M > 1 else vr
    errs = dict(mean=maxdiff(mean, mr), var=maxdiff(var, vr), rm=maxdiff(rm, 0.9 * 0.25 + 0.1 * mr), rv=maxdiff(rv, 0.9 * 2.0 + 0.1 * vu))
    report('bn_stats', M=M, N=N, layout=lay, chunks=R.chunking(M)[0], **errs)
    assert max(errs.values()) < 1e-5, errs
    assert int(tracked) == 6
    assert torch.equal(xd.cpu(), buf), 'st_bn_stats wrote to its input'
    if N > 1:
        assert 0.0 <= float(var[N - 1]) < 1e-10, float(var[N - 1])


@pytest.mark.parametrize('M', [2064, 4097, 4128, 8256, 16512, 33024])
def test_bn_stats_of_columns_far_from_zero(dev, M):
    """columns with |mean| = 100 std, std from 0.05 to 20: the chunk-local two-pass keeps the variance to float precision"""
    from semi_tts_amd import ops
    N = 80
    g = gen(M)
    std = torch.exp(torch.rand(N, generator=g) * 6 - 3)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    xf = torch.randn(M, N, generator=g) * std + 100 * std * sign
    mean, var = ops.bn_stats(xf.to(dev), 0, N)
    x = xf.double()
    mr, vr = x.mean(0), x.var(0, unbiased=False)
    e_var = float(((var.cpu().double() - vr).abs() / vr).max())
    e_mean = float(((mean.cpu().double() - mr).abs() / vr.sqrt()).max())
    report('bn_stats_far_from_zero', M=M, N=N, var_rel=e_var, mean_over_std=e_mean)
    assert e_var < 1e-5 and e_mean < 1e-4, (e_var, e_mean)


# ------------------------------------------------------------------------------------------------------------------- normalisation
NORM_ROWS = [(1, 1, 'c'), (33, 17, 'off'), (65, 65, 'off'), (2064, 512, 'c'), (4128, 80, 'off'), (8256, 64, 'c')]


@pytest.mark.parametrize('act', [None, 'relu', 'tanh'])
@pytest.mark.parametrize('M,N,lay', NORM_ROWS, ids=['M%d-N%d-%s' % r for r in NORM_ROWS])
def test_bn_norm_and_apply_write_only_their_window(dev, M, N, lay, act):
    """st_bn_norm_fwd (out of place, xoff / yoff into wider rows) and st_bn_apply (in place) against float64 with the same statistics;
    a zero-variance column; the columns outside the window stay as they were"""
    from semi_tts_amd import ops
    g = gen(M + N)
    buf, coff = buffer(M, N, lay, g)
    mean = torch.randn(N, generator=g) * 0.3 + 0.5
    var = torch.rand(N, generator=g) * 2 + 0.5
    var[0] = 0.0                                     # a zero-variance column: every x equals its mean, y = b
    buf[:, coff] = mean[0]
    w, b = torch.randn(N, generator=g) * 0.3 + 1, torch.randn(N, generator=g) * 0.3
    eps = 1e-3
    x = buf[:, coff:coff + N].double()
    ref = ACTS[act]((x - mean.double()) / torch.sqrt(var.double() + eps) * w.double() + b.double())
    md, vd, wd, bd = mean.to(dev), var.to(dev), w.to(dev), b.to(dev)
    out = torch.full((M, N + 9), -5.0, device=dev)
    ops.bn_norm(buf.to(dev), coff, N, md, vd, wd, bd, eps, act, out=out, yoff=5)
    inpl = buf.to(dev)
    ops.bn_apply(inpl, coff, N, md, vd, wd, bd, eps, act)
    errs = dict(norm=maxdiff(out[:, 5:5 + N], ref), apply=maxdiff(inpl[:, coff:coff + N], ref))
    report('bn_norm_apply', M=M, N=N, layout=lay, act=str(act), **errs)
    assert max(errs.values()) < 1e-5, errs
    assert bool((out[:, :5] == -5.0).all()) and bool((out[:, 5 + N:] == -5.0).all()), 'st_bn_norm_fwd wrote outside its window'
    inpl = inpl.cpu()
    assert torch.equal(inpl[:, :coff], buf[:, :coff]) and torch.equal(inpl[:, coff + N:], buf[:, coff + N:]), 'st_bn_apply wrote outside'


RES_MASK_ROWS = [(4128, 512, True, True), (2064, 512, True, False), (4128, 80, False, True), (33, 64, True, True), (1, 4, False, False)]


@pytest.mark.parametrize('want_t', [True, False])
@pytest.mark.parametrize('act', [None, 'tanh'])
@pytest.mark.parametrize('M,N,res,mask', RES_MASK_ROWS, ids=['M%d-N%d-res%d-mask%d' % r for r in RES_MASK_ROWS])
def test_bn_norm_res_mask_against_float64(dev, M, N, res, mask, act, want_t):
    """ConvLayer's fused tail: t = act(BN(x)) (kept when asked), y = (t + res) * mask"""
    from semi_tts_amd import ops
    g = gen(M * 3 + N)
    x = torch.randn(M, N, generator=g) * 2 + 0.5
    mean, var = torch.randn(N, generator=g) * 0.2 + 0.5, torch.rand(N, generator=g) * 3 + 0.5
    w, b = torch.randn(N, generator=g) * 0.3 + 1, torch.randn(N, generator=g) * 0.3
    r = torch.randn(M, N, generator=g) if res else None
    k = (torch.rand(M, N, generator=g) > 0.1).float() / 0.9 if mask else None
    eps = 1e-5
    t_ref = ACTS[act]((x.double() - mean.double()) / torch.sqrt(var.double() + eps) * w.double() + b.double())
    y_ref = t_ref + (r.double() if res else 0)
    y_ref = y_ref * (k.double() if mask else 1)
    t, y = ops.bn_norm_res_mask(x.to(dev), mean.to(dev), var.to(dev), w.to(dev), b.to(dev), eps, act,
                                r.to(dev) if res else None, k.to(dev) if mask else None, want_t=want_t)
    errs = dict(y=maxdiff(y, y_ref))
    if want_t:
        errs['t'] = maxdiff(t, t_ref)
    else:
        assert t is None
    report('bn_norm_res_mask', M=M, N=N, res=int(res), mask=int(mask), act=str(act), **errs)
    assert max(errs.values()) < 1e-5, errs


# ------------------------------------------------------------------------------------------------------------------- backward
BWD_ROWS = [(31, 1), (33, 65), (2064, 512), (4128, 80), (8256, 17), (16512, 64)]
BWD_FORMS = ['plain', 'masked_dres', 'masked', 'sync', 'masked_sync']


@pytest.mark.parametrize('form', BWD_FORMS)
@pytest.mark.parametrize('act', [None, 'relu', 'tanh'])
@pytest.mark.parametrize('M,N', BWD_ROWS, ids=['M%d-N%d' % r for r in BWD_ROWS])
def test_bn_backward_halves_against_float64(dev, M, N, act, form):
    """st_bn_bwd_reduce / st_bn_bwd_apply (dy a column slice of wider rows, Mstat = M), their masked forms (dy * mask on the way in,
    dres = dy * mask out), the SyncBN form (1 / row count read from the device) and the two together (the ConvLayer node under SyncBN)
    against float64 autograd of (act(BN(x)) [+ res]) [* mask]: the sums are (d bias, d weight), the apply half writes dx"""
    from semi_tts_amd import ops
    g = gen(M * 5 + N)
    x = torch.randn(M, N, generator=g) * 1.5 + 0.3
    w, b = torch.randn(N, generator=g) * 0.3 + 1, torch.randn(N, generator=g) * 0.3
    dy = torch.randn(M, N, generator=g)
    masked = form.startswith('masked')
    k = (torch.rand(M, N, generator=g) > 0.2).float() / 0.8 if masked else None
    eps = 1e-3
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    yr, _, _ = bn_ref(xr, wr, br, eps, act)
    (yr * (k.double() if masked else 1)).backward(dy.double())
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    mean, var = ops.bn_stats(xd, 0, N)
    t = ops.bn_norm(xd, 0, N, mean, var, wd, bd, eps, act) if act else None
    wide = torch.full((M, N + 8), float('nan'), device=dev)          # dy: columns [4, 4 + N) of rows of N + 8 (the plain forms)
    wide[:, 4:4 + N] = dy.to(dev)
    dyd = wide[:, 4:4 + N] if not masked else dy.to(dev)
    kd = k.to(dev) if masked else None
    s = ops.bn_bwd_reduce(dyd, t, act, xd, mean, var, eps, mask2d=kd)
    dres = None
    if form == 'sync':
        dx = ops.bn_bwd_apply(dyd, t, act, xd, mean, var, wd, eps, s, M, torch.full((1,), 1.0 / M, device=dev))
    elif form == 'masked_sync':
        dx, dres = ops.bn_bwd_apply(dyd, t, act, xd, mean, var, wd, eps, s, M, torch.full((1,), 1.0 / M, device=dev), mask2d=kd, want_dres=True)
    elif masked:
        dx, dres = ops.bn_bwd_apply(dyd, t, act, xd, mean, var, wd, eps, s, M, mask2d=kd, want_dres=form == 'masked_dres')
    else:
        dx = ops.bn_bwd_apply(dyd, t, act, xd, mean, var, wd, eps, s, M)
    errs = dict(dx=relerr(dx, xr.grad), db=relerr(s[:N], br.grad), dw=relerr(s[N:], wr.grad))
    report('bn_backward', M=M, N=N, act=str(act), form=form, **errs)
    assert max(errs.values()) < 2e-5, errs
    if form in ('masked_dres', 'masked_sync'):
        assert torch.equal(dres.cpu(), dy * k)
    else:
        assert dres is None


def test_sync_bn_over_ragged_shards_at_production_rows(dev):
    """SyncBN over M = 16512 rows (the C3 encoder's 64 x 258) in five ragged shards: the records merged in rank order give the statistics
    of the whole batch; each shard's apply half with the summed sums and 1 / (global count) from the device gives the whole batch's dx"""
    from semi_tts_amd import ops
    N, eps = 80, 1e-5
    sizes = [4128, 1, 33, 8256, 4094]
    M = sum(sizes)
    assert M == 16512
    g = gen(16512)
    x = torch.randn(M, N, generator=g) * 2 + 3.0
    w = torch.randn(N, generator=g) * 0.3 + 1
    dy = torch.randn(M, N, generator=g)
    xd, wd = x.to(dev), w.to(dev)
    shards = list(torch.split(xd, sizes))
    tracked = torch.zeros(1, dtype=torch.int64, device=dev)
    recs = torch.stack([ops.bn_stats_record(s, 0, N, tracked if i == 0 else None) for i, s in enumerate(shards)])
    rm, rv = torch.full((N,), 0.25, device=dev), torch.full((N,), 2.0, device=dev)
    mean, var, inv_total = ops.bn_sync_merge(recs, N, rm, rv, 0.1)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr, mr, vr = bn_ref(xr, wr, None, eps, 'tanh')
    yr.backward(dy.double())
    dys = torch.split(dy.to(dev), sizes)
    ts = [ops.bn_norm(s, 0, N, mean, var, wd, None, eps, 'tanh') for s in shards]
    ssum = sum(ops.bn_bwd_reduce(d, t, 'tanh', s, mean, var, eps) for d, t, s in zip(dys, ts, shards))
    dx = torch.cat([ops.bn_bwd_apply(d, t, 'tanh', s, mean, var, wd, eps, ssum, M, inv_total) for d, t, s in zip(dys, ts, shards)])
    errs = dict(mean=maxdiff(mean, mr), var=maxdiff(var, vr), rm=maxdiff(rm, 0.9 * 0.25 + 0.1 * mr.detach()),
                rv=maxdiff(rv, 0.9 * 2.0 + 0.1 * x.double().var(0, unbiased=True)), y=maxdiff(torch.cat(ts), yr),
                dx=relerr(dx, xr.grad), dw=relerr(ssum[N:], wr.grad))
    report('sync_bn_ragged_shards', M=M, N=N, **errs)
    assert [float(r[2 * N]) for r in recs] == [float(m) for m in sizes] and int(tracked) == 1
    assert float(inv_total) == pytest.approx(1.0 / M, rel=1e-7)
    assert max(errs['mean'], errs['var'], errs['rm'], errs['rv'], errs['y']) < 1e-5, errs
    assert max(errs['dx'], errs['dw']) < 2e-5, errs


# ------------------------------------------------------------------------------------------------------------------- conv bank
def bank_layers(K, N, seed):
    g = gen(seed)
    bns = [torch.nn.BatchNorm1d(N, momentum=0.1, eps=1e-5) for _ in range(K)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.copy_(torch.randn(N, generator=g) * 0.3 + 1)
            bn.bias.copy_(torch.randn(N, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(N, generator=g) * 0.1)
    return bns, g


def bank_reference(pres, bns, T, relu_in, dy):
    """float64 nn.BatchNorm1d per layer (statistics over all T_k frames) -> trim to T -> torch.cat, and its backward"""
    pr = [p.double().requires_grad_() for p in pres]
    bref = [copy.deepcopy(bn).double() for bn in bns]
    yr = torch.cat([bref[k]((torch.relu(pr[k]) if relu_in else pr[k]).transpose(1, 2)).transpose(1, 2)[:, :T] for k in range(len(pres))], -1)
    yr.backward(dy.double())
    return yr, pr, bref


BANK_ROWS = [(8, 80, False), (16, 80, True), (16, 18, False), (8, 18, True)]


@pytest.mark.parametrize('K,N,relu_in', BANK_ROWS, ids=['K%d-N%d-relu%d' % r for r in BANK_ROWS])
def test_batch_norm_bank_at_production_rows(dev, K, N, relu_in):
    """AG.batch_norm_bank at B = 32, T = 258 (segments of 8256 and 8288 rows: 128 chunks, a one-row last chunk), K = 8 and K = 16 =
    ST_BN_BANK_MAX; N = 80 takes the four-channel (vec) kernels, N = 18 the scalar ones"""
    from semi_tts_amd import autograd as AG
    B, T = 32, 258
    bns, g = bank_layers(K, N, seed=K * 100 + N)
    Ts = [T + 1 if (k + 1) % 2 == 0 else T for k in range(K)]
    pres = [torch.randn(B, Ts[k], N, generator=g) * 1.5 + 0.2 for k in range(K)]
    dy = torch.randn(B, T, K * N, generator=g)
    bnd = [copy.deepcopy(bn).to(dev) for bn in bns]
    if relu_in:      # the bank returns gradients at the PRE-activations: its leaves are the ReLU outputs, compared with the chain rule
        xs = [torch.relu(p.to(dev)).requires_grad_() for p in pres]
    else:
        xs = [p.to(dev).requires_grad_() for p in pres]
    bank = AG.batch_norm_bank(xs, bnd, T, relu_in)
    bank.backward(dy.to(dev))
    yr, pr, bref = bank_reference(pres, bns, T, relu_in, dy)
    errs = dict(y=maxdiff(bank, yr), dx=0.0, dw=0.0, db=0.0, rm=0.0, rv=0.0)
    for k in range(K):
        errs['dx'] = max(errs['dx'], relerr(xs[k].grad, pr[k].grad))
        errs['dw'] = max(errs['dw'], relerr(bnd[k].weight.grad, bref[k].weight.grad))
        errs['db'] = max(errs['db'], relerr(bnd[k].bias.grad, bref[k].bias.grad))
        errs['rm'] = max(errs['rm'], maxdiff(bnd[k].running_mean, bref[k].running_mean))
        errs['rv'] = max(errs['rv'], maxdiff(bnd[k].running_var, bref[k].running_var))
        assert int(bnd[k].num_batches_tracked) == 1, k
    report('bn_bank', K=K, N=N, relu_in=int(relu_in), **errs)
    assert bank.shape == (B, T, K * N)
    assert max(errs['y'], errs['rm'], errs['rv']) < 1e-5, errs
    assert max(errs['dx'], errs['dw'], errs['db']) < 2e-5, errs


def test_more_layers_than_the_bank_takes_go_through_the_group_function(dev):
    """K = 17 > ST_BN_BANK_MAX: the CBHG runs AG.batch_norm_train_group + trim + torch.cat instead -- the same values at B = 32, T = 258"""
    from semi_tts_amd import autograd as AG
    B, T, N, K = 32, 258, 80, 17
    bns, g = bank_layers(K, N, seed=1700)
    Ts = [T + 1 if (k + 1) % 2 == 0 else T for k in range(K)]
    pres = [torch.randn(B, Ts[k], N, generator=g) * 1.5 + 0.2 for k in range(K)]
    dy = torch.randn(B, T, K * N, generator=g)
    bnd = [copy.deepcopy(bn).to(dev) for bn in bns]
    xs = [p.to(dev).requires_grad_() for p in pres]
    bank = torch.cat([y[:, :T] for y in AG.batch_norm_train_group(xs, bnd)], dim=-1)
    bank.backward(dy.to(dev))
    yr, pr, bref = bank_reference(pres, bns, T, False, dy)
    errs = dict(y=maxdiff(bank, yr), dx=max(relerr(xs[k].grad, pr[k].grad) for k in range(K)),
                dw=max(relerr(bnd[k].weight.grad, bref[k].weight.grad) for k in range(K)),
                db=max(relerr(bnd[k].bias.grad, bref[k].bias.grad) for k in range(K)),
                rv=max(maxdiff(bnd[k].running_var, bref[k].running_var) for k in range(K)))
    report('bn_group_K17', K=K, N=N, **errs)
    assert errs['y'] < 1e-5 and errs['rv'] < 1e-5, errs
    assert max(errs['dx'], errs['dw'], errs['db']) < 2e-5, errs
    assert all(int(bn.num_batches_tracked) == 1 for bn in bnd)


@pytest.mark.parametrize('N', [80, 18])
def test_one_segment_bank_is_the_per_layer_kernels(dev, N):
    """the comment above BnBank: st_bn_stats runs the bank's statistics kernels on one segment, so statistics and running statistics of a
    one-segment bank and of the per-layer call are the same kernels' (equal bit for bit, whichever entry fills the segment).  Output and
    the two sums are still two kernels each with the same chunking and merge order -- bit for bit st_bn_norm_fwd / ops.bn_bwd -- and dx
    agrees to rounding: the two apply kernels compile to different multiply-add sequences (measured: 2.5 % / 3.6 % of the elements
    differ at N = 80 / 18, by at most 4.8e-7 on O(1) values); the per-layer apply on the bank's sums is bitwise the per-layer dx.
    N = 80 vec path, N = 18 scalar path; B = 32, T = 258: 128 chunks."""
    from semi_tts_amd import ops
    B, T = 32, 258
    bns, g = bank_layers(1, N, seed=N)
    x = (torch.randn(B, T, N, generator=g) * 1.5 + 0.2).to(dev)
    dy = torch.randn(B, T, N, generator=g).to(dev)
    bn_a, bn_b = copy.deepcopy(bns[0]).to(dev), copy.deepcopy(bns[0]).to(dev)
    Y, stats = ops.bn_bank_fwd([x], [bn_a], T)
    dxs, sums = ops.bn_bank_bwd(dy, [x], [bn_a], stats, False)
    x2 = x.view(-1, N)
    mean, var = ops.bn_stats(x2, 0, N, bn_b.running_mean, bn_b.running_var, bn_b.momentum, bn_b.num_batches_tracked)
    y = ops.bn_norm(x2, 0, N, mean, var, bn_b.weight, bn_b.bias, bn_b.eps)
    dx, dw, db = ops.bn_bwd(dy.view(-1, N), None, None, x2, mean, var, bn_b.weight, bn_b.eps)
    assert torch.equal(stats[0, 0], mean) and torch.equal(stats[0, 1], var)
    assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)
    assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == 1
    assert torch.equal(Y.view(-1, N), y)
    assert torch.equal(sums[0, 0], db) and torch.equal(sums[0, 1], dw)
    dx_on_bank_sums = ops.bn_bwd_apply(dy.view(-1, N), None, None, x2, mean, var, bn_b.weight, bn_b.eps, sums[0].reshape(-1).contiguous(),
                                       B * T)
    assert torch.equal(dx_on_bank_sums, dx)
    e = relerr(dxs[0].view(-1, N), dx)
    report('bn_bank_one_segment', N=N, dx=e, dx_maxdiff=maxdiff(dxs[0].view(-1, N), dx), dx_differing=float((dxs[0].view(-1, N) != dx).float().mean()))
    assert e < 1e-6, e


UNEQUAL_ROWS = [(3, (5, 43, 190), 5, 20, False), (3, (5, 43, 190), 5, 20, True), (3, (5, 43, 190), 5, 18, False), (3, (5, 43, 190), 5, 18, True),
                (17, (241,), 241, 18, False)]


@pytest.mark.parametrize('Bn,Ts,Tout,N,relu_in', UNEQUAL_ROWS, ids=['B%d-T%s-N%d-relu%d' % (r[0], 'x'.join(map(str, r[1])), r[3], r[4]) for r in UNEQUAL_ROWS])
def test_batch_norm_bank_with_unequal_segments(dev, Bn, Ts, Tout, N, relu_in):
    """AG.batch_norm_bank over segments of very different length.  Bn = 3, Ts = (5, 43, 190): 15, 129 and 570 rows = 1, 4 and 17 chunks, so
    the launches are sized for 17 chunks and the blocks past a segment's own count must return without writing; 17 chunks puts a second
    chunk into lane 0's registers in the merge kernels; the last chunks are ragged (30 of 33 rows, 26 of 34); frames t >= Tout = 5 far
    outnumber the kept ones.  Bn = 17, Ts = (241,): 4097 rows in 128 chunks of 33, of which chunks 125 to 127 are empty, in the statistics
    and in the backward's sums.  N = 20 takes the four-channel (vec) kernels, N = 18 the scalar ones."""
    from semi_tts_amd import autograd as AG
    assert [R.chunking(Bn * T)[0] for T in Ts] == ([1, 4, 17] if Bn == 3 else [128])
    K = len(Ts)
    bns, g = bank_layers(K, N, seed=Bn * 1000 + N)
    pres = [torch.randn(Bn, Ts[k], N, generator=g) * 1.5 + 0.2 for k in range(K)]
    dy = torch.randn(Bn, Tout, K * N, generator=g)
    bnd = [copy.deepcopy(bn).to(dev) for bn in bns]
    xs = [(torch.relu(p.to(dev)) if relu_in else p.to(dev)).requires_grad_() for p in pres]
    bank = AG.batch_norm_bank(xs, bnd, Tout, relu_in)
    bank.backward(dy.to(dev))
    yr, pr, bref = bank_reference(pres, bns, Tout, relu_in, dy)
    errs = dict(y=maxdiff(bank, yr), dx=max(relerr(xs[k].grad, pr[k].grad) for k in range(K)),
                dw=max(relerr(bnd[k].weight.grad, bref[k].weight.grad) for k in range(K)),
                db=max(relerr(bnd[k].bias.grad, bref[k].bias.grad) for k in range(K)),
                rm=max(maxdiff(bnd[k].running_mean, bref[k].running_mean) for k in range(K)),
                rv=max(maxdiff(bnd[k].running_var, bref[k].running_var) for k in range(K)))
    report('bn_bank_unequal', Bn=Bn, Ts=str(Ts), N=N, relu_in=int(relu_in), **errs)
    assert bank.shape == (Bn, Tout, K * N)
    assert max(errs['y'], errs['rm'], errs['rv']) < 1e-5, errs
    assert max(errs['dx'], errs['dw'], errs['db']) < 2e-5, errs
    assert all(int(bn.num_batches_tracked) == 1 for bn in bnd)


def test_bank_sync_stages_over_ragged_shards(dev):
    """the bank's SyncBN stages, driven through st_bn_bank_fwd / st_bn_bank_bwd directly, in one process: the batch of 4 utterances cut into
    shards of 1 and 3, Ts = (43, 44), Tout = 43, N = 20.  STATS with rec per shard -> the records stacked (2, nseg, 2N + 1) -> MERGE on
    every shard's job (the running statistics given on the first only) -> NORM per shard; REDUCE per shard -> the sums added -> APPLY per
    shard with inv_total: the float64 BatchNorm of the whole batch."""
    import ctypes as C
    from semi_tts_amd import _lib, ops
    lib = _lib.load()
    Bn, Ts, Tout, N, cuts = 4, (43, 44), 43, 20, [(0, 1), (1, 4)]
    K = len(Ts)
    bns, g = bank_layers(K, N, seed=4344)
    pres = [torch.randn(Bn, Ts[k], N, generator=g) * 1.5 + 0.2 for k in range(K)]
    dy = torch.randn(Bn, Tout, K * N, generator=g)
    bnd = [copy.deepcopy(bn).to(dev) for bn in bns]
    xd, dyd = [p.to(dev) for p in pres], dy.to(dev)

    def run(entry, j, stages):
        ops.check(getattr(lib, entry)(C.byref(j), stages, ops.stream_handle()), '%s(%d)' % (entry, stages))

    jobs = [ops._bn_bank_job([x[b0:b1] for x in xd], bnd, Tout) for b0, b1 in cuts]
    for k in range(K):          # the second shard's job updates no running statistics and counts no batch
        sg = jobs[1][0].segs[k]
        sg.run_mean = sg.run_var = sg.batches_tracked = None
    recs = [torch.empty(K, 2 * N + 1, device=dev) for _ in cuts]
    for (j, _), rec in zip(jobs, recs):
        j.rec = ops._p(rec)
        run('st_bn_bank_fwd', j, ops.BN_STATS)
    allrec = torch.stack(recs)
    invs = [torch.empty(K, device=dev) for _ in cuts]
    for (j, _), inv in zip(jobs, invs):
        j.allrec, j.world, j.inv_total = ops._p(allrec), len(cuts), ops._p(inv)
        run('st_bn_bank_fwd', j, ops.BN_MERGE)
        run('st_bn_bank_fwd', j, ops.BN_NORM)
    bjobs = [ops._bn_bank_job([x[b0:b1] for x in xd], bnd, Tout, t['stats'], dyd[b0:b1], False) for (b0, b1), (_, t) in zip(cuts, jobs)]
    for j, _ in bjobs:
        run('st_bn_bank_bwd', j, ops.BN_REDUCE)
    glob = bjobs[0][1]['sums'] + bjobs[1][1]['sums']
    for (j, _), inv in zip(bjobs, invs):
        for k in range(K):
            j.segs[k].sums = ops._p(glob[k])
        j.inv_total = ops._p(inv)
        run('st_bn_bank_bwd', j, ops.BN_APPLY)
    yr, pr, bref = bank_reference(pres, bns, Tout, False, dy)
    stats = jobs[0][1]['stats']
    x64 = [p.double().reshape(-1, N) for p in pres]
    errs = dict(y=maxdiff(torch.cat([t['Y'] for _, t in jobs]), yr),
                mean=max(maxdiff(stats[k, 0], x64[k].mean(0)) for k in range(K)),
                var=max(maxdiff(stats[k, 1], x64[k].var(0, unbiased=False)) for k in range(K)),
                rm=max(maxdiff(bnd[k].running_mean, bref[k].running_mean) for k in range(K)),
                rv=max(maxdiff(bnd[k].running_var, bref[k].running_var) for k in range(K)),
                dx=max(relerr(torch.cat([t['dxs'][k] for _, t in bjobs]), pr[k].grad) for k in range(K)),
                db=max(relerr(glob[k, 0], bref[k].bias.grad) for k in range(K)),
                dw=max(relerr(glob[k, 1], bref[k].weight.grad) for k in range(K)))
    report('bn_bank_sync_ragged_shards', Bn=Bn, N=N, **errs)
    assert torch.equal(stats, jobs[1][1]['stats']) and torch.equal(invs[0], invs[1]), 'the shards merged the same records differently'
    assert [[float(rec[k, 2 * N]) for k in range(K)] for rec in recs] == [[float((b1 - b0) * T) for T in Ts] for b0, b1 in cuts]
    for k in range(K):
        assert float(invs[0][k]) == pytest.approx(1.0 / (Bn * Ts[k]), rel=1e-7)
        assert int(bnd[k].num_batches_tracked) == 1, k
    assert max(errs['y'], errs['mean'], errs['var'], errs['rm'], errs['rv']) < 1e-5, errs
    assert max(errs['dx'], errs['dw'], errs['db']) < 2e-5, errs


# ------------------------------------------------------------------------------------------------------------------- ConvLayer
CONV_ROWS = [(1, True, True, True), (1, False, True, False), (2, True, False, True), (2, False, False, False)]


@pytest.mark.parametrize('stride,bias,residual,mask', CONV_ROWS, ids=['s%d-bias%d-res%d-mask%d' % r for r in CONV_ROWS])
def test_conv_layer_against_float64(dev, stride, bias, residual, mask):
    """AG.conv_layer (the speech encoder's training layer: Conv1d(k 3, pad 1, stride) -> BatchNorm1d over the batch -> tanh -> + x ->
    dropout mask) at 16 x 258 x 512 against float64 Conv1d + BatchNorm1d + tanh + residual + mask: the output, the input / weight / bias /
    BatchNorm-parameter gradients, the running statistics and num_batches_tracked"""
    from semi_tts_amd import autograd as AG
    B, T, C, KT, pad = 16, 258, 512, 3, 1
    torch.manual_seed(stride * 10 + bias)
    conv = torch.nn.Conv1d(C, C, KT, stride, padding=pad, bias=bias)
    bn = torch.nn.BatchNorm1d(C)
    g = gen(stride * 100 + bias * 10 + residual)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) * 0.3 + 1)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    To = (T + 2 * pad - KT) // stride + 1
    x = torch.randn(B, T, C, generator=g)
    k = (torch.rand(B, To, C, generator=g) > 0.1).float() / 0.9 if mask else None
    dy = torch.randn(B, To, C, generator=g)
    convd, bnd = copy.deepcopy(conv).to(dev), copy.deepcopy(bn).to(dev)
    xd = x.to(dev).requires_grad_()
    y = AG.conv_layer(xd, convd, bnd, k.to(dev) if mask else None, pad, stride, 'tanh', residual)
    y.backward(dy.to(dev))
    convr, bnr = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    xr = x.double().requires_grad_()
    pre = convr(xr.transpose(1, 2))
    pre.retain_grad()
    yr = torch.tanh(bnr(pre)).transpose(1, 2)
    if residual:
        yr = yr + xr
    if mask:
        yr = yr * k.double()
    yr.backward(dy.double())
    errs = dict(y=maxdiff(y, yr), dx=relerr(xd.grad, xr.grad), dw=relerr(convd.weight.grad, convr.weight.grad),
                dbn_w=relerr(bnd.weight.grad, bnr.weight.grad), dbn_b=relerr(bnd.bias.grad, bnr.bias.grad),
                rm=maxdiff(bnd.running_mean, bnr.running_mean), rv=maxdiff(bnd.running_var, bnr.running_var))
    if bias:
        # analytically zero (a bias in front of a batch-statistics BatchNorm): the round-off of a sum over the rows, measured against
        # the size of that sum's terms
        scale = float(pre.grad.abs().sum((0, 2)).max())
        errs['db_over_terms'] = maxdiff(convd.bias.grad, convr.bias.grad) / scale
    report('conv_layer', stride=stride, bias=int(bias), residual=int(residual), mask=int(mask), M=B * To, **errs)
    assert y.shape == (B, To, C)
    assert max(errs['y'], errs['rm'], errs['rv']) < 1e-5, errs
    assert max(errs['dx'], errs['dw'], errs['dbn_w'], errs['dbn_b'], errs.get('db_over_terms', 0.0)) < 2e-5, errs
    assert int(bnd.num_batches_tracked) == 1
