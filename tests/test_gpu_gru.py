"""The GRU layer (st_gru_seq_fwd / st_gru_seq_bwd) on every kernel it can launch, against float64: the forward of every H row of
norm_rnn_cases.py against oracle.tts_oracle.gru_layer, the backward of every backward kernel through AG.bigru against float64 nn.GRU
autograd, the one-direction backward against a float64 recurrence with the recurrent product gh = W_hh h + b_hh as an explicit
intermediate.  Needs a real MI355X: pytest -m gpu

Tolerances: outputs maxdiff < 1e-5 on O(1) data, gradients relerr < 2e-5 (the suite's conventions)."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_rnn_cases as R   # noqa: E402
from helpers import maxdiff, report   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def relerr(a, b):
    b = b.detach().cpu().double()
    return float((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-12))


@contextlib.contextmanager
def float64_default():
    """the oracle allocates its state with torch.zeros: run it with float64 as the default type"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def gru_params(H, ndir, seed):
    """nn.GRU's initialisation (U(-1/sqrt(H), 1/sqrt(H))) for W_hh, b_hh of each direction, and input projections gi ~ N(0, 0.6^2)"""
    g = torch.Generator().manual_seed(seed)
    k = H ** -0.5
    p = []
    for _ in range(ndir):
        p.append(((torch.rand(3 * H, H, generator=g) * 2 - 1) * k, (torch.rand(3 * H, generator=g) * 2 - 1) * k))
    return p, g


def oracle_gru(gi, w_hh, b_hh, reverse):
    """oracle.tts_oracle.gru_layer in float64 on precomputed input projections (W_ih = I, b_ih = 0 makes its gi the given one)"""
    from oracle import tts_oracle as O
    H3 = gi.shape[-1]
    W = {'g.weight_ih' + ('_l0_reverse' if reverse else '_l0'): torch.eye(H3, dtype=torch.float64),
         'g.bias_ih' + ('_l0_reverse' if reverse else '_l0'): torch.zeros(H3, dtype=torch.float64),
         'g.weight_hh' + ('_l0_reverse' if reverse else '_l0'): w_hh.double(),
         'g.bias_hh' + ('_l0_reverse' if reverse else '_l0'): b_hh.double()}
    with float64_default():
        return O.gru_layer(gi.double(), W, 'g', reverse)


def run_fwd(dev, gis, params, H, tape=None):
    from semi_tts_amd import ops
    B, T, _ = gis[0].shape
    ndir = len(gis)
    out = torch.full((B, T, ndir * H), float('nan'), device=dev)
    gd = [x.to(dev) for x in gis]
    pd = [(w.to(dev), b.to(dev)) for w, b in params]
    ops.gru_seq(gd[0], gd[1] if ndir == 2 else None, pd[0][0], pd[1][0] if ndir == 2 else None, pd[0][1], pd[1][1] if ndir == 2 else None,
                out, tape)
    return out


@pytest.mark.parametrize('H,T,B,ndir', R.gru_fwd_rows(), ids=['H%d-T%d-B%d-d%d' % r for r in R.gru_fwd_rows()])
def test_gru_forward_against_the_oracle(dev, H, T, B, ndir):
    """every H row (tri / quad / general kernels) at T = 258, and T = 1, 7, 8, 9 around the prefetch blocks; the training forward
    (with the tape) returns bitwise the inference forward"""
    from semi_tts_amd import _lib
    params, g = gru_params(H, ndir, seed=H * 31 + T)
    gis = [torch.randn(B, T, 3 * H, generator=g) * 0.6 for _ in range(ndir)]
    out = run_fwd(dev, gis, params, H)
    tape = torch.full((ndir, B, T, 4, H), float('nan'), device=dev)
    out_t = run_fwd(dev, gis, params, H, tape)
    torch.cuda.synchronize()
    ref = torch.cat([oracle_gru(gis[d], params[d][0], params[d][1], d == 1) for d in range(ndir)], -1)
    err = maxdiff(out, ref)
    report('gru_forward', H=H, T=T, B=B, ndir=ndir, variant=R.gru_name(_lib.load().st_gru_seq_variant(H, 0)), y=err)
    assert err < 1e-5, err
    assert torch.equal(out, out_t), 'the training forward differs from the inference forward'
    assert not torch.isnan(tape).any(), 'tape entries left unwritten'


def gru_bwd_rows():
    """every backward kernel on both sides of its edges, T around the 4-step operand block and at the CBHG's 258"""
    return [(84, 258, 3), (83, 9, 2), (85, 258, 3), (128, 7, 1), (127, 33, 2), (129, 258, 2), (200, 5, 3), (341, 40, 2)]


@pytest.mark.parametrize('H,T,B', gru_bwd_rows(), ids=['H%d-T%d-B%d' % r for r in gru_bwd_rows()])
def test_bigru_backward_on_every_backward_kernel(dev, H, T, B):
    """AG.bigru (the CBHG's GRU: forward with tape, st_gru_seq_bwd, weight gradients from the recurrent products) against float64
    nn.GRU autograd: the input gradient, both W_hh and both b_hh (and W_ih, b_ih through the products in front)"""
    from semi_tts_amd import _lib
    from semi_tts_amd import autograd as AG
    torch.manual_seed(H + T)
    gru = torch.nn.GRU(H, H, batch_first=True, bidirectional=True).double()
    g = torch.Generator().manual_seed(7 * H + T)
    x = torch.randn(B, T, H, generator=g)
    dy = torch.randn(B, T, 2 * H, generator=g)
    p = {k: v.detach().float().to(dev).requires_grad_() for k, v in gru.named_parameters()}
    xd = x.to(dev).requires_grad_()
    gi_f = AG.conv(xd, p['weight_ih_l0'], p['bias_ih_l0'])
    gi_b = AG.conv(xd, p['weight_ih_l0_reverse'], p['bias_ih_l0_reverse'])
    y = AG.bigru(gi_f, gi_b, p['weight_hh_l0'], p['bias_hh_l0'], p['weight_hh_l0_reverse'], p['bias_hh_l0_reverse'])
    y.backward(dy.to(dev))
    xr = x.double().requires_grad_()
    yr, _ = gru(xr)
    yr.backward(dy.double())
    errs = {'y': maxdiff(y, yr), 'dx': relerr(xd.grad, xr.grad)}
    for k, v in gru.named_parameters():          # (W_hh / b_hh of both directions, and the input projections' W_ih / b_ih)
        errs[k] = relerr(p[k].grad, v.grad)
    report('gru_backward', H=H, T=T, B=B, variant=R.gru_name(_lib.load().st_gru_seq_variant(H, 1)), **errs)
    assert errs.pop('y') < 1e-5
    assert max(errs.values()) < 2e-5, errs


def recurrence_grads(gi, w_hh, b_hh, dout):
    """float64 GRU (one direction, forward in time) and its backward step by step, with gh_t = W_hh h_{t-1} + b_hh an explicit
    intermediate: -> (out, dgi, dgh), dgh the gradient w.r.t. gh_t (the operand of the W_hh / b_hh gradients)"""
    w, b, gi = w_hh.double(), b_hh.double(), gi.double()
    B, T, H3 = gi.shape
    H = H3 // 3

    def cell(git, gh, hp):
        r = torch.sigmoid(git[:, :H] + gh[:, :H])
        z = torch.sigmoid(git[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(git[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * hp

    hs = [torch.zeros(B, H, dtype=torch.float64)]
    for t in range(T):
        hs.append(cell(gi[:, t], hs[-1] @ w.t() + b, hs[-1]))
    dgi = torch.zeros(B, T, H3, dtype=torch.float64)
    dgh = torch.zeros(B, T, H3, dtype=torch.float64)
    dh = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        git = gi[:, t].clone().requires_grad_()
        hp = hs[t].clone().requires_grad_()
        gh = (hs[t] @ w.t() + b).requires_grad_()
        dgi[:, t], dgh[:, t], dhp = torch.autograd.grad(cell(git, gh, hp), (git, gh, hp), dh + dout[:, t].double())
        dh = dhp + dgh[:, t] @ w                  # h_{t-1} reaches the loss directly and through gh_t
    return torch.stack(hs[1:], 1), dgi, dgh


@pytest.mark.parametrize('H,T,B', [(80, 258, 2), (84, 9, 3), (100, 8, 2), (128, 1, 1), (130, 7, 3), (341, 12, 1)])
def test_one_direction_gru_backward_against_the_recurrence(dev, H, T, B):
    """ops.gru_seq_bwd with ndir = 1: dgi (gradient of the input projections) and dgh (gradient of W_hh h + b_hh, what the weight
    gradients are made of) step by step against float64"""
    from semi_tts_amd import ops
    params, g = gru_params(H, 1, seed=5 * H + T)
    gi = torch.randn(B, T, 3 * H, generator=g) * 0.6
    dout = torch.randn(B, T, H, generator=g)
    tape = torch.empty(1, B, T, 4, H, device=dev)
    out = run_fwd(dev, [gi], params, H, tape)
    dgi_f, dgi_b, dgh_f, dgh_b = ops.gru_seq_bwd(dout.to(dev), out, tape, params[0][0].to(dev), None)
    assert dgi_b is None and dgh_b is None
    ref_out, ref_dgi, ref_dgh = recurrence_grads(gi, params[0][0], params[0][1], dout)
    errs = dict(y=maxdiff(out, ref_out), dgi=relerr(dgi_f, ref_dgi), dgh=relerr(dgh_f, ref_dgh))
    report('gru_bwd_one_direction', H=H, T=T, B=B, **errs)
    assert errs['y'] < 1e-5 and errs['dgi'] < 2e-5 and errs['dgh'] < 2e-5, errs


def test_gru_refuses_hidden_sizes_no_kernel_takes(dev):
    """3H > 1024 (H = 342): both calls raise before launching anything -- the output and the gradients stay as they were"""
    from semi_tts_amd import ops
    H, B, T = 342, 2, 5
    gi = torch.zeros(B, T, 3 * H, device=dev)
    w, b = torch.zeros(3 * H, H, device=dev), torch.zeros(3 * H, device=dev)
    out = torch.full((B, T, 2 * H), 7.0, device=dev)
    with pytest.raises(RuntimeError, match='too large'):
        ops.gru_seq(gi, gi, w, w, b, b, out, None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    tape = torch.zeros(2, B, T, 4, H, device=dev)
    with pytest.raises(RuntimeError, match='too large'):
        ops.gru_seq_bwd(out, out, tape, w, w)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
