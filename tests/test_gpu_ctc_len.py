"""CTC with per-utterance frame counts (st_ctc_loss_len, paras.actual_len of bin/train_vqvae.py:436-444) and the device-side frame
counts it takes (st_frame_lengths), against torch.nn.functional.ctc_loss in float64 on the CPU with input_lengths.

The bounds are the derived ones of the CTC edge tests with T the padded length (u = 2^-24): each frame's log-sum-exp adds a few ulps of
|log alpha| <= T max|lp|, so the nll is within 8u (T + 4) relative to max(1, |nll|), and the occupancies exp(alpha + beta - lp + nll) turn
that absolute log error into a relative one on every gradient element: 8u (T + 4) max(1, max|lp|) of the largest gradient element.
The gradient is written into a buffer pre-filled with NaN, so an unwritten row shows; rows t >= T_b must be +0 bit for bit."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import U, bits, gen, report, same_bits   # noqa: E402
from semi_tts_amd import ops   # noqa: E402
from semi_tts_amd import autograd as AG   # noqa: E402

pytestmark = pytest.mark.gpu

INF = float('inf')
TC = ops.CTC_TC


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ref(x, text, in_len, log_input):
    """torch.nn.CTCLoss() (blank 0, mean of nll / target length, zero_infinity=False) in float64 with input_lengths = min(in_len, T)"""
    B, T, V = x.shape
    xr = x.double().requires_grad_()
    lp = xr if log_input else (xr + 1e-10).log()
    il = torch.as_tensor(in_len, dtype=torch.long).clamp(0, T)
    loss = F.ctc_loss(lp.transpose(0, 1), text[text != 0], il, (text != 0).sum(-1), blank=0, reduction='mean', zero_infinity=False)
    loss.backward()
    return float(loss.detach()), xr.grad


def _input(B, T, V, seed, log_input):
    lp = torch.log_softmax(torch.randn(B, T, V, generator=gen(seed)) * 1.5, dim=-1)
    return lp if log_input else lp.exp()


def _tols(T, x, log_input):
    lp = x if log_input else (x.double() + 1e-10).log()
    m = max(1.0, float(lp[torch.isfinite(lp)].abs().max()))
    return 8 * U * (T + 4), 8 * U * (T + 4) * m


def _rel_max(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _run(dev, x, text, in_len, log_input):
    """(loss, gradient) with the gradient written into a NaN-filled buffer of the test's own"""
    buf = torch.full(x.shape, float('nan'), device=dev)
    il = None if in_len is None else torch.tensor(in_len, dtype=torch.int32, device=dev)
    loss, grad = ops.ctc_loss(x.to(dev), text.to(dev), 1e-10, log_input=log_input, in_len=il, dprob=buf)
    assert grad.data_ptr() == buf.data_ptr()
    return loss, grad


def _zero_rows_ok(grad, in_len):
    """rows t >= T_b are +0 bit for bit (T_b = in_len clamped to [0, T])"""
    T = grad.shape[1]
    g = bits(grad)
    return all(bool((g[b, max(0, min(int(n), T)):] == 0).all()) for b, n in enumerate(in_len))


def _check(dev, x, text, in_len, log_input, name):
    B, T, V = x.shape
    loss, grad = _run(dev, x, text, in_len, log_input)
    ref, gref = _ref(x, text, in_len, log_input)
    tl, tg = _tols(T, x, log_input)
    el = abs(float(loss) - ref) / max(1.0, abs(ref))
    eg = _rel_max(grad, gref)
    report('ctc_len', case=name, B=B, T=T, V=V, log_input=int(log_input), err_loss=el, err_grad=eg, tol_loss=tl, tol_grad=tg)
    print(name, 'err_loss %.3g (tol %.3g) err_grad %.3g (tol %.3g)' % (el, tl, eg, tg))
    assert math.isfinite(ref) and bool(torch.isfinite(grad).all())
    assert el <= tl and eg <= tg, (el, tl, eg, tg)
    assert _zero_rows_ok(grad, in_len)
    again = _run(dev, x, text, in_len, log_input)
    assert same_bits(loss, again[0]) and same_bits(grad, again[1])
    return loss, grad


TEXT4 = torch.tensor([[3, 4, 4, 2, 0],        # 4 tokens, one adjacent repeat: 5 frames
                      [1, 5, 0, 0, 0],
                      [6, 0, 0, 0, 0],        # one token: one frame is enough
                      [2, 3, 2, 0, 0]])


@pytest.mark.parametrize('log_input', [False, True])
def test_ragged_batch_against_torch(dev, log_input):
    x = _input(4, 12, 7, seed=21, log_input=log_input)
    _check(dev, x, TEXT4, [12, 7, 1, 5], log_input, 'B4_T12')


@pytest.mark.parametrize('log_input', [False, True])
def test_lengths_around_the_tile_edge(dev, log_input):
    """T_b = CTC_TC - 1, CTC_TC, CTC_TC + 1 at T = 2 CTC_TC + 1: the alpha walk ends, and the beta walk starts, just before, on and just
    after a tile boundary; the gradient launch has workgroups that are all live, mixed and all zero"""
    T = 2 * TC + 1
    x = _input(3, T, 11, seed=5, log_input=log_input)
    text = torch.tensor([[1, 2, 2, 3, 0, 4], [5, 5, 5, 0, 0, 0], [7, 8, 9, 10, 1, 2]])
    _check(dev, x, text, [TC - 1, TC, TC + 1], log_input, 'tile_edge')


@pytest.mark.parametrize('log_input', [False, True])
def test_full_lengths_are_bitwise_the_unlengthed_call(dev, log_input):
    x = _input(4, 12, 7, seed=22, log_input=log_input)
    a = _run(dev, x, TEXT4, None, log_input)
    b = _run(dev, x, TEXT4, [12] * 4, log_input)
    c = _run(dev, x, TEXT4, [13, 12, 1 << 30, 99], log_input)          # in_len > T is T
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert same_bits(a[0], c[0]) and same_bits(a[1], c[1])
    assert bool(torch.isfinite(a[1]).all())


@pytest.mark.parametrize('log_input', [False, True])
def test_utterance_infeasible_at_its_length_only(dev, log_input):
    """utterance 0 needs 5 frames: feasible at T = 12, not at T_b = 4 -> loss inf, NaN rows below T_b, zero rows above; the others match"""
    B, T, V = 4, 12, 7
    in_len = [4, 7, 1, 5]
    x = _input(B, T, V, seed=23, log_input=log_input)
    full, gfull = _run(dev, x, TEXT4, None, log_input)
    assert math.isfinite(float(full)) and bool(torch.isfinite(gfull).all())
    loss, grad = _run(dev, x, TEXT4, in_len, log_input)
    ref, gref = _ref(x, TEXT4, in_len, log_input)
    grad = grad.cpu()
    assert ref == INF and float(loss) == INF
    assert bool(torch.isnan(gref[0, :4]).all()) and bool(torch.isnan(grad[0, :4]).all())
    assert _zero_rows_ok(grad, in_len)
    keep = [1, 2, 3]
    assert bool(torch.isfinite(grad[keep]).all())
    _, tg = _tols(T, x, log_input)
    eg = _rel_max(grad[keep], gref[keep])
    print('infeasible err_grad %.3g (tol %.3g)' % (eg, tg))
    assert eg <= tg, (eg, tg)


@pytest.mark.parametrize('log_input', [False, True])
def test_zero_frames_by_definition(dev, log_input):
    """T_b = 0: +inf when the utterance has tokens, 0 when it has none, all-zero rows either way"""
    B, T, V = 2, 5, 7
    x = _input(B, T, V, seed=24, log_input=log_input)
    empty = torch.tensor([[0, 0, 0], [0, 0, 0]])
    loss, grad = _run(dev, x, empty, [0, -3], log_input)
    assert float(loss) == 0.0 and bool((bits(grad) == 0).all())
    some = torch.tensor([[0, 0, 0], [2, 0, 0]])
    loss, grad = _run(dev, x, some, [0, 0], log_input)
    assert float(loss) == INF and bool((bits(grad) == 0).all())
    # one utterance without frames beside a live one: only its own rows are zero
    loss, grad = _run(dev, x, some, [0, T], log_input)
    ref, gref = _ref(x, some, [T, T], log_input)           # utterance 0 (no tokens) at full length, for utterance 1's rows
    assert bool((bits(grad)[0] == 0).all())
    _, tg = _tols(T, x, log_input)
    assert _rel_max(grad[1], gref[1]) <= tg


def test_autograd_takes_lengths_and_scales(dev):
    x = _input(4, 12, 7, seed=25, log_input=False)
    in_len = [12, 7, 1, 5]
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    xd = x.to(dev).requires_grad_()
    loss = AG.ctc_loss(xd, TEXT4.to(dev), 1e-10, in_len=il)
    (loss * 0.5).backward()
    l2, g2 = _run(dev, x, TEXT4, in_len, False)
    assert same_bits(loss, l2) and same_bits(xd.grad, g2 * 0.5)


# ---------------------------------------------------------------------------------------------------------------- st_frame_lengths
def _frames(seed=3):
    B, T, D = 3, 9, 5
    x = torch.randn(B, T, D, generator=gen(seed))
    x[0, 4] = 0                      # an all-zero frame in the middle: not counted
    x[0, 8] = 0
    x[1, 2:] = 0
    x[1, 6, 3] = 0.25                # a frame with one non-zero value: counted
    x[2, 0] = 0
    x[2, 7, 0] = 0                   # a zero value inside a live frame
    return x


@pytest.mark.parametrize('div', [1, 2, 4])
def test_frame_lengths_is_the_reference_expression(dev, div):
    x = _frames()
    want = torch.sum((x == 0).long().sum(dim=-1) != x.shape[-1], dim=-1) // div
    got = ops.frame_lengths(x.to(dev), 0.0, div)
    assert got.dtype == torch.int32 and got.tolist() == want.tolist()
    assert want.tolist() == [7 // div, 3 // div, 8 // div]        # odd counts with div = 2


def test_frame_lengths_other_pad_value_and_wide_frames(dev):
    x = torch.full((2, 70, 130), -5.0)                             # more frames than waves, more values than lanes
    x[0, 69, 129] = 1.0
    x[1, ::2, 64] = 0.0
    want = torch.sum((x == -5.0).long().sum(dim=-1) != x.shape[-1], dim=-1) // 3
    assert ops.frame_lengths(x.to(dev), -5.0, 3).tolist() == want.tolist() == [0, 35 // 3]


@pytest.mark.parametrize('r,factor', [(1, 2), (5, 2), (4, 4), (7, 1)])
def test_text_first_lengths(dev, r, factor):
    text = torch.tensor([[3, 1, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0], [2, 2, 2, 2, 2, 2], [5, 0, 6, 0, 0, 0]])
    len6 = (text != 0).sum(dim=-1) * 6
    want = 1 + (len6 + len6 % r) // factor                          # bin/train_vqvae.py:238-240
    got = ops.frame_lengths(text=text.to(dev), r=r, div=factor)
    assert got.dtype == torch.int32 and got.tolist() == want.tolist()
