"""The bidirectional LSTM layer as ONE launch for all time steps (the ST_LSTM_PERSIST form of st_lstm_seq_fwd: recurrent weights and cell states in
registers, h handed from workgroup to workgroup through the output tensor) against the one-launch-per-step form and against
the float64 statement of the layer on the CPU (lstm_seq_cases.lstm_ref).  Needs a real MI355X."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import maxdiff   # noqa: E402
from lstm_seq_cases import lstm_ref, lstm_ref_bwd   # noqa: E402

pytestmark = pytest.mark.gpu


def _one_launch(backward, B, T, H, ld, col0, col1):
    """whether st_lstm_seq_variant takes the shape as ONE launch on this device (cus = 0), every operand aligned"""
    import ctypes as C
    from semi_tts_amd import _lib
    q = _lib.StLstmSeqQuery(backward, 2, B, T, H, ld, (C.c_int * 2)(col0, col1), 0x7f, 1, 0, 0)
    p = _lib.StLstmSeqPlan()
    assert _lib.load().st_lstm_seq_variant(C.byref(q), C.byref(p)) == 0
    return p.form == 2        # ST_LSTM_PERSIST


def _layer(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    xp = [torch.randn(B, T, 4 * H, generator=g) for _ in range(2)]
    w = [torch.randn(4 * H, H, generator=g) / H ** 0.5 for _ in range(2)]
    b = [torch.randn(4 * H, generator=g) * 0.1 for _ in range(2)]
    return xp, w, b


def _run(xp, w, b, dev, persist, tapes):
    from semi_tts_amd import ops
    B, T, H4 = xp[0].shape
    H = H4 // 4
    out = torch.zeros(B, T, 2 * H, device=dev)
    gs = [torch.zeros(T, B, 4, H, device=dev) for _ in range(2)] if tapes else None
    cs = [torch.zeros(T, B, H, device=dev) for _ in range(2)] if tapes else None
    old = ops.LSTM_PERSIST
    ops.LSTM_PERSIST = persist
    try:
        ops.lstm_layer([t.to(dev) for t in xp], [t.to(dev) for t in w], [t.to(dev) for t in b], out, gs, cs)
    finally:
        ops.LSTM_PERSIST = old
    torch.cuda.synchronize()
    ops.check_persist_status(dev)
    return out, gs, cs


@pytest.mark.parametrize('B,T,H', [(32, 43, 256), (5, 7, 64), (64, 20, 128), (33, 9, 256), (16, 129, 256), (17, 5, 512)])
def test_one_launch_bilstm_equals_the_per_step_form(B, T, H):
    dev = torch.device('cuda:0')
    assert _one_launch(0, B, T, H, 2 * H, 0, H)
    xp, w, b = _layer(B, T, H, seed=B + T + H)
    out_p, gs_p, cs_p = _run(xp, w, b, dev, True, True)
    out_s, gs_s, cs_s = _run(xp, w, b, dev, False, True)
    assert torch.isfinite(out_p).all()
    assert maxdiff(out_p, out_s) < 3e-6
    for d in range(2):
        assert maxdiff(gs_p[d], gs_s[d]) < 3e-6 and maxdiff(cs_p[d], cs_s[d]) < 1e-5
    # and the float64 statement of the layer on the same input projections
    for d in range(2):
        assert maxdiff(out_p[:, :, d * H:(d + 1) * H], lstm_ref(xp[d], w[d], b[d], d == 1)[0]) < 2e-5


def test_one_launch_bilstm_is_deterministic_and_replays_in_a_graph():
    from semi_tts_amd import ops
    dev = torch.device('cuda:0')
    B, T, H = 32, 43, 256
    xp, w, b = _layer(B, T, H, seed=1)
    a, _, _ = _run(xp, w, b, dev, True, False)
    args = [[t.to(dev) for t in ts] for ts in (xp, w, b)]
    out = torch.zeros(B, T, 2 * H, device=dev)
    g = ops.Graph()
    with g.capture():
        ops.lstm_layer(*args, out)
    for _ in range(3):
        out.zero_()
        g.launch()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
    ops.check_persist_status(dev)


def test_unsupported_shapes_take_the_per_step_form():
    assert not _one_launch(0, 32, 43, 96, 192, 0, 96)        # H % 64
    assert not _one_launch(0, 65, 43, 256, 512, 0, 256)      # more than four row tiles
    assert not _one_launch(0, 32, 43, 1024, 2048, 0, 1024)   # 512 workgroups cannot be resident at once
    assert not _one_launch(0, 32, 43, 256, 512, 0, 128)      # overlapping output columns
    dev = torch.device('cuda:0')
    xp, w, b = _layer(3, 5, 24, seed=2)
    out, _, _ = _run(xp, w, b, dev, True, False)
    ref, _, _ = _run(xp, w, b, dev, False, False)
    assert torch.equal(out, ref)


@pytest.mark.parametrize('B,T,H,In', [(32, 43, 256, 512), (5, 7, 64, 32), (17, 5, 512, 48)])
def test_one_launch_bilstm_against_oracle(B, T, H, In):
    """the whole layer as the product path runs it -- input projections of both directions (ops.gemm), then the ONE-launch recurrence
    -- against oracle.tts_oracle.lstm_layer (the restatement of nn.LSTM at src/module.py:432-438,458-460) on the same weights"""
    from oracle import tts_oracle as O
    from semi_tts_amd import ops
    dev = torch.device('cuda:0')
    assert _one_launch(0, B, T, H, 2 * H, 0, H)
    g = torch.Generator().manual_seed(1000 + B + T + H)
    x = torch.randn(B, T, In, generator=g)
    W = {}
    for sfx in ('_l0', '_l0_reverse'):
        W['lstm.weight_ih' + sfx] = torch.randn(4 * H, In, generator=g) / In ** 0.5
        W['lstm.weight_hh' + sfx] = torch.randn(4 * H, H, generator=g) / H ** 0.5
        W['lstm.bias_ih' + sfx] = torch.randn(4 * H, generator=g) * 0.1
        W['lstm.bias_hh' + sfx] = torch.randn(4 * H, generator=g) * 0.1
    ref = torch.cat([O.lstm_layer(x, W, 'lstm', False), O.lstm_layer(x, W, 'lstm', True)], dim=-1)
    xd = x.to(dev)
    xp = [ops.gemm(xd, W['lstm.weight_ih' + sfx].to(dev), bias=W['lstm.bias_ih' + sfx].to(dev)) for sfx in ('_l0', '_l0_reverse')]
    out = torch.zeros(B, T, 2 * H, device=dev)
    assert ops.LSTM_PERSIST
    ops.lstm_layer(xp, [W['lstm.weight_hh_l0'].to(dev), W['lstm.weight_hh_l0_reverse'].to(dev)],
                   [W['lstm.bias_hh_l0'].to(dev), W['lstm.bias_hh_l0_reverse'].to(dev)], out)
    torch.cuda.synchronize()
    ops.check_persist_status(dev)
    err = maxdiff(out, ref)
    from helpers import report
    report('bilstm_one_launch_vs_oracle', B=B, T=T, H=H, err=err)
    assert err < 2e-5, err


# ------------------------------------------------------------------------------------------------ backward through time, one launch
@pytest.mark.parametrize('B,T,H', [(32, 43, 256), (5, 7, 64), (33, 9, 128), (16, 129, 256), (3, 1, 32), (20, 6, 32)])
def test_one_launch_bilstm_backward_against_float64_autograd(B, T, H):
    """The ST_LSTM_PERSIST form of st_lstm_seq_bwd (BPTT of both directions in one launch, gate gradients handed over through the returned tensor) against
    the one-launch-per-step form and against float64 autograd through the plain statement of the layer (lstm_seq_cases.lstm_ref_bwd).
    ref: backward of nn.LSTM(bidirectional=True) src/module.py:432-438,458-460"""
    from semi_tts_amd import ops
    from helpers import report
    dev = torch.device('cuda:0')
    assert _one_launch(1, B, T, H, 2 * H, 0, H)
    xp, w, b = _layer(B, T, H, seed=7 + B + T + H)
    g = torch.Generator().manual_seed(99)
    dout = torch.randn(B, T, 2 * H, generator=g)
    out, gs, cs = _run(xp, w, b, dev, False, True)
    wd = [t.to(dev) for t in w]

    def bwd(persist):
        old = ops.LSTM_PERSIST
        ops.LSTM_PERSIST = persist
        try:
            dx = ops.lstm_layer_bwd(dout.to(dev), gs, cs, wd)
        finally:
            ops.LSTM_PERSIST = old
        torch.cuda.synchronize()
        ops.check_persist_status(dev)
        return dx

    dx_p, dx_p2, dx_s = bwd(True), bwd(True), bwd(False)
    worst = 0.0
    for d in range(2):
        ref = lstm_ref_bwd(xp[d], w[d], b[d], d == 1, dout[:, :, d * H:(d + 1) * H])
        scale = float(ref.abs().max())
        assert torch.isfinite(dx_p[d]).all()
        assert torch.equal(dx_p[d], dx_p2[d])                                    # run to run: bit for bit
        e_ref = float((dx_p[d].cpu().double() - ref).abs().max()) / scale
        e_step = float((dx_p[d] - dx_s[d]).abs().max()) / scale
        worst = max(worst, e_ref)
        assert e_ref < 2e-5 and e_step < 2e-5, (d, e_ref, e_step)
    report('bilstm_backward_one_launch', B=B, T=T, H=H, err=worst)


def test_bilstm_backward_shapes_outside_the_one_launch_form():
    assert not _one_launch(1, 32, 43, 24, 48, 0, 24)         # H % 32
    assert not _one_launch(1, 32, 43, 512, 1024, 0, 512)     # the 4H x 16 slice no longer fits the registers
    assert not _one_launch(1, 32, 43, 256, 514, 0, 256)      # rows of dout not 16-byte addressable
    assert not _one_launch(1, 2048, 43, 256, 512, 0, 256)    # more workgroups than can be resident at once


# ------------------------------------------------------------------------------------------------ one direction, one launch per step
@functools.lru_cache(maxsize=None)
def _one_direction_reference(B, T, H):
    """inputs of a unidirectional layer and, per walk (forward, reverse), the float64 output and gradient of the input projection
    (lstm_seq_cases.lstm_ref / lstm_ref_bwd)"""
    xp, w, b = _layer(B, T, H, seed=31 + B + T + H)
    dout = torch.randn(B, T, H, generator=torch.Generator().manual_seed(5))
    ref = [(lstm_ref(xp[0], w[0], b[0], rev)[0], lstm_ref_bwd(xp[0], w[0], b[0], rev, dout)) for rev in (False, True)]
    return xp[0], w[0], b[0], dout, ref


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('B,T,H', [(3, 5, 24), (17, 4, 32)])
def test_one_direction_layer_against_float64(B, T, H, reverse):
    """ndir = 1 of st_lstm_seq_fwd / st_lstm_seq_bwd, walking forward or backward in time (the speech encoder with rnn_bid: False runs
    the forward walk; nothing else reaches the reverse one): the kernels of the bidirectional per-step form, so its bounds apply"""
    from semi_tts_amd import ops
    dev = torch.device('cuda:0')
    xp, w, b, dout, ref = _one_direction_reference(B, T, H)
    y_ref, dx_ref = ref[1 if reverse else 0]
    xd, wd, bd = xp.to(dev), w.to(dev), b.to(dev)
    out = torch.zeros(B, T, H, device=dev)
    gs, cs = torch.zeros(T, B, 4, H, device=dev), torch.zeros(T, B, H, device=dev)
    ops.lstm_layer((xd,), (wd,), (bd,), out, (gs,), (cs,), reverse=reverse)
    out_inf = torch.zeros(B, T, H, device=dev)
    ops.lstm_layer((xd,), (wd,), (bd,), out_inf, reverse=reverse)          # inference: the cell states ping-pong in the workspace
    dx, = ops.lstm_layer_bwd(dout.to(dev), (gs,), (cs,), (wd,), reverse=reverse)
    torch.cuda.synchronize()
    e_out, e_inf = maxdiff(out.cpu().double(), y_ref), maxdiff(out_inf.cpu().double(), y_ref)
    e_dx = float((dx.cpu().double() - dx_ref).abs().max()) / float(dx_ref.abs().max())
    print('one direction B=%d T=%d H=%d reverse=%d: out %.3g, out (inference) %.3g, dxproj (relative) %.3g' % (B, T, H, reverse, e_out, e_inf, e_dx))
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    assert e_out < 2e-5 and e_inf < 2e-5
    assert e_dx < 2e-5
