"""Every form and layout of the nn.LSTM sequence layers (st_lstm_seq_fwd / st_lstm_seq_bwd, csrc/rnn.hip) on the GPU against the float64
statement of the layer (lstm_seq_cases.lstm_ref): one case per entry of lstm_seq_cases.GPU_CASES, driven through ops.lstm_layer /
ops.lstm_layer_bwd with the column offsets and strided tensors of the case's layout recipe.  A case first asserts that the planner, asked
about the very tensors it passes, names the form the case is about -- a case that ran another form fails.  Bounds: the project's own from
test_gpu_lstm_persist.py (2e-5 against the reference, 3e-6 / 2e-5 between forms), established on the same input scaling up to T = 129;
the same loop in float32 on the CPU is about a hundred times inside them (test_lstm_seq_dispatch_host.py).  Every case writes its
measured error and the ratio to that float32 loop's error to the parity report.  Needs a real MI355X."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_seq_cases as LC   # noqa: E402
from helpers import bits, report, same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 7.0                    # what out, the guard columns and the tapes hold before the layer runs: no h, gate or c of these inputs is 7.0
TOL = 2e-5                    # against float64: out and gates absolute, c relative to max(1, max|c|), dxproj relative to max|dxproj|
TOL_FORMS_FWD, TOL_FORMS_C, TOL_FORMS_BWD = 3e-6, 1e-5, 2e-5       # one launch against one launch per step (test_gpu_lstm_persist.py)
FWD = [c for c in LC.GPU_CASES if not c['backward']]
BWD = [c for c in LC.GPU_CASES if c['backward']]


@contextlib.contextmanager
def persist(on):
    from semi_tts_amd import ops
    old = ops.LSTM_PERSIST
    ops.LSTM_PERSIST = on
    try:
        yield
    finally:
        ops.LSTM_PERSIST = old


def device():
    dev = torch.device('cuda:0')
    assert torch.cuda.get_device_properties(dev).multi_processor_count == LC.CUS      # the forms the cases name are those of 256 units
    return dev


def one_float_in(t):
    """a contiguous copy of t that starts one float into its 16-byte aligned buffer"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def embed(case, dev, fill):
    """(buf, x, cols, inside): the (B, T, ld) tensor of the case's layout as a view into the flat buffer `buf` (filled by `fill(n)`), the
    columns of the directions, and the mask over buf of the layer's own words"""
    B, T, H = case['B'], case['T'], case['H']
    lay = LC.layout(case['recipe'], H, case['backward'])
    n = B * T * lay['ld']
    buf = fill(lay['off'] + n + (4 - lay['off']) % 4).to(dev)
    x = buf[lay['off']:lay['off'] + n].view(B, T, lay['ld'])
    assert buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4 * lay['off']
    inside = torch.zeros(buf.shape, dtype=torch.bool)
    for c in lay['cols']:
        inside[lay['off']:lay['off'] + n].view(B, T, lay['ld'])[:, :, c:c + H] = True
    return buf, x, lay['cols'], inside


def inputs(case, dev):
    xp, w, b, dout = LC.layer_inputs(case['B'], case['T'], case['H'])
    nd = case['ndir']
    wd = [t.to(dev) for t in w[:nd]]
    if case['recipe'] == 'w1_unaligned':
        wd[1] = one_float_in(wd[1])
    return [t.to(dev) for t in xp[:nd]], wd, [t.to(dev) for t in b[:nd]], dout[:nd]


def forward(case, dev, xp, w, b, tapes, allow):
    """the layer into a fresh FILL-ed tensor of the case's layout -> (buf, out, cols, inside, gates tapes, c tapes, form it ran as)"""
    from semi_tts_amd import ops
    B, T, H, nd = case['B'], case['T'], case['H'], case['ndir']
    buf, out, cols, inside = embed(case, dev, lambda n: torch.full((n,), FILL))
    gs = [torch.full((T, B, 4, H), FILL, device=dev) for _ in range(nd)] if tapes else None
    cs = [torch.full((T, B, H), FILL, device=dev) for _ in range(nd)] if tapes else None
    with persist(allow):
        form = ops.lstm_plan(False, nd, out, cols, H, [out] + w).form
        ops.lstm_layer(xp, w, b, out, gs, cs, reverse=bool(case['reverse']), ocols=cols)
    torch.cuda.synchronize()
    ops.check_persist_status(dev)
    return buf, out, cols, inside, gs, cs, form


def err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max())


@pytest.mark.parametrize('case', FWD, ids=[c['id'] for c in FWD])
def test_forward_form_against_float64(case):
    dev = device()
    H, nd = case['H'], case['ndir']
    allow = bool(LC.layout(case['recipe'], H, 0)['allow_persist'])
    one = case['form'] == LC.PERSIST
    refs = LC.case_references(case)
    xp, w, b, _ = inputs(case, dev)
    buf, out, cols, inside, gs, cs, form = forward(case, dev, xp, w, b, True, allow)
    assert form == case['form']
    fill_bits = bits(torch.tensor([FILL]))[0]
    assert bool((bits(buf)[~inside] == fill_bits).all()), 'a word outside the layer\'s columns was written'
    assert not bool((buf.cpu()[inside] == FILL).any()), 'a word of the layer\'s columns was not written'
    e_out = e_g = e_c = e32_out = e32_c = 0.0
    for d in range(nd):
        assert not bool((gs[d] == FILL).any()) and not bool((cs[d] == FILL).any()), 'a word of the tapes was not written'
        h = out[:, :, cols[d]:cols[d] + H]
        assert torch.isfinite(h).all()
        e_out, e_g = max(e_out, err(h, refs[d]['out'])), max(e_g, err(gs[d], refs[d]['gates']))
        e_c = max(e_c, err(cs[d], refs[d]['c']) / max(1.0, float(refs[d]['c'].abs().max())))
        e32_out, e32_c = max(e32_out, refs[d]['e32_out']), max(e32_c, refs[d]['e32_c'])
    report('lstm_seq_forms', case=case['id'], err_out=e_out, err_gates=e_g, err_c=e_c, out_over_f32=e_out / e32_out, c_over_f32=e_c / e32_c)
    print('%s: out %.3g (%.1f x the float32 loop), gates %.3g, c %.3g (%.1f x)' % (case['id'], e_out, e_out / e32_out, e_g, e_c, e_c / e32_c))
    assert e_out < TOL and e_g < TOL and e_c < TOL, (e_out, e_g, e_c)
    # inference: no tapes (the per-step form keeps c in its workspace; the one launch is the same kernel instance)
    buf2, out2, _, _, _, _, form2 = forward(case, dev, xp, w, b, False, allow)
    assert form2 == case['form'] and bool((bits(buf2)[~inside] == fill_bits).all())
    if one:
        assert same_bits(buf2, buf)
        # ... and against one launch per step on the same inputs and layout
        _, out_s, _, _, gs_s, cs_s, form_s = forward(case, dev, xp, w, b, True, False)
        assert form_s == LC.STEP
        for d in range(nd):
            sl = slice(cols[d], cols[d] + H)
            assert err(out[:, :, sl], out_s[:, :, sl].cpu().double()) < TOL_FORMS_FWD and err(gs[d], gs_s[d].cpu().double()) < TOL_FORMS_FWD
            assert err(cs[d], cs_s[d].cpu().double()) < TOL_FORMS_C
    else:
        for d in range(nd):
            assert err(out2[:, :, cols[d]:cols[d] + H], refs[d]['out']) < TOL


def tapes_of(case, dev, xp, w, b):
    """the tapes of the per-step forward in the plain layout, as test_gpu_lstm_persist.py produces them"""
    from semi_tts_amd import ops
    B, T, H, nd = case['B'], case['T'], case['H'], case['ndir']
    out = torch.zeros(B, T, nd * H, device=dev)
    gs = [torch.zeros(T, B, 4, H, device=dev) for _ in range(nd)]
    cs = [torch.zeros(T, B, H, device=dev) for _ in range(nd)]
    with persist(False):
        ops.lstm_layer(xp, w, b, out, gs, cs, reverse=bool(case['reverse']))
    if case['recipe'] == 'c1_unaligned':
        cs[1] = one_float_in(cs[1])
    return gs, cs


def backward(case, dev, dout, cols, gs, cs, w, allow):
    from semi_tts_amd import ops
    B, T, H, nd = case['B'], case['T'], case['H'], case['ndir']
    with persist(allow):
        dx_like = list(torch.empty(nd, B, T, 4 * H, device=dev).unbind(0))        # (laid out as ops.lstm_layer_bwd lays out its result)
        form = ops.lstm_plan(True, nd, dout, cols, H, [dout] + gs + cs + dx_like).form
        dx = ops.lstm_layer_bwd(dout, gs, cs, w, reverse=bool(case['reverse']), dcols=cols)
    torch.cuda.synchronize()
    ops.check_persist_status(dev)
    return dx, form


@pytest.mark.parametrize('case', BWD, ids=[c['id'] for c in BWD])
def test_backward_form_against_float64(case):
    dev = device()
    B, T, H, nd = case['B'], case['T'], case['H'], case['ndir']
    allow = bool(LC.layout(case['recipe'], H, 1)['allow_persist'])
    refs = LC.case_references(case)
    xp, w, b, douts = inputs(case, dev)
    gs, cs = tapes_of(case, dev, xp, w, b)
    # dout: random everywhere (a read from a wrong column or row is a wrong number), the directions' gradients in their columns
    buf, dout, cols, _ = embed(case, dev, lambda n: torch.randn(n, generator=torch.Generator().manual_seed(17)))
    for d in range(nd):
        dout[:, :, cols[d]:cols[d] + H] = douts[d].to(dev)
    before = bits(buf).clone()
    dx, form = backward(case, dev, dout, cols, gs, cs, w, allow)
    assert form == case['form']
    assert torch.equal(bits(buf), before), 'dout was written'
    e = e32 = 0.0
    for d in range(nd):
        assert dx[d].shape == (B, T, 4 * H) and torch.isfinite(dx[d]).all()
        e, e32 = max(e, err(dx[d], refs[d]['dx']) / float(refs[d]['dx'].abs().max())), max(e32, refs[d]['e32_dx'])
    report('lstm_seq_forms', case=case['id'], err_dx=e, dx_over_f32=e / e32)
    print('%s: dxproj %.3g relative (%.1f x the float32 loop)' % (case['id'], e, e / e32))
    assert e < TOL, e
    if case['form'] == LC.PERSIST:
        dx2, form2 = backward(case, dev, dout, cols, gs, cs, w, allow)
        dx_s, form_s = backward(case, dev, dout, cols, gs, cs, w, False)
        assert form2 == LC.PERSIST and form_s == LC.PACKED
        for d in range(nd):
            assert same_bits(dx2[d], dx[d])
            assert err(dx[d], dx_s[d].cpu().double()) / float(refs[d]['dx'].abs().max()) < TOL_FORMS_BWD
        assert torch.equal(bits(buf), before)


# ------------------------------------------------------------------------------------------------ non-finite input, one launch
# The waits poll for "not the sentinel bit pattern" and are bounded by LP_SPINS, ending in a status bit: a NaN that travels through the
# hand-over must neither look like the sentinel nor reach another batch row.
NF = dict(B=17, T=3, H=64, ndir=2, reverse=0, recipe='plain', backward=0, form=LC.PERSIST)


def status_word(dev):
    from semi_tts_amd import ops
    return int(ops.persist_status(dev).item())


def test_forward_one_launch_keeps_a_nan_in_its_row():
    dev = device()
    B, T, H = NF['B'], NF['T'], NF['H']
    xp, w, b, _ = inputs(NF, dev)
    _, clean, _, _, gs0, cs0, form = forward(NF, dev, xp, w, b, True, True)
    assert form == LC.PERSIST
    others = [r for r in range(B) if r != 3]

    def run(poison):
        x0 = xp[0].clone()
        poison(x0)
        _, out, _, _, gs, cs, form = forward(NF, dev, [x0, xp[1]], w, b, True, True)      # (raises if the status word is set)
        assert form == LC.PERSIST and status_word(dev) == 0
        assert same_bits(out[others], clean[others]) and same_bits(out[3, :, H:], clean[3, :, H:]) and same_bits(out[3, 0], clean[3, 0])
        for d in range(2):
            rows = others if d == 0 else list(range(B))
            assert same_bits(gs[d][:, rows], gs0[d][:, rows]) and same_bits(cs[d][:, rows], cs0[d][:, rows])
        return out

    def nan_row(x0):
        x0[3, 1, :] = float('nan')

    out = run(nan_row)
    assert bool(torch.isnan(out[3, 1:, :H]).all())                  # direction 0 walks t = 0, 1, 2: NaN from t = 1 on

    def inf_gate(x0):
        x0[3, 1, 2 * H + 5] = float('inf')                          # the g gate of unit 5

    out = run(inf_gate)
    assert not bool(torch.isinf(out).any())


def test_backward_one_launch_keeps_a_nan_in_its_row():
    dev = device()
    case = dict(NF, backward=1)
    B, T, H = case['B'], case['T'], case['H']
    xp, w, b, douts = inputs(case, dev)
    gs, cs = tapes_of(case, dev, xp, w, b)
    dout = torch.cat([t.to(dev) for t in douts], dim=2)
    clean, form = backward(case, dev, dout, (0, H), gs, cs, w, True)
    assert form == LC.PERSIST
    bad = dout.clone()
    bad[3, 2, H // 2] = float('nan')                                # direction 0 processes t = 2 first: every earlier step of row 3 sees it
    dx, form = backward(case, dev, bad, (0, H), gs, cs, w, True)    # (raises if the status word is set)
    assert form == LC.PERSIST and status_word(dev) == 0
    others = [r for r in range(B) if r != 3]
    assert same_bits(dx[0][others], clean[0][others]) and same_bits(dx[1], clean[1])
    # t = 2: the four gate gradients of that unit; t = 1: every unit, through W_hh (t = 0 too, but its f gate has no c before it: zero)
    assert bool(torch.isnan(dx[0][3, 2].view(4, H)[:, H // 2]).all()) and bool(torch.isnan(dx[0][3, 1]).all())
