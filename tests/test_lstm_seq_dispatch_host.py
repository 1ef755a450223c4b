"""Which form an nn.LSTM sequence layer takes -- host arithmetic only, no GPU: st_lstm_seq_variant looks at the shape, the leading
dimension and columns, the alignment bits and the compute-unit budget it is given (cus > 0: no device is asked).  Every row of
lstm_seq_cases.ROWS reaches the form, weight layout, workspace size and one-launch geometry named in it; together the rows reach every
form of both passes; and the edges where the forms hand over are pinned one by one.  Then the table of what runs on the GPU
(lstm_seq_cases.GPU_CASES): its float64 reference agrees with torch.nn.LSTM, each case reaches the form it names, the cases and NOT_RUN
together account for every row, and float32 rounding alone stays twenty times inside the bounds the GPU test applies."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_seq_cases as LC   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def plan(lib, backward=0, ndir=2, B=32, T=43, H=256, ld=None, col=None, aligned=None, allow_persist=1, cus=LC.CUS, cu_reserve=0, **_):
    ld = 2 * H if ld is None else ld
    col = (0, H) if col is None else col
    aligned = (LC.AL_BWD if backward else LC.AL_FWD) if aligned is None else aligned
    q = _lib.StLstmSeqQuery(backward, ndir, B, T, H, ld, (C.c_int * 2)(*col), aligned, allow_persist, cus, cu_reserve)
    p = _lib.StLstmSeqPlan()
    rc = lib.st_lstm_seq_variant(C.byref(q), C.byref(p))
    return rc, p


@pytest.mark.parametrize('row', LC.ROWS, ids=[r['id'] for r in LC.ROWS])
def test_row_reaches_its_form(lib, row):
    rc, p = plan(lib, **row)
    assert rc == 0
    assert (p.form, p.weights) == (row['form'], row['weights'])
    assert p.ws_floats == LC.ws_floats(row['backward'], row['ndir'], row['B'], row['H'], row['form'])
    geo = row['geo'] or dict(rt=0, nkb=0, rg=0, xcd_map=0, grid=(0, 0, 0), block=0)
    assert dict(rt=p.rt, nkb=p.nkb, rg=p.rg, xcd_map=p.xcd_map, grid=(p.grid_x, p.grid_y, p.grid_z), block=p.block) == geo


def test_rows_reach_every_form_of_both_passes():
    reached = {(r['backward'], r['form']) for r in LC.ROWS}
    assert reached == {(0, LC.STEP), (0, LC.PERSIST), (1, LC.STEP), (1, LC.PACKED), (1, LC.PERSIST)}
    assert {r['rg'] for r in (r['geo'] for r in LC.ROWS if r['backward'] and r['geo'])} == {8, 16}
    assert {r['ndir'] for r in LC.ROWS} == {1, 2} and {r['reverse'] for r in LC.ROWS if r['ndir'] == 1} == {0, 1}


def form(lib, **kw):
    rc, p = plan(lib, **kw)
    assert rc == 0
    return p.form


def test_forward_edges(lib):
    for H in (64, 128, 256, 512):
        assert form(lib, H=H) == LC.PERSIST, H
    for H in (96, 192, 576, 1024):
        assert form(lib, H=H) == LC.STEP, H
    assert form(lib, B=64) == LC.PERSIST and form(lib, B=65) == LC.STEP
    assert form(lib, ld=516) == LC.PERSIST and form(lib, ld=514) == LC.STEP
    assert form(lib, ld=516, col=(0, 260)) == LC.PERSIST and form(lib, ld=516, col=(0, 258)) == LC.STEP
    assert form(lib, ld=516, col=(2, 260)) == LC.STEP
    assert form(lib, col=(0, 128)) == LC.STEP and form(lib, ld=1024, col=(512, 384)) == LC.STEP       # overlapping output columns
    for bit in (1, 2, 4):
        assert form(lib, aligned=LC.AL_FWD & ~bit) == LC.STEP, bit
    assert form(lib, allow_persist=0) == LC.STEP
    assert form(lib, ndir=1, ld=256, col=(0, 0)) == LC.STEP
    assert form(lib, H=512, cus=256) == LC.PERSIST and form(lib, H=512, cus=255) == LC.STEP
    assert form(lib, H=256, cus=128) == LC.PERSIST and form(lib, H=256, cus=128, cu_reserve=1) == LC.STEP


def test_backward_edges(lib):
    for H in (32, 64, 128, 256):
        assert form(lib, backward=1, H=H) == LC.PERSIST, H
    for H in (96, 512):
        assert form(lib, backward=1, H=H) == LC.PACKED, H
    assert form(lib, backward=1, H=24) == LC.STEP
    assert form(lib, backward=1, ld=516) == LC.PERSIST and form(lib, backward=1, ld=514) == LC.STEP
    # the packed launch loads dout and the tapes and stores dxproj in 16-byte pieces: rows, columns and operands it cannot address so
    # go to the per-step form, with one-launch allowed or not
    for allow in (0, 1):
        assert form(lib, backward=1, allow_persist=allow, ld=514) == LC.STEP
        assert form(lib, backward=1, allow_persist=allow, ld=516, col=(0, 258)) == LC.STEP
        assert form(lib, backward=1, allow_persist=allow, ld=516, col=(2, 260)) == LC.STEP
        assert form(lib, backward=1, allow_persist=allow, H=512, ld=1028, col=(4, 516)) == LC.PACKED
    assert form(lib, backward=1, B=2048) == LC.PACKED
    assert form(lib, backward=1, B=128) == LC.PERSIST and form(lib, backward=1, B=129) == LC.PACKED
    for B, rg in ((32, 8), (33, 16)):        # 2 * (H/16) * ceil(B/8) against half of the 256 compute units
        rc, p = plan(lib, backward=1, B=B)
        assert rc == 0 and p.form == LC.PERSIST and p.rg == rg and p.grid_y == (B + rg - 1) // rg
    # the units left to the all-reduce count against the residency test only, not against the choice of rg
    assert form(lib, backward=1, B=128, cu_reserve=0) == LC.PERSIST and form(lib, backward=1, B=128, cu_reserve=32) == LC.PACKED
    rc, p = plan(lib, backward=1, B=32, cu_reserve=32)
    assert rc == 0 and p.form == LC.PERSIST and p.rg == 8
    for bit in (1, 2, 4, 8, 16, 32, 64):
        rc, p = plan(lib, backward=1, aligned=LC.AL_BWD & ~bit)
        assert rc == 0 and (p.form, p.weights, p.ws_floats) == (LC.STEP, LC.W_T, 4 * 32 * 256), bit
    assert form(lib, backward=1, allow_persist=0) == LC.PACKED
    for H in (24, 32, 256, 512):             # one direction: always per step, on the transposed weights
        rc, p = plan(lib, backward=1, ndir=1, H=H, ld=H, col=(0, 0))
        assert rc == 0 and (p.form, p.weights) == (LC.STEP, LC.W_T) and p.ws_floats == 2 * 32 * H, H


@pytest.mark.parametrize('bad', LC.REFUSED, ids=[r['id'] for r in LC.REFUSED])
def test_refused_queries(lib, bad):
    for backward in (0, 1):
        assert plan(lib, backward=backward, **bad)[0] == -1


def test_run_entry_points_refuse_before_any_launch(lib):
    """a job whose `weights` is not the plan's, or whose ws is NULL while the plan needs one, is refused (fake addresses: nothing is
    launched); so is `reverse` with two directions"""
    B, T, H = 3, 5, 24
    j = _lib.StLstmSeqBwdJob(ndir=2, dout=0x1000000, ldd=2 * H, B=B, T=T, H=H, weights=LC.W_NATURAL, allow_persist=1)
    for d in range(2):
        j.dcol[d], j.gates_tape[d], j.c_tape[d], j.w[d], j.dxproj[d] = d * H, 0x2000000, 0x3000000, 0x4000000, 0x5000000
    assert lib.st_lstm_seq_bwd(C.byref(j), None) == -22 and b'layout 0, the plan names 1' in lib.st_last_error()
    j.weights = LC.W_T
    assert lib.st_lstm_seq_bwd(C.byref(j), None) == -22 and b'ws is NULL (%d floats' % (4 * B * H) in lib.st_last_error()
    f = _lib.StLstmSeqJob(ndir=1, out=0x1000000, ldo=H, B=B, T=T, H=H)
    f.xproj[0], f.w_hh[0] = 0x2000000, 0x3000000
    assert lib.st_lstm_seq_fwd(C.byref(f), None) == -22 and b'ws is NULL (%d floats' % (3 * B * H) in lib.st_last_error()
    f.ndir, f.reverse = 2, 1
    assert lib.st_lstm_seq_fwd(C.byref(f), None) == -22 and lib.st_lstm_seq_fwd(None, None) == -22 and lib.st_lstm_seq_bwd(None, None) == -22


def test_null_pointers(lib):
    q, p = _lib.StLstmSeqQuery(), _lib.StLstmSeqPlan()
    assert lib.st_lstm_seq_variant(None, C.byref(p)) == -1 and lib.st_lstm_seq_variant(C.byref(q), None) == -1


# ------------------------------------------------------------------------------------------------ the reference and the GPU case table
GPU_IDS = [c['id'] for c in LC.GPU_CASES]


@pytest.mark.parametrize('B,T,H', [(3, 5, 24), (2, 1, 16)])
def test_reference_agrees_with_torch(B, T, H):
    """lstm_ref / lstm_ref_bwd against torch.nn.LSTM(bidirectional=True).double() fed the projections through W_ih = I, both directions"""
    import torch
    xp, w, b, dout = LC.layer_inputs(B, T, H)
    lstm = torch.nn.LSTM(4 * H, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in enumerate(('', '_reverse')):
            getattr(lstm, 'weight_ih_l0' + sfx).copy_(torch.eye(4 * H))
            getattr(lstm, 'bias_ih_l0' + sfx).zero_()
            getattr(lstm, 'weight_hh_l0' + sfx).copy_(w[d])
            getattr(lstm, 'bias_hh_l0' + sfx).copy_(b[d])
    for d in range(2):
        x = xp[d].double().requires_grad_()
        y = lstm(x)[0][:, :, d * H:(d + 1) * H]
        y.backward(dout[d].double())
        out, gates, c = LC.lstm_ref(xp[d], w[d], b[d], d == 1)
        dx = LC.lstm_ref_bwd(xp[d], w[d], b[d], d == 1, dout[d])
        assert out.dtype == torch.float64 and out.shape == (B, T, H) and gates.shape == (T, B, 4, H) and c.shape == (T, B, H)
        assert float((out - y.detach()).abs().max()) < 1e-12 and float((dx - x.grad).abs().max()) < 1e-12
        # the tapes restate the cell: h = o tanh(c), c_t = f c_prev + i g along the direction's walk
        assert float((gates[:, :, 3] * torch.tanh(c) - out.transpose(0, 1)).abs().max()) < 1e-12
        order = list(range(T - 1, -1, -1)) if d else list(range(T))
        for s, t in enumerate(order):
            prev = c[order[s - 1]] if s else torch.zeros(B, H, dtype=torch.float64)
            assert float((gates[t, :, 1] * prev + gates[t, :, 0] * gates[t, :, 2] - c[t]).abs().max()) < 1e-12


def case_query(case):
    lay = LC.layout(case['recipe'], case['H'], case['backward'])
    col = tuple(lay['cols']) + (0,) * (2 - len(lay['cols']))
    aligned = (LC.AL_BWD if case['backward'] else LC.AL_FWD) & ~lay['unaligned']
    return dict(backward=case['backward'], ndir=case['ndir'], B=case['B'], T=case['T'], H=case['H'], ld=lay['ld'], col=col, aligned=aligned,
                allow_persist=lay['allow_persist'], cus=LC.CUS)


@pytest.mark.parametrize('case', LC.GPU_CASES, ids=GPU_IDS)
def test_gpu_case_reaches_its_form(lib, case):
    """the planner, asked with 256 compute units and the alignment bits the recipe implies, names what the case says it runs"""
    rc, p = plan(lib, **case_query(case))
    assert rc == 0
    assert (p.form, p.weights, p.rg, p.rt) == (case['form'], case['weights'], case['rg'], case['rt'])
    row = next(r for r in LC.ROWS if r['id'] == case['row'])
    assert (row['backward'], row['form'], row['weights']) == (case['backward'], case['form'], case['weights'])
    assert row['ndir'] == case['ndir']
    if row['geo']:
        assert row['geo']['rg'] == p.rg      # (the row keeps the workload's H and B: nkb and rt are the case's own)


def test_gpu_cases_cover_every_row():
    """every ROWS id is run on the GPU or named in NOT_RUN, never both; NOT_RUN holds exactly the ten ids that cannot or need not run"""
    assert len(set(GPU_IDS)) == len(GPU_IDS)
    ids, run = {r['id'] for r in LC.ROWS}, {c['row'] for c in LC.GPU_CASES}
    assert run <= ids and set(LC.NOT_RUN) <= ids
    assert not run & set(LC.NOT_RUN)
    assert run | set(LC.NOT_RUN) == ids, sorted(ids - run - set(LC.NOT_RUN))
    assert set(LC.NOT_RUN) == {'fwd_h512_255_cus', 'fwd_h512_reserve', 'bwd_b33_512_cus', 'bwd_b128_reserve', 'bwd_b112_reserve',
                               'fwd_overlap', 'fwd_h1024', 'bwd_b2048', 'bwd_b128', 'bwd_dx0_unaligned'}
    for id in LC.NOT_RUN:
        row = next(r for r in LC.ROWS if r['id'] == id)
        assert (row['cus'] != LC.CUS or row['cu_reserve'] != 0) == ('cus' in id or 'reserve' in id)
    # every template instance of the one-launch kernels is run: (RT, NKB) of the forward, (NKB, RG) of the backward that 256 units reach
    one = [c for c in LC.GPU_CASES if c['form'] == LC.PERSIST]
    assert {c['rt'] for c in one if not c['backward']} == {1, 2, 3, 4} and {c['H'] // 64 for c in one if not c['backward']} == {1, 2, 4, 8}
    assert {(c['H'] // 32, c['rg']) for c in one if c['backward']} == {(1, 8), (2, 8), (4, 8), (8, 8), (4, 16), (8, 16)}
    assert {c['recipe'] for c in one} == {'plain', 'swapped', 'embedded'}


def test_float32_reference_leaves_room_under_the_bound(capsys):
    """The bounds of test_gpu_lstm_seq_forms.py (2e-5) must not be within reach of float32 rounding alone: the same loop in float32 on the
    CPU stays below 1e-6 from the float64 result at every GPU shape -- out absolute, c relative to max(1, max|c|), dxproj relative to
    max|dxproj|."""
    worst = {}
    for case in LC.GPU_CASES:
        for ref in LC.case_references(case):
            e = (ref['e32_out'], ref['e32_c'], ref['e32_dx'])
            worst[(case['B'], case['T'], case['H'])] = tuple(max(a, b) for a, b in zip(e, worst.get((case['B'], case['T'], case['H']), (0, 0, 0))))
            assert max(e) < 1e-6, (case['id'], e)
    with capsys.disabled():
        print()
        for shape, e in sorted(worst.items()):
            print('float32 loop against float64 at (B, T, H) = %-14s out %.2e  c %.2e  dxproj %.2e' % ((shape,) + e))
