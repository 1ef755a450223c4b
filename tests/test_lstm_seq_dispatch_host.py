"""Which form an nn.LSTM sequence layer takes -- host arithmetic only, no GPU: st_lstm_seq_variant looks at the shape, the leading
dimension and columns, the alignment bits and the compute-unit budget it is given (cus > 0: no device is asked).  Every row of
lstm_seq_cases.ROWS reaches the form, weight layout, workspace size and one-launch geometry named in it; together the rows reach every
form of both passes; and the edges where the forms hand over are pinned one by one."""
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
    assert form(lib, backward=1, ld=516) == LC.PERSIST and form(lib, backward=1, ld=514) == LC.PACKED
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
        assert form(lib, backward=1, aligned=LC.AL_BWD & ~bit) == LC.PACKED, bit
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
