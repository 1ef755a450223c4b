"""The conv bank's one job struct and its stage masks -- host only, no GPU: st_bn_bank_fwd / st_bn_bank_bwd refuse a stage combination
nobody uses, and a stage without what it reads or writes, with -22 and their own name before any launch (made-up addresses that nothing
dereferences; a fully valid job is never sent, it would launch), and ops._bn_bank_job fills pointers, strides and geometry from the
tensors it is given."""
import ctypes as C
import os

import pytest
import torch

from semi_tts_amd import _lib, ops

FAKE = 0x1000000
STATS, MERGE, NORM, REDUCE, APPLY = ops.BN_STATS, ops.BN_MERGE, ops.BN_NORM, ops.BN_REDUCE, ops.BN_APPLY
N, TOUT = 4, 5


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def valid_job(nseg=2):
    """every field any stage needs, at made-up addresses: two segments of 3 x 5 and 3 x 6 rows of N = 4"""
    segs = (_lib.StBnBankSeg * max(nseg, 1))()
    for k in range(len(segs)):
        sg = segs[k]
        sg.x, sg.ldx, sg.T, sg.mean, sg.var, sg.dx, sg.lddx, sg.sums, sg.momentum, sg.eps = FAKE, N, TOUT + k, FAKE, FAKE, FAKE, N, FAKE, 0.1, 1e-5
    return _lib.StBnBankJob(segs=segs, nseg=nseg, Bn=3, N=N, Y=FAKE, dY=FAKE, ld=2 * N, Tout=TOUT, relu_in=0, rec=None, allrec=FAKE, world=2,
                            inv_total=FAKE, ws=FAKE)


def refused(lib, entry, stages, seg=None, **fields):
    """the job with `fields` (and the fields `seg` of segment 1) overwritten is refused with -22 and the entry's name"""
    j = valid_job()
    for k, v in fields.items():
        setattr(j, k, v)
    for k, v in (seg or {}).items():
        setattr(j.segs[1], k, v)
    rc = getattr(lib, entry)(C.byref(j), stages, None)
    msg = lib.st_last_error()
    return rc == -22 and msg.startswith(entry.encode() + b':'), (rc, msg)


def ids(rows):
    return ['%s-%s-%s' % (st, '-'.join('%s=%s' % kv for kv in (seg or {}).items()), '-'.join('%s=%s' % kv for kv in f.items())) for st, seg, f in rows]


COMMON = [(None, dict(segs=None)), (None, dict(nseg=0)), (None, dict(nseg=17)), (None, dict(Bn=0)), (None, dict(N=0)), (None, dict(N=-1)),
          (dict(x=None), {}), (dict(T=0), {}), (dict(ldx=N - 1), {})]

FWD_STAGES = [0, 8, STATS | 8, MERGE | STATS, MERGE | NORM, MERGE | STATS | NORM, -1]
FWD = ([(STATS | NORM, s, f) for s, f in COMMON] + [(MERGE, s, f) for s, f in COMMON] + [(NORM, s, f) for s, f in COMMON] +
       [(STATS, s, dict(f, rec=FAKE)) for s, f in COMMON] +
       [(STATS, None, {}),                                    # the record stage without rec
        (STATS | NORM, None, dict(rec=FAKE)),                 # the one-device forward with rec
        (STATS | NORM, dict(mean=None), {}), (STATS | NORM, dict(var=None), {}), (STATS | NORM, None, dict(ws=None)),
        (STATS, None, dict(rec=FAKE, ws=None)),
        (MERGE, None, dict(allrec=None)), (MERGE, None, dict(world=0)), (MERGE, None, dict(inv_total=None)), (MERGE, dict(mean=None), {}),
        (MERGE, dict(var=None), {}),
        (NORM, None, dict(Y=None)), (NORM, None, dict(ld=2 * N - 1)), (NORM, None, dict(Tout=0)), (NORM, dict(T=TOUT - 1), {}),
        (NORM, dict(mean=None), {}), (STATS | NORM, None, dict(Y=None)), (STATS | NORM, dict(T=TOUT - 1), {})])

BWD_STAGES = [0, 4, REDUCE | 4, APPLY | 8, -1]
BWD = ([(st, s, f) for st in (REDUCE, APPLY, REDUCE | APPLY) for s, f in COMMON] +
       [(st, s, f) for st in (REDUCE, APPLY, REDUCE | APPLY)
        for s, f in [(None, dict(dY=None)), (None, dict(ld=2 * N - 1)), (None, dict(Tout=0)), (dict(T=TOUT - 1), {}), (dict(sums=None), {}),
                     (dict(mean=None), {}), (dict(var=None), {})]] +
       [(REDUCE, None, dict(ws=None)), (REDUCE | APPLY, None, dict(ws=None)),
        (APPLY, dict(dx=None), {}), (APPLY, dict(lddx=N - 1), {}), (REDUCE | APPLY, dict(dx=None), {}), (REDUCE | APPLY, dict(lddx=N - 1), {})])


@pytest.mark.parametrize('stages', FWD_STAGES)
def test_forward_refuses_stage_masks_nobody_uses(lib, stages):
    """no stage, unknown bits, MERGE with anything else -- with and without rec"""
    for rec in (None, FAKE):
        ok, got = refused(lib, 'st_bn_bank_fwd', stages, rec=rec)
        assert ok, got


@pytest.mark.parametrize('stages', BWD_STAGES)
def test_backward_refuses_stage_masks_nobody_uses(lib, stages):
    ok, got = refused(lib, 'st_bn_bank_bwd', stages)
    assert ok, got


@pytest.mark.parametrize('stages,seg,fields', FWD, ids=ids(FWD))
def test_forward_stage_refuses_what_it_cannot_run_on(lib, stages, seg, fields):
    ok, got = refused(lib, 'st_bn_bank_fwd', stages, seg, **fields)
    assert ok, got


@pytest.mark.parametrize('stages,seg,fields', BWD, ids=ids(BWD))
def test_backward_stage_refuses_what_it_cannot_run_on(lib, stages, seg, fields):
    ok, got = refused(lib, 'st_bn_bank_bwd', stages, seg, **fields)
    assert ok, got


def test_null_job_is_named_as_such(lib):
    assert lib.st_bn_bank_fwd(None, STATS | NORM, None) == -22 and lib.st_last_error() == b'st_bn_bank_fwd: null job'
    assert lib.st_bn_bank_bwd(None, REDUCE | APPLY, None) == -22 and lib.st_last_error() == b'st_bn_bank_bwd: null job'


def test_record_stage_does_not_ask_for_mean_and_var(lib):
    """STATS with rec never reads mean / var: a job without them passes that check and is refused for the next thing missing, the
    workspace; the same segments under STATS | NORM are refused for the missing mean"""
    j = valid_job()
    for k in range(2):
        j.segs[k].mean = j.segs[k].var = None
    j.rec, j.ws = FAKE, None
    assert lib.st_bn_bank_fwd(C.byref(j), STATS, None) == -22
    assert lib.st_last_error() == b'st_bn_bank_fwd: null workspace'
    j.rec, j.ws = None, FAKE
    assert lib.st_bn_bank_fwd(C.byref(j), STATS | NORM, None) == -22
    assert lib.st_last_error() == b'st_bn_bank_fwd: segment 0 without mean / var'


def test_a_stage_does_not_ask_for_what_only_another_reads(lib):
    """NORM without ws / allrec / inv_total, MERGE without Y, REDUCE without dx, APPLY without ws: each passes those checks and is refused
    for the one thing of its own that is missing"""
    for entry, stages, absent, missing, seg in [
            ('st_bn_bank_fwd', NORM, dict(ws=None, allrec=None, inv_total=None, world=0), dict(Y=None), None),
            ('st_bn_bank_fwd', MERGE, dict(ws=None, Y=None, Tout=0, ld=0), dict(allrec=None), None),
            ('st_bn_bank_bwd', REDUCE, dict(inv_total=None), dict(ws=None), dict(dx=None, lddx=0)),
            ('st_bn_bank_bwd', APPLY, dict(ws=None, inv_total=None), dict(dY=None), None)]:
        j = valid_job()
        for k, v in dict(absent, **missing).items():
            setattr(j, k, v)
        for k, v in (seg or {}).items():
            setattr(j.segs[0], k, v)
        assert getattr(lib, entry)(C.byref(j), stages, None) == -22
        msg = lib.st_last_error()
        assert msg.startswith(entry.encode()) and b'segment' not in msg, msg
        want = {'Y': b'bad output', 'allrec': b'MERGE without', 'ws': b'workspace', 'dY': b'bad gradient'}[list(missing)[0]]
        assert want in msg, msg


def test_signature_rows_and_struct_fields():
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('st_bn_bank')) == ['st_bn_bank_bwd', 'st_bn_bank_fwd', 'st_bn_bank_workspace_floats']
    assert _lib.SIGNATURES['st_bn_bank_fwd'] == _lib.SIGNATURES['st_bn_bank_bwd'] == [C.POINTER(_lib.StBnBankJob), C.c_int, C.c_void_p]
    assert [f[0] for f in _lib.StBnBankJob._fields_] == ['segs', 'nseg', 'Bn', 'N', 'Y', 'dY', 'ld', 'Tout', 'relu_in', 'rec', 'allrec', 'world',
                                                         'inv_total', 'ws']
    assert [f[0] for f in _lib.StBnBankSeg._fields_] == ['x', 'ldx', 'T', 'w', 'b', 'run_mean', 'run_var', 'batches_tracked', 'momentum', 'eps',
                                                         'mean', 'var', 'dx', 'lddx', 'sums']
    assert (STATS, MERGE, NORM, REDUCE, APPLY) == (1, 2, 4, 1, 2)


def test_builder_fills_pointers_strides_and_geometry(lib, monkeypatch):
    monkeypatch.setattr(ops, '_p', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    Bn, n, Tout = 3, 4, 5
    Ts = [5, 6, 5]
    wide = torch.zeros(Bn, 6, n + 4)
    xs = [torch.zeros(Bn, Ts[0], n), wide[:, :, 4:], torch.zeros(Bn, Ts[2], n)]          # segment 1: a column slice of wider rows
    bns = [torch.nn.BatchNorm1d(n, momentum=0.25, eps=1e-3), torch.nn.BatchNorm1d(n, affine=False), torch.nn.BatchNorm1d(n, track_running_stats=False)]
    j, t = ops._bn_bank_job(xs, bns, Tout)
    assert (j.nseg, j.Bn, j.N, j.Tout, j.ld, j.relu_in) == (3, Bn, n, Tout, 3 * n, 0)
    assert t['Y'].shape == (Bn, Tout, 3 * n) and t['stats'].shape == (3, 2, n)
    assert (j.Y, j.dY, j.ws) == (t['Y'].data_ptr(), None, t['ws'].data_ptr())
    assert t['ws'].numel() == lib.st_bn_bank_workspace_floats(3, Bn * 6, n)
    assert (j.rec, j.allrec, j.world, j.inv_total) == (None, None, 0, None)                 # the SyncBN wrapper fills its own
    for k in range(3):
        sg = j.segs[k]
        assert (sg.x, sg.ldx, sg.T) == (xs[k].data_ptr(), n + 4 if k == 1 else n, Ts[k])
        assert (sg.mean, sg.var) == (t['stats'][k, 0].data_ptr(), t['stats'][k, 1].data_ptr())
        assert (sg.dx, sg.lddx, sg.sums) == (None, 0, None)
    assert xs[1].data_ptr() == wide.data_ptr() + 16
    assert (j.segs[0].w, j.segs[0].b) == (bns[0].weight.data_ptr(), bns[0].bias.data_ptr()) and (j.segs[1].w, j.segs[1].b) == (None, None)
    assert (j.segs[0].run_mean, j.segs[0].run_var, j.segs[0].batches_tracked) == (bns[0].running_mean.data_ptr(), bns[0].running_var.data_ptr(),
                                                                                  bns[0].num_batches_tracked.data_ptr())
    assert (j.segs[2].run_mean, j.segs[2].run_var, j.segs[2].batches_tracked) == (None, None, None)
    assert j.segs[0].momentum == pytest.approx(0.25) and j.segs[0].eps == pytest.approx(1e-3, rel=1e-6)
    # backward: dY a window of wider rows, the forward's statistics, no running statistics
    dwide = torch.zeros(Bn, Tout, 3 * n + 8)
    dY = dwide[:, :, 8:]
    jb, tb = ops._bn_bank_job(xs, bns, Tout, t['stats'], dY, True)
    assert (jb.Y, jb.dY, jb.ld, jb.Tout, jb.relu_in) == (None, dwide.data_ptr() + 32, 3 * n + 8, Tout, 1)
    assert tb['stats'] is t['stats'] and tb['sums'].shape == (3, 2, n)
    for k in range(3):
        sg = jb.segs[k]
        assert (sg.dx, sg.lddx, sg.sums) == (tb['dxs'][k].data_ptr(), n, tb['sums'][k].data_ptr()) and tb['dxs'][k].shape == xs[k].shape
        assert (sg.mean, sg.run_mean, sg.batches_tracked) == (t['stats'][k, 0].data_ptr(), None, None)
