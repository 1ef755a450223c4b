"""The BatchNorm backward's one job struct -- host only, no GPU: st_bn_bwd_reduce / st_bn_bwd_apply refuse a bad job with -22 and their
own name before any launch (made-up addresses that nothing dereferences; a fully valid job is never sent, it would launch), and
ops._bn_bwd_job fills pointers, row strides, M and N from the tensors it is given."""
import ctypes as C
import os

import pytest
import torch

from semi_tts_amd import _lib, ops

FAKE = 0x1000000


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def valid_job():
    """every field either half needs, at made-up addresses: M = 5 rows of N = 3, tanh, masked, with a residual gradient"""
    return _lib.StBnBwdJob(dy=FAKE, ldd=3, y=FAKE, ldy=3, act=ops.ACT['tanh'], x=FAKE, ldx=3, mean=FAKE, var=FAKE, w=FAKE, eps=1e-5, M=5, N=3,
                           mask=FAKE, ldm=3, s=FAKE, Mstat=5, inv_total=None, dx=FAKE, lddx=3, dres=FAKE, lddr=3)


COMMON = [dict(dy=None), dict(x=None), dict(mean=None), dict(var=None), dict(s=None), dict(M=0), dict(M=-1), dict(N=0), dict(N=-1), dict(y=None)]


def refused(lib, call, name, **fields):
    j = valid_job()
    for k, v in fields.items():
        setattr(j, k, v)
    rc = call(j)
    msg = lib.st_last_error()
    return rc == -22 and name in msg and b'bad arguments' in msg


@pytest.mark.parametrize('bad', COMMON + [dict(ws=None)], ids=lambda d: '-'.join('%s=%s' % kv for kv in d.items()))
def test_reduce_refuses_before_any_launch(lib, bad):
    bad = dict(bad)
    ws = bad.pop('ws', FAKE)
    assert refused(lib, lambda j: lib.st_bn_bwd_reduce(C.byref(j), ws, None), b'st_bn_bwd_reduce', **bad)


@pytest.mark.parametrize('bad', COMMON + [dict(dx=None), dict(Mstat=4), dict(Mstat=0)], ids=lambda d: '-'.join('%s=%s' % kv for kv in d.items()))
def test_apply_refuses_before_any_launch(lib, bad):
    assert refused(lib, lambda j: lib.st_bn_bwd_apply(C.byref(j), None), b'st_bn_bwd_apply', **bad)


def test_null_job_is_named_as_such(lib):
    assert lib.st_bn_bwd_reduce(None, FAKE, None) == -22 and lib.st_last_error() == b'st_bn_bwd_reduce: null job'
    assert lib.st_bn_bwd_apply(None, None) == -22 and lib.st_last_error() == b'st_bn_bwd_apply: null job'


def test_null_y_is_refused_only_with_an_activation(lib):
    """act == ST_ACT_NONE takes a NULL y: the job then passes that check and is refused for the next thing missing"""
    assert refused(lib, lambda j: lib.st_bn_bwd_reduce(C.byref(j), FAKE, None), b'st_bn_bwd_reduce', y=None, act=ops.ACT['relu'])
    assert refused(lib, lambda j: lib.st_bn_bwd_reduce(C.byref(j), None, None), b'st_bn_bwd_reduce', y=None, act=ops.ACT[None])


def test_signature_rows_and_struct_fields():
    assert _lib.SIGNATURES['st_bn_bwd_reduce'] == [C.POINTER(_lib.StBnBwdJob), C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES['st_bn_bwd_apply'] == [C.POINTER(_lib.StBnBwdJob), C.c_void_p]
    assert not [n for n in _lib.SIGNATURES if n.startswith('st_bn_bwd') and n not in ('st_bn_bwd_reduce', 'st_bn_bwd_apply')]
    assert [f[0] for f in _lib.StBnBwdJob._fields_] == [
        'dy', 'ldd', 'y', 'ldy', 'act', 'x', 'ldx', 'mean', 'var', 'w', 'eps', 'M', 'N', 'mask', 'ldm', 's', 'Mstat', 'inv_total', 'dx', 'lddx',
        'dres', 'lddr']


def test_builder_fills_pointers_strides_and_shape(monkeypatch):
    monkeypatch.setattr(ops, '_p', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    M, N = 7, 5
    wide = torch.zeros(M, N + 8)
    x, y, k = torch.zeros(M, N), torch.zeros(M, N + 3)[:, :N], torch.zeros(M, N)
    mean, var, w = torch.zeros(N), torch.ones(N), torch.ones(N)
    j = ops._bn_bwd_job(wide[:, 4:4 + N], y, 'tanh', x, mean, var, w, 1e-3, mask2d=k)
    assert (j.dy, j.ldd) == (wide.data_ptr() + 16, N + 8)                   # a column slice: pointer + row stride
    assert (j.y, j.ldy, j.act) == (y.data_ptr(), N + 3, ops.ACT['tanh'])
    assert (j.x, j.ldx, j.M, j.N) == (x.data_ptr(), N, M, N)
    assert (j.mean, j.var, j.w) == (mean.data_ptr(), var.data_ptr(), w.data_ptr())
    assert (j.mask, j.ldm) == (k.data_ptr(), N)
    assert j.eps == pytest.approx(1e-3, rel=1e-6)
    assert (j.s, j.Mstat, j.inv_total, j.dx, j.lddx, j.dres, j.lddr) == (None, 0, None, None, 0, None, 0)   # the halves fill their own
    j = ops._bn_bwd_job(wide[:, 4:4 + N], None, None, x, mean, var, None, 1e-3)
    assert (j.y, j.ldy, j.act) == (None, 0, 0)
    assert (j.mask, j.ldm, j.w) == (None, 0, None)
