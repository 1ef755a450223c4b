"""Which kernel the GEMM dispatchers choose -- host arithmetic only, no GPU: st_gemm_fwd_variant / st_gemm_fwd_batch_variant /
st_gemm_wgrad_variant / st_gemm_wgrad_batch_variant look at pointer values for their alignment and never read through them, so fake
addresses stand in for the buffers.  Every row of the case tables (gemm_cases.py) reaches the variant named in it, and together the rows
reach every kernel, slab count and slab sum the dispatchers can choose -- the GPU test runs each row against a float64 reference."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402

BASE_A, BASE_W, BASE_C, BASE_WS = 0x100000, 0x2000000, 0x4000000, 0x8000000


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def fwd_job(c):
    """st_gemm_job of a forward row on fake, suitably (mis)aligned addresses"""
    lib = _lib.load()
    ep = _lib.StGemmEpilogue()
    ep.w_tap_major = 1 if c['w'] == 'tm' else 0
    if c['split']:
        S = int(lib.st_gemm_splitk_slabs(c['Bn'], c['Tout'], c['Cin'], c['N'], c['KT']))
        if S > 1:
            ep.splitk_ws, ep.splitk_slabs = BASE_WS, S
    j = _lib.StGemmJob()
    j.A, j.lda = BASE_A + 4 * G.a_offset(c), G.lda_of(c)
    j.W = BASE_W + 4 * G.w_offset(c)
    j.C, j.ldc, j.coff = BASE_C, c['N'] + 8, 4
    j.Bn, j.Tin, j.Tout, j.Cin, j.N, j.KT = c['Bn'], c['Tin'], c['Tout'], c['Cin'], c['N'], c['KT']
    j.pad, j.stride, j.pool_prev, j.ep = c['pad'], c['stride'], 1 if c['pool'] else 0, ep
    return j


def fwd_variant(c):
    lib = _lib.load()
    j = fwd_job(c)
    code = lib.st_gemm_fwd_variant(j.A, j.lda, j.W, j.C, j.ldc, j.coff, j.Bn, j.Tin, j.Tout, j.Cin, j.N, j.KT, j.pad, j.stride,
                                   j.pool_prev, C.byref(j.ep))
    return G.fwd_name(code)


def fwd_batch_variant(b):
    lib = _lib.load()
    arr = (_lib.StGemmJob * len(b['jobs']))(*[fwd_job(c) for c in b['jobs']])
    bits = lib.st_gemm_fwd_batch_variant(arr, len(b['jobs']))
    assert bits > 0, bits
    return '|'.join(n for k, n in sorted(G.FWD_BATCH_BITS.items()) if bits & k)


def wgrad_args(c):
    lddc, dcoff = G.dc_layout(c)
    lda = G.lda_of(dict(c, a=c['a']))
    return BASE_C + (4 if c['dc'] == 'odd' else 0), lddc, dcoff, BASE_A, lda


def wgrad_variant(c):
    lib = _lib.load()
    dC, lddc, dcoff, A, lda = wgrad_args(c)
    code = lib.st_gemm_wgrad_variant(dC, lddc, dcoff, A, lda, c['Bn'], c['Tin'], c['Tout'], c['Cin'], c['N'], c['KT'], c['pad'],
                                     1 if c['pool'] else 0, 1 if c['acc'] else 0, 1 if c['db'] else 0, 1 if c['split'] else 0)
    return code


def wgrad_batch_codes(jobs):
    lib = _lib.load()
    arr = (_lib.StWgradJob * len(jobs))()
    for q, c in zip(arr, jobs):
        q.dC, q.lddc, q.dcoff, q.A, q.lda = wgrad_args(c)
        q.dW, q.db = BASE_W, BASE_WS if c['db'] else None
        q.Bn, q.Tin, q.Tout, q.Cin, q.N, q.KT, q.pad = c['Bn'], c['Tin'], c['Tout'], c['Cin'], c['N'], c['KT'], c['pad']
    codes = (C.c_int * len(jobs))()
    groups = lib.st_gemm_wgrad_batch_variant(arr, len(jobs), codes)
    return groups, list(codes)


@pytest.mark.parametrize('c', G.FWD, ids=[c['id'] for c in G.FWD])
def test_fwd_row_reaches_its_variant(lib, c):
    assert fwd_variant(c) == c['want']


@pytest.mark.parametrize('b', G.FWD_BATCH, ids=[b['id'] for b in G.FWD_BATCH])
def test_fwd_batch_row_reaches_its_variant(lib, b):
    assert fwd_batch_variant(b) == b['want']


@pytest.mark.parametrize('c', G.WGRAD, ids=[c['id'] for c in G.WGRAD])
def test_wgrad_row_reaches_its_variant(lib, c):
    assert G.wgrad_name(wgrad_variant(c)) == c['want']


def test_every_variant_is_reached(lib):
    """the rows together reach every forward kernel (the LDS-DMA tiles, the 8 pipelined forms, the element-wise and one-block forms),
    split-K with every slab count 2..8 on both kernels that take it and both finishes, every batch form, every weight-gradient product
    with each of its layout flags, every slab sum with and without accumulate, Z = 1 direct writes, and a weight-gradient batch with
    group launches, single calls in between and a group of one"""
    fwd = [fwd_variant(c) for c in G.FWD]
    kernels = {v.split('/')[0] for v in fwd}
    assert kernels == set(G.FWD_KERNELS.values()), sorted(set(G.FWD_KERNELS.values()) - kernels)
    slabs = {int(v.split('/')[1][1:]) for v in fwd if '/S' in v}
    assert slabs == set(range(2, 9)), slabs
    assert {v.split('/')[2] for v in fwd if '/S' in v} == {'fin4', 'fin1'}
    assert {v.split('/')[0] for v in fwd if '/S' in v} >= {'gd64x64', 'pipe_vw0_pl0_mt2', 'pipe_vw0_pl1_mt2', 'pipe_vw1_pl0_mt2',
                                                           'pipe_vw1_pl1_mt2'}
    assert any(c['stride'] == 2 and c['Tin'] % 2 == 1 for c in G.FWD)
    bits = set()
    for b in G.FWD_BATCH:
        bits |= set(fwd_batch_variant(b).split('|'))
    assert bits == set(G.FWD_BATCH_BITS.values()), bits
    assert max(len(b['jobs']) for b in G.FWD_BATCH) > 8

    wg = [(wgrad_variant(c), c) for c in G.WGRAD]
    names = [G.wgrad_name(code) for code, _ in wg]
    assert {n.split('+')[0].split('/')[0] for n in names} == set(G.WG_PRODUCTS.values())
    for flag in ('fold', 'lin', 'pool', 'direct'):
        assert any('+' + flag in n for n in names), flag
    for s in ('partials', 'tall', 'partials2', 'partials2_split'):
        for acc in (False, True):
            assert any(n.endswith('/' + s) and c['acc'] == acc for n, (_, c) in zip(names, wg)), (s, acc)
    assert any(c['split'] and c['db'] for c in G.WGRAD) and any(c['split'] and not c['db'] for c in G.WGRAD)
    assert any(G.wgrad_z(code) >= 64 for code, _ in wg)

    for b in G.WGRAD_BATCH:
        jobs = b['jobs']
        assert len(jobs) > 16
        groups, codes = wgrad_batch_codes(jobs)
        assert groups >= 1 and codes.count(1) == 16, codes      # a full group of 16
        grouped = [c for c, k in zip(jobs, codes) if k]
        alone = [c for c, k in zip(jobs, codes) if not k]
        # single calls in between, Z = 1 jobs and a tall-sum job inside a group, and a groupable job left alone (a group of one)
        assert alone and any(G.wgrad_name(wgrad_variant(c)).endswith('+direct') for c in grouped)
        assert any(G.wgrad_name(wgrad_variant(c)).endswith('/tall') for c in grouped)
        assert any(G.wgrad_name(wgrad_variant(c)).startswith('dma64') for c in alone)


def test_variant_queries_refuse_bad_arguments(lib):
    ep = _lib.StGemmEpilogue()
    assert lib.st_gemm_fwd_variant(BASE_A, 8, BASE_W, BASE_C, 8, 0, 1, 10, 10, 16, 8, 1, 0, 1, 0, C.byref(ep)) < 0      # lda < Cin
    ep.splitk_ws, ep.splitk_slabs = BASE_WS, 3          # a slab count that is not st_gemm_splitk_slabs()'s
    assert lib.st_gemm_fwd_variant(BASE_A, 1536, BASE_W, BASE_C, 257, 0, 1, 63, 63, 1536, 257, 1, 0, 1, 0, C.byref(ep)) < 0
    assert lib.st_gemm_wgrad_variant(BASE_C, 8, 0, BASE_A, 8, 1, 10, 10, 8, 0, 1, 0, 0, 0, 0, 0) < 0                  # N = 0
