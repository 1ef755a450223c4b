"""Which launch the attention-step backward and the BPTT loop take -- host arithmetic only, no GPU: st_attn_bwd_variant and
st_decoder_bwd_forms look at shapes, flags and pointer values and never read through them, so fake addresses stand in for the buffers.
Every row of the case tables (attn_bwd_cases.py) reaches the launch named in it, and together the rows reach every kernel, block, LDS
tier and refusal of the step, and every loop form -- the GPU test runs the rows against a float64 reference."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as T   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402

BASE = 0x1000000
ENV = ('ST_AB_NB2', 'ST_AB_NO_DUAL', 'ST_PART_KW16')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def step_code(lib, c):
    wl = BASE + (4 if c['wl'] == 'off1' else 0)
    return lib.st_attn_bwd_variant(c['L'], c['A'], c['E'], c['F'], c['K'], 1 if c['s'] else 0, c['parts'], c['hosted'], c['B'],
                                   c['N'], wl)


def step_variant(lib, c, monkeypatch):
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    for e in c['env']:
        monkeypatch.setenv(e, '1')
    return T.step_name(step_code(lib, c))


@pytest.mark.parametrize('c', T.STEP, ids=[c['id'] for c in T.STEP])
def test_step_row_reaches_its_variant(lib, c, monkeypatch):
    assert step_variant(lib, c, monkeypatch) == c['want']


def test_step_rows_cover_every_variant_and_refusal(lib, monkeypatch):
    got = [step_variant(lib, c, monkeypatch) for c in T.STEP]
    kernels = {g.split('.')[0] for g in got}
    assert kernels >= set(T.KERNELS.values()) | set(T.REFUSALS.values()), sorted(set(T.KERNELS.values()) | set(T.REFUSALS.values()) - kernels)
    ok = [g for g in got if not g.startswith('refused')]
    for kern in ('plain', 'hosted'):       # both blocks, both LDS tiers, both W_l loads, with and without the memory prefetch
        mine = [g.split('.')[1:] for g in ok if g.split('.')[0] == kern]
        assert {'w48', 'w16'} <= {f[0] for f in mine}, kern
        assert any('opt' in f for f in mine) and any('opt' not in f for f in mine), kern
    assert any('wlf' not in g for g in ok) and any('mpf' not in g for g in ok) and any('.s' not in g for g in ok)
    assert any('opt' in g for g in ok if g.startswith('parts4')) and any('opt' not in g for g in ok if g.startswith('parts4'))


def test_step_limits_at_the_full_size_attention(lib):
    """The exact L where each block stops fitting (A = 256, E = 512, F = 32, K = 31): the rows on both sides of each limit are in the
    table; here the limits themselves are pinned, and st_attn_bwd_wide_fits agrees with the hosted launch's own choice."""
    full = dict(A=256, E=512, F=32, K=31)

    def code(L, **kw):
        return T.step_name(step_code(lib, T.S('x', L, **dict(full, **kw))))
    assert code(T.WIDE_LAST).startswith('plain.w48') and code(T.WIDE_LAST + 1).startswith('plain.w16')
    assert code(T.NARROW_S_LAST).startswith('plain.w16') and code(T.NARROW_S_LAST + 1) == 'refused_lds'
    assert code(T.NARROW_LAST, s=False).startswith('plain.w16') and code(T.NARROW_LAST + 1, s=False) == 'refused_lds'
    assert code(T.WIDE_HOSTED_LAST, hosted=1).startswith('hosted.w48') and code(T.WIDE_HOSTED_LAST + 1, hosted=1).startswith('hosted.w16')
    assert code(T.HOSTED_LAST, hosted=1).startswith('hosted.') and code(T.HOSTED_LAST + 1, hosted=1).startswith('fallback.')
    for L in (1, 16, 48, 97, T.WIDE_HOSTED_LAST, T.WIDE_HOSTED_LAST + 1, 200):
        fits = lib.st_attn_bwd_wide_fits(L, 256, 512, 32, 31)
        assert fits == (1 if code(L, hosted=1).startswith('hosted.w48') else 0), L
    assert lib.st_attn_bwd_wide_fits(T.WIDE_HOSTED_LAST, 256, 512, 32, 31) == 1
    assert lib.st_attn_bwd_wide_fits(T.WIDE_HOSTED_LAST + 1, 256, 512, 32, 31) == 0
    assert lib.st_attn_bwd_variant(43, 256, 512, 32, 31, 1, 2, 0, 3, 0, BASE) == -1      # the plain entry points have no parts
    assert lib.st_attn_bwd_variant(43, 256, 512, 32, 31, 1, 1, 3, 3, 0, BASE) == -1


def forms_word(lib, c):
    d = c['dims']
    dims = _lib.StDecoderDims()
    for k in ('B', 'L', 'E', 'P', 'Q', 'D', 'A', 'F', 'K'):
        setattr(dims, k, d[k])
    dims.n_mels, dims.r = 80, 3
    io = _lib.StDecoderBwdIO()
    io.Bp = c['Bp']
    io.fuse_pw = 1 if c['fuse'] else 0
    io.overlap_attn = 1 if c['overlap'] else 0
    io.attn_s_tape = BASE if c['s_tape'] else None
    io.attn_parts, io.dloc_part = c['parts'], BASE + 0x100000
    io.dxd_splits, io.dxd_part = c['dsplits'], (BASE + 0x200000) if c['dxd_part'] else None
    io.dxq_splits, io.dxq_part = c['qsplits'], (BASE + 0x300000) if c['dxq_part'] else None
    return int(lib.st_decoder_bwd_forms(C.byref(dims), C.byref(io)))


@pytest.mark.parametrize('c', T.FORMS, ids=[c['id'] for c in T.FORMS])
def test_forms_row_reaches_its_form(lib, c):
    w = forms_word(lib, c)
    assert T.forms_name(w) == c['want'], hex(w)
    d = c['dims']
    if w & 1:       # the split form needs the wide block next to the product: the decoder asks st_attn_bwd_wide_fits
        assert lib.st_attn_bwd_wide_fits(d['L'], d['A'], d['E'], d['F'], d['K']) == 1


def test_forms_rows_cover_every_form(lib):
    got = {T.forms_name(forms_word(lib, c)) for c in T.FORMS}
    want = {'six', 'fused', 'overlap', 'split2', 'split4'} | {'split2.d%d.q4' % s for s in (1, 2, 4)} | {'split2.d2.q%d' % s for s in (1, 2, 4)}
    want |= {'split2.d2'}
    assert got >= want, sorted(want - got)
