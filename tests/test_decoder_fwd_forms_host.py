"""Which forms the decode loop (st_decoder_forward) takes -- host arithmetic only, no GPU: st_decoder_fwd_forms looks at shapes, flags,
pointer values and the host array step_src and never reads through the device pointers, so fake addresses stand in for the buffers.
Every row of the table reaches the forms named in it, and together the rows reach every attention form, every host of the decoder
cell's partial gate product, paired cells, deferred projection and the fall-back when a workgroup budget does not fit the device.

The second half does the same for decoder_fwd_cases.CASES, the small-size cases that tests/test_gpu_decoder_fwd_forms.py runs on the GPU
against float64: st_decoder_io filled the way Decoder._run_loop fills it for the case's knobs and mode, on an MI355X's 256 compute units."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_fwd_cases as FC   # noqa: E402
from helpers import FWD_ATTN as ATTN, FWD_PROD as PROD, fwd_forms as decode   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402

BASE = 0x1000000
# dims of the full-size decoder (helpers.FULL_CFG): P 256, Q = D = 1024, E 512, A 256, F 32, K 31; the C2 headline text length
FULL_DIMS = dict(B=32, L=43, E=512, P=256, Q=1024, D=1024, A=256, F=32, K=31)
C2_CUS, C2_RNG = 256, 512          # MI355X: 256 compute units, two range workgroups per compute unit
# the hosted product beside pq + fin: 16 * 2 pq workgroups + 32 * 2 fin workgroups + 4096 / 32 product workgroups; the same count
# beside pq + attention pre (16 * 2 + 32 * 2 pre workgroups + 128)
HOSTED_CUS = 16 * 2 + 32 * 2 + 4096 // 32
assert HOSTED_CUS == 224
C2_WORD = 3 | (2 << 4) | (2 << 12) | (80 << 16)     # pq + fin, product beside it, 2 fin parts, the cell keeps 80 of 160 k-blocks


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def R(id, want, mode='free', steps=10, s_buf=True, fin_parts=2, pre_parts=4, split_parts=0, xchg=False, pq_gran=True, gate_part=True,
      gate_part_k=0, defer=False, pair=False, Bt=None, cus=C2_CUS, rng=C2_RNG, **dims):
    """one row: `want` = (attention form, product host, flags) with flags a subset of {'tf', 'defer', 'pre_in_pq', 'pair'}"""
    return dict(id=id, want=want, mode=mode, steps=steps, s_buf=s_buf, fin_parts=fin_parts, pre_parts=pre_parts, split_parts=split_parts,
                xchg=xchg, pq_gran=pq_gran, gate_part=gate_part, gate_part_k=gate_part_k, defer=defer, pair=pair, Bt=Bt, cus=cus, rng=rng,
                dims=dict(FULL_DIMS, **dims))


def forms_word(lib, c):
    d = c['dims']
    dims = _lib.StDecoderDims()
    for k in ('B', 'L', 'E', 'P', 'Q', 'D', 'A', 'F', 'K'):
        setattr(dims, k, d[k])
    dims.n_mels, dims.r = 80, 3
    steps, Tt = c['steps'], c['steps']
    io = _lib.StDecoderIO()
    io.steps = steps
    # the one host array the planner reads: -1 = own output; a teacher-forced step t takes teacher frame min(t, Tt - 1)
    src = [-1] * steps if c['mode'] == 'free' else [min(t, Tt - 1) for t in range(steps)]
    src_arr = (C.c_int * steps)(*src)
    io.step_src = C.cast(src_arr, C.POINTER(C.c_int))
    if c['mode'] != 'free':
        io.teacher_pre, io.Tt = BASE + 0x10000, Tt
        io.Bt = d['B'] if c['Bt'] is None else c['Bt']
    io.defer_proj, io.pair_cells = int(c['defer']), int(c['pair'])
    io.attn_s_buf = BASE + 0x100000 if c['s_buf'] else None
    io.attn_fin_parts, io.attn_pre_parts = c['fin_parts'], c['pre_parts']
    if c['split_parts']:
        io.attn_split_ws, io.attn_split_parts = BASE + 0x200000, c['split_parts']
    io.pq_granules = BASE + 0x300000 if c['pq_gran'] else None
    io.attn_xchg = BASE + 0x400000 if c['xchg'] else None
    gp = c['gate_part']
    io.gate_part = None if not gp else BASE + 0x500000 + (4 if gp == 'misaligned' else 0)
    io.gate_part_k = c['gate_part_k']
    return int(lib.st_decoder_fwd_forms(C.byref(dims), C.byref(io), c['cus'], c['rng']))


TF = dict(mode='tf', defer=True, pair=True, pq_gran=False)      # the teacher-forced training step (tapes kept, projection deferred)
C5 = dict(B=64, L=171, split_parts=4, xchg=True)     # the long-text workload: 4 position ranges of 43
TRAIN = {'tf', 'defer', 'pre_in_pq', 'pair'}

ROWS = [
    R('c2', ('pq_fin', 'pq_fin', set())),
    R('c2_224_cus', ('pq_fin', 'pq_fin', set()), cus=HOSTED_CUS),
    R('c2_223_cus', ('pq_fin', 'own', set()), cus=HOSTED_CUS - 1),
    R('pq_fin_96_cus', ('pq_fin', 'own', set()), cus=16 * 2 + 32 * 2),
    R('pq_fin_95_cus', ('pre_fin', 'own', set()), cus=16 * 2 + 32 * 2 - 1),
    R('fin_parts4', ('pq_fin', 'own', set()), fin_parts=4),                # 32 + 128 fin workgroups: no room for the product
    R('fin_parts8', ('pre_fin', 'own', set()), fin_parts=8),               # 32 + 256: pq + fin does not fit either
    R('fin_parts3', ('pq_fin', 'pq_fin', set()), fin_parts=3),             # (not 1, 2, 4 or 8: one part)
    R('no_pq_granules', ('pre_fin', 'own', set()), pq_gran=False),
    R('no_s_buf', ('whole', 'own', set()), s_buf=False, pq_gran=False),
    R('no_gate_part', ('pq_fin', 'none', set()), gate_part=False),
    R('misaligned_gate_part', ('pq_fin', 'none', set()), gate_part='misaligned'),
    R('b16', ('pq_fin', 'none', set()), B=16),
    R('b17', ('pq_fin', 'pq_fin', set()), B=17),
    R('b33', ('pq_fin', 'none', set()), B=33),
    R('a_not_16', ('pre_fin', 'own', set()), A=200),
    R('c5', ('pq_rng', 'none', set()), **C5),
    R('c5_rng_320', ('pq_rng', 'none', set()), rng=16 * 4 + 64 * 4, **C5),
    R('c5_rng_319', ('fin_split', 'none', set()), rng=16 * 4 + 64 * 4 - 1, **C5),
    R('c5_no_xchg', ('fin_split', 'none', set()), **dict(C5, xchg=False)),
    R('long_b32', ('pq_rng', 'own', set()), L=171, split_parts=4, xchg=True),
    R('split_parts16', ('fin_split', 'own', set()), L=688, split_parts=16, xchg=True),
    R('train', ('pre_fin', 'pq_pre', TRAIN), **TF),
    R('train_224_cus', ('pre_fin', 'pq_pre', TRAIN), cus=HOSTED_CUS, **TF),
    R('train_223_cus', ('pre_fin', 'own', TRAIN), cus=HOSTED_CUS - 1, **TF),
    R('train_pre_parts1', ('pre_fin', 'pq_pre', TRAIN), pre_parts=1, cus=HOSTED_CUS - 32, **TF),
    R('train_unpaired', ('pre_fin', 'pq_pre', {'tf', 'defer', 'pre_in_pq'}), **dict(TF, pair=False)),
    R('train_no_s_buf', ('whole', 'none', {'tf', 'defer', 'pair'}), s_buf=False, **TF),
    R('train_no_gate_part', ('pre_fin', 'none', TRAIN), gate_part=False, **TF),
    R('tf_eager', ('pq_fin', 'pq_fin', {'tf'}), mode='tf'),                # teacher forcing without deferral: the inference forms
    R('tf_partial_rows', ('pq_fin', 'pq_fin', set()), mode='tf', Bt=20),    # some rows feed their own output: not pure
    R('single_step', ('pq_fin', 'pq_fin', set()), steps=1),
]


@pytest.mark.parametrize('c', ROWS, ids=[c['id'] for c in ROWS])
def test_row_reaches_its_forms(lib, c):
    w = forms_word(lib, c)
    assert decode(w) == c['want'], hex(w)
    fp = c['fin_parts'] if c['fin_parts'] in (2, 4, 8) else 1
    assert (w >> 12) & 15 == fp, hex(w)


def test_rows_cover_every_form(lib):
    got = [decode(forms_word(lib, c)) for c in ROWS]
    assert {g[0] for g in got} == set(ATTN)
    assert {g[1] for g in got} == set(PROD)
    assert {(g[0], g[1]) for g in got} >= {('pq_fin', 'pq_fin'), ('pre_fin', 'pq_pre'), ('pq_rng', 'own'), ('fin_split', 'own'),
                                            ('whole', 'own'), ('pre_fin', 'own'), ('pq_fin', 'own')}
    flags = set().union(*(g[2] for g in got))
    assert flags == TRAIN


def test_c2_headline_word(lib):
    """the free-running C2 step at 256 compute units: pq + fin as one launch with the decoder cell's product beside it, 2 fin
    workgroups per utterance, the cell keeping 80 of its 160 k-blocks (st_decoder_gate_split_k: 1280 of 2560 columns)"""
    assert forms_word(lib, ROWS[0]) == C2_WORD
    dims = _lib.StDecoderDims(**{k: v for k, v in FULL_DIMS.items()}, n_mels=80, r=3)
    assert lib.st_decoder_gate_split_k(C.byref(dims)) == 16 * 80


def test_explicit_cell_share(lib):
    """gate_part_k sets the cell's share; bits 16.. carry it in k-blocks, and only with a partial product"""
    assert forms_word(lib, R('k', None, gate_part_k=512)) >> 16 == 32
    assert forms_word(lib, R('k', None, gate_part_k=512, gate_part=False)) >> 16 == 0
    assert forms_word(lib, R('k', None, gate_part_k=2048, **TF)) >> 16 == 128


def test_null_arguments(lib):
    io = _lib.StDecoderIO()
    io.steps = 4               # more than one step and no step_src: nothing to plan from
    dims = _lib.StDecoderDims(**FULL_DIMS, n_mels=80, r=3)
    assert lib.st_decoder_fwd_forms(None, None, 256, 512) == -1
    assert lib.st_decoder_fwd_forms(C.byref(dims), C.byref(io), 256, 512) == -1


# ------------------------------------------------------------------------------------ the cases the GPU test runs
def case_word(lib, c):
    """the planner's word for a decoder_fwd_cases case: the io fields of decoder_fwd_cases.io_plan, fake addresses for the buffers"""
    p = FC.io_plan(c)
    dims = _lib.StDecoderDims(B=c['B'], L=c['L'], n_mels=FC.COMMON['n_mels'], r=FC.COMMON['r'], F=FC.COMMON['F'], K=FC.COMMON['K'],
                              **FC.DIMS[c['dims']])
    io = _lib.StDecoderIO()
    io.steps = p['steps']
    src_arr = (C.c_int * p['steps'])(*p['step_src'])
    io.step_src = C.cast(src_arr, C.POINTER(C.c_int))
    if p['teacher']:
        io.teacher_pre, io.Tt = BASE + 0x10000, p['Tt']
    io.Bt = p['Bt']
    io.defer_proj, io.pair_cells = int(p['defer']), int(p['pair'])
    io.attn_s_buf = BASE + 0x100000 if p['s_buf'] else None
    io.attn_fin_parts, io.attn_pre_parts = p['fin_parts'], p['pre_parts']
    if p['split_parts']:
        io.attn_split_ws, io.attn_split_parts = BASE + 0x200000, p['split_parts']
    io.pq_granules = BASE + 0x300000 if p['pq_gran'] else None
    io.attn_xchg = BASE + 0x400000 if p['xchg'] else None
    io.gate_part = BASE + 0x500000 if p['gate_part'] else None
    io.gate_part_k = p['gate_part_k']
    return int(lib.st_decoder_fwd_forms(C.byref(dims), C.byref(io), FC.CUS, FC.RNG_CAPACITY))


def word_fields(w):
    """(forms, fin parts, k0) of a planner word"""
    return decode(w), (w >> 12) & 15, w >> 16


@pytest.mark.parametrize('c', FC.CASES, ids=FC.IDS)
def test_case_reaches_its_forms(lib, c):
    w = case_word(lib, c)
    assert word_fields(w) == (c['want'], c['fp'], c['k0']), hex(w)


def test_cases_cover_every_form(lib):
    got = [word_fields(case_word(lib, c)) for c in FC.CASES]
    assert {g[0][0] for g in got} == set(ATTN)
    assert {g[0][1] for g in got} == set(PROD)
    assert {g[1] for g in got} == {1, 2, 4, 8}
    assert set().union(*(g[0][2] for g in got)) == TRAIN
    assert len({g[2] for g in got if g[0][1] != 'none'}) >= 2                # cuts of the cell's reduction
    # every fused form beside every host it can have at these sizes, and each mode behind the forms it is meant to reach
    assert {(g[0][0], g[0][1]) for g in got} >= {('pq_fin', 'pq_fin'), ('pq_fin', 'none'), ('pre_fin', 'pq_pre'), ('pre_fin', 'own'),
                                                  ('pre_fin', 'none'), ('pq_rng', 'none'), ('fin_split', 'none'), ('whole', 'none')}
    by_mode = {}
    for c, g in zip(FC.CASES, got):
        by_mode.setdefault(c['mode'], set()).add((g[0][0], g[0][1]))
    assert set(by_mode) == set(FC.MODES)
    assert ('pq_fin', 'pq_fin') in by_mode['tf_eval'] and ('pq_fin', 'pq_fin') in by_mode['tf_partial']
    for ds in FC.DIMS:                  # every dims set has a case with expanding dynamics
        assert any(c['dims'] == ds and c['gain'] != 1.0 for c in FC.CASES), ds
    assert any(c['steps'] == 1 for c in FC.CASES) and any(c['B'] == 1 and c['L'] == 1 for c in FC.CASES)


def test_cases_cover_every_cut_the_loop_accepts(lib):
    """split_cell_k at M16: every multiple of 16 in the range st_decoder_forward accepts, [16 * ceil(E / 16), 16 * (k-blocks of the cell))"""
    d = FC.DIMS['M16']
    lo, hi = 16 * ((d['E'] + 15) // 16), 16 * sum((d[k] + 15) // 16 for k in ('E', 'Q', 'D'))
    cuts = {c['knobs']['split_cell_k'] for c in FC.CASES if c['dims'] == 'M16' and c['mode'] == 'free' and 'split_cell_k' in c['knobs']}
    assert cuts == set(range(lo, hi, 16))
    dims = _lib.StDecoderDims(B=20, L=11, n_mels=8, r=2, F=8, K=7, **d)
    assert lib.st_decoder_gate_split_k(C.byref(dims)) == 16 * FC.cell_k0('M16')


def test_bit_identical_pairs_share_everything_but_the_form():
    for a, b in FC.BIT_IDENTICAL:
        ca, cb = FC.BY_ID[a], FC.BY_ID[b]
        same = ('dims', 'B', 'L', 'steps', 'mode', 'Bt', 'gain', 'k0')
        assert [ca[k] for k in same] == [cb[k] for k in same], (a, b)
        assert ca['want'][:2] == ('pq_fin', 'pq_fin') and cb['want'][:2] == ('pre_fin', 'own')
