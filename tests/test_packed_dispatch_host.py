"""Which launch a forward product on packed operands takes -- host arithmetic only, no GPU: st_packed_fwd_variant looks at shapes and
never touches memory, and pk_dispatch, st_lstm_cell_packed_pair_fwd and pk_linear_impl (skinny_packed.hip) take their decision from the
functions it calls.  Every row of the case tables (packed_cases.py) reaches the launch named in it, the rule restated there agrees with
the library over a sweep of shapes, together the rows reach every instantiation the three launchers can launch, the P16 / T16 index
functions are bijections onto the non-pad slots, and the float64 references agree with float64 torch -- the GPU test
(test_gpu_packed_products.py) runs the rows against those references."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_cases as PC   # noqa: E402
from semi_tts_amd import _lib   # noqa: E402


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsemitts_hip.so is not built (python -m semi_tts_amd.build)')
    return _lib.load()


def variant(lib, mode, B, n, **kw):
    """[(family, nb, grid_x, grid_y, vec)] as the library reports it, None for a refusal"""
    q = _lib.StPackedFwdQuery(mode=mode, B=B, n=n, pre_aligned=1)
    for k, v in kw.items():
        setattr(q, k, v)
    out = (_lib.StPackedFwdLaunch * 2)()
    n_launch = lib.st_packed_fwd_variant(C.byref(q), out)
    if n_launch < 0:
        return None
    return [(PC.FAMILIES[o.family], o.nb, o.grid_x, o.grid_y, o.vec) for o in out[:n_launch]]


def at_kw(c):
    return dict(pre_parts=c['parts'], pre_A=c['A'], pre_F=c['F'], part_n=4 * PC.PART_H if c['part'] else 0)


def all_row_launches(lib):
    got = [variant(lib, PC.MODE_LINEAR, c['B'], c['N'])[0] for c in PC.LINEAR]
    got += [variant(lib, PC.MODE_CELL, c['B'], c['H'])[0] for c in PC.CELL]
    for c in PC.CELL_PAIR:
        j0, j1 = c['jobs']
        got += variant(lib, PC.MODE_PAIR, j0['B'], j0['H'], B1=j1['B'], n1=j1['H'])
    got += [variant(lib, PC.MODE_LINEAR, c['B'], c['N'], **at_kw(c))[0] for c in PC.ATTNPRE]
    return got


# ------------------------------------------------------------------------------------------------ rows reach their launches
@pytest.mark.parametrize('c', PC.LINEAR, ids=[c['id'] for c in PC.LINEAR])
def test_linear_row_reaches_its_launch(lib, c):
    assert variant(lib, PC.MODE_LINEAR, c['B'], c['N']) == [c['want'] + (0,)]
    assert PC.plan(PC.MODE_LINEAR, c['B'], c['N']) == [c['want'] + (0,)]


@pytest.mark.parametrize('c', PC.CELL, ids=[c['id'] for c in PC.CELL])
def test_cell_row_reaches_its_launch(lib, c):
    assert variant(lib, PC.MODE_CELL, c['B'], c['H']) == [c['want'] + (0,)]


@pytest.mark.parametrize('c', PC.CELL_PAIR, ids=[c['id'] for c in PC.CELL_PAIR])
def test_pair_row_reaches_its_launches(lib, c):
    j0, j1 = c['jobs']
    assert variant(lib, PC.MODE_PAIR, j0['B'], j0['H'], B1=j1['B'], n1=j1['H']) == [w + (0,) for w in c['want']]


@pytest.mark.parametrize('c', PC.ATTNPRE, ids=[c['id'] for c in PC.ATTNPRE])
def test_attnpre_row_reaches_its_launch(lib, c):
    assert variant(lib, PC.MODE_LINEAR, c['B'], c['N'], **at_kw(c)) == [c['want']]
    # an operand that is not 16-byte aligned takes the element-wise attention kernel whatever A and F are
    assert variant(lib, PC.MODE_LINEAR, c['B'], c['N'], pre_aligned=0, **at_kw(c)) == [c['want'][:4] + (0,)]


def test_rows_reach_every_instantiation(lib):
    """pk_dispatch: pk_kernel<mode, 1..4> for both modes and pk_lstm_rt2_kernel<1 | 2>; the pair entry: the pair kernel and the
    fall-back; pk_launch_attnpre<1..4> with both attention kernels, the hosted partial product with both"""
    cells = {variant(lib, PC.MODE_CELL, c['B'], c['H'])[0][:2] for c in PC.CELL}
    assert cells == {('pk_kernel', nb) for nb in (1, 2, 3, 4)} | {('pk_lstm_rt2', 1), ('pk_lstm_rt2', 2)}
    lin = {variant(lib, PC.MODE_LINEAR, c['B'], c['N'])[0][:2] for c in PC.LINEAR}
    assert lin == {('pk_kernel', nb) for nb in (1, 2, 3, 4)}
    pairs = [variant(lib, PC.MODE_PAIR, c['jobs'][0]['B'], c['jobs'][0]['H'], B1=c['jobs'][1]['B'], n1=c['jobs'][1]['H']) for c in PC.CELL_PAIR]
    assert {len(p) for p in pairs} == {1, 2} and any(p[0][0] == 'pk_lstm_rt2_pair' for p in pairs)
    at = {(v[0], v[1], v[4]) for v in (variant(lib, PC.MODE_LINEAR, c['B'], c['N'], **at_kw(c))[0] for c in PC.ATTNPRE)}
    assert at == {('pk_attnpre', nb, vec) for nb in (1, 2, 3, 4) for vec in (0, 1)} | {('pk_attnpre_part', 1, 0), ('pk_attnpre_part', 1, 1)}
    # aliasing of surplus batch tiles: a second grid row that starts past BT - nb, for the linear, the cell and the attention-pre form
    for rows, key, mode in ((PC.LINEAR, 'N', PC.MODE_LINEAR), (PC.CELL, 'H', PC.MODE_CELL)):
        assert any(c['want'][1] > 1 and c['want'][3] * c['want'][1] > (c['B'] + 15) // 16 for c in rows), key
    assert any(c['want'][1] == 4 and c['B'] > 64 for c in PC.ATTNPRE)


def test_linear_rows_cover_the_k_loop_and_the_epilogues():
    """the K loop: 1..4 load groups, ragged last groups, a rotated start (up to group 2), the epilogue operands requested before the loop
    and inside it; NB > 1 rows once with K = 16 and once with a ragged k-block count; every epilogue variant the issue lists"""
    kbs = {sum(PC.kb16(k) for k in c['Ks']) for c in PC.LINEAR if c['want'][1] == 1}
    assert {1, 15, 16, 17, 32, 33, 48, 49} <= kbs and {PC.k_groups(kb) for kb in kbs} >= {1, 2, 3, 4}
    rots = {PC.k_rot(t, sum(PC.kb16(k) for k in c['Ks'])) for c in PC.LINEAR for t in range(c['want'][2])}
    assert rots >= {0, 1, 2}
    late = [c for c in PC.LINEAR if PC.k_groups(sum(PC.kb16(k) for k in c['Ks'])) >= 3]
    assert any(sum(PC.kb16(k) for k in c['Ks']) % PC.STEP for c in late)          # epi_late with a ragged last group
    for nb in (2, 3, 4):
        mine = [c for c in PC.LINEAR if c['want'][1] == nb]
        assert any(c['Ks'] == (16,) for c in mine) and any(sum(PC.kb16(k) for k in c['Ks']) % 16 for c in mine), nb
    es = [c['epi'] for c in PC.LINEAR]
    assert {e['act'] for e in es} == set(PC.ACT) and {e['out'] for e in es} == {'y', 't16', 'both'}
    assert {e['y_way'] for e in es if e['out'] != 't16'} == {'vec', 'ld', 'ptr'}
    assert any(e['mask'] for e in es) and any(not e['bias'] for e in es) and any(e['ydst_kb0'] > 0 for e in es if e['out'] != 'y')
    assert any(e['split'] and e['split'][1] > 1 for e in es)
    thirds = [e for e in es if e['third']]
    assert any(e['third'][0] % 4 == 0 for e in thirds) and any(e['third'][0] % 4 for e in thirds) and any(not e['split'] for e in thirds)
    assert any(e['split'] and e['split'][0] % 4 for e in thirds) and any(e['third'][2] for e in thirds) and any(not e['third'][2] for e in thirds)


def test_cell_rows_cover_the_operand_and_destination_subsets():
    for fam in ('pk_kernel', 'pk_lstm_rt2'):
        mine = [c for c in PC.CELL if c['want'][0] == fam]
        assert {c['absent'] for c in mine} == set(PC.CELL_ABSENT) and {c['dests'] for c in mine} == set(PC.CELL_DESTS), fam
        assert any(c['wide_ld'] for c in mine) and any(c['saturate'] for c in mine), fam
    assert {c['B'] for c in PC.CELL} >= {5, 17, 20, 32, 33, 48, 49, 64, 70}


# ------------------------------------------------------------------------------------------------ the rule itself
def test_python_rule_agrees_with_the_library_on_a_sweep(lib):
    bad = []
    for B in range(1, 81):
        for tiles in range(1, 601):
            N = 16 * tiles - (B + tiles) % 16           # every N of the tile in turn
            if variant(lib, PC.MODE_LINEAR, B, N) != PC.plan(PC.MODE_LINEAR, B, N):
                bad.append(('linear', B, N))
            for parts in (1, 2):
                kw = dict(pre_parts=parts, pre_A=16 + 4 * (tiles % 2) + (B % 3 == 0), pre_F=4 - (tiles % 3 == 0))
                if variant(lib, PC.MODE_LINEAR, B, N, **kw) != PC.plan(PC.MODE_LINEAR, B, N, **kw):
                    bad.append(('attnpre', B, N, parts))
            if tiles <= 150:
                kw = dict(pre_parts=1, pre_A=16, pre_F=4, part_n=32 * (1 + tiles % 3) - (16 if tiles % 7 == 0 else 0))
                if variant(lib, PC.MODE_LINEAR, B, N, **kw) != PC.plan(PC.MODE_LINEAR, B, N, **kw):
                    bad.append(('part', B, N))
            if tiles <= 40:
                H = 4 * tiles
                if variant(lib, PC.MODE_CELL, B, H) != PC.plan(PC.MODE_CELL, B, H):
                    bad.append(('cell', B, H))
                for B1, H1 in ((20, 8), (32, 12), (B, H), (33, 16)):
                    if variant(lib, PC.MODE_PAIR, B, H, B1=B1, n1=H1) != PC.plan(PC.MODE_PAIR, B, H, B1=B1, n1=H1):
                        bad.append(('pair', B, H, B1, H1))
    assert not bad, bad[:10]


def test_no_launch_spans_batch_tiles_that_do_not_exist(lib):
    """pk_body<mode, NB> reads NB batch tiles from batch tile max(BT - NB, 0) on through one descriptor: nb <= BT always, or the loads
    run past the T16 buffer (the uncapped rule gave B = 17..32 with more than 512 row tiles nb = 4).  And the grid covers every tile"""
    for B in range(1, 81):
        BT = (B + 15) // 16
        for tiles in list(range(1, 40)) + list(range(120, 140)) + list(range(250, 262)) + list(range(505, 520)) + [600, 1024, 4096]:
            for v in (variant(lib, PC.MODE_LINEAR, B, 16 * tiles)[0], variant(lib, PC.MODE_LINEAR, B, 16 * tiles, pre_parts=1, pre_A=16, pre_F=4)[0],
                      variant(lib, PC.MODE_CELL, B, 4 * tiles)[0]):
                fam, nb, gx, gy, _ = v
                assert 1 <= nb <= min(BT, 4), (B, tiles, v)
                if fam == 'pk_kernel':
                    assert gx == tiles and gy == -(-BT // nb), (B, tiles, v)
                elif fam == 'pk_lstm_rt2':
                    assert gx * 2 == tiles and gy * nb == BT, (B, tiles, v)
                else:
                    assert gx == tiles * -(-BT // nb) + B, (B, tiles, v)
    # the fewest batch tiles per workgroup that keep the grid within 512 workgroups, on both sides of each step
    assert variant(lib, PC.MODE_LINEAR, 33, 16 * 170)[0][:4] == ('pk_kernel', 1, 170, 3)
    assert variant(lib, PC.MODE_LINEAR, 33, 16 * 171)[0][:4] == ('pk_kernel', 2, 171, 2)
    assert variant(lib, PC.MODE_LINEAR, 33, 16 * 256)[0][:4] == ('pk_kernel', 2, 256, 2)
    assert variant(lib, PC.MODE_LINEAR, 33, 16 * 257)[0][:4] == ('pk_kernel', 3, 257, 1)
    assert variant(lib, PC.MODE_LINEAR, 64, 16 * 128)[0][:4] == ('pk_kernel', 1, 128, 4)
    assert variant(lib, PC.MODE_LINEAR, 64, 16 * 129)[0][:4] == ('pk_kernel', 2, 129, 2)
    assert variant(lib, PC.MODE_LINEAR, 64, 16 * 257)[0][:4] == ('pk_kernel', 4, 257, 1)
    assert variant(lib, PC.MODE_LINEAR, 20, 16 * 256)[0][:4] == ('pk_kernel', 1, 256, 2)
    assert variant(lib, PC.MODE_LINEAR, 20, 16 * 257)[0][:4] == ('pk_kernel', 2, 257, 1)
    assert variant(lib, PC.MODE_LINEAR, 20, 16 * 513)[0][:4] == ('pk_kernel', 2, 513, 1)       # was 4
    assert variant(lib, PC.MODE_LINEAR, 33, 16 * 513)[0][:4] == ('pk_kernel', 3, 513, 1)       # was 4
    assert variant(lib, PC.MODE_LINEAR, 16, 16 * 4096)[0][:4] == ('pk_kernel', 1, 4096, 1)


def test_refusals(lib):
    assert variant(lib, PC.MODE_LINEAR, 0, 16) is None and variant(lib, PC.MODE_LINEAR, 4, 0) is None and variant(lib, 3, 4, 16) is None
    assert variant(lib, PC.MODE_CELL, 4, 6) is None and variant(lib, PC.MODE_PAIR, 20, 8, B1=20, n1=6) is None
    assert variant(lib, PC.MODE_LINEAR, 20, 33, part_n=32) is None                                    # a slab without the attention-pre job
    assert variant(lib, PC.MODE_LINEAR, 20, 16 * 129, pre_parts=1, pre_A=16, pre_F=4, part_n=32) is None      # more than 128 row tiles
    assert variant(lib, PC.MODE_LINEAR, 16, 33, pre_parts=1, pre_A=16, pre_F=4, part_n=32) is None
    assert variant(lib, PC.MODE_LINEAR, 33, 33, pre_parts=1, pre_A=16, pre_F=4, part_n=32) is None
    assert variant(lib, PC.MODE_LINEAR, 20, 33, pre_parts=1, pre_A=16, pre_F=4, part_n=48) is None
    assert lib.st_packed_fwd_variant(None, None) == -1


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('c', PC.PACK_CASES + PC.PACK_BATCH[1:], ids=[c['id'] for c in PC.PACK_CASES + PC.PACK_BATCH[1:]])
def test_p16_index_is_a_bijection_onto_the_logical_slots(c):
    pos = torch.cat([p.reshape(-1) for p in PC.p16_positions(c['ks'], c['N'], c['lstm_H'])])
    total = PC.p16_floats(c['ks'], c['N'], c['lstm_H'])
    assert pos.numel() == c['N'] * sum(c['ks']) == pos.unique().numel() and int(pos.min()) >= 0 and int(pos.max()) < total
    # the image puts every value at its slot and zero everywhere else; the slot arithmetic read backwards gives (row, k) again
    ws = [torch.arange(1, c['N'] * k + 1, dtype=torch.float32).view(c['N'], k) + 1e6 * s for s, k in enumerate(c['ks'])]
    img = PC.p16_image(ws, c['N'], c['lstm_H'])
    assert int((img != 0).sum()) == pos.numel()
    KB = sum(PC.kb16(k) for k in c['ks'])
    idx = torch.nonzero(img).reshape(-1)
    blk, lane, comp = idx // 256, (idx // 4) % 64, idx % 4
    tile, kb, i, kq = blk // KB, blk % KB, lane % 16, lane // 16
    row = (i % 4) * c['lstm_H'] + 4 * tile + i // 4 if c['lstm_H'] else 16 * tile + i
    starts = torch.tensor([sum(PC.kb16(k) for k in c['ks'][:s]) for s in range(len(c['ks']))])
    seg = (kb[:, None] >= starts[None, :]).sum(1) - 1
    k = (kb - starts[seg]) * 16 + kq * 4 + comp
    want = torch.stack([ws[int(s)][int(r), int(kk)] for s, r, kk in zip(seg, row, k)])
    assert torch.equal(img[idx], want)


@pytest.mark.parametrize('c', PC.TILE_CASES, ids=[c['id'] for c in PC.TILE_CASES])
def test_t16_index_is_a_bijection_onto_the_logical_slots(c):
    B, K, kb0 = c['B'], c['K'], c['kb0']
    stride = kb0 + PC.kb16(K) + c['kb_extra']
    pos = PC.t16_positions(range(B), K, stride, kb0).reshape(-1)
    assert pos.unique().numel() == B * K and int(pos.min()) >= 0 and int(pos.max()) < PC.t16_floats(B, stride)
    blk = pos // 256
    assert bool(((blk % stride >= kb0) & (blk % stride < kb0 + PC.kb16(K))).all())      # inside the view's k-block range
    x = torch.arange(1, B * K + 1, dtype=torch.float32).view(B, K)
    img = PC.t16_image(x, stride, kb0, fill=-1.0)
    assert torch.equal(img[pos], x.reshape(-1)) and int((img == -1).sum()) == img.numel() - B * K


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize('c', [c for c in PC.LINEAR if c['N'] <= 33 and c['id'].startswith('L1')][::3], ids=lambda c: c['id'])
def test_linear_reference_is_float64_torch(c):
    xs, w, bias, mask, mask2 = PC.linear_operands(c, seed=3)
    ref = PC.linear_ref(c, xs, w, bias, mask, mask2)
    e, N = c['epi'], c['N']
    F = torch.nn.functional
    act = {'none': lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
    v = act[e['act']](F.linear(torch.cat(xs, 1).double(), w.double(), bias.double() if e['bias'] else None))
    if e['mask']:
        v = v * mask.double()
    n_split = e['split'][0] if e['split'] else 0
    n_split2 = e['third'][0] if e['third'] else 0
    lim = n_split or n_split2 or N
    assert torch.allclose(ref['plain'][0], v[:, :lim], rtol=0, atol=1e-14) and ref['plain'][0].shape == (c['B'], lim)
    assert bool((ref['plain'][1] >= 0).all()) and float(ref['plain'][1].max()) < 1e-3      # a bound, and within two orders of the fixed 2e-5 (which stays as a cap)
    if n_split:
        hi = n_split2 or N
        assert torch.allclose(ref['y2'][0], v[:, n_split:hi].repeat_interleave(e['split'][1], 1), rtol=0, atol=1e-14)
    else:
        assert ref['y2'] is None
    if n_split2:
        v3 = act[e['third'][1]](v[:, n_split2:])
        v3 = v3 * mask2[:, :N - n_split2].double() if e['third'][2] else v3
        assert torch.allclose(ref['y3'][0], v3, rtol=0, atol=1e-14) and bool((ref['y3'][1] >= ref['plain'][1].min() * 0).all())
    else:
        assert ref['y3'] is None


@pytest.mark.parametrize('c', [c for c in PC.CELL if 'absent' in c['id'] or 'saturated' in c['id']], ids=lambda c: c['id'])
def test_cell_reference_is_float64_lstm_cell(c):
    o = PC.cell_operands(c, seed=5)
    H, ab = c['H'], c['absent']
    bi, bh = (None, None) if 'bias' in ab else (o['b_ih'], o['b_hh'])
    cp, mk = (None if 'c_prev' in ab else o['c_prev']), (None if 'mask' in ab else o['mask'])
    ref = PC.cell_ref(o['xs'], o['w'], bi, bh, cp, mk, o['std'], o['mean'])
    cell = torch.nn.LSTMCell(sum(c['Ks']), H, bias=True).double()
    with torch.no_grad():
        cell.weight_ih.copy_(o['w'].double())
        cell.weight_hh.zero_()
        cell.bias_ih.copy_(bi.double() if bi is not None else torch.zeros(4 * H))
        cell.bias_hh.copy_(bh.double() if bh is not None else torch.zeros(4 * H))
        c0 = cp.double() if cp is not None else torch.zeros(c['B'], H, dtype=torch.float64)
        h, c1 = cell(torch.cat(o['xs'], 1).double(), (torch.zeros(c['B'], H, dtype=torch.float64), c0))
    m = mk.double() if mk is not None else 1.0
    assert torch.allclose(ref['c'][0], c1, rtol=0, atol=1e-14) and torch.allclose(ref['h'][0], h * m, rtol=0, atol=1e-14)
    assert torch.allclose(ref['adain'][0], o['std'].double() * (h * m - o['mean'].double()), rtol=0, atol=1e-14)
    z = torch.cat(o['xs'], 1).double() @ o['w'].double().t() + (bi.double() + bh.double() if bi is not None else 0.0)
    assert torch.allclose(ref['gates'][0][:, 3], torch.sigmoid(z[:, 3 * H:]), rtol=0, atol=1e-14)
    assert torch.allclose(ref['gates'][0][:, 2], torch.tanh(z[:, 2 * H:3 * H]), rtol=0, atol=1e-14)
    # the derived bounds are of the order of the fixed 1e-5 of test_lstm_cell_packed, which the GPU test keeps as a cap on top of them
    # (PC.CELL_CAP), and never below the gate functions' own error
    for k in ('c', 'h', 'gates'):
        assert float(ref[k][1].max()) <= 5e-5 and (k != 'gates' or PC.E_FAST <= float(ref[k][1].min())), (k, float(ref[k][1].max()))
    if c['saturate']:       # a gate 40 away from 0 is 0 or 1 to the last bit and its bound is the function's own error
        sat = z.view(c['B'], 4, H).abs() > 30
        assert bool(sat.any()) and float(ref['gates'][1][sat].max()) <= PC.E_FAST * (1 + 1e-9)


def test_fast_gate_bound_is_within_what_the_issue_allows():
    assert 0 < PC.E_FAST_MEASURED and PC.E_FAST == 4 * PC.E_FAST_MEASURED and PC.E_FAST_MEASURED <= 1e-6
