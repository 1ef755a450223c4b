"""Case tables, layout index functions and float64 references of the forward products on pre-packed operands (skinny_packed.hip): the
weight-streaming linear and LSTM cell on P16 weights and T16 activations, the layout kernels that make those operands, and the linear
with attention-pre workgroups (and a hosted partial product) in the same launch -- shared by the host-side test
(test_packed_dispatch_host.py: every row reaches, through st_packed_fwd_variant, the launch it names; the rule restated here agrees with
the library; the index functions are bijections; the references agree with float64 torch) and the GPU test
(test_gpu_packed_products.py: every row against these references).

Pure torch on the CPU: nothing here needs a GPU or the HIP library.

  layout     p16_index / p16_image (the P16 layout stated independently of the kernels), PACK_CASES, PACK_BATCH, PACK_T_CASES,
             TILE_CASES, UNTILE_CASES, the *_CAP rows (one size per layout kernel just past its grid cap)
  dispatch   plan() -- pk_plan / pk_pair_shape / pk_attnpre_plan of skinny_packed.hip restated
  linear     LINEAR (rows L1..L9, K1..K4), EPILOGUES, linear_ref (value and first-order bound)
  cell       CELL (rows C1..C8 and the operand / destination subsets), CELL_PAIR (C9, C10), cell_ref
  attnpre    ATTNPRE"""
import itertools

import torch

from step_glue_cases import U, gen, kb16, t16_floats, t16_index, t16_positions   # noqa: F401  (the T16 helpers: reused, not copied)

# The fixed tolerances of test_skinny_linear_packed / test_lstm_cell_packed (test_gpu_parity.py; same operand distributions, K <= 1536)
# stay in force as caps: a row passes when its error is within the derived bound AND within these
LINEAR_CAP, CELL_CAP = 2e-5, 1e-5
KW = 8                         # waves per workgroup of every forward product: the reduction over them adds KW - 1 times
STEP = 16                      # k-blocks per load group of a workgroup (KW waves x TRIP = 2 k-blocks)
GRID_LIMIT = 512               # the linear takes the fewest batch tiles per workgroup that keep its grid within this
ACT = {'none': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3}      # ST_ACT_*
MODE_CELL, MODE_LINEAR, MODE_PAIR = 0, 1, 2                 # ST_PK_MODE_*
FAMILIES = ('pk_kernel', 'pk_lstm_rt2', 'pk_lstm_rt2_pair', 'pk_attnpre', 'pk_attnpre_part')      # ST_PK_* in order

# st_sigmoid_fast / st_tanh_fast (exp2 and rcp instructions): the largest absolute error against float64 measured on an MI355X by
# test_fast_gate_functions_error over pre-activations swept through [-30, 30] ("Packed forward products") was 1.02e-7 (sigmoid,
# at z = 3.58) and 1.27e-7 (tanh, at z = -1.53); the sweep is not exhaustive, so the bound every cell test uses is 4 x the larger of the two.
E_FAST_MEASURED = 1.27e-7
E_FAST = 4 * E_FAST_MEASURED


# ===================================================================================================== P16 layout
def p16_tiles(N, lstm_H=0):
    return lstm_H // 4 if lstm_H > 0 else (N + 15) // 16


def p16_slot(row, lstm_H=0):
    """(row tile, row within the tile) of weight row `row`.  Plain: rows 16 t .. 16 t + 15 are tile t.  LSTM (lstm_H = H, N = 4 H, torch
    gate order): tile t holds the (i, f, g, o) rows of hidden units 4 t .. 4 t + 3, slot i of it is row (i & 3) * H + 4 t + (i >> 2)"""
    if lstm_H > 0:
        gate, u = row // lstm_H, row % lstm_H
        return u >> 2, gate + 4 * (u & 3)
    return row >> 4, row & 15


def p16_index(row, k, kb0, KB, lstm_H=0):
    """float index of element (row, k) of the segment that starts at k-block kb0 of a P16 image with KB k-blocks per row tile
    (include/semitts.h): [row tile][k block of 16][lane 0..63][4 floats], element (i, k) of a block at lane 16 * ((k >> 2) & 3) + i,
    component k & 3.  row, k: broadcastable int64 tensors"""
    tile, i = p16_slot(row, lstm_H)
    return ((tile * KB + kb0 + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + i) * 4 + (k & 3)


def p16_floats(ks, N, lstm_H=0):
    return p16_tiles(N, lstm_H) * sum(kb16(k) for k in ks) * 256


def p16_positions(ks, N, lstm_H=0, device=None):
    """per segment the (N, k_s) float indices of its elements; every segment starts at its own k-block"""
    KB = sum(kb16(k) for k in ks)
    out, kb0 = [], 0
    row = torch.arange(N, dtype=torch.int64, device=device)[:, None]
    for k in ks:
        out.append(p16_index(row, torch.arange(k, dtype=torch.int64, device=device)[None, :], kb0, KB, lstm_H))
        kb0 += kb16(k)
    return out


def p16_image(ws, N, lstm_H=0):
    """the P16 image of the K-concatenation of ws (each (N, k_s)): what st_pack_weight must write, pads zero.  Runs on the device of ws
    (the index arithmetic is integer and the values are copied, so the image is exact wherever it is computed)"""
    ks = [int(w.shape[1]) for w in ws]
    img = torch.zeros(p16_floats(ks, N, lstm_H), dtype=torch.float32, device=ws[0].device)
    for w, pos in zip(ws, p16_positions(ks, N, lstm_H, ws[0].device)):
        img[pos.reshape(-1)] = w.reshape(-1).to(torch.float32)
    return img


def t16_image(x, kb_stride, kb0, fill=0.0):
    """the T16 buffer of kb_stride k-blocks per batch tile that holds x (B, K) from k-block kb0 on and `fill` everywhere else"""
    B, K = x.shape
    img = torch.full((t16_floats(B, kb_stride),), fill, dtype=torch.float32, device=x.device)
    b = torch.arange(B, dtype=torch.int64, device=x.device)[:, None]
    k = torch.arange(K, dtype=torch.int64, device=x.device)[None, :] + 16 * kb0
    img[t16_index(b, k, kb_stride).reshape(-1)] = x.reshape(-1)
    return img


# ===================================================================================================== dispatch rule
def rt2_shape(B, tiles):
    """shapes the 2-D tiled LSTM cell takes: an even number of row tiles, 2 or 4 batch tiles and the last of them not empty"""
    BT = (B + 15) // 16
    return tiles % 2 == 0 and BT in (2, 4) and B > 16 * (BT - 1)


def _plan_single(mode, B, tiles):
    BT = (B + 15) // 16
    if mode == MODE_CELL and rt2_shape(B, tiles):
        return ('pk_lstm_rt2', 1 if BT == 2 else 2, tiles // 2, 2, 0)
    if mode == MODE_LINEAR:
        nb = 1
        while nb < 4 and nb < BT and tiles * -(-BT // nb) > GRID_LIMIT:      # nb < BT: a batch tile that does not exist adds nothing
            nb += 1
    else:
        nb = min(BT, 4)
    return ('pk_kernel', nb, tiles, -(-BT // nb), 0)


def plan(mode, B, n, B1=0, n1=0, pre_parts=0, pre_A=0, pre_F=0, pre_aligned=1, part_n=0):
    """the launches [(family, nb, grid_x, grid_y, vec)] of a forward product (st_packed_fwd_variant), None for a refusal"""
    if B <= 0 or n <= 0:
        return None
    if mode == MODE_CELL:
        return None if n % 4 or pre_parts or part_n else [_plan_single(MODE_CELL, B, n // 4)]
    if mode == MODE_PAIR:
        if n % 4 or B1 <= 0 or n1 <= 0 or n1 % 4 or pre_parts or part_n:
            return None
        if rt2_shape(B, n // 4) and rt2_shape(B1, n1 // 4) and (B + 15) // 16 == 2 and (B1 + 15) // 16 == 2 and n % 8 == 0 and n1 % 8 == 0:
            return [('pk_lstm_rt2_pair', 1, n // 4 + n1 // 4, 1, 0)]
        return [_plan_single(MODE_CELL, B, n // 4), _plan_single(MODE_CELL, B1, n1 // 4)]
    if mode != MODE_LINEAR:
        return None
    tiles, BT = (n + 15) // 16, (B + 15) // 16
    if pre_parts <= 0:
        return None if part_n > 0 else [_plan_single(MODE_LINEAR, B, tiles)]
    if part_n > 0 and (tiles > 128 or not 16 < B <= 32 or part_n % 32):
        return None
    nb = 1 if (part_n > 0 or BT == 1 or tiles <= 128) else min(BT, 4)
    vec = 1 if (pre_A % 4 == 0 and pre_F % 4 == 0 and pre_aligned) else 0
    return [('pk_attnpre_part' if part_n > 0 else 'pk_attnpre', nb, tiles * -(-BT // nb) + B * pre_parts + max(part_n, 0) // 32, 1, vec)]


def k_groups(KB):
    return -(-KB // STEP)


def k_rot(tile, KB):
    """the group a workgroup's K walk starts from (pk_body)"""
    return ((tile & 255) * k_groups(KB)) >> 8


# ===================================================================================================== linear
def epi(act='none', bias=True, mask=False, out='both', y_way='vec', ydst_kb0=0, split=None, third=None):
    """one epilogue of st_skinny_linear_packed_fwd.  out: 'y' | 't16' | 'both'; y_way: 'vec' (ldy % 4 == 0, 16-byte aligned y) | 'ld'
    (ldy % 4 != 0) | 'ptr' (y one float past a 16-byte boundary) -- the last two take the scalar store branch; ydst_kb0: y_dst is a view
    that starts at this k-block of a wider buffer; split = (n_split, rep); third = (n_split2, act2, mask2)"""
    return dict(act=act, bias=bias, mask=mask, out=out, y_way=y_way, ydst_kb0=ydst_kb0, split=split, third=third)


def _epilogues(N):
    """the epilogues a linear of N outputs can carry (the split points need columns to split)"""
    out = [epi(), epi('relu', mask=True), epi('tanh', out='y', y_way='ld'), epi('sigmoid', out='t16', ydst_kb0=2),
           epi('relu', bias=False, out='y', y_way='ptr'), epi('none', mask=True, out='both', y_way='ld', ydst_kb0=1)]
    if N >= 17:
        a, b = (N - 9) & ~3, (N - 5) & ~3          # split points on the boundary of a 4-column group ...
        out += [epi('relu', split=(N - 1, 3)), epi('none', mask=True, split=(a, 2), third=(b, 'relu', True)),
                epi('tanh', split=(a - 2, 1), third=(b - 1, 'sigmoid', False), y_way='ptr'),      # ... and inside one
                epi('relu', third=(b + 1, 'tanh', True), ydst_kb0=1)]                              # a third range without a second
    return out


def _lin(id_, B, N, Ks, e, want):
    return dict(id=id_, B=B, N=N, Ks=tuple(Ks), epi=e, want=want)


def _linear_rows():
    rows = []
    # L1: one batch tile per workgroup at every (B, N) edge, the epilogues in turn (every epilogue of _epilogues(33) at least once)
    i, turn = 0, {}
    for B, N in itertools.product((1, 16, 17, 33, 70), (1, 16, 17, 33)):
        es = _epilogues(N)
        for j in range(2):
            e = es[turn.get(N, 0) % len(es)]          # ten rows per N: every epilogue of that N
            turn[N] = turn.get(N, 0) + 1
            Ks = ((24,), (16, 20), (5, 18, 9))[(i + j) % 3]
            rows.append(_lin('L1_B%d_N%d_%d' % (B, N, j), B, N, Ks, e, ('pk_kernel', 1, (N + 15) // 16, (B + 15) // 16)))
            i += 1
    # L2..L9: more than one batch tile per workgroup; each with K = 16 and with a K whose k-blocks are no multiple of 16
    for name, B, N, nb, gy in (('L2', 33, 2736, 2, 2), ('L3', 49, 2064, 2, 2), ('L4', 33, 4112, 3, 1), ('L5', 65, 2736, 3, 2),
                               ('L6', 49, 4112, 4, 1), ('L7', 65, 4112, 4, 2), ('L8', 20, 8208, 2, 1), ('L9', 33, 8208, 3, 1)):
        for Ks in ((16,), (24, 10)):
            e = epi('relu', mask=(Ks != (16,)), y_way='vec' if name != 'L5' else 'ld')
            rows.append(_lin('%s_B%d_N%d_K%d' % (name, B, N, sum(Ks)), B, N, Ks, e, ('pk_kernel', nb, (N + 15) // 16, gy)))
    # K1: the K loop with one batch tile per workgroup: 1..4 load groups, ragged last groups, both exits of the two-stage loop, the
    # epilogue operands requested before the loop (G < 3) and inside it
    for KB in (1, 15, 16, 17, 32, 33, 48, 49):
        rows.append(_lin('K1_KB%d' % KB, 5, 17, (16 * KB - 3,), epi('relu', mask=True), ('pk_kernel', 1, 2, 1)))
    # K2..K4: the rotated K walk (rot > 0 needs tile * G >= 256); K4 is this table's own: at the 171 row tiles of K3 the walk of three
    # groups starts from group 1 at the most (170 * 3 >> 8), one more row tile (N = 2752) starts from group 2
    rows.append(_lin('K2_B49_N2064_K272', 49, 2064, (272,), epi('relu'), ('pk_kernel', 2, 129, 2)))
    rows.append(_lin('K3_B33_N2736_K528', 33, 2736, (528,), epi('none', mask=True), ('pk_kernel', 2, 171, 2)))
    rows.append(_lin('K4_B33_N2752_K528', 33, 2752, (520,), epi('relu'), ('pk_kernel', 2, 172, 2)))
    return rows


LINEAR = _linear_rows()
X_KB0, X_KB_EXTRA = 1, 2       # the activation operand of every linear / cell row: a view one k-block into a buffer two k-blocks wider


def linear_operands(c, seed=0):
    """x_s (B, k_s) ~ N(0, 1), w (N, K) ~ N(0, 1 / K), bias, masks (dropout masks scaled by 2) of a LINEAR / ATTNPRE row"""
    g = gen(seed)
    B, N, K = c['B'], c['N'], sum(c['Ks'])
    xs = [torch.randn(B, k, generator=g) for k in c['Ks']]
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g)
    mask = (torch.rand(B, N, generator=g) > 0.5).float() * 2
    mask2 = (torch.rand(B, N, generator=g) > 0.5).float() * 2       # (its first N - n_split2 columns are used)
    return xs, w, bias, mask, mask2


def ulp(v):
    """the spacing of float32 at |v| (float64 tensor; the smallest normal's for smaller values)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 24)


def act_ref(z, tol, act):
    """act(z) in float64 and the bound that follows tol through it: every activation is 1-Lipschitz; tanhf and the sigmoid add 4 ulp of
    their output"""
    if act == 'relu':
        return torch.relu(z), tol
    if act == 'tanh':
        v = torch.tanh(z)
        return v, tol + 4 * ulp(v)
    if act == 'sigmoid':
        v = torch.sigmoid(z)
        return v, tol + 4 * ulp(v)
    return z, tol


def preact_ref(xs, w, biases, extra_adds=0):
    """z = sum_s x_s W_s^T + sum biases in float64 and its bound  2 (16 KB + KW + 3) U (sum |x| |w| + sum |bias|):  a k-block adds its 16
    products to the accumulator one after the other (16 KB roundings along the longest chain, the products themselves exact in the
    bound's sense: first order), the KW partial sums of the waves and the bias are KW more additions, 3 for what the epilogue does with
    the value; the factor 2 covers the MFMA's internal accumulation order, which the code does not state"""
    x, KB = torch.cat(xs, 1).double(), sum(kb16(t.shape[1]) for t in xs)
    wd = w.double()
    z, a = x @ wd.t(), x.abs() @ wd.abs().t()
    for b in biases:
        z, a = z + b.double(), a + b.double().abs()
    return z, 2 * (16 * KB + KW + 3 + extra_adds) * U * a


def linear_ref(c, xs, w, bias, mask, mask2):
    """float64 statement of one st_skinny_linear_packed_fwd: {'plain': (value (B, n_plain), tol), 'y2': (value (B, n2 * rep), tol) |
    None, 'y3': ... | None} -- the plain range goes to y and / or y_dst, columns [n_split, n_split2 or N) to y2 (each `rep` times),
    columns [n_split2, N) through act2 and mask2 to y3_dst"""
    e, N = c['epi'], c['N']
    z, tol = preact_ref(xs, w, [bias] if e['bias'] else [])
    v, tol = act_ref(z, tol, e['act'])
    if e['mask']:
        m = mask.double()
        v, tol = v * m, tol * m.abs() + U * (v * m).abs()
    n_split = e['split'][0] if e['split'] else 0
    n_split2 = e['third'][0] if e['third'] else 0
    lim = n_split if n_split > 0 else n_split2 if n_split2 > 0 else N
    out = {'plain': (v[:, :lim], tol[:, :lim]), 'y2': None, 'y3': None}
    if n_split > 0:
        hi, rep = (n_split2 if n_split2 > 0 else N), e['split'][1]
        out['y2'] = (v[:, n_split:hi].repeat_interleave(rep, 1), tol[:, n_split:hi].repeat_interleave(rep, 1))
    if n_split2 > 0:
        v3, t3 = act_ref(v[:, n_split2:], tol[:, n_split2:], e['third'][1])
        if e['third'][2]:
            m2 = mask2[:, :N - n_split2].double()
            v3, t3 = v3 * m2, t3 * m2.abs() + U * (v3 * m2).abs()
        out['y3'] = (v3, t3)
    return out


# ===================================================================================================== LSTM cell
CELL_ABSENT = [frozenset(s) for r in range(4) for s in itertools.combinations(('bias', 'c_prev', 'mask'), r)]      # 8 subsets
CELL_DESTS = [frozenset(s) for r in range(4) for s in itertools.combinations(('gates', 'h_dst1', 'adain'), r)]     # 8 subsets


def _cell(id_, B, H, Ks, absent, dests, want, wide_ld=False, saturate=False):
    return dict(id=id_, B=B, H=H, Ks=tuple(Ks), absent=frozenset(absent), dests=frozenset(dests), want=want, wide_ld=wide_ld, saturate=saturate)


def _cell_rows():
    shapes = [('C1', 5, 12, ('pk_kernel', 1, 3, 1)), ('C2', 20, 12, ('pk_kernel', 2, 3, 1)), ('C3', 33, 8, ('pk_kernel', 3, 2, 1)),
              ('C4', 49, 12, ('pk_kernel', 4, 3, 1)), ('C5', 70, 8, ('pk_kernel', 4, 2, 2)),
              ('C6', 17, 8, ('pk_lstm_rt2', 1, 1, 2)), ('C6', 32, 8, ('pk_lstm_rt2', 1, 1, 2)),
              ('C7', 49, 8, ('pk_lstm_rt2', 2, 1, 2)), ('C7', 64, 16, ('pk_lstm_rt2', 2, 2, 2)), ('C8', 48, 8, ('pk_kernel', 3, 2, 1))]
    rows = []
    for i, (name, B, H, want) in enumerate(shapes):
        # every shape: everything present, and one more subset of absent operands / destinations (in turn), K with a ragged k-block
        # count (KB = 3: the k-blocks 3..15 of the load group are the neighbour contract's)
        rows.append(_cell('%s_B%d_H%d_all' % (name, B, H), B, H, (24, 10), (), CELL_DESTS[-1], want, wide_ld=i % 2 == 0))
        rows.append(_cell('%s_B%d_H%d_sub%d' % (name, B, H, i % 8), B, H, (16, 16, 12) if i % 2 else (16,), CELL_ABSENT[1 + i % 7],
                          CELL_DESTS[(3 * i) % 8], want, wide_ld=i % 2 == 1))
    # every subset of absent operands and every subset of destinations on pk_kernel<0, 1> and on the 2-D tiled cell
    for name, B, H, want in (shapes[0], shapes[5]):
        for j, (ab, de) in enumerate(zip(CELL_ABSENT, CELL_DESTS)):
            rows.append(_cell('%s_B%d_H%d_absent%d' % (name, B, H, j), B, H, (20,), ab, de, want))
    # saturated gates: biases of +-40 put the gates at 0 and 1 to the last bit
    for name, B, H, want in (shapes[1], shapes[7]):
        rows.append(_cell('%s_B%d_H%d_saturated' % (name, B, H), B, H, (24,), (), CELL_DESTS[-1], want, saturate=True))
    return rows


CELL = _cell_rows()
# C9: both jobs 2-D tiled with one batch tile per workgroup and whole row-tile pairs -> one launch; C10: one job with H % 8 == 4 -> a launch each
CELL_PAIR = [
    dict(id='C9_pair', jobs=[_cell('j0', 17, 8, (24, 10), (), CELL_DESTS[-1], None), _cell('j1', 32, 16, (16,), ('c_prev',), ('gates',), None)],
         want=[('pk_lstm_rt2_pair', 1, 6, 1)]),
    dict(id='C9_pair_same', jobs=[_cell('j0', 20, 16, (20,), ('mask',), ('h_dst1',), None), _cell('j1', 20, 16, (40,), ('bias',), ('adain',), None)],
         want=[('pk_lstm_rt2_pair', 1, 8, 1)]),
    dict(id='C10_fallback', jobs=[_cell('j0', 20, 12, (24, 10), (), CELL_DESTS[-1], None), _cell('j1', 20, 8, (16,), (), ('gates',), None)],
         want=[('pk_kernel', 2, 3, 1), ('pk_lstm_rt2', 1, 1, 2)]),
]


def cell_operands(c, seed=0):
    """x_s, w (4H, K), b_ih, b_hh, c_prev, mask (dropout 0.1), AdaIN std / mean of a CELL row"""
    g = gen(seed)
    B, H, K = c['B'], c['H'], sum(c['Ks'])
    xs = [torch.randn(B, k, generator=g) for k in c['Ks']]
    w = torch.randn(4 * H, K, generator=g) * K ** -0.5
    b_ih, b_hh = torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1
    if c['saturate']:
        b_ih[::3] = 40.0
        b_ih[1::3] = -40.0
    c_prev = torch.randn(B, H, generator=g)
    mask = (torch.rand(B, H, generator=g) > 0.1).float() / 0.9
    std, mean = torch.relu(torch.randn(B, H, generator=g)), torch.randn(B, H, generator=g)
    return dict(xs=xs, w=w, b_ih=b_ih, b_hh=b_hh, c_prev=c_prev, mask=mask, std=std, mean=mean)


def _dsig(a):
    s = torch.sigmoid(a)
    return s * (1 - s)


def cell_ref(xs, w, b_ih, b_hh, c_prev, mask, std=None, mean=None, e_fast=E_FAST):
    """float64 nn.LSTMCell (gate order i, f, g, o) with the dropout mask on h and AdaIN std * (h - mean); absent operands None.
    -> dict of (value, bound) for c (B, H), h, gates (B, 4, H) and adain.  The pre-activation bound tz (preact_ref, with both biases)
    goes through each gate with the largest slope the gate has within tz of z (sigmoid' and tanh' fall with |z|, so that is the slope at
    max(|z| - tz, 0): 1 / 4 and 1 at the most) plus e_fast for st_sigmoid_fast / st_tanh_fast; then first order through
    c = f c_prev + i g (three roundings), h = o tanh(c) m (e_fast again, two roundings) and std (h - mean) (two roundings)"""
    z, tz = preact_ref(xs, w, [b for b in (b_ih, b_hh) if b is not None])
    B, H = z.shape[0], z.shape[1] // 4
    z, tz = z.view(B, 4, H), tz.view(B, 4, H)
    near = (z.abs() - tz).clamp_min(0)
    i, f, o = (torch.sigmoid(z[:, j]) for j in (0, 1, 3))
    g = torch.tanh(z[:, 2])
    di, df, do = (_dsig(near[:, j]) * tz[:, j] + e_fast for j in (0, 1, 3))
    dg = (1 - torch.tanh(near[:, 2]) ** 2) * tz[:, 2] + e_fast
    cp = c_prev.double() if c_prev is not None else torch.zeros(B, H, dtype=torch.float64)
    c = f * cp + i * g
    dc = cp.abs() * df + g.abs() * di + i.abs() * dg + 2 * U * ((f * cp).abs() + (i * g).abs()) + U * c.abs()
    m = mask.double() if mask is not None else torch.ones(B, H, dtype=torch.float64)
    tc = torch.tanh(c)
    h = o * tc * m
    dh = m.abs() * (tc.abs() * do + o.abs() * (dc + e_fast)) + 2 * U * h.abs()      # (tanh' <= 1)
    out = {'c': (c, dc), 'h': (h, dh), 'gates': (torch.stack([i, f, g, o], 1), torch.stack([di, df, dg, do], 1)), 'adain': None}
    if std is not None:
        s, mu = std.double(), mean.double()
        out['adain'] = (s * (h - mu), s.abs() * dh + 2 * U * s.abs() * (h.abs() + mu.abs()))
    return out


# ===================================================================================================== linear + attention pre
AT_L, AT_K = 5, 3              # the attention dims at their smallest; (A, F) = (16, 4): 16-byte loads, (20, 3): the element-wise kernel


def _at(id_, B, N, A, F, parts, want, part=False):
    vec = 1 if (A % 4 == 0 and F % 4 == 0) else 0
    return dict(id=id_, B=B, N=N, Ks=(24, 10), epi=epi('relu'), A=A, F=F, parts=parts, part=part, want=want + (vec,))


ATTNPRE = [
    _at('A1_B5_nb1', 5, 33, 16, 4, 1, ('pk_attnpre', 1, 3 + 5, 1)),
    _at('A1_B5_nb1_novec', 5, 17, 20, 3, 2, ('pk_attnpre', 1, 2 + 10, 1)),
    _at('A2_B16_129tiles', 16, 2064, 20, 3, 2, ('pk_attnpre', 1, 129 + 32, 1)),          # one batch tile stays at nb = 1
    _at('A2_B20_128tiles', 20, 2048, 16, 4, 1, ('pk_attnpre', 1, 256 + 20, 1)),          # ... and so do at most 128 row tiles
    _at('A3_B20_nb2', 20, 2064, 16, 4, 2, ('pk_attnpre', 2, 129 + 40, 1)),
    _at('A3_B20_nb2_novec', 20, 2064, 20, 3, 1, ('pk_attnpre', 2, 129 + 20, 1)),
    _at('A4_B33_nb3', 33, 2064, 20, 3, 1, ('pk_attnpre', 3, 129 + 33, 1)),
    _at('A4_B33_nb3_vec', 33, 2064, 16, 4, 2, ('pk_attnpre', 3, 129 + 66, 1)),
    _at('A5_B49_nb4', 49, 2064, 16, 4, 1, ('pk_attnpre', 4, 129 + 49, 1)),
    _at('A6_B70_nb4_two_rows', 70, 2064, 20, 3, 2, ('pk_attnpre', 4, 258 + 140, 1)),     # second grid row: batch tile 4, aliasing 1..3
    _at('A6_B70_nb4_vec', 70, 2064, 16, 4, 2, ('pk_attnpre', 4, 258 + 140, 1)),
    _at('A7_B20_part', 20, 33, 16, 4, 1, ('pk_attnpre_part', 1, 6 + 20 + 1, 1), part=True),
    _at('A7_B20_part_novec', 20, 33, 20, 3, 2, ('pk_attnpre_part', 1, 6 + 40 + 1, 1), part=True),
]
PART_H, PART_KS, PART_K0 = 8, (16, 16, 16), 1       # the hosted partial product: the slab (B, 4 H = 32) of a cell's k-blocks 1..2


def attnpre_operands(c, seed=0):
    g = gen(seed)
    B, A, F = c['B'], c['A'], c['F']
    pm = torch.randn(B, AT_L, A, generator=g)
    w_prev = torch.softmax(torch.randn(B, AT_L, generator=g), 1)
    w_cum = w_prev + torch.rand(B, AT_L, generator=g)
    return dict(pm=pm, w_prev=w_prev, w_cum=w_cum, loc_conv_w=torch.randn(F, 2, AT_K, generator=g) * 0.3,
                loc_lin_w=torch.randn(A, F, generator=g) * 0.3)


# ===================================================================================================== layout rows
def _pk(id_, N, ks, lstm_H=0, ld_extra=0, off=0):
    """st_pack_weight: segments (N, k_s) with row stride k_s + ld_extra, the first `off` floats past a 16-byte boundary"""
    return dict(id=id_, N=N, ks=tuple(ks), lstm_H=lstm_H, ld_extra=ld_extra, off=off)


PACK_CASES = [
    _pk('one_seg', 32, (32,)), _pk('ragged_k_N33', 33, (20,)), _pk('two_seg', 40, (16, 30), ld_extra=4), _pk('three_seg_N17', 17, (5, 18, 9), ld_extra=3),
    _pk('lstm_H12', 48, (24, 10), lstm_H=12, ld_extra=8), _pk('lstm_H8_three_seg', 32, (16, 33, 7), lstm_H=8),
    _pk('off1', 20, (32,), ld_extra=4, off=1),             # an aligned shape from an unaligned source: the scalar loads with rem >= 4
    _pk('rem_lt4', 16, (18, 3), ld_extra=1),               # 16-byte pieces with 1..3 columns left
]
PACK_CAP = _pk('past_8192_workgroups', 16 * 129 + 5, (16 * 253 - 3,))      # 130 tiles x 253 k-blocks x 64 lanes > 8192 x 256 threads
PACK_BATCH = [_pk('b0', 16 * 64 + 3, (16 * 253 - 3,)),                     # 65 x 253 x 64 > 4096 x 256: the batch launch's cap
              _pk('b1', 33, (20,)), _pk('b2', 48, (24, 10), lstm_H=12), _pk('b3', 17, (5, 18, 9), ld_extra=3), _pk('b4', 1, (1,)),
              _pk('b5', 40, (16, 30), ld_extra=4), _pk('b6', 20, (32,), ld_extra=4, off=1), _pk('b7', 256, (100,))]

# st_pack_weight_t: (K, cols per segment, per segment whether it is a view with a row stride > cols); 16-byte loads need every segment
# aligned, every stride a multiple of 4 and every segment boundary on a multiple of 4
PACK_T_CASES = [
    dict(id='vec_one', K=32, cols=(32,), strided=(False,)), dict(id='vec_three_ragged_K', K=37, cols=(8, 20, 12), strided=(True, False, True)),
    dict(id='vec_N_ragged', K=48, cols=(16, 22), strided=(False, True)),         # the last 4-row group runs past N: element-wise
    dict(id='scalar_cut_groups', K=37, cols=(5, 18, 9), strided=(False, True, False)),      # boundaries cut 4-row groups
    dict(id='scalar_ld', K=20, cols=(30, 34), strided=(False, False)),
]
PACK_T_CAP = dict(id='past_8192_workgroups', K=16 * 362 - 5, cols=(16 * 362 + 4,), strided=(False,))      # 363 x 362 x 16 > 8192 x 256

# st_tile_rows / st_untile_rows: (B, K, view's first k-block, k-blocks after the view, ld - K)
TILE_CASES = [dict(id='B%d_K%d_kb%d' % (B, K, kb0), B=B, K=K, kb0=kb0, kb_extra=ex, ld_extra=ld)
              for B, K, kb0, ex, ld in ((1, 4, 0, 0, 0), (5, 24, 2, 1, 3), (16, 16, 1, 0, 4), (17, 33, 3, 2, 1), (33, 50, 0, 1, 2), (70, 100, 1, 1, 0))]
TILE_CAP = dict(id='past_4096_workgroups', B=16 * 64 + 1, K=16 * 253 - 3, kb0=0, kb_extra=0, ld_extra=0)      # 65 x 253 x 64 > 4096 x 256
# ld % 4 == 0 takes untile_rows_vec_kernel (whole 16-byte pieces and the 1..3 last columns of a row), anything else the element-wise one
UNTILE_CASES = [dict(id='B%d_K%d_ld%d' % (B, K, K + ld), B=B, K=K, kb0=kb0, kb_extra=ex, ld_extra=ld)
                for B, K, kb0, ex, ld in ((1, 4, 0, 0, 0), (5, 24, 2, 1, 4), (17, 33, 3, 2, 3), (17, 33, 1, 0, 2), (33, 50, 0, 1, 2), (33, 50, 1, 1, 1),
                                          (70, 99, 1, 1, 1), (70, 101, 0, 0, 3), (16, 18, 0, 1, 2))]
UNTILE_VEC_CAP = dict(id='vec_past_16384_workgroups', B=16 * 128 + 1, K=16 * 509 - 3, kb0=0, kb_extra=0, ld_extra=3)     # ld % 4 == 0
UNTILE_CAP = dict(id='past_4096_workgroups', B=1025, K=1027, kb0=0, kb_extra=0, ld_extra=0)      # 1025 x 1027 > 4096 x 256, ld odd


def untile_is_vec(c):
    return (c['K'] + c['ld_extra']) % 4 == 0
