"""Case table of the nn.LSTM sequence layers' planner (st_lstm_seq_variant, include/semitts.h), for the host-side test
test_lstm_seq_dispatch_host.py: every row reaches the form named in it, and together the rows reach every form of both passes.

Row: the query -- pass, ndir, (B, T, H), ld and the two columns of the output (forward) or output gradient (backward), allow_persist, the
device's compute units, the units to leave free, cleared ST_LSTM_AL_* bits -- and what the plan must say: the form, the weight layout
and, for a one-launch row, rt / nkb / rg / xcd_map and (grid, block).  `reverse` travels in the job only (ndir == 1); the planner does
not see it, so a row with ndir == 1 stands for both walks.  The constants below restate the planner's; they are not imported from it.

Below the rows: the float64 reference of the layer (lstm_ref, lstm_ref_bwd), and GPU_CASES -- the small shape and layout at which
test_gpu_lstm_seq_forms.py runs each row's form against that reference -- with NOT_RUN, the rows that stay planner-only.  Nothing here
touches a device."""
import functools

import torch


STEP, PACKED, PERSIST = 0, 1, 2                  # ST_LSTM_STEP / _PACKED / _PERSIST
W_NATURAL, W_T, W_PACKED_T = 0, 1, 2             # ST_LSTM_W_*
AL_FWD = 1 | 2 | 4                               # out, w_hh[0], w_hh[1]
AL_BWD = 1 | 2 | 4 | 8 | 16 | 32 | 64            # dout, gates_tape[0..1], c_tape[0..1], dxproj[0..1]
CUS = 256                                        # MI355X
CU_RESERVE = 32                                  # ops.PERSIST_CU_RESERVE's default


def t16_floats(B, K):
    """st_t16_floats: ceil(B/16) batch tiles of ceil(K/16) k-blocks of 16 x 16 floats"""
    return ((B + 15) // 16) * ((K + 15) // 16) * 256


def ws_floats(backward, ndir, B, H, form):
    if form == PERSIST:
        return 0
    if form == PACKED:
        return 2 * B * H + 4 * t16_floats(B, 4 * H)
    return (2 * ndir if backward else 2 * ndir + 1) * B * H


def fwd_geometry(B, H):
    """the one-launch forward: (tile, d) owns four hidden units, four waves of H/64 k-blocks each"""
    return dict(rt=(B + 15) // 16, nkb=H // 64, rg=0, xcd_map=int((H // 4) % 4 == 0), grid=(H // 4, 2, 1), block=256)


def bwd_geometry(B, H, rg):
    """the one-launch backward: (tile, bg, d) owns 16 hidden units and rg batch rows, eight waves of H/32 k-blocks each"""
    return dict(rt=(B + 15) // 16, nkb=H // 32, rg=rg, xcd_map=0, grid=(H // 16, (B + rg - 1) // rg, 2), block=512)


def R(id, backward, form, weights, B=32, T=43, H=256, ndir=2, reverse=0, ld=None, col=None, allow_persist=1, cus=CUS, cu_reserve=0,
      unaligned=0, rg=None):
    ld = ndir * H if ld is None else ld
    col = (0, H if ndir == 2 else 0) if col is None else col
    geo = None
    if form == PERSIST:
        geo = bwd_geometry(B, H, rg) if backward else fwd_geometry(B, H)
    return dict(id=id, backward=backward, ndir=ndir, reverse=reverse, B=B, T=T, H=H, ld=ld, col=col, allow_persist=allow_persist, cus=cus,
                cu_reserve=cu_reserve, aligned=(AL_BWD if backward else AL_FWD) & ~unaligned, form=form, weights=weights, geo=geo)


def F(id, form, **kw):
    return R('fwd_' + id, 0, form, W_NATURAL, **kw)


def B_(id, form, **kw):
    return R('bwd_' + id, 1, form, {PERSIST: W_NATURAL, PACKED: W_PACKED_T, STEP: W_T}[form], **kw)


ROWS = [
    # ---- forward: 2 * H/4 workgroups, H/64 in {1, 2, 4, 8}, at most four row tiles
    F('h64', PERSIST, H=64, B=5, T=7),
    F('h128', PERSIST, H=128, B=64, T=20),
    F('c2', PERSIST),                                         # the text encoder: B 32, T 43, H 256
    F('h512', PERSIST, H=512, B=17, T=5),                     # 256 workgroups on 256 compute units
    F('h512_255_cus', STEP, H=512, B=17, T=5, cus=255),
    F('h512_reserve', STEP, H=512, B=17, T=5, cu_reserve=1),
    F('h96', STEP, H=96),                                     # H % 64
    F('h192', STEP, H=192),                                   # three k-blocks per wave: no such kernel
    F('h576', STEP, H=576),
    F('h1024', STEP, H=1024),
    F('h24', STEP, H=24, B=3, T=5),
    F('b64', PERSIST, B=64),
    F('b65', STEP, B=65),                                     # a fifth row tile
    F('ldo_odd', STEP, ld=514),                               # rows of out not 16-byte addressable
    F('ocol_odd', STEP, ld=516, col=(0, 258)),
    F('overlap', STEP, col=(0, 128)),                         # the sentinel of one direction would be the other's data
    F('swapped_cols', PERSIST, col=(256, 0)),
    F('out_unaligned', STEP, unaligned=1),
    F('w1_unaligned', STEP, unaligned=4),
    F('no_persist', STEP, allow_persist=0),
    F('one_dir', STEP, ndir=1, H=256),
    F('one_dir_reverse', STEP, ndir=1, reverse=1, H=64, ld=128, col=(64, 0)),
    # ---- backward: 2 * H/16 * ceil(B/16) workgroups, H/32 in {1, 2, 4, 8}
    B_('h32', PERSIST, H=32, B=20, T=6, rg=8),
    B_('h64', PERSIST, H=64, B=5, T=7, rg=8),
    B_('h128', PERSIST, H=128, B=33, T=9, rg=8),
    B_('c2', PERSIST, rg=8),                                  # 2 * 16 * 4 = 128 workgroups of eight rows: half the device exactly
    B_('b33', PERSIST, B=33, rg=16),                          # 160 workgroups of eight rows would be more than half: sixteen rows
    B_('b33_512_cus', PERSIST, B=33, cus=512, rg=8),
    B_('b128', PERSIST, B=128, rg=16),                        # 2 * 16 * 8 = 256 workgroups
    B_('b128_reserve', PACKED, B=128, cu_reserve=CU_RESERVE),       # ... which do not fit beside the units left to the all-reduce
    B_('b112_reserve', PERSIST, B=112, cu_reserve=CU_RESERVE, rg=16),      # 224 workgroups do
    B_('b129', PACKED, B=129),
    B_('b2048', PACKED, B=2048, T=2),
    B_('h512', PACKED, H=512),                                # the 4H x 16 slice no longer fits the registers
    B_('h96', PACKED, H=96),                                  # three k-blocks per wave: no such kernel
    B_('h48', PACKED, H=48),
    B_('h24', STEP, H=24, B=3, T=5),                          # H % 16: no packed operands either
    B_('ldd_odd', STEP, ld=514),                              # rows of dout not 16-byte addressable: the packed launch loads 16 bytes too
    B_('dcol_odd', STEP, ld=516, col=(0, 258)),
    B_('dout_unaligned', STEP, unaligned=1),
    B_('c1_unaligned', STEP, unaligned=16),
    B_('dx0_unaligned', STEP, unaligned=32),
    B_('no_persist', PACKED, allow_persist=0),
    B_('no_persist_h24', STEP, allow_persist=0, H=24),
    B_('one_dir', STEP, ndir=1),                              # one direction: always per step, on W_hh^T
    B_('one_dir_reverse', STEP, ndir=1, reverse=1, H=32, B=17, T=4),
    B_('one_dir_h24', STEP, ndir=1, H=24, B=3, T=5),
]

# queries no form takes: st_lstm_seq_variant returns -1 and the run entry points refuse the job
REFUSED = [
    dict(id='ndir3', ndir=3),
    dict(id='ndir0', ndir=0),
    dict(id='B0', B=0),
    dict(id='T0', T=0),
    dict(id='H0', H=0),
    dict(id='ld_short', ld=511),
    dict(id='col_negative', col=(-4, 256)),
]


# ------------------------------------------------------------------------------------------------ the float64 reference of the layer
def lstm_ref(xproj, w_hh, b_hh, reverse, dtype=torch.float64):
    """One direction of the layer as include/semitts.h states it, a plain loop in `dtype`: zero initial state, gates in torch order
    i, f, g, o, b_hh added in the cell; the walk runs t = T-1 .. 0 with `reverse`.  xproj (B,T,4H), w_hh (4H,H), b_hh (4H).
    Returns out (B,T,H), the activated gates (T,B,4,H) and c (T,B,H), all indexed by time step."""
    x, w, b = xproj.to(dtype), w_hh.to(dtype), b_hh.to(dtype)
    B, T, H4 = x.shape
    H = H4 // 4
    h = c = torch.zeros(B, H, dtype=dtype)
    out, gates, cs = [None] * T, [None] * T, [None] * T
    for s in range(T):
        t = T - 1 - s if reverse else s
        a = (x[:, t] + h @ w.t() + b).view(B, 4, H)
        i, f, g, o = torch.sigmoid(a[:, 0]), torch.sigmoid(a[:, 1]), torch.tanh(a[:, 2]), torch.sigmoid(a[:, 3])
        c = f * c + i * g
        h = o * torch.tanh(c)
        out[t], gates[t], cs[t] = h, torch.stack((i, f, g, o), 1), c
    return torch.stack(out, 1), torch.stack(gates, 0), torch.stack(cs, 0)


def lstm_ref_bwd(xproj, w_hh, b_hh, reverse, dout, dtype=torch.float64):
    """dL/dxproj (B,T,4H) for the output gradient dout (B,T,H): autograd in `dtype` through lstm_ref"""
    x = xproj.detach().to(dtype).requires_grad_()
    out = lstm_ref(x, w_hh, b_hh, reverse, dtype)[0]
    return torch.autograd.grad(out, x, dout.to(dtype))[0]


@functools.lru_cache(maxsize=None)
def layer_inputs(B, T, H):
    """the inputs the bounds of the GPU tests were established on (_layer of test_gpu_lstm_persist.py): randn projections, w / sqrt(H),
    0.1 * randn bias, for two directions; and one randn output gradient (B,T,H) per direction.  Shared and never written."""
    g = torch.Generator().manual_seed(4000 + 64 * B + 8 * T + H)
    xp = [torch.randn(B, T, 4 * H, generator=g) for _ in range(2)]
    w = [torch.randn(4 * H, H, generator=g) / H ** 0.5 for _ in range(2)]
    b = [torch.randn(4 * H, generator=g) * 0.1 for _ in range(2)]
    dout = [torch.randn(B, T, H, generator=g) for _ in range(2)]
    return xp, w, b, dout


@functools.lru_cache(maxsize=None)
def reference(B, T, H, d, reverse):
    """float64 out / gates / c / dxproj of set d of layer_inputs(B, T, H) walked forward or in reverse, and how far the same loop in
    float32 on the CPU is from them: e32_out (absolute), e32_c (relative to max(1, max|c|)), e32_dx (relative to max|dxproj|)"""
    xp, w, b, dout = layer_inputs(B, T, H)
    out, gates, c = lstm_ref(xp[d], w[d], b[d], reverse)
    dx = lstm_ref_bwd(xp[d], w[d], b[d], reverse, dout[d])
    out32, _, c32 = lstm_ref(xp[d], w[d], b[d], reverse, torch.float32)
    dx32 = lstm_ref_bwd(xp[d], w[d], b[d], reverse, dout[d], torch.float32)
    return dict(out=out, gates=gates, c=c, dx=dx,
                e32_out=float((out32.double() - out).abs().max()),
                e32_c=float((c32.double() - c).abs().max()) / max(1.0, float(c.abs().max())),
                e32_dx=float((dx32.double() - dx).abs().max()) / float(dx.abs().max()))


def case_references(case):
    """reference() of each direction of a GPU case: set d walks in reverse if it is the second of two, or the one of a reversed layer"""
    return [reference(case['B'], case['T'], case['H'], d, bool(d == 1 or case['reverse'])) for d in range(case['ndir'])]


# ------------------------------------------------------------------------------------------------ what runs on the GPU
# Layout recipes of the (B, T, ld) output (forward) or output gradient (backward) for the case's own H: leading dimension, columns of the
# directions, floats between the 16-byte aligned buffer and the tensor, cleared ST_LSTM_AL_* bits, allow_persist.  `embedded` leaves the
# guard columns [0,4), [H+4,H+8) and [2H+8,2H+12); `w1_unaligned` / `c1_unaligned` shift w_hh[1] / c_tape[1] by one float instead.
def layout(recipe, H, backward):
    ld, cols, off, unaligned, allow = 2 * H, (0, H), 0, 0, 1
    if recipe == 'swapped':
        cols = (H, 0)
    elif recipe == 'embedded':
        ld, cols = 2 * H + 12, (4, H + 8)
    elif recipe == 'ld_odd':
        ld = 2 * H + 2
    elif recipe == 'col_odd':
        ld, cols = 2 * H + 4, (0, H + 2)
    elif recipe == 'x_unaligned':
        off, unaligned = 1, 1
    elif recipe == 'w1_unaligned':
        assert not backward
        unaligned = 4
    elif recipe == 'c1_unaligned':
        assert backward
        unaligned = 16
    elif recipe == 'no_persist':
        allow = 0
    elif recipe == 'one_dir':                 # ndir = 1: the whole (B, T, H) tensor
        ld, cols = H, (0,)
    elif recipe == 'one_dir_col':             # ndir = 1: the right half of a (B, T, 2H) tensor
        cols = (H,)
    else:
        assert recipe == 'plain', recipe
    return dict(ld=ld, cols=cols, off=off, unaligned=unaligned, allow_persist=allow)


FORM_NAMES = {STEP: 'step', PACKED: 'packed', PERSIST: 'one'}


def G(backward, row, form, shape, recipe='plain', reverse=None, rt=0, rg=0):
    """one GPU case: the ROWS id it realises, the small (B, T, H) it runs at, its layout recipe and what the plan must name (rt: row tiles of
    a one-launch forward, rg: batch rows per workgroup of a one-launch backward).  reverse = 0 / 1: one direction, that walk."""
    B, T, H = shape
    ndir = 2 if reverse is None else 1
    pre = 'bwd_' if backward else 'fwd_'
    if ndir == 1 and recipe == 'plain':
        recipe = 'one_dir'
    if form == PERSIST and backward:
        rt = (B + 15) // 16
    weights = {PERSIST: W_NATURAL, PACKED: W_PACKED_T, STEP: W_T}[form] if backward else W_NATURAL
    id = '%s%s_%s_%dx%dx%d' % (pre, FORM_NAMES[form], recipe, B, T, H) + ('' if ndir == 2 else '_rev' if reverse else '_fwd')
    return dict(id=id, row=pre + row, backward=backward, ndir=ndir, reverse=reverse or 0, B=B, T=T, H=H, recipe=recipe, form=form,
                weights=weights, rt=rt, rg=rg)


GPU_CASES = [
    # ---- forward, one launch: lstm_seq2_persist_kernel<RT, NKB>
    G(0, 'h64', PERSIST, (1, 1, 64), rt=1),                     # every lane of the row tile clamps to row 0; no wait at all
    G(0, 'h64', PERSIST, (16, 2, 64), rt=1),                    # one wait
    G(0, 'h64', PERSIST, (17, 3, 64), rt=2),
    G(0, 'h128', PERSIST, (48, 3, 128), rt=3),
    G(0, 'h128', PERSIST, (49, 3, 128), rt=4),
    G(0, 'c2', PERSIST, (32, 2, 256), rt=2),
    G(0, 'b64', PERSIST, (64, 4, 256), rt=4),
    G(0, 'h512', PERSIST, (17, 2, 512), rt=2),
    G(0, 'swapped_cols', PERSIST, (5, 4, 64), 'swapped', rt=1),
    G(0, 'swapped_cols', PERSIST, (5, 4, 64), 'embedded', rt=1),
    G(0, 'h128', PERSIST, (33, 3, 128), 'embedded', rt=3),
    # ---- forward, one launch per step
    G(0, 'h96', STEP, (5, 4, 96)),
    G(0, 'h192', STEP, (3, 3, 192)),
    G(0, 'h576', STEP, (2, 2, 576)),
    G(0, 'h24', STEP, (3, 5, 24)),
    G(0, 'b65', STEP, (65, 3, 64)),
    G(0, 'ldo_odd', STEP, (5, 4, 64), 'ld_odd'),
    G(0, 'ocol_odd', STEP, (5, 4, 64), 'col_odd'),
    G(0, 'out_unaligned', STEP, (5, 4, 64), 'x_unaligned'),
    G(0, 'w1_unaligned', STEP, (5, 4, 64), 'w1_unaligned'),
    G(0, 'no_persist', STEP, (5, 4, 64), 'no_persist'),
    G(0, 'one_dir', STEP, (3, 3, 256), reverse=0),
    G(0, 'one_dir_reverse', STEP, (3, 3, 256), reverse=1),
    G(0, 'one_dir', STEP, (5, 4, 64), 'one_dir_col', reverse=0),
    G(0, 'one_dir_reverse', STEP, (5, 4, 64), 'one_dir_col', reverse=1),
    # ---- backward, one launch: lstm_seq2_bwd_persist_kernel<NKB, RG>
    G(1, 'h32', PERSIST, (1, 1, 32), rg=8),
    G(1, 'h32', PERSIST, (8, 2, 32), rg=8),
    G(1, 'h64', PERSIST, (9, 3, 64), rg=8),                     # a last group of one row
    G(1, 'h128', PERSIST, (16, 3, 128), rg=8),
    G(1, 'h128', PERSIST, (17, 3, 128), rg=8),
    G(1, 'c2', PERSIST, (9, 2, 256), rg=8),                     # eight k-blocks per wave, eight rows per workgroup
    G(1, 'b33', PERSIST, (33, 4, 256), rg=16),                  # a last group of one row
    G(1, 'b33', PERSIST, (40, 3, 256), rg=16),                  # a last group of eight rows
    G(1, 'b33', PERSIST, (72, 3, 128), rg=16),                  # four k-blocks per wave
    G(1, 'h64', PERSIST, (5, 4, 64), 'swapped', rg=8),
    G(1, 'h64', PERSIST, (5, 4, 64), 'embedded', rg=8),
    # ---- backward, packed operands
    G(1, 'b129', PACKED, (129, 2, 256)),
    G(1, 'h512', PACKED, (5, 3, 512)),
    G(1, 'h96', PACKED, (17, 3, 96)),
    G(1, 'h48', PACKED, (16, 2, 48)),
    G(1, 'h48', PACKED, (1, 1, 16)),
    G(1, 'no_persist', PACKED, (20, 6, 32), 'no_persist'),
    # ---- backward, a pointwise and a W_hh^T launch per step (the packed launch takes 16-byte addressable operands only)
    G(1, 'ldd_odd', STEP, (5, 4, 64), 'ld_odd'),
    G(1, 'dcol_odd', STEP, (5, 4, 64), 'col_odd'),
    G(1, 'dout_unaligned', STEP, (5, 4, 64), 'x_unaligned'),
    G(1, 'c1_unaligned', STEP, (5, 4, 64), 'c1_unaligned'),
    G(1, 'h24', STEP, (3, 5, 24), 'ld_odd'),
    G(1, 'no_persist_h24', STEP, (3, 5, 24), 'no_persist'),
    G(1, 'one_dir', STEP, (3, 3, 256), reverse=0),
    G(1, 'one_dir_reverse', STEP, (3, 3, 256), reverse=1),
    G(1, 'one_dir_h24', STEP, (3, 5, 24), reverse=0),
    G(1, 'one_dir_h24', STEP, (3, 5, 24), reverse=1),
]

# the ROWS that stay planner-only, and why
NOT_RUN = {
    'fwd_h512_255_cus': 'cus != 256: ops.lstm_layer takes no compute-unit count',
    'fwd_h512_reserve': 'cu_reserve != 0: ops.lstm_layer takes no reserve',
    'bwd_b33_512_cus': 'cus != 256: ops.lstm_layer_bwd takes no compute-unit count',
    'bwd_b128_reserve': 'cu_reserve != 0: ops.lstm_layer_bwd takes no reserve',
    'bwd_b112_reserve': 'cu_reserve != 0: ops.lstm_layer_bwd takes no reserve',
    'fwd_overlap': 'overlapping output columns have no defined result',
    'fwd_h1024': 'size only: the code of fwd_h576',
    'bwd_b2048': 'size only: the code of bwd_b129',
    'bwd_b128': '256 workgroups of 512 threads need every compute unit of a shared device: a starved launch is not the kernel failing',
    'bwd_dx0_unaligned': 'ops.lstm_layer_bwd allocates dxproj itself; nothing in the product reaches the row',
}
