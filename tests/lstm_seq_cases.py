"""Case table of the nn.LSTM sequence layers' planner (st_lstm_seq_variant, include/semitts.h), for the host-side test
test_lstm_seq_dispatch_host.py: every row reaches the form named in it, and together the rows reach every form of both passes.

Row: the query -- pass, ndir, (B, T, H), ld and the two columns of the output (forward) or output gradient (backward), allow_persist, the
device's compute units, the units to leave free, cleared ST_LSTM_AL_* bits -- and what the plan must say: the form, the weight layout
and, for a one-launch row, rt / nkb / rg / xcd_map and (grid, block).  `reverse` travels in the job only (ndir == 1); the planner does
not see it, so a row with ndir == 1 stands for both walks.  The constants below restate the planner's; they are not imported from it."""

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
    B_('ldd_odd', PACKED, ld=514),                            # rows of dout not 16-byte addressable
    B_('dcol_odd', PACKED, ld=516, col=(0, 258)),
    B_('dout_unaligned', PACKED, unaligned=1),
    B_('c1_unaligned', PACKED, unaligned=16),
    B_('dx0_unaligned', PACKED, unaligned=32),
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
