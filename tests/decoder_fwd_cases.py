"""The decode loop's forward forms at small decoder sizes: one table for two tests (no GPU imports here).

tests/test_decoder_fwd_forms_host.py proves on the host that every case reaches the forms it names -- it fills st_decoder_io the way
Decoder._run_loop does (`io_plan` below restates that) and asks the planner, st_decoder_fwd_forms, for an MI355X (256 compute
units, range capacity 512).  tests/test_gpu_decoder_fwd_forms.py runs every case through `Decoder` on the GPU, checks that the loop
really took those forms, and compares mel / alignment / stop with the float64 oracle.

A case = decoder dims, B, L, steps, a mode, the `Decoder` knobs it sets, and the expected planner word as
(attention form, host of the decoder cell's partial gate product, flags), fin parts and k0 (k-blocks the cell keeps; 0 without a
partial product).  Modes:
  free           eval, free running (every step feeds its own output back; prenet layer 1 fused into the proj launch)
  tf_eval        eval, teacher forcing for every row (no tapes, no deferral: the inference forms with the flag tf)
  tf_partial     eval, the first Bt rows have a teacher (shorter than the run), the others feed their own output back
  train_tf       training, teacher forcing through the differentiable path (tapes kept, projection deferred, cells paired)
  train_partial  training with a partial teacher batch: not pure teacher forcing, so the whole attention step and nothing deferred
"""

COMMON = dict(n_mels=8, r=2, F=8, K=7, S=12)
DIMS = {
    'M16': dict(P=32, Q=48, D=64, E=32, A=32),      # the smallest set that admits every fused form; the cell's K is 2 + 3 + 4 = 9 k-blocks
    'MID': dict(P=48, Q=80, D=96, E=64, A=48),      # 4 + 5 + 6 = 15 k-blocks, A / 16 = 3
    'RAG': dict(P=24, Q=40, D=36, E=28, A=24),      # nothing is a multiple of 16; E % 8 != 0
    'A20': dict(P=32, Q=48, D=64, E=32, A=20),      # A % 4 == 0, A % 16 != 0: long texts get fin_split and never pq_rng
}
MODES = ('free', 'tf_eval', 'tf_partial', 'train_tf', 'train_partial')
# the knobs a case may set, with the values every other case runs under (set explicitly: the environment cannot move them)
KNOBS = dict(attn_split=True, attn_pq_in_fin=True, attn_fin_parts=2, attn_pre_parts=4, split_gates=True, split_cell_k=0,
             split_gates_train=True, fwd_pair_cells=True, attn_rng_one_launch=True)
SPLIT_MIN_LEN, SPLIT_POSITIONS = 128, 43           # Decoder.attn_split_min_len / attn_split_positions
CUS, RNG_CAPACITY = 256, 512                       # MI355X: 256 compute units, two range workgroups per compute unit

TRAIN = frozenset({'tf', 'defer', 'pre_in_pq', 'pair'})
NONE = frozenset()


def case(id, dims, B, L, want, mode='free', steps=6, fp=2, k0=0, Bt=None, gain=1.0, **knobs):
    assert dims in DIMS and mode in MODES and not set(knobs) - set(KNOBS), (id, knobs)
    assert (Bt is not None) == (mode in ('tf_partial', 'train_partial')), id
    assert 1 <= steps <= (6 if L >= 130 else 8), id
    return dict(id=id, dims=dims, B=B, L=L, steps=steps, mode=mode, Bt=Bt, gain=gain, knobs=knobs,
                want=(want[0], want[1], frozenset(want[2])), fp=fp, k0=k0)


def cell_k0(dims):
    """k-blocks the decoder cell keeps by the library's own rule (st_decoder_gate_split_k) at these sizes: fewer than 32 k-blocks
    leave no whole round of 16 to host, so everything behind the context columns rides and the cell keeps ceil(E / 16)"""
    return (DIMS[dims]['E'] + 15) // 16


def _cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))
    # ---- free running, short text: pq + fin as one launch
    for ds in ('M16', 'MID'):
        for B in (1, 3, 16, 33):
            add('%s_free_b%d' % (ds, B), ds, B, 11, ('pq_fin', 'none', NONE), steps={1: 4, 3: 5, 16: 6, 33: 7}[B])
        for B in (17, 20, 32):       # 16 < B <= 32: the cell's partial product beside pq + fin
            add('%s_free_b%d' % (ds, B), ds, B, 11, ('pq_fin', 'pq_fin', NONE), k0=cell_k0(ds), steps=8 if B == 20 else 6)
    for fp in (1, 4, 8):
        add('M16_fin_parts%d' % fp, 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), fp=fp, k0=2, attn_fin_parts=fp)
    add('MID_fin_parts4', 'MID', 20, 11, ('pq_fin', 'pq_fin', NONE), fp=4, k0=4, attn_fin_parts=4)
    add('MID_b32_fin_parts8', 'MID', 32, 11, ('pre_fin', 'own', NONE), fp=8, k0=4, attn_fin_parts=8)     # 6 + 256 workgroups: no pq + fin
    add('M16_fin_parts3', 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), fp=1, k0=2, attn_fin_parts=3)         # (not 1, 2, 4 or 8: one part)
    add('M16_two_launches', 'M16', 20, 11, ('pre_fin', 'own', NONE), k0=2, steps=8, attn_pq_in_fin=False)
    add('MID_two_launches', 'MID', 20, 11, ('pre_fin', 'own', NONE), k0=4, steps=8, attn_pq_in_fin=False)
    add('M16_two_launches_b3', 'M16', 3, 11, ('pre_fin', 'none', NONE), steps=5, attn_pq_in_fin=False)
    add('M16_whole', 'M16', 20, 11, ('whole', 'none', NONE), fp=1, steps=8, attn_split=False)
    add('M16_no_gate_split', 'M16', 20, 11, ('pq_fin', 'none', NONE), steps=8, split_gates=False)
    for k in range(32, 144, 16):     # every cut st_decoder_forward accepts at M16: 16 * ceil(E / 16) <= k < 16 * 9
        add('M16_cell_k%d' % k, 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), k0=k // 16, steps=8, split_cell_k=k)
    add('M16_two_launches_cell_k96', 'M16', 20, 11, ('pre_fin', 'own', NONE), k0=6, steps=8, attn_pq_in_fin=False, split_cell_k=96)
    add('MID_cell_k160', 'MID', 32, 11, ('pq_fin', 'pq_fin', NONE), k0=10, split_cell_k=160)
    add('M16_pre_parts1', 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), k0=2, steps=8, attn_pre_parts=1)
    add('M16_tf_eval', 'M16', 20, 11, ('pq_fin', 'pq_fin', {'tf'}), mode='tf_eval', k0=2, steps=8)
    add('M16_tf_eval_b3', 'M16', 3, 11, ('pq_fin', 'none', {'tf'}), mode='tf_eval', steps=5)
    add('M16_tf_partial', 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), mode='tf_partial', Bt=12, k0=2, steps=8)
    add('MID_tf_partial', 'MID', 17, 11, ('pq_fin', 'pq_fin', NONE), mode='tf_partial', Bt=5, k0=4)
    add('M16_single_step', 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), k0=2, steps=1)
    add('M16_b1_l1', 'M16', 1, 1, ('pq_fin', 'none', NONE), steps=4)
    # ---- nothing a multiple of 16: the library's own fall-backs (A % 16 != 0: no pq + fin; E % 8 != 0: one fin part; 512 % (E / 4) != 0:
    # no position ranges for long texts either)
    for mode, want in (('free', ('pre_fin', 'none', NONE)), ('train_tf', ('pre_fin', 'none', TRAIN))):
        for B in (3, 20):
            for L in (11, 130):
                add('RAG_%s_b%d_l%d' % (mode, B, L), 'RAG', B, L, want, mode=mode, fp=1, steps=6 if L == 130 else 8)
    # ---- long texts: position ranges
    for B in (3, 20):
        add('M16_l130_b%d' % B, 'M16', B, 130, ('pq_rng', 'none', NONE), steps=6)            # 4 ranges
    add('MID_l130_b17', 'MID', 17, 130, ('pq_rng', 'none', NONE), steps=4)
    add('M16_l344_8_ranges', 'M16', 3, 344, ('pq_rng', 'none', NONE), steps=4)
    add('M16_l345_9_ranges', 'M16', 3, 345, ('fin_split', 'none', NONE), steps=4)
    add('M16_l688_16_ranges', 'M16', 3, 688, ('fin_split', 'none', NONE), steps=4)
    add('M16_l130_three_launches', 'M16', 20, 130, ('fin_split', 'none', NONE), steps=6, attn_rng_one_launch=False)
    add('M16_l130_two_launches', 'M16', 20, 130, ('fin_split', 'none', NONE), steps=6, attn_pq_in_fin=False)
    add('A20_l11_b20', 'A20', 20, 11, ('pre_fin', 'own', NONE), k0=2, steps=8)
    add('A20_l11_b3', 'A20', 3, 11, ('pre_fin', 'none', NONE), steps=5)
    add('A20_l130_b20', 'A20', 20, 130, ('fin_split', 'none', NONE), steps=6)
    add('A20_l130_b3', 'A20', 3, 130, ('fin_split', 'none', NONE), steps=4)
    # ---- teacher-forced training: pre part in the pq launch, cells paired, projection deferred
    for ds in ('M16', 'MID'):
        for B in (17, 20, 32):
            for L in (11, 130):
                add('%s_train_b%d_l%d' % (ds, B, L), ds, B, L, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=cell_k0(ds),
                    steps=(6 if L == 130 else 8) if B == 20 else 4)
    for B in (3, 33):
        add('M16_train_b%d' % B, 'M16', B, 11, ('pre_fin', 'none', TRAIN), mode='train_tf', steps=5)
    add('M16_train_unpaired', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN - {'pair'}), mode='train_tf', k0=2, steps=8, fwd_pair_cells=False)
    add('M16_train_no_gate_split', 'M16', 20, 11, ('pre_fin', 'none', TRAIN), mode='train_tf', steps=8, split_gates_train=False)
    add('M16_train_pre_parts1', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=2, steps=8, attn_pre_parts=1)
    add('M16_train_pre_parts2', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=2, steps=8, attn_pre_parts=2)
    add('M16_train_cell_k96', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=6, steps=8, split_cell_k=96)
    add('M16_train_fin_parts4', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', fp=4, k0=2, steps=8, attn_fin_parts=4)
    add('M16_train_whole', 'M16', 20, 11, ('whole', 'none', {'tf', 'defer', 'pair'}), mode='train_tf', fp=1, steps=8, attn_split=False)
    add('M16_train_partial', 'M16', 20, 11, ('whole', 'none', NONE), mode='train_partial', Bt=12, fp=1, steps=8)
    add('M16_train_single_step', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=2, steps=1)
    # ---- LSTM weights x 2.5: expanding dynamics, so that an error made in one step is not damped in the next
    add('M16_gain_free', 'M16', 20, 11, ('pq_fin', 'pq_fin', NONE), k0=2, steps=8, gain=2.5)
    add('M16_gain_train', 'M16', 20, 11, ('pre_fin', 'pq_pre', TRAIN), mode='train_tf', k0=2, steps=8, gain=2.5)
    add('M16_gain_l130', 'M16', 3, 130, ('pq_rng', 'none', NONE), steps=6, gain=2.5)
    add('MID_gain_free', 'MID', 20, 11, ('pq_fin', 'pq_fin', NONE), k0=4, steps=8, gain=2.5)
    add('RAG_gain_free', 'RAG', 20, 11, ('pre_fin', 'none', NONE), fp=1, steps=8, gain=2.5)
    add('A20_gain_l130', 'A20', 20, 130, ('fin_split', 'none', NONE), steps=6, gain=2.5)
    return out


CASES = _cases()
IDS = [c['id'] for c in CASES]
assert len(set(IDS)) == len(IDS)
BY_ID = dict(zip(IDS, CASES))

# pairs the project states to be bit-identical: the cell's partial product hosted beside pq + fin against a launch of its own behind the
# two-launch form of the attention step (what a starved hand-off degrades to), at the same cut
BIT_IDENTICAL = [('M16_free_b20', 'M16_two_launches'), ('MID_free_b20', 'MID_two_launches'),
                 ('M16_cell_k96', 'M16_two_launches_cell_k96')]


def knobs_of(c):
    return dict(KNOBS, **c['knobs'])


def step_plan(c):
    """(training, steps, step_src, Bt, Tt) of a case, as Decoder.forward / plan_decode arrive at them (tf_rate 1 in every teacher mode;
    a partial teacher is two groups shorter than the run, so that its last frame repeats)"""
    steps, mode = c['steps'], c['mode']
    training = mode.startswith('train')
    if mode == 'free':
        return training, steps, [-1] * steps, c['B'], 0
    Tt = max(1, steps - 2) if c['Bt'] is not None else steps
    return training, steps, [min(t, Tt - 1) for t in range(steps)], c['B'] if c['Bt'] is None else c['Bt'], Tt


def io_plan(c):
    """what Decoder._run_loop puts into the st_decoder_io fields the planner reads, for this case's knobs and mode (booleans stand for
    buffers: the host test gives them fake addresses)"""
    k, B, L = knobs_of(c), c['B'], c['L']
    training, steps, src, Bt, Tt = step_plan(c)
    keep_tapes = training                   # the differentiable path keeps the tapes
    pure_tf = c['mode'] != 'free' and Bt == B and all(src[t] == min(t, Tt - 1) for t in range(steps - 1))
    defer = keep_tapes and pure_tf
    io = dict(steps=steps, step_src=src, teacher=c['mode'] != 'free', Bt=Bt, Tt=Tt, defer=defer, pair=defer and k['fwd_pair_cells'],
              s_buf=False, fin_parts=0, pre_parts=0, split_parts=0, xchg=False, pq_gran=False, gate_part=False, gate_part_k=0)
    if k['attn_split'] and (not training or defer):
        parts = k['attn_pre_parts']
        while parts < 64 and (L + parts - 1) // parts > 512:
            parts *= 2
        io.update(s_buf=True, pre_parts=parts, fin_parts=k['attn_fin_parts'])
        if L >= SPLIT_MIN_LEN and not keep_tapes:
            io['split_parts'] = sp = max(2, min(64, (L + SPLIT_POSITIONS - 1) // SPLIT_POSITIONS))
            io['xchg'] = k['attn_pq_in_fin'] and sp <= 8 and k['attn_rng_one_launch']
        if k['split_gates'] and 16 < B <= 32 and ((not keep_tapes and L < SPLIT_MIN_LEN) or (defer and k['split_gates_train'])):
            io.update(gate_part=True, gate_part_k=k['split_cell_k'])
        io['pq_gran'] = k['attn_pq_in_fin'] and not keep_tapes
    return io
