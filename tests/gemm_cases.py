"""Case tables of the GEMM family -- st_gemm_fwd / st_gemm_fwd_batch and st_gemm_wgrad[_db|_split] / st_gemm_wgrad_batch -- shared by
the host-side dispatch test (test_gemm_dispatch_host.py: every kernel the dispatchers can choose is reached, each row reaches the one
named in it) and the GPU test (test_gpu_gemm_paths.py: every row against a float64 reference).

A forward row: Bn utterances of Tin frames, Cin channels -> N, KT taps, pad, stride, Tout (None: the natural conv length);
  a   -- layout of the activations: 'c' contiguous rows (lda = Cin), 'slice' a column slice (lda = Cin + 4), 'slice2' a column slice
         whose rows are not 16-byte addressable (lda = Cin + 2), 'off1' contiguous rows starting one float past a 16-byte boundary;
  w   -- the weight: 'lin' torch Linear (N, Cin) (KT = 1), 'torch' torch Conv1d (N, Cin, KT), 'tm' tap-major (N, KT, Cin),
         'torch_off1' / 'lin_off1' the same one float past a 16-byte boundary;
  pool -- MaxPool1d(2, 1, 1)[:T] fused into the load of A;  split -- the split-K workspace is passed when st_gemm_splitk_slabs() > 1;
  want -- the variant the dispatcher must choose (fwd_name()).
A weight-gradient row: the same shape keys, dc -- layout of dC: 'c' (lddc = N), 'slice' (columns [4, 4 + N) of rows of N + 8),
  'odd' (columns [1, 1 + N) of rows of N + 3: not 16-byte addressable); a -- 'c' / 'slice' (lda = Cin + 4) / 'slice2' (Cin + 2);
  db, split (cut of the input columns for st_gemm_wgrad_split, KT = 1), acc (accumulate into dW), pool, want (wgrad_name())."""

# ---------------------------------------------------------------- variant codes (include/semitts.h)
FWD_KERNELS = {0: 'gd64x64', 1: 'gd32x64', 2: 'gd64x32', 11: 'elem_adj', 12: 'elem', 13: 'gm_vw', 14: 'gm'}
for _k in range(8):
    FWD_KERNELS[3 + _k] = 'pipe_vw%d_pl%d_mt%d' % ((_k >> 2) & 1, (_k >> 1) & 1, 1 if _k & 1 else 2)
FWD_FINISH = {0: '', 1: 'fin4', 2: 'fin4rt', 3: 'fin1'}
FWD_BATCH_BITS = {1: 'separate', 2: 'gd_batch64x32', 4: 'gd_batch64x64', 8: 'pipe_batch'}
WG_PRODUCTS = {0: 'convw_small', 1: 'dma64', 2: 'dma_rc16_128', 3: 'tn64', 4: 'tn128'}
WG_FLAGS = ((8, 'fold'), (16, 'lin'), (32, 'pool'), (64, 'direct'))
WG_SUMS = {0: '', 1: 'partials', 2: 'tall', 3: 'partials2', 4: 'partials2_split'}


def fwd_name(code):
    """'kernel[/S<slabs>/<finish>]' of a st_gemm_fwd_variant() code"""
    assert code >= 0, code
    k, S, fin = code & 0xff, (code >> 8) & 0xff, code >> 16
    return FWD_KERNELS[k] + ('/S%d/%s' % (S, FWD_FINISH[fin]) if S > 1 else '')


def wgrad_name(code):
    """'product[+flags][/sum]' of a st_gemm_wgrad_variant() code"""
    assert code >= 0, code
    prod, s = code & 0xff, (code >> 8) & 0xff
    name = WG_PRODUCTS[prod & 7] + ''.join('+' + f for b, f in WG_FLAGS if prod & b)
    return name + ('/' + WG_SUMS[s] if s else '')


def wgrad_z(code):
    return code >> 16


# ---------------------------------------------------------------- forward rows
def F(id, Bn, Tin, Cin, N, KT=1, pad=0, stride=1, Tout=None, a='c', w='lin', pool=False, split=True, want=None):
    if Tout is None:
        Tout = (Tin + 2 * pad - KT) // stride + 1
    return dict(id=id, Bn=Bn, Tin=Tin, Tout=Tout, Cin=Cin, N=N, KT=KT, pad=pad, stride=stride, a=a, w=w, pool=pool, split=split,
                want=want)


FWD = [
    # LDS-DMA kernel, no split
    F('postnet_lin_160_1025', 1, 4033, 160, 1025, want='gd64x64'),                       # 64 x 17 tiles >= 1024; M = 63 * 64 + 1
    F('lin_m65_n128_k20', 1, 65, 20, 128, want='gd32x64'),                                 # K tail 20 (not a multiple of 16 / 32)
    F('lin_m33_n64_k36', 1, 33, 36, 64, want='gd32x64'),
    F('lin_slice_m127_n129', 1, 127, 44, 129, a='slice', want='gd64x32'),                  # KT = 1 takes a column slice
    F('bank_k3_80', 2, 37, 80, 80, KT=3, pad=1, w='tm', want='gd64x32'),                   # the CBHG bank at 80 channels
    F('proj_128_80_k3', 3, 29, 128, 80, KT=3, pad=1, w='tm', want='gd64x32'),
    F('conv_stride2_odd', 2, 41, 32, 100, KT=3, pad=1, stride=2, w='tm', want='gd32x64'),   # stride 2, odd Tin
    F('conv_tout_over', 2, 20, 16, 64, KT=4, pad=3, Tout=30, w='tm', want='gd32x64'),      # Tout above the natural length (25)
    F('conv_pad0_m64', 2, 34, 16, 63, KT=3, pad=0, w='tm', want='gd32x64'),                # pad 0: Tout = 32, M = 64; N = 63
    # split-K on the LDS-DMA kernel: S = 2 .. 8 and both finishes
    F('splitk_s2', 1, 4800, 1536, 256, want='gd64x64/S2/fin4'),
    F('splitk_s3', 1, 3520, 1536, 256, want='gd64x64/S3/fin4'),
    F('enc_c2_512x5_s6', 3, 50, 512, 512, KT=5, pad=2, w='tm', want='gd64x64/S6/fin4'),   # the C2 encoder conv
    F('splitk_s4_n257', 1, 63, 1536, 257, want='gd64x64/S4/fin1'),                         # N % 4 != 0: one column per thread
    F('splitk_s5_n50', 1, 100, 2048, 50, want='gd64x64/S5/fin1'),
    F('splitk_s7_conv', 2, 40, 448, 64, KT=6, pad=2, w='tm', want='gd64x64/S7/fin4'),
    F('splitk_s8_m129', 1, 129, 3072, 128, want='gd64x64/S8/fin4'),
    F('proj_640_128_k3', 2, 33, 640, 128, KT=3, pad=1, w='tm', want='gd64x64/S5/fin4'),  # the 640 -> 128 projection
    # the pipelined kernel: 32-row tiles (small grids) ...
    F('pipe_torch_k5', 2, 31, 20, 33, KT=5, pad=2, w='torch', want='pipe_vw0_pl0_mt1'),
    F('pipe_torch_pool', 2, 30, 16, 64, KT=3, pad=1, w='torch', pool=True, want='pipe_vw0_pl1_mt1'),
    F('pipe_tm_slice_k2', 3, 21, 24, 65, KT=2, pad=1, a='slice', w='tm', want='pipe_vw1_pl0_mt1'),
    F('pipe_tm_pool_s2', 2, 33, 16, 31, KT=3, pad=1, stride=2, w='tm', pool=True, want='pipe_vw1_pl1_mt1'),
    F('pipe_lin_pool', 1, 129, 32, 80, pool=True, want='pipe_vw1_pl1_mt1'),
    # ... and split-K inside it (64-row tiles)
    F('pipe_torch_splitk', 2, 24, 256, 64, KT=7, pad=3, w='torch', want='pipe_vw0_pl0_mt2/S4/fin4'),
    F('pipe_torch_pool_splitk', 1, 40, 192, 62, KT=8, pad=4, w='torch', pool=True, want='pipe_vw0_pl1_mt2/S4/fin1'),
    F('pipe_tm_slice_splitk', 2, 30, 256, 64, KT=7, pad=3, a='slice', w='tm', want='pipe_vw1_pl0_mt2/S4/fin4'),
    F('pipe_tm_pool_splitk', 1, 64, 512, 128, KT=4, pad=2, w='tm', pool=True, want='pipe_vw1_pl1_mt2/S5/fin4'),
    # rows that are not 16-byte addressable: the element-wise pipelined form
    F('postnet_dgrad_1025_160', 1, 65, 1025, 160, want='elem_adj'),                       # Linear(160, 1025) input gradient
    F('elem_off1_tm', 2, 17, 16, 40, KT=3, pad=1, a='off1', w='tm', want='elem_adj'),
    F('elem_cin5_torch', 2, 19, 5, 16, KT=3, pad=1, w='torch', want='elem'),
    F('elem_cin7_s2', 3, 25, 7, 33, KT=4, pad=1, stride=2, a='slice2', w='torch', want='elem'),
    # the one-block kernel: Cin < 4, or a fused max-pool on rows that are not 16-byte addressable
    F('locconv_2x31', 4, 40, 2, 32, KT=31, pad=15, w='torch', want='gm'),                 # the attention's location conv
    F('gm_cin1_k16', 2, 50, 1, 17, KT=16, pad=0, w='torch', want='gm'),
    F('gm_cin3_s2', 3, 23, 3, 64, KT=2, pad=1, stride=2, w='torch', want='gm'),
    F('gm_pool_off1_tm', 2, 27, 16, 48, KT=3, pad=1, a='off1', w='tm', pool=True, want='gm_vw'),
    F('gm_pool_slice2_lin', 1, 70, 20, 65, a='slice2', pool=True, want='gm_vw'),
    F('gm_pool_off1_torch', 2, 21, 8, 24, KT=2, pad=1, a='off1', w='torch', pool=True, want='gm'),
]

# batches of forward jobs for st_gemm_fwd_batch: lists of F rows (their 'want' is not used) and the variant bits of the batch
BANK80 = [F('bank%d' % k, 2, 37, 80, 80, KT=k, pad=k // 2, Tout=37, w='tm' if k > 1 else 'lin') for k in range(1, 9)]
FWD_BATCH = [
    dict(id='bank_80_k1_8', jobs=BANK80, want='gd_batch64x32'),
    dict(id='mixed_11_jobs', want='gd_batch64x64', jobs=[          # > 8 jobs of mixed single-call tile forms
        F('j0', 2, 37, 80, 80, KT=3, pad=1, w='tm'), F('j1', 1, 65, 20, 128), F('j2', 1, 33, 36, 64),
        F('j3', 1, 70, 44, 129, a='slice'), F('j4', 2, 37, 80, 80, KT=2, pad=1, Tout=37, w='tm'), F('j5', 1, 31, 16, 33),
        F('j6', 2, 20, 16, 64, KT=4, pad=3, Tout=30, w='tm'), F('j7', 3, 17, 48, 80, KT=5, pad=2, w='tm'),
        F('j8', 1, 129, 64, 80), F('j9', 2, 41, 32, 96, KT=3, pad=1, stride=2, w='tm'), F('j10', 1, 64, 24, 80)]),
    dict(id='pipe_slices', want='pipe_batch', jobs=[
        F('p0', 2, 30, 24, 65, KT=2, pad=1, a='slice', w='tm'), F('p1', 2, 30, 32, 80, KT=3, pad=1, w='tm'), F('p2', 1, 50, 16, 33)]),
    # a job whose taps are not whole 16-float blocks (Cin = 24) would leave the LDS-DMA kernel's k order in a pipelined launch
    dict(id='pipe_cin24_taps', want='separate', jobs=[
        F('u0', 2, 30, 24, 65, KT=2, pad=1, a='slice', w='tm'), F('u1', 2, 30, 24, 80, KT=3, pad=1, w='tm')]),
    dict(id='fallback_pool', want='separate', jobs=[
        F('q0', 2, 30, 16, 64, KT=3, pad=1, w='tm'), F('q1', 2, 30, 16, 64, KT=3, pad=1, w='tm', pool=True)]),
    dict(id='fallback_off1', want='separate', jobs=[F('r0', 1, 40, 16, 64), F('r1', 1, 40, 16, 64, a='off1')]),
    dict(id='fallback_splitk', want='separate', jobs=[F('s0', 1, 63, 1536, 257), F('s1', 1, 65, 20, 128)]),
    dict(id='single_job', want='separate', jobs=[F('t0', 1, 65, 20, 128)]),
]


# ---------------------------------------------------------------- weight-gradient rows
def W(id, Bn, Tin, Cin, N, KT=1, pad=0, Tout=None, dc='c', a='c', db=False, split=0, acc=False, pool=False, want=None):
    if Tout is None:
        Tout = Tin + 2 * pad - KT + 1
    return dict(id=id, Bn=Bn, Tin=Tin, Tout=Tout, Cin=Cin, N=N, KT=KT, pad=pad, dc=dc, a=a, db=db, split=split, acc=acc, pool=pool,
                want=want)


WGRAD = [
    # few input channels: the location conv (2 x 31 -> 32) and its neighbours
    W('locconv_2x31', 8, 45, 2, 32, KT=31, pad=15, Tout=45, want='convw_small/tall'),
    W('locconv_2x31_acc', 8, 45, 2, 32, KT=31, pad=15, Tout=45, acc=True, want='convw_small/tall'),
    W('cs_cin1_k16_trim', 3, 90, 1, 64, KT=16, pad=0, Tout=50, want='convw_small/tall'),   # Tout below the natural 75: unread rows
    W('cs_cin3_k2_tail', 2, 70, 3, 4, KT=2, pad=0, Tout=41, want='convw_small/tall'),
    # register-staged form with folded (channel, tap) columns
    W('fold_cin2_k31_db', 4, 33, 2, 32, KT=31, pad=15, Tout=33, db=True, want='tn64+fold/partials2'),
    W('fold_cin5_k3', 4, 200, 5, 17, KT=3, pad=1, want='tn64+fold/partials'),
    W('fold_cin3_k5_odd_acc', 3, 40, 3, 24, KT=5, pad=2, dc='odd', acc=True, want='tn64+fold/partials'),
    # LDS-DMA 64-tiles
    W('bank_80_k5', 8, 100, 80, 80, KT=5, pad=2, Tout=100, want='dma64/partials'),
    W('bank_80_k4_db_acc', 2, 37, 80, 80, KT=4, pad=2, Tout=37, db=True, acc=True, want='dma64/partials2'),
    W('lin_64x64_tall', 1, 16400, 64, 64, want='dma64+lin/tall'),                        # 128 slabs of a 4096-element matrix
    W('lin_64x64_tall_acc', 1, 16400, 64, 64, acc=True, want='dma64+lin/tall'),
    W('lin_direct_m200', 1, 200, 128, 64, db=True, want='dma64+lin+direct'),
    W('enc_c2_512x5', 4, 100, 512, 512, KT=5, pad=2, want='dma64/partials'),              # the C2 encoder conv
    W('postnet_160_1025', 1, 600, 160, 1024, dc='slice', db=True, want='dma64+lin/partials2'),
    # LDS-DMA 128-tiles: the decoder LSTM's 4096 x 2560 gradient
    W('declstm_4096x2560_direct', 1, 64, 2560, 4096, want='dma_rc16_128+lin+direct'),
    W('declstm_4096x2560_split', 1, 300, 2560, 4096, split=1536, db=True, want='dma_rc16_128+lin/partials2_split'),
    # register-staged 64 / 128-tiles: dC or A not 16-byte addressable, partial pieces, max-pool
    W('tn64_odd_dc_lin', 1, 600, 36, 63, dc='odd', want='tn64+lin/partials'),
    W('tn64_n63_conv_db', 10, 31, 20, 63, KT=2, pad=1, Tout=31, db=True, want='tn64/partials2'),
    W('tn64_pool_k3', 6, 100, 80, 80, KT=3, pad=1, pool=True, want='tn64+pool/partials'),
    W('tn64_pool_k2_acc', 2, 29, 16, 32, KT=2, pad=1, Tout=29, pool=True, acc=True, a='slice', want='tn64+pool/partials'),
    W('tn64_slice2_k1_pad1', 2, 200, 18, 40, KT=1, pad=1, Tout=201, a='slice2', want='tn64/partials'),
    W('tn128_pool_512x512x16', 4, 80, 512, 512, KT=16, pad=8, Tout=80, pool=True, want='tn128+pool/partials'),
    W('tn128_odd_dc_split', 1, 96, 2560, 4096, dc='odd', split=1024, want='tn128+lin/partials2_split'),
    W('split_small_acc_db', 1, 300, 96, 64, split=40, db=True, acc=True, want='dma64+lin/partials2_split'),
    W('split_tall_nodb', 1, 20000, 40, 32, split=8, want='dma64+lin/partials2_split'),
]

# a weight-gradient batch of > 16 jobs: groups of DMA jobs, single calls in between (fold, odd dC, 128-tiles), Z = 1 jobs, a tall-sum
# job and -- the 17th groupable job -- a group of one
_WB = [W('b%d' % k, 2, 37, 80, 80, KT=k, pad=k // 2, Tout=37, db=k % 2 == 0) for k in range(1, 9)] + [
    W('b_fold', 2, 29, 5, 17, KT=3, pad=1), W('b_direct', 1, 200, 128, 64, db=True), W('b_tall', 1, 16400, 64, 64),
    W('b_odd', 1, 129, 36, 64, dc='odd'), W('b_direct2', 1, 100, 64, 32), W('b_lin_db', 1, 600, 160, 96, db=True),
    W('b_c2', 2, 60, 512, 128, KT=5, pad=2), W('b_cs', 8, 45, 2, 32, KT=31, pad=15, Tout=45), W('b_k1', 2, 37, 80, 80, Tout=37),
    W('b_k2', 2, 37, 80, 80, KT=2, pad=1, Tout=37), W('b_db', 1, 300, 96, 64, db=True), W('b_m65', 1, 65, 20, 128)]
WGRAD_BATCH = [dict(id='mixed_%d_jobs' % len(_WB), jobs=_WB)]


def lda_of(c):
    return {'c': c['Cin'], 'slice': c['Cin'] + 4, 'slice2': c['Cin'] + 2, 'off1': c['Cin']}[c['a']]


def a_offset(c):
    """floats between the 16-byte aligned base and the first element of A"""
    return 1 if c['a'] == 'off1' else 0


def w_offset(c):
    return 1 if c['w'].endswith('_off1') else 0


def dc_layout(c):
    """(lddc, dcoff) of a weight-gradient row"""
    return {'c': (c['N'], 0), 'slice': (c['N'] + 8, 4), 'odd': (c['N'] + 3, 1)}[c['dc']]
