"""Case tables of the BatchNorm column reductions and the GRU layer, shared by the host-side test (test_norm_rnn_dispatch_host.py: every
GRU kernel and every chunking regime of the column reductions is reached, each row reaches the one named in it) and the GPU tests
(test_gpu_batchnorm.py, test_gpu_gru.py: the rows against float64 references).

GRU row: hidden size H, the kernel st_gru_seq_fwd must launch (fwd) and the one st_gru_seq_bwd must launch (bwd), named as GRU_VARIANTS.

BatchNorm row: M rows; the row-split reductions (st_bn_stats, st_bn_bwd_reduce, the bank kernels) cut them into chunks =
clamp(M / 32, 1, 128) chunks of rpc = ceil(M / chunks) rows, the last `empty` of which hold no row and the last non-empty one `last`
rows.  The merge kernels keep 8 chunks for each of 16 lanes in registers: chunks >= 16 live in register slots j >= 1."""

# ---------------------------------------------------------------- GRU (include/semitts.h: ST_GRU_*)
GRU_VARIANTS = {0: 'tri', 1: 'quad', 2: 'reg32', 3: 'general', -1: 'refused'}
GRU_MAX_H = 341                              # 3H <= 1024: one thread per gate row


def gru_name(code):
    return GRU_VARIANTS[code]


def G(H, fwd, bwd):
    return dict(id='H%d' % H, H=H, fwd=fwd, bwd=bwd)


GRU = [
    G(1, 'tri', 'tri'),
    G(8, 'tri', 'tri'),
    G(83, 'tri', 'tri'),
    G(84, 'tri', 'tri'),                      # 4 waves x 21 units: the last H the three-lane kernels take
    G(85, 'quad', 'reg32'),
    G(127, 'quad', 'reg32'),
    G(128, 'quad', 'reg32'),                  # 4 KQ = 128 padded entries exactly
    G(129, 'general', 'general'),
    G(200, 'general', 'general'),
    G(341, 'general', 'general'),
    G(342, 'refused', 'refused'),
]
GRU_RUNNABLE = [g for g in GRU if g['fwd'] != 'refused']
# T: 1 (one step), 7 / 8 / 9 (around the 8-step input prefetch block of the forward, the 4-step block of the backward), 258 (the CBHG)
GRU_T = (1, 7, 8, 9, 258)


def gru_fwd_rows():
    """(H, T, B, ndir) of the forward test: every H at T = 258 with both directions, and the short-T cases on the H at the edges of
    every kernel, alternating B = 1 / 3 and ndir = 1 / 2 (the full product would be 200 runs of the float64 recurrence)"""
    rows = [(g['H'], 258, 3, 2) for g in GRU_RUNNABLE]
    i = 0
    for H in (1, 84, 85, 128, 129, 341):
        for T in GRU_T[:-1]:
            rows.append((H, T, 1 + 2 * (i % 2), 1 + (i // 2) % 2))
            i += 1
    return rows


# ---------------------------------------------------------------- BatchNorm column reductions
CHUNK_ROWS = 32                              # st_colreduce_chunks: M / 32 chunks ...
MAX_CHUNKS = 128                             # ... at most 128 (8 register slots x 16 lanes of the merge kernels)
MERGE_LANES = 16


def chunking(M):
    """(chunks, rows per chunk, trailing empty chunks, rows of the last non-empty chunk) of the row split, as the kernels compute it"""
    chunks = min(max(M // CHUNK_ROWS, 1), MAX_CHUNKS)
    rpc = -(-M // chunks)
    used = -(-M // rpc)
    return chunks, rpc, chunks - used, M - (used - 1) * rpc


def B(M, chunks, rpc, empty, last, note=''):
    return dict(id='M%d' % M, M=M, chunks=chunks, rpc=rpc, empty=empty, last=last, note=note)


BN_ROWS = [
    B(1, 1, 1, 0, 1),
    B(2, 1, 2, 0, 2),
    B(31, 1, 31, 0, 31),
    B(32, 1, 32, 0, 32),
    B(33, 1, 33, 0, 33),
    B(64, 2, 32, 0, 32),
    B(65, 2, 33, 0, 32),
    B(2064, 64, 33, 1, 18, 'speech encoder after the stride-2 layer (16 x 129)'),
    B(4095, 127, 33, 2, 3),
    B(4096, 128, 32, 0, 32),
    B(4097, 128, 33, 3, 5),
    B(4128, 128, 33, 2, 3, 'speech encoder, cycle test (16 x 258)'),
    B(8256, 128, 65, 0, 1, 'CBHG at C4 (32 x 258): a one-row last chunk'),
    B(8288, 128, 65, 0, 33, 'CBHG even-k segment at C4 (32 x 259)'),
    B(16512, 128, 129, 0, 129, 'C3 encoder (64 x 258)'),
    B(33024, 128, 258, 0, 258),
]
BN_N = (1, 17, 64, 65, 80, 512)
# column windows of a wider buffer: (coff, ld - coff - N): 'c' the whole row, 'off' columns [3, 3 + N) of rows of N + 7 floats
BN_LAYOUTS = {'c': (0, 0), 'off': (3, 4)}


def bn_stat_rows():
    """(M, N, layout) of the statistics test: every M with the N and the layout cycling, every N at the cycle test's M = 4128 in
    both layouts, and the production widths at the largest M"""
    rows = [(r['M'], BN_N[i % len(BN_N)], 'c' if i % 2 == 0 else 'off') for i, r in enumerate(BN_ROWS)]
    rows += [(4128, N, lay) for N in BN_N for lay in BN_LAYOUTS]
    rows += [(16512, 80, 'off'), (33024, 512, 'c'), (8256, 80, 'c')]
    return sorted(set(rows))
