"""Case tables of the attention-step backward and the decoder's BPTT loop forms, shared by the host-side dispatch test
(test_attn_bwd_dispatch_host.py: every launch the planners can choose -- and every refusal -- is reached, each row reaches the one named in
it) and the GPU test (test_gpu_attn_bwd.py: every runnable step row and every loop form against a float64 reference).

A step row: B utterances of L positions, A attention dims, E context dims, F location filters, K taps;
  s      -- the forward's S is given (st_attn_bwd_job.s_in; without it the kernel recomputes S from pm and the location conv);
  hosted -- 0 st_attn_step_bwd, 1 st_skinny_linear_packed_lstm_bwd_attn_bwd beside a product of N outputs, 2 st_skinny_partial_attn_bwd;
  parts  -- attention workgroups per utterance (hosted only);  wl -- 'al' a 16-byte aligned W_l, 'off1' one float past a boundary;
  env    -- environment switches of the hosted launches;  gpu -- the GPU test runs the row (the refusals and the longest texts it does not);
  want   -- the launch (step_name()) or the refusal (REFUSALS) st_attn_bwd_variant reports."""

# ---------------------------------------------------------------- st_attn_bwd_variant codes (include/semitts.h)
KERNELS = {0: 'plain', 1: 'hosted', 2: 'fallback', 3: 'dual', 4: 'nb2', 5: 'parts2', 6: 'parts4', 7: 'partial', 8: 'partial_kw16'}
REFUSALS = {-1: 'refused_dims', -2: 'refused_lds', -3: 'refused_needs_s', -4: 'refused_parts', -5: 'refused_partial'}
FLAGS = ((32, 'opt'), (64, 's'), (128, 'wlf'), (256, 'mpf'))

# the LDS limits at the full-size attention (A = 256, E = 512, F = 32, K = 31), pinned by the host test
WIDE_LAST = 168            # last L of the 48-position block on its own
WIDE_HOSTED_LAST = 137     # ... next to a hosting product's 8 KB (st_attn_bwd_wide_fits: the split forms' limit)
NARROW_S_LAST = 350        # last L of the 16-position block with S
NARROW_LAST = 230          # ... without S
HOSTED_LAST = 320          # last L the hosted launch shares a workgroup with its product (then: the two launches in turn)


def step_name(code):
    """'kernel.w48|w16[.opt][.s][.wlf][.mpf]' of an st_attn_bwd_variant() code, or the refusal's name"""
    if code < 0:
        return REFUSALS[code]
    return KERNELS[code & 15] + ('.w48' if code & 16 else '.w16') + ''.join('.' + n for b, n in FLAGS if code & b)


def S(id, L, B=3, A=256, E=512, F=32, K=31, s=True, hosted=0, parts=1, N=512, wl='al', env=(), gpu=True, want=None):
    return dict(id=id, L=L, B=B, A=A, E=E, F=F, K=K, s=s, hosted=hosted, parts=parts, N=N, wl=wl, env=tuple(env), gpu=gpu, want=want)


FULL = '.s.wlf.mpf'
STEP = [
    # the plain launch with S: the wide block up to WIDE_LAST (its image alone is > 64 KiB at A = 256: opt-in), then the narrow one
    S('s_L1', 1, want='plain.w48.opt' + FULL),
    S('s_L15', 15, want='plain.w48.opt' + FULL),
    S('s_L16', 16, want='plain.w48.opt' + FULL),
    S('s_L17', 17, want='plain.w48.opt' + FULL),
    S('s_L47', 47, want='plain.w48.opt' + FULL),
    S('s_L48', 48, want='plain.w48.opt' + FULL),
    S('s_L49', 49, B=2, want='plain.w48.opt' + FULL),
    S('s_L168', WIDE_LAST, B=2, want='plain.w48.opt' + FULL),
    S('s_L169', WIDE_LAST + 1, B=2, want='plain.w16.opt' + FULL),
    S('s_L350', NARROW_S_LAST, B=1, want='plain.w16.opt' + FULL),
    S('s_L351', NARROW_S_LAST + 1, B=1, gpu=False, want='refused_lds'),
    # without S (the kernel runs the location conv and S = pq + pm + W_l loc itself): always the narrow block
    S('nos_L1', 1, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L16', 16, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L17', 17, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L48', 48, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L49', 49, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L230', NARROW_LAST, B=1, s=False, want='plain.w16.opt.wlf.mpf'),
    S('nos_L231', NARROW_LAST + 1, B=1, s=False, gpu=False, want='refused_lds'),
    # small images (<= 64 KiB: no opt-in), scalar W_l loads (ragged F or a misaligned W_l), no memory prefetch (E > 512), ragged dims
    S('small_A32_F8_K7', 11, B=5, A=32, E=28, F=8, K=7, s=False, want='plain.w16.mpf'),
    S('small_A32_F8_K7_s', 11, B=5, A=32, E=28, F=8, K=7, want='plain.w48.s.mpf'),
    S('A128_wl_off1', 43, B=4, A=128, wl='off1', want='plain.w48.opt.s.mpf'),
    S('A128_wl_off1_nos', 43, B=4, A=128, wl='off1', s=False, want='plain.w16.opt.mpf'),
    S('A64_E768', 40, B=3, A=64, E=768, want='plain.w48.opt.s.wlf'),
    S('A256_E768_nos', 33, B=2, E=768, s=False, want='plain.w16.opt.wlf'),
    S('F31_K33', 50, B=3, A=128, F=31, K=33, want='plain.w48.opt.s.mpf'),
    S('F31_K33_nos', 50, B=3, A=128, F=31, K=33, s=False, want='plain.w16.opt.mpf'),
    S('A192', 20, A=192, gpu=False, want='refused_dims'),
    S('E30', 20, E=30, gpu=False, want='refused_dims'),
    S('F33', 20, F=33, gpu=False, want='refused_dims'),
    S('K30', 20, K=30, gpu=False, want='refused_dims'),
    # hosted beside a product (S is required): whole step per workgroup, wide up to WIDE_HOSTED_LAST, then narrow, then two launches
    S('h1_L43', 43, B=3, hosted=1, want='hosted.w48.opt' + FULL),
    S('h1_L137', WIDE_HOSTED_LAST, B=2, hosted=1, want='hosted.w48.opt' + FULL),
    S('h1_L138', WIDE_HOSTED_LAST + 1, B=2, hosted=1, want='hosted.w16.opt' + FULL),
    S('h1_L320', HOSTED_LAST, B=1, hosted=1, want='hosted.w16.opt' + FULL),
    S('h1_L321', HOSTED_LAST + 1, B=1, hosted=1, want='fallback.w16.opt' + FULL),
    S('h1_L350', NARROW_S_LAST, B=1, hosted=1, gpu=False, want='fallback.w16.opt' + FULL),
    S('h1_L351', NARROW_S_LAST + 1, B=1, hosted=1, gpu=False, want='refused_lds'),
    S('h1_small', 11, B=5, A=32, E=28, F=8, K=7, hosted=1, want='hosted.w48.s.mpf'),
    S('h1_nos', 43, hosted=1, s=False, gpu=False, want='refused_needs_s'),
    # hosted, split over the attention dims: two parts (dual / NB2 / generic) and four (lean)
    S('h2_dual_B32', 43, B=32, hosted=1, parts=2, want='dual.w48.opt' + FULL),
    S('h2_dual_B17_L137', WIDE_HOSTED_LAST, B=17, hosted=1, parts=2, want='dual.w48.opt' + FULL),
    S('h2_nb2_B32', 49, B=32, hosted=1, parts=2, env=('ST_AB_NB2',), want='nb2.w48.opt' + FULL),
    S('h2_nodual_B32', 43, B=32, hosted=1, parts=2, env=('ST_AB_NO_DUAL',), want='parts2.w48.opt' + FULL),
    S('h2_generic_B16', 43, B=16, hosted=1, parts=2, want='parts2.w48.opt' + FULL),
    S('h2_generic_B33', 20, B=33, hosted=1, parts=2, want='parts2.w48.opt' + FULL),
    S('h2_generic_wide_N', 43, B=20, N=3840, hosted=1, parts=2, gpu=False, want='parts2.w48.opt' + FULL),   # tiles + 2 B > 256
    S('h4_B20_L43', 43, B=20, hosted=1, parts=4, want='parts4.w48' + FULL),
    S('h4_B5_L88', 88, B=5, hosted=1, parts=4, want='parts4.w48' + FULL),
    S('h4_B5_L89', 89, B=5, hosted=1, parts=4, want='parts4.w48.opt' + FULL),
    S('h4_B2_L137', WIDE_HOSTED_LAST, B=2, hosted=1, parts=4, want='parts4.w48.opt' + FULL),
    S('h3', 43, B=20, hosted=1, parts=3, gpu=False, want='refused_parts'),
    S('h4_A32', 43, B=20, A=32, E=28, F=8, K=7, hosted=1, parts=4, gpu=False, want='refused_parts'),
    # the K-split partial product beside the two-part form (16 < B <= 32)
    S('p_B32', 43, B=32, hosted=2, parts=2, N=512, want='partial.w48.opt' + FULL),
    S('p_B17_L137', WIDE_HOSTED_LAST, B=17, hosted=2, parts=2, N=512, want='partial.w48.opt' + FULL),
    S('p_kw16_B20', 49, B=20, hosted=2, parts=2, N=512, env=('ST_PART_KW16',), want='partial_kw16.w48.opt' + FULL),
    S('p_B16', 43, B=16, hosted=2, parts=2, gpu=False, want='refused_partial'),
    S('p_parts1', 43, B=32, hosted=2, parts=1, gpu=False, want='refused_partial'),
    S('p_nos', 43, B=32, hosted=2, parts=2, s=False, gpu=False, want='refused_partial'),
]


# ---------------------------------------------------------------- st_decoder_bwd_forms rows
# dims of the full-size decoder (helpers.FULL_CFG): P 256, Q = D = 1024, E 512, A 256, F 32, K 31
FULL_DIMS = dict(B=32, L=43, E=512, P=256, Q=1024, D=1024, A=256, F=32, K=31)


def D(id, want, fuse=True, overlap=True, s_tape=True, parts=2, dsplits=2, qsplits=4, dxd_part=True, dxq_part=True, Bp=None, **dims):
    d = dict(FULL_DIMS, **dims)
    return dict(id=id, dims=d, fuse=fuse, overlap=overlap, s_tape=s_tape, parts=parts, dsplits=dsplits, qsplits=qsplits,
                dxd_part=dxd_part, dxq_part=dxq_part, Bp=d['B'] if Bp is None else Bp, want=want)


def forms_name(word):
    """'six' | 'fused' | 'overlap' | 'split<parts>[.d<S>][.q<S>]' of an st_decoder_bwd_forms() word"""
    if not word & 8:
        return 'six'
    if not word & 16:
        return 'fused'
    parts = (word >> 8) & 15
    if parts == 1:
        assert word & 7 == 0, word
        return 'overlap'
    ds, qs = (word >> 12) & 15, (word >> 16) & 15
    assert (word & 1) and bool(word & 2) == (ds > 0) and bool(word & 4) == (qs > 0), word
    return 'split%d' % parts + ('.d%d' % ds if ds else '') + ('.q%d' % qs if qs else '')


FORMS = [
    D('six', 'six', fuse=False),
    D('fused', 'fused', overlap=False),
    D('no_s_tape', 'fused', s_tape=False),
    D('overlap_parts1', 'overlap', parts=1),
    D('split2_default', 'split2.d2.q4'),
    D('split4', 'split4', parts=4),
    D('parts3', 'overlap', parts=3),
    D('dsplits1', 'split2.d1.q4', dsplits=1),
    D('dsplits4', 'split2.d4.q4', dsplits=4),
    D('dsplits5', 'split2', dsplits=5),            # 4 D / 16 = 256 k-blocks do not split in 5: no partial product
    D('dsplits3', 'split2', dsplits=3),
    D('qsplits1', 'split2.d2.q1', qsplits=1),
    D('qsplits2', 'split2.d2.q2', qsplits=2),
    D('qsplits5', 'split2.d2', qsplits=5),                               # more than four slabs: the whole product
    D('qsplits3', 'split2.d2', qsplits=3),
    D('no_dxd_part', 'split2', dxd_part=False),
    D('no_dxq_part', 'split2.d2', dxq_part=False),
    D('B16', 'split2', B=16),
    D('B17', 'split2.d2.q4', B=17),
    D('B20_pad', 'split2', B=20, Bp=32),
    D('B20', 'split2.d2.q4', B=20),
    D('B33', 'split2', B=33),
    D('B1', 'split2', B=1),
    D('L137', 'split2.d2.q4', L=137),
    D('L138', 'overlap', L=138),
    D('L138_parts4', 'overlap', L=138, parts=4),
    D('F31', 'overlap', F=31),
    D('K33', 'overlap', K=33),
    D('A128', 'split2.d2.q4', A=128),
    D('A128_parts4', 'split4', A=128, parts=4),
    D('A192', 'overlap', A=192),
    D('A64_parts4', 'split4', A=64, parts=4),                            # 16 dims per part
    D('A32_parts4', 'overlap', A=32, parts=4),                           # 8 dims per part: not whole MFMA tiles
]
