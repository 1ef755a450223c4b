"""Case tables, input generator, float64 reference and error bounds of the forward attention step, shared by the host-side test
(test_attn_fwd_dispatch_host.py: every row reaches the launch or refusal named in it, the reference agrees with the oracle, the bounds
are neither slack nor blind) and the GPU test (test_gpu_attn_fwd.py: every runnable row against the float64 reference).

No GPU and no library in here.  A row: B utterances of L positions, A attention dims, E context dims, F location filters, K taps;
  part   -- 'whole' st_attn_step_fwd | 'prefin' st_attn_pre_fwd + st_attn_fin_fwd | 'split' st_attn_fin_split_fwd (S given) |
            'cf' st_skinny_linear_packed_attnpre_fwd with cf_out (the location conv on its own);
  pre, fin -- workgroups per utterance of the pre part (position ranges) and of the fin part (context slices; 'split': position ranges);
  opts   -- operand options: 'wl_off1' W_l one float past a 16-byte boundary, 'ld' w_prev / w_out / ctx at leading dimensions larger
            than their widths, 't16' T16 context alone, 'nat_t16' natural + one T16, 't16x3' three T16 destinations at k-block offsets
            inside wider buffers, 'adain', 'adain_t16' (a refusal), 'mem_off1' / 'pq_off1' a misaligned operand (refusals);
  special -- None (Gaussian) | 'sat' | 'onehot' | 'equal' | 'zero_hist' (see gen_inputs) | 'plan_only' (no operands are made);
  gpu    -- the GPU test runs the row;
  want   -- plan_name() of the launch (for 'prefin' of the pre launch; want_fin of the fin launch), or the refusal."""
import math

import torch

U = 2.0 ** -24            # float32 unit roundoff
TANH_ERR = 2e-7           # absolute error of the kernels' fast tanh, as attention_body.h states it ("|error| <= ~2e-7")
FLOOR = 2.0 ** -126       # the hardware exp flushes denormal results: a weight below this may read as 0

# ---------------------------------------------------------------- st_attn_fwd_variant (include/semitts.h)
AL = dict(pm=1, pq=2, v=4, wl=8, mem=16, s=32, ws=64)
AL_ALL = 127
REFUSALS = {-1: 'refused_dims', -2: 'refused_k_even', -3: 'refused_e', -4: 'refused_align', -5: 'refused_lds', -6: 'refused_parts',
            -7: 'refused_range_dims', -8: 'refused_lp'}


def plan_name(rc, plan):
    """'vec|scalar[.wlv][.mfma].kp32|kgen[.opt]' of the pre part and the whole step, 'vec|scalar[.opt]' of the fin part,
    'ranges<parts>x<Lp>' of the position-range form, or the refusal's name.  plan: dict of the st_attn_fwd_plan fields + 'part'"""
    if rc < 0:
        return REFUSALS[rc]
    if plan['part'] == 3:
        return 'ranges%dx%d' % (plan['parts'], plan['Lp'])
    s = 'vec' if plan['vec'] else 'scalar'
    if plan['part'] != 2:
        s += ('.wlv' if plan['wl_vec'] else '') + ('.mfma' if plan['s_mfma'] else '') + ('.kp32' if plan['kp32'] else '.kgen')
    return s + ('.opt' if plan['opt_in'] else '')


# ---------------------------------------------------------------- restatement of at_pos_per / at_layout (attention_body.h)
AT_THREADS, AT_LP, AT_CB = 512, 6, 4


def pos_per(L, nparts):
    return ((-(-L // nparts) + 11) // 12) * 12 if nparts > 1 else L


def pre_parts_eff(parts):
    return parts if 2 <= parts <= 64 and parts & (parts - 1) == 0 else 1


def lds_bytes(part, L, A, E, F, K, pre_parts=1, s_mfma=False):
    """dynamic LDS of a workgroup of part 0 (whole), 1 (pre), 2 (fin): W_l^T [F][A4 + 4] (whole; pre without MFMA), conv filters
    [F][2][kp] and the padded history [2][hl] (not fin), conv features [F][cf_ld] (not fin), energies [L4], context partials [4 x 512]"""
    Lh = pos_per(L, pre_parts) if part == 1 else L
    up4 = lambda n: (n + 3) & ~3
    p = 0
    if part == 0 or (part == 1 and not s_mfma):
        p += F * (up4(A) + 4)
    kp = 32 if K <= 32 else up4(K)
    if part != 2:
        p += F * 2 * kp
        p += 2 * up4(Lh + AT_CB + kp + 3)
        p += F * (up4(-(-Lh // AT_LP) * AT_LP + AT_CB) + (16 if part == 1 else 0))
    p += up4(L) + 4 * AT_THREADS
    return 4 * p


# the limits at the full-size attention (A = 256, E = 512, F = 32, K = 31), pinned by the host test
WHOLE_64K_LAST = 102       # last L of the whole step within 64 KiB (no opt-in)
WHOLE_LAST = 804           # last L of the whole step within 160 KiB
PRE1_64K_LAST = 324        # the pre part on the matrix cores, one range
PRE1_LAST = 1032
FIN_64K_LAST = 14336       # the fin part (any dims: energies + context partials)
LP_LAST = 512              # positions per range of st_attn_fin_split_fwd


# ---------------------------------------------------------------- inputs
def gen_inputs(c):
    """float32 operands of a row, seeded by the row's id: pq (B, A), pm (B, L, A), mem (B, L, E) standard Gaussian; the conv and W_l
    weights Gaussian x 0.3; v Gaussian x A^-0.5 (energies are O(1)); w_prev a softmax, w_cum the sum of two; AdaIN operands (Q = 12).
    special: 'sat' -- pq[:, 0] = 60, pq[:, 1 % A] = -60 (every tanh argument of those dims saturates); 'onehot' -- v rescaled to
    sum |v| = 400 and position L // 2 given pq + pm = 60 sign(v) (its energy is 400, more than 100 above every other);
    'equal' -- v = 0; 'zero_hist' -- w_prev = w_cum = 0"""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c['id'])) % (2 ** 31))
    B, L, A, E, F, K, Q = c['B'], c['L'], c['A'], c['E'], c['F'], c['K'], 12
    r = lambda *s: torch.randn(*s, generator=g)
    x = dict(pq=r(B, A), pm=r(B, L, A), mem=r(B, L, E), wc=r(F, 2, K) * 0.3, wl=r(A, F) * 0.3, v=r(A) * A ** -0.5)
    x['w_prev'] = torch.softmax(r(B, L), -1)
    x['w_cum'] = x['w_prev'] + torch.softmax(r(B, L), -1)
    x['hq'], x['std'], x['mean'] = r(B, Q), torch.relu(r(B, Q)), r(B, Q)
    sp = c.get('special')
    if sp == 'sat':
        x['pq'][:, 0], x['pq'][:, 1 % A] = 60.0, -60.0
    elif sp == 'onehot':
        x['v'] = x['v'] * (400.0 / float(x['v'].abs().sum()))
        sgn = torch.where(x['v'] >= 0, 1.0, -1.0)
        x['pm'][:, L // 2, :] = 60.0 * sgn - x['pq']
        x['wl'] = x['wl'] * 0.0        # (no location term: the peak's arguments stay saturated)
    elif sp == 'equal':
        x['v'] = x['v'] * 0.0
    elif sp == 'zero_hist':
        x['w_prev'], x['w_cum'] = x['w_prev'] * 0.0, x['w_cum'] * 0.0
    return x


# ---------------------------------------------------------------- float64 reference
def conv_features(w_prev, w_cum, wc, shift=0, reverse=False, swap=False, zero_from=None):
    """cf[b, l, f] = sum_c sum_k wc[f, c, k] hist[b, c, l + k - pad], hist = [w_prev; w_cum], pad = (K - 1) / 2, zero outside [0, L)
    (ref: location conv of Attention.forward, src/module.py:371-388).  The keyword arguments are the DEFECTS of the host test."""
    K = wc.shape[2]
    pad = (K - 1) // 2 + shift
    hist = torch.stack([w_cum, w_prev] if swap else [w_prev, w_cum], 1)            # (B, 2, L)
    L = hist.shape[2]
    w = wc.flip(2) if reverse else wc
    hp = torch.zeros(hist.shape[0], 2, L + 2 * K + 2, dtype=hist.dtype)
    hp[:, :, K + 1:K + 1 + L] = hist
    win = hp.unfold(2, K, 1)                                                       # win[b, c, i, k] = hp[b, c, i + k]
    win = win[:, :, K + 1 - pad:K + 1 - pad + L]                                   # i = l + K + 1 - pad: hist[l + k - pad]
    cf = torch.einsum('bclk,fck->blf', win, w)
    if zero_from is not None and zero_from < L:      # defect: the range starting at zero_from sees zero history before it
        h2 = hist.clone()
        h2[:, :, :zero_from] = 0
        hp2 = torch.zeros_like(hp)
        hp2[:, :, K + 1:K + 1 + L] = h2
        win2 = hp2.unfold(2, K, 1)[:, :, K + 1 - pad:K + 1 - pad + L]
        cf2 = torch.einsum('bclk,fck->blf', win2, w)
        cf = torch.cat([cf[:, :zero_from], cf2[:, zero_from:]], 1)
    return cf


def reference(x, S_in=None, defect=None):
    """Attention.forward + the state update in float64 (ref: src/module.py:371-407, :262-264, AdaIN :267-269), from the formulas of
    include/semitts.h.  x: operands (any float dtype); S_in: S is given (the fin forms).  defect: one of DEFECTS (host test only)."""
    d = {k: t.double() for k, t in x.items()}
    kw = {}
    if defect == 'taps_reversed':
        kw['reverse'] = True
    elif defect == 'window_plus1':
        kw['shift'] = 1
    elif defect == 'window_minus1':
        kw['shift'] = -1
    elif defect == 'channels_swapped':
        kw['swap'] = True
    elif isinstance(defect, tuple) and defect[0] == 'range_zero_history':
        kw['zero_from'] = defect[1]
    cf = conv_features(d['w_prev'], d['w_cum'], d['wc'], **kw)
    loc = cf @ d['wl'].t()
    S = d['pm'] + loc if S_in is None else S_in.double()
    t = torch.tanh(d['pq'].unsqueeze(1) + S)
    v = d['v']
    if defect == 'last_dim_dropped':
        e = t[..., :-1] @ v[:-1]
    else:
        e = t @ v
    if defect == 'last_position_dropped':
        w = torch.cat([torch.softmax(e[:, :-1], -1), torch.zeros_like(e[:, -1:])], 1)
    else:
        w = torch.softmax(e, -1)
    cum = w + (d['w_prev'] if defect == 'cum_from_w_prev' else d['w_cum'])
    if defect == 'last_memory_row_dropped':
        ctx = torch.einsum('bl,ble->be', w[:, :-1], d['mem'][:, :-1])
    else:
        ctx = torch.einsum('bl,ble->be', w, d['mem'])
    return dict(cf=cf, loc=loc, S=S, e=e, w=w, cum=cum, ctx=ctx, hadapt=d['std'] * (d['hq'] - d['mean']))


DEFECTS = ('taps_reversed', 'window_plus1', 'window_minus1', 'channels_swapped', 'cum_from_w_prev', 'last_position_dropped',
           'last_memory_row_dropped', 'last_dim_dropped', 'range_zero_history')


def expressible(defect, c):
    """does the defect change anything at this row's shape? (and the argument of 'range_zero_history': the first position of the
    second pre range)"""
    if c['part'] == 'cf' and defect not in ('taps_reversed', 'window_plus1', 'window_minus1', 'channels_swapped', 'range_zero_history'):
        return False
    if defect == 'taps_reversed':         # (one position sees the centre tap alone)
        return c['K'] > 1 and c['L'] > 1
    if defect in ('last_position_dropped', 'last_memory_row_dropped'):
        return c['L'] > 1
    if defect == 'last_dim_dropped':      # (one position: the weight is 1 whatever the energy)
        return c['A'] > 1 and c['L'] > 1
    if defect == 'range_zero_history':       # needs a second range that holds positions and a window that reaches back
        pp = pre_parts_eff(c['pre'])
        return c['part'] in ('prefin', 'cf') and pp > 1 and pos_per(c['L'], pp) < c['L'] and c['K'] > 1
    return True


LAM = 8.0                 # confidence factor of the rounding model (see bounds)
MFMA_ORDER = [k + 8 * g for k in range(8) for g in range(4)]      # filters in the order the 8 MFMA steps of the pre part take them


def _chain_var(terms):
    """sum of squared partial sums of a chain of fmas over the last axis (a step that adds an exact zero rounds nothing)"""
    s = terms.cumsum(-1)
    return ((s * s) * (terms != 0)).sum(-1)


def bounds(x, ref, form, E_slices=1, ranges=1, mfma=False):
    """Per-element bounds of |kernel - float64| for cf (B, L, F), S (B, L, A), w, cum (B, L) and ctx (B, E), from the operand magnitudes
    of the row.  form: 'whole' | 'pre' (cf and S only; mfma: S on the matrix cores) | 'fin' (S is an exact input) | 'ranges' (the
    same, over `ranges` position ranges).

    Model.  Every float32 rounding is off by at most u = 2^-24 times the value it rounds.  A worst-case sum of those (n u sum |terms|
    for an n-term product, then again through the F-term and the A-term sums) is 30 to 100 times what the arithmetic does and would
    let a wrong kernel pass; instead the roundings are taken as independent and zero-mean: an output whose first-order error is
    sum_i c_i d_i, |d_i| <= u, is held to LAM u sqrt(sum_i c_i^2) with LAM = 8 (Hoeffding: exceeded with probability below
    2 exp(-32) per element).  V_q below is sum c_i^2 of quantity q; the values being rounded come from the float64 reference, the
    partial sums in the kernel's order.  What is not a rounding -- the fast tanh -- is added in full, with the worst sign.

      cf   2K products in one fma chain, channel by channel, taps ascending:  V_cf = sum_i s_i^2 over the chain's partial sums s_i
      loc  sum_f W_l[a][f] cf[f], one fma chain over f (matrix cores: 8 steps of 4 filters, taken in turn), on the rounded cf:
                                                                             V_loc = sum_f W_l^2 V_cf + sum_f s_f^2
      S    one addition of pm, the output's last rounding (taken in full):   b_S = LAM u sqrt(V_loc) + u |S|
      x    whole: (pq + loc) + pm, two roundings; fin: pq + S, one:          V_x = V_loc + (pq + loc)^2 + x^2   [fin: x^2]
      e    v . tanh(x); the kernel forms sum_a v_a r_a, r = 1 / (1 + exp(2x)), 4 fmas per lane, then vsum - 2 acc (vsum = the lane's
           sum of v, 3 roundings), a round per 256 dims, a 6-step tree over the 64 lanes (taken over aligned blocks of lanes):
                                                                             V_e = sum_a (v_a tanh'(x_a))^2 V_x + V_tree
           the fast tanh is off by at most TANH_ERR per dim, whatever the sign: T_e = TANH_ERR sum |v|
      w    w_l = exp(e_l - m) / sum_j exp(e_j - m):  dw_l = w_l (de_l - sum_j w_j de_j), so
             roundings of e:   w_l LAM u sqrt((1 - w_l)^2 V_e[l] + sum_{j != l} w_j^2 V_e[j])
             the fast tanh:    w_l 2 (1 - w_l) T_e
             the softmax's own roundings, relative and added up plainly: the subtraction and the exponential's argument reduction
             (2u d_l, d_l = m - e_l, capped at 104 where the weight underflows), the exponential (4u), the same for the terms of the
             sum (weighted mean d_w = sum_j w_j d_j), the sum (ceil(L / 64) serial terms per lane + 6 tree steps), the division (2u):
                               w_l u (2 d_l + 2 d_w + ceil(L / 64) + 18)
             position ranges: the rescale exp(m_p - M) / D of a range (another 2u d_l + 6u) and the sum over the ranges (ranges u)
           + FLOOR (the hardware exponential flushes denormal results)
      cum  w + w_cum_prev, one rounding:                                     b_cum = b_w + u |cum|
      ctx  sum_l w_l mem_l on the rounded weights, whose errors share causes (no independence taken): sum_l b_w |mem|; each thread
           chains ceil(L / ng) fmas over its rows (ng = 512 / (E / (4 slices)) row groups) and the ng partial sums are added in
           turn, plainly:                                                    + u (ceil(L / ng) + ng) sum_l w |mem|
           position ranges: per range, then `ranges` fmas with rounded scales: + u (ranges + 4) sum_l w |mem|"""
    d = {k: t.double() for k, t in x.items()}
    K, F, A = d['wc'].shape[2], d['wc'].shape[0], d['wl'].shape[0]
    B, L, E = d['mem'].shape
    out = {}
    pq = d['pq'].unsqueeze(1)
    if form in ('whole', 'pre'):
        pad = (K - 1) // 2
        hist = torch.stack([d['w_prev'], d['w_cum']], 1)
        hp = torch.zeros(B, 2, L + 2 * pad, dtype=torch.float64)
        hp[:, :, pad:pad + L] = hist
        win = hp.unfold(2, K, 1)                                                   # (B, 2, L, K)
        prod = win.unsqueeze(1) * d['wc'].unsqueeze(0).unsqueeze(3)                # (B, F, 2, L, K)
        V_cf = _chain_var(prod.permute(0, 3, 1, 2, 4).reshape(B, L, F, 2 * K))     # (B, L, F)
        out['cf'] = LAM * U * V_cf.sqrt()
        order = MFMA_ORDER if mfma else list(range(F))
        V_loc = torch.empty(B, L, A, dtype=torch.float64)
        for b in range(B):      # (per utterance: the (L, A, F) products of a long text are large)
            t = ref['cf'][b].unsqueeze(1) * d['wl'].unsqueeze(0)                   # (L, A, F)
            V_loc[b] = _chain_var(t[..., order]) + V_cf[b] @ (d['wl'] ** 2).t()
        out['S'] = LAM * U * V_loc.sqrt() + U * ref['S'].abs()
        if form == 'pre':
            return out
        xarg = (pq + ref['loc']) + d['pm']
        V_x = V_loc + (pq + ref['loc']) ** 2 + xarg ** 2
    else:
        xarg = pq + ref['S']
        V_x = xarg ** 2
    th = torch.tanh(xarg)
    v = d['v']
    # the energy reduction: lane = 4 consecutive dims, rounds of 256 dims, a tree over the 64 lanes
    Ap = -(-A // 256) * 256
    padA = lambda t: torch.nn.functional.pad(t, (0, Ap - A))
    q = padA(v * (1 - th) / 2).reshape(B, L, Ap // 256, 64, 4)
    V_tree = _chain_var(q).sum((-1, -2))
    v4 = padA(v).reshape(Ap // 256, 64, 4)
    V_tree = V_tree + ((v4[..., 0] + v4[..., 1]) ** 2 + (v4[..., 2] + v4[..., 3]) ** 2 + v4.sum(-1) ** 2).sum()
    z = padA(v * th).reshape(B, L, Ap // 256, 64, 4).sum(-1)                       # vsum - 2 acc of a lane and round
    V_tree = V_tree + (z ** 2).sum((-1, -2))
    y = z.cumsum(2)                                                                # esum += ... over the rounds
    V_tree = V_tree + (y[:, :, 1:] ** 2).sum((-1, -2))
    y = y[:, :, -1]
    for _ in range(6):
        y = y.reshape(B, L, -1, 2).sum(-1)
        V_tree = V_tree + (y ** 2).sum(-1)
    V_e = ((v * (1 - th ** 2)) ** 2 * V_x).sum(-1) + V_tree                        # (B, L)
    T_e = TANH_ERR * float(v.abs().sum())
    w = ref['w']
    m = ref['e'].amax(-1, keepdim=True)
    dl = (m - ref['e']).clamp(max=104.0)
    dw = (w * dl).sum(-1, keepdim=True)
    wV = (w ** 2 * V_e).sum(-1, keepdim=True)
    rnd = LAM * U * ((1 - w) ** 2 * V_e + (wV - w ** 2 * V_e).clamp(min=0)).sqrt()
    own = U * (2 * dl + 2 * dw + math.ceil(L / 64) + 18)
    if form == 'ranges':
        own = own + U * (2 * dl + 6 + ranges)
    out['w'] = w * (rnd + 2 * (1 - w) * T_e + own) + FLOOR
    out['cum'] = out['w'] + U * ref['cum'].abs()
    ng = AT_THREADS // max(1, E // (4 * E_slices))
    Lr = -(-L // ranges)
    wm = torch.einsum('bl,ble->be', w, d['mem'].abs())
    out['ctx'] = torch.einsum('bl,ble->be', out['w'], d['mem'].abs()) + U * (math.ceil(Lr / ng) + ng + (ranges + 4 if form == 'ranges' else 0)) * wm
    return out


# ---------------------------------------------------------------- rows
FULL = dict(A=256, E=512, F=32, K=31)
SMALL = dict(A=24, E=40, F=8, K=7)            # vector, W_l through LDS, E / 4 = 10 (idle context threads, integer-division path)
A24F32 = dict(A=24, E=40, F=32, K=7)          # vector, F = 32 but no whole MFMA tiles
SCAL = dict(A=20, E=24, F=3, K=3)             # scalar W_l
A18 = dict(A=18, E=24, F=8, K=7)              # A % 4 != 0: guarded loads, masked pad columns
A3 = dict(A=3, E=8, F=4, K=3)
A320 = dict(A=320, E=512, F=32, K=31)         # second round of the dims loop; MFMA fragments fetched in place
F31K33 = dict(A=32, E=64, F=31, K=33)         # generic conv, scalar
F4K35 = dict(A=16, E=32, F=4, K=35)           # generic conv, vector
K1 = dict(A=24, E=40, F=8, K=1)


def R(id, part, L, dims, B=2, pre=1, fin=1, opts=(), special=None, gpu=True, want=None, want_fin=None):
    return dict(id=id, part=part, L=L, B=B, pre=pre, fin=fin, opts=tuple(opts), special=special, gpu=gpu, want=want, want_fin=want_fin, **dims)


LENGTHS = (1, 2, 5, 6, 7, 12, 13, 16, 17, 47, 48, 49, 64, 65)
ROWS = []
for _L in LENGTHS:      # the block edges of every phase: 4 (conv), 6 (energies), 12 (pre ranges), 16 (MFMA tiles), 48 (one round), 64 (softmax)
    ROWS.append(R('whole_full_L%d' % _L, 'whole', _L, FULL, want='vec.wlv.kp32'))
    ROWS.append(R('whole_small_L%d' % _L, 'whole', _L, SMALL, B=3, want='vec.wlv.kp32'))
    ROWS.append(R('prefin_full_L%d' % _L, 'prefin', _L, FULL, want='vec.wlv.mfma.kp32', want_fin='vec'))
    ROWS.append(R('prefin_small_L%d' % _L, 'prefin', _L, SMALL, B=3, want='vec.wlv.kp32', want_fin='vec'))
ROWS += [
    # ---- every dim set, whole and in two parts
    R('whole_a24f32', 'whole', 13, A24F32, B=3, want='vec.wlv.kp32'),
    R('prefin_a24f32', 'prefin', 29, A24F32, B=3, pre=2, want='vec.wlv.kp32', want_fin='vec'),
    R('whole_scal', 'whole', 70, SCAL, want='scalar.kp32'),
    R('prefin_scal', 'prefin', 70, SCAL, pre=2, want='scalar.kp32', want_fin='scalar'),
    R('whole_a18', 'whole', 19, A18, B=3, want='scalar.wlv.kp32'),
    R('prefin_a18', 'prefin', 19, A18, B=3, want='scalar.wlv.kp32', want_fin='scalar'),
    R('whole_a3', 'whole', 9, A3, B=5, want='scalar.wlv.kp32'),
    R('prefin_a3', 'prefin', 9, A3, B=5, want='scalar.wlv.kp32', want_fin='scalar'),
    R('whole_a320', 'whole', 43, A320, want='vec.wlv.kp32'),
    R('prefin_a320', 'prefin', 50, A320, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('whole_f31k33', 'whole', 40, F31K33, want='scalar.kgen'),
    R('prefin_f31k33', 'prefin', 40, F31K33, pre=2, want='scalar.kgen', want_fin='scalar'),
    R('whole_f4k35', 'whole', 40, F4K35, want='vec.wlv.kgen'),
    R('prefin_f4k35', 'prefin', 40, F4K35, pre=2, want='vec.wlv.kgen', want_fin='vec'),
    R('whole_k1', 'whole', 13, K1, B=3, want='vec.wlv.kp32'),
    R('prefin_k1', 'prefin', 13, K1, B=3, pre=2, want='vec.wlv.kp32', want_fin='vec'),
    R('whole_wl_off1', 'whole', 43, FULL, opts=('wl_off1',), want='scalar.kp32'),
    R('prefin_wl_off1', 'prefin', 43, FULL, opts=('wl_off1',), want='scalar.kp32', want_fin='vec'),
    # ---- the existing shapes of test_attention_step (the bounds are held to the project's thresholds there)
    R('whole_full_L43', 'whole', 43, FULL, B=4, want='vec.wlv.kp32'),
    R('whole_full_L171', 'whole', 171, FULL, B=2, want='vec.wlv.kp32.opt'),
    # ---- the LDS limits of the whole step at the full size
    R('whole_full_64k_last', 'whole', WHOLE_64K_LAST, FULL, B=1, want='vec.wlv.kp32'),
    R('whole_full_64k_first', 'whole', WHOLE_64K_LAST + 1, FULL, B=1, want='vec.wlv.kp32.opt'),
    R('whole_full_last', 'whole', WHOLE_LAST, FULL, B=1, want='vec.wlv.kp32.opt'),
    R('whole_full_refused', 'whole', WHOLE_LAST + 1, FULL, B=1, want='refused_lds'),
    R('pre_full_64k_last', 'prefin', PRE1_64K_LAST, FULL, B=1, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('pre_full_64k_first', 'prefin', PRE1_64K_LAST + 1, FULL, B=1, fin=8, want='vec.wlv.mfma.kp32.opt', want_fin='vec'),
    R('pre_full_last', 'prefin', PRE1_LAST, FULL, B=1, fin=8, want='vec.wlv.mfma.kp32.opt', want_fin='vec'),
    R('pre_full_refused', 'prefin', PRE1_LAST + 1, FULL, B=1, want='refused_lds', want_fin='vec'),
    # (the fin part's image is the energies and the context partials: its opt-in starts past L = 14336; plan only)
    R('fin_full_64k_last', 'prefin', FIN_64K_LAST, FULL, B=1, pre=64, special='plan_only', gpu=False, want='vec.wlv.mfma.kp32.opt', want_fin='vec'),
    R('fin_full_64k_first', 'prefin', FIN_64K_LAST + 1, FULL, B=1, pre=64, special='plan_only', gpu=False, want='vec.wlv.mfma.kp32.opt', want_fin='vec.opt'),
    # ---- pre parts: empty ranges (L = 5, 4 parts), a one-position range (13 = 12 + 1), exact multiples of 12; 8 runs as 8, 3 as 1
]
for _L in (5, 12, 13, 24, 25, 49):
    for _p in (2, 4):
        ROWS.append(R('pre%d_full_L%d' % (_p, _L), 'prefin', _L, FULL, pre=_p, want='vec.wlv.mfma.kp32', want_fin='vec'))
    ROWS.append(R('pre2_small_L%d' % _L, 'prefin', _L, SMALL, B=3, pre=2, want='vec.wlv.kp32', want_fin='vec'))
ROWS += [
    R('pre8_full_L100', 'prefin', 100, FULL, B=1, pre=8, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('pre3_full_L49', 'prefin', 49, FULL, pre=3, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('pre2_full_L25_k31', 'prefin', 25, FULL, B=3, pre=2, want='vec.wlv.mfma.kp32', want_fin='vec'),     # the window crosses the boundary both ways
    R('pre4_scal_L50', 'prefin', 50, SCAL, pre=4, want='scalar.kp32', want_fin='scalar'),
    # ---- fin parts (context slices)
    R('fin2_full_L43', 'prefin', 43, FULL, fin=2, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('fin4_full_L43', 'prefin', 43, FULL, fin=4, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('fin8_full_L43', 'prefin', 43, FULL, fin=8, want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('fin8_full_L385', 'prefin', 385, FULL, B=1, fin=8, want='vec.wlv.mfma.kp32.opt', want_fin='vec'),   # past the 384 prefetched rows of a 64-dim slice
    R('fin2_small_L13', 'prefin', 13, SMALL, B=3, fin=2, want='vec.wlv.kp32', want_fin='vec'),              # Es / 4 = 5
    R('fin2_scal_L20', 'prefin', 20, SCAL, fin=2, want='scalar.kp32', want_fin='scalar'),                   # Es / 4 = 3
    R('fin4_small_refused', 'prefin', 13, SMALL, fin=4, gpu=True, want='vec.wlv.kp32', want_fin='refused_parts'),   # 40 % 16 != 0
    R('fin3_full_refused', 'prefin', 13, FULL, fin=3, want='vec.wlv.mfma.kp32', want_fin='refused_parts'),
    # ---- position ranges (st_attn_fin_split_fwd; S is an input)
    R('split_lp44', 'split', 88, FULL, B=2, fin=2, want='ranges2x44'),            # the 44 prefetched memory rows of a range
    R('split_lp45', 'split', 90, FULL, B=2, fin=2, want='ranges2x45'),
    R('split_lp64', 'split', 128, FULL, B=1, fin=2, want='ranges2x64'),           # the 64 prefetched S rows (8 per wave)
    R('split_lp65', 'split', 130, FULL, B=1, fin=2, want='ranges2x65'),
    R('split_lp512', 'split', 1024, dict(A=32, E=64, F=8, K=7), B=1, fin=2, want='ranges2x512'),
    R('split_lp513', 'split', 1026, dict(A=32, E=64, F=8, K=7), B=1, fin=2, want='refused_lp'),
    R('split_L9_p4', 'split', 9, FULL, B=3, fin=4, want='ranges3x3'),             # the trailing empty part is trimmed
    R('split_L3_p64', 'split', 3, FULL, B=3, fin=64, want='ranges3x1'),
    R('split_p1', 'split', 40, FULL, fin=1, want='refused_parts'),
    R('split_p65', 'split', 400, FULL, B=1, fin=65, want='refused_parts'),
    R('split_a320', 'split', 40, A320, fin=2, want='refused_range_dims'),
    R('split_e40', 'split', 40, SMALL, fin=2, want='refused_range_dims'),
    R('split_a4', 'split', 23, dict(A=4, E=16, F=4, K=3), B=5, fin=3, want='ranges3x8'),
    R('split_small_L171_p7', 'split', 171, dict(A=24, E=64, F=8, K=7), B=3, fin=7, want='ranges7x25'),
    # ---- outputs and strides
    R('whole_ld', 'whole', 13, SMALL, B=3, opts=('ld',), want='vec.wlv.kp32'),
    R('whole_full_ld', 'whole', 49, FULL, B=2, opts=('ld',), want='vec.wlv.kp32'),
    R('prefin_ld', 'prefin', 49, FULL, B=2, pre=2, fin=2, opts=('ld',), want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('split_ld', 'split', 90, FULL, B=2, fin=4, opts=('ld',), want='ranges4x23'),
    R('whole_t16', 'whole', 13, SMALL, B=3, opts=('t16',), want='vec.wlv.kp32'),
    R('whole_nat_t16', 'whole', 13, SMALL, B=3, opts=('nat_t16',), want='vec.wlv.kp32'),
    R('whole_t16x3', 'whole', 43, FULL, B=5, opts=('t16x3',), want='vec.wlv.kp32'),
    R('fin_t16x3', 'prefin', 43, FULL, B=5, fin=2, opts=('t16x3',), want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('split_t16x3', 'split', 90, FULL, B=5, fin=2, opts=('t16x3',), want='ranges2x45'),
    R('whole_adain', 'whole', 13, SMALL, B=3, opts=('adain',), want='vec.wlv.kp32'),
    R('whole_full_adain', 'whole', 43, FULL, B=2, opts=('adain',), want='vec.wlv.kp32'),
    R('whole_adain_t16', 'whole', 13, SMALL, B=3, opts=('adain_t16',), want='vec.wlv.kp32'),      # refused by the entry point (not a launch decision)
    # ---- the location conv on its own (cf_out, through the hosted pre part)
    R('cf_vec_L13', 'cf', 13, SMALL, B=3, pre=1, want='vec.wlv.kp32'),
    R('cf_scal_L29_p2', 'cf', 29, SCAL, B=3, pre=2, want='scalar.kp32'),
    # ---- refusals of the launch plan
    R('whole_k_even', 'whole', 13, dict(A=24, E=40, F=8, K=6), want='refused_k_even'),
    R('whole_e_odd', 'whole', 13, dict(A=24, E=42, F=8, K=7), want='refused_e'),
    R('whole_e_wide', 'whole', 13, dict(A=24, E=2052, F=8, K=7), gpu=False, want='refused_e'),
    R('whole_l0', 'whole', 0, SMALL, gpu=False, want='refused_dims'),
    R('whole_mem_off1', 'whole', 13, SMALL, opts=('mem_off1',), want='refused_align'),
    R('whole_pq_off1', 'whole', 13, SMALL, opts=('pq_off1',), want='refused_align'),
    R('whole_a18_pq_off1', 'whole', 13, A18, opts=('pq_off1',), want='scalar.wlv.kp32'),              # A % 4 != 0: no alignment asked of pq
    R('split_pq_off1', 'split', 40, FULL, fin=2, opts=('pq_off1',), want='refused_align'),
    # ---- special values
    R('whole_sat', 'whole', 13, SMALL, B=3, special='sat', want='vec.wlv.kp32'),
    R('whole_full_sat', 'whole', 49, FULL, special='sat', want='vec.wlv.kp32'),
    R('split_sat', 'split', 90, FULL, fin=2, special='sat', want='ranges2x45'),
    R('whole_onehot', 'whole', 13, SMALL, B=3, special='onehot', want='vec.wlv.kp32'),
    R('whole_full_onehot', 'whole', 49, FULL, special='onehot', want='vec.wlv.kp32'),
    R('prefin_onehot', 'prefin', 49, FULL, fin=2, special='onehot', want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('split_onehot', 'split', 90, FULL, fin=2, special='onehot', want='ranges2x45'),
    R('whole_equal_L16', 'whole', 16, SMALL, B=3, special='equal', want='vec.wlv.kp32'),
    R('whole_full_equal_L64', 'whole', 64, FULL, special='equal', want='vec.wlv.kp32'),
    R('split_equal_L128', 'split', 128, FULL, fin=4, special='equal', want='ranges4x32'),
    R('prefin_zero_hist', 'prefin', 49, FULL, pre=2, special='zero_hist', want='vec.wlv.mfma.kp32', want_fin='vec'),
    R('prefin_small_zero_hist', 'prefin', 13, SMALL, B=3, special='zero_hist', want='vec.wlv.kp32', want_fin='vec'),
    R('prefin_scal_zero_hist', 'prefin', 13, SCAL, B=3, special='zero_hist', want='scalar.kp32', want_fin='scalar'),
]
assert len({c['id'] for c in ROWS}) == len(ROWS)

REFUSED_BY_ENTRY = ('whole_adain_t16',)       # rows the entry point refuses before it plans a launch


def align_bits(c):
    """ST_ATTN_AL_* mask of the row's operands"""
    al = AL_ALL
    for o, bit in (('wl_off1', 'wl'), ('mem_off1', 'mem'), ('pq_off1', 'pq')):
        if o in c['opts']:
            al &= ~AL[bit]
    return al


def is_gaussian(c):
    return c['special'] is None
