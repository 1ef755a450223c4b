"""Case tables and float64 references of the small kernels between the products of a decode step and of its backward step, and of the
unpacked skinny products -- shared by the host-side test (test_step_glue_host.py: the references agree with float64 torch.autograd, every
cell a kernel can be run at has a case) and the GPU test (test_gpu_step_glue.py: every case against these references).

Pure torch on the CPU: nothing here needs a GPU or the HIP library.

  st_prenet_norm_fwd / _bwd   prenet_fwd_cases / prenet_bwd_cases, prenet_fwd_ref / prenet_bwd_ref, norm_bounds
  st_lstm_cell_bwd_pointwise  LSTM_PW_COMBOS x LSTM_PW_SHAPES, lstm_pw_ref (values and first-order error bounds)
  st_act_bwd                  ACT_BWD_SHAPES, act_bwd_ref
  st_decoder_pack_dout / st_decoder_unpack_out   PACK_CASES, pack_ref / unpack_ref
  st_decoder_dteacher_sum     DTEACHER_CASES, dteacher_ref
  st_adain_bwd                ADAIN_CASES, adain_ref
  st_scalar_combine / st_scalar_fanout / st_scale_by   SCALAR_CASES, SCALE_BY_N
  st_skinny_linear_fwd / st_lstm_cell_fwd / st_skinny_linear_pair_fwd / st_lstm_cell_pair_fwd
                              SK_LINEAR, SK_CELL, SK_LINEAR_PAIR, SK_CELL_PAIR, sk_nb / sk_vec (the dispatch rule of skinny.hip restated)"""
import itertools
import math

import torch

U = 2.0 ** -24                 # float32 unit roundoff
ST_SCALAR_MAX = 8              # include/semitts.h
GRID_CAP = 4096 * 256          # the elementwise launches cap their grid at 4096 workgroups of 256 threads (blocks_for() in grad.hip, the
#                                same cap written out in decoder_bwd.hip and loss.hip): past this many elements the grid-stride loop runs again
ACTS = {0: 'none', 1: 'relu', 2: 'tanh', 3: 'sigmoid'}      # ST_ACT_*


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ===================================================================================================== T16 layout
def kb16(k):
    return (int(k) + 15) // 16


def t16_index(b, k, kb_stride):
    """float index of element (b, k) of a T16 buffer (include/semitts.h): [batch tile of 16][k block of 16][lane 0..63][4 floats], element
    (r, k) of a block at lane 16 * ((k >> 2) & 3) + (r & 15), component k & 3.  b, k: broadcastable int64 tensors"""
    return (((b >> 4) * kb_stride + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (b & 15)) * 4 + (k & 3)


def t16_floats(B, kb_stride):
    return ((B + 15) // 16) * kb_stride * 256


def t16_positions(rows, K, kb_stride, kb0):
    """(len(rows), K) float indices of the logical elements (rows x columns 0..K-1 of the view that starts at k-block kb0)"""
    b = torch.as_tensor(list(rows), dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :] + 16 * kb0
    return t16_index(b, k, kb_stride)


# ===================================================================================================== prenet norm
PN_MODES = (1, 2, 3)                       # LayerNorm, eval BatchNorm1d, training BatchNorm1d
PN_P = (8, 80, 256, 257, 1024, 1040)       # 80: ragged last k-block; 257: second workgroup of the column-per-thread modes; 1024 | 1040: NR_REG
PN_B = (1, 5, 17, 33)
PN_ROWS = (1, 5, 33)
PN_EPS, PN_MOMENTUM = 1e-5, 0.3            # a momentum that is not nn.BatchNorm1d's default
PN_KB0, PN_KB_EXTRA = 2, 3                 # destination view: two k-blocks before the layer, three after it


def prenet_fwd_cases():
    out = []
    for mode, P, B in itertools.product(PN_MODES, PN_P, PN_B):
        for b0 in sorted({0, 3, B - 2}):
            if 0 <= b0 < B:
                for mask in (False, True):
                    out.append(dict(mode=mode, P=P, B=B, b0=b0, mask=mask, ldy=P + 5, ldmask=P + 3, kb0=PN_KB0,
                                    kb_stride=kb16(P) + PN_KB0 + PN_KB_EXTRA))
    return out


def prenet_bwd_cases():
    return [dict(mode=mode, P=P, rows=rows, ld=P + 7, ldy=P + 6) for mode, P, rows in itertools.product(PN_MODES, PN_P, PN_ROWS)]


def prenet_has_big_mean(mode, rows, P):
    """whether prenet_input puts a mean of 1e4 at unit spread into the normalised direction (a one-pass variance loses all 24 bits there)"""
    return (mode == 1 and rows >= 2) or (mode != 1 and P >= 2 and (mode == 2 or rows >= 2))


def prenet_input(mode, B, b0, P, seed):
    """y (B, P), gamma, beta, running mean / var (P).  Among the rows b0.. that are normalised: mode 1 -- row b0 + 1 has mean 1e4; modes
    2 / 3 -- column 1 has mean 1e4 (mode 2: with a running mean next to it)"""
    g = gen(seed)
    y = torch.randn(B, P, generator=g)
    gamma, beta = torch.rand(P, generator=g) + 0.5, torch.randn(P, generator=g) * 0.5
    rm, rv = torch.randn(P, generator=g) * 0.3, torch.rand(P, generator=g) + 0.5
    if prenet_has_big_mean(mode, B - b0, P):
        if mode == 1:
            y[b0 + 1] += 1e4
        else:
            y[b0:, 1] += 1e4
            if mode == 2:
                rm[1] += 1e4
    return y, gamma, beta, rm, rv


def prenet_mask(B, P, seed):
    """dropout mask already scaled by 1 / (1 - p), p = 0.5"""
    return (torch.rand(B, P, generator=gen(seed)) > 0.5).float() * 2


def _pn_stats(x, mode, rm, rv):
    if mode == 1:
        return x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    if mode == 2:
        return rm.double()[None], rv.double()[None]
    return x.mean(0, keepdim=True), x.var(0, unbiased=False, keepdim=True)


def prenet_fwd_ref(y, mode, gamma, beta, rm, rv, eps, momentum, mask, b0):
    """float64 statement of st_prenet_norm_fwd on rows b0..: (out (B - b0, P), new running mean, new running var).  The running
    statistics come back None where the call must leave them alone (modes 1 and 2); the new running variance is None for a batch of one
    row (its unbiased variance does not exist: nn.BatchNorm1d refuses that input, the header promises nothing for it)"""
    x = y[b0:].double()
    mean, var = _pn_stats(x, mode, rm, rv)
    out = torch.relu((x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double())
    if mask is not None:
        out = out * mask[b0:].double()
    if mode != 3:
        return out, None, None
    new_rm = (1 - momentum) * rm.double() + momentum * mean[0]
    new_rv = (1 - momentum) * rv.double() + momentum * x.var(0, unbiased=True) if x.shape[0] > 1 else None
    return out, new_rm, new_rv


def prenet_bwd_ref(dn, y, mode, gamma, rm, rv, eps):
    """float64 closed form of st_prenet_norm_bwd: (dx, dgamma, dbeta) of one call (what autograd gives through F.layer_norm, eval
    F.batch_norm, training F.batch_norm -- test_step_glue_host.py holds it to that)"""
    x, d, g = y.double(), dn.double(), gamma.double()[None]
    mean, var = _pn_stats(x, mode, rm, rv)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rs
    dgamma, dbeta = (d * xh).sum(0), d.sum(0)
    if mode == 2:
        return g * rs * d, dgamma, dbeta
    dim = 1 if mode == 1 else 0
    gg = d * g
    dx = rs * (gg - gg.mean(dim, keepdim=True) - xh * (gg * xh).mean(dim, keepdim=True))
    return dx, dgamma, dbeta


def norm_bounds(x, gg, dim, eps, k):
    """First-order error bounds of a two-pass normalisation over `dim` of float64 x (the bounds of test_layer_norm_forward_and_backward
    in test_gpu_kernel_edges.py, with the reduced dimension a parameter).  k = the additions in the longest chain of the mean + 8:
      mean:  |d mean| <= k u max|x| (with the division)
      xhat:  dxh = k u (max|x| rstd + |xhat|)  -- inherits d mean * rstd and the rstd error k u |xhat|
      dx = rstd (g - mean g - xhat mean(g xhat)), g = dy * gamma (`gg`): the two means carry k u of mean |.|, the xhat error enters through
           xhat * s2 and through s2 itself (<= max|g| dxh); 2 u for the last subtractions and the product; the whole times 4.
    -> (xhat, rstd, dxh, tdx); tdx is None when gg is"""
    mu = x.mean(dim, keepdim=True)
    rs = 1.0 / torch.sqrt(x.var(dim, unbiased=False, keepdim=True) + eps)
    xh = (x - mu) * rs
    dxh = k * U * (x.abs().amax(dim, keepdim=True) * rs + xh.abs())
    if gg is None:
        return xh, rs, dxh, None
    s1, s2 = gg.mean(dim, keepdim=True), (gg * xh).mean(dim, keepdim=True)
    ax = gg.abs().amax(dim, keepdim=True)
    tdx = 4 * rs * (k * U * (gg.abs() + gg.abs().mean(dim, keepdim=True) + xh.abs() * (gg * xh).abs().mean(dim, keepdim=True))
                    + dxh * s2.abs() + xh.abs() * ax * dxh.amax(dim, keepdim=True) + 2 * U * (gg - s1 - xh * s2).abs())
    return xh, rs, dxh, tdx


def prenet_k(mode, rows, P):
    """additions in the longest chain of a mean + 8 (norm_bounds): mode 1 -- a lane adds ceil(P / 64) columns, then 6 wave levels (the k of
    test_layer_norm_forward_and_backward); mode 3 -- one thread adds the `rows` rows of its column in order"""
    return (math.ceil(P / 64) if mode == 1 else rows) + 8


# ===================================================================================================== LSTM cell backward, pointwise
# (dh1, dh2 state, mask, c_prev): dh2 state 0 absent, 1 present, 2 present with scale2 -- scale2 only ever next to dh2: 2 * 3 * 2 * 2 = 24
LSTM_PW_COMBOS = [dict(dh1=a, dh2=b >= 1, scale2=b == 2, mask=c, c_prev=d)
                  for a, b, c, d in itertools.product((False, True), (0, 1, 2), (False, True), (False, True))]
LSTM_PW_SHAPES = ((1, 4), (5, 40), (17, 52), (33, 64))
LSTM_PW_T16 = (None, dict(kb0=1, kb_extra=2))       # no T16 copy | a view one k-block into a buffer two k-blocks wider than 4H + 1


def lstm_pw_inputs(B, H, seed):
    """fp32 operands of one step: activated gates (B, 4, H) in (i, f, g, o) order, c = f c_prev + i g, the dh addends, scale2, mask, dc"""
    g = gen(seed)
    z = torch.randn(B, 4, H, generator=g) * 1.5
    gates = torch.stack([torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])], 1).contiguous()
    c_prev = torch.randn(B, H, generator=g)
    d = dict(gates=gates, c_prev=c_prev, dh0=torch.randn(B, H, generator=g), dh1=torch.randn(B, H, generator=g),
             dh2=torch.randn(B, H, generator=g), scale2=torch.rand(B, H, generator=g) + 0.5,
             mask=(torch.rand(B, H, generator=g) > 0.1).float() / 0.9, dc=torch.randn(B, H, generator=g))
    return d


def lstm_pw_c(inp, with_c_prev):
    """the cell state the forward kept on its tape, in fp32 (c_prev absent = zeros)"""
    g = inp['gates']
    return (g[:, 1] * inp['c_prev'] + g[:, 0] * g[:, 2]) if with_c_prev else (g[:, 0] * g[:, 2])


def lstm_pw_ref(dh0, dh1, dh2, scale2, mask, gates, c, c_prev, dc_in):
    """float64 formula of the pointwise half of nn.LSTMCell's backward on the fp32 values the kernel reads (absent operands None).
    -> (dgates (B, 4H), dc_out (B, H), tol_dgates, tol_dc): the tolerances count the roundings of the float32 evaluation, first order, the
    whole times 2 (the suite's margin for second-order terms):
      dh = (dh0 + dh1 + dh2 s) m: at most 4 roundings of at most sum |addend| |m|                           e_dh = 4u sum|.| |m|
      tc = tanhf(c): 2 ulp = 4u absolute (|tc| < 1);  1 - tc^2: 2 * 4u from tc, 2u of its own                = 10u absolute
      T = dh o (1 - tc^2): e_T = |o| (e_dh (1 - tc^2) + |dh| 10u) + 3u |T|;  dc = dc_in + T: e_dc = e_T + u (|dc_in| + |T|)
      di = dc g i (1 - i), df = dc c_prev f (1 - f): e_dc |factor| + 5u |value|      (1 - i rounds relative to itself, i being given)
      dg = dc i (1 - g^2): e_dc |i (1 - g^2)| + 3u |dc i| + 3u |dg|                 (1 - g^2: 2u absolute)
      do = dh tc o (1 - o): e_dh |tc o (1 - o)| + 4u |dh o (1 - o)| + 5u |do|        (4u: tanhf)
      dc_out = dc f: e_dc |f| + u |dc f|"""
    D = lambda t: None if t is None else t.double()
    dh0, dh1, dh2, scale2, mask, gates, c, c_prev, dc_in = map(D, (dh0, dh1, dh2, scale2, mask, gates, c, c_prev, dc_in))
    gi, gf, gg, go = gates[:, 0], gates[:, 1], gates[:, 2], gates[:, 3]
    dh, mag = dh0.clone(), dh0.abs()
    if dh1 is not None:
        dh, mag = dh + dh1, mag + dh1.abs()
    if dh2 is not None:
        t = dh2 * scale2 if scale2 is not None else dh2
        dh, mag = dh + t, mag + t.abs()
    if mask is not None:
        dh, mag = dh * mask, mag * mask.abs()
    e_dh = 4 * U * mag
    tc = torch.tanh(c)
    cp = c_prev if c_prev is not None else torch.zeros_like(c)
    T = dh * go * (1 - tc * tc)
    dc = dc_in + T
    e_dc = go.abs() * (e_dh * (1 - tc * tc) + dh.abs() * 10 * U) + 3 * U * T.abs() + U * (dc_in.abs() + T.abs())
    d0, d1 = dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf)
    d2, d3 = dc * gi * (1 - gg * gg), dh * tc * go * (1 - go)
    t0 = e_dc * (gg * gi * (1 - gi)).abs() + 5 * U * d0.abs()
    t1 = e_dc * (cp * gf * (1 - gf)).abs() + 5 * U * d1.abs()
    t2 = e_dc * (gi * (1 - gg * gg)).abs() + 3 * U * (dc * gi).abs() + 3 * U * d2.abs()
    t3 = e_dh * (tc * go * (1 - go)).abs() + 4 * U * (dh * go * (1 - go)).abs() + 5 * U * d3.abs()
    dc_out = dc * gf
    t_dc = e_dc * gf.abs() + U * dc_out.abs()
    return torch.cat([d0, d1, d2, d3], 1), dc_out, 2 * torch.cat([t0, t1, t2, t3], 1), 2 * t_dc


# ===================================================================================================== st_act_bwd
ACT_BWD_SHAPES = ((1, 1), (7, 33), (300, 257), (4100, 257))       # the last: 4100 * 257 > GRID_CAP, the grid-stride loop runs a second pass
ACT_BWD_PAD = dict(ldd=3, ldo=5, ldm=2, ldp=7)                    # every stride = N + this


def act_bwd_ref(dout, out, act, mask):
    """float64 dpre = dout * mask * act'(out) and its bound: 1 - out^2 (2u absolute) or out (1 - out) (2u relative) and two products: at
    most 3u |dout mask| + 3u |dpre|, times 2.  No activation and ReLU round nothing but the mask product (bit equality with float32)"""
    d = dout.double() * (mask.double() if mask is not None else 1.0)
    o = out.double() if out is not None else None
    name = ACTS[act]
    if name == 'relu':
        d_act = (o > 0).double()
    elif name == 'tanh':
        d_act = 1 - o * o
    elif name == 'sigmoid':
        d_act = o * (1 - o)
    else:
        d_act = 1.0
    ref = d * d_act
    return ref, 2 * (3 * U * d.abs() + 3 * U * ref.abs())


# ===================================================================================================== decoder pack / unpack
def _pk(id, B, Bp, steps, r, n_mels, pad):
    return dict(id=id, B=B, Bp=Bp, steps=steps, r=r, n_mels=n_mels, ld=r * n_mels + pad)


PACK_CASES = [
    _pk('r1_m3_pad1', 3, 5, 4, 1, 3, 1), _pk('r1_m80_pad8', 2, 3, 3, 1, 80, 8),
    _pk('r2_m3_pad8', 3, 4, 5, 2, 3, 8), _pk('r2_m80_pad1', 5, 8, 2, 2, 80, 1),
    _pk('r5_m3_pad1', 4, 6, 3, 5, 3, 1), _pk('r5_m80_pad8', 3, 4, 2, 5, 80, 8),
    _pk('grid_stride', 9, 10, 300, 5, 80, 8),       # 300 * 9 * 408 (pack) and 300 * 9 * 405 (unpack) elements > GRID_CAP
]
PACK_PRESENT = (('dmel', 'dstop'), ('dstop',), ('dmel',))       # both, dmel NULL, dstop NULL


def pack_ref(dmel, dstop, B, steps, r, n_mels, ld):
    """dY (steps, B, ld) in float32: [dmel(b, t r .. t r + r - 1, :) | sum_j dstop(b, t r + j) | zeros]; the r stop gradients are added
    in order j = 0 .. r - 1 starting from 0.0f, as float32 addition does here -- bit equality"""
    dY = torch.zeros(steps, B, ld)
    if dmel is not None:
        dY[:, :, :r * n_mels] = dmel.reshape(B, steps, r * n_mels).transpose(0, 1)
    if dstop is not None:
        s = torch.zeros(B, steps)
        for j in range(r):
            s = s + dstop.reshape(B, steps, r)[:, :, j]
        dY[:, :, r * n_mels] = s.t()
    return dY


def unpack_ref(Y, B, steps, r, n_mels):
    """Y (steps, >= B, ld) -> mel (B, steps r, n_mels), stop (B, steps r): a step's stop value repeated r times"""
    mel = Y[:, :B, :r * n_mels].transpose(0, 1).reshape(B, steps * r, n_mels)
    stop = Y[:, :B, r * n_mels].t()[:, :, None].expand(B, steps, r).reshape(B, steps * r)
    return mel.contiguous(), stop.contiguous()


# ===================================================================================================== dteacher sum
DTEACHER_CASES = [dict(S=S, steps=steps, Tt=5, Bt=3, Bp=5, P=7, XQw=12) for S in (1, 3) for steps in (1, 5, 3)]      # steps = 1 | Tt | < Tt
DTEACHER_CASES.append(dict(S=3, steps=4, Tt=4, Bt=17, Bp=32, P=40, XQw=48))


def dteacher_ref(part, S, Bt, Tt, P, steps, dtype):
    """part (steps + 1, S, Bp, XQw) -> dteacher (Bt, Tt, P): frame t = the first P columns of slot t + 1, slabs added in slab order from
    0; frames t >= steps - 1 zero.  dtype float32: the kernel's own sum, bit for bit; float64: the exact one"""
    out = torch.zeros(Bt, Tt, P, dtype=dtype)
    for t in range(min(Tt, steps - 1)):
        for s in range(S):
            out[:, t] = out[:, t] + part[t + 1, s, :Bt, :P].to(dtype)
    return out


# ===================================================================================================== AdaIN backward
ADAIN_STEPS = (1, 7, 8, 9, 17)        # either side of the unroll of 8
ADAIN_BQ = ((1, 4), (5, 100), (33, 256))
ADAIN_CASES = [dict(B=B, Q=Q, steps=s, da_ld=Q + 3, hq_ld=Q + 5, da_rows=B + 1, hq_rows=B + 2)
               for (B, Q), s in itertools.product(ADAIN_BQ, ADAIN_STEPS)]


def adain_ref(da, hq, std, mean):
    """da, hq (steps, B, Q): dstd = sum_t da (hq - mean), dmean = -std sum_t da, and their bounds: a chain of `steps` additions of terms
    that carry 2 roundings (hq - mean, the product) / none -> (steps + 2) u sum |terms|, one more product for dmean; times 2"""
    da, hq, std, mean = da.double(), hq.double(), std.double(), mean.double()
    steps = da.shape[0]
    dstd, dmean = (da * (hq - mean)).sum(0), -std * da.sum(0)
    t_dstd = 2 * (steps + 2) * U * (da * (hq - mean)).abs().sum(0)
    t_dmean = 2 * (steps + 1) * U * std.abs() * da.abs().sum(0)
    return dstd, dmean, t_dstd, t_dmean


# ===================================================================================================== scalars
SCALAR_CASES = [dict(n=n, m=m, nan=nan) for n in (1, ST_SCALAR_MAX) for m in (1, 4) for nan in (False, True)]
SCALE_BY_N = (1, 1000, GRID_CAP + 5)       # past 4096 * 256 + 3: a second grid stride with a ragged end


def scalar_weights(n, m, nan, seed):
    """W (m, n): row 0 all non-zero but for the NaN term (weight 0: the total is NaN all the same, as sum(w_i x_i) is in torch); rows
    j > 0 are sums over subsets (zero weight = not a member) that leave the NaN term out"""
    g = gen(seed)
    W = torch.rand(m, n, generator=g) + 0.25
    for j in range(1, m):
        W[j, torch.rand(n, generator=g) < 0.4] = 0.0
    if nan:
        W[:, n // 2] = 0.0
    return W


def scalar_combine_ref(W, x):
    """float64 out[j] = sum_i W[j, i] x_i over the members (row 0: every term; rows j > 0: the non-zero weights), and the bound: n
    products and n additions in a chain -> (n + 1) u sum |w x|, times 2"""
    W, x = W.double(), x.double()
    out, tol = [], []
    for j in range(W.shape[0]):
        member = torch.ones_like(W[j], dtype=torch.bool) if j == 0 else W[j] != 0
        t = W[j][member] * x[member]
        out.append(t.sum())
        tol.append(2 * (W.shape[1] + 1) * U * t.abs().sum())
    return torch.stack(out), torch.stack(tol)


# ===================================================================================================== unpacked skinny products
SK_B = (3, 16, 17, 32, 33, 70)
SK_N = (1, 16, 17, 33)
SK_H = (4, 8, 52)
SK_WAYS = ('k', 'ldx', 'ptr')       # vec = false through: k % 4 != 0 | ldx % 4 != 0 with k % 4 == 0 | an operand one float past 16 bytes
SK_KMAX = 1536                      # the largest K of test_skinny_linear (test_gpu_parity.py), whose 2e-5 holds for every K up to it
SK_TOL_LINEAR, SK_TOL_CELL = 2e-5, 1e-5      # test_skinny_linear (K <= 1536, inputs as sk_operands makes them) | test_lstm_cell


def sk_nb(B):
    """batch tiles per workgroup (sk_dispatch / sk_dispatch_pair in skinny.hip)"""
    return 1 if B <= 16 else 2 if B <= 32 else 4


def sk_seg(k, way=None):
    """one segment: k columns, row strides ldx / ldw and the operands' offsets in floats from a 16-byte boundary"""
    s = dict(k=k, ldx=k + 4, ldw=k + 8, xoff=0, woff=0)
    if way == 'k':
        assert k % 4 != 0
    elif way == 'ldx':
        assert k % 4 == 0
        s['ldx'] = k + 5
    elif way == 'ptr':
        assert k % 4 == 0
        s['xoff'], s['ldx'] = 1, k + 8
    else:
        assert way is None and k % 4 == 0
    return s


def sk_seg_vec(s):
    return s['xoff'] % 4 == 0 and s['woff'] % 4 == 0 and s['ldx'] % 4 == 0 and s['ldw'] % 4 == 0 and s['k'] % 4 == 0


def sk_vec(segs):
    """the 16-byte load path is taken when every segment's pointers are 16-byte aligned and ldx, ldw and k are multiples of 4 (the pair
    forms: over both jobs' one segment)"""
    return all(sk_seg_vec(s) for s in segs)


def sk_way(s):
    """which of SK_WAYS takes a segment off the 16-byte path (None: it is on it)"""
    if s['k'] % 4 != 0:
        return 'k'
    if s['ldx'] % 4 != 0:
        return 'ldx'
    if s['xoff'] % 4 != 0 or s['woff'] % 4 != 0:
        return 'ptr'
    return None


_SK_K = {None: (32, 64, 20), 'k': (30, 33, 21), 'ldx': (36, 64, 12), 'ptr': (40, 96, 8)}      # K of up to three segments per way


def _sk_single(key, sizes):
    """for every B: one case on the 16-byte path and one off it (the three ways in turn), nseg 1..3 and the sizes in turn"""
    out = []
    for i, B in enumerate(SK_B):
        for way in (None, SK_WAYS[i % 3]):
            nseg = 1 + (i + (way is not None)) % 3
            if way is None:
                segs = [sk_seg(k) for k in _SK_K[None][:nseg]]
            else:               # the last segment is the one off the path, the others are on it
                segs = [sk_seg(k) for k in _SK_K[None][:nseg - 1]] + [sk_seg(_SK_K[way][nseg - 1], way)]
            size = sizes[(i + (way is not None) * 2) % len(sizes)]
            out.append({'id': 'B%d_%s%d_seg%d_%s' % (B, key, size, nseg, way or 'vec'), 'B': B, key: size, 'segs': segs})
    return out


SK_LINEAR = _sk_single('N', SK_N)
SK_CELL = _sk_single('H', SK_H)


def _sk_pair(key, sizes):
    """for every B: both jobs aligned, and one job off the 16-byte path -- job 1 and job 0 in turn, through the three ways in turn (the two
    jobs always differ in K, inputs and weights).  opt: the cell's optional arrays present (b_hh2, pre2, c_prev2, gates_out2)"""
    out = []
    for i, B in enumerate(SK_B):
        for aligned in (True, False):
            way = SK_WAYS[i % 3]
            good, bad = sk_seg(64 + 4 * i), sk_seg({'k': 30, 'ldx': 36, 'ptr': 40}[way], way)
            if aligned:
                jobs = [sk_seg(64 + 4 * i), sk_seg(48)]
            else:
                jobs = [good, bad] if (i // 3) % 2 == 0 else [bad, good]
            size = sizes[(i + (not aligned) * 2) % len(sizes)]
            out.append({'id': 'B%d_%s%d_%s' % (B, key, size, 'vec' if aligned else way + '_job%d' % (0 if sk_way(jobs[0]) else 1)),
                        'B': B, key: size, 'jobs': jobs, 'opt': (i + aligned) % 2 == 0})
    return out


SK_LINEAR_PAIR = _sk_pair('N', SK_N)
SK_CELL_PAIR = _sk_pair('H', SK_H)


def sk_operands(B, rows, seg, seed):
    """x (B, k) ~ N(0, 1) and w (rows, k) ~ N(0, 1 / k), the distributions of test_skinny_linear / test_lstm_cell"""
    g = gen(seed)
    return torch.randn(B, seg['k'], generator=g), torch.randn(rows, seg['k'], generator=g) * seg['k'] ** -0.5


def sk_linear_ref(xs, ws, bias, act, mask):
    y = sum(x.double() @ w.double().t() for x, w in zip(xs, ws))
    if bias is not None:
        y = y + bias.double()
    if act == 'relu':
        y = torch.relu(y)
    return y * mask.double() if mask is not None else y


def sk_cell_ref(xs, ws, b_ih, b_hh, pre, c_prev, mask):
    """float64 nn.LSTMCell with torch.sigmoid / torch.tanh on gates = sum_s x_s W_s^T + b_ih + b_hh + pre, order (i, f, g, o)
    -> (h * mask, c, activated gates (B, 4, H))"""
    z = sum(x.double() @ w.double().t() for x, w in zip(xs, ws))
    for t in (b_ih, b_hh, pre):
        if t is not None:
            z = z + t.double()
    B, H = z.shape[0], z.shape[1] // 4
    z = z.view(B, 4, H)
    i, f, g, o = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])
    c = i * g + (f * c_prev.double() if c_prev is not None else 0.0)
    h = o * torch.tanh(c)
    if mask is not None:
        h = h * mask.double()
    return h, c, torch.stack([i, f, g, o], 1)
