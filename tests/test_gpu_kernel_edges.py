"""The small kernels every training step runs -- losses, row softmax / argmax, normalisations, gather / scatter, copies -- at the edge
shapes the configurations reach and on non-finite input, against plain float64 torch on the CPU.

Comparisons are elementwise (one wrong element among millions fails), tolerances are derived from each kernel's summation length
and stated next to the check; u = 2^-24 is the unit roundoff of float32.  Kernels that sum in a fixed order without atomics must give
bitwise-identical results on a second call.  Outputs with a leading dimension are written inside a larger buffer filled with a
sentinel whose guard columns and rows must stay bitwise unchanged.  Non-finite rules: an infeasible CTC alignment gives
loss inf and a NaN gradient for that utterance, an argmax over a NaN softmax row is 0, scatter keeps a non-finite gradient in the row
that owns it."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import SENTINEL, U, bits, gen, guard_ok, guarded, inside, report, same_bits   # noqa: E402,F401
from semi_tts_amd import _lib, ops   # noqa: E402
from semi_tts_amd import autograd as AG   # noqa: E402
from oracle import tts_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def rel_max(got, ref):
    """max |got - ref| / max |ref| over the elements (both finite there)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# ===================================================================================================== freq_loss
def _freq_ref(pred, label, n_low, w_all, w_low, w_diff, l1):
    """float64 restatement of src/util.py:80-126 with explicit weights (n_low = 0: no low-band term)"""
    p = pred.detach().cpu().double().requires_grad_()
    lab = label.detach().cpu().double()
    crit = F.l1_loss if l1 else F.mse_loss
    out = w_all * crit(p, lab)
    if n_low > 0 and w_low != 0.0:
        out = out + w_low * crit(p[..., :n_low], lab[..., :n_low])
    if w_diff != 0.0:
        out = out + w_diff * crit(p[:, 1:] - p[:, :-1], lab[:, 1:] - lab[:, :-1])
    out.backward()
    return float(out), p.grad


def _freq_inputs(B, T, D, seed, zeros=False):
    """pred, label on a 2^-10 grid in [-4, 4]: pred - label and its frame differences are exact in float32, so the sign of every L1
    term is the float64 sign (a rounded difference could flip sign(x) near 0).  zeros: exact zeros in pred - label (first channels)
    and in its frame differences (label = pred + a per-channel constant on the last channels)"""
    g = gen(seed)
    pred = torch.round(torch.rand(B, T, D, generator=g) * 8192 - 4096) / 1024
    label = torch.round(torch.rand(B, T, D, generator=g) * 8192 - 4096) / 1024
    if zeros:
        k = max(1, D // 4)
        label[..., :k] = pred[..., :k]
        label[..., -k:] = pred[..., -k:] + torch.round(torch.rand(1, 1, k, generator=g) * 64) / 1024
    return pred, label


def _freq_gpu(dev, pred, label, n_low, w_all, w_low, w_diff, l1, scale=1.0):
    pd = pred.to(dev).requires_grad_()
    loss = AG._FreqLossFn.apply(pd, label.to(dev), n_low, w_all, w_low, w_diff, l1)
    (loss * scale).backward()
    return float(loss.detach()), pd.grad


def _freq_tols(N):
    """loss: a thread adds its ceil(N / 262144) grid-stride terms in order, then 6 wave levels, 4 waves, 16 partials per lane of the
    final wave and 6 more levels; each term is c * val with up to 3 roundings -> |err| <= 4u (ceil(N / 262144) + 32) * loss (all terms
    >= 0).  gradient: the inputs are exact, so an element is at most 4 terms c_i * (+-1 or 2e), c_i = w / count rounded once, added in
    float32 and scaled by dloss: |err| <= 8u * sum |terms| <= 32u * max |grad| (a term never exceeds the largest gradient by 4x)"""
    return 4 * U * (math.ceil(N / 262144) + 32), 32 * U


@pytest.mark.parametrize('D,l1', [(1025, False), (1025, True), (80, False), (80, True)])
def test_freq_loss_at_config_size_against_oracle(dev, D, l1):
    """C2 batch (32 x 258 frames): the linear spectrogram takes the low-band term (n_low = 139 of 1025 at 22050 Hz), the mel the
    differential term -- about 33 grid strides of the kernel for the linear one, the (channel, frame) carry runs through all of them"""
    B, T, sr, n_mels = 32, 258, 22050, 80
    pred, label = _freq_inputs(B, T, D, seed=D + l1, zeros=l1)
    pd = pred.to(dev).requires_grad_()
    loss = AG.freq_loss(pd, label.to(dev), sr, n_mels, loss='l1' if l1 else 'mse')
    (loss * 1.5).backward()
    p64 = pred.double().requires_grad_()
    ref = O.freq_loss(p64, label.double(), sr, n_mels, loss='l1' if l1 else 'mse')
    (ref * 1.5).backward()
    tl, tg = _freq_tols(pred.numel())
    el = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    eg = rel_max(pd.grad, p64.grad)
    report('edge_freq_loss_config', D=D, l1=int(l1), err_loss=el, err_grad=eg, tol_loss=tl, tol_grad=tg)
    assert el <= tl and eg <= tg, (el, tl, eg, tg)


@pytest.mark.parametrize('B,T,D,n_low,w_diff,l1', [
    (32, 258, 1025, 139, 0.5, False),     # every term on at config size: the frame carry of the differential term over ~33 strides
    (400, 3, 997, 100, 0.5, False),       # prime D, T = 3: the frame index wraps inside every stride
    (400, 3, 997, 100, 0.5, True),
    (2, 2, 300000, 5000, 0.5, False),     # D > one stride (262144): a whole stride inside one row
    (2, 2, 300000, 5000, 0.5, True),
    (7, 2, 65, 65, 0.5, True),            # T = 2 with the differential term; n_low = D
    (5, 1, 513, 1, 0.0, False),           # T = 1 (differential term off); n_low = 1
    (5, 1, 513, 0, 0.0, True),            # n_low = 0: no low-band term whatever w_low says
    (3, 17, 80, 40, 0.5, True),           # L1 with exact zeros in e and in its frame differences
])
def test_freq_loss_strides_and_carries(dev, B, T, D, n_low, w_diff, l1):
    w_all, w_low = 0.5, 0.5
    pred, label = _freq_inputs(B, T, D, seed=B * 7 + T + D, zeros=l1)
    loss, grad = _freq_gpu(dev, pred, label, n_low, w_all, w_low, w_diff, l1, scale=0.75)
    ref, gref = _freq_ref(pred, label, n_low, w_all, w_low, w_diff, l1)
    gref = gref * 0.75
    tl, tg = _freq_tols(pred.numel())
    el, eg = abs(loss - ref) / abs(ref), rel_max(grad, gref)
    report('edge_freq_loss', B=B, T=T, D=D, n_low=n_low, l1=int(l1), err_loss=el, err_grad=eg, tol_loss=tl, tol_grad=tg)
    assert el <= tl and eg <= tg, (el, tl, eg, tg)
    if l1:     # sign(0) = 0 where torch's is: the exact zeros of e and of its differences give exactly the float64 gradient's zeros
        assert torch.equal(grad.cpu() == 0, gref == 0)


def test_freq_loss_is_bitwise_repeatable(dev):
    pred, label = _freq_inputs(4, 33, 1025, seed=5)
    a = _freq_gpu(dev, pred, label, 139, 0.5, 0.5, 0.5, False)
    b = _freq_gpu(dev, pred, label, 139, 0.5, 0.5, 0.5, False)
    assert a[0] == b[0] and same_bits(a[1], b[1])


# ===================================================================================================== CTC
def _ctc_ref(x, text, log_input):
    """torch.nn.CTCLoss() (blank 0, mean of nll / target length, zero_infinity=False) in float64, as bin/train_vqvae.py:430-444 calls
    it: log(prob + 1e-10) of posteriors, or log-probabilities as they are"""
    B, T, V = x.shape
    xr = x.double().requires_grad_()
    lp = xr if log_input else (xr + 1e-10).log()
    tl = (text != 0).sum(-1)
    loss = F.ctc_loss(lp.transpose(0, 1), text[text != 0], torch.full((B,), T, dtype=torch.long), tl, blank=0, reduction='mean',
                      zero_infinity=False)
    loss.backward()
    return float(loss.detach()), xr.grad


def _ctc_input(B, T, V, seed, log_input):
    lp = torch.log_softmax(torch.randn(B, T, V, generator=gen(seed)) * 1.5, dim=-1)
    return lp if log_input else lp.exp()


def _ctc_text(B, L, V, seed, n_tok=5):
    """few distinct labels (many adjacent repeats), a zero inside a row, a short row"""
    g = gen(seed)
    text = torch.randint(1, min(V, n_tok + 1), (B, L), generator=g)
    if L > 2:
        text[0, L // 2] = 0
    if B > 1:
        text[1, max(1, L // 3):] = 0
    return text


def _ctc_tols(T, x, log_input):
    """each frame's log-sum-exp adds a few ulps of |log alpha| <= T max|lp|: the nll is within 8u (T + 4) of itself in relative terms
    (normalised by max(1, |nll|) like the existing test); the occupancies exp(alpha + beta - lp + nll) turn that absolute log error into a
    relative one on every gradient element: 8u (T + 4) max(1, max|lp|) of the largest gradient"""
    lp = x if log_input else (x.double() + 1e-10).log()
    m = max(1.0, float(lp[torch.isfinite(lp)].abs().max()))
    return 8 * U * (T + 4), 8 * U * (T + 4) * m


def _ctc_check(dev, x, text, log_input, name):
    B, T, V = x.shape
    loss, grad = ops.ctc_loss(x.to(dev), text.to(dev), 1e-10, want_grad=True, log_input=log_input)
    ref, gref = _ctc_ref(x, text, log_input)
    tl, tg = _ctc_tols(T, x, log_input)
    el = abs(float(loss) - ref) / max(1.0, abs(ref))
    eg = rel_max(grad, gref)
    report('edge_ctc', case=name, B=B, T=T, V=V, L=text.shape[1], log_input=int(log_input), err_loss=el, err_grad=eg, tol_loss=tl,
           tol_grad=tg)
    assert math.isfinite(ref) and bool(torch.isfinite(grad).all())
    assert el <= tl and eg <= tg, (el, tl, eg, tg)
    return loss, grad


@pytest.mark.parametrize('log_input', [False, True])
@pytest.mark.parametrize('B,T,V,L,name', [
    (3, 1, 43, 3, 'T=1'),
    (3, 17, 43, 6, 'T=17'),            # T not a multiple of the 16-frame chunk
    (2, 33, 43, 10, 'T=33'),
    (2, 300, 43, 127, 'L=127'),        # 255 states: one thread short of the workgroup
    (65, 8, 20, 3, 'B=65'),            # the final mean walks two 64-utterance chunks
    (130, 8, 20, 3, 'B=130'),
    (2, 4, 10240, 2, 'V=10240'),       # the largest codebook the LDS class table takes
])
def test_ctc_edges_against_torch(dev, B, T, V, L, name, log_input):
    x = _ctc_input(B, T, V, seed=B + T + V + L, log_input=log_input)
    if T == 1:
        text = torch.tensor([[5, 0, 0], [0, 0, 0], [0, 7, 0]])          # S <= 1: the only lengths one frame can align
    else:
        text = _ctc_text(B, L, V, seed=L + T)
    if name == 'L=127':
        text[0] = torch.arange(L) % 3 + 1                               # no adjacent repeat: S = 127
        text[1] = 2                                                      # 126 adjacent repeats: T >= 253
    _ctc_check(dev, x, text, log_input, name)


def test_ctc_refuses_a_codebook_past_the_lds_cap(dev):
    x = _ctc_input(1, 4, 10241, seed=3, log_input=False).to(dev)
    with pytest.raises(RuntimeError, match='too large'):
        ops.ctc_loss(x, torch.tensor([[1, 2]], device=dev), 1e-10)


@pytest.mark.parametrize('log_input', [False, True])
def test_ctc_infeasible_utterance_gives_inf_loss_and_nan_gradient(dev, log_input):
    """T < S + adjacent repeats: no alignment, nll = inf.  torch (zero_infinity=False) returns loss inf and a NaN gradient for that
    utterance only; the other utterances' gradients stay finite and match"""
    B, T, V = 4, 6, 43
    x = _ctc_input(B, T, V, seed=11, log_input=log_input)
    text = torch.tensor([[3, 4, 0, 0, 0],        # feasible
                         [0, 0, 0, 0, 0],        # empty: all blank
                         [2, 2, 2, 2, 0],        # 4 tokens + 3 repeats = 7 frames > 6: infeasible
                         [5, 6, 7, 8, 9]])       # 5 frames: feasible
    loss, grad = ops.ctc_loss(x.to(dev), text.to(dev), 1e-10, want_grad=True, log_input=log_input)
    ref, gref = _ctc_ref(x, text, log_input)
    grad = grad.cpu()
    assert ref == INF and float(loss) == INF
    assert bool(torch.isnan(gref[2]).all()) and bool(torch.isnan(grad[2]).all())
    keep = [0, 1, 3]
    assert bool(torch.isfinite(gref[keep]).all()) and bool(torch.isfinite(grad[keep]).all())
    _, tg = _ctc_tols(T, x, log_input)
    eg = rel_max(grad[keep], gref[keep])
    report('edge_ctc_infeasible', log_input=int(log_input), err_grad=eg, tol_grad=tg)
    assert eg <= tg, (eg, tg)


def test_ctc_is_bitwise_repeatable(dev):
    x = _ctc_input(5, 40, 43, seed=2, log_input=False).to(dev)
    text = _ctc_text(5, 9, 43, seed=4).to(dev)
    a = ops.ctc_loss(x, text, 1e-10)
    b = ops.ctc_loss(x, text, 1e-10)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ===================================================================================================== softmax / argmax
def _logits(n, V, seed, special=True):
    """logits on a 1/64 grid (distinct values differ by >= 1/64, so float32 and float64 order them alike; equal values are exact ties)
    with -inf entries; special rows: an exact tie at the maximum, an all -inf row, a NaN, a +inf, a NaN after a -inf"""
    g = gen(seed)
    x = torch.round(torch.randn(n, V, generator=g) * 3 * 64) / 64
    x[torch.rand(n, V, generator=g) < 0.1] = -INF
    if special and n >= 5:
        if V >= 3:
            x[0, V // 3] = x[0, -1] = 40.0                          # exact tie: the first one wins
        x[1] = -INF
        x[2, V // 2] = NAN
        x[3, V - 1] = INF
        x[4, 0] = -INF
        x[4, V - 1] = NAN
    return x


def _softmax_check(p, idx, x):
    ref = torch.softmax(x.double(), -1)
    ridx = ref.argmax(-1)           # torch: the first maximum; the first NaN of a NaN row (every entry: index 0)
    p, idx = p.cpu().double(), idx.cpu()
    V = x.shape[-1]
    assert bool(((idx >= 0) & (idx < V)).all())
    assert torch.equal(idx, ridx)
    assert torch.equal(torch.isnan(p), torch.isnan(ref))
    fin = ~torch.isnan(ref)
    # p = exp(x - m) / s: the argument x - m is rounded (u |x - m|), expf adds ~2 ulp, the sum s of V terms over ceil(V / 64) steps
    # per lane and 6 wave levels carries (ceil(V / 64) + 6) u, the division one more: per element relative
    # (ceil(V / 64) + 10 + max |x - m|) u, with an absolute floor for exponentials that underflow float32
    xf = x.double()
    m = torch.where(torch.isfinite(xf), xf, torch.full_like(xf, -1e300)).max(-1, keepdim=True).values
    spread = float(((xf - m)[torch.isfinite(xf)]).abs().max()) if bool(torch.isfinite(xf).any()) else 0.0
    tol = (math.ceil(V / 64) + 10 + spread) * U
    err = ((p - ref).abs() - tol * ref)[fin]
    worst = float(((p - ref).abs() / ref.clamp_min(1e-37))[fin].max()) if bool(fin.any()) else 0.0
    assert bool((err <= 1e-37).all()), (worst, tol)
    return worst, tol


@pytest.mark.parametrize('n,V', [(5, 1), (5, 43), (5, 63), (5, 64), (5, 65), (5, 512), (5, 4096), (1, 4096), (1, 1), (8193, 43),
                                 (8256, 43), (8256, 64), (16385, 65)])
def test_softmax_argmax_edges(dev, n, V):
    """st_softmax_argmax (the 'seperate' codebook, src/embed.py:190-193): the grid caps at 2048 x 4 rows, so 8193 / 8256 (a C2 batch of
    32 x 258 frames) / 16385 rows run the row grid-stride loop"""
    x = _logits(n, V, seed=n + V)
    p, idx = ops.softmax_argmax(x.to(dev))
    worst, tol = _softmax_check(p, idx, x)
    report('edge_softmax_argmax', n=n, V=V, err=worst, tol=tol)
    p2, idx2 = ops.softmax_argmax(x.to(dev))
    assert same_bits(p, p2) and torch.equal(idx, idx2)


def _softmax_bwd_ref(p, dp, s):
    p, dp = p.double(), dp.double()
    dot = (dp * p).sum(-1, keepdim=True)
    dz = s * p * (dp - dot)
    # dot: ceil(V / 64) fma steps per lane + 6 wave levels -> (ceil(V / 64) + 6) u sum |dp p|; dp - dot, the two products and the scale
    # add 4 roundings: per element |err| <= s p ((ceil(V / 64) + 10) u (sum |dp p| + |dp| + |dot|))
    k = math.ceil(p.shape[-1] / 64) + 10
    tol = abs(s) * p * k * U * ((dp * p).abs().sum(-1, keepdim=True) + dp.abs() + dot.abs())
    return dz, tol


@pytest.mark.parametrize('n,V', [(5, 1), (5, 43), (5, 64), (5, 65), (5, 4096), (16385, 43), (8256, 512)])
def test_softmax_bwd_edges(dev, n, V):
    """st_softmax_bwd with and without the row sums; its grid caps at 4096 x 4 = 16384 rows"""
    x = _logits(n, V, seed=3 * n + V, special=False)
    x[torch.isinf(x).all(-1), 0] = 0.0
    p = torch.softmax(x, -1)
    dp = torch.randn(n, V, generator=gen(n * V))
    ref, tol = _softmax_bwd_ref(p, dp, float(torch.tensor(0.7)) * float(torch.tensor(1.3)))      # the float32 scale and temperature
    temp = torch.tensor([1.3], device=dev)
    dz, rs = ops.softmax_bwd(p.to(dev), dp.to(dev), 0.7, temp, want_rowsum=True)
    dz = dz.cpu().double()
    assert bool(((dz - ref).abs() <= tol + 1e-37).all()), float(((dz - ref).abs() - tol).max())
    # row sum of dz: its own (ceil(V / 64) + 6) u sum |dz| plus the elements' errors
    rtol = tol.sum(-1) + (math.ceil(V / 64) + 6) * U * ref.abs().sum(-1)
    assert bool(((rs.cpu().double() - ref.sum(-1)).abs() <= rtol + 1e-37).all())
    dz1 = ops.softmax_bwd(p.to(dev), dp.to(dev), 0.7 * 1.3)
    assert bool(((dz1.cpu().double() - ref).abs() <= tol + 1e-37).all())
    report('edge_softmax_bwd', n=n, V=V, err=rel_max(dz, ref))
    # a negative temperature: relu(temp) = 0, the gradient is exactly zero
    dz0, rs0 = ops.softmax_bwd(p.to(dev), dp.to(dev), 0.7, torch.tensor([-0.5], device=dev), want_rowsum=True)
    assert bool((dz0 == 0).all()) and bool((rs0 == 0).all())


# ===================================================================================================== VQ L2 search, non-finite rows
def _vq_ref(x, table, temp):
    """L2Embedding.forward in float64 in the reference's association order (src/embed.py:210-212): (|x|^2 + |e|^2) - 2 x e^T"""
    x, e = x.double(), table.double()
    dist = (x.pow(2).sum(-1, keepdim=True) + e.pow(2).sum(-1)) - 2 * x @ e.t()
    p = torch.softmax(torch.relu(temp.double()) * -dist, -1)
    return p, p.argmax(-1)


def _vq_run(dev, x, table, temp, path):
    xd, td, tp = x.to(dev), table.to(dev), temp.to(dev)
    if path == 'packed':
        return ops.vq_l2(xd, td, tp, packed=ops.vq_pack_table(td))
    return ops.vq_l2(xd, td, tp, scalar_kernel=(path == 'lds'))


VQ_PATHS = [(43, 64, 'mfma'), (512, 64, 'mfma'), (512, 64, 'packed'), (43, 70, 'mfma'), (43, 64, 'lds'), (512, 20, 'lds')]


@pytest.mark.parametrize('V,D,path', VQ_PATHS)
def test_vq_l2_non_finite_rows(dev, V, D, path):
    """NaN and +-inf in rows of x: torch's softmax row is NaN, its argmax 0 (the first NaN).  The index stays inside [0, V) -- it
    addresses the code table -- and the finite rows come out bitwise as in a run without the bad rows.  (D = 70 is not a matrix-core
    shape: the LDS kernel serves it)"""
    if path == 'mfma' and D == 64:
        assert ops.vq_mfma_shape(D, V)
    g = gen(V + D)
    n = 100                                          # a partial last tile of 16 vectors
    x = torch.randn(n, D, generator=g)
    table = torch.randn(V, D, generator=g)
    temp = torch.tensor([1.5])
    bad = x.clone()
    bad[3, D // 2] = NAN
    bad[10, 0] = INF
    bad[11, D - 1] = -INF
    bad[50] = NAN
    bad[99, 1] = INF
    bad_rows = [3, 10, 11, 50, 99]
    p, idx, out = _vq_run(dev, bad, table, temp, path)
    pc, idxc, outc = _vq_run(dev, x, table, temp, path)
    pref, iref = _vq_ref(bad, table, temp)
    p, idx = p.cpu(), idx.cpu()
    assert bool(((idx >= 0) & (idx < V)).all())
    assert torch.equal(idx, iref)
    assert torch.equal(torch.isnan(p), torch.isnan(pref))
    assert bool(torch.isnan(pref[bad_rows]).all())
    good = [r for r in range(n) if r not in bad_rows]
    assert torch.equal(idx[good], idxc.cpu()[good])
    assert same_bits(p[good], pc[good]) and same_bits(out[good], outc[good])
    # every code row of a NaN-free table is finite: the straight-through value of a bad row is (x + table[0]) - x
    assert bool(torch.isfinite(outc).all())


@pytest.mark.parametrize('V,D,path', VQ_PATHS)
def test_vq_l2_nan_code_row_or_nan_temperature(dev, V, D, path):
    """one NaN code row (its similarity is NaN in every row) or a NaN temperature (relu(NaN) = NaN): every softmax row is NaN and every
    index is 0, as torch gives"""
    g = gen(V * D)
    x = torch.randn(37, D, generator=g)
    table = torch.randn(V, D, generator=g)
    tbad = table.clone()
    tbad[V // 2, 1] = NAN
    for tab, temp in ((tbad, torch.tensor([1.5])), (table, torch.tensor([NAN]))):
        p, idx, _ = _vq_run(dev, x, tab, temp, path)
        pref, iref = _vq_ref(x, tab, temp)
        assert bool(torch.isnan(pref).all()) and bool((iref == 0).all())
        assert bool(torch.isnan(p).all()) and bool((idx == 0).all())


def test_vq_l2_autograd_entry_with_a_nan_row(dev):
    """the autograd entry L2Embedding uses: the index of a NaN row is 0, the others are those of the ops call"""
    g = gen(9)
    x = torch.randn(40, 64, generator=g)
    x[7, 5] = NAN
    table = torch.randn(43, 64, generator=g)
    temp = torch.tensor([1.0])
    p, out, idx = AG.vq_l2(x.to(dev), table.to(dev), temp.to(dev))
    p2, idx2, _ = ops.vq_l2(x.to(dev), table.to(dev), temp.to(dev))
    assert int(idx[7]) == 0 and torch.equal(idx, idx2) and same_bits(p, p2)


# ===================================================================================================== layer_norm
def _ln_rows(M, N, seed):
    x = torch.randn(M, N, generator=gen(seed))
    if M >= 2:
        x[0] = 0.3                                   # constant row: variance 0
        x[1] = 1e4 + torch.randn(N, generator=gen(seed + 1))     # a one-pass E[x^2] - E[x]^2 loses all 24 bits here
    return x


def _lnf(dev, x, gamma, beta, eps, ldx, ldy):
    """st_layer_norm_fwd on strided input and output inside guard buffers -> (y view, y buffer, mean, rstd)"""
    M, N = x.shape
    xb, xv = guarded(M, N, ldx, dev)
    xv.copy_(x.to(dev))
    yb, yv = guarded(M, N, ldy, dev)
    mean = torch.empty(M, device=dev)
    rstd = torch.empty(M, device=dev)
    lib = _lib.load()
    _lib.check(lib.st_layer_norm_fwd(ops._p(xv), ldx, ops._p(gamma), ops._p(beta), float(eps), ops._p(yv), ldy, ops._p(mean),
                                     ops._p(rstd), M, N, ops.stream_handle()), 'st_layer_norm_fwd')
    assert guard_ok(xb, inside(M, N))
    return yv, yb, xv, mean, rstd


@pytest.mark.parametrize('N', [1, 63, 64, 65, 1024, 1025, 2500])
def test_layer_norm_forward_and_backward(dev, N):
    """nn.LayerNorm over the last dimension (src/asr.py:38-39,58): rows kept in registers up to 1024 columns, re-read beyond; every M
    from a single row to a partial last workgroup; gamma / beta None and set; strided operands with guard bands"""
    eps = 1e-5
    for M in (1, 3, 4, 5, 1000):
        for affine in (False, True):
            x = _ln_rows(M, N, seed=M * 31 + N)
            g = gen(M + N + affine)
            gamma = (torch.rand(N, generator=g) + 0.5) if affine else None
            beta = torch.randn(N, generator=g) if affine else None
            gd = gamma.to(dev) if affine else None
            bd = beta.to(dev) if affine else None
            ldx, ldy = N + 7, N + 5
            y, yb, xv, mean, rstd = _lnf(dev, x, gd, bd, eps, ldx, ldy)
            assert guard_ok(yb, inside(M, N))
            x64 = x.double().requires_grad_()
            yr = F.layer_norm(x64, (N,), gamma.double() if affine else None, beta.double() if affine else None, eps)
            mu = x.double().mean(-1, keepdim=True)
            rs = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + eps)
            xh = (x.double() - mu) * rs
            # mean: ceil(N / 64) adds per lane + 6 wave levels -> |d mean| <= k u max|x|, k = ceil(N / 64) + 8 (with the division);
            # xhat inherits d mean * rstd and the rstd error k u |xhat|; gamma, beta and the fma add 3u |y|
            k = math.ceil(N / 64) + 8
            gm = gamma.double().abs() if affine else torch.ones(N, dtype=torch.float64)
            dxh = k * U * (x.double().abs().max(-1, keepdim=True).values * rs + xh.abs())
            tol = 2 * (gm * dxh + 3 * U * yr.detach().abs())
            err = (y.cpu().double() - yr.detach()).abs()
            assert bool((err <= tol + 1e-30).all()), (M, affine, float((err - tol).max()))
            assert bool(torch.isfinite(y).all())
            # backward, strided dy / x / dx with guards; d gamma's input dy * xhat comes back contiguous
            dy = torch.randn(M, N, generator=g)
            yr.backward(dy.double())
            dyb, dyv = guarded(M, N, N + 3, dev)
            dyv.copy_(dy.to(dev))
            dxb, dxv = guarded(M, N, N + 9, dev)
            dyxhat = torch.empty(M, N, device=dev)
            lib = _lib.load()
            _lib.check(lib.st_layer_norm_bwd(ops._p(dyv), N + 3, ops._p(xv), ldx, ops._p(gd), ops._p(mean), ops._p(rstd), ops._p(dxv),
                                             N + 9, ops._p(dyxhat), M, N, ops.stream_handle()), 'st_layer_norm_bwd')
            assert guard_ok(dxb, inside(M, N)) and guard_ok(dyb, inside(M, N))
            gg = dy.double() * gm
            s1 = gg.mean(-1, keepdim=True)
            s2 = (gg * xh).mean(-1, keepdim=True)
            # dx = rstd (g - mean g - xhat mean(g xhat)): the two means carry k u of sum |.| / N, the xhat error dxh enters through
            # xhat s2 and through s2 itself (<= max|g| dxh)
            ax = gg.abs().max(-1, keepdim=True).values
            tdx = 4 * rs * (k * U * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
                            + dxh * s2.abs() + xh.abs() * ax * dxh.max(-1, keepdim=True).values + 2 * U * (gg - s1 - xh * s2).abs())
            edx = (dxv.cpu().double() - x64.grad).abs()
            assert bool((edx <= tdx + 1e-30).all()), (M, affine, float((edx - tdx).max()))
            edy = (dyxhat.cpu().double() - dy.double() * xh).abs()
            assert bool((edy <= dy.double().abs() * (dxh + 2 * U * xh.abs()) * 2 + 1e-30).all())
    report('edge_layer_norm', N=N)


# ===================================================================================================== log_softmax
@pytest.mark.parametrize('N', [1, 43, 512, 5000])
def test_log_softmax_forward_and_backward(dev, N):
    """ASRPostnet's output (src/asr.py:80): logits up to +-80, -inf entries and an all -inf row (NaN in torch and here)"""
    M = 7
    g = gen(N)
    x = (torch.rand(M, N, generator=g) * 160 - 80)
    x[0, 0] = 80.0
    x[0, -1] = -80.0
    x[2][torch.rand(N, generator=g) < 0.3] = -INF
    if N > 1:
        x[2, 0] = 1.0
    x[3] = -INF
    y = ops.log_softmax(x.to(dev)).cpu().double()
    ref = torch.log_softmax(x.double(), -1)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isinf(y), torch.isinf(ref))
    fin = torch.isfinite(ref)
    # y = x - (m + log s): s sums N terms over ceil(N / 64) steps per lane + 6 levels -> (ceil(N / 64) + 6) u relative, log adds
    # 2 ulp; x - lse rounds once: |err| <= 2u (|x| + |lse|) + (ceil(N / 64) + 10) u
    lse = (x.double() - ref)
    tol = 2 * U * (x.double().abs() + lse.abs()) + (math.ceil(N / 64) + 10) * U
    assert bool(((y - ref).abs() <= tol)[fin].all())
    # backward on the finite rows: dx = dy - exp(y) sum dy; the sum carries (ceil(N / 64) + 6) u sum |dy|, exp(y) ~ (|y| + 2) u relative
    rows = [r for r in range(M) if r != 3]
    yf = ref[rows].float()
    dy = torch.randn(len(rows), N, generator=g)
    dx = ops.log_softmax_bwd(dy.to(dev), yf.to(dev)).cpu().double()
    y64 = yf.double()
    s = dy.double().sum(-1, keepdim=True)
    dref = dy.double() - y64.exp() * s
    k = math.ceil(N / 64) + 6
    tol = 2 * U * dref.abs() + y64.exp() * (k * U * dy.double().abs().sum(-1, keepdim=True) + s.abs() * (y64.clamp_min(-1e4).abs() + 4) * U)
    assert bool(((dx - dref).abs() <= tol + 1e-30).all())
    assert bool((dx[y64 == -INF] == dy.double()[y64 == -INF]).all())       # exp(-inf) = 0: dx = dy exactly
    report('edge_log_softmax', N=N, err_fwd=rel_max(y[fin], ref[fin]), err_bwd=rel_max(dx, dref))


# ===================================================================================================== scatter_add_rows / gather_rows
@pytest.mark.parametrize('n', [1, 7, 8, 9, 8256])
@pytest.mark.parametrize('D', [1, 63, 64, 65, 256])
def test_scatter_add_rows_against_embedding_backward(dev, n, D):
    """dtable = F.embedding's backward: many repeats, rows nobody picks stay exactly 0; a fixed-order sum, bitwise repeatable"""
    V = 43
    g = gen(n * 1000 + D)
    idx = torch.randint(0, 20, (n,), generator=g) * 2            # even codes below 40 only: odd ones and 40, 41, 42 are never picked
    dout = torch.randn(n, D, generator=g)
    dt = ops.scatter_add_rows(dout.to(dev), idx.to(dev), V)
    tab = torch.zeros(V, D, dtype=torch.float64, requires_grad=True)
    F.embedding(idx, tab).backward(dout.double())
    ref = tab.grad
    # a row's sum runs over 8 lane slices of ceil(n / 8) rows, then the 8 partials: |err| <= (ceil(n / 8) + 8) u sum |dout|
    aref = torch.zeros(V, D, dtype=torch.float64).index_add_(0, idx, dout.double().abs())
    tol = (math.ceil(n / 8) + 8) * U * aref
    assert bool(((dt.cpu().double() - ref).abs() <= tol).all())
    unpicked = torch.ones(V, dtype=torch.bool)
    unpicked[idx] = False
    assert bool((dt.cpu()[unpicked] == 0).all())
    assert same_bits(dt, ops.scatter_add_rows(dout.to(dev), idx.to(dev), V))


def test_scatter_add_rows_keeps_non_finite_gradients_in_their_rows(dev):
    """one inf and one NaN in dout: torch's embedding backward makes only the owning rows' columns non-finite; a 0 / 1 factor would make
    0 * inf = NaN in that column of every row"""
    V, n, D = 43, 300, 65
    g = gen(17)
    idx = torch.randint(0, V, (n,), generator=g)
    dout = torch.randn(n, D, generator=g)
    dout[5, 7] = INF
    dout[200, 64] = NAN
    dt = ops.scatter_add_rows(dout.to(dev), idx.to(dev), V).cpu()
    tab = torch.zeros(V, D, dtype=torch.float64, requires_grad=True)
    F.embedding(idx, tab).backward(dout.double())
    ref = tab.grad
    assert torch.equal(torch.isnan(dt), torch.isnan(ref)) and torch.equal(torch.isinf(dt), torch.isinf(ref))
    assert int((~torch.isfinite(ref)).sum()) == 2
    fin = torch.isfinite(ref)
    aref = torch.zeros(V, D, dtype=torch.float64).index_add_(0, idx, dout.double().abs().nan_to_num(0, 0, 0))
    assert bool(((dt.double() - ref).abs() <= (math.ceil(n / 8) + 8) * U * aref)[fin].all())


def test_gather_rows_clamps_out_of_range_indices(dev):
    """st_gather_rows clamps an index to [0, V - 1] (torch would raise): pinned as a deliberate difference"""
    V, D = 43, 65
    table = torch.randn(V, D, generator=gen(1))
    idx = torch.tensor([[0, 5, V - 1, -3], [V, V + 10, 7, -1]])
    out = ops.gather_rows(table.to(dev), idx.to(dev)).cpu()
    assert out.shape == (2, 4, D)
    assert same_bits(out, table[idx.clamp(0, V - 1)])


# ===================================================================================================== copies, means, combines
@pytest.mark.parametrize('Bn,T,Cc', [(1, 1, 1), (3, 7, 65), (5, 301, 700)])
@pytest.mark.parametrize('accumulate', [False, True])
def test_copy3d_strided_with_guards(dev, Bn, T, Cc, accumulate):
    """dst(b, t, :Cc) (+)= src(b, t, :Cc) over arbitrary strides: float32 adds are exact restatements, so bitwise; nothing outside the
    destination view changes (the largest case crosses the 4096-block grid cap)"""
    g = gen(Bn * T + Cc)
    big = torch.full((Bn, T + 2, Cc + 9), SENTINEL)
    big[:, 1:T + 1, 4:4 + Cc] = torch.randn(Bn, T, Cc, generator=g)
    dstb = big.to(dev)
    dst = dstb[:, 1:T + 1, 4:4 + Cc]
    srcb = torch.randn(Bn, 2 * T, Cc + 5, generator=g).to(dev)
    src = srcb[:, ::2, 2:2 + Cc]
    want = (dst + src) if accumulate else src.clone()
    ops.copy3d(dst, src, Bn, T, Cc, accumulate=accumulate)
    assert same_bits(dst, want)
    out = dstb.cpu()
    keep = torch.zeros(out.shape, dtype=torch.bool)
    keep[:, 1:T + 1, 4:4 + Cc] = True
    assert bool((out[~keep] == SENTINEL).all())


@pytest.mark.parametrize('rows,cols', [(1, 1), (37, 65), (3000, 300)])
def test_copy2d_strided_with_guards(dev, rows, cols):
    src_b, src = guarded(rows, cols, cols + 11, dev)
    src.copy_(torch.randn(rows, cols, generator=gen(rows + cols)).to(dev))
    dstb, dst = guarded(rows, cols, cols + 6, dev, off=2)
    ops.copy2d(dst, src, rows, cols)
    assert same_bits(dst, src)
    assert guard_ok(dstb, inside(rows, cols, off=2)) and guard_ok(src_b, inside(rows, cols))


@pytest.mark.parametrize('B,T,D', [(2, 1, 5), (3, 257, 65), (64, 3, 8500)])
def test_mean_rows(dev, B, T, D):
    """mean over T: a sequential float32 sum of T terms and one division -> |err| <= (T + 1) u sum_t |x| / T"""
    x = torch.randn(B, T, D, generator=gen(B + T + D)) + 2.0
    got = ops.mean_rows(x.to(dev)).cpu().double()
    ref = x.double().mean(1)
    tol = (T + 1) * U * x.double().abs().mean(1)
    assert bool(((got - ref).abs() <= tol).all())


@pytest.mark.parametrize('M,D', [(1, 1), (37, 65), (1100, 1000)])
def test_rowscale_combine(dev, M, D):
    """alpha a + beta r[m] x (+ c): alpha a, beta r, the fma and the + c round once each -> |err| <= 4u (|alpha a| + |beta r x| + |c|)"""
    g = gen(M + D)
    a, x, c = (torch.randn(M, D, generator=g) for _ in range(3))
    r = torch.randn(M, generator=g)
    alpha, beta = 2.0, -2.0
    for with_x, with_c in ((True, True), (True, False), (False, True), (False, False)):
        got = ops.rowscale_combine(a.to(dev), alpha, x.to(dev) if with_x else None, r.to(dev) if with_x else None, beta,
                                   c.to(dev) if with_c else None).cpu().double()
        ref = alpha * a.double()
        mag = ref.abs()
        if with_x:
            t = beta * r.double()[:, None] * x.double()
            ref, mag = ref + t, mag + t.abs()
        if with_c:
            ref, mag = ref + c.double(), mag + c.double().abs()
        assert bool(((got - ref).abs() <= 4 * U * mag).all()), (with_x, with_c)


# ===================================================================================================== trainer level
def test_paired_step_with_an_infeasible_transcript_skips_the_update(dev):
    """A paired step whose batch holds one transcript too long for its frames: the CTC loss is inf and its gradient NaN, so the gradient
    norm is non-finite and BaseSolver.backward's `if math.isnan(grad_norm)` skip (src/solver.py:145-147) leaves every parameter bitwise
    unchanged"""
    from argparse import Namespace
    from conftest import load_golden
    from helpers import tiny_vqvae
    from semi_tts_amd.optim import Optimizer
    from semi_tts_amd.solver import VqvaeTrainer
    W, A, meta = load_golden('text_first_unpaired')
    h = meta['hparas']
    config = dict(data=dict(audio=meta['audio'], corpus=dict(batch_size=3)), hparas=h, model=meta['model'])
    tr = VqvaeTrainer(config, Namespace(vocab_size=meta['vocab_size'], n_spkr=meta['n_spkr'], verbose=False, max_step=1), 'train')
    tr.model = tiny_vqvae(meta, W, dev, strict=True).train()
    tr.optimizer = Optimizer(tr.model.parameters(), h['optimizer'], h['lr'], h['lr_scheduler'], tf_start=h['tf_start'],
                             tf_end=h['tf_end'], tf_step=h['tf_step'])
    text, sid, mel, linear = (A[k].to(dev) for k in ('text', 'sid', 'mel', 'linear'))
    L = 30                                   # 30 equal tokens need 59 frames: more than the mel's 24 frames give the speech encoder
    wide = torch.zeros(text.shape[0], L, dtype=text.dtype, device=dev)
    wide[:, :text.shape[1]] = text
    wide[0] = 7
    before = {k: p.detach().clone() for k, p in tr.model.named_parameters()}
    st = tr.text_first_step(mel, mel, linear, wide, sid)
    report('edge_infeasible_step', asr_loss=st['asr_loss'], grad_norm=st['grad_norm'])
    assert st['asr_loss'] == INF
    assert not math.isfinite(st['grad_norm'])
    for k, p in tr.model.named_parameters():
        assert same_bits(p, before[k]), k
