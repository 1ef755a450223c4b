"""Case tables, float64 references and rounding bounds for the multi-tensor optimiser kernels (optim.hip: gradient norm, clip scale,
Adam, multi-tensor copy).  No GPU and no library here: test_optim_host.py checks the tables and references on the CPU (and the restated
splitting rule against st_mt_launch_plan), test_gpu_optim.py runs the kernels against them."""
import math

import numpy as np
import torch

from helpers import U          # float32 unit roundoff, 2^-24

MT_T, MT_NB, MT_CHUNK, MT_THREADS = 24, 640, 32768, 256      # optim.hip: tensor slots / blocks per launch, floats per block
MC_T, MC_NB, MC_CHUNK = 96, 512, 4096                        # st_mt_copy
MT_TABS = 16                                                 # entries of the device-side table cache
LIMITS = {0: (MT_T, MT_NB, MT_CHUNK, 65535 * MT_CHUNK), 1: (MC_T, MC_NB, MC_CHUNK, 65535 * MC_CHUNK - 1)}

# ------------------------------------------------------------------------------------------------ sizes and alignments
# every size exists for an edge of mt_body: the n % 4 tail, the loop rounds of the norm (1 piece = 4 floats per thread: 1024 floats per
# round of 256 threads; 2 pieces: 2048; 8 pieces: 8192) and of Adam (1 piece: 1024; 4 pieces: 4096), and the 32768-float chunk
SIZE_ROWS = [
    (1, 'one_element_tail_only'), (2, 'tail_2'), (3, 'tail_3'), (4, 'one_piece_no_tail'), (5, 'one_piece_tail_1'),
    (1023, 'below_1_piece_round'), (1024, 'exactly_1_piece_round'), (1025, 'above_1_piece_round'),
    (2047, 'below_norm_2_piece_round'), (2048, 'exactly_norm_2_piece_round'), (2049, 'above_norm_2_piece_round'),
    (4095, 'below_adam_4_piece_round'), (4096, 'exactly_adam_4_piece_round'), (4097, 'above_adam_4_piece_round'),
    (8191, 'below_norm_8_piece_round'), (8192, 'exactly_norm_8_piece_round'), (8193, 'above_norm_8_piece_round'),
    (32767, 'below_one_chunk'), (32768, 'exactly_one_chunk'), (32769, 'one_chunk_and_one_element'),
    (65535, 'below_two_chunks'), (65536, 'exactly_two_chunks'), (65537, 'two_chunks_and_one_element'),
    (3 * 32768 + 5, 'three_chunks_and_a_ragged_fourth'),
]
SIZES = [n for n, _ in SIZE_ROWS]
# norm only: sizes at which EVERY thread of a block runs an eight-piece round, then a two-piece round, then a single piece, with an
# n % 4 tail (the table above sends at most one thread of a block through a mixed sequence: each size sits at ONE round's edge)
NORM_EXTRA_ROWS = [
    (8192 + 2048 + 1024 + 3, 'every_thread_8_then_2_then_1_piece_rounds_tail_3'),
    (32768 + 8192 + 2048 + 1, 'full_chunk_then_every_thread_8_then_2_piece_rounds_tail_1'),
    (8192 + 1024 + 2, 'every_thread_8_then_1_piece_rounds_tail_2'),
    (2048 + 1024, 'every_thread_2_then_1_piece_rounds'),
]
NORM_SIZES = SIZES + [n for n, _ in NORM_EXTRA_ROWS]
OFFSETS = (0, 1, 2, 3)           # floats past a 16-byte boundary: 0 takes the 16-byte loops, the others the float-by-float ones

# ------------------------------------------------------------------------------------------------ launch splits (kernel-argument form)
_SMALL = [7, 165, 1, 1025, 33, 4096, 5, 2049]


def _small(k):
    return [_SMALL[i % len(_SMALL)] + i for i in range(k)]


# want: the launches [(tensor slots, blocks)] of the kernel-argument form; reach: what the row is there for
SPLIT_ROWS = [
    dict(id='24_tensors_fill_one_launch', sizes=_small(24), want=[(24, 24)], reach='single'),
    dict(id='25_tensors_spill_one', sizes=_small(25), want=[(24, 24), (1, 1)], reach='tensors'),
    dict(id='48_tensors_fill_two_launches', sizes=_small(48), want=[(24, 24), (24, 24)], reach='tensors'),
    dict(id='49_tensors_spill_one_twice', sizes=_small(49), want=[(24, 24), (24, 24), (1, 1)], reach='tensors'),
    dict(id='640_chunks_fill_one_launch', sizes=[MT_NB * MT_CHUNK], want=[(1, 640)], reach='single', big=True),
    dict(id='640_chunks_and_one_element_cut', sizes=[MT_NB * MT_CHUNK + 1], want=[(1, 640), (1, 1)], reach='cut', big=True),
    dict(id='23_one_chunk_then_700_chunks_reregistered_at_slot_0', sizes=[3 + i for i in range(23)] + [700 * MT_CHUNK],
         want=[(24, 640), (1, 83)], reach='cut', big=True),
]
COPY_SPLIT_ROWS = [
    dict(id='copy_4095', sizes=[4095], want=[(1, 1)]), dict(id='copy_4096', sizes=[4096], want=[(1, 1)]),
    dict(id='copy_512_chunks_fill_one_launch', sizes=[MC_NB * MC_CHUNK], want=[(1, 512)]),
    dict(id='copy_512_chunks_and_one_element_cut', sizes=[MC_NB * MC_CHUNK + 1], want=[(1, 512), (1, 1)]),
    dict(id='copy_96_tensors_fill_one_launch', sizes=[17 + i for i in range(96)], want=[(96, 96)]),
    dict(id='copy_97_tensors_spill_one', sizes=[17 + i for i in range(97)], want=[(96, 96), (1, 1)]),
]


def blocks(sizes, chunk=MT_CHUNK):
    """st_mt_blocks"""
    return sum(-(-n // chunk) for n in sizes if n > 0)


def plan(sizes, kind=0):
    """mt_split (optim.hip) restated: the launches [(tensor slots, blocks)] the kernel-argument form makes for a size list -- tensors in
    list order, empty ones skipped; a launch closes when its slots or its blocks are used up, and a tensor with chunks left takes the
    next launch's next free slot.  None: refused (a tensor whose chunk index would not fit 16 bits).  kind 1: st_mt_copy's limits."""
    T, NB, chunk, n_max = LIMITS[kind]
    if any(n > n_max for n in sizes):
        return None
    out, ti, bl = [], 0, 0
    for n in sizes:
        if n <= 0:
            continue
        left = -(-n // chunk)
        while left:
            if ti == T or bl == NB:
                out.append((ti, bl))
                ti = bl = 0
            take = min(left, NB - bl)
            bl, left, ti = bl + take, left - take, ti + 1
    if bl:
        out.append((ti, bl))
    return out


def reaches(launches, sizes, kind=0):
    """the split cases a plan contains: 'single', 'tensors' (a launch closed because its slots ran out), 'blocks' (... its blocks),
    'cut' (one tensor's chunks in two launches)"""
    T, NB, chunk, _ = LIMITS[kind]
    out = set()
    if len(launches) == 1:
        out.add('single')
    for t, b in launches[:-1]:
        if t == T:
            out.add('tensors')
        if b == NB:
            out.add('blocks')
    if sum(t for t, _ in launches) > sum(1 for n in sizes if n > 0):
        out.add('cut')
    return out


class TableLru:
    """mt_table's cache as a model: MT_TABS entries, a hit on the same key (pass kind, list, stream) refreshes it, a miss replaces the
    least recently used entry.  use(key) -> True for a miss."""

    def __init__(self, primed=()):
        self.order = list(primed)[-MT_TABS:]

    def use(self, key):
        miss = key not in self.order
        if not miss:
            self.order.remove(key)
        elif len(self.order) == MT_TABS:
            self.order.pop(0)
        self.order.append(key)
        return miss


# ------------------------------------------------------------------------------------------------ Adam: reference, bound, emulation
def f32(x):
    return float(np.float32(x))


def adam_scalars(step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """(b1, b2, eps, step_size, bc2_sqrt) as FusedAdam.step hands them to st_mt_adam (Python floats: the betas travel as doubles, the others are rounded to fp32 by the C ABI)"""
    return b1, b2, eps, lr / (1.0 - b1 ** step), (1.0 - b2 ** step) ** 0.5


def _scal(b1, b2, eps, step_size, bc2_sqrt, exact):
    if exact:
        return b1, b2, eps, step_size, bc2_sqrt, 1.0 - b1, 1.0 - b2
    return f32(b1), f32(b2), f32(eps), f32(step_size), f32(bc2_sqrt), f32(1.0 - b1), f32(1.0 - b2)


def adam_ref(p, g, m, v, b1, b2, eps, step_size, bc2_sqrt, exact_scalars=False):
    """One Adam step in float64, in the kernel's formulation (mt_body<2>):
        m' = m + (g - m)(1 - b1);  v' = (1 - b2) g^2 + b2 v;  denom = sqrt(v') / bc2_sqrt + eps;  q = m' / denom;  p' = p - step_size q
    The scalars are INPUTS of the kernel: they are taken at their fp32-rounded values, and 1 - b at its own: (float)(1.0 - b), rounded
    once from the double as the kernel's entry point forms it -- and as torch's Adam does: 1.0f - (float)0.999 = 0.00099998713 is 1.3e-5 off
    (exact_scalars: everything in float64, for the comparison with float64 torch.optim.Adam).  -> p', m', v', denom, q (float64)"""
    b1, b2, eps, step_size, bc2_sqrt, omb1, omb2 = _scal(b1, b2, eps, step_size, bc2_sqrt, exact_scalars)
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    m1 = m + (g - m) * omb1
    v1 = omb2 * (g * g) + v * b2
    denom = v1.sqrt() / bc2_sqrt + eps
    q = m1 / denom
    return p - step_size * q, m1, v1, denom, q


def adam_bound(p, g, m, v, b1, b2, eps, step_size, bc2_sqrt):
    """First-order rounding bounds (E_p, E_m, E_v) of the kernel's operation sequence against adam_ref, U = 2^-24, every operation
    correctly rounded (the library is built without fast-math: hipcc's default is a correctly rounded fp32 divide and square root):
        d = fl(g - m): U|g - m|, carried through the multiply by (1 - b1);  m' = fma(d, 1 - b1, m): U|m'|
            E_m = U(|m'| + (1 - b1)|g - m|)
        g2 = fl(g g): U g^2;  vb = fl(v b2): U v b2;  v' = fma(1 - b2, g2, vb): U v'.  All terms are >= 0, so (1 - b2) g^2 + b2 v = v'
        and the three sum to 2U v'; the bound is stated with one more U as margin (test_optim_host.py holds an fp32 emulation of
        the sequence to it)
            E_v = 3U v'
        sqrt(v'): 3U / 2 inherited + U;  / bc2_sqrt: U;  + eps: U;  q = m' / denom: U and E_m / denom -- 5.5U |q| in all; 14U |q| is the
        chosen ceiling over that;  p' = fma(-step_size, q, p): U|p'|
            E_p = U|p'| + step_size (E_m / denom + 14U |q|)
    The tests assert 2x these (second-order terms, and a divide / square root of 2 ulp instead of 0.5)."""
    p1, m1, v1, denom, q = adam_ref(p, g, m, v, b1, b2, eps, step_size, bc2_sqrt)
    omb1 = _scal(b1, b2, eps, step_size, bc2_sqrt, False)[5]
    gd, md = g.detach().cpu().double(), m.detach().cpu().double()
    e_m = U * (m1.abs() + omb1 * (gd - md).abs())
    e_v = 3 * U * v1
    e_p = U * p1.abs() + f32(step_size) * (e_m / denom + 14 * U * q.abs())
    return e_p, e_m, e_v


def _fma32(a, b, c):
    # a * b is exact in float64 (24 + 24 bits); the sum rounds to 53 bits and then to 24: the double rounding moves a result by one
    # ulp only when the float64 sum falls within 2^-29 ulp of a tie
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_emulate_f32(p, g, m, v, b1, b2, eps, step_size, bc2_sqrt):
    """mt_body<2>'s `upd`, operation by operation, in numpy float32 (every operation correctly rounded) -> p', m', v' (float32 arrays)"""
    p, g, m, v = (np.asarray(t, dtype=np.float32) for t in (p, g, m, v))
    omb1, omb2 = np.float32(1.0 - b1), np.float32(1.0 - b2)
    b1, b2, eps, step_size, bc2_sqrt = (np.float32(x) for x in (b1, b2, eps, step_size, bc2_sqrt))
    m1 = _fma32(g - m, np.broadcast_to(omb1, g.shape), m)
    g2, vb = g * g, v * b2
    v1 = _fma32(np.broadcast_to(omb2, g.shape), g2, vb)
    denom = np.sqrt(v1) / bc2_sqrt + eps
    q = m1 / denom
    p1 = _fma32(np.broadcast_to(-step_size, g.shape), q, p)
    return p1, m1, v1


def adam_operands(n, seed):
    """(p, g, m, v) float32 CPU tensors: magnitudes log-uniform over 1e-12 ... 1e4 (v >= 0), random signs, exact zeros in g, m and v
    (about one element in eight each) and all three zero together (every 16th element); no fp32 subnormal goes in or comes up inside
    (the smallest intermediate, (1 - b2) g^2 at |g| = 1e-12, is 1e-27)"""
    gen = torch.Generator().manual_seed(seed)

    def mag():
        return 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 16.0 - 12.0)

    def sign():
        return torch.randint(0, 2, (n,), generator=gen).double() * 2.0 - 1.0
    p, g, m, v = mag() * sign(), mag() * sign(), mag() * sign(), mag()
    for t in (g, m, v):
        t[torch.rand(n, generator=gen) < 0.125] = 0.0
    idx = torch.arange(n)
    for t in (g, m, v):
        t[idx % 16 == 5] = 0.0
    out = [t.float() for t in (p, g, m, v)]
    for t in out:
        assert bool(((t == 0) | (t.abs() >= 1e-15)).all())
    return out


# ------------------------------------------------------------------------------------------------ gradient norm
def norm_bound(n_blocks, scaled=False):
    """Relative bound of st_mt_grad_norm against the float64 norm, from the depth of its fixed summation order.  Every term is a square,
    so a sum of k roundings is off by at most k U relative (first order), whatever the data.  Deepest path of one value:
      64  fused multiply-adds into its running sum: a chunk is 8192 four-float pieces over 256 threads = 32 pieces per thread, which
          alternate between two running sums, 16 pieces x 4 floats each (unaligned tensors take the same pieces float by float)
      1   acc + acc2
      6   levels of the wave sum (st_wave_sum over 64 lanes)
      4   the four waves' sums added in turn by thread 0: the first, to 0.0, is exact, so 3 -- the fourth pays for the one tail float
          (n % 4 of them, one each for threads 0 .. 2) that a thread of a 32767-float chunk adds to a first sum that already took 64
      ceil(blocks / 64)   partials per lane in mt_norm_final_kernel
      6   levels of its wave sum
    = (81 + ceil(blocks / 64)) U on the sum of squares; the square root halves it and rounds once more: (41.5 + ceil(blocks / 64) / 2) U,
    stated as (42 + ceil(blocks / 64) / 2) U.  scaled: one more rounding for the multiplication by pre_scale."""
    return (42.0 + math.ceil(n_blocks / 64) / 2.0 + (1.0 if scaled else 0.0)) * U


def _fma32x(a, b, c):
    # (extended precision where numpy has it: 48-bit product + 24-bit addend round to 64 bits, then to 24 -- a double rounding needs
    # the sum within 2^-40 ulp of a tie)
    ld = np.longdouble
    return (a.astype(ld) * b.astype(ld) + c.astype(ld)).astype(np.float32)


def _wave_sum32(v):
    """st_wave_sum: v += shuffle_xor(v, off) for off = 32, 16, ... 1, over the last axis of 64 lanes"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v


def norm_emulate_f32(tensors, pre_scale=1.0):
    """st_mt_grad_norm's FIXED summation order in numpy float32, addition by addition -- what the device must give bit for bit.
    A block takes one 32768-float chunk; thread t of 256 takes the four-float pieces t, t + 256, ... of the chunk: its even pieces (in the
    order it meets them) go through four fused multiply-adds each into `acc`, the odd ones into `acc2` -- whether a piece is met in an
    eight-piece round, a two-piece round or alone; the chunk's n % 4 last floats go to `acc` of threads 0 .. 2.  Then acc + acc2, the
    xor-butterfly over each wave's 64 lanes, the four waves' sums added in turn from 0.0: the block's partial.  One wave sums the partials
    (lane j: j, j + 64, ... in turn from 0.0), the butterfly again, the square root, and the multiplication by pre_scale unless it is 1."""
    partials = []
    for t in tensors:
        x = np.asarray(t.detach().cpu().reshape(-1).numpy() if torch.is_tensor(t) else t, dtype=np.float32)
        for beg in range(0, x.size, MT_CHUNK):
            ch = x[beg:beg + MT_CHUNK]
            npc = ch.size // 4
            rounds = -(-npc // MT_THREADS)
            pieces = np.zeros((rounds * MT_THREADS, 4), dtype=np.float32)          # (a zero piece adds nothing: x + 0 = x)
            pieces[:npc] = ch[:npc * 4].reshape(npc, 4)
            pieces = pieces.reshape(rounds, MT_THREADS, 4)
            acc = [np.zeros(MT_THREADS, dtype=np.float32), np.zeros(MT_THREADS, dtype=np.float32)]
            for k in range(rounds):
                for c in range(4):
                    acc[k % 2] = _fma32x(pieces[k, :, c], pieces[k, :, c], acc[k % 2])
            tail = np.zeros(MT_THREADS, dtype=np.float32)
            tail[:ch.size - npc * 4] = ch[npc * 4:]
            acc[0] = _fma32x(tail, tail, acc[0])
            waves = _wave_sum32((acc[0] + acc[1]).reshape(4, 64))[:, 0]
            s = np.float32(0.0)
            for w in waves:
                s = np.float32(s + w)
            partials.append(s)
    lanes = np.zeros(64, dtype=np.float32)
    for i, part in enumerate(partials):
        lanes[i % 64] = np.float32(lanes[i % 64] + part)
    out = np.sqrt(_wave_sum32(lanes)[0])
    return np.float32(out) if pre_scale == 1.0 else np.float32(out * np.float32(pre_scale))


def order_probes(n):
    """[(label, gradient)]: gradients of n floats whose norm shows WHICH running sum a piece joined.  On random data a piece that joins
    the other sum moves the last bit of one thread's sum, which the wave sums and the square root mostly absorb.  Here one thread of one
    chunk holds everything: its piece `parity` (0 or 1: the first of one running sum) is [4096, 0, 0, 0], so that sum stands at 2^24,
    where a further 1.0 * 1.0 is absorbed (2^24 + 1 is a tie and rounds to the even 2^24); its later pieces of the same parity, and its
    tail float, are ones, every other float of the tensor is zero.  As long as each of those pieces joins the sum it belongs to, the
    norm is 4096 exactly; one that joins the other sum is counted there (+ 4 in 2^24: one ulp of the norm).  One probe per chunk, per
    parity and for threads 0 and 255 (the last thread takes one piece fewer in a ragged chunk), and one for the tail."""
    out = []
    for c0 in range(0, n, MT_CHUNK):
        ln = min(MT_CHUNK, n - c0)
        npc = ln // 4
        for thread in (0, MT_THREADS - 1):
            mine = list(range(thread, npc, MT_THREADS))          # this thread's pieces, in the order it meets them
            for parity in (0, 1):
                if len(mine) <= parity:
                    continue
                x = torch.zeros(n)
                for k, piece in enumerate(mine):
                    if k % 2 == parity:
                        x[c0 + 4 * piece:c0 + 4 * piece + 4] = 1.0
                x[c0 + 4 * mine[parity]:c0 + 4 * mine[parity] + 4] = torch.tensor([4096.0, 0.0, 0.0, 0.0])
                if parity == 0 and npc * 4 + thread < ln:      # (the tail floats join the first sum)
                    x[c0 + npc * 4 + thread] = 1.0
                out.append(('chunk%d_thread%d_parity%d' % (c0 // MT_CHUNK, thread, parity), x))
        if ln % 4 and npc > MT_THREADS:
            # the tail float of thread 0 joins the FIRST sum: that one holds 1 + 1 from piece 0, the other 2^24 from piece 1; with the
            # tail's 1 the sums join to 2^24 + 3 -> 2^24 + 4 (a tie, to even), without it to 2^24 + 2: one ulp of the norm apart
            x = torch.zeros(n)
            x[c0:c0 + 2] = 1.0
            x[c0 + 4 * MT_THREADS] = 4096.0
            x[c0 + npc * 4] = 1.0
            out.append(('chunk%d_tail' % (c0 // MT_CHUNK), x))
    return out


def norm_ref(tensors, pre_scale=1.0):
    """float64 L2 norm over a tensor list (pre_scale at its fp32 value: an input of the kernel)"""
    s = sum(float((t.detach().double() ** 2).sum()) for t in tensors)
    return math.sqrt(s) * f32(pre_scale)


def clip_coef(norm_f32, max_norm, pre_scale=1.0):
    """the clip launch's factor, formed in fp32 from the DEVICE norm as mt_body<1> forms it"""
    with np.errstate(all='ignore'):
        coef = np.float32(max_norm) / (np.float32(norm_f32) + np.float32(1e-6))
        coef = (coef if coef < np.float32(1.0) else np.float32(1.0)) * np.float32(pre_scale)
    return float(coef)
