"""The shared, seeded case table of the silence-trimming tests (tests/test_trim_host.py guards it on the CPU, tests/test_gpu_trim.py
runs it on the MI355X).  A case is a dict(name, fl, hop, top_db, pad, max_iv, x): x one float32 utterance.

Signals: a floor of white noise at 1e-4 (or none) with bursts at 0.3 -- uniform noise, or a constant (`dc`) where a frame's share of
a burst has to be an exact count of samples.  Every case on which the GPU tests compare integers with the float64 oracle has to keep
trim_oracle.margin_db >= MARGIN_DB: a seed that does not is replaced HERE, never skipped."""
import numpy as np

FRAMINGS = ((64, 16), (64, 64), (65, 7), (2048, 512))
WIDE = (8192, 1)                 # the widest frame at the smallest hop, on one short signal
RUN, CHUNK = 16, 256             # ops.TRIM_RUN (16 at every framing above) and ops.TRIM_CHUNK: the frame counts straddle both
MARGIN_DB = 0.01


def signal(L, bursts, seed, amp=0.3, floor=1e-4, dc=False):
    rs = np.random.RandomState([seed, L])
    x = floor * rs.randn(L)
    for a, b in bursts:
        a, b = max(int(a), 0), min(int(b), L)
        if b > a:
            x[a:b] = amp if dc else amp * rs.uniform(-1.0, 1.0, b - a)
    return x.astype(np.float32)


def _case(name, fl, hop, x, top_db=30.0, pad=0, max_iv=0):
    return dict(name='%dx%d/%s' % (fl, hop, name), fl=fl, hop=hop, top_db=float(top_db), pad=int(pad), max_iv=int(max_iv), x=x)


def single_frame_top_db(fl, hop):
    """a threshold half way (in dB) between a frame that holds a whole constant burst of fl samples and its neighbours, which hold
    fl - hop of them"""
    return 30.0 if hop >= fl else 0.5 * -10.0 * np.log10((fl - hop) / float(fl))


def framing_cases(fl, hop):
    h, out = hop, []
    for L in sorted({1, hop - 1, hop, hop + 1, fl // 2 - 1, fl // 2 + 1, 5 * hop + 3} - {0}):
        out.append(_case('len%d' % L, fl, hop, signal(L, [(0, max(1, L // 2))], 1), max_iv=2))
    L = 40 * h + 5
    out.append(_case('ends', fl, hop, signal(L, [(0, 6 * h), (L - 5 * h, L)], 2), max_iv=4))
    s = 8 * h - fl // 2
    out.append(_case('single', fl, hop, signal(20 * h + 3, [(s, s + fl)], 3, floor=0.0, dc=True), top_db=single_frame_top_db(fl, hop), max_iv=2))
    out.append(_case('silence', fl, hop, np.zeros(10 * h + 3, np.float32), max_iv=2))
    out.append(_case('loud', fl, hop, signal(12 * h + 1, [(0, 12 * h + 1)], 4), max_iv=2))
    L = 30 * h + 7
    out.append(_case('pad', fl, hop, signal(L, [(10 * h, 15 * h)], 5), pad=10 * L))
    L = 60 * h + 11
    for k in (2, 3, 5):          # three runs: max_iv below, at and above
        out.append(_case('bursts_iv%d' % k, fl, hop, signal(L, [(5 * h, 9 * h), (25 * h, 30 * h), (48 * h, 52 * h)], 6), pad=h // 2, max_iv=k))
    for T in (RUN - 1, RUN, RUN + 1):
        L = (T - 1) * h + h // 2
        out.append(_case('run_T%d' % T, fl, hop, signal(L, [(0, h), ((T - 3) * h, L)], 7), max_iv=3))
    for T in (CHUNK - 1, CHUNK, CHUNK + 1):
        L = (T - 1) * h + h // 2
        out.append(_case('chunk_T%d' % T, fl, hop, signal(L, [(100 * h, 101 * h), (250 * h, L)], 8), max_iv=4))
    # a run that starts on the first frame of the second chunk (one sample of a constant burst inside frame 256) and one across 511 / 512
    s = CHUNK * h - fl // 2 + fl - 1
    out.append(_case('chunk_start', fl, hop, signal(600 * h + 1, [(s, s + 3 * h), (510 * h, 514 * h)], 9, floor=0.0, dc=True), top_db=40.0, max_iv=4))
    return out


def wide_case():
    fl, hop = WIDE
    return _case('short', fl, hop, signal(6000, [(100, 600)], 10, floor=0.0, dc=True), top_db=9.957, max_iv=2)


def kernel_cases():
    return [c for fl, hop in FRAMINGS for c in framing_cases(fl, hop)] + [wide_case()]


def pool(n, fl, hop, seed):
    """n ragged utterances of 1 .. 40 hop samples with one or two bursts: the batches of the independence tests"""
    rs = np.random.RandomState([seed, n, fl, hop])
    out = []
    for k in range(n):
        L = int(rs.randint(1, 40 * hop + 1))
        bursts = [(int(a), int(a) + int(rs.randint(1, 6 * hop))) for a in rs.randint(0, L, int(rs.randint(1, 3)))]
        out.append(_case('pool%d_%d' % (n, k), fl, hop, signal(L, bursts, seed + k), pad=hop, max_iv=3))
    return out


POOLS = ((1, 64, 16, 20), (3, 64, 16, 21), (64, 64, 16, 22), (65, 64, 16, 23), (3, 2048, 512, 24), (5, 65, 7, 25))


def neighbour_case():
    """a quiet utterance with one small burst, to be placed between loud samples of a larger buffer"""
    return _case('quiet', 64, 16, signal(403, [(150, 190)], 30, amp=0.01, floor=1e-5), pad=8, max_iv=3)


def nonfinite_cases():
    """[(case, sample index, value)]: one non-finite sample each; the frames that read it carry it"""
    base = signal(50 * 16 + 5, [(200, 400)], 31)
    out = []
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        x = base.copy()
        i = 300 + 37 * k
        x[i] = v
        out.append((_case('nonfinite%d' % k, 64, 16, x, max_iv=3), i, v))
    return out


def integer_cases():
    """every case whose bounds / n_iv / intervals a GPU test compares with the oracle"""
    return kernel_cases() + [c for p in POOLS for c in pool(*p)] + [neighbour_case()]


# ---------------------------------------------------------------- the exact tie
TIE_FL, TIE_HOP, TIE_TOP_DB = 64, 32, 10.0 * np.log10(256.0)      # ratio = 2^-8 exactly once rounded to float32
TIE_BLOCKS = (0.0, 0.0, 2.0 ** -4, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3, 1.0, 1.0, 2.0 ** -3, 2.0 ** -4, 2.0 ** -4, 0.0, 0.0)


def tie_signal():
    """power-of-two amplitudes held over blocks of TIE_FL / 2 samples: frame t covers blocks t - 1 and t, so its energy
    (a[t-1]^2 + a[t]^2) / 2 is exact in float32 in any summation order.  ref = 1 (frame 7); frames 3, 4 and 10 hold two blocks of 2^-4:
    exactly ref * 2^-8, silent; frames 5 and 9 hold one block of 2^-3 and one of 2^-4: 5 / 512, non-silent.
    -> (x, expected bounds, expected intervals)"""
    x = np.repeat(np.array(TIE_BLOCKS, np.float32), TIE_FL // 2)
    return x, [5 * TIE_HOP, 10 * TIE_HOP, 5, 0], [[5 * TIE_HOP, 10 * TIE_HOP]]
