"""The shared, seeded case table of the alignment tests (tests/test_xcorr_host.py guards it on the CPU, tests/test_gpu_xcorr.py runs it on
the MI355X).  A case is a dict(name, x, y, D, shift, pcm, zero_mean, dc, nan): x the reference, y the processed signal (float32, the
lengths may differ), D the search bound, shift the planted delay (None where the signals are too short or too special to plant one).

Shapes follow the kernel's constants, so the table moves with them: C = ops.XCORR_CHUNK (the staged piece, the smallest chunk of x),
T = ops.XCORR_LAG_TILE (the lags of a workgroup), M = ops.XCORR_MAX_CHUNKS (past M C samples the chunk grows to 2 C).
Signals: an AR(1) sequence with coefficient 0.9, peak 0.5, its mean over the planted overlap removed, rounded to 16-bit PCM; the processed side is the copy
shifted by `shift` samples (y[n + shift] = x[n], zeros where x has nothing) plus white noise at a tenth of the level, rounded again.
The float cases are the same signals times an irrational gain, not rounded."""
import numpy as np

from semi_tts_amd import ops

C, T, M = ops.XCORR_CHUNK, ops.XCORR_LAG_TILE, ops.XCORR_MAX_CHUNKS
GAP = 1e-6              # every float case keeps this relative gap between its two largest r
MEAN_SHARE = 0.01       # every zero-mean case keeps (sum x)^2 / n <= this share of sum x^2 (but the marked DC case)


def pcm(v):
    return (np.rint(np.clip(np.asarray(v, np.float64), -1.0, 1.0) * 32767.0) / 32768.0).astype(np.float32)


def ar1(L, rs):
    e = rs.randn(L + 64)
    s = np.zeros(L + 64)
    for n in range(1, L + 64):
        s[n] = 0.9 * s[n - 1] + e[n]
    s = s[64:]
    s = s - s.mean()
    return s * (0.5 / max(np.abs(s).max(), 1e-9))


def shifted(x, Ly, shift, rs, noise=0.1):
    """y[m] = x[m - shift] inside x, 0 outside, plus noise"""
    y = np.zeros(Ly)
    m = np.arange(Ly)
    src = m - shift
    ok = (src >= 0) & (src < len(x))
    y[ok] = x[src[ok]]
    return y + noise * np.sqrt(np.mean(x ** 2)) * rs.randn(Ly)


# (name, Lx, Ly, D, shift, float?)
SHAPES = (
    ('L1', 1, 1, 1, None, False),
    ('L2', 2, 2, 1, None, False),
    ('C-1/D=T-1/+1', C - 1, C - 1, T - 1, 1, False),
    ('C/D=T/-1', C, C, T, -1, False),
    ('C+1/D=T+1/0', C + 1, C + 1, T + 1, 0, False),             # D > L: most lags have an empty overlap
    ('2C+1/D=1/+D', 2 * C + 1, 2 * C + 1, 1, 1, False),          # the delay on the search bound
    ('2C+1/D=1/-D', 2 * C + 1, 2 * C + 1, 1, -1, False),
    ('2C+1/D=0', 2 * C + 1, 2 * C + 1, 0, 0, False),
    ('Lx>Ly/+D', 2 * C + 1, C + 100, 37, 37, False),
    ('Lx<Ly/-D', C - 1, 2 * C + 1, 37, -37, False),
    ('300/D=T+1', 300, 280, T + 1, 5, False),                    # D > L on both sides
    ('MC/D=3', M * C, M * C - 50, 3, -2, False),                 # the last length with chunks of C
    ('MC+1/D=3', M * C + 1, M * C - 50, 3, 2, False),            # the first with chunks of 2 C
    ('f/C+1/D=T+1', C + 1, C + 1, T + 1, 0, True),
    ('f/Lx>Ly/+D', 2 * C + 1, C + 100, 37, 37, True),
    ('f/Lx<Ly/-1', C - 1, 2 * C + 1, 1, -1, True),
    ('f/MC+1/D=3', M * C + 1, M * C - 50, 3, 2, True),
)


def _case(name, x, y, D, shift, **kw):
    d = dict(name=name, x=np.ascontiguousarray(x, np.float32), y=np.ascontiguousarray(y, np.float32), D=D, shift=shift, pcm=True, zero_mean=True,
             dc=False, nan=False)
    d.update(kw)
    return d


def _build():
    out = []
    for i, (name, Lx, Ly, D, shift, flt) in enumerate(SHAPES):
        rs = np.random.RandomState([11, i])
        x = ar1(Lx, rs)
        x0, n = max(0, -(shift or 0)), min(Lx - max(0, -(shift or 0)), Ly - max(0, shift or 0))
        x = x - x[x0:x0 + n].mean()                                 # mean-free over the overlap the planted delay leaves (the zero-mean guard)
        y = shifted(x, Ly, shift or 0, rs)
        if flt:
            g = np.float32(0.7371)
            out.append(_case(name, x.astype(np.float32) * g, y.astype(np.float32) * np.float32(1.1317), D, shift, pcm=False))
        else:
            out.append(_case(name, pcm(x), pcm(y), D, shift, zero_mean=min(Lx, Ly) >= 16))
    # ties: x an impulse at 5, y impulses at 3 and 7 -> r[-2] = r[+2], +2 wins
    x, y = np.zeros(16), np.zeros(16)
    x[5], y[3], y[7] = 0.5, 0.25, 0.25
    out.append(_case('tie/+-2', pcm(x), pcm(y), 4, 2, zero_mean=False))
    # every r is 0 or negative: r[0] < 0, the others 0 -> +1 (the smallest |d| among the zeros, the non-negative one)
    x, y = np.zeros(8), np.zeros(8)
    x[3], y[3] = 0.5, -0.5
    out.append(_case('negative', pcm(x), pcm(y), 2, 1, zero_mean=False))
    rs = np.random.RandomState([11, 100])
    a = pcm(ar1(100, rs))
    out.append(_case('zero-x', np.zeros(100), a, 5, 0, zero_mean=False))             # an all-zero side: delay 0 (coef 0 / 0 = NaN)
    out.append(_case('zero-y', a, np.zeros(90), 5, 0, zero_mean=False))
    # a large DC offset on both sides: the marked case of the zero-mean guard
    rs = np.random.RandomState([11, 101])
    x = ar1(C + 1, rs) * 0.5
    out.append(_case('dc', pcm(x + 0.4), pcm(shifted(x, C + 1, 3, rs) + 0.4), 8, None, dc=True))
    # a NaN in x, three samples before its end: the lags d >= 3 do not reach it
    rs = np.random.RandomState([11, 102])
    x = ar1(C + 1, rs)
    xn = pcm(x)
    xn[C - 2] = np.nan
    out.append(_case('nan-x', xn, pcm(shifted(x, C + 1, 2, rs)), 5, None, pcm=False, zero_mean=False, nan=True))
    return out


CASES = _build()
assert len(CASES) <= 64 and len({c['name'] for c in CASES}) == len(CASES)


def by_name(name):
    return next(c for c in CASES if c['name'] == name)


_ORACLE = {}


def oracle(case, D=None):
    """xcorr_oracle.delay of a case at its own D (or another), computed once and shared by the tests that need it (not to be modified)"""
    import xcorr_oracle as XO
    D = case['D'] if D is None else D
    key = (case['name'], D)
    if key not in _ORACLE:
        _ORACLE[key] = XO.delay(case['x'], case['y'], D)
    return _ORACLE[key]
