"""The shared, seeded case table of the intelligibility tests (tests/test_stoi_host.py guards it on the CPU, tests/test_gpu_stoi.py runs
it on the MI355X).  A case is a dict(name, L, deg, x, y): x the clean float32 signal at 10 kHz, y the processed one, equally long.

Signals: harmonic "speech" (a 120 Hz fundamental with vibrato, harmonics to 4 kHz at 1 / h) under a 4 Hz syllable envelope, with muted
stretches at 1e-4 of the level (80 dB down: far under the 40 dB range of the silent-frame rule, so they are dropped).
Degradations: none; white noise at 20, 5 and -5 dB SNR; one loud burst of noise over a twentieth of the signal.
Every case on which the GPU tests compare integers with the float64 oracle has to keep stoi_oracle.margin_db >= MARGIN_DB: a seed that
does not is replaced HERE, never skipped."""
import numpy as np

MARGIN_DB = 0.01
CHUNK = 256                      # ops.STOI_CHUNK: the kept frames of the longest case cross it
# (length, muted stretches as fractions of the length, seed)
LENGTHS = (
    (200, (), 1),                                             # F = 0
    (257, (), 1),                                             # F = 1, M = 0
    (4096, (), 1),                                            # F = K = 30, M = 29: the sentinel
    (4097, (), 1),                                            # M = 30: exactly one segment
    (4097 + 128, (), 1),                                      # two segments
    (7000, ((0.10, 0.18), (0.45, 0.56), (0.80, 0.86)), 1),    # with gaps
    (30000, ((0.05, 0.12), (0.30, 0.33), (0.61, 0.75), (0.93, 1.0)), 1),
    (37000, ((0.20, 0.24), (0.70, 0.73)), 1),                 # F = 288, K > 256: the selection scan carries across its chunk
)
DEGRADATIONS = ('none', 'snr20', 'snr5', 'snr-5', 'burst')
CLIPPING = ('snr5', 'snr-5', 'burst')                         # rule 7 clips some band cells under these, none under snr20 at L = 4097


def speech(L, mutes, seed):
    rs = np.random.RandomState([seed, L])
    t = np.arange(L) / 10000.0
    f0 = 120.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f0) / 10000.0
    x = np.zeros(L)
    for h in range(1, 34):                                    # 33 * 120 Hz = 3960 Hz
        x += np.sin(h * ph + rs.uniform(0, 2 * np.pi)) / h
    env = 0.08 + 0.92 * (0.5 - 0.5 * np.cos(2 * np.pi * 4.0 * t + rs.uniform(0, 2 * np.pi)))
    x *= env
    x *= 0.3 / np.abs(x).max()
    for a, b in mutes:
        x[int(a * L):int(b * L)] *= 1e-4
    return x.astype(np.float32)


def degrade(x, deg, seed):
    rs = np.random.RandomState([seed, len(x), DEGRADATIONS.index(deg)])
    x64 = x.astype(np.float64)
    if deg == 'none':
        return x.copy()
    if deg == 'burst':
        y = x64.copy()
        a = int(0.4 * len(x))
        b = min(len(x), a + max(1, len(x) // 20))
        y[a:b] += 0.8 * rs.uniform(-1.0, 1.0, b - a)
        return y.astype(np.float32)
    snr = float(deg[3:])
    n = rs.randn(len(x))
    n *= np.sqrt((x64 ** 2).mean() / (n ** 2).mean()) * 10.0 ** (-snr / 20.0)
    return (x64 + n).astype(np.float32)


def _build():
    out = []
    for L, mutes, seed in LENGTHS:
        x = speech(L, mutes, seed)
        for deg in DEGRADATIONS:
            out.append(dict(name='L%d/%s' % (L, deg), L=L, deg=deg, x=x, y=degrade(x, deg, seed)))
    return out


CASES = _build()


def by_name(name):
    return next(c for c in CASES if c['name'] == name)


_ORACLE = {}


def oracle(case, dtype=np.float64):
    """the oracle's result for a case, computed once and shared by the tests that need it (not to be modified)"""
    import stoi_oracle as SO
    key = (case['name'], np.dtype(dtype).name)
    if key not in _ORACLE:
        _ORACLE[key] = SO.stoi(case['x'], case['y'], dtype)
    return _ORACLE[key]


def clips(case):
    """whether rule 7 clips some band cells of this case: the noisy and burst degradations of every length that has a segment -- but
    for the burst on 4097 samples, whose one segment holds the burst in every row: its norm scales it back under the bound"""
    return case['deg'] in CLIPPING and case['L'] >= 4097 and case['name'] != 'L4097/burst'
