"""The shared, seeded case table of the loudness tests (tests/test_loudness_host.py guards it on the CPU, tests/test_gpu_loudness.py
runs it on the MI355X).  A case is a dict(name, fs, x, target, peak_db, max_gain_db): x one float32 utterance.

Rates: 8000 (hop 800, the main one: smallest and fastest), 11025 (hop 1103, odd: the short run at the front of a hop), 16000, and
48000 for two cases only (hop 4800, the longest run and the poles nearest 1).  Nothing is longer than 3 s.  Every case on which the
GPU tests compare integers with the float64 oracle has to keep MARGIN_LU between every block loudness and both gates
(tests/test_loudness_host.py asserts it): an amplitude that does not is tuned HERE, never skipped."""
import numpy as np

MARGIN_LU = 0.05
TARGET, PEAK_DB, MAX_GAIN_DB = -23.0, -1.0, 30.0
RATES = (8000, 11025, 16000)
THREADS = 256


def hop_of(fs):
    return (fs + 5) // 10


def run_of(fs):
    """what st_loudness_run_length returns: samples one thread owns"""
    return (hop_of(fs) + THREADS - 1) // THREADS


def noise(L, seed, amp=0.1):
    return (amp * np.random.RandomState([seed, L]).randn(L)).astype(np.float32)


def sine(L, fs, amp=0.5, f=997.0):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(L) / fs)).astype(np.float32)


def _case(name, fs, x, target=TARGET, peak_db=PEAK_DB, max_gain_db=MAX_GAIN_DB):
    return dict(name='%d/%s' % (fs, name), fs=fs, x=np.ascontiguousarray(x, np.float32), target=target, peak_db=peak_db, max_gain_db=max_gain_db)


def length_cases(fs):
    """4 hops - 1 (no block), exactly 4 hops, 4 hops + 1, 7 hops - 1, and lengths one either side of a multiple of the run length"""
    hop, r = hop_of(fs), run_of(fs)
    k = (11 * hop // 2) // r                                       # k r lies inside hop 5
    return [_case('len%d' % L, fs, noise(L, 1)) for L in (4 * hop - 1, 4 * hop, 4 * hop + 1, 7 * hop - 1, k * r - 1, k * r + 1)]


def signal_cases(fs):
    hop = hop_of(fs)
    out = [_case('noise', fs, noise(9 * hop + 17, 2)), _case('sine997', fs, sine(8 * hop + 3, fs))]
    for name, i in (('impulse0', 0), ('impulse_end_hop1', 2 * hop - 1), ('impulse_start_hop2', 2 * hop)):
        x = np.zeros(7 * hop - 1, np.float32)
        x[i] = 1.0
        out.append(_case(name, fs, x))
    rs = np.random.RandomState([3, fs])
    out.append(_case('burst_then_silence', fs, np.concatenate([rs.uniform(-1.0, 1.0, 3 * hop), np.zeros(5 * hop + 7)])))
    loud, quiet = 0.3, 0.3 * 10.0 ** (-25.0 / 20.0)
    out.append(_case('loud_quiet_loud', fs, np.concatenate([loud * rs.randn(6 * hop), quiet * rs.randn(8 * hop), loud * rs.randn(6 * hop + 5)]).clip(-1, 1)))
    out.append(_case('minus80', fs, noise(8 * hop, 4, amp=1e-4)))
    out.append(_case('zeros', fs, np.zeros(6 * hop + 1, np.float32)))
    x = noise(10 * hop, 5, amp=0.01)
    x[hop // 2::hop] = 0.95                                        # high crest: the peak ceiling binds
    out.append(_case('high_crest', fs, x))
    out.append(_case('very_quiet', fs, noise(8 * hop + 9, 6, amp=1e-3)))       # about -58 LUFS: more than max_gain_db from the target
    return out


def wide_cases():
    """48 kHz, two cases: DC 0.5 (a missing or wrong carry restarts the high-pass transient in every unit) and noise"""
    fs = 48000
    return [_case('dc', fs, np.full(15 * hop_of(fs) + 100, 0.5, np.float32)), _case('noise', fs, noise(6 * hop_of(fs) + 4801, 7))]


def nonfinite_case(fs=8000):
    """-> (case, index of its one NaN sample)"""
    hop = hop_of(fs)
    x = noise(8 * hop + 5, 8)
    i = 3 * hop + 123
    x[i] = np.nan
    return _case('nan', fs, x), i


def kernel_cases():
    return [c for fs in RATES for c in length_cases(fs) + signal_cases(fs)] + wide_cases()


def integer_cases():
    """every case whose counts and flags a GPU test compares with the oracle"""
    return kernel_cases()


def neighbours(fs, seed=9):
    """two full-scale utterances to pack a case between"""
    hop = hop_of(fs)
    rs = np.random.RandomState([seed, fs])
    return [_case('full_a', fs, rs.uniform(-1.0, 1.0, 5 * hop + 3)), _case('full_b', fs, rs.uniform(-1.0, 1.0, 4 * hop + 11))]


def ragged_pool(fs, n, seed=10):
    """n ragged utterances of 1 sample .. 9 hops at assorted levels: the B = 64 / 65 batches"""
    rs = np.random.RandomState([seed, fs, n])
    hop = hop_of(fs)
    return [_case('pool%d' % k, fs, noise(int(rs.randint(1, 9 * hop)), 100 + k, amp=float(10.0 ** rs.uniform(-3.0, -0.7)))) for k in range(n)]
