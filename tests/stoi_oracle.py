"""STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) in float64 numpy: the definition st_stoi_batch implements
(include/semitts.h), written from the papers' steps as pystoi / the authors' Matlab realise them, for signals already at 10 kHz.
`stoi(x, y)` is the yardstick.  `stoi(x, y, dtype=np.float32)` runs the SAME steps with every array in float32 (window, products,
overlap-add, FFT in complex64, band sums, both normalisations, the sums over segments): its distance from the float64 form sizes the
bound the GPU tests grant (8 times it), so it has to really be float32 -- asserted below."""
import numpy as np

FS, N_FRAME, HOP, NFFT, J, N_SEG = 10000, 256, 128, 512, 15, 30
BETA, DYN = -15.0, 40.0
EPS = float(np.finfo(np.float64).eps)          # 2^-52
SENTINEL = 1e-5
MIN_FREQ = 150.0

assert np.fft.rfft(np.zeros(8, np.float32)).dtype == np.complex64, 'this numpy transforms float32 in float64: the float32 form would not be float32'


def band_edges():
    """[(lo, hi)] of the 15 third-octave bands: the bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid k * 10000 / 512"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(J, dtype=np.float64)
    lo = MIN_FREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MIN_FREQ * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


EDGES = band_edges()


def window(dtype=np.float64):
    """hanning(258)[1:-1], computed in float64 and rounded once"""
    n = np.arange(N_FRAME, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 1) / (N_FRAME + 1))).astype(dtype)


def n_frames(L):
    """#{i >= 0 : 128 i < L - 256}"""
    return len(range(0, L - N_FRAME, HOP)) if L > N_FRAME else 0


def frames(x, dtype=np.float64):
    """(F, 256) windowed frames of x by the strict rule"""
    F = n_frames(len(x))
    w = window(dtype)
    if F == 0:
        return np.zeros((0, N_FRAME), dtype)
    idx = HOP * np.arange(F)[:, None] + np.arange(N_FRAME)[None, :]
    return w[None, :] * np.asarray(x, dtype)[idx]


def frame_norms(x, dtype=np.float64):
    """||w x_i||_2 of every frame"""
    fx = frames(x, dtype)
    return np.sqrt((fx * fx).sum(axis=1, dtype=dtype))


def keep_mask(norms):
    """frame i is kept iff 20 log10(norm_i + EPS) > max - 40 dB"""
    if len(norms) == 0:
        return np.zeros(0, bool)
    e = 20.0 * np.log10(np.asarray(norms, np.float64) + EPS)
    return e > e.max() - DYN


def margin_db(x):
    """the smallest distance in dB between a frame's energy and the threshold (inf without frames): the guard of the integer comparisons"""
    nrm = frame_norms(x)
    if len(nrm) == 0:
        return float('inf')
    e = 20.0 * np.log10(nrm + EPS)
    return float(np.abs(e - (e.max() - DYN)).min())


def overlap_add(fr, dtype=np.float64):
    """the (K, 256) frames added at hop 128 in their order -> (K - 1) 128 + 256 samples"""
    K = len(fr)
    out = np.zeros((K - 1) * HOP + N_FRAME, dtype)
    for i in range(K):
        out[i * HOP:i * HOP + N_FRAME] += fr[i]
    return out


def bands_of(sig, dtype=np.float64):
    """(15, M) third-octave band magnitudes of a re-synthesised signal"""
    fr = frames(sig, dtype)                                   # framed and windowed again: M = K - 1 frames
    if len(fr) == 0:
        return np.zeros((J, 0), dtype)
    spec = np.fft.rfft(fr, n=NFFT, axis=1)                    # complex64 for float32 input
    p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    return np.sqrt(np.stack([p[:, lo:hi].sum(axis=1, dtype=dtype) for lo, hi in EDGES]))


def _rows(a, dtype):
    a = a - a.mean(axis=-1, keepdims=True, dtype=dtype)
    return a / (np.sqrt((a * a).sum(axis=-1, keepdims=True, dtype=dtype)) + dtype(EPS))


def correlate(X, Y, dtype=np.float64):
    """(STOI, ESTOI, clipped share) from the (15, M) bands, M >= 30"""
    M = X.shape[1]
    S = M - N_SEG + 1
    idx = np.arange(S)[:, None] + np.arange(N_SEG)[None, :]
    xs, ys = X[:, idx].transpose(1, 0, 2), Y[:, idx].transpose(1, 0, 2)          # (S, 15, 30)
    nx = np.sqrt((xs * xs).sum(axis=2, keepdims=True, dtype=dtype))
    ny = np.sqrt((ys * ys).sum(axis=2, keepdims=True, dtype=dtype))
    c = nx / (ny + dtype(EPS))
    clip = dtype(1.0 + 10.0 ** (-BETA / 20.0)) * xs
    yp = np.minimum(c * ys, clip)                                                # (np.minimum keeps a NaN)
    clipped = float((c * ys > clip).mean())
    d = (_rows(xs, dtype) * _rows(yp, dtype)).sum(dtype=dtype) / dtype(J * S)
    xn, yn = _rows(xs, dtype), _rows(ys, dtype)
    xn = _rows(xn.transpose(0, 2, 1), dtype)                                     # columns: (S, 30, 15)
    yn = _rows(yn.transpose(0, 2, 1), dtype)
    de = (xn * yn).sum(dtype=dtype) / dtype(N_SEG * S)
    return float(d), float(de), clipped


def stoi(x, y, dtype=np.float64):
    """clean x against processed y, both at 10 kHz and equally long -> dict(score (STOI, ESTOI), counts (F, K, M, S), norms (F,), kept
    (K,) frame indices, bands (2, 15, M), clipped: the share of band cells rule 7 clips)"""
    dtype = np.dtype(dtype).type
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.ndim == 1 and x.shape == y.shape
    F = n_frames(len(x))
    nrm = frame_norms(x, dtype)
    empty = dict(norms=nrm, kept=np.zeros(0, np.int64), bands=np.zeros((2, J, 0), dtype), clipped=0.0)
    if not np.isfinite(nrm).all():                            # a non-finite clean energy: NaN, nothing kept
        return dict(empty, score=(float('nan'), float('nan')), counts=(F, 0, 0, 0))
    with np.errstate(all='ignore'):
        kept = np.nonzero(keep_mask(nrm))[0]
        K = len(kept)
        M = max(K - 1, 0)
        if K == 0:
            return dict(empty, score=(SENTINEL, SENTINEL), counts=(F, 0, 0, 0))
        fx, fy = frames(x, dtype)[kept], frames(y, dtype)[kept]
        X, Y = bands_of(overlap_add(fx, dtype), dtype), bands_of(overlap_add(fy, dtype), dtype)
        res = dict(norms=nrm, kept=kept, bands=np.stack([X, Y]), clipped=0.0)
        if M < N_SEG:
            return dict(res, score=(SENTINEL, SENTINEL), counts=(F, K, M, 0))
        d, de, clipped = correlate(X, Y, dtype)
    return dict(res, score=(d, de), counts=(F, K, M, M - N_SEG + 1), clipped=clipped)
