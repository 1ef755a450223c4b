"""Case tables of the audio kernels (semi_tts_amd/csrc/audio.hip) -- STFT / iSTFT, Griffin-Lim, the final overlap-add with its
blocked de-emphasis scan, feature extraction and the built-in noise generator -- shared by the host-side test
(test_audio_cases_host.py: every row is accepted by the library's checks and by the float64 oracles, and the oracles alone stay
inside every bound with a margin of four) and the GPU tests (test_gpu_audio_edges.py, test_gpu_features_edges.py: every row
against gl_oracle / feat_oracle in float64).

The bounds are the project's own (test_gpu_audio.py `_close` / `_check_gl`, test_gpu_features.py LIN_TOL / MEL_TOL), restated here
so that both sides read one value.  Two have no precedent: DEEMPH_SLACK (the blocked scan may err DEEMPH_SLACK times what a plain
serial float32 evaluation of y[n] = x[n] + 0.97 y[n-1] errs on the same input) and NOISE_TOL (the generator against
`feature_noise_ref`, about five float32 roundings on magnitudes <= sqrt(2 * 24 ln 2) = 5.77; samples whose u1 mantissa is within
NOISE_EXEMPT_U1 of 2^24 are exempt, where the cancellation of logf near 1 dominates).

This module also holds the numpy restatement of the generator: Philox4x32-10 (Salmon et al., SC'11) on the counter
(i lo, i hi, utterance, 0) with the key (seed lo, seed hi), then Box-Muller in float64 on u1 = ((r0 >> 8) + 1) / 2^24 and
u2 = (r1 >> 8) / 2^24."""
import numpy as np
import torch

import feat_oracle as FO
import gl_oracle as GL

# ---------------------------------------------------------------- bounds
STFT_TOL = (1e-6, 1e-5)            # rel-L2, max-abs / scale  (test_gpu_audio._close as its STFT / iSTFT tests call it)
GL_TOL = (1e-4, 1e-3)              # test_gpu_audio._check_gl
LIN_TOL, MEL_TOL = 5e-4, 1e-4      # test_gpu_features
DEEMPH_SLACK = 8
NOISE_TOL = 4e-6
NOISE_EXEMPT_U1 = 64               # u1 mantissa >= 2^24 - 64
NOISE_EXEMPT_MAX = 1e-4            # at most this fraction of the compared samples


# ---------------------------------------------------------------- signals
def harmonic(B, L, seed=0):
    """test_gpu_audio._signal: six harmonics under a 3 Hz tremolo plus 2 % noise"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 22050
    f0 = 110 + 200 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = sum(0.4 / (h + 1) * torch.sin(2 * np.pi * f0 * (h + 1) * t) for h in range(6))
    return (x * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t)) + 0.02 * torch.randn(B, L, generator=g, dtype=torch.float64)).float()


def white(B, L, seed=0):
    return (0.3 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).float()


def impulses(B, L, seed=0):
    """unit impulses at samples 0, 1, L // 2 and L - 1 (scaled per utterance): an index or reflection error moves whole bins"""
    x = torch.zeros(B, L)
    for b in range(B):
        x[b, [0, 1, L // 2, L - 1]] = 1.0 / (b + 1)
    return x


SIGNALS = {'harmonic': harmonic, 'white': white, 'impulses': impulses}

# ---------------------------------------------------------------- A. STFT / iSTFT
# (n_fft, hop, win, L)
STFT_CASES = [
    (2048, 275, 1102, 1025),            # the shortest legal signal: T = 4, a frame reflecting at both ends
    (2048, 275, 1102, 275 * 7 + 274),   # the largest remainder modulo hop
    (2048, 275, 1101, 2475),            # n_fft - win odd
    (1024, 128, 1023, 128 * 9 + 5),     # n_fft - win odd with the radix-2 stage
    (512, 128, 256, 1152),              # 2 hop == win
    (512, 256, 512, 1280),              # win == n_fft == 2 hop
    (512, 3, 7, 300),                   # a small hop: 101 frames
    (4096, 512, 4096, 2049),            # the shortest legal signal at the largest size
    (4096, 1024, 2048, 5120),
]
# one case per FFT size also runs at B = 1 and an odd B = 5
STFT_BATCH_CASES = [STFT_CASES[2], STFT_CASES[3], STFT_CASES[6], STFT_CASES[8]]


def n_frames(hop, L):
    return 1 + L // hop


def istft_legal(case):
    n_fft, hop, _, L = case
    return hop * (n_frames(hop, L) - 1) > n_fft // 2


ISTFT_CASES = [c for c in STFT_CASES if istft_legal(c)]
ISTFT_REFUSED = [c for c in STFT_CASES if not istft_legal(c)]          # the first and the eighth


def with_batches(cases):
    """[(case, B)]: every case at B = 2, the batch cases also at 1 and 5"""
    return [(c, 2) for c in cases] + [(c, B) for c in STFT_BATCH_CASES if c in cases for B in (1, 5)]


def case_id(p):
    (n_fft, hop, win, L), B = p
    return 'n%d-h%d-w%d-L%d-B%d' % (n_fft, hop, win, L, B)


def stft_input(case, B, signal):
    n_fft, hop, win, L = case
    return SIGNALS[signal](B, L, seed=n_fft + hop + 7 * B)


def stft_reference(x, case, dtype=torch.float64):
    n_fft, hop, win, _ = case
    return GL.stft(x.to(dtype), n_fft, hop, win)                        # (B, F, T) complex


def istft_reference(spec, case, dtype=torch.float64):
    n_fft, hop, win, _ = case
    return GL.istft(spec.to(torch.complex128 if dtype == torch.float64 else torch.complex64), n_fft, hop, win)


# what the library refuses: (entry point, (n_fft, hop, win), L or T, the words its message must carry)
REFUSALS = [
    ('stft', (2048, 275, 1102), 1024, 'reflect'),                       # L = n_fft / 2 exactly
    ('stft', (512, 129, 257), 1152, r'2 \* hop <= win'),                # 2 hop = win + 1
    ('stft', (512, 128, 513), 1152, 'win <= n_fft'),                    # win = n_fft + 1
    ('istft', (2048, 275, 1102), 4, 'reflect'),                         # T below the minimum: hop (T - 1) <= n_fft / 2
    ('istft', (4096, 512, 4096), 5, 'reflect'),
]

# ---------------------------------------------------------------- B. Griffin-Lim
GL_DIMS = [(512, 128, 400), (512, 128, 256), (512, 3, 7), (1024, 128, 1024), (2048, 275, 1101), (4096, 512, 3000)]
GL_ITERS = (0, 1, 30)
GL_ZERO_DIMS = (1024, 128, 1024)        # whole zero frames at both reflected edges, away from 2048
# Griffin-Lim's phase projection X / |X| is discontinuous where a bin passes near zero, and some inputs sit next to such a fork:
# a one-ulp change of their magnitudes moves the float32 result of 30 iterations by 1e-4 (seen at (4096, 512, 3000), shift 0).
# These shifts of the signal's seed choose inputs whose float32 drift stays below 4e-6 under such changes (gl_perturbed).
GL_SEED_SHIFT = {(512, 128, 400): 9, (2048, 275, 1101): 2, (4096, 512, 3000): 3}


def gl_frames(n_fft, hop):
    return n_fft // 2 // hop + 9


def draw_phases(shape, seed):
    """semi_tts_amd.audio.draw_phases from a private generator"""
    return np.angle(np.exp(2j * np.pi * np.random.RandomState(seed).rand(*shape))).astype(np.float32)


def gl_input(dims, B=2, zero_frames=False):
    """-> magnitude (B, F, T) float32 of a real signal's STFT, initial phases (B, F, T) float32 numpy"""
    n_fft, hop, win = dims
    T = gl_frames(n_fft, hop)
    amp = GL.stft(harmonic(B, hop * (T - 1), seed=n_fft + win + GL_SEED_SHIFT.get(dims, 0)).double(), n_fft, hop, win).abs().float()
    if zero_frames:
        amp[0, :, 5:7] = 0               # angle(0) = 0 inside the iterations
        amp[0, :, :2] = 0                # at the reflected left edge
        amp[1, :, -3:] = 0               # and the right one
    return amp, draw_phases(tuple(amp.shape), n_fft + hop)


def gl_perturbed(amp, seed):
    """the magnitudes changed by about one float32 ulp each"""
    return (amp * (1 + 1.2e-7 * torch.randn(amp.shape, generator=torch.Generator().manual_seed(seed)))).float()


def gl_reference(amp, phases, n_iter, dims, dtype=torch.float64):
    n_fft, hop, win = dims
    return GL.griffin_lim(amp.to(dtype), torch.from_numpy(phases), n_iter, n_fft=n_fft, hop=hop, win=win)


# specgram_to_waveform options at the configs' dimensions: T = 12, B = 2.  `gain` scales the signal so that between 5 % and 50 %
# of the reference's samples sit on the clip (a saturated output could hide an error; the clip must be reached).
OPT_T, OPT_B = 12, 2
OPTION_CASES = {
    'power': dict(kw=dict(power=1.5), gain=0.05),
    'is_amp': dict(kw=dict(isAmp=True, power=2.0), gain=0.12),           # the power must be ignored (src/audio.py:186-188)
    # a magnitude again: without the de-emphasis a normalised feature (magnitudes <= 10) stays below 0.7 and never clips
    'no_deemph': dict(kw=dict(inv_preemphasis=False, isAmp=True), gain=2.0),
    'two_d': dict(kw=dict(), gain=0.2),                                  # an (F, T) input
    'clamp': dict(kw=dict(), gain=0.05),                                 # normalised values below 0 and above 1
}


def _normalise_raw(amp):
    """the normalisation without its clamps: (20 log10(amp) - REF_LEVEL_DB - MIN_LEVEL_DB) / -MIN_LEVEL_DB"""
    db = 20 * torch.log10(torch.clamp(amp.double(), min=1e-7)) - GL.REF_LEVEL_DB
    return (db - GL.MIN_LEVEL_DB) / -GL.MIN_LEVEL_DB


def option_input(name):
    """-> (specgram (B, F, T) or (F, T) float32, phases like it, kwargs of specgram_to_waveform)"""
    case = OPTION_CASES[name]
    x = harmonic(OPT_B, GL.HOP * (OPT_T - 1), seed=21).double() * case['gain']
    amp = GL.stft(x).abs()
    ph = draw_phases(tuple(amp.shape), 22)
    if case['kw'].get('isAmp'):
        spec = amp.float()
    elif name == 'clamp':
        spec = _normalise_raw(amp)
        spec[:, :40] += 0.35                                             # the strongest bins above 1 ...
        spec[:, 700:] -= 0.6                                             # ... and the weakest below 0
        assert float(spec.max()) > 1 and float(spec.min()) < 0
        spec = spec.float()
    else:
        spec = torch.clamp(_normalise_raw(amp), 0, 1).float()
    if name == 'two_d':
        spec, ph = spec[1], ph[1]
    return spec, ph, dict(case['kw'])


def option_reference(spec, phases, kw, dtype=torch.float64, clip=True):
    """src/audio.py:179-192 composed from the oracle's parts"""
    s = spec.to(dtype)
    amp = s if kw.get('isAmp') else GL.denormalize_to_amp(s, power=kw.get('power', 1.0))
    squeeze = amp.dim() == 2
    if squeeze:
        amp, phases = amp.unsqueeze(0), phases[None]
    wav = GL.griffin_lim(amp, torch.from_numpy(phases), kw.get('n_iter', GL.GFL_ITER)).double().numpy()
    if kw.get('inv_preemphasis', True):
        wav = GL.inv_preemphasis(wav)
    if clip:
        wav = np.clip(wav, -1, 1)
    return wav[0] if squeeze else wav


def unclipped_input():
    """a loud magnitude for ops.griffin_lim(post=GL_INV_PREEMPHASIS): the de-emphasised output exceeds 1 and is not clipped"""
    amp = GL.stft(harmonic(OPT_B, GL.HOP * (OPT_T - 1), seed=23).double() * 3).abs().float()
    return amp, draw_phases(tuple(amp.shape), 24)


# ---------------------------------------------------------------- C. final overlap-add: tile edges of the de-emphasis scan
OLA_N_FFT, OLA_WIN, OLA_B, OLA_TILE = 512, 400, 3, 16384
# (hop, T): L = hop (T - 1) = one below a tile, a tile, one above, two tiles and one, and one below half a tile
OLA_CASES = [(129, 128), (128, 129), (145, 114), (99, 332), (100, 50)]


def ola_input(hop, T):
    """-> magnitude (B, F, T) float32, phases (B, F, T) float32 numpy: a real signal's own spectrum (so that n_iter = 0 gives the
    signal back) plus a constant in the two lowest bins at phase 0: a large offset, whose de-emphasis decays slowly and is what
    the carry between tiles transports"""
    spec = GL.stft(harmonic(OLA_B, hop * (T - 1), seed=hop).double(), OLA_N_FFT, hop, OLA_WIN)
    amp, ph = spec.abs(), torch.angle(spec)
    amp[:, :2] += 20.0
    ph[:, :2] = 0.0
    return amp.float(), ph.float().numpy()


def deemph_serial_f32(x):
    """y[n] = x[n] + 0.97 y[n-1] along the last axis in plain float32 (two roundings per sample)"""
    x = np.asarray(x, np.float32)
    a = np.float32(0.97)
    y = np.zeros(x.shape[:-1], np.float32)
    out = np.empty_like(x)
    for n in range(x.shape[-1]):
        y = x[..., n] + a * y
        out[..., n] = y
    return out


def deemph_bound(x):
    """DEEMPH_SLACK times the max-abs error of the serial float32 recurrence on x (float32 values) against float64"""
    ref = GL.inv_preemphasis(np.asarray(x, np.float64))
    return DEEMPH_SLACK * float(np.abs(deemph_serial_f32(x).astype(np.float64) - ref).max()), ref


# ---------------------------------------------------------------- D. features
_FEAT_COMMON = dict(preemphasis_coeff=0.97, use_linear=True, snr_range=[10, 100], time_stretch_range=[0.9, 1.1])
FEAT_CONFIGS = {       # n_fft -> AudioConverter arguments; (n_fft, hop, win) = (512, 160, 400), (1024, 200, 800), (4096, 551, 2205)
    512: dict(num_freq=257, num_mels=40, frame_length_ms=25, frame_shift_ms=10, sample_rate=16000, **_FEAT_COMMON),
    1024: dict(num_freq=513, num_mels=80, frame_length_ms=50, frame_shift_ms=12.5, sample_rate=16000, **_FEAT_COMMON),
    4096: dict(num_freq=2049, num_mels=128, frame_length_ms=50, frame_shift_ms=12.5, sample_rate=44100, **_FEAT_COMMON),
}
FEAT_DIMS = {512: (512, 160, 400), 1024: (1024, 200, 800), 4096: (4096, 551, 2205)}
FEAT_RATES = (0.9, 1.0, 1.1)
FEAT_SNRS = (None, 15.0)


# The linear spectrogram's max-abs error is set by the bin of smallest magnitude (the dB scale divides by it), and float32 rounds the
# pre-emphasis relative to the tone, not to its much smaller difference.  Over the 0.002 floor of test_gpu_features._speech the
# float32 oracle drifts up to 7.7e-5 in linear (1.2e-5 in mel) at n_fft 4096, too close to a quarter of LIN_TOL to hold on another
# CPU; over this floor it stays at 3.0e-5 (3.5e-6) at all three sizes.
FEAT_FLOOR = 0.05


def feat_lens(n_fft):
    """a ragged batch of four, longest first: 3 n_fft + 17, two between, and the shortest legal n_fft / 2 + 1"""
    return [3 * n_fft + 17, 2 * n_fft + 2, n_fft + 131, n_fft // 2 + 1]


def feat_stretch_dims(n_fft, rate):
    c = FEAT_CONFIGS[n_fft]
    return FO.stretch_dims(rate, c['sample_rate'], c['frame_length_ms'], c['frame_shift_ms'])          # (win, hop)


def speech(L, seed, sr=FO.SR, floor=0.002):
    """test_gpu_features._speech: a harmonic tone with gated silences over a noise floor"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / sr
    f0 = 100 + 150 * rs.rand()
    x = sum(0.4 / (h + 1) * np.sin(2 * np.pi * f0 * (h + 1) * t + rs.rand()) for h in range(6))
    gate = (np.sin(2 * np.pi * 2 * t + 6 * rs.rand()) > -0.2)
    return (0.7 * x * gate + floor * rs.randn(L)).astype(np.float32)


def randn(L, seed):
    return np.random.RandomState(seed).randn(L).astype(np.float32)


def feat_batch(n_fft):
    """-> (wavs, noise): float32 numpy lists in the sorted (longest first) order"""
    lens = feat_lens(n_fft)
    return [speech(L, n_fft + i, floor=FEAT_FLOOR) for i, L in enumerate(lens)], [randn(L, 2 * n_fft + i) for i, L in enumerate(lens)]


def feat_reference(x, fb, n_fft, win=None, hop=None, noise=None, snr=None, dtype=torch.float64):
    """feat_oracle.features at a configuration's clean framing, or at (win, hop): -> (linear (F, T), mel (n_mels, T))"""
    _, h0, w0 = FEAT_DIMS[n_fft]
    return FO.features(x, fb, n_fft=n_fft, hop=h0 if hop is None else hop, win=w0 if win is None else win, noise=noise, snr=snr,
                       dtype=dtype)


# mixed batch (n_fft 512): SNRs in the sorted order; two utterances of n_fft / 2 + 1 samples so that one of them is noisy
MIXED_SNR = [12.0, None, 30.0, None]
MIXED_LENS = [1500, 900, 257, 257]

# the batch above FEATURES_MAX_BATCH = 64 (n_fft 512): 70 utterances of 1000 ... 310 samples, given longest first
BIG_B, BIG_SEED, BIG_SNR = 70, 99, 15.0
BIG_LENS = [1000 - 10 * u for u in range(BIG_B)]
BIG_CHECKED = (0, 1, 63, 64, 65, 69)
BIG_RATES = [FEAT_RATES[u % 3] for u in range(BIG_B)]

# ---------------------------------------------------------------- the noise generator
NOISE_N = 1048576 + 300          # past 4096 blocks of 256 threads: the grid-stride loop runs, the last 300 come from wrapped blocks
NOISE_STREAMS = [(0, 0), (3, 12345), (69, 2 ** 63 + 5)]                  # (utterance, seed)
NOISE_WINDOWS = [(0, 4096), (1048576 - 3946, 1048576 + 150), (NOISE_N - 4096, NOISE_N)]      # first, around the grid's end, last

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
PHILOX_KAT = [       # Random123's known answers for philox4x32-10: (counter, key, result)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two -> four uint32 arrays; ten rounds, the key bumped by the Weyl constants"""
    mask = np.uint64(0xffffffff)
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & mask for v in ctr]
    k = [np.atleast_1d(np.asarray(v, np.uint64)) & mask for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]              # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    return [v.astype(np.uint32) for v in c]


def feature_noise_ref(idx, utt, seed):
    """the standard normal of (seed, utterance, sample idx[...]) in float64 -> (values, u1 mantissas (r0 >> 8) + 1)"""
    idx = np.asarray(idx, np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    ctr = (idx & np.uint64(0xffffffff), idx >> np.uint64(32), np.full(idx.shape, utt, np.uint64), np.zeros(idx.shape, np.uint64))
    r = philox4x32_10(ctr, (seed & 0xffffffff, seed >> 32))
    m1 = (r[0] >> np.uint32(8)).astype(np.int64) + 1
    u1 = m1 / 16777216.0
    u2 = (r[1] >> np.uint32(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), m1
