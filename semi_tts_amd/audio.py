"""The reference's src/audio.py on the HIP kernels (semi_tts_amd/csrc/audio.hip, include/semitts.h).  Synthesis side: linear
spectrogram -> waveform by Griffin-Lim (st_griffin_lim_batch / st_stft_fwd / st_istft).

    conv = load_audio_transform(**config['data']['audio'])
    wav, sr = conv.feat_to_wave(linear_pred)          # (T, F) or (B, T, F), CPU or device tensor -> float64 numpy
    write_wav('utt-pred.wav', wav[0], sr)

feat_to_wave keeps to the linear branch of src/audio.py:397-407; the mel branch (the pseudo-inverse of :194-205, st_mel_to_linear)
is mel_to_wave, and a list of utterances of differing lengths is vocoded in one call by vocode_batch (st_griffin_lim_batch):

    wav, sr = conv.mel_to_wave(mel_pred)                # (T, n_mels) or (B, T, n_mels)
    wavs = conv.vocode_batch([np.load(f) for f in files], 'spec')      # [(T_i, F)] -> [hop * (T_i - 1) samples]

Analysis side (st_audio_features): waveform -> normalised mel / linear spectrograms and the augmented mel of the training loader.

    conv = load_audio_transform(**config['data']['audio'])
    msp, msp_aug, sp = conv.wave_to_feat('utt.wav')              # (T, n_mels), (T', n_mels), (T, F): src/audio.py:329-395
    mel, aug_mel, linear = conv.extract_batch(wavs, r=5)       # a ragged batch on the device, longest first (src/data.py:130)

Sample-rate conversion (st_resample_batch; not a step of the reference, whose load refuses a foreign rate): Hann-windowed sinc.

    wb = resample(wavs48k, 48000, 22050)                         # list of 1-D float / int16 waveforms -> WaveBatch on the device
    wb = conv.load_batch(paths, resample=True)                   # .wav files of any rate -> one WaveBatch at conv.sr
    mel, aug_mel, linear = conv.extract_batch(wb, r=5)

MFCC and phone segments (st_audio_mfcc, st_segment_gather; src/audio.py:94-154, 309-354):

    mfcc = conv.extract_mfcc_from_waveform(wave)                  # (39, T): 13 cepstra, their first and second derivatives
    mfcc = conv.extract_mfcc_batch(wavs)                          # device (B, T_pad, 39), longest first
    conv = load_audio_transform(**config['data']['audio'], segment_file='segments.csv', segment_feat='mfcc')
    seg = conv.segment_features('utt.wav')                        # (S, max_len, 39): the utterance cut at its phone boundaries
    seg, counts = conv.segment_batch(mfcc, frames, keys)          # a whole batch in one launch: (S_total, max_len, 39)
"""
import csv
import math
import random
import wave

import numpy as np
import torch

from . import toolops
from .ctc_align import segment_key      # a file's key in a segment table: its name up to the first '.' (src/audio.py:342)

GFL_ITER = 30                     # src/audio.py:15
MIN_LEVEL_DB = -100               # src/audio.py:17
REF_LEVEL_DB = 20                 # src/audio.py:18
INV_PREEMPHASIS_COEFF = 0.97      # the literal of src/audio.py:276 (_inv_preemphasis ignores preemphasis_coeff)
SUPPORTED_N_FFT = (512, 1024, 2048, 4096)
SNR_OFF = float('nan')            # extract_batch(snr=SNR_OFF): no noise (the reference's -1 in snr_range)
MFCC_HOP_LEN_MS, MFCC_WIN_LEN_MS, N_MFCC_NO_DELTA = 10, 25, 13      # src/audio.py:19-21
MFCC_DIM = 3 * N_MFCC_NO_DELTA    # cepstra + first and second derivatives (the reference's literal 39, :317)
SEGMENT_FEAT_KINDS = ('mfcc', 'mel', 'linear')
# librosa.feature.delta's 9-frame Savitzky-Golay filters in ascending frame order: order 1 (polyorder 1) and order 2 (polyorder 2)
MFCC_DELTA_TAPS = tuple(j / 60.0 for j in range(-4, 5))
MFCC_DELTA2_TAPS = tuple(v / 462.0 for v in (28, 7, -8, -17, -20, -17, -8, 7, 28))

# the shipped configs' data.audio (identical in all three YAMLs): num_freq 1025, 12.5 / 50 ms at 22050 Hz
DEFAULT_N_FFT, DEFAULT_HOP, DEFAULT_WIN = 2048, 275, 1102


def stft_dims(num_freq, frame_shift_ms, frame_length_ms, sample_rate):
    """(n_fft, hop, win) exactly as AudioProcessor.__init__ derives them (src/audio.py:28-32)"""
    return (num_freq - 1) * 2, int(frame_shift_ms / 1000 * sample_rate), int(frame_length_ms / 1000 * sample_rate)


def check_dims(n_fft, hop, win, T):
    """raise ValueError for what the kernels do not take, before anything touches a device"""
    if n_fft not in SUPPORTED_N_FFT:
        raise ValueError('Griffin-Lim: n_fft %d not supported (one of %s)' % (n_fft, SUPPORTED_N_FFT))
    if not (0 < 2 * hop <= win <= n_fft):
        raise ValueError('Griffin-Lim: need 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)' % (hop, win, n_fft))
    if hop * (T - 1) <= n_fft // 2:
        # torch.stft's reflect padding of n_fft // 2 needs a longer signal than the hop * (T - 1) samples the iSTFT gives
        raise ValueError('Griffin-Lim: %d frames are too few: reflect padding needs hop * (T - 1) > n_fft // 2 (hop %d, n_fft %d), '
                         'i.e. T >= %d' % (T, hop, n_fft, n_fft // 2 // hop + 2))


def mfcc_dims(sample_rate):
    """(win, hop) of the MFCC framing exactly as AudioProcessor.__init__ derives them (src/audio.py:33-34)"""
    return int(MFCC_WIN_LEN_MS / 1000 * sample_rate), int(MFCC_HOP_LEN_MS / 1000 * sample_rate)


def mfcc_dct(n_mfcc, n_mels):
    """(n_mfcc, n_mels) float64: the first rows of the orthonormal DCT-II over the mel axis (scipy.fftpack.dct(type=2, norm='ortho'),
    what librosa.feature.mfcc applies): sqrt(2 / M) cos(pi (2 m + 1) k / (2 M)), row 0 divided by sqrt(2).  The kernel takes it
    rounded once to float32."""
    k, m = np.arange(n_mfcc, dtype=np.float64)[:, None], np.arange(n_mels, dtype=np.float64)[None, :]
    d = np.sqrt(2.0 / n_mels) * np.cos(np.pi * (2.0 * m + 1.0) * k / (2.0 * n_mels))
    d[0] /= np.sqrt(2.0)
    return d


def clamped_filter(c, taps):
    """c (..., T) float64, T >= len(taps) -> the filter `taps` (ascending frame order, odd length 2 h + 1) along the last axis with
    its centre clamped into [h, T - 1 - h]: y[t] = sum_j taps[j] c[min(max(t, h), T - 1 - h) + j - h].  With MFCC_DELTA_TAPS /
    MFCC_DELTA2_TAPS this is scipy.signal.savgol_filter(c, 9, deriv=o, polyorder=o, mode='interp'); the host
    statement of what mfcc_delta_kernel computes."""
    c = np.asarray(c, np.float64)
    h, T = len(taps) // 2, c.shape[-1]
    if T < len(taps):
        raise ValueError('clamped_filter: %d frames, the filter has %d taps' % (T, len(taps)))
    tc = np.clip(np.arange(T), h, T - 1 - h)
    return sum(w * c[..., tc + j - h] for j, w in enumerate(taps))


def compute_len_ratio(seg):
    """'t1_t2_..._tlast' -> [t / tlast]: a row's boundary times as ratios of the utterance (src/audio.py:425-432)"""
    times = [float(t) for t in seg.split('_')]
    return [t / times[-1] for t in times]


def read_segment_table(path):
    """a segment_file (header `file,seg`, one row per utterance: key, boundary times joined by '_'; what --align-wav-dir writes as
    segments.csv) -> {key: boundary ratios}.  A missing column, a malformed row or a duplicate key raises ValueError naming the file."""
    table = {}
    with open(path, newline='') as f:
        rows = csv.reader(f)
        header = next(rows, None)
        if header is None or [h.strip() for h in header] != ['file', 'seg']:
            raise ValueError('%s: a segment file starts with the header file,seg (got %r)' % (path, header))
        for n, row in enumerate(rows, 2):
            if not row:
                continue
            try:
                key, ratios = row[0], compute_len_ratio(row[1])
                if len(row) != 2 or not all(np.isfinite(ratios)):
                    raise ValueError
            except (IndexError, ValueError, ZeroDivisionError):
                raise ValueError('%s, line %d: expected `key,t1_t2_..._tlast` with a last time above 0, got %r' % (path, n, row))
            if key in table:
                raise ValueError('%s, line %d: the key %r appears twice' % (path, n, key))
            table[key] = ratios
    return table


def segment_points(boundary, feat_len, min_segment_len=2):
    """Where a feature of feat_len frames is cut (the rule of AudioProcessor.segment, src/audio.py:94-117): every boundary ratio b
    gives the frame round(b * feat_len) -- Python's round, halves to even.  The piece from the end of the last emitted piece to that
    frame is emitted when it holds at least min_segment_len frames; a shorter one is not, and its frames go to the next piece.
    -> ([(start, end)], max_len), max_len the longest candidate piece seen (emitted or not): the padded length of the segments."""
    pieces, start, max_len = [], 0, 0
    for b in boundary:
        end = round(b * feat_len)
        max_len = max(max_len, end - start)
        if end - start >= min_segment_len:
            pieces.append((start, end))
            start = end
    return pieces, max_len


def min_frames(n_fft, hop):
    """the fewest frames check_dims takes: hop * (T - 1) > n_fft // 2"""
    return n_fft // 2 // hop + 2


def check_frames(frames, B, n_fft, hop, T):
    """per-utterance frame counts of a ragged batch -> int32 array (B,); raises ValueError unless they are B integers in
    [min_frames, T] (check_dims' "too few" rule for every utterance)"""
    arr = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)
    if arr.shape != (B,) or not (np.issubdtype(arr.dtype, np.integer) or (arr.dtype.kind == 'f' and np.all(arr == np.floor(arr)))):
        raise ValueError('Griffin-Lim: frames must be %d integers (one per utterance), got %s of shape %s'
                         % (B, arr.dtype, arr.shape))
    lo = min_frames(n_fft, hop)
    for b, n in enumerate(arr.tolist()):
        if n < lo:
            raise ValueError('Griffin-Lim: utterance %d: %d frames are too few: reflect padding needs hop * (T - 1) > n_fft // 2 '
                             '(hop %d, n_fft %d), i.e. T >= %d' % (b, n, hop, n_fft, lo))
        if n > T:
            raise ValueError('Griffin-Lim: utterance %d: %d frames, the batch holds %d' % (b, n, T))
    return arr.astype(np.int32)


def draw_phases(shape):
    """initial phases as src/audio.py:214-216: uniform in [0, 2 pi) from np.random, wrapped by np.angle(np.exp(1j phi)), float32"""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('semi_tts_amd.audio: Griffin-Lim runs on the HIP kernels and needs a GPU; there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _run(feat_btf, phases, n_fft, hop, win, n_iter, normalized, power, post, basis=None, frames=None):
    """feat_btf: (B, T, F) view, any strides -- or (B, T, n_mels) with `basis`, a callable device -> (n_mels, F) tensor, called
    once every check has passed; phases: (B, F, T) array/tensor or None (drawn); frames: per-utterance frame counts or None.
    -> (B, hop * (T - 1)) device tensor.  Every refusal is raised before a device is touched."""
    B, T, D = feat_btf.shape
    F = n_fft // 2 + 1
    if basis is None and D != F:
        raise ValueError('Griffin-Lim: %d frequency bins, expected n_fft // 2 + 1 = %d' % (D, F))
    if basis is not None and power != 1.0:
        raise ValueError('Griffin-Lim: mel input is an amplitude (the reference\'s isAmp branch): power must be 1, got %g' % power)
    check_dims(n_fft, hop, win, T)
    if frames is not None:
        frames = check_frames(frames, B, n_fft, hop, T)
    if phases is None:
        phases = draw_phases((B, F, T))
    phases = torch.as_tensor(phases, dtype=torch.float32)
    if tuple(phases.shape) != (B, F, T):
        raise ValueError('Griffin-Lim: phases of shape %s, expected %s' % (tuple(phases.shape), (B, F, T)))
    dev = feat_btf.device if feat_btf.is_cuda else _device()
    feat_btf = feat_btf.to(dev, torch.float32)
    return toolops.griffin_lim_batch(feat_btf, phases.to(dev).contiguous(), n_fft, hop, win, n_iter=n_iter, normalized=normalized,
                                     power=power, post=post, basis=None if basis is None else basis(dev),
                                     frames=None if frames is None else torch.from_numpy(frames).to(dev))


def griffin_lim(amp, phases=None, n_iter=GFL_ITER, n_fft=DEFAULT_N_FFT, hop=DEFAULT_HOP, win=DEFAULT_WIN):
    """AudioProcessor._griffin_lim (src/audio.py:208-226) on the device: magnitude (F, T) or (B, F, T) -> waveform (L,) or (B, L),
    L = hop * (T - 1), before inverse pre-emphasis.  phases: the initial phases, shaped like amp (None: drawn from np.random)."""
    squeeze = amp.dim() == 2
    a = amp.unsqueeze(0) if squeeze else amp
    if phases is not None and squeeze:
        phases = torch.as_tensor(phases).unsqueeze(0)
    wav = _run(a.transpose(1, 2), phases, n_fft, hop, win, n_iter, normalized=False, power=1.0, post=0)
    return wav[0] if squeeze else wav


class AudioConverter:
    """The reference's AudioProcessor / AudioConverter (src/audio.py:23, :292): feature extraction (clean and augmented) and
    the synthesis methods for the linear branch."""

    def __init__(self, num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear=True,
                 snr_range=(-1, -1), time_stretch_range=(1.0, 1.0), segment_file=None, segment_feat=None, min_segment_len=2, **_unused):
        self.n_fft, self.hop_length, self.win_length = stft_dims(num_freq, frame_shift_ms, frame_length_ms, sample_rate)
        self.win_length_mfcc, self.hop_length_mfcc = mfcc_dims(sample_rate)
        self._dct = {}
        self.frame_length_ms, self.frame_shift_ms = frame_length_ms, frame_shift_ms
        self.snr_range, self.time_stretch_range = list(snr_range), list(time_stretch_range)
        self._fb = {}
        self._basis = {}
        self.num_freq, self.n_mels = num_freq, num_mels
        self.preemphasis_coeff = preemphasis_coeff       # read by the reference's _preemphasis only, never by the inverse (:274-276)
        self.sr = sample_rate
        self.use_linear = use_linear
        self.feat_dim = (num_mels, num_freq) if use_linear else (num_mels, None)      # src/audio.py:307
        self.use_segment = segment_file is not None                                   # src/audio.py:309-327
        if self.use_segment:
            self.segment_src = segment_file
            self.segment_feat = str(segment_feat).lower()
            self.min_segment_len = min_segment_len
            if self.segment_feat not in SEGMENT_FEAT_KINDS:
                raise NotImplementedError('segment_feat %r: one of %s' % (segment_feat, ', '.join(SEGMENT_FEAT_KINDS)))
            self.seg_feat_dim = {'mfcc': MFCC_DIM, 'mel': num_mels, 'linear': num_freq}[self.segment_feat]
            self.boundary_table = read_segment_table(segment_file)

    def specgram_to_waveform(self, specgram, power=1.0, inv_preemphasis=True, isAmp=False, phases=None, n_iter=GFL_ITER):
        """src/audio.py:179-192: specgram (F, T) or (B, F, T) -> float64 numpy waveform(s), clipped to [-1, 1].
        Denormalisation, Griffin-Lim, inverse pre-emphasis and clip all run on the device."""
        squeeze = specgram.dim() == 2
        s = specgram.unsqueeze(0) if squeeze else specgram
        if phases is not None and squeeze:
            phases = torch.as_tensor(phases).unsqueeze(0)
        post = toolops.GL_CLIP | (toolops.GL_INV_PREEMPHASIS if inv_preemphasis else 0)
        wav = _run(s.transpose(1, 2), phases, self.n_fft, self.hop_length, self.win_length, n_iter, normalized=not isAmp,
                   power=power, post=post)
        wav = wav.cpu().numpy().astype(np.float64)
        return wav[0] if squeeze else wav

    def feat_to_wave(self, feat, phases=None):
        """src/audio.py:397-407: the decoder's (T, F) or (B, T, F) linear output -> (float64 waveform(s), sample rate).
        The reference transposes to (F, T) and draws its phases in that shape; here the first kernel reads (B, T, F) directly.
        Mel-sized input is refused here; mel_to_wave is the reference's mel branch."""
        if feat.size(-1) == self.feat_dim[0] and feat.size(-1) != self.num_freq:
            raise NotImplementedError('feat_to_wave: mel input (%d bins): the mel -> linear pseudo-inverse of src/audio.py:194-205 '
                                      "needs librosa's filterbank and is not implemented; pass the linear spectrogram" % feat.size(-1))
        return self.specgram_to_waveform(feat.transpose(-2, -1), phases=phases), self.sr

    def mel_basis(self, device=None):
        """mel_basis(sr, n_fft, n_mels) of this converter, computed once: the float32 numpy array (device None) or its copy on
        `device`, cached per device like filterbank.  Raises ValueError for a rank-deficient bank."""
        if None not in self._basis:
            self._basis[None] = mel_basis(self.sr, self.n_fft, self.n_mels)
        if device is None:
            return self._basis[None]
        key = str(device)
        if key not in self._basis:
            self._basis[key] = torch.from_numpy(self._basis[None]).to(device)
        return self._basis[key]

    def _check_mel(self, width):
        if width != self.n_mels:
            raise ValueError('mel vocoding: %d mel bins, expected num_mels = %d' % (width, self.n_mels))
        if self.n_fft not in SUPPORTED_N_FFT:
            raise ValueError('mel vocoding: n_fft %d not supported (one of %s)' % (self.n_fft, SUPPORTED_N_FFT))
        if not 1 <= self.n_mels <= toolops.MEL_MAX:
            raise ValueError('mel vocoding: %d mels outside [1, %d]' % (self.n_mels, toolops.MEL_MAX))
        self.mel_basis()                                 # (a rank-deficient bank raises here, on the host)

    def melspecgram_to_specgram(self, melspecgram):
        """src/audio.py:194-205: normalised mel (n_mels, T) or (B, n_mels, T) -> the signed amplitude spectrogram (F, T) /
        (B, F, T) = pinverse(fb).T @ db_to_amp(denormalize(mel) + REF_LEVEL_DB), on the device"""
        squeeze = melspecgram.dim() == 2
        m = melspecgram.unsqueeze(0) if squeeze else melspecgram
        self._check_mel(m.size(1))
        dev = m.device if m.is_cuda else _device()
        lin = toolops.mel_to_linear(m.to(dev, torch.float32).transpose(1, 2), self.mel_basis(dev), normalized=True, take_abs=False)
        lin = lin.transpose(1, 2)
        return lin[0] if squeeze else lin

    def mel_to_wave(self, mel, phases=None, frames=None):
        """The mel branch of src/audio.py:397-407: the decoder's (T, n_mels) or (B, T, n_mels) mel output -> (float64 waveform(s),
        sample rate).  phases: (F, T) / (B, F, T) as the reference draws them; frames: per-utterance frame counts of a padded batch
        (row b is then zero beyond hop * (frames[b] - 1) samples).  Product, Griffin-Lim, inverse pre-emphasis and clip on the device."""
        squeeze = mel.dim() == 2
        m = mel.unsqueeze(0) if squeeze else mel
        if phases is not None and squeeze:
            phases = torch.as_tensor(phases).unsqueeze(0)
        wav = self.gen_wav_device(m, phases, frames=frames, mel=True).cpu().numpy().astype(np.float64)
        return (wav[0] if squeeze else wav), self.sr

    def vocode_batch(self, feats, kind='spec', loudness=None):
        """Utterances of differing lengths in one st_griffin_lim_batch call (the file loop of the reference's
        util/gen_wav_from_specgram.py as one batch): feats, a list of (T_i, D) normalised spectrograms, D = num_freq for kind 'spec'
        or num_mels for 'mel' -> list of float64 waveforms of hop * (T_i - 1) samples, in the given order.  The initial phases are
        drawn per utterance in that order as draw_phases((F, T_i)): one np.random seed gives the reference loop's phases.
        loudness: a dict of loudness_batch's arguments; each waveform is then normalised on the device before the copy to the host."""
        if kind not in ('spec', 'mel'):
            raise ValueError("vocode_batch: kind %r is neither 'spec' nor 'mel'" % (kind,))
        feats = [torch.as_tensor(f) for f in feats]
        if not feats:
            raise ValueError('vocode_batch: an empty batch')
        D = self.num_freq if kind == 'spec' else self.n_mels
        for i, f in enumerate(feats):
            if f.dim() != 2 or f.size(1) != D:
                raise ValueError('vocode_batch: utterance %d has shape %s, expected (T, %d) for kind %r' % (i, tuple(f.shape), D, kind))
        if kind == 'mel':
            self._check_mel(D)
        F = self.n_fft // 2 + 1
        lens = [int(f.size(0)) for f in feats]
        B, T = len(feats), max(lens)
        check_dims(self.n_fft, self.hop_length, self.win_length, T)
        check_frames(lens, B, self.n_fft, self.hop_length, T)
        phases = np.zeros((B, F, T), np.float32)
        for b, n in enumerate(lens):
            phases[b, :, :n] = draw_phases((F, n))
        dev = feats[0].device if feats[0].is_cuda else _device()
        batch = torch.zeros(B, T, D, device=dev, dtype=torch.float32)
        for b, f in enumerate(feats):
            batch[b, :lens[b]] = f.to(dev, torch.float32)
        wav = self.gen_wav_device(batch, phases, frames=lens, mel=kind == 'mel')
        if loudness is not None:
            self.normalize_rows(wav, [self.hop_length * (n - 1) for n in lens], **loudness)
        wav = wav.cpu().numpy().astype(np.float64)
        return [wav[b, :self.hop_length * (n - 1)] for b, n in enumerate(lens)]

    # -- analysis side (src/audio.py:68-77, 156-177, 329-395)
    def load(self, wav_path):
        """src/audio.py:68-77: (channels, samples) float32; a different sample rate raises"""
        return load_wav(wav_path, self.sr)

    def load_batch(self, paths, resample=False, trim=None, loudness=None):
        """Channel 0 of the .wav files `paths` as one WaveBatch at self.sr on the device (`.order`: the position in `paths` of each
        utterance).  A file at another rate raises load()'s error -- or, with resample=True, is converted on the GPU: the files are
        grouped by source rate and each foreign group is uploaded as int16 PCM and resampled in one resample() call.  Every file
        is read and every rate checked before a device is touched.  trim: a dict of trim_batch's keyword arguments (top_db,
        frame_length, hop_length, pad_ms); the leading and trailing silence of every utterance is then cut, after resampling (`.bounds`:
        the kept (start, end) of each file, in the order of `paths`).  loudness: a dict of loudness_batch's keyword arguments (target,
        peak_db, max_gain_db); every utterance is then metered and, with a target, normalised in place -- after resampling and
        trimming, so the meter sees the kept span (`.loudness`: loudness_batch's dict, in the order of `paths`)."""
        paths = [str(p) for p in paths]
        if not paths:
            raise ValueError('load_batch: no files')
        if trim is not None:
            self._check_trim(**trim)
        if loudness is not None:
            self._check_loudness(**loudness)
        read = [_read_pcm(p) for p in paths]
        groups = {}
        for i, ((_, sr), p) in enumerate(zip(read, paths)):
            if sr != self.sr:
                if not resample:
                    raise ValueError('Sample rate mismatch. Expected %d but get %d (%s)' % (self.sr, sr, p))
                resample_table(sr, self.sr)                       # (a ratio the kernel does not take raises here)
                groups.setdefault(sr, []).append(i)
        dev = _device()
        waves = [None] * len(paths)
        for i, (pcm, sr) in enumerate(read):
            if sr == self.sr:
                waves[i] = torch.from_numpy(pcm[:, 0].astype(np.float32) / 32768.0).to(dev)
        for sr, idx in sorted(groups.items()):
            wb = _resample([torch.from_numpy(read[i][0][:, 0].copy()) for i in idx], sr, self.sr)
            y = wb.packed(dev)
            for row, k in enumerate(wb.order):
                waves[idx[k]] = y[int(wb.offsets[row]):int(wb.offsets[row] + wb.lens[row])]
        if trim is None:
            wb = WaveBatch(waves)
        else:
            res = self.trim_batch(waves, **trim)
            wb = res[0]
            wb.bounds = res[1]
        if loudness is not None:
            rows = np.asarray(wb.order)
            res = self.loudness_batch(wb, **loudness)
            info, out = res if isinstance(res, tuple) else (res, wb)
            out.order = rows
            if trim is not None:
                out.bounds = wb.bounds
            out.loudness = {}
            for k, v in info.items():                              # row i of the batch is file rows[i]
                out.loudness[k] = np.empty_like(v)
                out.loudness[k][rows] = v
            wb = out
        return wb

    # -- loudness (not a step of the reference): st_loudness_batch, ITU-R BS.1770-4 / EBU R 128 integrated loudness
    def _check_loudness(self, target=None, peak_db=-1.0, max_gain_db=30.0, lens=(1,)):
        """every refusal of loudness_batch that does not need the waveforms"""
        lens = np.asarray(lens, np.int64)
        toolops._loudness_check(lens[:toolops.FEATURES_MAX_BATCH], self.sr, target, peak_db, max_gain_db)
        if (lens < 1).any() or (lens >= 2 ** 31).any():
            raise ValueError('loudness: every length must lie in [1, 2^31)')

    def normalize_rows(self, wav, lens=None, target=None, peak_db=-1.0, max_gain_db=30.0):
        """The rows of a contiguous (B, N) float32 device tensor of waveforms (what gen_wav_device returns), row b its first lens[b]
        samples (None: all N), metered and multiplied by their gains IN PLACE on the device: no host read.  Rows of no samples and
        flagged rows (non-finite, under 400 ms, silent) keep their level.  -> wav"""
        if not (torch.is_tensor(wav) and wav.is_cuda and wav.dim() == 2 and wav.dtype == torch.float32 and wav.is_contiguous()):
            raise ValueError('normalize_rows: a contiguous (B, N) float32 device tensor is needed')
        B, N = wav.shape
        lens = np.full(B, N, np.int64) if lens is None else np.asarray(lens, np.int64)
        if lens.shape != (B,) or (lens > N).any():
            raise ValueError('normalize_rows: lens must be %d lengths of at most %d samples' % (B, N))
        rows = np.flatnonzero(lens >= 1)
        if target is None or len(rows) == 0:
            return wav
        self._check_loudness(target, peak_db, max_gain_db, lens=lens[rows])
        x = wav.view(-1)
        for b0 in range(0, len(rows), toolops.FEATURES_MAX_BATCH):
            r = rows[b0:b0 + toolops.FEATURES_MAX_BATCH]
            _, stats, _ = toolops.loudness(x, r * N, lens[r], self.sr, target, peak_db, max_gain_db)
            toolops.wave_gain(x, r * N, lens[r], stats, out=x)
        return wav

    def loudness_batch(self, wavs, target=None, peak_db=-1.0, max_gain_db=30.0):
        """Integrated loudness (ITU-R BS.1770-4, mono) of a ragged batch on the device, one st_loudness_batch call per 64 utterances and
        ONE host read: wavs, a list of 1-D waveforms or a WaveBatch.  -> a dict of host arrays, entry i for utterance i of `wavs` (a
        list's position; a WaveBatch's row): lufs, momentary_max, rel_gate, peak (linear), ungated, gain_db (float64) and n_blocks, n_abs,
        n_rel, flags (int64; toolops.LOUDNESS_FLAGS).  With a target (LUFS) the utterances are also multiplied by the gain that brings them
        to it, limited so that the sample peak stays at or under peak_db dBFS and the gain at or under max_gain_db -- flagged
        utterances (non-finite, shorter than 400 ms, silent) keep their level -- and (dict, WaveBatch) is returned: the normalised
        batch with the input's rows, offsets and lens.  A WaveBatch is normalised IN PLACE in its packed buffer; a list is not touched."""
        wb = wavs if isinstance(wavs, WaveBatch) else WaveBatch(wavs)
        self._check_loudness(target, peak_db, max_gain_db, lens=wb.lens)
        dev = wb.device if wb.device is not None else _device()
        B = len(wb.lens)
        x = wb.packed(dev)
        parts = []
        for b0 in range(0, B, toolops.FEATURES_MAX_BATCH):
            sl = slice(b0, min(B, b0 + toolops.FEATURES_MAX_BATCH))
            _, stats, counts = toolops.loudness(x, wb.offsets[sl], wb.lens[sl], self.sr, target, peak_db, max_gain_db)
            if target is not None:
                toolops.wave_gain(x, wb.offsets[sl], wb.lens[sl], stats, out=x)
            parts.append((stats, counts))
        host = torch.cat([p[0].reshape(-1).view(torch.int32) for p in parts] + [p[1].reshape(-1) for p in parts]).cpu().numpy()
        stats = host[:8 * B].view(np.float32).reshape(B, 8).astype(np.float64)
        counts = host[8 * B:].reshape(B, 4).astype(np.int64)
        given = isinstance(wavs, WaveBatch)
        inv = np.arange(B) if given else wb.inverse()                       # row of wb of utterance i of a list
        with np.errstate(divide='ignore'):
            info = dict(lufs=stats[inv, 0], momentary_max=stats[inv, 1], rel_gate=stats[inv, 2], peak=stats[inv, 3], ungated=stats[inv, 4],
                        gain_db=20.0 * np.log10(stats[inv, 5]), n_blocks=counts[inv, 0], n_abs=counts[inv, 1], n_rel=counts[inv, 2],
                        flags=counts[inv, 3])
        if target is None:
            return info
        out = WaveBatch.window(x, wb.offsets, wb.lens)
        out.order = np.asarray(wb.order)
        return info, out

    # -- silence trimming (not a step of the reference): st_trim_silence, the definition of librosa.effects.trim / split
    def _check_trim(self, top_db=60., frame_length=2048, hop_length=512, pad_ms=0., with_intervals=False, lens=(1,)):
        """every refusal of trim_batch that does not need the waveforms -> pad in samples"""
        if isinstance(pad_ms, bool) or not isinstance(pad_ms, (int, float, np.integer, np.floating)) or not 0.0 <= pad_ms < float('inf'):
            raise ValueError('trim: pad_ms must be a finite number >= 0 (got %r)' % (pad_ms,))
        pad = int(round(float(pad_ms) / 1000.0 * self.sr))
        toolops._trim_check(np.asarray(lens, np.int64), frame_length, hop_length, top_db, pad, 0)
        return pad

    def trim_batch(self, wavs, top_db=60., frame_length=2048, hop_length=512, pad_ms=0., with_intervals=False):
        """Leading and trailing silence of a ragged batch cut on the device (one st_trim_silence call per 64 utterances, ONE host read):
        wavs, a list of 1-D waveforms or a WaveBatch.  A frame of frame_length samples every hop_length is non-silent when its mean
        square lies less than top_db dB under the loudest frame's; the kept span runs from the first to the last non-silent frame,
        widened by pad_ms milliseconds on both sides.  -> (WaveBatch, bounds, n_short[, intervals]):
            WaveBatch   the trimmed utterances INSIDE the packed buffer of the input (nothing is copied: moved offsets, shorter lens),
                        sorted longest first again (stable), `.order[i]` the position in the caller's list of the i-th utterance
            bounds      host int64 (B, 2): the kept samples [start, end) of utterance i of `wavs` (a list's position; a WaveBatch's row)
            n_short     utterances whose kept span would hold n_fft // 2 samples or fewer -- the feature kernels refuse those --
                        and are therefore returned untrimmed
            intervals   (with_intervals) per utterance of `wavs`, an int64 (n, 2) array of its non-silent intervals in samples (no pad),
                        what librosa.effects.split returns
        An utterance with a non-finite sample is returned whole."""
        wb = wavs if isinstance(wavs, WaveBatch) else WaveBatch(wavs)
        pad = self._check_trim(top_db, frame_length, hop_length, pad_ms, lens=wb.lens)
        dev = wb.device if wb.device is not None else _device()
        B = len(wb.lens)
        max_iv = (2 + int(wb.lens.max()) // hop_length) // 2 if with_intervals else 0      # runs of T frames: at most ceil(T / 2)
        x = wb.packed(dev)
        _, bounds, iv, n_iv = toolops.trim_silence(x, wb.offsets, wb.lens, frame_length, hop_length, top_db, pad=pad, max_iv=max_iv)
        if with_intervals:
            host = torch.cat([bounds.reshape(-1), n_iv, iv.reshape(-1)]).cpu().numpy().astype(np.int64)
            n_iv, iv = host[4 * B:5 * B], host[5 * B:].reshape(B, max_iv, 2)
        else:
            host = bounds.cpu().numpy().astype(np.int64).reshape(-1)
        start, end = host[0:4 * B:4].copy(), host[1:4 * B:4].copy()
        short = end - start <= self.n_fft // 2
        start[short], end[short] = 0, wb.lens[short]
        rows = np.argsort(-(end - start), kind='stable')
        out = WaveBatch.window(x, (wb.offsets + start)[rows], (end - start)[rows])
        out.order = np.asarray(wb.order)[rows]
        given = isinstance(wavs, WaveBatch)
        inv = np.arange(B) if given else wb.inverse()                       # row of wb of utterance i of a list
        res = (out, np.stack([start, end], 1)[inv], int(short.sum()))
        if with_intervals:
            res += ([iv[r, :n_iv[r]].copy() for r in inv],)
        return res

    def nonsilent_intervals(self, waveform, top_db=60., frame_length=2048, hop_length=512, channel=0):
        """librosa.effects.split for one utterance: waveform (channels, samples) or (samples,) -> int64 (n, 2), the non-silent
        intervals [start, end) of `channel` in samples (computed on the GPU)"""
        x = torch.as_tensor(waveform)
        x = x[channel] if x.dim() == 2 else x
        return self.trim_batch([x], top_db, frame_length, hop_length, with_intervals=True)[3][0]

    def stretch_dims(self, rate):
        """(win, hop) of the augmented framing at stretch `rate`, exactly as src/audio.py:366-373"""
        stretch_sr = int(self.sr * rate)
        return int(self.frame_length_ms / 1000 * stretch_sr), int(self.frame_shift_ms / 1000 * stretch_sr)

    def filterbank(self, device):
        """the mel filterbank as the kernel takes it, cached per device: (start bin, count, offset) per mel + packed weights"""
        key = str(device)
        if key not in self._fb:
            start, cnt, off, w = band_pack(mel_filterbank(self.sr, self.n_fft, self.n_mels))
            self._fb[key] = tuple(torch.from_numpy(a).to(device) for a in (start, cnt, off, w))
        return self._fb[key]

    def _check(self, lens, aug_dims=()):
        """every refusal of st_audio_features, raised before any device is touched"""
        if self.n_fft not in SUPPORTED_N_FFT:
            raise ValueError('features: n_fft %d not supported (one of %s)' % (self.n_fft, SUPPORTED_N_FFT))
        for win, hop, what in [(self.win_length, self.hop_length, 'clean')] + [(w, h, 'augmented') for w, h in aug_dims]:
            if not (0 < 2 * hop <= win <= self.n_fft):
                raise ValueError('features: the %s framing needs 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)'
                                 % (what, hop, win, self.n_fft))
        for L in lens:
            if L <= self.n_fft // 2:
                raise ValueError('features: an utterance of %d samples is too short: reflect padding needs more than n_fft // 2 = %d'
                                 % (L, self.n_fft // 2))

    def extract_feature_from_waveform(self, waveform, preemphasis=True, channel=0):
        """src/audio.py:156-177: waveform (channels, samples) -> (specgram (F, T), melspecgram (n_mels, T)) of `channel`, normalised,
        on the waveform's device (computed on the GPU either way)"""
        x = torch.as_tensor(waveform)
        x = x[channel] if x.dim() == 2 else x
        self._check([x.shape[-1]])
        dev = x.device if x.is_cuda else _device()
        xd = x.to(dev, torch.float32).contiguous()
        T = 1 + xd.numel() // self.hop_length
        mel, lin, _ = toolops.audio_features(xd, [0], [xd.numel()], self.n_fft, self.win_length, self.hop_length,
                                             self.preemphasis_coeff if preemphasis else 0.0, self.filterbank(dev), T)
        return lin[0].t().to(x.device), mel[0].t().to(x.device)

    # -- MFCC (src/audio.py:119-154) and phone segments (:94-117, :339-354)
    def mfcc_table(self, device):
        """the (13, n_mels) DCT table as the kernel takes it (mfcc_dct rounded once to float32), cached per device"""
        key = str(device)
        if key not in self._dct:
            self._dct[key] = torch.from_numpy(mfcc_dct(N_MFCC_NO_DELTA, self.n_mels).astype(np.float32)).to(device)
        return self._dct[key]

    def _check_mfcc(self, lens):
        """every refusal of st_audio_mfcc, raised before any device is touched"""
        win, hop = self.win_length_mfcc, self.hop_length_mfcc
        if self.n_fft not in SUPPORTED_N_FFT:
            raise ValueError('mfcc: n_fft %d not supported (one of %s)' % (self.n_fft, SUPPORTED_N_FFT))
        if not (0 < 2 * hop <= win <= self.n_fft):
            raise ValueError('mfcc: the MFCC framing needs 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)' % (hop, win, self.n_fft))
        if not N_MFCC_NO_DELTA <= self.n_mels <= toolops.MEL_MAX:
            raise ValueError('mfcc: %d mels outside [%d, %d]' % (self.n_mels, N_MFCC_NO_DELTA, toolops.MEL_MAX))
        for L in lens:
            if L <= self.n_fft // 2 or L >= 2 ** 30:
                raise ValueError('mfcc: an utterance of %d samples: reflect padding needs more than n_fft // 2 = %d (and fewer than 2^30)'
                                 % (L, self.n_fft // 2))
            if 1 + L // hop < toolops.MFCC_MIN_FRAMES:
                raise ValueError('mfcc: an utterance of %d samples has fewer than 9 MFCC frames (%d at hop %d): the 9-frame derivatives '
                                 'need at least %d samples' % (L, 1 + L // hop, hop, (toolops.MFCC_MIN_FRAMES - 1) * hop))

    def extract_mfcc_batch(self, wavs, preemphasis=True, with_mel=False):
        """extract_mfcc_from_waveform for a ragged batch in one st_audio_mfcc call: wavs, a list of 1-D waveforms (or a WaveBatch),
        sorted longest first -> device (B, T_pad, 39), T_pad the longest utterance's 1 + L // hop_length_mfcc, rows past an utterance's
        own frames 0.  Each utterance is bitwise what it gives alone.  with_mel: -> (mfcc, mel (B, T_pad, n_mels) at the MFCC framing)."""
        wb = wavs if isinstance(wavs, WaveBatch) else WaveBatch(wavs)
        self._check_mfcc(wb.lens.tolist())
        dev = wb.device if wb.device is not None else _device()
        T_pad = int(1 + wb.lens.max() // self.hop_length_mfcc)
        mfcc, mel = toolops.audio_mfcc(wb.packed(dev), wb.offsets, wb.lens, self.n_fft, self.win_length_mfcc, self.hop_length_mfcc,
                                       self.preemphasis_coeff if preemphasis else 0.0, self.filterbank(dev), self.mfcc_table(dev), T_pad,
                                       with_mel=with_mel)
        return (mfcc, mel) if with_mel else mfcc

    def extract_mfcc_from_waveform(self, waveform, preemphasis=True, channel=0):
        """src/audio.py:132-154: waveform (channels, samples) -> (39, T) of `channel`, T = 1 + samples // hop_length_mfcc: 13 cepstra of
        the normalised mel at the 25 / 10 ms framing, their first and second derivatives; on the waveform's device (computed on the GPU
        either way)"""
        x = torch.as_tensor(waveform)
        x = x[channel] if x.dim() == 2 else x
        return self.extract_mfcc_batch([x], preemphasis=preemphasis)[0].t().to(x.device)

    # -- pitch (not a step of the reference): the YIN tracker st_f0_yin at the MFCC hop
    def f0_lags(self, fmin=60., fmax=500., window=None):
        """(tau_min, tau_max, W) of extract_f0_batch: tau_max = ceil(sr / fmin), tau_min = floor(sr / fmax), W = window or 2 tau_max;
        ValueError naming the limit of st_f0_yin an fmin / fmax / window leaves"""
        fmin, fmax = float(fmin), float(fmax)
        if not (0.0 < fmin < fmax < float('inf')):
            raise ValueError('f0: needs 0 < fmin < fmax (got fmin %r, fmax %r)' % (fmin, fmax))
        tau_max, tau_min = int(math.ceil(self.sr / fmin)), int(math.floor(self.sr / fmax))       # (fmin < fmax: tau_min < tau_max)
        if tau_max > toolops.F0_MAX_TAU:
            raise ValueError('f0: fmin %g Hz at %d Hz needs lags up to tau_max = %d; the limit is tau_max <= %d (fmin >= %.2f Hz)'
                             % (fmin, self.sr, tau_max, toolops.F0_MAX_TAU, self.sr / toolops.F0_MAX_TAU))
        if tau_min < 2:
            raise ValueError('f0: fmax %g Hz at %d Hz gives tau_min = %d; the limit is tau_min >= 2 (fmax <= %.1f Hz)'
                             % (fmax, self.sr, tau_min, self.sr / 2.0))
        W = 2 * tau_max if window is None else int(window)
        if not 1 <= W <= toolops.F0_MAX_W:
            raise ValueError('f0: window %d outside the limit 1 <= W <= %d' % (W, toolops.F0_MAX_W))
        return tau_min, tau_max, W

    def extract_f0_batch(self, wavs, fmin=60., fmax=500., threshold=0.15, window=None, with_aper=False):
        """F0 in Hz of a ragged batch in one st_f0_yin call: wavs as extract_mfcc_batch takes them (a list of 1-D waveforms or a
        WaveBatch), sorted longest first -> device (B, T_pad), frame t of an utterance centred on sample t * hop_length_mfcc, T_pad the
        longest utterance's 1 + L // hop_length_mfcc (the rows of extract_mfcc_batch), 0 on unvoiced frames and past an utterance's own
        frames.  The raw waveform, no pre-emphasis.  Lags and window: f0_lags.  with_aper: -> (f0, aper (B, T_pad)), the normalised
        difference d' at the chosen lag (the minimum of d' on an unvoiced frame).  Each utterance is bitwise what it gives alone."""
        tau_min, tau_max, W = self.f0_lags(fmin, fmax, window)
        wb = wavs if isinstance(wavs, WaveBatch) else WaveBatch(wavs)
        hop = self.hop_length_mfcc
        toolops._f0_check(wb.lens, hop, W, tau_min, tau_max, self.sr, threshold)
        dev = wb.device if wb.device is not None else _device()
        T_pad = int(1 + wb.lens.max() // hop)
        f0, aper = toolops.f0_yin(wb.packed(dev), wb.offsets, wb.lens, hop, W, tau_min, tau_max, float(self.sr), threshold, T_pad, with_aper=with_aper)
        return (f0, aper) if with_aper else f0

    def extract_f0_from_waveform(self, waveform, fmin=60., fmax=500., threshold=0.15, window=None, channel=0):
        """the single-utterance form of extract_f0_batch: waveform (channels, samples) or (samples,) -> (T,) F0 in Hz of `channel`,
        T = 1 + samples // hop_length_mfcc, on the waveform's device (computed on the GPU either way)"""
        x = torch.as_tensor(waveform)
        x = x[channel] if x.dim() == 2 else x
        return self.extract_f0_batch([x], fmin, fmax, threshold, window)[0].to(x.device)

    def extract_mfcc_from_file(self, wav_path, preemphasis=True, channel=0):
        """src/audio.py:119-130: the file-taking form of extract_mfcc_from_waveform"""
        return self.extract_mfcc_from_waveform(self.load(wav_path), preemphasis, channel)

    def boundary(self, file):
        """the boundary ratios of `file` (a path or a key) from the segment table; KeyError naming the file when it has no row"""
        if not self.use_segment:
            raise ValueError('segments: this converter was built without a segment_file')
        key = segment_key(str(file))
        if key not in self.boundary_table:
            raise KeyError('%s: no row %r in the segment file %s' % (file, key, self.segment_src))
        return self.boundary_table[key]

    def segment(self, feat, boundary):
        """src/audio.py:94-117: feat (T, D), boundary ratios -> (S, max_len, D), segment s the rows [start_s, end_s) of feat
        (segment_points), zero-padded to the longest candidate piece; on feat's device (gathered on the GPU either way)"""
        feat = torch.as_tensor(feat)
        if feat.dim() != 2:
            raise ValueError('segment: feat of shape %s, expected (T, D)' % (tuple(feat.shape),))
        seg, _ = self._gather(feat.unsqueeze(0), [feat.size(0)], [boundary])
        return seg.to(feat.device)

    def segment_batch(self, feats, lens, keys):
        """A whole batch cut in one st_segment_gather call: feats (B, T_pad, D), lens the frames of each utterance, keys their files
        (paths or table keys) -> (device (S_total, max_len, D), the segments of utterance 0 first, max_len the longest candidate piece
        of the batch; [segments per utterance]).  A key without a row is a KeyError before a device is touched."""
        feats = torch.as_tensor(feats)
        if feats.dim() != 3 or not len(lens) == len(keys) == feats.size(0):
            raise ValueError('segment_batch: feats of shape %s for %d lengths and %d keys' % (tuple(feats.shape), len(lens), len(keys)))
        return self._gather(feats, lens, [self.boundary(k) for k in keys])

    def _gather(self, feats, lens, boundaries):
        min_len = getattr(self, 'min_segment_len', 2)
        utt, start, length, counts, max_len = [], [], [], [], 0
        for b, (T, bd) in enumerate(zip(lens, boundaries)):
            if not 0 <= int(T) <= feats.size(1):
                raise ValueError('segments: utterance %d has %d frames, the batch holds %d' % (b, T, feats.size(1)))
            pieces, longest = segment_points(bd, int(T), min_len)
            max_len = max(max_len, longest)
            counts.append(len(pieces))
            for lo, hi in pieces:
                utt.append(b)
                start.append(lo)
                length.append(hi - lo)
        dev = feats.device if feats.is_cuda else _device()
        feats = feats.to(dev, torch.float32)
        if feats.stride(2) != 1:
            feats = feats.contiguous()
        table = torch.tensor([utt, start, length], dtype=torch.int32).reshape(3, len(utt)).to(dev)
        return toolops.segment_gather(feats, table[0], table[1], table[2], max_len), counts

    def segment_features(self, file):
        """the segmented feature of src/audio.py:339-354, which wave_to_feat computes there and does not return: segment_feat
        ('mfcc': the file's MFCC, what the reference's undefined `_mfcc` plainly means; 'mel' / 'linear': its clean spectrograms) of
        `file` cut at its row of the segment table -> CPU (S, max_len, seg_feat_dim)"""
        boundary = self.boundary(file)
        wave = self.load(file)
        if self.segment_feat == 'mfcc':
            feat = self.extract_mfcc_from_waveform(wave)
        else:
            sp, msp = self.extract_feature_from_waveform(wave)
            feat = msp if self.segment_feat == 'mel' else sp
        return self.segment(feat.t(), boundary).cpu()

    def _draw(self):
        """one utterance's augmentation draws in the order of src/audio.py:356-364: (snr or None, stretch rate)"""
        snr = None if -1 in self.snr_range else random.uniform(self.snr_range[0], self.snr_range[1])
        return snr, random.uniform(self.time_stretch_range[0], self.time_stretch_range[1])

    def wave_to_feat(self, file):
        """src/audio.py:329-395: -> (msp (T, n_mels), msp_aug (T', n_mels), sp (T, F) or None) as CPU tensors.  The SNR and the
        stretch rate are drawn from `random`; the noise comes from the kernel's generator, seeded from torch's."""
        wave = self.load(file)
        mel, aug, lin = self.extract_batch([wave[0]])
        return mel[0].cpu(), aug[0].cpu(), lin[0].cpu() if lin is not None else None

    def extract_batch(self, wavs, r=None, seed=None, snr=None, stretch=None, noise=None):
        """The training loader's features for a ragged batch in one launch sequence (collect_fn + fetch_data, src/data.py:120-140,
        bin/train_vqvae.py:33-53): wavs, a list of 1-D waveforms (or a WaveBatch), sorted longest first.  -> device tensors
        (mel (B, T_pad, n_mels), aug_mel (B, Ta_pad, n_mels), linear (B, T_pad, F) or None when use_linear is off); mel / linear
        padded with zero frames to a multiple of r with at least one extra frame (r None: to the longest), aug_mel to its own
        longest.  snr / stretch: None draws them per utterance as wave_to_feat does; else one value or one per utterance (in the
        sorted order); an SNR of SNR_OFF (NaN), or None inside a list, means no noise.  noise: explicit noise waveforms, one per utterance of wavs (for
        tests); else the generator of `seed` (None: drawn from torch's generator)."""
        wb = wavs if isinstance(wavs, WaveBatch) else WaveBatch(wavs)
        B = len(wb.lens)
        per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * B    # noqa: E731
        if snr is None or stretch is None:
            draws = [self._draw() for _ in range(B)]
            snr = [d[0] for d in draws] if snr is None else snr
            stretch = [d[1] for d in draws] if stretch is None else stretch
        snr, stretch = per(snr), per(stretch)
        if len(snr) != B or len(stretch) != B:
            raise ValueError('features: %d utterances, %d SNRs and %d stretch rates' % (B, len(snr), len(stretch)))
        aug_dims = [self.stretch_dims(s) for s in stretch]
        self._check(wb.lens, aug_dims)
        snr_db = np.array([np.nan if v is None else v for v in snr], np.float32)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)))
        dev = wb.device if wb.device is not None else _device()
        x = wb.packed(dev)
        nz = None
        if noise is not None:
            nz = WaveBatch(noise, order=wb.order).packed(dev)
            if nz.shape != x.shape:
                raise ValueError('features: the noise waveforms do not have the lengths of the utterances')
        T = 1 + wb.lens // self.hop_length
        T_pad = int(T.max()) if r is None else int(T.max()) + r - int(T.max()) % r
        Ta_pad = max(1 + L // h for L, (_, h) in zip(wb.lens, aug_dims))
        mel, lin, aug = toolops.audio_features(x, wb.offsets, wb.lens, self.n_fft, self.win_length, self.hop_length, self.preemphasis_coeff,
                                               self.filterbank(dev), T_pad, with_linear=self.use_linear,
                                               aug_win=[d[0] for d in aug_dims], aug_hop=[d[1] for d in aug_dims], Ta_pad=Ta_pad,
                                               snr_db=snr_db, noise=nz, seed=seed)
        return mel, aug, lin

    def gen_wav_device(self, lin, phases=None, frames=None, mel=False):
        """feat_to_wave for a device batch (B, T, F) without the host copy: -> (B, hop * (T - 1)) device tensor (SpecgramGenerator).
        mel=True: `lin` is the mel output (B, T, n_mels) instead (mel_to_wave).  frames: per-utterance frame counts (vocode_batch)."""
        if mel:
            self._check_mel(lin.size(-1))
        elif lin.size(-1) != self.num_freq:
            raise NotImplementedError('gen_wav: only the linear spectrogram (%d bins) is vocoded, got %d' % (self.num_freq, lin.size(-1)))
        return _run(lin, phases, self.n_fft, self.hop_length, self.win_length, GFL_ITER, normalized=True, power=1.0,
                    post=toolops.GL_CLIP | toolops.GL_INV_PREEMPHASIS, basis=self.mel_basis if mel else None, frames=frames)


def load_audio_transform(num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear=True,
                         **kwargs):
    """src/audio.py:439-448 (segment_file / segment_feat / min_segment_len travel in kwargs: AudioConverter reads them)"""
    return AudioConverter(num_freq, num_mels, frame_length_ms, frame_shift_ms, preemphasis_coeff, sample_rate, use_linear, **kwargs)


class WaveBatch:
    """a ragged batch of 1-D waveforms sorted longest first (stable: src/data.py:130), packed into one float32 buffer the first
    time a device asks for it and kept there: `order[i]` is the index in the given list of the i-th utterance"""

    def __init__(self, wavs, order=None):
        wavs = [torch.as_tensor(w).reshape(-1) for w in wavs]
        if not wavs:
            raise ValueError('features: an empty batch')
        lens = np.array([w.numel() for w in wavs], np.int64)
        self.order = np.argsort(-lens, kind='stable') if order is None else np.asarray(order)
        self._wavs = [wavs[i] for i in self.order]
        self.lens = lens[self.order]
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64)
        self.device = self._wavs[0].device if self._wavs[0].is_cuda else None
        self._packed = {}

    @classmethod
    def window(cls, buffer, offsets, lens):
        """a batch that lives inside a larger packed float32 device buffer (the corpus loader's split): utterance b is
        buffer[offsets[b] : offsets[b] + lens[b]], nothing is copied and the offsets need not be cumulative.  The utterances must come
        longest first already (what the constructor's stable sort would leave as it is)."""
        lens, offsets = np.asarray(lens, np.int64), np.asarray(offsets, np.int64)
        if not (buffer.is_cuda and buffer.dtype == torch.float32 and buffer.dim() == 1 and buffer.is_contiguous()):
            raise ValueError('features: a window needs a contiguous 1-D float32 device buffer')
        if lens.ndim != 1 or lens.shape != offsets.shape or len(lens) == 0:
            raise ValueError('features: an empty batch')
        if (lens < 1).any() or (offsets < 0).any() or (offsets + lens > buffer.numel()).any():
            raise ValueError('features: a window outside its buffer of %d samples' % buffer.numel())
        if (np.diff(lens) > 0).any():
            raise ValueError('features: the utterances of a window come longest first')
        wb = cls.__new__(cls)
        wb.order = np.arange(len(lens))
        wb._wavs = None
        wb.lens, wb.offsets = lens.copy(), offsets.copy()
        wb.device = buffer.device
        wb._packed = {str(buffer.device): buffer}
        return wb

    @classmethod
    def from_packed(cls, buffer, lens, order):
        """a batch over a packed float32 device buffer that holds the utterances back to back in the order given: the i-th stretch of
        `buffer` is utterance order[i] of the caller's list and has lens[order[i]] samples (lens: in the caller's order).  Nothing is
        sorted or copied here -- the layout is the caller's statement, and the lengths must not grow along it."""
        lens, order = np.asarray(lens, np.int64), np.asarray(order, np.int64)
        if not (buffer.is_cuda and buffer.dtype == torch.float32 and buffer.dim() == 1 and buffer.is_contiguous()):
            raise ValueError('features: a packed batch needs a contiguous 1-D float32 device buffer')
        if lens.ndim != 1 or len(lens) == 0 or (lens < 1).any() or not np.array_equal(np.sort(order), np.arange(len(lens))):
            raise ValueError('features: a packed batch needs positive lengths and a permutation of their indices')
        if int(lens.sum()) != buffer.numel() or (np.diff(lens[order]) > 0).any():
            raise ValueError('features: the buffer holds the utterances back to back, longest first')
        off = np.concatenate([[0], np.cumsum(lens[order])[:-1]])
        views = [None] * len(lens)
        for i, o in zip(order, off):
            views[i] = buffer[int(o):int(o + lens[i])]
        wb = cls(views, order=order)
        wb._packed[str(buffer.device)] = buffer
        return wb

    def inverse(self):
        """the inverse of `order`: element i is the row of this batch that holds the i-th given utterance"""
        return np.argsort(np.asarray(self.order), kind='stable')

    def packed(self, device):
        key = str(device)
        if key not in self._packed:
            self._packed[key] = torch.cat([w.to(device, torch.float32) for w in self._wavs]).contiguous()
        return self._packed[key]


def hz_to_mel(f):
    """Slaney's mel scale (Auditory Toolbox): linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 mels per factor 6.4)"""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3)
    logs = 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, logs, lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """(n_mels, n_fft // 2 + 1) float32 filterbank: triangles between n_mels + 2 points equally spaced on the Slaney mel scale
    from fmin to fmax (default sr / 2), each scaled by 2 / (f[m + 2] - f[m]) to unit area (Slaney normalisation).  Float64
    throughout, cast at the end (the reference's create_mel_filterbank, lib/filters.py)."""
    fmax = sr / 2.0 if fmax is None else fmax
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    rise = (freqs[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    fall = (f[2:, None] - freqs[None, :]) / (f[2:] - f[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(rise, fall)) * (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


RANK_RATIO_MIN = 1e-6             # smallest / largest singular value below which a filterbank counts as rank deficient


def mel_basis(sr, n_fft, n_mels):
    """(n_mels, n_fft // 2 + 1) float32: pinverse(mel_filterbank).T, the matrix of melspecgram_to_specgram (src/audio.py:202), in
    float64 and cast once.  A rank-deficient bank (smallest / largest singular value < 1e-6: mel bands narrower than one FFT bin
    give zero rows) raises ValueError: its pseudo-inverse is not a usable inverse (the reference's float32 torch.pinverse returns
    values off by orders of magnitude there)."""
    fb = mel_filterbank(sr, n_fft, n_mels).astype(np.float64)
    sv = np.linalg.svd(fb, compute_uv=False)
    if not sv[-1] >= RANK_RATIO_MIN * sv[0]:
        raise ValueError('mel_basis: the mel filterbank (%d Hz, n_fft %d, %d mels) is rank deficient (singular values %.3g .. %.3g): '
                         'mel -> linear has no usable pseudo-inverse; use fewer mels or a larger n_fft' % (sr, n_fft, n_mels, sv[-1], sv[0]))
    return np.ascontiguousarray(np.linalg.pinv(fb).T.astype(np.float32))


def band_pack(fb):
    """a filterbank (n_mels, F) whose rows are single contiguous bands -> int32 (start, count, offset) per row and the packed
    float32 weights of every band, back to back"""
    start, cnt, w = [], [], []
    for row in np.asarray(fb, np.float32):
        nz = np.flatnonzero(row)
        s, e = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        start.append(s)
        cnt.append(e - s)
        w.append(row[s:e])
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return (np.array(start, np.int32), np.array(cnt, np.int32), off.astype(np.int32),
            np.concatenate(w).astype(np.float32) if w else np.zeros(0, np.float32))


def load_wav(path, sample_rate=None):
    """16-bit PCM .wav through the standard library, scaled by 1 / 32768 as torchaudio.load: -> (channels, samples) float32.
    A sample rate other than `sample_rate` raises (src/audio.py:70-77)."""
    with wave.open(str(path), 'rb') as w:
        sr, ch, width = w.getframerate(), w.getnchannels(), w.getsampwidth()
        if width != 2:
            raise ValueError('load_wav: %s is %d-bit; only 16-bit PCM is read' % (path, 8 * width))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
    if sample_rate is not None and sr != sample_rate:
        raise ValueError('Sample rate mismatch. Expected %d but get %d (%s)' % (sample_rate, sr, path))
    return torch.from_numpy(np.ascontiguousarray(pcm.reshape(-1, ch).T, dtype=np.float32) / 32768.0)


def _read_pcm(path):
    """16-bit PCM .wav through the standard library: -> ((samples, channels) int16 array, sample rate)"""
    with wave.open(str(path), 'rb') as w:
        sr, ch, width = w.getframerate(), w.getnchannels(), w.getsampwidth()
        if width != 2:
            raise ValueError('read_wav: %s is %d-bit; only 16-bit PCM is read' % (path, 8 * width))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
    return pcm.reshape(-1, ch), sr


def read_wav(path):
    """load_wav at the file's own rate: -> ((channels, samples) float32 scaled by 1 / 32768, sample rate)"""
    pcm, sr = _read_pcm(path)
    return torch.from_numpy(np.ascontiguousarray(pcm.T, dtype=np.float32) / 32768.0), sr


def write_wav(path, wav, sr):
    """16-bit PCM mono .wav through the standard library (soundfile's default subtype for .wav): round(clip(x, -1, 1) * 32767)"""
    wav = np.asarray(wav, dtype=np.float64).reshape(-1)
    write_pcm16(path, np.rint(np.clip(wav, -1.0, 1.0) * 32767.0), sr)


def write_pcm16(path, pcm, sr):
    """16-bit PCM mono .wav of samples that are int16 values already"""
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(np.ascontiguousarray(pcm, dtype='<i2').tobytes())


# -- sample-rate conversion (st_resample_batch; the definition is in include/semitts.h and DESIGN.md 3.14)
RESAMPLE_LPW, RESAMPLE_ROLLOFF = 6, 0.99      # torchaudio.functional.resample's defaults
_RESAMPLE = {}                                # (o, n, lpw, rolloff) -> host table; (.., device) -> its copy on that device


def _ratio(orig_sr, new_sr):
    """(o, n) = the two rates in lowest terms; anything but positive integers raises ValueError"""
    for v, what in ((orig_sr, 'orig_sr'), (new_sr, 'new_sr')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError('resample: %s must be a positive integer, got %r' % (what, v))
    g = np.gcd(int(orig_sr), int(new_sr))
    return int(orig_sr) // int(g), int(new_sr) // int(g)


def resampled_len(L, orig_sr, new_sr):
    """samples of an L-sample waveform after conversion: ceil(L new_sr / orig_sr), in integers"""
    o, n = _ratio(orig_sr, new_sr)
    return (n * int(L) + o - 1) // o


def resample_table(orig_sr, new_sr, lowpass_filter_width=RESAMPLE_LPW, rolloff=RESAMPLE_ROLLOFF, device=None):
    """The polyphase filter of orig_sr -> new_sr: (o, n, taps, first, table), o / n the ratio in lowest terms.  Output m (phase
    p = m mod n) is sum_k table[p, k] * x[floor(m o / n) + first[p] + k]: table (n, taps) float32 holds the Hann-windowed sinc of
    the header's definition, scale base / o included, computed in float64 and rounded once, exactly 0 where |i - tau| >= W (rows
    with fewer taps than the widest are padded with such zeros).  first (n,) int32.  device None: numpy arrays; else the copies on
    that device.  Cached per ratio and per device.  Raises ValueError, before any device is touched, for rates that are not
    positive integers and for a ratio the kernel does not take (toolops.RESAMPLE_MAX_TABLE_FLOATS / RESAMPLE_MAX_STAGE_FLOATS)."""
    o, n = _ratio(orig_sr, new_sr)
    lpw, rolloff = int(lowpass_filter_width), float(rolloff)
    if lpw != lowpass_filter_width or lpw < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError('resample: need an integer lowpass_filter_width >= 1 and 0 < rolloff <= 1, got %r and %r'
                         % (lowpass_filter_width, rolloff))
    key = (o, n, lpw, rolloff)
    if key not in _RESAMPLE:
        if o * n >= 2 ** 31:
            raise ValueError('resample: %d -> %d Hz is the ratio %d / %d; the kernel needs o * n < 2^31' % (orig_sr, new_sr, o, n))
        base = min(o, n) * rolloff
        W = lpw * o / base
        frac = ((np.arange(n, dtype=np.int64) * o) % n) / float(n)       # tau - floor(tau) of each phase
        first = np.floor(frac - W).astype(np.int64) + 1
        last = np.ceil(frac + W).astype(np.int64) - 1
        taps = int((last - first + 1).max())
        tab_f, stage_f = toolops.resample_lds_floats(o, n, taps, int(first.min()), int(first.max()))
        if tab_f > toolops.RESAMPLE_MAX_TABLE_FLOATS or stage_f > toolops.RESAMPLE_MAX_STAGE_FLOATS:
            raise ValueError('resample: %d -> %d Hz (ratio %d / %d, %d taps) needs %d floats of staged table (limit %d) and %d of staged '
                             'input (limit %d)' % (orig_sr, new_sr, o, n, taps, tab_f, toolops.RESAMPLE_MAX_TABLE_FLOATS, stage_f,
                                                   toolops.RESAMPLE_MAX_STAGE_FLOATS))
        t = (first[:, None] + np.arange(taps)[None, :]) - frac[:, None]  # i - tau
        a = np.pi * base * t / o
        h = (base / o) * np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a)) * np.cos(a / (2.0 * lpw)) ** 2
        table = np.ascontiguousarray(np.where(np.abs(t) < W, h, 0.0).astype(np.float32))
        _RESAMPLE[key] = (o, n, taps, first.astype(np.int32), table)
    if device is None:
        return _RESAMPLE[key]
    dkey = key + (str(device),)
    if dkey not in _RESAMPLE:
        _, _, taps, first, table = _RESAMPLE[key]
        _RESAMPLE[dkey] = (o, n, taps, torch.from_numpy(first).to(device), torch.from_numpy(table).to(device))
    return _RESAMPLE[dkey]


# -- K-weighting (st_loudness_batch; the definition is in include/semitts.h and DESIGN.md 3.22)
_KWEIGHT = {}                                 # sr -> host table; (sr, device) -> its copy on that device


def kweight_coeffs(sr):
    """The two biquads of the BS.1770 K-weighting at the sample rate sr, in float64: ((b, a) of the shelf, (b, a) of the high-pass),
    each three coefficients with a[0] = 1.  The standard's table at 48 kHz to its 14 printed digits."""
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return (b1, a1), (b2, a2)


def kweight_state_matrix(sr):
    """A of s' = A s + B x for the cascade of the two biquads in DF2-transposed form, state (shelf s1, s2, high-pass s1, s2), float64"""
    (_, a), (_, p) = kweight_coeffs(sr)
    return np.array([[-a[1], 1.0, 0.0, 0.0], [-a[2], 0.0, 0.0, 0.0], [-2.0 - p[1], 0.0, -p[1], 1.0], [1.0 - p[2], 0.0, -p[2], 0.0]])


def kweight_tables(sr, device=None):
    """What st_loudness_batch needs at the rate sr, toolops.LOUDNESS_TABLE_DOUBLES float64 values laid out as include/semitts.h says: the
    coefficients, A^(r 2^k) for k < 8, A^hop and A^max(0, t r - pad) for t < 256 (r the samples a thread owns, pad = 256 r - hop).
    device None: a numpy array; else its copy on that device.  Cached per rate and per device."""
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or not toolops.LOUDNESS_MIN_SR <= sr <= toolops.LOUDNESS_MAX_SR:
        raise ValueError('loudness: the sample rate must be an integer in [%d, %d] (got %r)' % (toolops.LOUDNESS_MIN_SR, toolops.LOUDNESS_MAX_SR, sr))
    sr = int(sr)
    if sr not in _KWEIGHT:
        (b, a), (_, p) = kweight_coeffs(sr)
        A = kweight_state_matrix(sr)
        hop, r, nt = toolops.loudness_hop(sr), toolops.loudness_run_length(sr), toolops.LOUDNESS_THREADS
        pad = nt * r - hop
        power = np.linalg.matrix_power
        tab = np.concatenate([[b[0], b[1], b[2], a[1], a[2], p[1], p[2], 0.0]] + [power(A, r << k).reshape(-1) for k in range(8)]
                             + [power(A, hop).reshape(-1)] + [power(A, max(0, t * r - pad)).reshape(-1) for t in range(nt)])
        assert tab.shape == (toolops.LOUDNESS_TABLE_DOUBLES,) and tab.dtype == np.float64
        _KWEIGHT[sr] = tab
    if device is None:
        return _KWEIGHT[sr]
    dkey = (sr, str(device))
    if dkey not in _KWEIGHT:
        _KWEIGHT[dkey] = torch.from_numpy(_KWEIGHT[sr]).to(device)
    return _KWEIGHT[dkey]


def resample(wavs, orig_sr, new_sr):
    """Sample-rate conversion of a ragged batch on the GPU (st_resample_batch, one launch per 64 utterances): wavs, a list of 1-D
    waveforms (tensors or arrays, floating point or int16 PCM -- int16 counts as x / 32768 and is uploaded as PCM) or a WaveBatch
    -> a WaveBatch at new_sr on the device, ready for extract_batch: sorted longest first again, `.order[i]` the index in the
    caller's list of the i-th utterance.  orig_sr == new_sr launches nothing and returns the input's values as they are (a
    WaveBatch itself).  Every refusal (resample_table's, an empty batch or utterance, a dtype that is neither) raises ValueError
    before a device is touched."""
    o, n, _, first, _ = resample_table(orig_sr, new_sr)
    given = wavs if isinstance(wavs, WaveBatch) else None
    src = given._wavs if given is not None else [torch.as_tensor(w).reshape(-1) for w in wavs]
    if not src:
        raise ValueError('resample: an empty batch')
    for i, w in enumerate(src):
        if not (w.dtype == torch.int16 or w.dtype.is_floating_point):
            raise ValueError('resample: utterance %d is %s; waveforms are floating point or int16 PCM' % (i, w.dtype))
        if w.numel() < 1 or resampled_len(w.numel(), o, n) >= 2 ** 31:
            raise ValueError('resample: utterance %d has %d samples' % (i, w.numel()))
    pcm = all(w.dtype == torch.int16 for w in src)
    as_float = lambda w: w.to(torch.float32) / 32768.0 if w.dtype == torch.int16 else w.to(torch.float32)      # noqa: E731
    if o == n:
        return given if given is not None else WaveBatch([as_float(w) if w.dtype == torch.int16 else w for w in src])
    dev = next((w.device for w in src if w.is_cuda), None) or _device()
    x = torch.cat([w.to(dev) if pcm else as_float(w).to(dev) for w in src]).contiguous()
    lens = np.array([w.numel() for w in src], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    _, _, _, first_d, table_d = resample_table(orig_sr, new_sr, device=dev)
    y, out_off, out_lens = toolops.resample_batch(x, off, lens, o, n, first_d, table_d, int(first.min()), int(first.max()))
    out = WaveBatch([y[int(a):int(a + b)] for a, b in zip(out_off, out_lens)])
    if np.array_equal(out.order, np.arange(len(src))):
        out._packed[str(dev)] = y                       # already packed in the sorted order: no second copy
    if given is not None:
        out.order = np.asarray(given.order)[out.order]
    return out


_resample = resample      # (AudioConverter.load_batch has an argument of that name)
