"""The directory tools of main.py that build no model: each is picked by a flag, reads a directory of files, runs a GPU routine in
batches of --batch-size and writes files or a table (`Tool(config, paras, mode).load_data().set_model().exec()`, the solver protocol).
DirTool holds what they share -- the constructor, the batching, the table writer -- and the functions under it the checks of .wav
headers, the loading of a batch and the choice of a feature.  solver.py imports every public name of this module, so the tools stay
reachable as solver.X; the tools that build a model (Transcriber, Aligner, Synthesiser) live there."""
import math
import os
import time

import numpy as np
import torch

from . import toolops


class DirTool:
    def __init__(self, config, paras, mode):
        self.config, self.paras, self.mode = config, paras, mode
        self.exp_name = getattr(paras, 'name', None) or 'synthetic'
        self.logdir = os.path.join(getattr(paras, 'logdir', 'log/'), self.exp_name)

    def set_model(self):
        return self

    def batches(self, items, cap=None):
        """slices of --batch-size items (of a range: sub-ranges); cap: the batch size is clamped to [1, cap]"""
        B = int(self.paras.batch_size)
        if cap is not None:
            B = max(1, min(B, cap))
        for i in range(0, len(items), B):
            yield items[i:i + B]

    def write_lines(self, name, lines):
        """<logdir>/<name>, one line each -> its path"""
        path = os.path.join(self.logdir, name)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return path


# -- .wav directories
def list_wavs(directory, flag):
    """the .wav files of a directory sorted by name; ValueError naming the command-line flag when it holds none"""
    files = sorted(f for f in os.listdir(directory) if f.lower().endswith('.wav'))
    if not files:
        raise ValueError('%s %s: no .wav files' % (flag, directory))
    return files


def wav_header(path, flag=None):
    """-> (sample rate, channels, bytes per sample, frames).  A file `wave` does not open raises wave's own error, or with `flag`
    a ValueError naming that flag and the path"""
    import wave
    try:
        with wave.open(path, 'rb') as w:
            return w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
    except (OSError, EOFError, wave.Error) as e:
        if flag is None:
            raise
        raise ValueError('%s: %s is not a readable .wav file (%s)' % (flag, path, e))


def check_wav(directory, f, flag, rate=None):
    """the header of directory/f: 16-bit, not empty and, with `rate`, at that rate -> its rate; the messages name f without its path"""
    sr, _, width, n = wav_header(os.path.join(directory, f))
    if width != 2:
        raise ValueError('%s: %s is %d-bit; only 16-bit PCM is read' % (flag, f, 8 * width))
    if n < 1:
        raise ValueError('%s: %s holds no samples' % (flag, f))
    if rate is not None and sr != rate:
        raise ValueError('Sample rate mismatch. Expected %d but get %d (%s)' % (rate, sr, f))
    return sr


def check_out_dir(out_flag, out_dir, wav_flag, wav_dir):
    if os.path.realpath(wav_dir) == os.path.realpath(out_dir):
        raise ValueError('%s %s is the directory %s reads' % (out_flag, out_dir, wav_flag))


def trim_args(paras):
    """the `trim` argument of AudioConverter.load_batch / corpus.load_splits from --trim-silence and its options; None without the flag"""
    if not getattr(paras, 'trim_silence', False):
        return None
    return dict(top_db=float(getattr(paras, 'trim_top_db', 60.0)), frame_length=int(getattr(paras, 'trim_frame_length', 2048)),
                hop_length=int(getattr(paras, 'trim_hop', 512)), pad_ms=float(getattr(paras, 'trim_pad_ms', 0.0)))


def loudness_args(paras):
    """the `loudness` argument of AudioConverter.load_batch / vocode_batch / corpus.load_splits from --normalize-loudness and its options;
    None without the flag"""
    if not getattr(paras, 'normalize_loudness', False):
        return None
    return dict(target=float(getattr(paras, 'loudness_target', -23.0)), peak_db=float(getattr(paras, 'loudness_peak', -1.0)),
                max_gain_db=float(getattr(paras, 'loudness_max_gain', 30.0)))


def load_waves(conv, directory, names, paras, resample=None):
    """channel 0 of the files `names` of `directory` as one WaveBatch on the device (AudioConverter.load_batch), trimmed and normalised
    as --trim-silence and --normalize-loudness say; resample: load_batch's argument, left at its default when None"""
    kw = {} if resample is None else dict(resample=resample)
    return conv.load_batch([os.path.join(directory, f) for f in names], trim=trim_args(paras), loudness=loudness_args(paras), **kw)


def mfcc_frames(conv, lens):
    """the MFCC (and pitch) frames of utterances of `lens` samples"""
    return 1 + lens // conv.hop_length_mfcc


def extract_features(conv, wb, feat, f0=None):
    """the feature `feat` (mfcc, mel, linear, or f0 with the tracker's settings `f0`) of a WaveBatch -> (features (B, T_pad, D) on the
    device in the batch's sorted order, frames per row, order)"""
    from .audio import SNR_OFF
    if feat == 'mfcc':
        return conv.extract_mfcc_batch(wb), mfcc_frames(conv, wb.lens), wb.order
    if feat == 'f0':
        return conv.extract_f0_batch(wb, **f0), mfcc_frames(conv, wb.lens), wb.order
    mel, _, lin = conv.extract_batch(wb, snr=SNR_OFF, stretch=1.0)
    return (mel if feat == 'mel' else lin), 1 + wb.lens // conv.hop_length, wb.order


VOCODE_SUFFIX = {'spec': '-spec.npy', 'mel': '-mel.npy'}


def list_vocode_files(feat_dir, kind, conv):
    """the saved spectrograms of --vocode-dir: the files of `feat_dir` ending in -spec.npy (kind 'spec') or -mel.npy ('mel'), sorted
    by name -> [(file name, stem)], the stem being the name without that ending (the .wav written is <stem>.wav, as the reference's
    util/gen_wav_from_specgram.py names it).  Every file's header is read: one that is not (T, bins) with the converter's bin
    count, or has fewer frames than Griffin-Lim takes, raises ValueError naming it."""
    from .audio import min_frames
    suffix = VOCODE_SUFFIX[kind]
    names = sorted(f for f in os.listdir(feat_dir) if f.endswith(suffix))
    if not names:
        raise ValueError('--vocode-dir %s: no *%s files' % (feat_dir, suffix))
    bins = conv.num_freq if kind == 'spec' else conv.n_mels
    lo = min_frames(conv.n_fft, conv.hop_length)
    for f in names:
        shape = np.load(os.path.join(feat_dir, f), mmap_mode='r', allow_pickle=False).shape
        if len(shape) != 2 or shape[1] != bins:
            raise ValueError('--vocode-dir: %s has shape %s, expected (frames, %d) for --vocode-feat %s' % (f, tuple(shape), bins, kind))
        if shape[0] < lo:
            raise ValueError('--vocode-dir: %s has %d frames, too few: Griffin-Lim needs at least %d (hop %d, n_fft %d)'
                             % (f, shape[0], lo, conv.hop_length, conv.n_fft))
    return [(f, f[:-len(suffix)]) for f in names]


def vocode(conv, feats, kind, paras):
    """AudioConverter.vocode_batch, with --normalize-loudness the waveforms normalised on the device before the copy to the host
    (without the flag the call is the one it always was)"""
    args = loudness_args(paras)
    return conv.vocode_batch(feats, kind) if args is None else conv.vocode_batch(feats, kind, loudness=args)


class Vocoder(DirTool):
    """main.py --vocode-dir: the saved -spec.npy (or, with --vocode-feat mel, -mel.npy) files of a directory, sorted by name, in
    batches of --batch-size -> AudioConverter.vocode_batch (one Griffin-Lim call per batch, each utterance at its own length) ->
    <logdir>/<stem>.wav.  The counterpart of the reference's util/gen_wav_from_specgram.py; it reads no checkpoint and builds no
    model.  Every file is checked in load_data: a bad one stops the run before anything is written."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.kind = getattr(paras, 'vocode_feat', 'spec')

    def load_data(self):
        from .audio import load_audio_transform
        self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        self.feat_dir = self.paras.vocode_dir
        self.files = list_vocode_files(self.feat_dir, self.kind, self.audio_converter)
        if self.kind == 'mel':
            self.audio_converter.mel_basis()             # (a rank-deficient filterbank stops the run here too)
        return self

    def exec(self):
        from .audio import write_wav
        os.makedirs(self.logdir, exist_ok=True)
        t0, n = time.perf_counter(), 0
        for chunk in self.batches(self.files):
            wavs = vocode(self.audio_converter, [np.load(os.path.join(self.feat_dir, f), allow_pickle=False) for f, _ in chunk], self.kind, self.paras)
            for (_, stem), w in zip(chunk, wavs):
                write_wav(os.path.join(self.logdir, stem + '.wav'), w, self.audio_converter.sr)
                n += 1
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', 'Vocoded %d %s files into %s, %.2f s' % (n, VOCODE_SUFFIX[self.kind], self.logdir, time.perf_counter() - t0))
        return n


class Resampler(DirTool):
    """main.py --resample-wav-dir DIR --resample-out DIR2 [--resample-rate N]: channel 0 of every .wav of DIR (sorted by name, batches of
    --batch-size) converted to N Hz (default: data.audio.sample_rate of --config) on the GPU (audio.resample, the files of a batch
    grouped by their rate, uploaded as int16 PCM) and written as 16-bit mono to DIR2/<same name> through write_wav.  No checkpoint,
    no model.  Every header is read in load_data: an unreadable file or a ratio the kernel refuses stops the run before anything
    is written."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        rate = getattr(paras, 'resample_rate', None)
        self.rate = int(rate if rate is not None else config['data']['audio']['sample_rate'])

    def load_data(self):
        from .audio import resample_table
        self.wav_dir, self.out_dir = self.paras.resample_wav_dir, self.paras.resample_out
        check_out_dir('--resample-out', self.out_dir, '--resample-wav-dir', self.wav_dir)
        self.files = list_wavs(self.wav_dir, '--resample-wav-dir')
        for f in self.files:
            resample_table(check_wav(self.wav_dir, f, '--resample-wav-dir'), self.rate)
        return self

    def exec(self):
        from .audio import _read_pcm, resample, write_wav
        os.makedirs(self.out_dir, exist_ok=True)
        t0, n = time.perf_counter(), 0
        for names in self.batches(self.files):
            read = [_read_pcm(os.path.join(self.wav_dir, f)) for f in names]
            groups = {}
            for k, (_, sr) in enumerate(read):
                groups.setdefault(sr, []).append(k)
            for sr, idx in sorted(groups.items()):
                if sr == self.rate:                                 # nothing to convert: channel 0 as it is
                    for k in idx:
                        write_wav(os.path.join(self.out_dir, names[k]), read[k][0][:, 0] / 32768.0, self.rate)
                        n += 1
                    continue
                wb = resample([torch.from_numpy(read[k][0][:, 0].copy()) for k in idx], sr, self.rate)
                y = wb.packed(wb.device).cpu().numpy()
                for row, k in enumerate(wb.order):
                    write_wav(os.path.join(self.out_dir, names[idx[k]]), y[wb.offsets[row]:wb.offsets[row] + wb.lens[row]], self.rate)
                    n += 1
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', 'Resampled %d files to %d Hz into %s, %.2f s' % (n, self.rate, self.out_dir, time.perf_counter() - t0))
        return n


class LoudnessWriter(DirTool):
    """main.py --loudness-wav-dir DIR [--loudness-out DIR2] --config CFG [--loudness-target -23 --loudness-peak -1 --loudness-max-gain 30
    --resample --trim-silence ...]: channel 0 of every .wav of DIR (sorted by name, batches of --batch-size, at data.audio.sample_rate;
    with --resample files of another rate are converted, with --trim-silence the kept span is metered) measured on the GPU
    (st_loudness_batch: ITU-R BS.1770-4 integrated loudness) into loudness.csv: file, samples, seconds, lufs, momentary_max, rel_gate,
    peak_dbfs, n_blocks, n_abs, n_rel, gain_db (what brings the file to the target within the two limits), flags
    (toolops.LOUDNESS_FLAGS).  With --loudness-out every file is also written there normalised, as 16-bit mono from the device's int16
    output (st_wave_gain); a file the meter flags as non-finite, under 400 ms or silent is copied at the level it has (channel 0 of its
    own samples when it is at the rate already).  The table goes
    into DIR2, or into DIR when nothing is written back.  No checkpoint, no model."""

    COLUMNS = ['file', 'samples', 'seconds', 'lufs', 'momentary_max', 'rel_gate', 'peak_dbfs', 'n_blocks', 'n_abs', 'n_rel', 'gain_db', 'flags']

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.args = dict(target=float(paras.loudness_target), peak_db=float(paras.loudness_peak), max_gain_db=float(paras.loudness_max_gain))

    def load_data(self):
        from .audio import load_audio_transform
        self.wav_dir, self.out_dir = self.paras.loudness_wav_dir, getattr(self.paras, 'loudness_out', None)
        if self.out_dir is not None:
            check_out_dir('--loudness-out', self.out_dir, '--loudness-wav-dir', self.wav_dir)
        self.files = list_wavs(self.wav_dir, '--loudness-wav-dir')
        self.audio_converter = conv = load_audio_transform(**self.config['data']['audio'])
        conv._check_loudness(**self.args)
        if trim_args(self.paras) is not None:
            conv._check_trim(**trim_args(self.paras))
        for f in self.files:
            check_wav(self.wav_dir, f, '--loudness-wav-dir', None if getattr(self.paras, 'resample', False) else conv.sr)
        return self

    @staticmethod
    def _db(v):
        return '%.3f' % v

    def exec(self):
        import csv
        from .audio import _read_pcm, write_pcm16
        conv = self.audio_converter
        if self.out_dir is not None:
            os.makedirs(self.out_dir, exist_ok=True)
        t0, rows = time.perf_counter(), []
        for names in self.batches(self.files):
            wb = conv.load_batch([os.path.join(self.wav_dir, f) for f in names], resample=bool(getattr(self.paras, 'resample', False)),
                                 trim=trim_args(self.paras))      # (never normalised here: the meter reads the file's own level)
            x = wb.packed(wb.device)
            pcm = torch.zeros(x.numel(), device=x.device, dtype=torch.int16) if self.out_dir is not None else None
            parts = []
            for b0 in range(0, len(wb.lens), toolops.FEATURES_MAX_BATCH):
                sl = slice(b0, b0 + toolops.FEATURES_MAX_BATCH)
                _, stats, counts = toolops.loudness(x, wb.offsets[sl], wb.lens[sl], conv.sr, **self.args)
                if pcm is not None:
                    toolops.wave_gain(x, wb.offsets[sl], wb.lens[sl], stats, out=pcm, pcm16=True)
                parts.append((stats, counts))
            stats = torch.cat([p[0] for p in parts]).cpu().numpy().astype(np.float64)
            counts = torch.cat([p[1] for p in parts]).cpu().numpy()
            pcm = None if pcm is None else pcm.cpu().numpy()
            batch = [None] * len(names)
            for row, k in enumerate(wb.order):
                f, n, st, ct = names[k], int(wb.lens[row]), stats[row], counts[row]
                with np.errstate(divide='ignore'):
                    batch[k] = [f, n, '%.6f' % (n / conv.sr), self._db(st[0]), self._db(st[1]), self._db(st[2]), self._db(20.0 * np.log10(st[3])),
                                int(ct[0]), int(ct[1]), int(ct[2]), self._db(20.0 * np.log10(st[5])), int(ct[3])]
                if pcm is not None:
                    data = pcm[int(wb.offsets[row]):int(wb.offsets[row]) + n]
                    if int(ct[3]) & 7:                              # left alone: the file's own samples (of the kept span), not a requantisation
                        raw, sr = _read_pcm(os.path.join(self.wav_dir, f))
                        if sr == conv.sr:
                            lo, hi = wb.bounds[k] if hasattr(wb, 'bounds') else (0, raw.shape[0])
                            data = raw[int(lo):int(hi), 0]
                    write_pcm16(os.path.join(self.out_dir, f), data, conv.sr)
            rows += batch
        with open(os.path.join(self.out_dir if self.out_dir is not None else self.wav_dir, 'loudness.csv'), 'w', newline='') as fh:
            out = csv.writer(fh)
            out.writerow(self.COLUMNS)
            out.writerows(rows)
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', 'Metered %d files%s, %.2f s' % (len(rows), '' if self.out_dir is None else ' and wrote them at %.1f LUFS into %s'
                                                            % (self.args['target'], self.out_dir), time.perf_counter() - t0))
        return len(rows)


class Trimmer(DirTool):
    """main.py --trim-wav-dir DIR --trim-out DIR2 --config CFG [--trim-top-db 60 --trim-frame-length 2048 --trim-hop 512 --trim-pad-ms 0]:
    channel 0 of every .wav of DIR (sorted by name, batches of --batch-size, at data.audio.sample_rate) trimmed on the GPU
    (AudioConverter.trim_batch) and its kept span written to DIR2/<same name> as the exact int16 samples of the file -- the bounds come
    from the device, the samples never leave the host as floats.  DIR2/trim.csv: file, samples, start, end, seconds, kept_seconds,
    n_intervals (the non-silent intervals of librosa.effects.split inside the file).  A file whose kept span would hold n_fft // 2 samples
    or fewer is written whole (trim_batch's rule).  No checkpoint, no model.  Every header is read in load_data: an unreadable file or a
    foreign rate stops the run before anything is written."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.trim = dict(top_db=float(paras.trim_top_db), frame_length=int(paras.trim_frame_length), hop_length=int(paras.trim_hop),
                         pad_ms=float(paras.trim_pad_ms))

    def load_data(self):
        from .audio import load_audio_transform
        self.wav_dir, self.out_dir = self.paras.trim_wav_dir, self.paras.trim_out
        check_out_dir('--trim-out', self.out_dir, '--trim-wav-dir', self.wav_dir)
        self.files = list_wavs(self.wav_dir, '--trim-wav-dir')
        self.audio_converter = conv = load_audio_transform(**self.config['data']['audio'])
        conv._check_trim(**self.trim)
        for f in self.files:
            check_wav(self.wav_dir, f, '--trim-wav-dir', conv.sr)
        return self

    def exec(self):
        import csv
        from .audio import _read_pcm, write_pcm16
        conv = self.audio_converter
        os.makedirs(self.out_dir, exist_ok=True)
        t0, rows = time.perf_counter(), []
        for names in self.batches(self.files):
            pcm = [_read_pcm(os.path.join(self.wav_dir, f))[0][:, 0] for f in names]
            waves = [torch.from_numpy(p.astype(np.float32) / 32768.0) for p in pcm]
            _, bounds, _, intervals = conv.trim_batch(waves, with_intervals=True, **self.trim)
            for f, p, (a, b), iv in zip(names, pcm, bounds.tolist(), intervals):
                write_pcm16(os.path.join(self.out_dir, f), p[a:b], conv.sr)
                rows.append([f, len(p), a, b, '%.6f' % (len(p) / conv.sr), '%.6f' % ((b - a) / conv.sr), len(iv)])
        with open(os.path.join(self.out_dir, 'trim.csv'), 'w', newline='') as fh:
            out = csv.writer(fh)
            out.writerow(['file', 'samples', 'start', 'end', 'seconds', 'kept_seconds', 'n_intervals'])
            out.writerows(rows)
        if getattr(self.paras, 'verbose', True):
            total, kept = sum(r[1] for r in rows), sum(r[3] - r[2] for r in rows)
            print('[INFO]', 'Trimmed %d files into %s: %.1f s -> %.1f s, %.2f s' % (len(rows), self.out_dir, total / conv.sr, kept / conv.sr,
                                                                                  time.perf_counter() - t0))
        return len(rows)


def f0_args(paras):
    """the pitch tracker's settings from --f0-min / --f0-max / --f0-threshold (their defaults when the flags are absent)"""
    return dict(fmin=float(getattr(paras, 'f0_min', None) or 60.0), fmax=float(getattr(paras, 'f0_max', None) or 500.0),
                threshold=float(getattr(paras, 'f0_threshold', None) or 0.15))


class FeatureWriter(DirTool):
    """main.py --feat-wav-dir DIR --feat mfcc|mel|linear [--segment-file FILE --min-segment-len N]: channel 0 of the .wav files of DIR,
    sorted by name, in batches of --batch-size -> AudioConverter.extract_mfcc_batch (mfcc) or the clean extract_batch (mel, linear) ->
    <logdir>/<stem>-<feat>.npy, (frames, dim) float32.  With --segment-file each utterance is also cut at its row of that table
    (AudioConverter.segment_batch, one launch per batch) into <stem>-<feat>-seg.npy, (segments, its longest piece, dim): what
    AudioConverter.segment_features gives for the file.  No checkpoint, no model.  Every key is looked up in load_data: a file
    without a row stops the run before anything is written.
    --feat f0 [--f0-min 60 --f0-max 500 --f0-threshold 0.15]: AudioConverter.extract_f0_batch -> <stem>-f0.npy, (frames,) float32 in Hz at
    the MFCC hop, 0 where unvoiced; a pitch track has no phone segments: --segment-file with it is refused in load_data."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.feat = paras.feat
        self.f0_args = f0_args(paras)

    def load_data(self):
        from .audio import load_audio_transform
        self.wav_dir = self.paras.feat_wav_dir
        self.files = list_wavs(self.wav_dir, '--feat-wav-dir')
        audio = dict(self.config['data']['audio'])
        self.segment_file = getattr(self.paras, 'segment_file', None)
        if self.feat == 'f0' and self.segment_file is not None:
            raise ValueError('--feat f0 does not combine with --segment-file: a pitch track is not cut into phone segments')
        if self.segment_file is not None:
            audio.update(segment_file=self.segment_file, segment_feat=self.feat, min_segment_len=int(getattr(self.paras, 'min_segment_len', 2)))
        self.audio_converter = conv = load_audio_transform(**audio)
        if self.feat == 'linear' and not conv.use_linear:
            raise ValueError('--feat linear: data.audio.use_linear is off')
        if self.feat == 'f0':
            conv.f0_lags(self.f0_args['fmin'], self.f0_args['fmax'])       # (ValueError naming the limit)
        if self.segment_file is not None:
            for f in self.files:
                conv.boundary(f)                          # (KeyError naming the file)
        return self

    def extract(self, names):
        """the files `names` of the .wav directory -> (features (B, T_pad, D) on the device in the sorted order, frames per row, order)"""
        conv = self.audio_converter
        return extract_features(conv, load_waves(conv, self.wav_dir, names, self.paras), self.feat, self.f0_args)

    def exec(self):
        from .audio import segment_points
        os.makedirs(self.logdir, exist_ok=True)
        conv = self.audio_converter
        t0, n, n_seg = time.perf_counter(), 0, 0
        for names in self.batches(self.files):
            feats, frames, order = self.extract(names)
            rows = [names[k] for k in order]                         # the batch is sorted by length: row `row` is names[order[row]]
            host = feats.cpu().numpy()
            seg = counts = None
            if self.segment_file is not None:
                seg, counts = conv.segment_batch(feats, frames.tolist(), rows)
                seg, first = seg.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)])
            for row, f in enumerate(rows):
                stem = os.path.join(self.logdir, '%s-%s' % (os.path.splitext(f)[0], self.feat))
                np.save(stem + '.npy', host[row, :frames[row]], allow_pickle=False)
                if seg is not None:                                  # padded to the utterance's own longest piece, not the batch's
                    own = segment_points(conv.boundary(f), int(frames[row]), conv.min_segment_len)[1]
                    np.save(stem + '-seg.npy', seg[first[row]:first[row + 1], :own], allow_pickle=False)
                    n_seg += counts[row]
                n += 1
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', 'Wrote %s features of %d files%s into %s, %.2f s'
                  % (self.feat, n, '' if self.segment_file is None else ' (%d segments)' % n_seg, self.logdir, time.perf_counter() - t0))
        return n


MCD_PRED_SUFFIX = '-pred'           # what --gen-specgram --gen-wav appends to an utterance's name
MCD_MAX_BATCH = 64                  # pairs per st_dtw_batch call
MCD_HEADER = 'file,frames,ref_frames,path_len,mcd_db'
F0_HEADER = 'file,path_len,voiced_pairs,f0_rmse_cents,vuv_error,gross_error,mean_cents'
F0_FIGURES = ('f0_rmse_cents', 'vuv_error', 'gross_error', 'mean_cents')


def mcd_key(filename):
    """the key of a synthesised file: its name up to the first '.', without one trailing '-pred'"""
    key = os.path.basename(filename).split('.')[0]
    return key[:-len(MCD_PRED_SUFFIX)] if key.endswith(MCD_PRED_SUFFIX) else key


def mcd_pairs(syn_dir, ref_dir, flag='--mcd-wav-dir'):
    """the .wav files of syn_dir sorted by name, each with its recording <key>.wav of ref_dir -> [(file, key, recording)] (names, not
    paths).  ValueError naming the file when syn_dir holds none, a recording is missing or two files share one.  flag: the command-line
    flag the messages name (--stoi-wav-dir pairs by the same rule)."""
    pairs = []
    for f in list_wavs(syn_dir, flag):
        key = mcd_key(f)
        ref = key + '.wav'
        if not key or not os.path.isfile(os.path.join(ref_dir, ref)):
            raise ValueError('%s: %s has no recording %s' % (flag, f, os.path.join(ref_dir, ref)))
        if any(key == k for _, k, _ in pairs):
            raise ValueError('%s: %s and %s share the recording %s' % (flag, [g for g, k, _ in pairs if k == key][0], f, ref))
        pairs.append((f, key, ref))
    return pairs


class McdScorer(DirTool):
    """main.py --mcd-wav-dir SYN --mcd-ref-dir REF [--mcd-path]: every .wav of SYN (sorted by name) against REF/<key>.wav (mcd_key), in
    batches of --batch-size (at most 64 pairs a call) -> AudioConverter.extract_mfcc_batch on both sides -> metrics.mcd (DTW over the
    cepstra 1 .. 12, one launch) -> one host read per batch -> <logdir>/mcd.csv (MCD_HEADER, one row per pair) and, with --mcd-path,
    <logdir>/<key>.dtw.npy, the (path_len, 2) int32 warp (synthesised frame, recording frame).  No checkpoint, no model.  Every pair is
    looked up and every header read in load_data: a missing recording, an unreadable file, a foreign sample rate or an utterance
    the MFCC or the DTW kernel does not take stops the run, naming the file, before any device work.
    --mcd-f0 [--f0-min 60 --f0-max 500 --f0-threshold 0.15]: AudioConverter.extract_f0_batch on both sides as well, and
    metrics.f0_scores along the path of the same metrics.mcd call (requested with or without --mcd-path) -> <logdir>/f0.csv (F0_HEADER);
    the figures ride in the batch's one host read.  mcd.csv and the .dtw.npy files are what they are without the flag."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.want_f0 = bool(getattr(paras, 'mcd_f0', False))
        self.f0_args = f0_args(paras)

    def _check_file(self, path):
        conv = self.audio_converter
        sr, _, width, L = wav_header(path, '--mcd-wav-dir')
        if width != 2:
            raise ValueError('--mcd-wav-dir: %s is %d-bit; only 16-bit PCM is read' % (path, 8 * width))
        if sr != conv.sr:
            raise ValueError('--mcd-wav-dir: sample rate mismatch. Expected %d but get %d (%s)' % (conv.sr, sr, path))
        try:
            conv._check_mfcc([L])
        except ValueError as e:
            raise ValueError('--mcd-wav-dir: %s: %s' % (path, e))
        if mfcc_frames(conv, L) > toolops.DTW_MAX_T:
            raise ValueError('--mcd-wav-dir: %s has %d MFCC frames; the warp takes at most %d' % (path, mfcc_frames(conv, L), toolops.DTW_MAX_T))

    def load_data(self):
        from .audio import load_audio_transform
        self.syn_dir, self.ref_dir = self.paras.mcd_wav_dir, self.paras.mcd_ref_dir
        self.pairs = mcd_pairs(self.syn_dir, self.ref_dir)
        self.audio_converter = load_audio_transform(**dict(self.config['data']['audio']))
        if self.want_f0:
            self.audio_converter.f0_lags(self.f0_args['fmin'], self.f0_args['fmax'])       # (ValueError naming the limit)
        for f, _, ref in self.pairs:
            self._check_file(os.path.join(self.syn_dir, f))
            self._check_file(os.path.join(self.ref_dir, ref))
        return self

    def score(self, pairs, want_path=False):
        """the pairs [(file, key, recording)] in one call -> per pair, in the given order: (frames, ref_frames, path_len, mcd_db, path
        (path_len, 2) int32 or None), with --mcd-f0 followed by (voiced_pairs, f0_rmse_cents, vuv_error, gross_error, mean_cents); one
        host read"""
        from .metrics import f0_scores, mcd
        conv = self.audio_converter
        ws = load_waves(conv, self.syn_dir, [f for f, _, _ in pairs], self.paras)
        wr = load_waves(conv, self.ref_dir, [r for _, _, r in pairs], self.paras)
        fs, fr = mfcc_frames(conv, ws.lens), mfcc_frames(conv, wr.lens)
        cs, cr = conv.extract_mfcc_batch(ws), conv.extract_mfcc_batch(wr)
        # both batches are sorted by length: bring the recordings into the row order of the synthesised side
        perm = wr.inverse()[ws.order]
        cr = cr.index_select(0, torch.from_numpy(perm).to(cr.device))
        fr = fr[perm]
        db, plen, path = mcd(cs, fs.tolist(), cr, fr.tolist())
        B = len(pairs)
        cols = [db.view(torch.int32).reshape(B, 1), plen.reshape(B, 1)] + ([path.reshape(B, -1)] if want_path else [])
        if self.want_f0:                                            # the figures as trailing columns of the same read
            ps, pr = conv.extract_f0_batch(ws, **self.f0_args), conv.extract_f0_batch(wr, **self.f0_args)
            pr = pr.index_select(0, torch.from_numpy(perm).to(pr.device))
            sc = f0_scores(ps, pr, path, plen)
            cols += [sc['n_both'].reshape(B, 1)] + [sc[k].view(torch.int32).reshape(B, 1) for k in F0_FIGURES]
        host = torch.cat(cols, dim=1).cpu().numpy()                 # (the one host read)
        out = [None] * B
        for row, k in enumerate(ws.order):
            P = int(host[row, 1])
            out[k] = (int(fs[row]), int(fr[row]), P, float(host[row, :1].view(np.float32)[0]),
                      host[row, 2:2 + 2 * P].reshape(P, 2).copy() if want_path else None)
            if self.want_f0:
                tail = host[row, -5:]
                out[k] += (int(tail[0]),) + tuple(float(v) for v in tail[1:].view(np.float32))
        return out

    def exec(self):
        os.makedirs(self.logdir, exist_ok=True)
        want_path = bool(getattr(self.paras, 'mcd_path', False))
        t0, rows, vals = time.perf_counter(), [MCD_HEADER], []
        f0_rows, f0_vals = [F0_HEADER], []
        for pairs in self.batches(self.pairs, MCD_MAX_BATCH):
            for (f, key, _), res in zip(pairs, self.score(pairs, want_path)):
                n, m, P, db, path = res[:5]
                rows.append('%s,%d,%d,%d,%.4f' % (f, n, m, P, db))
                vals.append(db)
                if want_path:
                    np.save(os.path.join(self.logdir, key + '.dtw.npy'), path.astype(np.int32), allow_pickle=False)
                if self.want_f0:
                    f0_rows.append('%s,%d,%d,%.2f,%.4f,%.4f,%.2f' % ((f, P) + res[5:]))
                    f0_vals.append(res[6:])
        table = self.write_lines('mcd.csv', rows)
        self.mean_mcd = float(np.mean(vals))
        print('[INFO]', 'MCD-DTW of %d pairs: mean %.4f dB; %s, %.2f s' % (len(vals), self.mean_mcd, table, time.perf_counter() - t0))
        if self.want_f0:
            table = self.write_lines('f0.csv', f0_rows)
            with np.errstate(all='ignore'):                           # (a pair without a both-voiced frame has NaN figures: left out of the means)
                self.mean_f0 = dict(zip(F0_FIGURES, np.nanmean(np.asarray(f0_vals, np.float64), axis=0).tolist()))
            print('[INFO]', 'F0 along the warp: mean RMSE %.2f cents, V/UV error %.4f, gross error %.4f, mean deviation %.2f cents; %s'
                  % (tuple(self.mean_f0[k] for k in F0_FIGURES) + (table,)))
        return len(vals)


STOI_HEADER = 'file,samples,frames,kept,segments,stoi,estoi'
STOI_MAX_LEN_DIFF = 0.05            # seconds: r = 3 decoder frames of 12.5 ms plus the vocoder's lost partial hop
STOI_MAX_DELAY = 0.05               # seconds: --stoi-align's default search bound
DELAY_HEADER = 'file,delay_samples,delay_s,coef'
SDR_HEADER = 'file,samples,si_sdr,snr,gain_db'


def stoi_row(file, samples, counts, score):
    """one line of stoi.csv: counts = (frames, kept, band frames, segments), score = (stoi, estoi)"""
    return '%s,%d,%d,%d,%d,%.6f,%.6f' % (file, samples, counts[0], counts[1], counts[3], score[0], score[1])


class StoiScorer(DirTool):
    """main.py --stoi-wav-dir SYN --stoi-ref-dir REF [--stoi-max-len-diff 0.05]: every .wav of SYN (sorted by name) against REF/<key>.wav
    (mcd_key, the pairing of --mcd-wav-dir), in batches of --batch-size (at most 64 pairs a call) -> metrics.stoi (both sides resampled
    to 10 kHz on the device when the files are at another rate, then st_stoi_batch) -> one host read per batch -> <logdir>/stoi.csv
    (STOI_HEADER, one row per pair: the samples scored at the files' rate, the frames at 10 kHz, the frames kept, the segments, STOI,
    ESTOI).  The two files of a pair must be time-aligned: a vocoded spectrogram against its recording, not free-running synthesis --
    or shifted by a constant delay that --stoi-align [--stoi-max-delay 0.05] searches first (metrics.align_pairs: the overlap is scored,
    delay.csv written, a best lag on the bound warned about); --stoi-sdr adds sdr.csv (metrics.si_sdr).  Without those flags nothing changes.
    A pair whose lengths differ by at most --stoi-max-len-diff seconds is cut to the shorter side at its end.  A pair too short for one
    segment (under 30 band frames) gets the sentinel row (segments 0, both scores 1e-5), a warning naming it, and no part in the means.
    No config, no checkpoint, no model.  Every pair is looked up and every header read in load_data: a missing or shared recording, an
    unreadable, multichannel or non-16-bit file, two rates within a pair, a rate the resampler refuses, a larger length difference or a
    signal past the kernel's limit stops the run, naming the file, before any device work."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        d = getattr(paras, 'stoi_max_len_diff', None)
        self.max_len_diff = STOI_MAX_LEN_DIFF if d is None else float(d)
        self.align, self.sdr = bool(getattr(paras, 'stoi_align', False)), bool(getattr(paras, 'stoi_sdr', False))
        d = getattr(paras, 'stoi_max_delay', None)
        self.max_delay = (STOI_MAX_DELAY if d is None else float(d)) if self.align else 0.0

    @staticmethod
    def _header(path):
        sr, ch, width, L = wav_header(path, '--stoi-wav-dir')
        if width != 2 or ch != 1:
            raise ValueError('--stoi-wav-dir: %s is %d-bit with %d channels; only 16-bit mono PCM is read' % (path, 8 * width, ch))
        if L < 1:
            raise ValueError('--stoi-wav-dir: %s holds no samples' % path)
        return sr, L

    def load_data(self):
        from . import audio
        self.syn_dir, self.ref_dir = self.paras.stoi_wav_dir, self.paras.stoi_ref_dir
        self.pairs = mcd_pairs(self.syn_dir, self.ref_dir, '--stoi-wav-dir')
        self.rates, self.samples, self.lens = [], [], []
        for f, _, ref in self.pairs:
            ps, pr = os.path.join(self.syn_dir, f), os.path.join(self.ref_dir, ref)
            (sr, L), (sr_ref, L_ref) = self._header(ps), self._header(pr)
            if sr != sr_ref:
                raise ValueError('--stoi-wav-dir: %s is at %d Hz and its recording %s at %d Hz; the two files of a pair share one rate' % (ps, sr, pr, sr_ref))
            try:
                audio.resample_table(sr, toolops.STOI_FS)
            except ValueError as e:
                raise ValueError('--stoi-wav-dir: %s: %s' % (ps, e))
            if self.align:
                if not 0.0 <= self.max_delay < math.inf or self.max_delay * sr > toolops.XCORR_MAX_LAG:
                    raise ValueError('--stoi-align: %s is at %d Hz: --stoi-max-delay %g must be finite, at least 0 and at most %d samples = %.4f s at '
                                     'that rate' % (ps, sr, self.max_delay, toolops.XCORR_MAX_LAG, toolops.XCORR_MAX_LAG / float(sr)))
                if abs(L - L_ref) > (self.max_len_diff + self.max_delay) * sr:
                    raise ValueError('--stoi-wav-dir: %s has %d samples and its recording %s %d: they differ by %.4f s, above --stoi-max-len-diff %g '
                                     'plus --stoi-max-delay %g' % (ps, L, pr, L_ref, abs(L - L_ref) / float(sr), self.max_len_diff, self.max_delay))
            elif abs(L - L_ref) > self.max_len_diff * sr:
                raise ValueError('--stoi-wav-dir: %s has %d samples and its recording %s %d: they differ by %.4f s, above --stoi-max-len-diff %g; '
                                 'the measure needs time-aligned signals' % (ps, L, pr, L_ref, abs(L - L_ref) / float(sr), self.max_len_diff))
            n = min(L, L_ref)
            if audio.resampled_len(n, sr, toolops.STOI_FS) > toolops.STOI_MAX_LEN:
                raise ValueError('--stoi-wav-dir: %s has %d samples at %d Hz; the measure takes at most %d' % (ps, audio.resampled_len(n, sr, toolops.STOI_FS),
                                                                                                        toolops.STOI_FS, toolops.STOI_MAX_LEN))
            if (self.align or self.sdr) and max(L, L_ref) > toolops.XCORR_MAX_LEN:
                raise ValueError('--stoi-wav-dir: %s and its recording have up to %d samples; --stoi-align and --stoi-sdr take at most %d'
                                 % (ps, max(L, L_ref), toolops.XCORR_MAX_LEN))
            self.rates.append(sr)
            self.samples.append(n)
            self.lens.append((L, L_ref))
        return self

    def lag(self, sr):
        """--stoi-max-delay in samples at this rate"""
        return int(math.floor(self.max_delay * sr + 1e-6))

    def score(self, lo, hi):
        """pairs [lo, hi) -> per pair (counts (4,) int32, score (2,) float32, delay, coef, sdr (3,) float32), one metrics.stoi call per
        sample rate among them and one host read of the scores.  Without --stoi-align and --stoi-sdr the two lists of waveforms go to
        metrics.stoi as they are and the last three fields are 0, NaN and NaNs of the host.  With either flag the files of a rate are
        uploaded once; the delay search (one host read of the delays inside metrics.align_pairs), the gather of the overlaps,
        metrics.stoi on the cut batches and metrics.si_sdr all read the device buffers."""
        from . import audio, metrics
        plain = not (self.align or self.sdr)
        idx, cols = [], []
        for sr in sorted(set(self.rates[lo:hi])):
            sel = [i for i in range(lo, hi) if self.rates[i] == sr]
            syn, rec = [], []
            for i in sel:
                f, _, ref = self.pairs[i]
                L, L_ref = self.lens[i] if self.align else (self.samples[i], self.samples[i])
                syn.append(audio.read_wav(os.path.join(self.syn_dir, f))[0][0, :L])
                rec.append(audio.read_wav(os.path.join(self.ref_dir, ref))[0][0, :L_ref])
            if plain:
                res = metrics.stoi(rec, syn, sr)
                cols.append(torch.cat([res.counts, res.score.view(torch.int32)], dim=1))
            else:
                syn, rec = audio.WaveBatch(syn), audio.WaveBatch(rec)
                dev = audio._device()
                syn.packed(dev), rec.packed(dev)                        # (the one upload of each side)
                syn.device = rec.device = dev
                if self.align:
                    cut_rec, cut_syn, dl, coef = metrics.align_pairs(rec, syn, self.lag(sr))
                else:
                    cut_rec, cut_syn = rec, syn
                    dl, coef = torch.zeros(len(sel), device=dev, dtype=torch.int32), torch.full((len(sel),), math.nan, device=dev)
                res = metrics.stoi(cut_rec, cut_syn, sr)
                sdr = metrics.si_sdr(rec, syn, dl if self.align else None).score if self.sdr else torch.full((len(sel), 3), math.nan, device=dev)
                cols.append(torch.cat([res.counts, res.score.view(torch.int32), dl.view(-1, 1), coef.view(torch.int32).view(-1, 1),
                                       sdr.view(torch.int32)], dim=1))
            idx += sel
        host = torch.cat(cols, dim=0).cpu().numpy()                     # (the one host read of the scores)
        out = [None] * (hi - lo)
        for row, i in enumerate(idx):
            d, coef, sdr = 0, math.nan, np.full(3, math.nan, np.float32)
            if not plain:
                d, coef, sdr = int(host[row, 6]), float(host[row, 7:8].copy().view(np.float32)[0]), host[row, 8:11].copy().view(np.float32)
            out[i - lo] = (host[row, :4].copy(), host[row, 4:6].copy().view(np.float32), d, coef, sdr)
        return out

    def exec(self):
        """stoi.csv, on the scored samples (with --stoi-align: the overlap); delay.csv with --stoi-align, sdr.csv with --stoi-sdr"""
        from .metrics import overlap
        os.makedirs(self.logdir, exist_ok=True)
        t0, rows, vals, drows, srows, delays, sdrs = time.perf_counter(), [STOI_HEADER], [], [DELAY_HEADER], [SDR_HEADER], [], []
        for r in self.batches(range(len(self.pairs)), toolops.STOI_MAX_BATCH):
            for i, (counts, score, d, coef, sdr) in zip(r, self.score(r.start, r.stop)):
                f, sr = self.pairs[i][0], self.rates[i]
                if self.align:
                    self.samples[i] = overlap(self.lens[i][1], self.lens[i][0], d)[2]
                    drows.append('%s,%d,%.6f,%.6f' % (f, d, d / float(sr), coef))
                    delays.append(abs(d) / float(sr))
                    if self.lag(sr) > 0 and abs(d) == self.lag(sr):
                        print('[WARNING]', '--stoi-align: the best lag of %s, %d samples, sits on the search bound of +-%d samples (--stoi-max-delay %g): '
                              'the true delay may lie outside it' % (f, d, self.lag(sr), self.max_delay))
                if self.sdr:
                    srows.append('%s,%d,%.4f,%.4f,%.4f' % (f, self.samples[i], sdr[0], sdr[1], sdr[2]))
                    sdrs.append(float(sdr[0]))
                rows.append(stoi_row(f, self.samples[i], counts, score))
                if counts[3] == 0 and not np.isnan(score[0]):
                    print('[WARNING]', '--stoi-wav-dir: %s has %d band frames, fewer than the %d of one segment: the sentinel %g is written and '
                          'the file is left out of the means' % (f, counts[2], toolops.STOI_SEG, toolops.STOI_SENTINEL))
                else:
                    vals.append(score)
        table = self.write_lines('stoi.csv', rows)
        self.mean_stoi, self.mean_estoi = (float(v) for v in np.mean(np.asarray(vals, np.float64), axis=0)) if vals else (math.nan, math.nan)
        extra = ''
        if self.align:
            self.write_lines('delay.csv', drows)
            self.mean_abs_delay = float(np.mean(delays)) if delays else math.nan
            extra += ', mean |delay| %.6f s' % self.mean_abs_delay
        if self.sdr:
            self.write_lines('sdr.csv', srows)
            finite = [v for v in sdrs if math.isfinite(v)]
            self.mean_si_sdr = float(np.mean(finite)) if finite else math.nan
            extra += ', mean SI-SDR %.2f dB over %d finite' % (self.mean_si_sdr, len(finite))
        print('[INFO]', 'STOI of %d pairs (%d scored): mean STOI %.4f, mean ESTOI %.4f%s; %s, %.2f s'
              % (len(self.pairs), len(vals), self.mean_stoi, self.mean_estoi, extra, table, time.perf_counter() - t0))
        return len(self.pairs)


ABX_FEATS = ('mfcc', 'mel', 'latent', 'code')


class FeatureTool(DirTool):
    """What the tools that score or cluster a representation share (AbxScorer, KMeansTrainer, UnitWriter): the representation `self.feat`
    -- mfcc: AudioConverter.extract_mfcc_batch, mel: the clean extract_batch, neither needs a checkpoint or a model; latent / code:
    VQVAE.represent of the model of --load, or of the synthetic weights -- of the files of `self.wav_dir`, sorted by name, in batches of
    --batch-size, packed into one (rows, D) device buffer.  load_data sets self.wav_dir and self.audio_converter."""

    def check_waves(self, wavs, flag):
        """the headers of the files `wavs` of self.wav_dir: a rate other than the converter's needs --resample, and an utterance the MFCC
        kernel refuses stops the run here, naming `flag` and the file -> the samples of every file at the converter's rate"""
        from .audio import resampled_len
        conv, samples = self.audio_converter, []
        for w in wavs:
            path = os.path.join(self.wav_dir, w)
            sr, _, _, L = wav_header(path, flag)
            if sr != conv.sr and not getattr(self.paras, 'resample', False):
                raise ValueError('%s: sample rate mismatch. Expected %d but get %d (%s); --resample converts it' % (flag, conv.sr, sr, path))
            if self.feat == 'mfcc' and sr == conv.sr:
                try:
                    conv._check_mfcc([L])
                except ValueError as e:
                    raise ValueError('%s: %s: %s' % (flag, path, e))
            samples.append(L if sr == conv.sr else resampled_len(L, sr, conv.sr))
        return samples

    def set_model(self):
        self.model = None
        if self.feat in ('latent', 'code'):
            from .solver import Transcriber
            self.model = Transcriber(self.config, self.paras, self.mode).set_model().model
        return self

    def frame_s(self):
        conv = self.audio_converter
        if self.feat == 'mfcc':
            return conv.hop_length_mfcc / float(conv.sr)
        if self.feat == 'mel':
            return conv.hop_length / float(conv.sr)
        return self.model.time_reduce_factor * conv.hop_length / float(conv.sr)

    def feature_rows(self, samples):
        """an upper bound of the rows of an utterance of `samples` samples (trimming and the encoder's time reduction only shorten it)"""
        conv = self.audio_converter
        return 1 + samples // (conv.hop_length_mfcc if self.feat == 'mfcc' else conv.hop_length)

    def feature_dim(self):
        """the columns of the representation; None for latent / code before the model is built"""
        from .audio import MFCC_DIM
        if self.feat in ('mfcc', 'mel'):
            return MFCC_DIM if self.feat == 'mfcc' else self.audio_converter.n_mels
        return None

    def extract(self, names):
        """the files `names` of the .wav directory -> (features (B, T_pad, D) on the device in the batch's sorted order, rows per
        utterance, the WaveBatch's inverse: the batch row of the k-th given file)"""
        conv = self.audio_converter
        wb = load_waves(conv, self.wav_dir, names, self.paras, resample=bool(getattr(self.paras, 'resample', False)))
        feats, frames, _ = extract_features(conv, wb, 'mfcc' if self.feat == 'mfcc' else 'mel')
        if self.feat in ('latent', 'code'):
            feats, frames = self.model.represent(feats, frames, self.feat)
            frames = frames.numpy()
        return feats, frames, wb.inverse()

    def pack(self, wavs):
        """-> (the packed (rows, D) device buffer of the files `wavs`, the first row of every file, its rows), files in the given order"""
        parts, n_rows = [], []
        for names in self.batches(wavs, math.inf):
            feats, frames, back = self.extract(list(names))
            for k in range(len(names)):
                r = int(min(int(frames[back[k]]), feats.shape[1]))
                parts.append(feats[back[k], :r])
                n_rows.append(r)
        first = np.concatenate([[0], np.cumsum(n_rows)[:-1]]).astype(np.int64)
        return torch.cat(parts, 0).float().contiguous(), first, np.asarray(n_rows, np.int64)


def load_codebook(flag, path, D=None):
    """a (K, D) float32 table of centroids from the .npy file of `flag` (what --kmeans-out writes); ValueError naming the flag for a file
    that is no such table, that holds a non-finite entry or, with D, whose rows are not D wide"""
    try:
        table = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise ValueError('%s %s: not a readable .npy file (%s)' % (flag, path, e))
    if table.ndim != 2 or table.dtype != np.float32 or not 1 <= table.shape[0] <= toolops.KM_MAX_K or not 1 <= table.shape[1] <= toolops.KM_MAX_D:
        raise ValueError('%s %s: a codebook is a (K, D) float32 array with K <= %d and D <= %d (got %s %s)'
                         % (flag, path, toolops.KM_MAX_K, toolops.KM_MAX_D, table.shape, table.dtype))
    if not np.isfinite(table).all():
        raise ValueError('%s %s: the codebook holds a non-finite entry' % (flag, path))
    if D is not None and table.shape[1] != D:
        raise ValueError('%s %s: the codebook has D = %d columns, the features have %d' % (flag, path, table.shape[1], D))
    return np.ascontiguousarray(table)


def abx_metric(paras):
    """--abx-metric, or its default: kl for the codebook posteriors (probability rows), angular for everything else"""
    return getattr(paras, 'abx_metric', None) or ('kl' if getattr(paras, 'abx_feat', 'mfcc') == 'code' else 'angular')


class AbxScorer(FeatureTool):
    """main.py --abx-ali-dir DIR --abx-wav-dir WAVS [--abx-feat mfcc|mel|latent|code --abx-metric angular|kl|euclid --abx-context
    triphone|none --abx-spk-map FILE --abx-ignore a,b --abx-max-items 50 --abx-min-frames 1]: the ABX phone-discrimination error of a
    representation, within speaker (semi_tts_amd.abx for the terms, metrics.abx for the computation).  Every <stem>.ali of DIR (what
    --align-wav-dir writes) names the phone boundaries of WAVS/<stem>.wav.  The features of the files (sorted by name, batches of
    --batch-size) are extracted on the GPU -- mfcc: AudioConverter.extract_mfcc_batch, mel: the clean extract_batch, neither needs a
    checkpoint or a model; latent / code: VQVAE.represent of the model of --load, or of the synthetic weights -- and packed into one
    (rows, D) device buffer; every token becomes an item of that buffer (abx.utterance_items at the feature's frame period:
    hop_length_mfcc / sr, hop_length / sr, time_reduce_factor hop_length / sr), keyed into cells by speaker and context; one
    metrics.abx call scores them.  -> <logdir>/<name>/abx.csv (phone_a,phone_b,cells,triples,error) and abx_phones.csv
    (phone,tokens,items,too_short,too_long), and one printed line.  A missing waveform, a malformed .ali, an .ali without tokens or a file
    the speaker map lacks stops the run in load_data, naming the file, before any device work.
    --abx-mode across | both (with --abx-spk-map, at least two speakers) scores the same features and items across speakers as well
    (metrics.abx_across, matrices and pair tables up to --abx-max-gb): abx_across.csv (phone_a,phone_b,groups,triples,error),
    abx_across_speakers.csv (speaker,groups,error) and a printed line of its own; `across` alone leaves abx.csv unwritten.
    --abx-codebook FILE.npy (a (K, D) table of --kmeans-out) replaces every feature row by its nearest centroid before the items are cut:
    the discrete-unit ABX of ZeroSpeech."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.feat = getattr(paras, 'abx_feat', None) or 'mfcc'
        self.metric = abx_metric(paras)
        self.context = getattr(paras, 'abx_context', None) or 'triphone'
        self.ignore = tuple(getattr(paras, 'abx_ignore', None) or ())
        self.max_items = int(getattr(paras, 'abx_max_items', None) or 50)
        self.min_frames = int(getattr(paras, 'abx_min_frames', None) or 1)
        self.abx_mode = getattr(paras, 'abx_mode', None) or 'within'
        self.max_bytes = int(float(getattr(paras, 'abx_max_gb', None) or 8) * (1 << 30))
        self.codebook_file = getattr(paras, 'abx_codebook', None)

    def load_data(self):
        from . import abx as A
        from .audio import load_audio_transform
        self.ali_dir, self.wav_dir = self.paras.abx_ali_dir, self.paras.abx_wav_dir
        self.pairs = A.ali_pairs(self.ali_dir, self.wav_dir)
        self.alis = [A.read_ali(os.path.join(self.ali_dir, f)) for f, _, _ in self.pairs]
        spk_map = getattr(self.paras, 'abx_spk_map', None)
        self.speakers = ['spk'] * len(self.pairs)
        if spk_map:
            table = A.read_spk_map(spk_map)
            for k, (f, stem, _) in enumerate(self.pairs):
                key = stem if stem in table else stem.split('.')[0]
                if key not in table:
                    raise ValueError('--abx-spk-map %s has no row for %s' % (spk_map, f))
                self.speakers[k] = table[key]
        if self.abx_mode != 'within' and len(set(self.speakers)) < 2:
            raise ValueError('--abx-mode %s needs --abx-spk-map FILE with at least two speakers among the files (got %s)'
                             % (self.abx_mode, 'no map' if not spk_map else '%d speaker' % len(set(self.speakers))))
        self.audio_converter = load_audio_transform(**dict(self.config['data']['audio']))
        self.check_waves([w for _, _, w in self.pairs], '--abx-wav-dir')
        self.codebook = None
        if self.codebook_file is not None:
            if self.feat == 'code':
                raise ValueError('--abx-codebook quantises feature rows; --abx-feat code scores probability rows and has no use for it')
            self.codebook = load_codebook('--abx-codebook', self.codebook_file, self.feature_dim())
        return self

    def features(self):
        """-> (the packed (rows, D) device buffer of all files, the first row of every file, its rows), files in the order of self.pairs;
        with --abx-codebook every row is replaced by its nearest centroid (kmeans.quantise, then index_select)"""
        feat, first, n_rows = self.pack([w for _, _, w in self.pairs])
        if self.codebook is not None:
            from .kmeans import quantise
            if self.codebook.shape[1] != feat.shape[1]:
                raise ValueError('--abx-codebook %s: the codebook has D = %d columns, the features have %d'
                                 % (self.codebook_file, self.codebook.shape[1], feat.shape[1]))
            table = torch.from_numpy(self.codebook).to(feat.device)
            idx, _ = quantise(feat, table)
            if int((idx < 0).sum().item()):                            # (a row without a unit has no centroid to stand for it)
                raise ValueError('--abx-codebook: %d feature rows hold a NaN or an infinity and have no nearest centroid' % int((idx < 0).sum().item()))
            feat = table.index_select(0, idx.long()).contiguous()
        return feat, first, n_rows

    def items(self, first, n_rows):
        """-> (item_start, item_len, label ids, cell ids, the phone names of the label ids, stats per phone)"""
        from . import abx as A
        fs = self.frame_s()
        rows, stats = [], {}
        for k, ali in enumerate(self.alis):
            its, st = A.utterance_items(ali, fs, int(n_rows[k]), self.ignore, self.min_frames)
            for sym, v in st.items():
                stats[sym] = [a + b for a, b in zip(stats.get(sym, [0, 0, 0, 0]), v)]
            rows += [(sym, int(first[k]) + r0, n, A.cell_key(self.speakers[k], prev, nxt, self.context)) for sym, r0, n, prev, nxt in its]
        names = sorted({r[0] for r in rows})
        cells = {c: i for i, c in enumerate(sorted({r[3] for r in rows}))}
        lab = {s: i for i, s in enumerate(names)}
        self.item_keys = [r[3] for r in rows]                       # (speaker, previous, next) or (speaker,): what exec_across splits
        return (np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.int64), np.array([lab[r[0]] for r in rows], np.int64),
                np.array([cells[r[3]] for r in rows], np.int64), names, stats)

    def exec(self):
        from . import abx as A
        from .metrics import abx
        t0 = time.perf_counter()
        feat, first, n_rows = self.features()
        start, length, label, cell, names, stats = self.items(first, n_rows)
        if self.abx_mode != 'within' and len({k[0] for k in self.item_keys}) < 2:
            raise ValueError('--abx-mode %s: the kept items come from fewer than two speakers; --abx-spk-map must name at least two' % self.abx_mode)
        os.makedirs(self.logdir, exist_ok=True)
        if self.abx_mode == 'across':
            with open(os.path.join(self.logdir, 'abx_phones.csv'), 'w') as f:
                f.write(A.format_phones_csv(stats))
            return self.exec_across(feat, start, length, label, names)
        self.result = res = abx(feat, start, length, label, cell, self.metric, self.max_items, int(getattr(self.paras, 'seed', 0)))
        with open(os.path.join(self.logdir, 'abx.csv'), 'w') as f:
            f.write(A.format_abx_csv(res.table, names))
        with open(os.path.join(self.logdir, 'abx_phones.csv'), 'w') as f:
            f.write(A.format_phones_csv(stats))
        print('[INFO]', 'ABX error of %s (%s, context %s): %.2f %% over %d phone pairs, %d triples, %d pairs of DTW; %s, %.2f s'
              % (self.feat, self.metric, self.context, 100.0 * res.score, len(res.table), sum(r[3] for r in res.table), res.pairs,
                 os.path.join(self.logdir, 'abx.csv'), time.perf_counter() - t0))
        if self.abx_mode == 'both':
            self.exec_across(feat, start, length, label, names)
        return len(res.table)

    def exec_across(self, feat, start, length, label, names):
        """the across-speaker score of the items of exec: abx_across.csv, abx_across_speakers.csv and one printed line"""
        from . import abx as A
        from .metrics import abx_across
        t0 = time.perf_counter()
        spk_names = sorted({k[0] for k in self.item_keys})
        ctx = {c: i for i, c in enumerate(sorted({k[1:] for k in self.item_keys}))}
        spk = {s: i for i, s in enumerate(spk_names)}
        speaker = np.array([spk[k[0]] for k in self.item_keys], np.int64)
        context = np.array([ctx[k[1:]] for k in self.item_keys], np.int64)
        self.result_across = res = abx_across(feat, start, length, label, context, speaker, self.metric, self.max_items,
                                              int(getattr(self.paras, 'seed', 0)), self.max_bytes)
        with open(os.path.join(self.logdir, 'abx_across.csv'), 'w') as f:
            f.write(A.format_abx_across_csv(res.table, names))
        with open(os.path.join(self.logdir, 'abx_across_speakers.csv'), 'w') as f:
            f.write(A.format_abx_across_speakers_csv(res.speakers, spk_names))
        print('[INFO]', 'across-speaker ABX error of %s (%s, context %s): %.2f %% over %d phone pairs, %d groups, %d triples, %d pairs of DTW; %s, %.2f s'
              % (self.feat, self.metric, self.context, 100.0 * res.score, len(res.table), sum(r[2] for r in res.table),
                 sum(r[3] for r in res.table), res.pairs, os.path.join(self.logdir, 'abx_across.csv'), time.perf_counter() - t0))
        return len(res.table)


SCORE_MAX_BATCH = 64                # utterances per st_edit_align call
SCORE_DEFAULT_IGNORE = (0, 1, 2)    # --score-ignore: the special tokens (cal_per's filter also drops id 42)
PER_HEADER = 'file,ref_tokens,hyp_tokens,correct,sub,del,ins,per'
PER_NBEST_HEADER = PER_HEADER + ',nbest_per,nbest_path'
CONFUSIONS_HEADER = 'ref,hyp,count'
PHONES_HEADER = 'phone,ref_count,correct,sub,del,ins_as_hyp'


def phn_pairs(hyp_dir, ref_dir):
    """the .phn files of hyp_dir sorted by name, each with its reference <key>.phn of ref_dir (key: mcd_key, so x-pred.phn scores
    against x.phn) -> [(file, key, reference)] (names, not paths).  ValueError naming the file when hyp_dir holds none, a reference is
    missing or two files share one."""
    files = sorted(f for f in os.listdir(hyp_dir) if f.lower().endswith('.phn'))
    if not files:
        raise ValueError('--score-phn-dir %s: no .phn files' % hyp_dir)
    pairs, seen = [], {}
    for f in files:
        key = mcd_key(f)
        ref = key + '.phn'
        if not key or not os.path.isfile(os.path.join(ref_dir, ref)):
            raise ValueError('--score-phn-dir: %s has no reference %s' % (f, os.path.join(ref_dir, ref)))
        if key in seen:
            raise ValueError('--score-phn-dir: %s and %s share the reference %s' % (seen[key], f, ref))
        seen[key] = f
        pairs.append((f, key, ref))
    return pairs


def _phone(vocab, t):
    return vocab[t] if vocab is not None and 0 <= t < len(vocab) else str(t)


def per_row(file, counts, nbest=None):
    """one row of per.csv: counts = (correct, sub, del, ins) of the scored path; nbest = (lowest dist over the paths, its path) or None"""
    c, s, d, i = (int(v) for v in counts)
    n = c + s + d
    row = '%s,%d,%d,%d,%d,%d,%d,%s' % (file, n, c + s + i, c, s, d, i, '%.6f' % ((s + d + i) / n) if n else 'nan')
    if nbest is not None:
        row += ',%s,%d' % ('%.6f' % (int(nbest[0]) / n) if n else 'nan', int(nbest[1]))
    return row


def format_confusions(conf, vocab=None):
    """the text of confusions.csv from the (V + 1, V + 1) matrix: every non-zero cell off the diagonal, the deletion column as <del> and
    the insertion row as <ins>, by count descending, then reference id, then hypothesis id"""
    conf = np.asarray(conf)
    V = conf.shape[0] - 1
    a, b = np.nonzero(conf)
    keep = a != b
    a, b = a[keep], b[keep]
    cnt = conf[a, b]
    lines = [CONFUSIONS_HEADER]
    for k in np.lexsort((b, a, -cnt)):
        lines.append('%s,%s,%d' % ('<ins>' if a[k] == V else _phone(vocab, int(a[k])), '<del>' if b[k] == V else _phone(vocab, int(b[k])), cnt[k]))
    return '\n'.join(lines) + '\n'


def format_phones(conf, vocab=None):
    """the text of phones.csv: one row per class that occurs on either side -- how often it stands in a reference, and how often that was
    correct, substituted or deleted; how often it was inserted"""
    conf = np.asarray(conf)
    V = conf.shape[0] - 1
    lines = [PHONES_HEADER]
    for t in range(V):
        n_ref = int(conf[t].sum())
        if n_ref == 0 and int(conf[:, t].sum()) == 0:
            continue
        ok, dele = int(conf[t, t]), int(conf[t, V])
        lines.append('%s,%d,%d,%d,%d,%d' % (_phone(vocab, t), n_ref, ok, n_ref - ok - dele, dele, int(conf[V, t])))
    return '\n'.join(lines) + '\n'


def format_ops(ali, vocab=None):
    """the text of one <key>.ops file from the aligned pairs (ali_len, 2): three lines REF: / HYP: / OP: whose columns line up -- the
    symbols (or ids) padded to the wider of the two, * for a gap, and C S D I"""
    cols = [[], [], []]
    for r, h in np.asarray(ali).reshape(-1, 2).tolist():
        x, y = ('*' if r < 0 else _phone(vocab, r)), ('*' if h < 0 else _phone(vocab, h))
        op = 'I' if r < 0 else 'D' if h < 0 else 'C' if r == h else 'S'
        w = max(len(x), len(y))
        for col, text in zip(cols, (x, y, op)):
            col.append(text.ljust(w))
    return ''.join((tag + ' '.join(col)).rstrip() + '\n' for tag, col in zip(('REF: ', 'HYP: ', 'OP:  '), cols))


class PhnScorer(DirTool):
    """main.py --score-phn-dir HYP --score-ref-dir REF [--vocab FILE --score-ignore 0,1,2 --score-nbest --score-ali]: every .phn of HYP
    (sorted by name) against REF/<key>.phn (mcd_key), in batches of --batch-size (at most 64 utterances a call) ->
    metrics.align_transcripts (st_edit_align: the Levenshtein alignment with its trace-back, one launch) -> one host read per batch ->
    <logdir>/per.csv (PER_HEADER), confusion.npy (int64 (V + 1, V + 1): [r, h] pairs, column V deletions, row V insertions),
    confusions.csv, phones.csv and, with --score-ali, <key>.ops.  The confusion matrix stays on the device across the run and is read
    once at the end.  Without --score-nbest the first line of a hypothesis file is scored; with it every line (the paths of
    --top-paths), and per.csv gains the lowest error over the paths and the first path that attains it (a file with fewer paths than
    the widest of its batch is filled up with copies of its first).  V = the size of --vocab, or 1 + the largest id seen.  No config,
    no checkpoint, no model.  Every file is paired and read in load_data: a missing or shared reference, an unreadable file or an
    unknown symbol stops the run, naming the file, before any device work."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.nbest = bool(getattr(paras, 'score_nbest', False))
        self.want_ali = bool(getattr(paras, 'score_ali', False))
        ignore = getattr(paras, 'score_ignore', None)
        self.ignore = SCORE_DEFAULT_IGNORE if ignore is None else tuple(int(t) for t in ignore)

    def load_data(self):
        from .ctc_align import read_phn, read_phn_paths
        from .solver import read_vocab
        self.hyp_dir, self.ref_dir = self.paras.score_phn_dir, self.paras.score_ref_dir
        self.pairs = phn_pairs(self.hyp_dir, self.ref_dir)
        vocab_file = getattr(self.paras, 'vocab', None)
        try:
            self.vocab = read_vocab(vocab_file) if vocab_file else None
        except (OSError, UnicodeDecodeError) as e:
            raise ValueError('--vocab %s: cannot read the vocabulary (%s)' % (vocab_file, e))
        self.hyps, self.refs, top = [], [], -1
        for f, _, ref in self.pairs:
            paths = read_phn_paths(os.path.join(self.hyp_dir, f), self.vocab)
            self.hyps.append(paths if self.nbest else paths[:1])
            self.refs.append(read_phn(os.path.join(self.ref_dir, ref), self.vocab))
            top = max([top] + self.refs[-1] + [t for p in self.hyps[-1] for t in p])
        self.n_classes = len(self.vocab) if self.vocab is not None else max(1, top + 1)
        if self.n_classes > toolops.EA_MAX_V:
            raise ValueError('--score-phn-dir: %d classes (%s); the confusion matrix takes at most %d'
                             % (self.n_classes, 'the size of --vocab' if self.vocab is not None else '1 + the largest id', toolops.EA_MAX_V))
        if len(self.ignore) > toolops.EA_MAX_IGNORE:
            raise ValueError('--score-ignore: %d ids, at most %d' % (len(self.ignore), toolops.EA_MAX_IGNORE))
        return self

    def score(self, lo, hi):
        """utterances [lo, hi) in one call, their path 0 added into self.confusion -> per utterance (counts (N, 4) int32, (lowest dist,
        its path) or None, ali (ali_len, 2) int32 of path 0 or None); one host read"""
        from .metrics import align_transcripts, nbest_per
        hyps, refs = self.hyps[lo:hi], self.refs[lo:hi]
        B, N = len(hyps), max(len(p) for p in hyps)
        Lh, Lr = max(1, max(len(t) for p in hyps for t in p)), max(1, max(len(r) for r in refs))
        hyp, ref = np.zeros((B, N, Lh), np.int64), np.zeros((B, Lr), np.int64)
        hyp_len, ref_len = np.zeros((B, N), np.int32), np.zeros(B, np.int32)
        for b, (paths, r) in enumerate(zip(hyps, refs)):
            ref[b, :len(r)], ref_len[b] = r, len(r)
            for k in range(N):
                t = paths[k] if k < len(paths) else paths[0]
                hyp[b, k, :len(t)], hyp_len[b, k] = t, len(t)
        dev = self.confusion.device
        res = align_transcripts(torch.from_numpy(hyp).to(dev), hyp_len.tolist(), torch.from_numpy(ref).to(dev), ref_len.tolist(),
                                ignore=self.ignore, confusion=self.confusion, want_ali=self.want_ali)
        cols = [torch.stack([res.correct, res.sub, res.dele, res.ins], dim=-1).reshape(B, 4 * N)]
        if self.nbest:
            nb = nbest_per(res.dist)
            cols += [nb.dist.reshape(B, 1), nb.path.to(torch.int32).reshape(B, 1)]
        if self.want_ali:
            cols += [res.ali_len[:, :1], res.ali[:, 0].reshape(B, -1)]
        host = torch.cat(cols, dim=1).cpu().numpy()                 # (the one host read)
        out = []
        for b in range(B):
            row = host[b]
            nb = (int(row[4 * N]), int(row[4 * N + 1])) if self.nbest else None
            ali = None
            if self.want_ali:
                o = 4 * N + (2 if self.nbest else 0)
                ali = row[o + 1:o + 1 + 2 * int(row[o])].reshape(-1, 2).copy()
            out.append((row[:4 * N].reshape(N, 4).copy(), nb, ali))
        return out

    def exec(self):
        os.makedirs(self.logdir, exist_ok=True)
        V = self.n_classes
        self.confusion = torch.zeros(V + 1, V + 1, device=torch.device('cuda', torch.cuda.current_device()), dtype=torch.int32)
        t0, rows = time.perf_counter(), [PER_NBEST_HEADER if self.nbest else PER_HEADER]
        tot, best_tot, rates = np.zeros(4, np.int64), 0, []
        for r in self.batches(range(len(self.pairs)), SCORE_MAX_BATCH):
            for (f, key, _), (counts, nb, ali) in zip(self.pairs[r.start:r.stop], self.score(r.start, r.stop)):
                rows.append(per_row(f, counts[0], nb))
                tot += counts[0]
                n = int(counts[0][:3].sum())
                if n:
                    rates.append(float(counts[0][1:].sum()) / n)
                if nb is not None:
                    best_tot += nb[0]
                if ali is not None:
                    with open(os.path.join(self.logdir, key + '.ops'), 'w') as fh:
                        fh.write(format_ops(ali, self.vocab))
        conf = self.confusion.cpu().numpy().astype(np.int64)        # (the one read of the matrix)
        self.confusion_host = conf
        np.save(os.path.join(self.logdir, 'confusion.npy'), conf, allow_pickle=False)
        table = self.write_lines('per.csv', rows)
        for name, text in (('confusions.csv', format_confusions(conf, self.vocab)), ('phones.csv', format_phones(conf, self.vocab))):
            with open(os.path.join(self.logdir, name), 'w') as fh:
                fh.write(text)
        n_ref = int(tot[:3].sum())
        share = lambda v: float(v) / n_ref if n_ref else math.nan
        self.corpus_per, self.mean_per = share(tot[1:].sum()), float(np.mean(rates)) if rates else math.nan
        self.oracle_per = share(best_tot) if self.nbest else None
        print('[INFO]', 'PER of %d transcripts (%d reference phones): corpus %.4f, mean per utterance %.4f; sub %.4f, del %.4f, ins %.4f%s; %s, %.2f s'
              % (len(self.pairs), n_ref, self.corpus_per, self.mean_per, share(tot[1]), share(tot[2]), share(tot[3]),
                 '; n-best oracle %.4f' % self.oracle_per if self.nbest else '', table, time.perf_counter() - t0))
        return len(self.pairs)


# -- k-means units
UNIT_FEATS = ('mfcc', 'mel', 'latent')
UNIT_ID_OFFSET = 3                  # a unit u is written as the id 3 + u: the special ids 0 .. 2 (<pad>, <space>, <eos>) stay free
KMEANS_HEADER = 'restart,iter,inertia,shift,empty'
KMEANS_UNITS_HEADER = 'unit,frames'


def merge_repeats(units):
    """a frame-level unit sequence with consecutive repeats merged -> list of units"""
    units = np.asarray(units).reshape(-1)
    return units[np.concatenate([[True], units[1:] != units[:-1]])].tolist() if len(units) else []


def format_units(units, dist):
    """the text of one <stem>.phn of --units-wav-dir in the layout of solver.format_phn(..., vocab=None): one line `score<TAB>ids`, the
    ids 3 + unit with consecutive repeats merged, the score -(mean squared distance of the frames to their centroids); frames without a
    unit (-1: a NaN row) are left out"""
    from .solver import format_phn
    units, dist = np.asarray(units).reshape(-1), np.asarray(dist, np.float64).reshape(-1)
    keep = units >= 0
    score = -float(dist[keep].mean()) if keep.any() else 0.0
    return format_phn([score], [[UNIT_ID_OFFSET + u for u in merge_repeats(units[keep])]], None)


def packed_bytes(rows, D):
    return int(rows) * int(D) * 4


class KMeansTrainer(FeatureTool):
    """main.py --kmeans-wav-dir DIR --kmeans-out FILE.npy [--kmeans-feat mfcc|mel|latent --kmeans-k 50 --kmeans-iters 100 --kmeans-tol 1e-4
    --kmeans-init ++|sample --kmeans-restarts 1 --kmeans-max-gb 8]: fits a codebook of K centroids to the frames of the .wav files of
    DIR (kmeans.fit over the packed (rows, D) buffer of FeatureTool.pack; --resample, --trim-silence, --normalize-loudness, --batch-size,
    --seed and --load are honoured; mfcc and mel need neither a checkpoint nor a model).  -> FILE.npy, (K, D) float32;
    <logdir>/<name>/kmeans.csv (restart,iter,inertia,shift,empty), kmeans_units.csv (unit,frames: the frames of the returned fit) and one
    printed line.  The buffer's size is computed from the .wav headers in load_data; above --kmeans-max-gb the run is refused there,
    before the device is touched."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.feat = getattr(paras, 'kmeans_feat', None) or 'mfcc'
        self.K = int(getattr(paras, 'kmeans_k', None) or 50)
        self.iters = int(getattr(paras, 'kmeans_iters', None) or 100)
        tol = getattr(paras, 'kmeans_tol', None)
        self.tol = 1e-4 if tol is None else float(tol)
        self.init = getattr(paras, 'kmeans_init', None) or '++'
        self.restarts = int(getattr(paras, 'kmeans_restarts', None) or 1)
        self.max_bytes = int(float(getattr(paras, 'kmeans_max_gb', None) or 8) * (1 << 30))
        self.out = paras.kmeans_out

    def load_data(self):
        from .audio import load_audio_transform
        self.wav_dir = self.paras.kmeans_wav_dir
        self.files = list_wavs(self.wav_dir, '--kmeans-wav-dir')
        self.audio_converter = load_audio_transform(**dict(self.config['data']['audio']))
        samples = self.check_waves(self.files, '--kmeans-wav-dir')
        self.max_rows = int(sum(self.feature_rows(L) for L in samples))
        D = self.feature_dim() or toolops.KM_MAX_D               # (latent: the widest row the kernels take)
        if packed_bytes(self.max_rows, D) > self.max_bytes:
            raise ValueError('--kmeans-wav-dir %s: %d files give up to %d rows of %d columns, %.2f GiB of features; --kmeans-max-gb allows %.2f'
                             % (self.wav_dir, len(self.files), self.max_rows, D, packed_bytes(self.max_rows, D) / float(1 << 30),
                                self.max_bytes / float(1 << 30)))
        if self.max_rows < self.K:
            raise ValueError('--kmeans-wav-dir %s: at most %d rows for --kmeans-k %d clusters' % (self.wav_dir, self.max_rows, self.K))
        return self

    def exec(self):
        from .kmeans import fit_all
        t0 = time.perf_counter()
        feat, _, n_rows = self.pack(self.files)
        fits = fit_all(feat, self.K, self.iters, self.tol, self.init, int(getattr(self.paras, 'seed', 0)), self.restarts)
        self.result = best = min(fits, key=lambda r: r.inertia)
        os.makedirs(self.logdir, exist_ok=True)
        out_dir = os.path.dirname(os.path.abspath(self.out))
        os.makedirs(out_dir, exist_ok=True)
        np.save(self.out, best.centroids.cpu().numpy(), allow_pickle=False)
        self.write_lines('kmeans.csv', [KMEANS_HEADER] + ['%d,%d,%.9g,%.9g,%d' % ((r,) + h) for r, res in enumerate(fits) for h in res.history])
        frames = torch.bincount(best.idx[best.idx >= 0].long(), minlength=self.K).cpu().numpy()
        table = self.write_lines('kmeans_units.csv', [KMEANS_UNITS_HEADER] + ['%d,%d' % (u, n) for u, n in enumerate(frames.tolist())])
        print('[INFO]', 'k-means of %s: %d units from %d frames of %d files, inertia %.6g after %d iterations (%s; %d restart%s), %d units unused; %s, %s, %.2f s'
              % (self.feat, self.K, int(n_rows.sum()), len(self.files), best.inertia, best.n_iter, 'converged' if best.converged else 'not converged',
                 self.restarts, '' if self.restarts == 1 else 's', int((frames == 0).sum()), self.out, table, time.perf_counter() - t0))
        return self.K


class UnitWriter(FeatureTool):
    """main.py --units-wav-dir DIR --units-codebook FILE.npy [--kmeans-feat mfcc|mel|latent --units-frames]: the unit sequence of every .wav
    of DIR under the codebook of --kmeans-out (kmeans.quantise over the packed buffer of a batch) -> <logdir>/<name>/<stem>.phn in the
    layout of --transcribe-wav-dir (format_units: ids 3 + unit, repeats merged, the score -mean squared distance), which
    --build-lm-phn-dir --lm-classes <3 + K> and --score-phn-dir read as they are; --units-frames also writes the unmerged frame-level units as
    <stem>-units.npy (int32).  A codebook whose D is not the feature's is refused in load_data (for latent: when the model is built)."""

    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.feat = getattr(paras, 'kmeans_feat', None) or 'mfcc'
        self.want_frames = bool(getattr(paras, 'units_frames', False))

    def load_data(self):
        from .audio import load_audio_transform
        self.wav_dir = self.paras.units_wav_dir
        self.files = list_wavs(self.wav_dir, '--units-wav-dir')
        self.audio_converter = load_audio_transform(**dict(self.config['data']['audio']))
        self.check_waves(self.files, '--units-wav-dir')
        self.codebook = load_codebook('--units-codebook', self.paras.units_codebook, self.feature_dim())
        return self

    def exec(self):
        from .kmeans import quantise
        os.makedirs(self.logdir, exist_ok=True)
        t0, n, table = time.perf_counter(), 0, None
        for names in self.batches(self.files):
            feat, first, n_rows = self.pack(list(names))
            if table is None:
                if self.codebook.shape[1] != feat.shape[1]:
                    raise ValueError('--units-codebook %s: the codebook has D = %d columns, the features have %d'
                                     % (self.paras.units_codebook, self.codebook.shape[1], feat.shape[1]))
                table = torch.from_numpy(self.codebook).to(feat.device)
            idx, dist = quantise(feat, table)
            host = torch.stack([idx.double(), dist.double()]).cpu().numpy()             # (the batch's one host read)
            for f, r0, r in zip(names, first.tolist(), n_rows.tolist()):
                stem = os.path.join(self.logdir, os.path.splitext(f)[0])
                units = host[0, r0:r0 + r].astype(np.int32)
                with open(stem + '.phn', 'w') as fh:
                    fh.write(format_units(units, host[1, r0:r0 + r]))
                if self.want_frames:
                    np.save(stem + '-units.npy', units, allow_pickle=False)
                n += r
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', 'Wrote the units of %d files (%d frames of %s, %d centroids) into %s, %.2f s'
                  % (len(self.files), n, self.feat, self.codebook.shape[0], self.logdir, time.perf_counter() - t0))
        return len(self.files)
