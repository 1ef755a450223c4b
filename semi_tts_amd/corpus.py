"""The corpus loader: the `data.corpus` layout of the reference (src/data.py, corpus/vctk.py, src/text.py) read with the standard
library, its batch sampler, and device-resident splits the trainers fetch batches from (main.py --corpus).

Host side (nothing here touches a device until DeviceSplit is built):
    Corpus(**config['data']['corpus'])     the four files, checked: every refusal is raised here
    corpus.measure(split, sample_rate)     actual sample counts from the .wav headers
    corpus.select(rows, n_fft, hop, ...)   utterances the kernels cannot take are dropped and counted
    Sampler(lengths, B, bucketing, train)  the reference's batches, from a generator of its own
Device side:
    DeviceSplit(conv, rows, sampler, r)    one packed float32 buffer per split; fetch() -> (mel, aug_mel, linear, text, sid)

Layout (corpus/vctk.py:25-34, src/text.py:106-113):
    partition_table   CSV, first column the file id, columns speaker, split (paired | unpaired | dev | test), duration
    map_table         tab-separated, first column the file id, columns phn_seq, spkr
    spkr_map          JSON object speaker name -> id; n_spkr = its length
    vocab_file        one symbol per line (solver.read_vocab): line k is id 3 + k
    wav               <path>/<speaker>/<id>.wav"""
import csv
import json
import os
import wave

import numpy as np

SPLITS = ('paired', 'unpaired', 'dev', 'test')
TRAIN_SPLITS = ('paired', 'unpaired')
USED_SPLITS = ('paired', 'unpaired', 'dev')          # (the test split belongs to --gen-specgram on files: not read here)
PAD_IDX, SPACE_IDX = 0, 1                            # src/text.py:33-39
NAMED = 5                                            # offenders named in a refusal


def _named(items):
    items = list(items)
    return ', '.join(str(i) for i in items[:NAMED]) + (' ... (%d in all)' % len(items) if len(items) > NAMED else '')


def _table(path, delimiter, columns, what):
    """rows of a delimited table with a header line whose FIRST column (whatever its name: pandas' index_col=0) is the file id"""
    with open(path, newline='') as f:
        rows = list(csv.reader(f, delimiter=delimiter))
    if not rows:
        raise ValueError('%s %s is empty' % (what, path))
    head = [h.strip() for h in rows[0]]
    missing = [c for c in columns if c not in head[1:]]
    if missing:
        raise ValueError('%s %s lacks the column(s) %s (has %s)' % (what, path, ', '.join(missing), ', '.join(head)))
    col = {c: head.index(c, 1) for c in columns}
    out = []
    for n, row in enumerate(rows[1:], 2):
        if not row or all(not c.strip() for c in row):
            continue
        if len(row) < len(head):
            raise ValueError('%s %s line %d has %d fields, the header %d' % (what, path, n, len(row), len(head)))
        out.append((row[0], {c: row[i] for c, i in col.items()}))
    return out


def read_partition_table(path):
    """-> list of dict(id, speaker, split, duration) in file order"""
    out, bad = [], []
    for fid, r in _table(path, ',', ('speaker', 'split', 'duration'), 'partition_table'):
        if r['split'] not in SPLITS:
            bad.append('%s (%s)' % (fid, r['split']))
            continue
        try:
            dur = float(r['duration'])
        except ValueError:
            raise ValueError('partition_table %s: %s has the duration %r' % (path, fid, r['duration']))
        out.append(dict(id=fid, speaker=r['speaker'], split=r['split'], duration=dur))
    if bad:
        raise ValueError('partition_table %s: split must be one of %s: %s' % (path, ' | '.join(SPLITS), _named(bad)))
    ids = [r['id'] for r in out]
    if len(set(ids)) != len(ids):
        seen, dup = set(), []
        for i in ids:
            if i in seen:
                dup.append(i)
            seen.add(i)
        raise ValueError('partition_table %s lists a file id more than once: %s' % (path, _named(dup)))
    return out


def read_spkr_map(path):
    """-> dict speaker name -> id"""
    with open(path) as f:
        m = json.load(f)
    if not isinstance(m, dict) or not m or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in m.values()):
        raise ValueError('spkr_map %s must be a JSON object of speaker name -> non-negative id' % path)
    over = [k for k, v in m.items() if v >= len(m)]
    if over:
        raise ValueError('spkr_map %s: ids must lie in [0, %d) (n_spkr is its length): %s' % (path, len(m), _named(over)))
    return m


def read_map_table(path):
    """-> dict file id -> dict(phn_seq, spkr)"""
    return {fid: r for fid, r in _table(path, '\t', ('phn_seq', 'spkr'), 'map_table')}


def encode(phn_seq, vocab2idx, file_id=None):
    """PhoneTextEncoder.encode (src/text.py:60-65): strip "\\r\\n ", split on single spaces, an empty piece is <space> (1), a symbol its
    id, one 0 appended.  An unknown symbol raises ValueError naming the file."""
    out = []
    for v in phn_seq.strip('\r\n ').split(' '):
        if v == '':
            out.append(SPACE_IDX)
        elif v in vocab2idx:
            out.append(vocab2idx[v])
        else:
            raise ValueError('transcript of %s: the symbol %r is not in the vocabulary' % (file_id if file_id is not None else '?', v))
    return out + [PAD_IDX]


class Utterance:
    __slots__ = ('id', 'speaker', 'sid', 'path', 'duration', 'text', 'samples', 'rate')

    def __init__(self, id, speaker, sid, path, duration, text):
        self.id, self.speaker, self.sid, self.path, self.duration, self.text = id, speaker, sid, path, duration, text
        self.samples = self.rate = None


class Corpus:
    """the tables of `data.corpus`, read and checked.  Everything wrong with them raises ValueError here: a speaker that is not in the
    map, an id without a transcript, a symbol outside the vocabulary, a .wav that does not exist (the first few offenders are named)."""

    def __init__(self, path, partition_table, map_table, spkr_map, vocab_file, batch_size=8, bucketing=False, name='vctk', **_):
        from .solver import read_vocab
        self.path, self.name = path, name
        self.batch_size, self.bucketing = int(batch_size), bool(bucketing)
        self.vocab = read_vocab(vocab_file)
        self.vocab_size = len(self.vocab)                          # 3 + number of vocabulary lines
        self.vocab2idx = {}
        for i, v in enumerate(self.vocab):
            self.vocab2idx.setdefault(v, i)
        self.spkr_map = read_spkr_map(spkr_map)
        self.n_spkr = len(self.spkr_map)
        self.map_table = read_map_table(map_table)
        table = [r for r in read_partition_table(partition_table) if r['split'] in USED_SPLITS]
        no_spkr = [r['id'] for r in table if r['speaker'] not in self.spkr_map]
        if no_spkr:
            raise ValueError('partition_table %s: speaker not in spkr_map %s: %s' % (partition_table, spkr_map, _named(
                '%s (%s)' % (i, s) for i, s in ((r['id'], r['speaker']) for r in table if r['speaker'] not in self.spkr_map))))
        no_text = [r['id'] for r in table if r['id'] not in self.map_table]
        if no_text:
            raise ValueError('map_table %s has no transcript for: %s' % (map_table, _named(no_text)))
        self.rows = {s: [] for s in USED_SPLITS}
        for r in table:
            wav = os.path.join(path, r['speaker'], r['id'] + '.wav')                  # corpus/vctk.py:31
            self.rows[r['split']].append(Utterance(r['id'], r['speaker'], self.spkr_map[r['speaker']], wav, r['duration'],
                                                   self.encode(self.map_table[r['id']]['phn_seq'], r['id'])))
        no_wav = [u.path for s in USED_SPLITS for u in self.rows[s] if not os.path.isfile(u.path)]
        if no_wav:
            raise ValueError('corpus %s: no such .wav: %s' % (path, _named(no_wav)))

    def encode(self, phn_seq, file_id=None):
        return encode(phn_seq, self.vocab2idx, file_id)

    def measure(self, split, sample_rate, resample=False):
        """the actual sample count of every utterance of `split` at `sample_rate`, from the .wav headers (no sample is read): fills
        .samples / .rate and returns the rows.  A foreign rate raises load_batch's error unless resample is set (then the count is that
        of the converted waveform); a file that is not 16-bit PCM raises."""
        from .audio import resampled_len
        for u in self.rows[split]:
            with wave.open(u.path, 'rb') as w:
                sr, width, n = w.getframerate(), w.getsampwidth(), w.getnframes()
            if width != 2:
                raise ValueError('read_wav: %s is %d-bit; only 16-bit PCM is read' % (u.path, 8 * width))
            if sr != sample_rate and not resample:
                raise ValueError('Sample rate mismatch. Expected %d but get %d (%s)' % (sample_rate, sr, u.path))
            u.rate = sr
            u.samples = n if sr == sample_rate else resampled_len(n, sr, sample_rate)
        return self.rows[split]


def select(rows, n_fft, hop, max_tokens, max_frames=None):
    """(the rows the kernels take, counts of the dropped): an utterance of n_fft // 2 samples or fewer (reflect padding), a transcript
    whose encoding -- the appended 0 included: it is the width of the text batch -- is longer than st_ctc_loss takes, more than
    max_frames frames (1 + samples // hop) where a limit is given.  Counted under the first rule that applies."""
    kept, counts = [], dict(short=0, tokens=0, frames=0)
    for u in rows:
        if u.samples <= n_fft // 2:
            counts['short'] += 1
        elif len(u.text) > max_tokens:
            counts['tokens'] += 1
        elif max_frames is not None and 1 + u.samples // hop > max_frames:
            counts['frames'] += 1
        else:
            kept.append(u)
    return kept, counts


def drop_report(split, n_rows, counts, n_fft, max_tokens, max_frames):
    """the one line per split that says what select dropped"""
    return ('%s: %d of %d utterances kept | dropped: %d of %d samples or fewer, %d over %d tokens, %d over %s frames'
            % (split, n_rows - sum(counts.values()), n_rows, counts['short'], n_fft // 2, counts['tokens'], max_tokens, counts['frames'],
               'any number of' if max_frames is None else str(max_frames)))


class Sampler:
    """The batches of one split for one rank, with the reference's semantics (corpus/vctk.py:21,41-47, src/data.py:35-63) and a seeded
    generator of its own: numpy.random.RandomState([seed, rank, epoch]), so the batches depend on nothing else that draws.

    The split is sorted by `lengths` (actual sample counts), longest first, stable; rank k of `world` takes rows k::world of that.  With N
    rows and batch size B:
        train, bucketing       a batch is the window [i, i + B) of the sorted rows, i clamped to N - B; an epoch is one permutation of
                               the N starts (N batches: the reference's DataLoader has batch size 1 over N buckets)
        train, no bucketing    an epoch is one permutation of the rows cut into N // B batches, the remainder dropped
        not train (dev)        the rows in order, ceil(N / B) batches, the remainder kept; bucketing does not apply
        N < B                  one batch of all rows
    A batch is an array of positions in the list `lengths` was taken from."""

    def __init__(self, lengths, batch_size, bucketing=False, train=True, seed=0, rank=0, world=1, sharded=False):
        """sharded: `lengths` are those of this rank's rows alone (a split trimmed after its upload): every row is taken, sorted as
        above, and `rank` only seeds the generator."""
        lengths = np.asarray(lengths, np.int64)
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError('Sampler: batch size %d, rank %d of %d' % (batch_size, rank, world))
        self.rows = np.argsort(-lengths, kind='stable')[slice(None) if sharded else slice(rank, None, world)]
        if len(self.rows) == 0:
            raise ValueError('Sampler: no utterance for rank %d of %d (%d in the split)' % (rank, world, len(lengths)))
        self.B, self.train, self.bucketing = int(batch_size), bool(train), bool(bucketing) and bool(train)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.rewind()

    def n_batches(self):
        N, B = len(self.rows), self.B
        if N < B:
            return 1
        if not self.train:
            return -(-N // B)
        return N if self.bucketing else N // B

    def epoch(self, e):
        """the batches of epoch e, in order"""
        N, B = len(self.rows), self.B
        if N < B:
            return [self.rows.copy()]
        if not self.train:
            return [self.rows[i:i + B] for i in range(0, N, B)]
        perm = np.random.RandomState([self.seed & 0xffffffff, self.rank, int(e)]).permutation(N)
        if self.bucketing:
            return [self.rows[min(int(i), N - B):min(int(i), N - B) + B] for i in perm]
        return [self.rows[perm[i:i + B]] for i in range(0, N - B + 1, B)]

    def rewind(self):
        self._epoch, self._pos, self._batches = 0, 0, None

    def next(self):
        """the next batch; a new epoch begins when this one is used up"""
        if self._batches is None:
            self._batches = self.epoch(self._epoch)
        if self._pos >= len(self._batches):
            self._epoch, self._pos = self._epoch + 1, 0
            self._batches = self.epoch(self._epoch)
        self._pos += 1
        return self._batches[self._pos - 1]


def too_large(name, n_utt, n_samples, max_bytes):
    return ('corpus: the %s split (%d utterances, %d samples) needs %.3f GB (%d bytes) on the device, the limit is %.3f GB (%d bytes) '
            '(--corpus-max-gb; default: half of the free device memory)'
            % (name, n_utt, n_samples, 4 * n_samples / 2.0 ** 30, 4 * n_samples, max_bytes / 2.0 ** 30, max_bytes))


TRIM_CALL = 64                                       # utterances per trimming call of a split (toolops.FEATURES_MAX_BATCH)


def apply_bounds(rows, mine, offsets, lens, start, end, sampler, n_fft, hop, max_frames=None):
    """What a split becomes once its rank's rows are trimmed: rows / offsets / lens of the whole split, `mine` the positions this
    rank uploaded, start / end the kept samples [start, end) of each of them (st_trim_silence's bounds).  The rows of other ranks
    leave the split (their trimmed lengths are not known here); offsets move by start, lens become end - start; `select` runs
    again on the trimmed lengths (too short for the reflect padding, over max_frames), and the sampler is rebuilt over the
    survivors with the batch size, flags, seed and rank of `sampler` (Sampler(sharded=True)).  The rows are COPIES whose .samples
    is the trimmed count.  -> (rows, offsets, lens, sampler, counts of the dropped)"""
    import copy
    mine = np.asarray(mine, np.int64)
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    if start.shape != mine.shape or end.shape != mine.shape or (start < 0).any() or (end > lens[mine]).any() or (start > end).any():
        raise ValueError('corpus: trim bounds outside their utterances')
    cand = []
    for i, a, b in zip(mine, start, end):
        u = copy.copy(rows[int(i)])
        u.samples = int(b - a)
        cand.append((u, int(offsets[int(i)] + a)))
    kept, counts = select([u for u, _ in cand], n_fft, hop, float('inf'), max_frames)
    if not kept:
        raise ValueError('corpus: no utterance left after trimming (%d trimmed)' % len(cand))
    keep = set(id(u) for u in kept)
    new_off = np.array([o for u, o in cand if id(u) in keep], np.int64)
    new_lens = np.array([u.samples for u in kept], np.int64)
    new_sampler = Sampler(new_lens, sampler.B, sampler.bucketing, sampler.train, sampler.seed, sampler.rank, sampler.world, sharded=True)
    return kept, new_off, new_lens, new_sampler, counts


def loudness_report(name, info, target):
    """the one line per split that says what the loudness pass found and did: utterances, mean / min / max LUFS before, and how many
    were peak-limited, gain-limited or left alone, by flag"""
    flags, lufs = np.asarray(info['flags']), np.asarray(info['lufs'], np.float64)
    ok = lufs[np.isfinite(lufs)]
    span = 'mean %.2f min %.2f max %.2f LUFS before' % (ok.mean(), ok.min(), ok.max()) if len(ok) else 'no utterance with a loudness'
    return ('%s: loudness of %d utterances, %s | %s | %d peak-limited, %d gain-limited | left alone: %d non-finite, %d under 400 ms, %d silent'
            % (name, len(flags), span, 'measured only' if target is None else 'normalised to %.1f LUFS' % target, int((flags & 8 != 0).sum()),
               int((flags & 16 != 0).sum()), int((flags & 1 != 0).sum()), int((flags & 2 != 0).sum()), int((flags & 4 != 0).sum())))


def trim_report(name, sample_rate, before, after, n_before, counts):
    """the one line per split that says what trimming did: seconds before / after, the share removed, the drops"""
    return ('%s: trimmed %.1f s -> %.1f s (%.1f%% removed) | %d of %d utterances kept | dropped after trimming: %d too short, %d over the frame limit'
            % (name, before / float(sample_rate), after / float(sample_rate), 100.0 * (before - after) / max(before, 1),
               n_before - counts['short'] - counts['frames'], n_before, counts['short'], counts['frames']))


class DeviceSplit:
    """One split of one rank on the device: every waveform read ONCE (AudioConverter's _read_pcm / resampling path) into one packed
    float32 buffer, with host offsets / lens.  A batch is not copied out of it: fetch() hands toolops.audio_features the buffer with the
    batch's offsets (WaveBatch.window).  The transcripts stay on the host; a fetch uploads the batch's text and speaker ids as one small
    int64 array (no host READ in a fetch, no file access).

    rows: the utterances of the split (measured and selected); sampler: a Sampler over their sample counts.
    fetch() -> (mel, aug_mel, linear, text, sid) as collect_fn + fetch_data deliver them (src/data.py:112-147, bin/train_vqvae.py:33-53):
    utterances longest first (WaveBatch's stable order by samples; text and sid follow), mel / linear zero-padded to a multiple of r with
    at least one extra frame, aug_mel to its own longest with fresh SNR / stretch draws (a dev split, train=False, draws nothing: no
    noise, no stretch, seed 0), text padded with 0 to the batch's longest.
    last_fetch = (file ids in batch order, seed, snr, stretch) of the latest batch.

    trim: a dict of AudioConverter.trim_batch's arguments (top_db, frame_length, hop_length, pad_ms).  Sharding and the size check
    stay on the header lengths; after the upload the rank's rows are trimmed on the device in calls of 64 utterances with ONE host
    read for the split, and the split becomes what apply_bounds says (rows / lens / offsets of this rank's survivors, a sampler over
    the trimmed lengths; the trimmed samples stay resident, nothing is copied).  trim_report: the line that says what it did.
    max_frames: the frame limit select() applied, applied again to the trimmed lengths.

    loudness: a dict of AudioConverter.loudness_batch's arguments (target, peak_db, max_gain_db).  After the upload, and after the
    trimming if any, this rank's rows are metered (ITU-R BS.1770-4) and multiplied by their gains IN PLACE in the resident buffer, in
    calls of 64 utterances with ONE host read for the split; offsets and lens do not change.  loudness_report: the line that says
    what it did; loudness_info: loudness_batch's dict over this rank's rows (`rows`: their positions)."""

    def __init__(self, conv, rows, sampler, r, name='split', train=True, resample=False, max_bytes=None, trim=None, max_frames=None,
                 loudness=None):
        import torch
        from .audio import _device
        self.conv, self.rows, self.sampler, self.r, self.name, self.train = conv, list(rows), sampler, int(r), name, bool(train)
        mine = sorted(int(i) for i in sampler.rows)
        self.lens = np.array([u.samples for u in self.rows], np.int64)
        self.offsets = np.full(len(self.rows), -1, np.int64)
        self.offsets[mine] = np.concatenate([[0], np.cumsum(self.lens[mine])[:-1]])
        total = int(self.lens[mine].sum())
        self.nbytes = 4 * total
        dev = _device()
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(dev)[0] // 2
        if self.nbytes > max_bytes:
            raise ValueError(too_large(name, len(mine), total, max_bytes))
        if trim is not None:
            pad = conv._check_trim(**trim)
        if loudness is not None:
            conv._check_loudness(**loudness)
        self.buffer = self._upload(mine, total, dev, resample)
        self.last_fetch = None
        self.trim_report = None
        self.loudness_report = self.loudness_info = None
        if trim is not None:
            self._trim(pad, max_frames, **trim)
        if loudness is not None:
            self._normalise(**loudness)

    def _normalise(self, target=None, peak_db=-1.0, max_gain_db=30.0):
        from .audio import WaveBatch
        mine = np.flatnonzero(self.offsets >= 0)
        mine = mine[np.argsort(-self.lens[mine], kind='stable')]
        info = self.conv.loudness_batch(WaveBatch.window(self.buffer, self.offsets[mine], self.lens[mine]), target, peak_db, max_gain_db)
        info = info[0] if isinstance(info, tuple) else info
        self.loudness_info = dict(info, rows=mine)
        self.loudness_report = loudness_report(self.name, info, target)

    def _trim(self, pad, max_frames, top_db=60., frame_length=2048, hop_length=512, pad_ms=0.):
        import torch
        from . import toolops
        mine = np.asarray(self.sampler.rows, np.int64)             # (longest first: a call's T_pad is its first utterance's)
        parts = [toolops.trim_silence(self.buffer, self.offsets[mine[i:i + TRIM_CALL]], self.lens[mine[i:i + TRIM_CALL]], frame_length, hop_length,
                                      top_db, pad=pad)[1] for i in range(0, len(mine), TRIM_CALL)]
        bounds = torch.cat(parts).cpu().numpy().astype(np.int64)   # the split's one host read
        before = int(self.lens[mine].sum())
        by_row = np.argsort(mine)                                  # (the surviving rows keep their listed order)
        mine, bounds = mine[by_row], bounds[by_row]
        self.rows, self.offsets, self.lens, self.sampler, counts = apply_bounds(
            self.rows, mine, self.offsets, self.lens, bounds[:, 0], bounds[:, 1], self.sampler, self.conv.n_fft, self.conv.hop_length, max_frames)
        self.trim_counts = counts
        self.trim_report = trim_report(self.name, self.conv.sr, before, int(self.lens.sum()), len(mine), counts)

    def _upload(self, mine, total, dev, resample):
        """the rank's utterances -> one device buffer.  Files at the converter's rate are laid out on the host and go up in ONE copy; with
        resample the files of each foreign rate are converted on the GPU in one call (as AudioConverter.load_batch does) and copied in."""
        import torch
        from .audio import _read_pcm, _resample
        host = np.zeros(total, np.float32)
        foreign = {}
        for i in mine:
            u = self.rows[i]
            pcm, sr = _read_pcm(u.path)
            if sr == self.conv.sr:
                if pcm.shape[0] != self.lens[i]:
                    raise ValueError('corpus: %s changed while loading' % u.path)
                host[self.offsets[i]:self.offsets[i] + self.lens[i]] = pcm[:, 0].astype(np.float32) / 32768.0
            elif not resample:
                raise ValueError('Sample rate mismatch. Expected %d but get %d (%s)' % (self.conv.sr, sr, u.path))
            else:
                foreign.setdefault(sr, []).append((i, torch.from_numpy(pcm[:, 0].copy())))
        buf = torch.from_numpy(host).to(dev)
        for sr, items in sorted(foreign.items()):
            wb = _resample([w for _, w in items], sr, self.conv.sr)
            y = wb.packed(dev)
            for row, k in enumerate(wb.order):
                i = items[k][0]
                if int(wb.lens[row]) != self.lens[i]:
                    raise ValueError('corpus: %s changed while loading' % self.rows[i].path)
                buf[self.offsets[i]:self.offsets[i] + self.lens[i]] = y[int(wb.offsets[row]):int(wb.offsets[row] + wb.lens[row])]
        return buf

    def rewind(self):
        self.sampler.rewind()

    def n_batches(self):
        return self.sampler.n_batches()

    def window(self, idx):
        """the WaveBatch of the utterances `idx` (positions in rows), addressed inside the buffer; -> (WaveBatch, idx in its order)"""
        from .audio import WaveBatch
        idx = np.asarray(idx, np.int64)
        idx = idx[np.argsort(-self.lens[idx], kind='stable')]
        if (self.offsets[idx] < 0).any():
            raise ValueError('corpus: an utterance of another rank')
        return WaveBatch.window(self.buffer, self.offsets[idx], self.lens[idx]), idx

    def fetch(self):
        import torch
        wb, idx = self.window(self.sampler.next())
        B = len(idx)
        if self.train:
            draws = [self.conv._draw() for _ in range(B)]
            snr, stretch = [d[0] for d in draws], [d[1] for d in draws]
            seed = int(torch.randint(0, 2 ** 62, (1,)))
        else:
            snr, stretch, seed = [None] * B, [1.0] * B, 0
        mel, aug_mel, linear = self.conv.extract_batch(wb, r=self.r, seed=seed, snr=snr, stretch=stretch)
        rows = [self.rows[i] for i in idx]
        L = max(len(u.text) for u in rows)
        host = np.zeros(B * L + B, np.int64)
        for b, u in enumerate(rows):
            host[b * L:b * L + len(u.text)] = u.text
            host[B * L + b] = u.sid
        t = torch.from_numpy(host).to(self.buffer.device)
        self.last_fetch = ([u.id for u in rows], seed, snr, stretch)
        return mel, aug_mel, linear, t[:B * L].view(B, L), t[B * L:]


def load_splits(corpus_cfg, conv, r, splits, batch_sizes, seed=0, rank=0, world=1, resample=False, max_frames=None, max_gb=None,
                verbose=print, trim=None, loudness=None):
    """Corpus + one DeviceSplit per name in `splits` (of 'paired', 'unpaired', 'dev').  batch_sizes: dict split -> B.  Everything the
    tables, the headers and the limits can refuse is raised for EVERY split before the first device allocation.  trim: every split
    (dev included) is trimmed with these settings after its upload (DeviceSplit), one report line per split.  loudness: every split
    (dev included) is then metered and normalised in place with these settings (DeviceSplit), one report line per split.
    -> (Corpus, dict split -> DeviceSplit)"""
    from . import ops
    corpus = Corpus(**corpus_cfg)
    conv._check([], [])                                        # (the framing itself: n_fft, hop, win)
    if trim is not None:
        conv._check_trim(**trim)
    if loudness is not None:
        conv._check_loudness(**loudness)
    plan = []
    for s in splits:
        rows = corpus.measure(s, conv.sr, resample)
        kept, counts = select(rows, conv.n_fft, conv.hop_length, ops.CTC_MAX_TOKENS, max_frames)
        verbose(drop_report(s, len(rows), counts, conv.n_fft, ops.CTC_MAX_TOKENS, max_frames))
        if not kept:
            raise ValueError('corpus: the %s split has no utterance left (%d listed)' % (s, len(rows)))
        train = s in TRAIN_SPLITS
        plan.append((s, kept, Sampler([u.samples for u in kept], batch_sizes[s], corpus.bucketing, train, seed, rank, world), train))
    max_bytes = None if max_gb is None else int(float(max_gb) * 2 ** 30)
    for s, kept, sampler, _ in plan:
        n = int(sum(kept[int(i)].samples for i in sampler.rows))
        if max_bytes is not None and 4 * n > max_bytes:
            raise ValueError(too_large(s, len(sampler.rows), n, max_bytes))
    sets = {}
    for s, kept, sampler, train in plan:
        sets[s] = DeviceSplit(conv, kept, sampler, r, name=s, train=train, resample=resample, max_bytes=max_bytes, trim=trim,
                              max_frames=max_frames, loudness=loudness)
        if trim is not None:
            verbose(sets[s].trim_report)
        if loudness is not None:
            verbose(sets[s].loudness_report)
    return corpus, sets
