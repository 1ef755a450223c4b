"""Solver-shaped entry points (`Solver(config, paras, mode).load_data().set_model().exec()`,
ref: main.py:65-68) for the decode path on synthetic data: the corpus, audio front end and
tokenizer of the reference are outside the hot path and absent here, so `load_data` draws seeded
synthetic batches of the shapes the real loaders would deliver.

SpecgramGenerator mirrors bin/gen_specgram.py:89-129: batched free-running decode for
`mel_len + INFERENCE_MARGIN_FRAMES` frames in eval mode, then per utterance `-mel.npy`, `-spec.npy`
(fp32) and `-align.npy` trimmed to [int(len*6)//r, text_len].
"""
import json
import math
import os
import time

import numpy as np
import torch

from . import ops, toolops
from .vqvae import VQVAE, FRAME_PHN_RATIO, INFERENCE_MARGIN_FRAMES, SYNTH_MAX_FRAMES_PER_PHONE


class BaseSolver:
    def __init__(self, config, paras, mode):
        self.config, self.paras, self.mode = config, paras, mode
        if not torch.cuda.is_available() or getattr(paras, 'cpu', False):
            raise RuntimeError('the MI355X path needs a GPU (there is no CPU fallback)')
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.exp_name = getattr(paras, 'name', None) or 'synthetic'
        self.logdir = os.path.join(getattr(paras, 'logdir', 'log/'), self.exp_name)
        self.step = 0
        audio = config['data']['audio']
        self.n_mels, self.linear_dim = audio['num_mels'], audio['num_freq']
        self.vocab_size = int(getattr(paras, 'vocab_size', 43))       # <pad>,<space>,<eos> + 40 phonemes
        self.n_spkr = int(getattr(paras, 'n_spkr', 109))              # corpus/spkr/lj_vctk.json

    def verbose(self, msg):
        if getattr(self.paras, 'verbose', True):
            print('[INFO]', msg)

    # -- checkpoints: the reference's on-disk format {"model", "optimizer", "global_step"} (src/solver.py:118-135, :203-216)
    def save_checkpoint(self, f_name, score=0.0):
        ckpdir = os.path.join(getattr(self.paras, 'ckpdir', 'ckpt/'), self.exp_name)
        os.makedirs(ckpdir, exist_ok=True)
        path = os.path.join(ckpdir, f_name)
        full = {'model': self.model.state_dict(), 'global_step': self.step}
        if getattr(self, 'optimizer', None) is not None:
            full['optimizer'] = self.optimizer.get_opt_state_dict()
        torch.save(full, path)
        self.verbose('Saved checkpoint (step = %d, score = %.2f) and status @ %s' % (self.step, score, path))
        return path

    def load_ckpt(self):
        """load `paras.load` into self.model (and, in training mode, the optimizer state and step counter)"""
        path = getattr(self.paras, 'load', None)
        if not path:
            return False
        ckpt = torch.load(path, map_location=self.device)
        if getattr(self, 'corpus', None) is not None:
            # --corpus: vocab_size and n_spkr come from the corpus files; a checkpoint trained on other tables is refused by name
            own = self.model.state_dict()
            n_ck = ckpt['model']['spkr_embed.weight'].shape[0] if 'spkr_embed.weight' in ckpt['model'] else self.n_spkr
            off = [k for k, v in ckpt['model'].items() if k.startswith('codebook.') and k in own and tuple(v.shape) != tuple(own[k].shape)]
            if n_ck != self.n_spkr or off:
                raise ValueError('--load %s disagrees with the corpus (vocab_size %d, n_spkr %d): the checkpoint has %d speakers%s'
                                 % (path, self.vocab_size, self.n_spkr, n_ck,
                                    ''.join('; %s is %s' % (k, tuple(ckpt['model'][k].shape)) for k in off[:3])))
        # strict, like the reference (bin/gen_specgram.py:80, bin/train_vqvae.py:106): a checkpoint of another architecture
        # must not leave the constructor's random weights in place silently
        self.model.load_state_dict(ckpt['model'], strict=True)
        if self.mode == 'train':
            self.step = ckpt.get('global_step', 0)
            if getattr(self, 'optimizer', None) is not None and 'optimizer' in ckpt:
                self.optimizer.load_opt_state_dict(ckpt['optimizer'])
            self.verbose('Load ckpt from %s, restarting at step %d' % (path, self.step))
        else:
            self.step = ckpt.get('global_step', 0)
            self.verbose('Evaluation target = %s (step %d)' % (path, self.step))
        return True

    def _build_model(self):
        cfg = json.loads(json.dumps(self.config['model']))
        attr = cfg['codebook'].get('phn_attr_pth')
        if attr and not os.path.exists(attr):
            # the attribute table ships with the reference checkout, not with this repository
            self.verbose('phoneme attribute table %s not found: codebook without projected attributes' % attr)
            cfg['codebook']['phn_attr_pth'], cfg['codebook']['proj_attr'] = '', None
        return VQVAE(self.n_mels, self.linear_dim, self.vocab_size, self.n_spkr, **cfg).to(self.device)


class SpecgramGenerator(BaseSolver):
    def load_data(self):
        """synthetic test set: `n_batches` batches of (mel length only is used, text ids, speaker ids)"""
        rs = np.random.RandomState(getattr(self.paras, 'seed', 0))
        B = int(getattr(self.paras, 'batch_size', self.config['data']['corpus'].get('batch_size', 8)))
        frames = int(getattr(self.paras, 'frames', 256))
        L = int(np.ceil(frames / FRAME_PHN_RATIO))
        self.test_set = []
        for i in range(int(getattr(self.paras, 'n_batches', 1))):
            text = rs.randint(3, self.vocab_size, (B, L)).astype(np.int64)
            text[:, -1] = 0                                     # PhoneTextEncoder appends index 0 (src/text.py:65)
            sid = rs.randint(0, self.n_spkr, (B,)).astype(np.int64)
            self.test_set.append((frames, torch.from_numpy(text), torch.from_numpy(sid)))
        self.filelist = ['utt%05d' % i for i in range(B * len(self.test_set))]
        # utterance-sharded replicas: under torch.distributed every rank decodes and writes only its own
        # contiguous range of each batch (no collective, no two ranks writing the same file)
        from . import parallel
        self.rank, self.world = parallel.rank_world()
        return self

    def set_model(self):
        self.model = self._build_model().eval()
        self.n_frames_per_step = self.model.n_frames_per_step
        if not self.load_ckpt():
            from .synthetic import load_synthetic
            load_synthetic(self.model, seed=getattr(self.paras, 'seed', 0) + 1234)
        return self

    def exec(self):
        return self.gen_specgram(self.logdir + '_%dk' % (self.step // 1000))

    def gen_specgram(self, output_dir):
        os.makedirs(output_dir, exist_ok=True)
        r = self.n_frames_per_step
        cnt, frames_out, t0 = 0, 0, time.perf_counter()
        rank, world = getattr(self, 'rank', 0), getattr(self, 'world', 1)
        from .parallel import shard_range
        gen_wav = bool(getattr(self.paras, 'gen_wav', False))
        if gen_wav:
            from .audio import load_audio_transform, write_wav
            self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        next_first = 0
        for frames, text, sid in self.test_set:
            batch_first, next_first = next_first, next_first + text.shape[0]
            lo, hi = shard_range(text.shape[0], world, rank)
            if hi <= lo:
                continue
            names = self.filelist[batch_first + lo:batch_first + hi]
            text, sid = text[lo:hi].to(self.device), sid[lo:hi].to(self.device)
            pad = r - frames % r                                                      # gen_specgram.py:36-37
            with torch.no_grad():
                mel, lin, align, _, _, _, _, _ = self.model.text_to_speech(
                    text, sid, None, None, None, None, frames + pad + INFERENCE_MARGIN_FRAMES, None, tf_rate=0.0)
            torch.cuda.synchronize()
            # (the eager forward has already checked the decode loop's hand-off status word: ops.check_handoff)
            ops.check_persist_status(self.device)
            if not (bool(torch.isfinite(mel).all()) and bool(torch.isfinite(lin).all())):
                raise RuntimeError('gen_specgram: non-finite spectrogram for batch starting at %s -- nothing written' % names[0])
            wavs = None
            if gen_wav:                                 # gen_specgram.py:114-115: Griffin-Lim of this rank's lin, on the device
                if getattr(self.paras, 'gen_wav_feat', 'linear') == 'mel':      # --gen-wav-feat mel: of its mel instead
                    wavs = self.audio_converter.gen_wav_device(mel, mel=True)
                else:
                    wavs = self.audio_converter.gen_wav_device(lin)
                if loudness_args(self.paras) is not None:           # --normalize-loudness: on the device, before the copy to the host
                    self.audio_converter.normalize_rows(wavs, None, **loudness_args(self.paras))
                wavs = wavs.cpu().numpy()
            enc_step = (text != 0).sum(dim=-1).cpu().tolist()
            dec_step = [int(n * FRAME_PHN_RATIO) // r for n in enc_step]
            for i, (msp, sp, ali) in enumerate(zip(mel, lin, align)):
                name = os.path.join(output_dir, names[i])
                np.save(name + '-mel.npy', msp.cpu().numpy().astype(np.float32), allow_pickle=False)
                np.save(name + '-spec.npy', sp.cpu().numpy().astype(np.float32), allow_pickle=False)
                np.save(name + '-align.npy', ali[:dec_step[i], :enc_step[i]].cpu().numpy())
                if wavs is not None:                    # gen_specgram.py:125-126: the full padded length, as wavs[idx]
                    write_wav(name + '-pred.wav', wavs[i], self.audio_converter.sr)
                cnt += 1
                frames_out += msp.shape[0]
        dt = time.perf_counter() - t0
        if rank == 0 or world == 1:
            self.verbose('Save %d spectrograms%s (%d frames) in %s, %.2f s' %
                         (cnt, ' on rank 0 of %d' % world if world > 1 else '', frames_out, output_dir, dt))
        return cnt


SPECIAL_TOKENS = ('<pad>', '<space>', '<eos>')     # ids 0, 1, 2 of the phone vocabulary (src/text.py); phones start at id 3


def read_vocab(path):
    """the phone symbols of a vocabulary file as the reference's data/cmu_phn.vocab lists them, one per line: -> list indexed by id
    (ids 0 .. 2 the special tokens, line k -> id 3 + k)"""
    with open(path) as f:
        phones = [ln.strip() for ln in f if ln.strip()]
    return list(SPECIAL_TOKENS) + phones


def format_phn(scores, hyps, vocab=None):
    """the text of one utterance's .phn file: one line per path, `score<TAB>tokens`, tokens space-separated phone symbols (vocab) or ids.
    An id outside the vocabulary is written as its number."""
    lines = []
    for sc, h in zip(scores, hyps):
        toks = [vocab[i] if vocab is not None and 0 <= i < len(vocab) else str(i) for i in h]
        lines.append('%.6f\t%s' % (sc, ' '.join(toks)))
    return '\n'.join(lines) + '\n'


class Transcriber(BaseSolver):
    """main.py --transcribe-wav-dir: the .wav files of a directory, sorted by name, in batches of --batch-size -> clean mel on the device
    (AudioConverter.extract_batch without noise or stretch) -> VQVAE.transcribe (speech encoder, codebook or ASR postnet, CTC prefix
    beam search) -> <logdir>/<name>.phn with --top-paths lines `score<TAB>tokens`.  Without --load the synthetic weights are used.
    --lm FILE fuses a phone n-gram table (ngram.load_table) into the search with --lm-weight and --ins-bonus; the table is read in
    load_data and refused there when its width is not that of the searched posteriors, before anything is written."""

    WAV_DIR_FLAG = 'transcribe_wav_dir'          # the attribute of paras that names the .wav directory

    def load_data(self):
        from .audio import load_audio_transform
        flag = '--' + self.WAV_DIR_FLAG.replace('_', '-')
        self.wav_dir = wav_dir = getattr(self.paras, self.WAV_DIR_FLAG)
        self.files = list_wavs(wav_dir, flag)
        self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        if self.audio_converter.n_mels != self.n_mels:
            raise ValueError('%s: data.audio has %d mels, the model %d' % (flag, self.audio_converter.n_mels, self.n_mels))
        vocab = getattr(self.paras, 'vocab', None)
        self.vocab = read_vocab(vocab) if vocab else None
        self.lm = None
        lm = getattr(self.paras, 'lm', None)
        if lm:
            from .ngram import load_table
            self.lm = load_table(lm)
            # the codebook has one entry per phone id; the ASR postnet is built with latent_dim classes (VQVAE.__init__)
            width = self.vocab_size if getattr(self.paras, 'asr_output', 'code') == 'code' else int(self.config['model']['codebook']['latent_dim'])
            if self.lm.shape[1] != width:
                raise ValueError('--lm %s: the table has %d classes, the %s posteriors %d'
                                 % (lm, self.lm.shape[1], getattr(self.paras, 'asr_output', 'code'), width))
        return self

    def set_model(self):
        self.model = self._build_model().eval()
        if not self.load_ckpt():
            from .synthetic import load_synthetic
            load_synthetic(self.model, seed=getattr(self.paras, 'seed', 0) + 1234)
        self.bonus = None
        if getattr(self, 'lm', None) is not None:               # fused once, kept on the device for every batch
            from .ngram import fusion_table
            host = fusion_table(self.lm, float(getattr(self.paras, 'lm_weight', 0.5)), float(getattr(self.paras, 'ins_bonus', 0.0)))
            self.bonus = torch.from_numpy(host).to(self.device)
        return self

    def load_waves(self, names):
        """channel 0 of the files `names` of the .wav directory as one WaveBatch on the device (AudioConverter.load_batch); with
        --resample a file at another rate is converted on the GPU, without it it raises"""
        return load_waves(self.audio_converter, self.wav_dir, names, self.paras, resample=bool(getattr(self.paras, 'resample', False)))

    def transcribe_batch(self, waves):
        """waves: 1-D waveforms on the device (or a WaveBatch) -> (hyp, hyp_len, score) as numpy arrays in the order of `waves`"""
        from .audio import WaveBatch, SNR_OFF
        wb = waves if isinstance(waves, WaveBatch) else WaveBatch(waves)
        mel, _, _ = self.audio_converter.extract_batch(wb, snr=SNR_OFF, stretch=1.0)
        frames = 1 + wb.lens // self.audio_converter.hop_length
        hyp, hyp_len, score = self.model.transcribe(mel, frames, int(self.paras.beam_width), int(self.paras.top_paths),
                                                    source=self.paras.asr_output, bonus=getattr(self, 'bonus', None))
        back = wb.inverse()                                         # sorted position of the i-th given utterance
        return hyp.cpu().numpy()[back], hyp_len.cpu().numpy()[back], score.cpu().numpy()[back]

    def exec(self):
        os.makedirs(self.logdir, exist_ok=True)
        B = int(self.paras.batch_size)
        t0, n = time.perf_counter(), 0
        for i in range(0, len(self.files), B):
            names = self.files[i:i + B]
            hyp, hyp_len, score = self.transcribe_batch(self.load_waves(names))
            for f, h, hl, sc in zip(names, hyp, hyp_len, score):
                with open(os.path.join(self.logdir, os.path.splitext(f)[0] + '.phn'), 'w') as out:
                    out.write(format_phn(sc.tolist(), [h[k, :hl[k]].tolist() for k in range(len(hl))], self.vocab))
                n += 1
        from .ngram import order_of as ngram_order_of
        fused = '' if getattr(self, 'lm', None) is None else ', %d-gram weight %g bonus %g' % (
            ngram_order_of(*self.lm.shape), self.paras.lm_weight, self.paras.ins_bonus)
        self.verbose('Transcribed %d files (beam %d, %d paths, %s posteriors%s) into %s, %.2f s'
                     % (n, self.paras.beam_width, self.paras.top_paths, self.paras.asr_output, fused, self.logdir, time.perf_counter() - t0))
        return n


class Aligner(Transcriber):
    """main.py --align-wav-dir: the .wav files of a directory (sorted by name, batches of --batch-size) and their transcripts
    <name>.phn from --phn-dir (default: the same directory; ctc_align.read_phn) -> clean mel on the device -> VQVAE.align (speech
    encoder, codebook or ASR postnet, CTC forced alignment) -> <logdir>/<name>/<file>.ali (ctc_align.format_ali) and segments.csv in
    the reference's segment_file layout (ctc_align.segment_row).  Every transcript is read in load_data: a missing or malformed one
    stops the run before anything is written.  Without --load the synthetic weights are used."""

    WAV_DIR_FLAG = 'align_wav_dir'

    def load_data(self):
        from .ctc_align import read_phn
        super().load_data()
        phn_dir = getattr(self.paras, 'phn_dir', None) or self.wav_dir
        self.transcripts = [read_phn(os.path.join(phn_dir, os.path.splitext(f)[0] + '.phn'), self.vocab) for f in self.files]
        return self

    def align_batch(self, waves, transcripts):
        """waves: 1-D waveforms on the device (or a WaveBatch), transcripts: their id lists -> (score, tok_start, tok_end, encoder
        frames) as numpy arrays in the order of `waves`"""
        from .audio import WaveBatch, SNR_OFF
        wb = waves if isinstance(waves, WaveBatch) else WaveBatch(waves)
        mel, _, _ = self.audio_converter.extract_batch(wb, snr=SNR_OFF, stretch=1.0)
        frames = 1 + wb.lens // self.audio_converter.hop_length
        L = max(1, max(len(t) for t in transcripts))
        text = np.zeros((len(wb.lens), L), np.int64)
        tl = np.zeros(len(wb.lens), np.int32)
        for row, k in enumerate(wb.order):                          # the batch is sorted by length: row `row` is waves[k]
            text[row, :len(transcripts[k])], tl[row] = transcripts[k], len(transcripts[k])
        score, path, ts, te = self.model.align(mel, frames, torch.from_numpy(text).to(self.device), tl.tolist(), source=self.paras.asr_output)
        t_enc = self.model.encoder_lengths(frames).clamp(0, path.shape[1]).numpy()
        back = wb.inverse()                                         # sorted position of the i-th given utterance
        return score.cpu().numpy()[back], ts.cpu().numpy()[back], te.cpu().numpy()[back], t_enc[back]

    def exec(self):
        from .ctc_align import format_ali, segment_row, SEGMENTS_HEADER
        os.makedirs(self.logdir, exist_ok=True)
        B = int(self.paras.batch_size)
        t0, n, n_bad = time.perf_counter(), 0, 0
        frame_s = self.model.time_reduce_factor * self.audio_converter.hop_length / self.audio_converter.sr
        rows = [SEGMENTS_HEADER]
        for i in range(0, len(self.files), B):
            names, trs = self.files[i:i + B], self.transcripts[i:i + B]
            score, ts, te, t_enc = self.align_batch(self.load_waves(names), trs)
            for f, tr, sc, a, b, T in zip(names, trs, score.tolist(), ts, te, t_enc.tolist()):
                targets = [x for x in tr if x != 0]                 # id 0 is the blank: not a target
                S = len(targets)
                with open(os.path.join(self.logdir, os.path.splitext(f)[0] + '.ali'), 'w') as out:
                    out.write(format_ali(sc, T, frame_s, targets, a[:S].tolist(), b[:S].tolist(), self.vocab))
                if sc == sc and sc != float('-inf'):
                    row = segment_row(f, a[:S].tolist(), T, frame_s)
                    if row is not None:
                        rows.append(row)
                else:
                    n_bad += 1
                    print('[WARNING] %s: no alignment (score %s: %d tokens, %d encoder frames)' % (f, sc, S, T))
                n += 1
        with open(os.path.join(self.logdir, 'segments.csv'), 'w') as out:
            out.write('\n'.join(rows) + '\n')
        self.verbose('Aligned %d files (%d without an alignment, %s posteriors) into %s, %.2f s'
                     % (n, n_bad, self.paras.asr_output, self.logdir, time.perf_counter() - t0))
        return n


SYNTH_HEADER = 'file,tokens,steps,frames,seconds,reached,focus,backward,skips,covered'


def synth_row(file, tokens, steps, frames, seconds, reached, focus, backward, skips, covered):
    """one row of synth.csv (SYNTH_HEADER): the .phn file, its phones, the decoder steps and frames kept, the length of the waveform in
    seconds (%.4f), whether the end was detected, the mean peak attention weight (%.4f), backward jumps, skips, phones attended"""
    return '%s,%d,%d,%d,%.4f,%d,%.4f,%d,%d,%d' % (file, tokens, steps, frames, seconds, reached, focus, backward, skips, covered)


def read_synth_transcripts(phn_dir, vocab, vocab_size):
    """the .phn files of --synth-phn-dir sorted by name -> ([file], [id list]) through ctc_align.read_phn (ids or `vocab` symbols, the
    `score<TAB>tokens` lines of --transcribe-wav-dir as they are) and vqvae.check_transcript.  ValueError naming the file for an
    unreadable or empty transcript, an id 0 inside one or an id outside the vocabulary; also when the directory holds none."""
    from .ctc_align import read_phn
    from .vqvae import check_transcript
    files = sorted(f for f in os.listdir(phn_dir) if f.endswith('.phn'))
    if not files:
        raise ValueError('--synth-phn-dir %s: no .phn files' % phn_dir)
    transcripts = []
    for f in files:
        try:
            transcripts.append(check_transcript(read_phn(os.path.join(phn_dir, f), vocab), vocab_size))
        except ValueError as e:
            raise ValueError('--synth-phn-dir: %s: %s' % (f, e))
    return files, transcripts


class Synthesiser(BaseSolver):
    """main.py --synth-phn-dir DIR: the .phn transcripts of DIR, sorted by name, in batches of --batch-size -> VQVAE.synthesise (speaker
    --synth-sid, --max-frames-per-phone frames of decode budget per phone) -> metrics.attention_endpoints (--end-patience,
    --end-max-jump) -> one host read of the end steps per batch -> every utterance cut to frames = max(r * end, audio.min_frames) and
    written as <logdir>/<name>-mel.npy, -spec.npy, -align.npy (align[:end, :n]), -dur.npy (int32 (n,), frames per phone) and, with
    --gen-wav, -pred.wav (AudioConverter.vocode_batch on the trimmed device tensors: each utterance is what it gives alone;
    --gen-wav-feat mel vocodes the mel), plus one synth.csv (SYNTH_HEADER).  -dur.npy is r * dur[:n] of attention_endpoints with the
    steps whose peak lies past the last phone -- on the appended index 0 or the padding, which the end rule counts as the last phone
    too -- added to the last phone, so the durations sum to r * end.  An utterance whose end was not found (reached == 0) or whose
    attention holds a NaN or an infinity gets a [WARNING] line and is written at full length.
    Padded phones are seen by the encoder and the attention, unmasked: this follows the reference and every batch the model was
    trained on, so an utterance's output depends on its batch's longest transcript; --batch-size 1 gives the alone result.
    Every transcript is read in load_data: a bad one (read_synth_transcripts), one too long for the kernel or a --synth-sid outside the
    speaker table stops the run, naming the file, before anything is written.  Without --load the synthetic weights are used."""

    def load_data(self):
        from .audio import load_audio_transform
        from .vqvae import synth_frames
        vocab = getattr(self.paras, 'vocab', None)
        self.vocab = read_vocab(vocab) if vocab else None
        self.phn_dir = self.paras.synth_phn_dir
        self.files, self.transcripts = read_synth_transcripts(self.phn_dir, self.vocab, self.vocab_size)
        self.sid = int(getattr(self.paras, 'synth_sid', 0) or 0)
        if not 0 <= self.sid < self.n_spkr:
            raise ValueError('--synth-sid %d: the speaker table has ids 0 .. %d' % (self.sid, self.n_spkr - 1))
        mfpp = getattr(self.paras, 'max_frames_per_phone', None)
        self.max_frames_per_phone = float(SYNTH_MAX_FRAMES_PER_PHONE if mfpp is None else mfpp)
        self.patience, self.max_jump = int(getattr(self.paras, 'end_patience', 3)), int(getattr(self.paras, 'end_max_jump', 4))
        r = int(self.config['model']['decoder']['decoder']['n_frames_per_step'])
        for f, t in zip(self.files, self.transcripts):
            steps = synth_frames(len(t), r, self.max_frames_per_phone) // r
            if len(t) + 1 > toolops.AE_MAX_L or steps > toolops.AE_MAX_S:
                raise ValueError('--synth-phn-dir: %s: %d phones decode %d steps; the end-of-speech kernel takes at most %d phones and %d steps'
                                 % (f, len(t), steps, toolops.AE_MAX_L - 1, toolops.AE_MAX_S))
        self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        return self

    def set_model(self):
        self.model = self._build_model().eval()
        self.n_frames_per_step = self.model.n_frames_per_step
        if not self.load_ckpt():
            from .synthetic import load_synthetic
            load_synthetic(self.model, seed=getattr(self.paras, 'seed', 0) + 1234)
        return self

    def write_batch(self, files, transcripts, mel, lin, align, enc_len):
        """one decoded batch (device tensors; enc_len as attention_endpoints takes it) -> the files of its utterances in self.logdir;
        -> the rows of synth.csv.  One host read of the end steps, the diagnostics and the durations, all integers of a few KiB."""
        from .audio import min_frames, write_wav
        from .metrics import attention_endpoints
        conv, r = self.audio_converter, self.n_frames_per_step
        B, S, T = align.shape[0], align.shape[1], mel.shape[1]
        ep = attention_endpoints(align, enc_len, self.patience, self.max_jump)
        host = torch.cat([torch.stack([ep.end, ep.reached, ep.n_back, ep.n_skip, ep.covered, ep.nonfinite, ep.focus.view(torch.int32)], 1),
                          ep.dur], 1).cpu().numpy()                  # (the one host read)
        floor = min_frames(conv.n_fft, conv.hop_length)
        kept, rows = [], []
        for i, (f, tr) in enumerate(zip(files, transcripts)):
            n = len(tr)
            end, reached, back, skip, cov, bad = (int(v) for v in host[i, :6])
            focus = float(host[i, 6:7].view(np.float32)[0])
            if not reached or bad:
                print('[WARNING] %s: %s; written at full length (%d steps)'
                      % (f, 'the attention holds a NaN or an infinity' if bad else
                         'the attention did not stay on the last phone for %d steps' % self.patience, S))
                end = S
            frames = min(max(r * end, floor), T)
            dur = host[i, 7:7 + n].astype(np.int32)
            dur[n - 1] += host[i, 7 + n:].sum()                      # peaks past the last phone: its trailing steps
            stem = os.path.join(self.logdir, os.path.splitext(f)[0])
            np.save(stem + '-mel.npy', mel[i, :frames].cpu().numpy().astype(np.float32), allow_pickle=False)
            np.save(stem + '-spec.npy', lin[i, :frames].cpu().numpy().astype(np.float32), allow_pickle=False)
            np.save(stem + '-align.npy', align[i, :end, :n].cpu().numpy(), allow_pickle=False)
            np.save(stem + '-dur.npy', (r * dur).astype(np.int32), allow_pickle=False)
            kept.append((stem, frames))
            rows.append(synth_row(f, n, end, frames, conv.hop_length * (frames - 1) / conv.sr, reached, focus, back, skip, cov))
        if getattr(self.paras, 'gen_wav', False):
            use_mel = getattr(self.paras, 'gen_wav_feat', 'linear') == 'mel'
            src = mel if use_mel else lin
            wavs = vocode(conv, [src[i, :frames] for i, (_, frames) in enumerate(kept)], 'mel' if use_mel else 'spec', self.paras)
            for (stem, _), w in zip(kept, wavs):
                write_wav(stem + '-pred.wav', w, conv.sr)
        return rows

    def exec(self):
        os.makedirs(self.logdir, exist_ok=True)
        B = max(1, int(self.paras.batch_size))
        t0, rows = time.perf_counter(), [SYNTH_HEADER]
        for i in range(0, len(self.files), B):
            files, trs = self.files[i:i + B], self.transcripts[i:i + B]
            mel, lin, align, enc_len = self.model.synthesise(trs, self.sid, self.max_frames_per_phone)
            ops.check_persist_status(self.device)
            rows += self.write_batch(files, trs, mel, lin, align, enc_len)
        with open(os.path.join(self.logdir, 'synth.csv'), 'w') as out:
            out.write('\n'.join(rows) + '\n')
        self.verbose('Synthesised %d transcripts (speaker %d, patience %d) into %s, %.2f s'
                     % (len(rows) - 1, self.sid, self.patience, self.logdir, time.perf_counter() - t0))
        return len(rows) - 1


class LazyStats(dict):
    """step statistics whose device scalars become Python floats when they are READ (st['loss'], st.items(), ...): a training loop
    that only logs every n-th step never waits for the GPU in between (TtsTrainer.async_stats)"""

    on_nonfinite = None      # callable(stats): runs once when a non-finite 'grad_norm' is read (the device skipped that update)

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if torch.is_tensor(v):
            v = float(v)
            dict.__setitem__(self, k, v)
            if k == 'grad_norm' and not math.isfinite(v) and self.on_nonfinite is not None:     # (NaN or inf: what the device guard skips)
                cb, self.on_nonfinite = self.on_nonfinite, None
                cb(self)
        return v

    def put(self, k, v):
        """the value of device scalar k, read by somebody else (drain_stats reads many in one copy); same side effects as reading it here"""
        dict.__setitem__(self, k, v)
        if k == 'grad_norm' and not math.isfinite(v) and self.on_nonfinite is not None:
            cb, self.on_nonfinite = self.on_nonfinite, None
            cb(self)

    def materialise(self):
        """read every device scalar (one wait for the GPU): the entry no longer holds device memory"""
        for k in dict.keys(self):
            self[k]
        return self

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in dict.keys(self)]

    def values(self):
        return [self[k] for k in dict.keys(self)]


class TtsTrainer(BaseSolver):
    """Synthetic-batch counterpart of the paired TTS branch of VqvaeTrainer.exec (bin/train_vqvae.py:132-270)
    with BaseSolver.backward (src/solver.py:138-151): per step

        tf_rate = optimizer.pre_step(step)                       (lr schedule, zero_grad)
        mel, linear = model.text_to_speech(text, sid, ..., paired_teacher=mel, tf_rate)
        loss = tts_weight * (freq_loss(mel) + freq_loss(linear))
        loss.backward(); [all-reduce over ranks]; clip_grad_norm_(5.0); optimizer.step()

    Forward, loss, backward, gradient clipping and Adam all run on the HIP kernels (semi_tts_amd/autograd.py,
    semi_tts_amd/optim.py).  The paired TTS branch alone (`main.py --tts-only`, `bench.py --workload train`); the whole loop of
    the reference -- the alternating speech <-> text cycles with the CTC speech encoder, codebook and run-length merge -- is
    VqvaeTrainer below, main.py's default mode."""
    GRAD_CLIP = 5.0
    STATIC_GRAPH = True      # the paired TTS step produces the same gradients in the same order every step (GradReducer: one hook per bucket)
    async_stats = False      # True: train_step never waits for the GPU -- LazyStats, NaN steps skipped on the device (optim.FusedAdam guard)

    @staticmethod
    def clip_grad_norm_(params, max_norm, pre_scale=1.0):
        from .optim import clip_grad_norm_
        return clip_grad_norm_(list(params), max_norm, pre_scale)

    def _clip(self):
        """clip_grad_norm_(GRAD_CLIP) over the model; under data parallelism the 1 / world of the gradient average rides in it"""
        scale = getattr(self, '_grad_scale', 1.0)
        params = self.__dict__.get('_clip_params')
        if params is None:       # (nn.Module.parameters() walks the module tree through three generators: 0.25 ms per call for ~110 parameters)
            params = self._clip_params = list(self.model.parameters())
        if scale != 1.0:
            return self.clip_grad_norm_(params, self.GRAD_CLIP, pre_scale=scale)
        return self.clip_grad_norm_(params, self.GRAD_CLIP)

    def __init__(self, config, paras, mode='train'):
        super().__init__(config, paras, mode)
        hp = config['hparas']
        self.hp = hp
        self.max_step = int(getattr(paras, 'max_step', None) or hp.get('max_step', 1))
        self.tts_weight = float(hp.get('tts_weight', 1.0))
        self.sample_rate = config['data']['audio']['sample_rate']
        self.log = []
        self._unread = []
        if getattr(paras, 'async_stats', False):
            self.async_stats = True

    def _load_corpus(self, splits, batch_sizes):
        """--corpus: the splits of data.corpus as device-resident sets (semi_tts_amd/corpus.py); vocab_size and n_spkr from its files"""
        from .audio import load_audio_transform
        from .corpus import load_splits
        pa = self.paras
        self.r = self.config['model']['decoder']['decoder']['n_frames_per_step']
        self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        if self.audio_converter.n_mels != self.n_mels:
            raise ValueError('--corpus: data.audio has %d mels, the model %d' % (self.audio_converter.n_mels, self.n_mels))
        self.corpus, self.corpus_sets = load_splits(
            self.config['data']['corpus'], self.audio_converter, self.r, splits, batch_sizes, seed=int(getattr(pa, 'seed', 0)),
            rank=int(os.environ.get('RANK', 0)), world=int(os.environ.get('WORLD_SIZE', 1)), resample=bool(getattr(pa, 'resample', False)),
            max_frames=getattr(pa, 'max_frames', None), max_gb=getattr(pa, 'corpus_max_gb', None), verbose=self.verbose,
            trim=trim_args(pa), loudness=loudness_args(pa))
        self.vocab_size, self.n_spkr = self.corpus.vocab_size, self.corpus.n_spkr
        return self.corpus_sets

    def load_data(self):
        from .synthetic import synthetic_train_batch
        B = int(getattr(self.paras, 'batch_size', None) or self.config['data']['corpus'].get('batch_size', 8))
        if getattr(self.paras, 'corpus', False):              # --tts-only --corpus: the paired split
            self._load_corpus(['paired'], {'paired': B})
            self.batches = None
            return self
        frames = int(getattr(self.paras, 'frames', 256))
        n = int(getattr(self.paras, 'n_batches', 1))
        self.r = self.config['model']['decoder']['decoder']['n_frames_per_step']
        rank = int(os.environ.get('RANK', 0))
        self.batches = [synthetic_train_batch(B, frames, self.r, self.vocab_size, self.n_spkr, self.n_mels, self.linear_dim,
                                              seed=1000 * rank + i + getattr(self.paras, 'seed', 0))
                        for i in range(n)]
        return self

    def set_model(self):
        from .optim import Optimizer
        from .synthetic import load_synthetic
        self.model = self._build_model().train()
        self._clip_params = None
        hp = self.hp
        self.optimizer = Optimizer(self.model.parameters(), hp['optimizer'], hp['lr'], hp['lr_scheduler'],
                                   **{k: hp[k] for k in ('tf_start', 'tf_end', 'tf_step') if k in hp})
        if not self.load_ckpt():
            load_synthetic(self.model, seed=getattr(self.paras, 'seed', 0) + 1234)
        from . import parallel
        parallel.sync_batchnorm(True)        # no-op for a single process; global-batch statistics under torch.distributed
        parallel.broadcast_parameters(self.model)
        self._attach_reducer()
        # the detached postnet branch on a second stream (Tacotron2.postnet_side; ST_POSTNET_SIDE=0 turns it off) -- without data parallelism
        # only: a gradient bucket that goes out while the backward still runs must not mix gradients of two streams.  Bitwise the serial step
        # (test_postnet_branch_on_a_second_stream_gives_bitwise_the_serial_step).  Measured (round 6, A/B pairs in one process on the box of
        # the final artifacts): 8.83 -> 8.62 ms per C2 training step, with or without the loop graphs (earlier boxes of the round: -0.07 ...
        # -0.18 ms): the ~1 ms of CBHG forward / backward mostly hides behind the decoder's backward through time, the host's issue time
        # (7.9 ms) is the next floor.
        self.postnet_side = (self.reducer is None and bool(getattr(self.model.tts, 'separate_postnet', False))
                             and os.environ.get('ST_POSTNET_SIDE', '1') != '0')
        # (Tacotron2.postnet_side itself is raised only around the trainer's own text_to_speech calls, _tts: anybody else who calls the model
        # gets every output on the stream it called on)
        return self

    def _tts(self, *args, **kw):
        """VQVAE.text_to_speech for a step of THIS trainer: with `postnet_side` the postnet output comes back on the second stream
        (Tacotron2.postnet_stream) and the caller continues the branch there (train_step, VqvaeTrainer._side_branch)"""
        tts = self.model.tts
        tts.postnet_side = bool(getattr(self, 'postnet_side', False))
        try:
            return self.model.text_to_speech(*args, **kw)
        finally:
            tts.postnet_side = False

    def _attach_reducer(self):
        """under torch.distributed: gradients live in flat buckets that are all-reduced while the backward pass still runs"""
        from . import parallel
        self.reducer = None
        if parallel.dist_on():               # more than one rank, or collectives forced in a world of one (bench.py --dist)
            # the static-graph promise (one hook per bucket) only where the step's autograd graph cannot change: no teacher-forcing
            # schedule (own-output feedback adds the prenet's gradients to the graph); the reducer checks the promise anyway
            static = self.STATIC_GRAPH and not getattr(self.optimizer, 'tf_type', False)
            self.reducer = parallel.GradReducer(self.model.parameters(), static_graph=static, defer_average=True)
        return self.reducer

    def _reduce_gradients(self):
        """sum the gradients over the ranks; what they must still be multiplied by (1 / world) goes into the clip launch"""
        from . import parallel
        self._grad_scale = 1.0
        if getattr(self, 'reducer', None) is not None:
            n = self.reducer.finish()
            self._grad_scale = self.reducer.grad_scale
            return n
        return parallel.allreduce_gradients(self.model.parameters())

    def freq_loss(self, pred, label):
        from . import autograd as AG
        hp = self.hp
        return AG.freq_loss(pred, label, self.sample_rate, self.n_mels, hp.get('freq_loss_type', 'mse'),
                            hp.get('differential_loss', True), hp.get('emphasize_linear_low', True))

    def train_step(self, text, sid, mel, linear, _masks=None):
        from . import parallel
        parallel.collective_counts(reset=True)
        tf_rate = self.optimizer.pre_step(self.step)
        if getattr(self, 'reducer', None) is not None:
            self.reducer.prepare()
        mel_pred, linear_pred, align, _, _, _, _, _ = self._tts(
            text, sid, None, None, None, None, mel, None, tf_rate, _masks=_masks)
        from . import autograd as AG
        side = getattr(self.model.tts, 'postnet_stream', None)
        w = self.tts_weight
        if side is not None:
            # separate_postnet (src/tts.py:47-50): the postnet saw mel_pred.detach(), on a second stream.  Its loss and its whole backward
            # (CBHG incl. both GRU passes: ~1 ms that neither feeds nor waits for the decoder's backward through time) stay on that
            # stream, beside the main chain; the streams join before the gradients are used.  d total / d linear_loss = tts_weight.
            with torch.cuda.stream(side):
                linear_loss = self.freq_loss(linear_pred, linear)
                lin_total, = AG.scalar_combine([[w]], [linear_loss])
                lin_total.backward()
                ops.flush_wgrads()
                ev = self.__dict__.setdefault('_side_event', torch.cuda.Event())
                ev.record(side)
            ops.side_pending(ev)                      # (the one-launch BiLSTM backward of the text encoder waits for it: it needs every compute unit)
            mel_loss = self.freq_loss(mel_pred, mel)
            mel_total, = AG.scalar_combine([[w]], [mel_loss])
            mel_total.backward()
            torch.cuda.current_stream().wait_event(ev)
            ops.side_pending(None)
            with torch.no_grad():
                total, = AG.scalar_combine([[1.0, 1.0]], [mel_total.detach(), lin_total.detach()])
        else:
            mel_loss = self.freq_loss(mel_pred, mel)
            linear_loss = self.freq_loss(linear_pred, linear)
            total, = AG.scalar_combine([[w, w]], [mel_loss, linear_loss])     # (one launch; `w * (a + b)` is two, and three backward)
            total.backward()
        self._reduce_gradients()
        grad_norm = self._clip()
        from .optim import FusedAdam
        if self.async_stats and torch.is_tensor(grad_norm) and grad_norm.is_cuda and isinstance(getattr(self.optimizer, 'opt', None), FusedAdam):
            # no host round trip inside the step: the NaN check of BaseSolver.backward (src/solver.py:147-150) runs on the device (a
            # non-finite norm makes the Adam launch a no-op) and the statistics stay device scalars until somebody reads them
            opt_step = getattr(getattr(self.optimizer, 'opt', None), 'guarded_steps', 0)      # (the key of this update in the optimiser's log)
            self.optimizer.step(guard_norm=grad_norm)
            self.step += 1
            st = self._ring_stats(dict(loss=total, mel_loss=mel_loss, linear_loss=linear_loss, grad_norm=grad_norm),
                                  tf_rate=tf_rate, lr=self.optimizer.lr_at(self.step - 1), step=self.step - 1, opt_step=opt_step)
            return st
        gn = float(grad_norm)
        if gn != gn:
            self.check_device_status()                   # (a starved one-launch LSTM layer is an error, not a skipped step)
            self.verbose('Error : grad norm is NaN @ step ' + str(self.step))
        else:
            self.optimizer.step()
        self.step += 1
        return dict(loss=float(total.detach()), mel_loss=float(mel_loss.detach()), linear_loss=float(linear_loss.detach()), grad_norm=gn,
                    tf_rate=tf_rate, lr=self.optimizer.lr_at(self.step - 1))

    STATS_COLS = 8           # device scalars per row of the statistics ring

    def _ring_stats(self, scalars, **extras):
        """async_stats: the step's device scalars go into a row of a persistent ring: LazyStats then holds VIEWS, no allocation outlives
        the step, and the caching allocator hands every tensor of the next step the address it had in this one -- which is what
        lets the optimiser's device-side tables (optim.hip: mt_table) be reused instead of rebuilt (scalars kept alive for 4 ... 8 steps
        made the addresses wander with a period of ~13 steps).  An event behind the row lets drain_stats wait for THIS step only."""
        keys = tuple(scalars)
        vals = [scalars[k] for k in keys]
        dev = vals[-1].device
        ring = self.__dict__.get('_stats_ring')
        if ring is None or ring.device != dev:
            ring = self._stats_ring = torch.zeros(self.STATS_RING, self.STATS_COLS, device=dev)
            self._stats_slot = 0
            self._stats_host = torch.zeros(self.STATS_RING, self.STATS_COLS).pin_memory()
            self._stats_events = [torch.cuda.Event() for _ in range(self.STATS_RING)]
            self._stats_stream = torch.cuda.Stream(device=dev)
        slot = self._stats_slot
        row = ring[slot]
        self._stats_slot = (slot + 1) % self.STATS_RING
        torch.stack([v.detach().reshape(()) for v in vals], out=row[:len(keys)])
        self._stats_events[slot].record()                 # (drain_stats waits for THIS step only, on a stream of its own)
        st = LazyStats({k: row[i] for i, k in enumerate(keys)}, **extras)
        st.ring_slot, st.ring_keys = slot, keys
        st.on_nonfinite = self._skipped_on_device
        self._unread.append(st)
        # bounded: at most STATS_WINDOW steps of device scalars are alive.  While the one-launch BiLSTM is in use the window is short:
        # a starved layer poisons every forward until somebody looks, and every poisoned step is an update skipped on the device
        # (only the older half is read: the wait is for a step that finished a while ago, the GPU keeps the newer half queued and the
        # host its lead -- a full drain every eighth step cost the data-parallel step 0.6 ms once the host was no longer far ahead)
        window = min(self.STATS_WINDOW_PERSIST if ops.LSTM_PERSIST else self.STATS_WINDOW, self.STATS_RING - 1)
        if len(self._unread) >= window:
            self.drain_stats(keep=window // 2)
        return st

    STATS_WINDOW = 64        # async_stats: steps whose statistics may stay unread on the device
    STATS_RING = 256         # rows of the ring the unread statistics live in (> any window)
    STATS_WINDOW_PERSIST = int(os.environ.get('ST_STATS_WINDOW_PERSIST', '8'))     # ... while ops.LSTM_PERSIST is on (see train_step)

    def check_device_status(self):
        """a kernel of the training step reported starvation since the last check (the one-launch BiLSTM's status word)?  Such a
        forward is NaN and the guarded Adam skips its update: the layer runs as one launch per time step from now on.  The synchronous
        trainer loses one step to it; the asynchronous one notices when its statistics window drains (at most STATS_WINDOW_PERSIST
        steps, each skipped on the device and rolled back individually).  Returns True if it fell back."""
        if ops.persist_starved(self.device):
            ops.degrade('one-launch BiLSTM layer', 'one launch per time step (ops.LSTM_PERSIST = False)')
            ops.LSTM_PERSIST = False
            return True
        return False

    def _skipped_on_device(self, st):
        """a step whose gradient norm turned out non-finite (read late, async_stats): the device skipped that update"""
        self.check_device_status()
        opt = getattr(self.optimizer, 'opt', None)
        if hasattr(opt, 'rollback_step'):
            # the host-side Adam step counts of the parameters of THAT update ran one ahead since then (bias corrections)
            opt.rollback_step(dict.get(st, 'opt_step'))
        self.verbose('Error : grad norm is not finite @ step %s (update skipped on the device)' % dict.get(st, 'step', '?'))

    def drain_stats(self, keep=0):
        """read the statistics of the steps issued so far -- all but the `keep` newest (waits for the GPU once: for the newest step that
        is read).  The device scalars of all those steps come back in ONE copy (one small gather launch) instead of one per scalar."""
        n = len(self._unread) - keep
        if n <= 0:
            return
        pending, self._unread = self._unread[:n], self._unread[n:]
        ringed = [st for st in pending if getattr(st, 'ring_slot', None) is not None]
        if ringed and self.__dict__.get('_stats_ring') is not None:
            # the ring comes to the host on a stream of its own, behind the event of the NEWEST step that is read: the host waits for that
            # step (finished a while ago when `keep` > 0), not for what has been issued since -- a read on the compute stream would be
            # ordered behind everything queued on it.  No device allocation either (see train_step).
            side = self._stats_stream
            side.wait_event(self._stats_events[ringed[-1].ring_slot])
            with torch.cuda.stream(side):
                self._stats_host.copy_(self._stats_ring, non_blocking=True)
            side.synchronize()
            host = self._stats_host.tolist()
            for st in ringed:
                r = host[st.ring_slot]
                for k, v in zip(st.ring_keys, r):
                    if torch.is_tensor(dict.__getitem__(st, k)):
                        st.put(k, v)
        for st in pending:
            st.materialise()
            self._stats_read(st)

    def _stats_read(self, st):
        """hook: the scalars of a step have just been read on the host"""

    def exec(self):
        t0 = time.perf_counter()
        frames = 0
        while self.step < self.max_step:
            if self.batches is None:                          # --corpus
                mel, _, linear, text, sid = self.corpus_sets['paired'].fetch()
            else:
                text, sid, mel, linear = (t.to(self.device) for t in self.batches[self.step % len(self.batches)])
            st = self.train_step(text, sid, mel, linear)
            frames += mel.shape[0] * mel.shape[1]
            self.log.append(st)
            if self.step == 1 or self.step % 10 == 0:
                self.verbose('Tr stat | step %d | Loss - %.4f | Grad. Norm - %.3f | lr %.2e' %
                             (self.step, st['loss'], st['grad_norm'], st['lr']))
        torch.cuda.synchronize()
        self.drain_stats()
        self.check_device_status()
        dt = time.perf_counter() - t0
        if getattr(self.paras, 'save', False):
            self.save_checkpoint('latest.pth', self.log[-1]['loss'] if self.log else 0.0)
        self.verbose('%d steps, %d frames in %.2f s (%.0f frames/s incl. first-step set-up)' %
                     (len(self.log), frames, dt, frames / max(dt, 1e-9)))
        return self.log


EPS = 1e-10                      # ref: bin/train_vqvae.py:18
SPEC_PAD_VALUE = 0.0             # ref: bin/train_vqvae.py:15 (what collect_fn pads spectrograms with)
CKPT_STEP = 10000                # ref: bin/train_vqvae.py:17
BEST_TTS_LOSS_INIT, BEST_PER_INIT = 100.0, 2.0          # ref: bin/train_vqvae.py:26-27 (a PER of 2.0 or more never saves)


def validation_checkpoints(step, tts_loss, per, post_per, best, store_best_per):
    """The checkpoint rules of VqvaeTrainer.validate (bin/train_vqvae.py:376-403) as a pure function.  best = (best_tts_loss, best_per);
    post_per is None for a model without an ASR postnet.  -> ([(file name, score), ...] in the order the reference saves them, new best).
    Kept as the reference has them: a post-net PER is compared with best_per AFTER the encoder's PER has updated it, best_post_per.pth
    is written at step 1 too, and best_per records whichever of the two was lower last."""
    best_tts, best_per = best
    files = []
    if store_best_per:
        if per < best_per:
            best_per = per
            files.append(('best_per.pth', per))
        if post_per is not None and post_per < best_per:
            best_per = post_per
            files.append(('best_post_per.pth', post_per))
    else:
        if tts_loss < best_tts:
            best_tts = tts_loss
            if step > 1:
                files.append(('tts_%d.pth' % step, tts_loss))
        if per < best_per:
            best_per = per
            if step > 1:
                files.append(('asr_%d.pth' % step, per))
        if post_per is not None and post_per < best_per:
            best_per = post_per
            files.append(('best_post_per.pth', post_per))
        if step > 1 and step % CKPT_STEP == 0:
            files.append(('step_%d.pth' % step, tts_loss))
    return files, (best_tts, best_per)


class VqvaeTrainer(TtsTrainer):
    """The speech -> text -> speech cycle of VqvaeTrainer.exec (bin/train_vqvae.py:139-176,208-270) on synthetic batches:

        pair_prob, _, unpair_prob, unpair_latent, unpair_len = model.speech_to_text(aug_mel, unpair_aug_mel)
        mel, linear, ..., unpair_mel, unpair_linear, ...     = model.text_to_speech(text, sid, unpair_sid, unpair_latent, ...)
        loss = asr_weight * CTC(log(pair_prob + EPS), text) + tts_weight * (freq_loss(mel) + freq_loss(linear))
               [+ unpair_speech_weight * (freq_loss(unpair_mel) + freq_loss(unpair_linear))]
        loss.backward(); all-reduce; clip_grad_norm_(5.0); optimizer.step()

    Everything between the inputs and the gradients runs on the HIP kernels: the CTC speech encoder and its backward
    (asr.py), the codebook lookup with the straight-through estimator (autograd.vq_l2), the run-length merge (autograd.mean_forward),
    the TTS branch, the CTC loss (autograd.ctc_loss)."""
    STATIC_GRAPH = False     # the cycles' autograd graphs depend on the data (ignore_speech_cycle, skip_prob draws, txt_update_codebook)

    def ctc_loss(self, prob, text, model_input=None, apply_log=True):
        """compute_ctcloss (bin/train_vqvae.py:430-444): the targets are the non-zero tokens; torch.nn.CTCLoss() defaults (blank 0, mean
        over the batch of nll / target length).  Without paras.actual_len every frame counts.  With it utterance b counts the frames of
        `model_input` (B, T, n_mels) that are not entirely SPEC_PAD_VALUE, divided by the encoder's time reduction (:437-438): computed
        and consumed on the device (ops.frame_lengths -> st_ctc_loss_len), no host read."""
        from . import autograd as AG
        return AG.ctc_loss(prob, text, EPS, apply_log=apply_log, in_len=self._ctc_in_len(model_input))

    def _ctc_in_len(self, model_input):
        if not getattr(self.paras, 'actual_len', False) or model_input is None:
            return None
        return ops.frame_lengths(model_input.contiguous(), SPEC_PAD_VALUE, int(self.model.time_reduce_factor))

    def _async(self):
        from .optim import FusedAdam
        return self.async_stats and isinstance(getattr(self.optimizer, 'opt', None), FusedAdam)

    def _paired_losses(self, pair_prob, pair_post_prob, pm, pl, mel, linear, text, terms, stats, linear_loss=None, aug_mel=None):
        """the terms both cycles share (bin/train_vqvae.py:208-224): CTC on the paired posteriors (+ the ASRPostnet term) and
        freq_loss on the paired reconstruction.  Appends (weight, loss, statistics name) to `terms`: the weighted sum itself -- and the
        partial sums the log prints -- are ONE launch in _finish_step (the reference's chain of one-element kernels)."""
        hp = self.hp
        asr_loss = self.ctc_loss(pair_prob, text, aug_mel)                                        # :209
        asr_w = float(hp.get('asr_weight', 1.0))
        if self.model.use_asr_postnet:                                                            # :210-213
            from . import autograd as AG
            pw = float(self.model.asr_postnet_weight)
            asr_post_loss = self.ctc_loss(pair_post_prob, text, aug_mel, apply_log=False)         # compute_ctcloss(..., apply_log=False)
            terms += [(asr_w * (1.0 - pw), asr_loss, None), (asr_w * pw, asr_post_loss, None)]
            stats['asr_post_loss'] = asr_post_loss.detach()
        else:
            terms.append((asr_w, asr_loss, None))                                                 # :215
        # (:216-218: a NaN / inf CTC value is counted when the statistics are read -- as in the reference it is already inside total,
        # the gradient norm is then NaN and the update is skipped)
        stats['asr_loss'] = asr_loss.detach()
        # (linear_loss: the value _side_branch computed -- and sent backward -- on the postnet's stream)                           :221-224
        terms += [(self.tts_weight, self.freq_loss(pm, mel), 'tts_loss'),
                  (self.tts_weight, linear_loss if linear_loss is not None else self.freq_loss(pl, linear), 'tts_loss')]

    def _total(self, terms, stats):
        """total = sum of weight * loss over `terms`; the named partial sums (unweighted, as the reference logs them) land in `stats`"""
        from . import autograd as AG
        names = []
        for _, _, nm in terms:
            if nm is not None and nm not in names:
                names.append(nm)
        W = [[w for w, _, _ in terms]] + [[1.0 if nm == k else 0.0 for _, _, nm in terms] for k in names]
        outs = AG.scalar_combine(W, [x for _, x, _ in terms])
        for k, v in zip(names, outs[1:]):
            stats[k] = v
        return outs[0]

    def _count_ctc_nan(self, st):
        for k in ('asr_loss', 'unpair_text_loss'):
            if k in st and not math.isfinite(st[k]):
                self.ctc_nan = getattr(self, 'ctc_nan', 0) + 1

    def _side_branch(self, side_terms):
        """separate_postnet (src/tts.py:47-50) cuts the gradient between the decoder and the postnet: when Tacotron2 ran the postnet on the
        second stream (`postnet_stream`, TtsTrainer.set_model), the branch's losses (freq_loss of the linear spectrograms: `side_terms`) and its
        whole backward (CBHG incl. both GRU passes) are issued there NOW, beside whatever the main stream does next; _finish_step joins the
        streams after the main backward.  d total / d loss_i = w_i whatever the rest of the sum, so the two backward passes give the gradients
        of the one pass bit for bit (the branch's parameters get no other contribution).  Returns None when the postnet ran on the main stream,
        else (event, the loss values in the order of `side_terms`): the caller puts them where the one-stream step has these terms."""
        side = getattr(self.model.tts, 'postnet_stream', None)
        if side is None:
            return None
        with torch.cuda.stream(side):
            vals = [f() for _, f, _ in side_terms]
            total = self._total([(w, x, nm) for (w, _, nm), x in zip(side_terms, vals)], {})
            total.backward()
            ops.flush_wgrads()
            ev = self.__dict__.setdefault('_side_event', torch.cuda.Event())
            ev.record(side)
        ops.side_pending(ev)                      # (one-launch BiLSTM layers of the main stream wait for it: they need every compute unit)
        return ev, [x.detach() for x in vals]

    def _finish_step(self, terms, stats, tf_rate, kind, side=None):
        """BaseSolver.backward (src/solver.py:138-151) + the step counter.  Synchronous form: the scalars are read here, a NaN gradient
        norm skips the update (as the reference does).  async_stats: nothing is read -- the scalars go into the statistics ring, the
        guarded Adam skips a non-finite step on the device (TtsTrainer.train_step).  `side`: what _side_branch returned."""
        if side is None:
            total = self._total(terms, stats)
            total.backward()
        else:
            # the terms the second stream has already sent backward (no graph: detached values) stay out of this backward pass ...
            self._total([t for t in terms if t[1].requires_grad], {}).backward()
            torch.cuda.current_stream().wait_event(side[0])
            ops.side_pending(None)
            # ... and the reported sums are ONE launch over all terms in the order of the one-stream step: the same arithmetic, bit for bit
            with torch.no_grad():
                total = self._total([(w, x.detach(), nm) for w, x, nm in terms], stats)
        self._reduce_gradients()
        grad_norm = self._clip()
        lr = self.optimizer.lr_at(self.step)
        if self._async() and torch.is_tensor(grad_norm) and grad_norm.is_cuda:
            opt_step = getattr(self.optimizer.opt, 'guarded_steps', 0)
            self.optimizer.step(guard_norm=grad_norm)
            self.step += 1
            scalars = dict(stats, loss=total, grad_norm=grad_norm)
            return self._ring_stats(scalars, tf_rate=tf_rate, lr=lr, step=self.step - 1, opt_step=opt_step, kind=kind,
                                    **{k: v for k, v in self._step_info.items()})
        gn = float(grad_norm)
        if gn == gn:
            self.optimizer.step()
        else:
            self.check_device_status()                   # (a starved one-launch LSTM layer: per-step form from the next step on)
            self.verbose('Error : grad norm is NaN @ step ' + str(self.step))
        self.step += 1
        out = {k: float(v) for k, v in stats.items()}
        out.update(loss=float(total.detach()), grad_norm=gn, tf_rate=tf_rate, lr=lr, kind=kind, **self._step_info)
        self._count_ctc_nan(out)
        return out

    def _begin_step(self):
        from . import parallel
        parallel.collective_counts(reset=True)
        self._step_info = {}
        tf_rate = self.optimizer.pre_step(self.step)
        if getattr(self, 'reducer', None) is not None:
            self.reducer.prepare()
        return tf_rate

    def speech_first_step(self, mel, aug_mel, linear, text, sid, unpair_mel=None, unpair_aug_mel=None, unpair_linear=None,
                          unpair_sid=None, _masks=None, _asr_masks=None):
        """The speech -> text -> speech cycle of VqvaeTrainer.exec (bin/train_vqvae.py:159-176,208-233).  The only host read of the
        forward pass is the merged lengths of the unpaired latents (autograd.mean_forward): they fix the text length the TTS branch
        runs at (the reference reads every index, src/vqvae.py:225)."""
        hp = self.hp
        tf_rate = self._begin_step()
        pair_prob, _, unpair_prob, unpair_latent, unpair_latent_len, pair_post_prob, _ = self.model.speech_to_text(
            paired_mel=aug_mel, unpaired_mel=unpair_aug_mel, **({'_masks': _asr_masks} if _asr_masks is not None else {}))
        ignore_speech_cycle = unpair_latent is None                                               # :163-172
        if unpair_aug_mel is not None:
            self._step_info.update(unpair_text_len=0 if ignore_speech_cycle else int(unpair_latent.shape[1]))
        out = self._tts(text, sid, None if ignore_speech_cycle else unpair_sid, unpair_latent, None,
                                        unpair_latent_len, mel, None if ignore_speech_cycle else unpair_mel, tf_rate, _masks=_masks)
        pm, pl, _, _, upm, upl, _, _ = out
        # :232: the unpaired term only counts after the warm-up steps (weight 0 before: computed and logged, as in the reference)
        w = float(hp.get('unpair_speech_weight', 10.0)) if self.step > int(hp.get('unpair_speech_start_step', 0)) else 0.0
        side = self._side_branch([(self.tts_weight, lambda: self.freq_loss(pl, linear), 'tts_loss')] +
                                 ([] if ignore_speech_cycle else [(w, lambda: self.freq_loss(upl, unpair_linear), 'unpair_speech_loss')]))
        lin = side[1] if side is not None else [None, None]
        stats, terms = {}, []
        self._paired_losses(pair_prob, pair_post_prob, pm, pl, mel, linear, text, terms, stats, linear_loss=lin[0], aug_mel=aug_mel)
        if not ignore_speech_cycle:                                                               # :227-233
            terms += [(w, self.freq_loss(upm, unpair_mel), 'unpair_speech_loss'),
                      (w, lin[1] if side is not None else self.freq_loss(upl, unpair_linear), 'unpair_speech_loss')]
        return self._finish_step(terms, stats, tf_rate, 'speech_first', side)

    def text_first_step(self, mel, aug_mel, linear, text, sid, unpair_text=None, unpair_sid=None, _masks=None, _asr_masks=None):
        """The text -> speech -> text cycle of VqvaeTrainer.exec (bin/train_vqvae.py:186-205,208-224,234-250): text_to_speech on the
        paired text (teacher forced) and, when given, the unpaired text (rows without a teacher feed their own output back); the
        unpaired prediction is DETACHED and goes through speech_to_text next to the paired mel with `using_fake_mel` (the codebook
        table is detached for the fake part); losses: the paired terms, plus CTC of the unpaired posteriors against the unpaired text
        (every frame counts; with paras.actual_len the frames the text predicts, :237-240).  A NaN / inf unpaired term is counted and dropped, as the reference does."""
        hp = self.hp
        tf_rate = self._begin_step()
        use_unpair_text = unpair_text is not None                                                 # the caller gates it (:128,:149-152)
        asr = None
        if not use_unpair_text:
            # Without unpaired text the two halves of this cycle do not feed each other: the speech encoder goes FIRST (the reference runs it
            # second, :203-205), so that everything behind text_to_speech is backward work the postnet branch can run beside (_side_branch)
            asr = self.model.speech_to_text(paired_mel=aug_mel, unpaired_mel=None, using_fake_mel=False,
                                            **({'_masks': _asr_masks} if _asr_masks is not None else {}))
        out = self._tts(text, sid, unpair_sid if use_unpair_text else None, None, unpair_text, None, mel, None,
                                        tf_rate, _masks=_masks)                                   # :190-199
        pm, pl, _, _, upm, _, _, _ = out
        side = self._side_branch([(self.tts_weight, lambda: self.freq_loss(pl, linear), 'tts_loss')])
        if use_unpair_text:
            upm = upm.detach()                                                                    # :201-202
            asr = self.model.speech_to_text(paired_mel=aug_mel, unpaired_mel=upm, using_fake_mel=True,
                                            **({'_masks': _asr_masks} if _asr_masks is not None else {}))   # :203-205
        pair_prob, _, unpair_prob, _, _, pair_post_prob, _ = asr
        stats, terms = {}, []
        self._paired_losses(pair_prob, pair_post_prob, pm, pl, mel, linear, text, terms, stats, linear_loss=side[1][0] if side is not None else None,
                            aug_mel=aug_mel)
        if use_unpair_text:                                                                       # :234-250
            if getattr(self.paras, 'actual_len', False):                                          # :237-240, on the device
                from . import autograd as AG
                ut = AG.ctc_loss(unpair_prob, unpair_text, EPS, in_len=ops.frame_lengths(
                    text=unpair_text.contiguous(), r=int(self.model.n_frames_per_step), div=int(self.model.time_reduce_factor)))
            else:
                ut = self.ctc_loss(unpair_prob, unpair_text)
            stats['unpair_text_loss'] = ut.detach()
            # :246-248: a non-finite unpaired term is dropped (and counted).  That decides what backward() sees, so it is the one scalar
            # this cycle reads inside the step (only configurations with unpair_text_weight > 0 get here; none of the shipped ones)
            v = float(ut.detach())
            if math.isfinite(v):
                terms.append((float(hp.get('unpair_text_weight', 0.0)), ut, None))
        return self._finish_step(terms, stats, tf_rate, 'text_first', side)

    def cycle_step(self, pair, unpair=None, _masks=None, _asr_masks=None):
        """One iteration of VqvaeTrainer.exec's loop body (bin/train_vqvae.py:124-150): even steps run the speech-first cycle, odd
        steps the text-first cycle; the unpaired batch joins only when its weight is positive and the step is past its start step.
        `pair` = (mel, aug_mel, linear, text, sid); `unpair` = the same five for the unpaired batch, or None."""
        mel, aug_mel, linear, text, sid = pair
        kw = dict(_masks=_masks, **({'_asr_masks': _asr_masks} if _asr_masks is not None else {}))
        kind, use_unpair = self.cycle_kind(self.step)
        if kind == 'speech_first':                                                                # :137
            if use_unpair and unpair is not None:
                umel, uaug, ulin, _, usid = unpair
                return self.speech_first_step(mel, aug_mel, linear, text, sid, unpair_mel=umel, unpair_aug_mel=uaug,
                                              unpair_linear=ulin, unpair_sid=usid, **kw)
            return self.speech_first_step(mel, aug_mel, linear, text, sid, **kw)
        if use_unpair and unpair is not None:
            _, _, _, utext, usid = unpair
            return self.text_first_step(mel, aug_mel, linear, text, sid, unpair_text=utext, unpair_sid=usid, **kw)
        return self.text_first_step(mel, aug_mel, linear, text, sid, **kw)

    def cycle_kind(self, step):
        """(which cycle step `step` runs, whether it takes an unpaired batch)        ref: bin/train_vqvae.py:128-129,137-150"""
        hp = self.hp
        if step % 2 == 0:
            return 'speech_first', float(hp.get('unpair_speech_weight', 10.0)) > 0 and step > int(hp.get('unpair_speech_start_step', 0))
        return 'text_first', float(hp.get('unpair_text_weight', 0.0)) > 0 and step > int(hp.get('unpair_text_start_step', 0))

    def _stats_read(self, st):
        self._count_ctc_nan(st)

    # -- the solver protocol of main.py:65-68 on synthetic batches
    def load_data(self):
        """Synthetic counterparts of the reference's pair_set / unpair_set loaders (bin/train_vqvae.py:55-69; src/data.py is
        outside the path): `n_batches` seeded batches each, a different seed per rank (utterance-level data parallelism), mel / linear
        zero-padded to a multiple of r and aug_mel unpadded exactly as fetch_data delivers them (:33-53).  The unpaired set has its
        own batch size and length (--unpair-batch-size / --unpair-frames; default: the paired ones).
        --corpus: the three sets are the paired / unpaired / dev splits of data.corpus instead (semi_tts_amd/corpus.py: device-resident
        waveforms, features extracted on every fetch, real text and speaker ids for the unpaired split too); nothing synthetic is drawn."""
        from .synthetic import synthetic_cycle_batch
        pa = self.paras
        B = int(getattr(pa, 'batch_size', None) or self.config['data']['corpus'].get('batch_size', 8))
        Bu = int(getattr(pa, 'unpair_batch_size', None) or B)
        if getattr(pa, 'corpus', False):
            # --corpus: pair_set / unpair_set / dev_set are the splits of data.corpus, resident on the device; --dev-batches K walks the
            # first K batches of the dev split, -1 all of it, 0 none (the split is then not loaded)
            k = int(getattr(pa, 'dev_batches', 0) or 0)
            sets = self._load_corpus(['paired', 'unpaired'] + (['dev'] if k != 0 else []), {'paired': B, 'unpaired': Bu, 'dev': B})
            self.pair_set, self.unpair_set = sets['paired'], sets['unpaired']
            self.unpair_waves = None
            n_dev = sets['dev'].n_batches() if k != 0 else 0
            self.dev_set = [None] * (n_dev if k < 0 else min(k, n_dev))      # (validate walks len(dev_set) batches from the start)
            self.dev_iter = self.pair_iter = self.unpair_iter = 0
            self.batches = None
            return self
        frames = int(getattr(pa, 'frames', 256))
        uframes = int(getattr(pa, 'unpair_frames', None) or frames)
        n = int(getattr(pa, 'n_batches', 1))
        self.r = self.config['model']['decoder']['decoder']['n_frames_per_step']
        rank = int(os.environ.get('RANK', 0))
        seed = getattr(pa, 'seed', 0)
        lo, hi = self.config['data']['audio'].get('time_stretch_range', [1.0, 1.0]) if getattr(pa, 'stretch', False) else (1.0, 1.0)
        rs = np.random.RandomState(seed + 77 + rank)
        mk = lambda b, f, sd: synthetic_cycle_batch(b, f, self.r, self.vocab_size, self.n_spkr, self.n_mels, self.linear_dim, seed=sd,
                                                    stretch=float(rs.uniform(lo, hi)))
        self.pair_set = [mk(B, frames, 1000 * rank + i + seed) for i in range(n)]
        self.unpair_set = [mk(Bu, uframes, 500000 + 1000 * rank + i + seed) for i in range(n)]
        self.unpair_waves = None
        if getattr(pa, 'unpair_wav_dir', None):
            self._load_unpair_waves(pa.unpair_wav_dir, Bu, uframes, rank, seed, mk)
        # --dev-batches K: the dev set validate() walks, drawn like the paired set (same batch size and frames, unstretched) from seeds of
        # its own, per rank.  Without it (K = 0, the default) nothing is drawn and the run is what it was before validation existed.
        k = int(getattr(pa, 'dev_batches', 0) or 0)
        self.dev_set = [synthetic_cycle_batch(B, frames, self.r, self.vocab_size, self.n_spkr, self.n_mels, self.linear_dim,
                                              seed=900000 + 1000 * rank + i + seed, stretch=1.0) for i in range(k)]
        self.dev_iter = 0
        self.pair_iter, self.unpair_iter = 0, 0
        # (mel, aug_mel, linear, text, sid) -> the paired TTS step's (text, sid, mel, linear): TtsTrainer.exec on the same data
        self.batches = [(b[3], b[4], b[0], b[2]) for b in self.pair_set]
        return self

    def _load_unpair_waves(self, wav_dir, Bu, uframes, rank, seed, mk):
        """--unpair-wav-dir: the unpaired set's (mel, aug_mel, linear) come from the .wav files of wav_dir, sorted by name, rank k of
        a world of w taking files k::w, in batches of Bu.  The waveforms are read once and stay on the device; fetch_data extracts
        the features again on every fetch (fresh SNR / stretch draws, as the reference's loader does every epoch).  text / sid stay
        synthetic: the speech-first cycle does not read the unpaired text."""
        from .audio import load_audio_transform
        world = int(os.environ.get('WORLD_SIZE', 1))
        files = sorted(f for f in os.listdir(wav_dir) if f.lower().endswith('.wav'))[rank::world]
        if not files:
            raise ValueError('--unpair-wav-dir %s: no .wav files for rank %d of %d' % (wav_dir, rank, world))
        self.audio_converter = load_audio_transform(**self.config['data']['audio'])
        if self.audio_converter.n_mels != self.n_mels:
            raise ValueError('--unpair-wav-dir: data.audio has %d mels, the model %d' % (self.audio_converter.n_mels, self.n_mels))
        paths = [os.path.join(wav_dir, f) for f in files]
        self.unpair_waves = [self.audio_converter.load_batch(paths[i:i + Bu], resample=bool(getattr(self.paras, 'resample', False)),
                                                             trim=trim_args(self.paras), loudness=loudness_args(self.paras))
                             for i in range(0, len(paths), Bu)]
        self.unpair_set = [mk(len(wb.lens), uframes, 500000 + 1000 * rank + i + seed) for i, wb in enumerate(self.unpair_waves)]

    def fetch_data(self, iter_name):
        """the next batch of `pair_iter` / `unpair_iter` on the device, the set restarting when it is exhausted (:33-41)"""
        data = getattr(self, iter_name.replace('iter', 'set'))
        i = getattr(self, iter_name)
        setattr(self, iter_name, i + 1)
        if getattr(self, 'corpus', None) is not None:       # --corpus: features extracted from the resident waveforms on every fetch
            return self.corpus_sets[{'pair_iter': 'paired', 'unpair_iter': 'unpaired', 'dev_iter': 'dev'}[iter_name]].fetch()
        if iter_name == 'unpair_iter' and self.unpair_waves is not None:
            j = i % len(self.unpair_waves)
            mel, aug_mel, linear = self.audio_converter.extract_batch(self.unpair_waves[j], r=self.r)
            text, sid = self.unpair_set[j][3].to(self.device), self.unpair_set[j][4].to(self.device)
            return mel, aug_mel, linear, text, sid
        cache = self.__dict__.setdefault('_dev_batches', {})
        key = (iter_name, i % len(data))
        if key not in cache:                     # (the synthetic sets are small and fixed: on the device once)
            cache[key] = tuple(t.to(self.device) for t in data[i % len(data)])
        return cache[key]

    def validate(self):
        """VqvaeTrainer.validate (bin/train_vqvae.py:330-428) without the tensorboard writes: in eval mode and without gradients, per dev
        batch the phone error rate of speech_to_text on the clean mel (and of the ASR postnet, when the model has one) and the freq_loss
        of free-running synthesis; each is the mean over the dev batches of the batch value.  Everything stays on the device until ONE
        host read after the cross-rank sum; the checkpoint rules are validation_checkpoints (rank 0 writes).  Parameters, gradients,
        optimiser state and BatchNorm statistics are left as they were; the dropout masks and teacher-forcing draws it makes (as the
        reference's do) move the torch / numpy generators, so a run with validation takes other draws afterwards than one without.
        -> (dev_tts_loss, dev_per, dev_post_per or None)"""
        from . import parallel
        from .metrics import per_sum
        # what the last training step left queued: its deferred weight-gradient products and the postnet branch's second stream
        ops.flush_wgrads()
        ev = self.__dict__.get('_side_event')
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
        ops.side_pending(None)
        self.model.eval()
        tts, per, post = [], [], []
        if getattr(self, 'corpus', None) is not None and self.dev_set:
            self.corpus_sets['dev'].rewind()                 # the dev split is walked from its first batch every time
        try:
            with torch.no_grad():
                for _ in range(len(self.dev_set)):
                    mel, _, linear, text, sid = self.fetch_data('dev_iter')
                    B = text.shape[0]
                    pair_prob, _, _, _, _, pair_post_prob, _ = self.model.speech_to_text(paired_mel=mel, unpaired_mel=None)     # :342-343
                    per.append(per_sum(pair_prob, text) / B)
                    if pair_post_prob is not None:
                        post.append(per_sum(pair_post_prob, text) / B)
                    mel_pred, lin_pred, _, _, _, _, _, _ = self.model.text_to_speech(text, sid, None, None, None, None, mel.shape[1], None,
                                                                                   tf_rate=0.0)      # :350-358
                    tts.append((self.freq_loss(mel_pred, mel) + self.freq_loss(lin_pred, linear)).to(torch.float64))
                zero = torch.zeros((), dtype=torch.float64, device=self.device)
                acc = torch.stack([sum(tts, zero), sum(per, zero), sum(post, zero),
                                   zero + len(tts), zero + len(post)])
                if parallel.dist_on():
                    parallel.all_reduce_sum_(acc)
                s_tts, s_per, s_post, n, n_post = acc.tolist()                                  # the one host read of the pass
        finally:
            self.model.train()
        dev_tts, dev_per = s_tts / n, s_per / n
        dev_post = s_post / n_post if n_post > 0 else None
        best = (getattr(self, 'best_tts_loss', BEST_TTS_LOSS_INIT), getattr(self, 'best_per', BEST_PER_INIT))
        files, (self.best_tts_loss, self.best_per) = validation_checkpoints(self.step, dev_tts, dev_per, dev_post, best,
                                                                            bool(getattr(self.paras, 'store_best_per', False)))
        rank, _ = parallel.rank_world()
        if rank == 0:
            for name, score in files:
                self.save_checkpoint(name, score)
            self.verbose('Dv stat | step %d | TTS loss - %.6f | PER - %.6f | post PER - %s' %
                         (self.step, dev_tts, dev_per, 'None' if dev_post is None else '%.6f' % dev_post))
        self.__dict__.setdefault('dev_log', []).append(dict(step=self.step, tts_loss=dev_tts, per=dev_per, post_per=dev_post, files=[f for f, _ in files]))
        return dev_tts, dev_per, dev_post

    def exec(self):
        """VqvaeTrainer.exec's loop (bin/train_vqvae.py:111-150,270-300) without the corpus-side logging: paired batch every step,
        the unpaired batch fetched only when the step's cycle uses it, cycles alternating"""
        t0 = time.perf_counter()
        frames = 0
        cnt = {'unp_sph': 0, 'unp_txt': 0}
        self.ctc_nan = 0
        self.dev_log = []
        self.valid_step = int(getattr(self.paras, 'valid_step', None) or self.hp.get('valid_step', 1))
        if not hasattr(self, 'dev_set'):
            self.dev_set = []
        while self.step < self.max_step:
            pair = self.fetch_data('pair_iter')
            kind, use_unpair = self.cycle_kind(self.step)
            unpair = self.fetch_data('unpair_iter') if use_unpair else None                       # :139-150
            st = self.cycle_step(pair, unpair)
            frames += pair[0].shape[0] * pair[0].shape[1] + (unpair[0].shape[0] * unpair[0].shape[1] if unpair is not None else 0)
            if unpair is not None:
                cnt['unp_sph' if kind == 'speech_first' else 'unp_txt'] += 1
            self.log.append(st)
            if self.step == 1 or self.step % 10 == 0:
                self.verbose('Tr stat | step %d (%s) | Loss - %.4f (CTC-nan/unp-sph/unp-txt=%d/%d/%d) | Grad. Norm - %.3f | lr %.2e' %
                             (self.step, kind, st['loss'], self.ctc_nan, cnt['unp_sph'], cnt['unp_txt'], st['grad_norm'], st['lr']))
            if self.dev_set and (self.step == 1 or self.step % self.valid_step == 0):                 # :313-314
                self.validate()
        torch.cuda.synchronize()
        self.drain_stats()
        self.check_device_status()
        dt = time.perf_counter() - t0
        if self.log and not (self.step == 1 or self.step % 10 == 0):          # the last step's statistics, when not logged above
            st = self.log[-1]
            self.verbose('Tr stat | step %d (%s) | Loss - %.4f (CTC-nan/unp-sph/unp-txt=%d/%d/%d) | Grad. Norm - %.3f | lr %.2e' %
                         (self.step, kind, st['loss'], self.ctc_nan, cnt['unp_sph'], cnt['unp_txt'], st['grad_norm'], st['lr']))
        if getattr(self.paras, 'save', False):
            self.save_checkpoint('latest.pth', self.log[-1]['loss'] if self.log else 0.0)
        self.verbose('%d steps, %d frames in %.2f s (%.0f frames/s incl. first-step set-up)' %
                     (len(self.log), frames, dt, frames / max(dt, 1e-9)))
        return self.log


# the tools that build no model live in dirtools.py; they stay reachable as solver.X (main.py, the tests and the tools look them up here)
from .dirtools import (  # noqa: E402,F401
    DirTool, Vocoder, Resampler, LoudnessWriter, Trimmer, FeatureWriter, McdScorer, StoiScorer, AbxScorer, PhnScorer, FeatureTool, KMeansTrainer,
    UnitWriter, load_codebook, merge_repeats, format_units, UNIT_FEATS, UNIT_ID_OFFSET, KMEANS_HEADER, KMEANS_UNITS_HEADER,
    list_wavs, wav_header, check_wav, check_out_dir, load_waves, mfcc_frames, extract_features,
    list_vocode_files, trim_args, loudness_args, vocode, f0_args, mcd_key, mcd_pairs, phn_pairs, per_row, format_confusions, format_phones,
    format_ops, stoi_row, abx_metric,
    VOCODE_SUFFIX, MCD_PRED_SUFFIX, MCD_MAX_BATCH, MCD_HEADER, F0_HEADER, F0_FIGURES, STOI_HEADER, STOI_MAX_LEN_DIFF, STOI_MAX_DELAY, DELAY_HEADER,
    SDR_HEADER, ABX_FEATS, SCORE_MAX_BATCH, SCORE_DEFAULT_IGNORE, PER_HEADER, PER_NBEST_HEADER, CONFUSIONS_HEADER, PHONES_HEADER)
