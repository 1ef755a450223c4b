"""VQVAE orchestration on the HIP path: the caller of the hot path (H1/H2 rows of SURVEY.md 8a).

Mirrors the reference's src/vqvae.py: constructor arguments and config splatting (:26-68),
`speech_to_text` (:106-141: CTC speech encoder -> codebook -> run-length merge of the unpaired part),
`text_to_speech` with its paired / unpaired batch concatenation and output slicing (:143-207),
`mean_forward` (:218-257), `padded_concat` (:259-271).
State-dict prefixes are the reference's (`asr.*`, `codebook.*`, `spkr_embed.weight`, `tts.*`).
"""
import math
import numbers

import torch
import torch.nn as nn

from . import ops
from . import autograd as AG
from .asr import CTC, ASRPostnet
from .embed import L2Embedding, SeperateEmbedding
from .tts import Tacotron2

FRAME_PHN_RATIO = 6.0          # ref: src/vqvae.py:18
SYNTH_MAX_FRAMES_PER_PHONE = 2.0 * FRAME_PHN_RATIO     # synthesise: the decode budget per phone, twice the corpus average
INFERENCE_MARGIN_FRAMES = 40   # ref: bin/gen_specgram.py:17
PRETRAINED_ENCODER_PREFIX = 'encoder.'      # ref: src/vqvae.py:13-15
PRETRAINED_DECODER_PREFIX = 'decoder.'
PRETRAINED_POSTNET_PREFIX = 'postnet.'


def check_transcript(ids, vocab_size):
    """a transcript synthesise takes: at least one id, every id in [1, vocab_size) (index 0 is the token appended after the last phone
    and the batch padding: inside a transcript it would end it early).  ValueError saying what is wrong otherwise."""
    ids = list(ids)
    if not ids:
        raise ValueError('empty transcript')
    for k, i in enumerate(ids):
        if isinstance(i, bool) or int(i) != i:
            raise ValueError('token %d is %r, not an id' % (k, i))
        if i == 0:
            raise ValueError('token %d is id 0, the end / padding index' % k)
        if not 0 < i < vocab_size:
            raise ValueError('token %d is id %d, outside the vocabulary of %d' % (k, i, vocab_size))
    return [int(i) for i in ids]


def synth_frames(n_max, r, max_frames_per_phone=SYNTH_MAX_FRAMES_PER_PHONE):
    """frames synthesise decodes for a batch whose longest transcript has n_max phones: n_max * max_frames_per_phone plus the
    reference's margin, rounded up to whole decoder steps of r frames"""
    if not (n_max >= 1 and r >= 1 and 0.0 < max_frames_per_phone < float('inf')):
        raise ValueError('synth_frames: n_max=%r, r=%r, max_frames_per_phone=%r: need n_max, r >= 1 and a finite positive budget'
                         % (n_max, r, max_frames_per_phone))
    return int(r) * int(math.ceil((n_max * max_frames_per_phone + INFERENCE_MARGIN_FRAMES) / r))


class VQVAE(nn.Module):
    def __init__(self, n_mels, linear_dim, vocab_size, n_spkr, encoder, codebook, decoder, spkr_latent_dim,
                 max_frames_per_phn, stop_threshold, asr_postnet_weight=0.0, txt_update_codebook=False,
                 pretrained_asr=None, pretrained_emb=None, pretrained_tts=None):
        super().__init__()
        self.in_dim = n_mels
        self.vocab_size = vocab_size
        self.n_spkr = n_spkr
        self.n_mels = n_mels
        self.linear_dim = linear_dim
        self.spkr_latent_dim = spkr_latent_dim
        self.stop_threshold = stop_threshold
        self.max_frames_per_phn = max_frames_per_phn
        self.txt_update_codebook = txt_update_codebook
        codebook = dict(codebook)
        self.code_bone = codebook.pop('bone')                          # :41
        self.latent_dim = codebook['latent_dim']
        self.n_frames_per_step = decoder['decoder']['n_frames_per_step']
        self.asr = CTC(n_mels, self.latent_dim, **encoder)                                    # :46
        self.time_reduce_factor = self.asr.time_reduce_factor
        self.use_asr_postnet = asr_postnet_weight > 0
        if self.use_asr_postnet:                                       # :50-52 (the reference passes latent_dim as the class count)
            self.asr_postnet_weight = asr_postnet_weight
            self.asr_postnet = ASRPostnet(self.latent_dim, self.latent_dim)
        if self.code_bone == 'l2':                                     # :56-61
            self.codebook = L2Embedding(vocab_size, False, **codebook)
        elif self.code_bone == 'seperate':
            self.codebook = SeperateEmbedding(vocab_size, False, **codebook)
        else:
            raise NotImplementedError
        self.spkr_embed = nn.Embedding(self.n_spkr, spkr_latent_dim)   # :64
        self.tts = Tacotron2(n_mels, self.linear_dim, self.codebook.out_dim, self.spkr_latent_dim, decoder)   # :68
        self._load_pretrained(pretrained_asr, pretrained_emb, pretrained_tts)

    def _load_pretrained(self, pretrained_asr, pretrained_emb, pretrained_tts):
        """Partial initialisation from earlier checkpoints with the reference's key rewriting (src/vqvae.py:70-90; advertised by
        config/*.yaml:94-97).  Every occurrence of the prefix is removed from every key (str.replace, as the reference does), the
        load is non-strict and must leave no key of the target module missing."""
        from collections import OrderedDict

        def ckpt(path):
            return torch.load(path, map_location='cpu')['model']

        def load_into(module, state, what):
            missing, _ = module.load_state_dict(state, strict=False)
            assert missing == [], 'Missing pretrained para. {} ({})'.format(missing, what)

        self.pretrain_asr = pretrained_asr is not None and pretrained_asr != ''
        if self.pretrain_asr:                                          # :71-76
            old = OrderedDict((k.replace(PRETRAINED_ENCODER_PREFIX, ''), v) for k, v in ckpt(pretrained_asr).items())
            load_into(self.asr, old, 'pretrained_asr')
        self.pretrained_emb = pretrained_emb is not None and pretrained_emb != ''
        if self.pretrained_emb:                                        # :77-80 (the reference reads the ASR checkpoint's path here)
            self.codebook.load_pretrained_embedding(ckpt(pretrained_asr))
        self.pretrained_tts = pretrained_tts is not None and pretrained_tts != ''
        if self.pretrained_tts:                                        # :81-90
            old = OrderedDict((k.replace(PRETRAINED_DECODER_PREFIX, ''), v) for k, v in ckpt(pretrained_tts).items())
            load_into(self.tts.decoder, old, 'pretrained_tts decoder')
            post = OrderedDict((k.replace(PRETRAINED_POSTNET_PREFIX, ''), v) for k, v in old.items() if PRETRAINED_POSTNET_PREFIX in k)
            load_into(self.tts.postnet, post, 'pretrained_tts postnet')

    def padded_concat(self, pair, unpair):
        """zero-pad the shorter of two (B, T, D) batches in time and stack them on the batch axis.  ref: :259-271"""
        return pair.shape[0], AG.padded_concat(pair, unpair)

    def embed_speakers(self, sid):
        if self.training and torch.is_grad_enabled():
            return AG.gather(self.spkr_embed.weight, sid)
        return ops.gather_rows(self.spkr_embed.weight, sid)

    def quantize(self, enc_latent, first_n_real_mel=0):
        """codebook lookup of speech-encoder latents: (p_code, quantized_latent)   ref: :119"""
        p_code, quantized, _, _ = self.codebook(enc_latent, first_n_real_mel)
        return p_code, quantized

    def mean_forward(self, p_code, latent):
        """run-length merge + blank filter of the quantised latents on device.      ref: :218-257"""
        return AG.mean_forward(p_code, latent, self.max_frames_per_phn)

    def speech_to_text(self, paired_mel, unpaired_mel, using_fake_mel=False, _masks=None):
        """same contract and return tuple as the reference (:106-141); `_masks` (tests only) = explicit dropout masks of the encoder"""
        use_unpaired = unpaired_mel is not None
        if use_unpaired:
            paired_mel_bs, all_mel = self.padded_concat(paired_mel, unpaired_mel)
        else:
            all_mel, paired_mel_bs = paired_mel, len(paired_mel)
        enc_latent = self.asr(all_mel, _masks) if _masks is not None else self.asr(all_mel)    # :116
        paired_post_prob = self.asr_postnet(enc_latent[:paired_mel_bs]) if self.use_asr_postnet else None   # :117
        first_n_real_mel = len(paired_mel) if using_fake_mel else 0
        p_code, quantized_latent, _, rest = self.codebook(enc_latent, first_n_real_mel)         # :119
        if use_unpaired:                                                                        # :122-133
            pair_prob, pair_latent = p_code[:paired_mel_bs], quantized_latent[:paired_mel_bs]
            unpair_prob, unpair_latent = p_code[paired_mel_bs:], quantized_latent[paired_mel_bs:]
            trim_out = self.mean_forward(unpair_prob, unpair_latent)
            unpair_latent, unpair_latent_len = trim_out if trim_out is not None else (None, None)
        else:
            pair_prob, pair_latent = p_code, quantized_latent
            unpair_prob = unpair_latent = unpair_latent_len = None
        return pair_prob, pair_latent, unpair_prob, unpair_latent, unpair_latent_len, paired_post_prob, rest

    def encoder_lengths(self, mel_lengths):
        """frames of the encoder output for mel_lengths input frames: each conv layer's out_len in turn (the LSTMs keep the length)"""
        t = torch.as_tensor(mel_lengths, dtype=torch.int64)
        for l in range(self.asr.layers):
            t = getattr(self.asr, 'layer' + str(l)).out_len(t)
        return t

    def transcribe(self, mel, mel_lengths, beam_width=16, top_paths=1, source='code', lm=None, lm_weight=0.5, ins_bonus=0.0, bonus=None):
        """CTC prefix beam search of the speech encoder's posteriors, in eval mode without gradients (the mode is restored after).
        mel (B, T, n_mels) padded batch on the device, mel_lengths its valid frames per utterance (host integers).  source 'code':
        the codebook posteriors of speech_to_text (probabilities, searched as log(p + 1e-10)); 'post': the ASRPostnet's log-posteriors
        (refused when the model has no postnet).  The encoder runs on the padded batch, as the reference's validate does, so its
        BiLSTM sees the padding frames; the search reads only each utterance's own encoder frames (encoder_lengths).  lm, lm_weight,
        ins_bonus: the n-gram fusion of ctc_decode.beam_search (None: the acoustic search); bonus: instead of lm, a fused table already
        on the device.
        -> (hyp (B, top_paths, T') int64, hyp_len (B, top_paths) int32, score (B, top_paths) float32) device tensors, best first."""
        from .ctc_decode import beam_search
        if source not in ('code', 'post'):
            raise ValueError("transcribe: source must be 'code' or 'post' (got %r)" % (source,))
        if source == 'post' and not self.use_asr_postnet:
            raise ValueError("transcribe: source 'post' needs an ASRPostnet (model.asr_postnet_weight > 0)")
        lengths = self.encoder_lengths(mel_lengths)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                p_code, _, _, _, _, post, _ = self.speech_to_text(paired_mel=mel, unpaired_mel=None)
                prob = post if source == 'post' else p_code
                return beam_search(prob, lengths.clamp(0, prob.shape[1]), beam_width, top_paths, log_input=source == 'post',
                                   lm=lm, lm_weight=lm_weight, ins_bonus=ins_bonus, bonus=bonus)
        finally:
            self.train(was_training)

    def represent(self, mel, mel_lengths, source='latent'):
        """The representations ABX scores (metrics.abx), in eval mode without gradients (the mode is restored after).  mel (B, T, n_mels)
        padded batch on the device, mel_lengths its valid frames per utterance (host integers).  source 'latent': the speech encoder's
        output, what feeds the codebook; 'code': p_code, the codebook posteriors of speech_to_text.  The encoder runs on the padded batch,
        as in transcribe; only the first encoder_lengths rows of an utterance are its own.
        -> ((B, T', D) float32 on the device, encoder_lengths (B,) int64 host tensor clamped to T')."""
        if source not in ('latent', 'code'):
            raise ValueError("represent: source must be 'latent' or 'code' (got %r)" % (source,))
        lengths = self.encoder_lengths(mel_lengths)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                if source == 'latent':
                    out = self.asr(mel)
                else:
                    out = self.speech_to_text(paired_mel=mel, unpaired_mel=None)[0]
                return out.float().contiguous(), lengths.clamp(0, out.shape[1])
        finally:
            self.train(was_training)

    def align(self, mel, mel_lengths, text, text_lengths=None, source='code'):
        """CTC forced alignment of transcripts to the speech encoder's posteriors, in eval mode without gradients (the mode is restored
        after).  mel (B, T, n_mels) padded batch on the device, mel_lengths its valid frames per utterance (host integers); text (B, L)
        int64 on the device, its non-blank (non-zero) entries the targets, text_lengths as in ctc_align.forced_align.  source 'code':
        the codebook posteriors of speech_to_text (probabilities, scored as log(p + 1e-10)); 'post': the ASRPostnet's log-posteriors
        (refused when the model has no postnet).  The encoder runs on the padded batch, as in transcribe, so its BiLSTM sees the
        padding frames; the aligner reads only each utterance's own encoder frames (encoder_lengths).
        -> (score (B,) float32, path (B, T') int32, tok_start (B, L) int32, tok_end (B, L) int32) device tensors, in encoder frames."""
        from .ctc_align import forced_align
        if source not in ('code', 'post'):
            raise ValueError("align: source must be 'code' or 'post' (got %r)" % (source,))
        if source == 'post' and not self.use_asr_postnet:
            raise ValueError("align: source 'post' needs an ASRPostnet (model.asr_postnet_weight > 0)")
        lengths = self.encoder_lengths(mel_lengths)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                p_code, _, _, _, _, post, _ = self.speech_to_text(paired_mel=mel, unpaired_mel=None)
                prob = post if source == 'post' else p_code
                return forced_align(prob, text, lengths.clamp(0, prob.shape[1]), text_lengths, log_input=source == 'post')
        finally:
            self.train(was_training)

    def synthesise(self, transcripts, sid, max_frames_per_phone=SYNTH_MAX_FRAMES_PER_PHONE):
        """Free-running synthesis of phone transcripts, in eval mode without gradients (the mode is restored after).  transcripts: a
        list of id lists (check_transcript: non-empty, ids in [1, vocab_size)); sid: one speaker id for all, or one per transcript.
        Each transcript becomes ids + [0] -- the index 0 PhoneTextEncoder appends (src/text.py:65) -- and the batch is padded with 0 to
        its longest, as training batches are.  The decoder runs synth_frames(n_max, r, max_frames_per_phone) frames at tf_rate 0
        through text_to_speech unchanged; where each utterance ends is for metrics.attention_endpoints to say.
        Padded phones are seen by the encoder and the attention, unmasked: this follows the reference and every batch the model was
        trained on, so an utterance's output depends on its batch's longest transcript.  A batch of one gives the alone result.
        -> (mel (B, T, n_mels), linear (B, T, linear_dim), align (B, T / r, n_max + 1), enc_len (B,) int32: the real phones of each
        utterance), device tensors."""
        rows = [check_transcript(t, self.vocab_size) for t in transcripts]
        if not rows:
            raise ValueError('synthesise: no transcripts')
        B, dev = len(rows), self.spkr_embed.weight.device
        sids = [int(sid)] * B if isinstance(sid, numbers.Integral) else [int(s) for s in (sid.reshape(-1).tolist() if torch.is_tensor(sid) else sid)]
        if len(sids) != B or any(not 0 <= s < self.n_spkr for s in sids):
            raise ValueError('synthesise: sid %r: one id, or one per transcript, in [0, %d)' % (sid, self.n_spkr))
        n_max = max(len(t) for t in rows)
        frames = synth_frames(n_max, self.n_frames_per_step, float(max_frames_per_phone))
        text = torch.zeros(B, n_max + 1, dtype=torch.int64)
        for b, t in enumerate(rows):
            text[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
        enc_len = torch.tensor([len(t) for t in rows], dtype=torch.int32)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                mel, linear, align, _, _, _, _, _ = self.text_to_speech(
                    text.to(dev), torch.tensor(sids, dtype=torch.int64).to(dev), None, None, None, None, frames, None, tf_rate=0.0)
        finally:
            self.train(was_training)
        return mel, linear, align, enc_len.to(dev)

    def text_to_speech(self, paired_text, paired_sid, unpaired_sid, unpaired_latent, unpaired_text, unpaired_latent_len,
                       paired_teacher, unpaired_teacher, tf_rate, _masks=None):
        """same contract and return tuple as the reference (:143-207); `_masks` (tests only) = explicit dropout masks"""
        paired_latent = self.codebook.inference(paired_text)                                   # :147
        unpair_max_frame = None
        if unpaired_text is not None:                       # text-to-text cycle              :150-163
            assert unpaired_latent is None
            use_unpaired = True
            unpaired_latent = self.codebook.inference(unpaired_text)
            paired_latent_bs, all_latent = self.padded_concat(paired_latent, unpaired_latent)
            paired_ts = paired_teacher.shape[1]
            unpaired_ts = int(FRAME_PHN_RATIO * unpaired_text.shape[1])
            unpaired_ts += unpaired_ts % self.n_frames_per_step
            unpair_max_frame = unpaired_ts
            all_teacher = paired_teacher
            all_spkr = self.embed_speakers(torch.cat([paired_sid, unpaired_sid]))
        elif unpaired_latent is not None:                   # speech-to-speech cycle          :164-173
            use_unpaired = True
            paired_latent_bs, all_latent = self.padded_concat(paired_latent, unpaired_latent)
            paired_ts, unpaired_ts = paired_teacher.shape[1], unpaired_teacher.shape[1]
            _, all_teacher = self.padded_concat(paired_teacher, unpaired_teacher)
            all_spkr = self.embed_speakers(torch.cat([paired_sid, unpaired_sid]))       # (one lookup of both id lists = the cat of two lookups)
        else:                                                                                   # :174-180
            use_unpaired = False
            all_latent, all_teacher = paired_latent, paired_teacher
            all_spkr = self.embed_speakers(paired_sid)
        mel, linear, align, stop = self.tts(all_latent, None, all_teacher, all_spkr, tf_rate=tf_rate,
                                            unpair_max_frame=unpair_max_frame, _masks=_masks)   # :183-184
        if use_unpaired:                                                                        # :187-195
            b = paired_latent_bs
            if mel.requires_grad or linear.requires_grad:
                # (the same slices; their backward writes both gradients into one tensor instead of zero-fill + copy + add per slice)
                pm, um = AG.split_pair(mel, b, paired_ts, unpaired_ts)
                side = getattr(self.tts, 'postnet_stream', None)
                if side is not None:                 # (the postnet ran on the second stream: the backward of its split belongs there too)
                    with torch.cuda.stream(side):
                        pl, ul = AG.split_pair(linear, b, paired_ts, unpaired_ts)
                else:
                    pl, ul = AG.split_pair(linear, b, paired_ts, unpaired_ts)
            else:
                pm, um, pl, ul = mel[:b, :paired_ts], mel[b:, :unpaired_ts], linear[:b, :paired_ts], linear[b:, :unpaired_ts]
            return (pm, pl, align[:b, :paired_ts], stop[:b], um, ul, align[b:, :unpaired_ts], stop[b:])
        return mel, linear, align, stop, None, None, None, None
