#!/usr/bin/env python
"""Entry point with the reference's flags (ref: main.py:14-68): YAML config + Solver dispatch.
The dispatch is the reference's (main.py:49-63): `--gen-specgram` runs batched free-running synthesis
(bin/gen_specgram.py), the default mode runs `VqvaeTrainer` -- the alternating speech -> text -> speech /
text -> speech -> text cycles of bin/train_vqvae.py:111-270 (CTC speech encoder, codebook, run-length merge,
TTS branch, CTC + freq losses, backward, clip + Adam, all on the HIP kernels) -- on synthetic paired and
unpaired batches, or with `--corpus` on the files `data.corpus` names.  `--tts-only` keeps the paired TTS step alone (TtsTrainer).
`--dev-batches K` adds the reference's validation (bin/train_vqvae.py:313-314,330-428) on K synthetic dev batches: at step 1
and every `--valid-step` (hparas.valid_step) steps it logs `Dv stat` (dev TTS loss, PER, post PER) and writes tts_<step>.pth /
asr_<step>.pth / best_post_per.pth / step_<step>.pth -- or, with --store-best-per, best_per.pth / best_post_per.pth -- under
--ckpdir/<name>.  Without it nothing is validated and no checkpoint is written (only --save's latest.pth).

    python main.py --config config/semi-single-spkr-paired-data.yaml --max-step 20 [--frames 256 --batch-size 8]
    python main.py --config config/semi-single-spkr-paired-data.yaml --max-step 20000 --dev-batches 4 [--valid-step 5000] [--store-best-per]
    python main.py --config config/semi-single-spkr-paired-data.yaml --corpus --max-step 20000 --dev-batches -1 [--actual-len --max-frames 800]
    python main.py --config config/supervised.yaml --tts-only --corpus --max-step 20000 [--corpus-max-gb 8 --resample]
    python main.py --config config/supervised.yaml --gen-specgram [--load ckpt.pth] [--frames 256 --batch-size 32]
    python main.py --config config/supervised.yaml --tts-only --max-step 20 [--frames 256 --batch-size 32]
    python main.py --config config/semi-single-spkr-paired-data.yaml --transcribe-wav-dir DIR [--beam-width 16 --top-paths 1 --vocab FILE]
    python main.py --config config/semi-single-spkr-paired-data.yaml --align-wav-dir DIR [--phn-dir DIR2 --vocab FILE]
    python main.py --config config/semi-single-spkr-paired-data.yaml --build-lm-phn-dir DIR --lm-order 2 --lm FILE [--lm-smooth 1 --lm-classes 43 --vocab F]
    python main.py --config config/semi-single-spkr-paired-data.yaml --transcribe-wav-dir DIR --lm FILE [--lm-weight 0.5 --ins-bonus 0]
    python main.py --config config/supervised.yaml --vocode-dir DIR [--vocode-feat spec|mel --batch-size 32]
    python main.py --config config/semi-single-spkr-paired-data.yaml --transcribe-wav-dir DIR --resample      (files of any sample rate)
    python main.py --resample-wav-dir DIR --resample-out DIR2 --resample-rate 16000 [--batch-size 32]
    python main.py --config config/supervised.yaml --feat-wav-dir DIR --feat mfcc|mel|linear [--segment-file FILE --min-segment-len 2]
    python main.py --config config/supervised.yaml --feat-wav-dir DIR --feat f0 [--f0-min 60 --f0-max 500 --f0-threshold 0.15]
    python main.py --config config/supervised.yaml --mcd-wav-dir SYN --mcd-ref-dir REF [--mcd-path --mcd-f0 --batch-size 32]
    python main.py --config config/supervised.yaml --synth-phn-dir DIR [--load ckpt.pth --vocab FILE --synth-sid 0 --gen-wav --batch-size 8]
    python main.py --config config/supervised.yaml --trim-wav-dir DIR --trim-out DIR2 [--trim-top-db 60 --trim-frame-length 2048 --trim-hop 512]
    python main.py --config config/semi-multi-spkr-paired-data.yaml --corpus --trim-silence [--trim-pad-ms 0]
    python main.py --score-phn-dir HYP --score-ref-dir REF [--vocab FILE --score-ignore 0,1,2 --score-nbest --score-ali --batch-size 64]
    python main.py --config config/supervised.yaml --loudness-wav-dir DIR [--loudness-out DIR2 --loudness-target -23 --loudness-peak -1 --loudness-max-gain 30]
    python main.py --config config/semi-multi-spkr-paired-data.yaml --corpus --normalize-loudness [--loudness-target -23]
    python main.py --config config/semi-single-spkr-paired-data.yaml --abx-ali-dir ALI --abx-wav-dir WAVS [--abx-feat mfcc|mel|latent|code --load ckpt.pth]
`--corpus` trains on the reference's corpus layout (semi_tts_amd/corpus.py: partition table, map table, speaker map, vocabulary file and
<path>/<speaker>/<id>.wav, src/data.py + corpus/vctk.py + src/text.py): each split of the rank's shard is read once and stays on the device as
one packed buffer, every fetch extracts mel / augmented mel / linear from it on the GPU, `--dev-batches K` (-1: all) validates on the real dev
split, vocab_size and n_spkr come from the files.  `--actual-len` gives the CTC terms the frame counts of each utterance (computed on the
device) instead of the padded length, as bin/train_vqvae.py:436-444 and :237-240.
`--transcribe-wav-dir` (not a mode of the reference) transcribes .wav files by CTC prefix beam search (solver.Transcriber); with
`--lm FILE` a phone n-gram table weights the search inside the kernel.  `--build-lm-phn-dir` counts such a table from .phn transcripts
(semi_tts_amd/ngram.py: a plain .npy of shape (V^(order-1), V) in the layout of the reference's NgramPrior, src/lm.py:233-290) on the host.
`--align-wav-dir` (not a mode of the reference either) aligns .wav files to their .phn transcripts by CTC forced alignment
(solver.Aligner): <file>.ali per utterance and segments.csv in the layout of the reference's segment_file.
`--vocode-dir` (the reference's util/gen_wav_from_specgram.py) vocodes the -spec.npy or -mel.npy files `--gen-specgram` writes into
<stem>.wav by Griffin-Lim, a batch of differing lengths per call (solver.Vocoder); `--gen-wav-feat mel` makes `--gen-specgram --gen-wav`
vocode the predicted mel instead of the predicted linear spectrogram.
`--resample` (with --unpair-wav-dir, --transcribe-wav-dir or --align-wav-dir) converts files whose rate is not data.audio.sample_rate on
the GPU (semi_tts_amd.audio.resample: Hann-windowed sinc, st_resample_batch) where the reference, and this path without the flag, refuse
them; `--resample-wav-dir` converts a directory of .wav files to another rate and writes them as 16-bit mono (solver.Resampler).
`--trim-silence` (not a step of the reference, which leaves trimming to an offline tool) cuts the leading and trailing silence of every
utterance that --corpus, --unpair-wav-dir, --transcribe-wav-dir, --mcd-wav-dir or --feat-wav-dir load, on the GPU and without a copy
(semi_tts_amd.audio.AudioConverter.trim_batch, st_trim_silence: the definition of librosa.effects.trim); `--trim-wav-dir` writes the kept
span of every .wav of a directory, bit for bit, and trim.csv (solver.Trimmer).
`--normalize-loudness` (not a step of the reference, whose features are absolute levels) brings every utterance that --corpus,
--unpair-wav-dir, --transcribe-wav-dir, --feat-wav-dir or --mcd-wav-dir (both sides) load, and every waveform that --gen-specgram --gen-wav,
--vocode-dir or --synth-phn-dir --gen-wav write, to --loudness-target LUFS of integrated loudness (ITU-R BS.1770-4 / EBU R 128, mono: K-weighting,
400 ms blocks, gates at -70 LKFS and 10 LU under the mean) on the GPU, in place, after resampling and trimming
(semi_tts_amd.audio.AudioConverter.loudness_batch, st_loudness_batch + st_wave_gain); the gain stops where the sample peak would pass
--loudness-peak dBFS or the gain --loudness-max-gain dB, and utterances with a non-finite sample, under 400 ms or under the absolute gate keep
their level.  This first version does not combine with --align-wav-dir or --segment-file.  `--loudness-wav-dir` meters every .wav of a directory
into loudness.csv and, with `--loudness-out`, writes every file normalised as 16-bit mono (solver.LoudnessWriter).
`--feat-wav-dir` writes the MFCC (13 cepstra and their two derivatives, src/audio.py:119-154), mel or linear features of .wav files as
<stem>-<feat>.npy and, with `--segment-file` (the segments.csv of --align-wav-dir), the same cut at the phone boundaries as
<stem>-<feat>-seg.npy (solver.FeatureWriter; the reference's segment_file / segment_feat / min_segment_len, src/audio.py:309-354).
`--mcd-wav-dir` (not a mode of the reference) scores synthesised .wav files against the recordings of `--mcd-ref-dir` by mel-cepstral
distortion along a dynamic-time-warping path (solver.McdScorer, semi_tts_amd.metrics.mcd): mcd.csv, one row per pair, and with
`--mcd-path` the warp of every pair as <key>.dtw.npy.
`--feat f0` writes the pitch track of every file as <stem>-f0.npy (frames,) in Hz, 0 where unvoiced (the YIN tracker of
AudioConverter.extract_f0_batch at the MFCC hop), and `--mcd-f0` adds f0.csv to --mcd-wav-dir: F0 RMSE in cents, voicing error and gross
pitch error of every pair along the warp of its MCD (semi_tts_amd.metrics.f0_scores).
`--synth-phn-dir` (not a mode of the reference, which decodes to the length of the ground-truth mel) synthesises the .phn transcripts of a
directory -- what `--transcribe-wav-dir` writes, as it is -- and finds where each utterance ends from its attention on the GPU
(solver.Synthesiser, semi_tts_amd.metrics.attention_endpoints): <name>-mel.npy, -spec.npy, -align.npy, -dur.npy cut at the end, with
`--gen-wav` <name>-pred.wav, and synth.csv with the alignment diagnostics of every utterance.
`--score-phn-dir HYP --score-ref-dir REF` (not a mode of the reference, whose cal_per returns one rate) scores .phn transcripts -- what
`--transcribe-wav-dir` writes -- against reference transcripts by Levenshtein alignment with its trace-back on the GPU (solver.PhnScorer,
semi_tts_amd.metrics.align_transcripts): per.csv with correct / substituted / deleted / inserted phones per file, confusion.npy,
confusions.csv, phones.csv, with `--score-ali` <key>.ops per file and with `--score-nbest` the lowest error over the paths of a file.
`--abx-ali-dir ALI --abx-wav-dir WAVS` (not a mode of the reference) scores a representation itself -- MFCC, mel, the speech-encoder latents or
the codebook posteriors -- by the ABX phone-discrimination error of ZeroSpeech / Libri-light: the phone tokens the .ali files of
`--align-wav-dir` delimit are compared within speaker and context by path-normalised DTW, one wave per pair on the GPU (solver.AbxScorer,
semi_tts_amd.metrics.abx, st_dtw_pairs + st_abx_count): abx.csv with the error of every ordered phone pair, abx_phones.csv with the tokens used.
`--abx-mode across|both --abx-spk-map FILE` takes X from another speaker of the same context instead (metrics.abx_across, st_abx_across):
abx_across.csv and abx_across_speakers.csv; `both` runs the within-speaker path first and then the across-speaker one.
`--kmeans-wav-dir DIR --kmeans-out FILE.npy` (not a mode of the reference) makes the representation those measures are compared against, the
k-means units of ZeroSpeech / HuBERT-style baselines: the MFCC, mel or latent frames of a directory are clustered on the GPU (solver.KMeansTrainer,
semi_tts_amd.kmeans.fit: st_kmeans_assign + st_kmeans_update per iteration, k-means++ seeding on the device) into a (K, D) codebook, with
kmeans.csv (restart,iter,inertia,shift,empty) and kmeans_units.csv (unit,frames).  `--units-wav-dir DIR --units-codebook FILE.npy` writes the unit
sequence of every file as <stem>.phn (ids 3 + unit, repeats merged), which `--build-lm-phn-dir --lm-classes <3 + K>` and `--score-phn-dir` read as they are, and
`--abx-ali-dir ... --abx-codebook FILE.npy` replaces every feature row by its nearest centroid before the items are cut: the discrete-unit ABX.
`--stoi-wav-dir SYN --stoi-ref-dir REF` (not a mode of the reference) scores processed .wav files -- what `--vocode-dir`, `--gen-specgram --gen-wav`,
`--resample-wav-dir` or `--loudness-out` write -- against the time-aligned recordings they were made from by short-time objective
intelligibility on the GPU (solver.StoiScorer, semi_tts_amd.metrics.stoi, st_stoi_batch): stoi.csv with STOI and ESTOI of every pair.  The
measure needs the two signals sample-aligned; it is not for `--synth-phn-dir`, whose timing is the model's own (`--mcd-wav-dir` warps time).
With `--stoi-align` a constant shift between the two files of a pair -- a codec's, another vocoder's, a foreign cutter's -- is searched first, to
the sample, within +-`--stoi-max-delay` seconds by an exact float64 cross-correlation on the GPU (semi_tts_amd.metrics.align_pairs,
st_xcorr_delay), the overlap is scored and delay.csv written; `--stoi-sdr` adds sdr.csv with SI-SDR, SNR and gain (st_sisdr_batch).
"""
import argparse
import os
import random

import numpy as np
import torch
import yaml

parser = argparse.ArgumentParser(description='semi-tts decode path on MI355X.')
parser.add_argument('--config', type=str, help='Path to experiment config.')
parser.add_argument('--name', default=None, type=str, help='Name for logging.')
parser.add_argument('--logdir', default='log/', type=str, help='Logging path.')
parser.add_argument('--ckpdir', default='ckpt/', type=str, help='Checkpoint/Result path.')
parser.add_argument('--load', default=None, type=str, help='Load pre-trained model')
parser.add_argument('--seed', default=0, type=int, help='Random seed for reproducable results.')
parser.add_argument('--njobs', default=5, type=int, help='(unused: no data loader workers)')
parser.add_argument('--cpu', action='store_true', help='Not supported: the path is MI355X-only.')
parser.add_argument('--debug', action='store_true', help='Debug use. (parsed and never read by the reference either)')
parser.add_argument('--no-pin', action='store_true', help='Disable pin-memory for dataloader (no data loader here: ignored)')
parser.add_argument('--asr-decode', action='store_true', help='ASR beam decode (the reference dispatches to bin/asr_decode.py, which its tree lacks)')
parser.add_argument('--gen-specgram', action='store_true', help='Generating mel/linear spectrogram.')
parser.add_argument('--gen-gt-specgram', action='store_true', help='(the reference dispatches to bin/gen_gt_specgram.py, which its tree lacks)')
parser.add_argument('--no-msg', action='store_true', help='Hide all messages.')
parser.add_argument('--actual-len', action='store_true', help='Using actual len for CTC loss: frames of each utterance that are not padding, counted on the device.')
parser.add_argument('--store-best-per', action='store_true', help='Only store the model with best PER. (with --dev-batches; without a dev set: no effect)')
parser.add_argument('--asr-only', action='store_true', help='(the reference dispatches to bin/train_asr.py, which its tree lacks)')
parser.add_argument('--gen-wav', action='store_true', help='Generate waveform using Griffin-Lim. (--gen-specgram: writes <name>-pred.wav)')
# synthetic-data knobs (the reference reads these from the corpus)
parser.add_argument('--frames', default=256, type=int, help='mel frames per synthetic utterance')
parser.add_argument('--batch-size', default=None, type=int)
parser.add_argument('--n-batches', default=1, type=int)
parser.add_argument('--unpair-batch-size', default=None, type=int, help='utterances per synthetic unpaired batch (default: --batch-size)')
parser.add_argument('--unpair-frames', default=None, type=int, help='mel frames per synthetic unpaired utterance (default: --frames)')
parser.add_argument('--unpair-wav-dir', default=None, type=str, help='unpaired batches: (mel, aug_mel, linear) extracted on the GPU from the '
                    '.wav files of this directory, sorted by name, batched by --unpair-batch-size, fresh augmentation every fetch '
                    '(text / sid stay synthetic)')
parser.add_argument('--corpus', action='store_true', help='train on the files data.corpus names (partition_table, map_table, spkr_map, vocab_file, '
                    '<path>/<speaker>/<id>.wav) instead of synthetic batches: the paired / unpaired / dev splits stay on the device as packed '
                    'waveforms, features are extracted on every fetch; vocab_size and n_spkr come from the files')
parser.add_argument('--corpus-max-gb', default=None, type=float, help='--corpus: the most device memory one split may take, in GB (default: half '
                    'of the free device memory when the split is loaded)')
parser.add_argument('--max-frames', default=None, type=int, help='--corpus: drop utterances of more mel frames than this (default: keep all)')
parser.add_argument('--stretch', action='store_true', help='aug_mel lengths drawn from data.audio.time_stretch_range (default: unstretched)')
parser.add_argument('--tts-only', action='store_true', help='train the paired TTS branch alone (TtsTrainer) instead of the two cycles')
parser.add_argument('--max-step', default=None, type=int, help='training steps (default: hparas.max_step)')
parser.add_argument('--save', action='store_true', help='write ckpt/<name>/latest.pth ({model, optimizer, global_step}) after training')
parser.add_argument('--dev-batches', default=0, type=int, help='validate on K synthetic dev batches (paired shapes) at step 1 and every '
                    'valid step: dev TTS loss, PER, post PER, checkpoints by the reference\'s rules (default 0: no validation); with --corpus '
                    'the first K batches of the dev split, -1: the whole split')
parser.add_argument('--valid-step', default=None, type=int, help='steps between validations (default: hparas.valid_step)')
parser.add_argument('--transcribe-wav-dir', default=None, type=str, help='transcribe the .wav files of this directory (sorted by name, '
                    'batched by --batch-size) by CTC prefix beam search into <logdir>/<name>/<file>.phn: --top-paths lines of score<TAB>tokens')
parser.add_argument('--beam-width', default=16, type=int, help='--transcribe-wav-dir: beam width (1 .. 128)')
parser.add_argument('--top-paths', default=1, type=int, help='--transcribe-wav-dir: paths written per file (1 .. --beam-width)')
parser.add_argument('--vocab', default=None, type=str, help='--transcribe-wav-dir / --align-wav-dir: phone list, one per line (id = 3 + line index); '
                    'without it the .phn files hold ids')
parser.add_argument('--asr-output', default='code', choices=('code', 'post'), help='--transcribe-wav-dir / --align-wav-dir: use the codebook '
                    'posteriors (code) or the ASR postnet log-posteriors (post)')
parser.add_argument('--align-wav-dir', default=None, type=str, help='align the .wav files of this directory (sorted by name, batched by '
                    '--batch-size) to their transcripts <name>.phn by CTC forced alignment: <logdir>/<name>/<file>.ali (one line per token: '
                    'symbol, start / end frame, start / end second) and segments.csv (file,seg); reads --vocab and --asr-output')
parser.add_argument('--phn-dir', default=None, type=str, help='--align-wav-dir: directory of the .phn transcripts (default: the .wav directory)')
parser.add_argument('--lm', default=None, type=str, help='--transcribe-wav-dir: fuse this phone n-gram table (.npy, (V^(order-1), V) '
                    'probabilities, contexts starting at (0, ..., 0, 1)) into the beam search; --build-lm-phn-dir: the table to write')
parser.add_argument('--lm-weight', default=None, type=float, help='--lm with --transcribe-wav-dir: weight of log P(phone | context) per '
                    'new phone (default 0.5)')
parser.add_argument('--ins-bonus', default=None, type=float, help='--lm with --transcribe-wav-dir: constant added per new phone (default 0)')
parser.add_argument('--build-lm-phn-dir', default=None, type=str, help='count an n-gram table of order --lm-order from the .phn '
                    'transcripts of this directory (ids or --vocab symbols, id 0 skipped) and write it to --lm; no GPU, no other mode')
parser.add_argument('--lm-order', default=None, type=int, help='--build-lm-phn-dir: order of the table (1 .. 4)')
parser.add_argument('--lm-classes', default=None, type=int, help='--build-lm-phn-dir: the classes V of the table (default 43: <pad>, <space>, <eos> and '
                    '40 phones); the unit transcripts of --units-wav-dir under a codebook of K centroids take V = 3 + K')
parser.add_argument('--lm-smooth', default=None, type=float, help='--build-lm-phn-dir: add-K smoothing over the non-blank phones (default 1)')
parser.add_argument('--gen-wav-feat', default='linear', choices=('linear', 'mel'), help='--gen-specgram --gen-wav: vocode the predicted '
                    'linear spectrogram (default) or the predicted mel (through the filterbank\'s pseudo-inverse) into <name>-pred.wav')
parser.add_argument('--vocode-dir', default=None, type=str, help='vocode the saved spectrograms of this directory (the *-spec.npy / '
                    '*-mel.npy files --gen-specgram writes; sorted by name, batched by --batch-size, each at its own length) by '
                    'Griffin-Lim into <logdir>/<name>/<stem>.wav; no checkpoint, no model')
parser.add_argument('--vocode-feat', default=None, choices=('spec', 'mel'), help='--vocode-dir: read *-spec.npy (default) or *-mel.npy')
parser.add_argument('--resample', action='store_true', help='--unpair-wav-dir / --transcribe-wav-dir / --align-wav-dir: convert files whose '
                    'sample rate is not data.audio.sample_rate on the GPU (windowed sinc) instead of refusing them')
parser.add_argument('--resample-wav-dir', default=None, type=str, help='convert channel 0 of the .wav files of this directory (sorted by name, '
                    'batched by --batch-size) to --resample-rate on the GPU and write them as 16-bit mono into --resample-out/<same name>; '
                    'no checkpoint, no model')
parser.add_argument('--resample-out', default=None, type=str, help='--resample-wav-dir: the directory to write (not the one read)')
parser.add_argument('--resample-rate', default=None, type=int, help='--resample-wav-dir: the output rate in Hz (default: data.audio.sample_rate '
                    'of --config)')
parser.add_argument('--feat-wav-dir', default=None, type=str, help='extract --feat from the .wav files of this directory (sorted by name, batched '
                    'by --batch-size) on the GPU into <logdir>/<name>/<stem>-<feat>.npy (frames, dim); no checkpoint, no model')
parser.add_argument('--feat', default=None, choices=('mfcc', 'mel', 'linear', 'f0'), help='--feat-wav-dir: the feature written: 39-dimensional MFCC '
                    '(25 / 10 ms framing), the clean mel / linear spectrogram of data.audio, or f0: the pitch track in Hz at the MFCC hop, '
                    '<stem>-f0.npy (frames,), 0 where unvoiced (not with --segment-file)')
parser.add_argument('--segment-file', default=None, type=str, help='--feat-wav-dir: a segment table (file,seg: the segments.csv of '
                    '--align-wav-dir); also write <stem>-<feat>-seg.npy (segments, longest piece, dim), the feature cut at its boundaries')
parser.add_argument('--min-segment-len', default=None, type=int, help='--segment-file: the fewest frames of a segment; a shorter piece joins '
                    'the next one (default 2)')
parser.add_argument('--mcd-wav-dir', default=None, type=str, help='score the synthesised .wav files of this directory (sorted by name, batched by '
                    '--batch-size) against their recordings in --mcd-ref-dir by mel-cepstral distortion along a DTW path on the GPU: '
                    '<logdir>/<name>/mcd.csv (file,frames,ref_frames,path_len,mcd_db); no checkpoint, no model')
parser.add_argument('--mcd-ref-dir', default=None, type=str, help='--mcd-wav-dir: the directory of the recordings, <key>.wav for every synthesised '
                    'file (key: its name up to the first ".", without one trailing "-pred")')
parser.add_argument('--mcd-path', action='store_true', help='--mcd-wav-dir: also write the warp of every pair as <key>.dtw.npy, (path_len, 2) int32')
parser.add_argument('--mcd-f0', action='store_true', help='--mcd-wav-dir: also track the pitch of both sides and write <logdir>/<name>/f0.csv '
                    '(file,path_len,voiced_pairs,f0_rmse_cents,vuv_error,gross_error,mean_cents) along the warp of the MCD')
parser.add_argument('--f0-min', default=None, type=float, help='--feat f0 / --mcd-f0: the lowest pitch searched, in Hz (default 60)')
parser.add_argument('--f0-max', default=None, type=float, help='--feat f0 / --mcd-f0: the highest pitch searched, in Hz (default 500)')
parser.add_argument('--f0-threshold', default=None, type=float, help='--feat f0 / --mcd-f0: the YIN threshold on the normalised difference, in '
                    '(0, 1] (default 0.15)')
parser.add_argument('--synth-phn-dir', default=None, type=str, help='synthesise the .phn transcripts of this directory (sorted by name, batched by '
                    '--batch-size; ids or --vocab symbols, the files of --transcribe-wav-dir as they are), each cut where its attention has '
                    'stayed on the last phone: <logdir>/<name>/<file>-mel.npy, -spec.npy, -align.npy, -dur.npy, with --gen-wav -pred.wav, and '
                    'synth.csv (file,tokens,steps,frames,seconds,reached,focus,backward,skips,covered)')
parser.add_argument('--synth-sid', default=None, type=int, help='--synth-phn-dir: the speaker id of every utterance (default 0)')
parser.add_argument('--end-patience', default=None, type=int, help='--synth-phn-dir: decoder steps the attention peak must stay at or past '
                    'the last phone before the utterance ends (default 3)')
parser.add_argument('--end-max-jump', default=None, type=int, help='--synth-phn-dir: a step whose attention peak moves forward by more '
                    'phones than this counts as a skip (default 4)')
parser.add_argument('--max-frames-per-phone', default=None, type=float, help='--synth-phn-dir: frames decoded per phone of the longest '
                    'transcript of a batch, before the margin of 40 (default 12, twice the corpus ratio)')
parser.add_argument('--trim-silence', action='store_true', help='--corpus / --unpair-wav-dir / --transcribe-wav-dir / --mcd-wav-dir (both sides) / '
                    '--feat-wav-dir (without --segment-file): cut the leading and trailing silence of every utterance on the GPU after loading '
                    '(AudioConverter.trim_batch: frames less than --trim-top-db dB under the loudest frame are silent)')
parser.add_argument('--trim-top-db', default=None, type=float, help='--trim-silence / --trim-wav-dir: the threshold in dB under the loudest frame (default 60)')
parser.add_argument('--trim-frame-length', default=None, type=int, help='--trim-silence / --trim-wav-dir: samples per energy frame (default 2048, at most 8192)')
parser.add_argument('--trim-hop', default=None, type=int, help='--trim-silence / --trim-wav-dir: samples between energy frames (default 512)')
parser.add_argument('--trim-pad-ms', default=None, type=float, help='--trim-silence / --trim-wav-dir: milliseconds kept on both sides of the speech (default 0)')
parser.add_argument('--trim-wav-dir', default=None, type=str, help='cut the leading and trailing silence of the .wav files of this directory (sorted by '
                    'name, batched by --batch-size, at data.audio.sample_rate of --config) and write the kept span of channel 0 -- the exact 16-bit '
                    'samples -- to --trim-out/<same name>, with --trim-out/trim.csv (file, samples, start, end, seconds, kept_seconds, n_intervals); no model')
parser.add_argument('--trim-out', default=None, type=str, help='--trim-wav-dir: the directory to write (not the one read)')
parser.add_argument('--normalize-loudness', action='store_true', help='--corpus / --unpair-wav-dir / --transcribe-wav-dir / --feat-wav-dir (without '
                    '--segment-file) / --mcd-wav-dir (both sides): bring every loaded utterance to --loudness-target LUFS on the GPU (ITU-R BS.1770-4 '
                    'integrated loudness, AudioConverter.loudness_batch), after resampling and trimming; --gen-specgram --gen-wav / --vocode-dir / '
                    '--synth-phn-dir --gen-wav: the written waveforms instead')
parser.add_argument('--loudness-target', default=None, type=float, help='--normalize-loudness / --loudness-wav-dir: the integrated loudness to reach, in LUFS, '
                    'within [-70, 0] (default -23, EBU R 128)')
parser.add_argument('--loudness-peak', default=None, type=float, help='--normalize-loudness / --loudness-wav-dir: the sample peak the gain must not pass, in dBFS, '
                    'at most 0 (default -1)')
parser.add_argument('--loudness-max-gain', default=None, type=float, help='--normalize-loudness / --loudness-wav-dir: the largest gain applied, in dB, at least 0 '
                    '(default 30)')
parser.add_argument('--loudness-wav-dir', default=None, type=str, help='meter the .wav files of this directory (sorted by name, batched by --batch-size, at '
                    'data.audio.sample_rate of --config; --resample and --trim-silence are honoured) and write loudness.csv (file, samples, seconds, lufs, '
                    'momentary_max, rel_gate, peak_dbfs, n_blocks, n_abs, n_rel, gain_db, flags) into --loudness-out, or into the directory itself without it; no model')
parser.add_argument('--loudness-out', default=None, type=str, help='--loudness-wav-dir: also write every file normalised as 16-bit mono into this directory '
                    '(not the one read); a file the meter flags (non-finite, under 400 ms, silent) keeps its level')
parser.add_argument('--score-phn-dir', default=None, type=str, help='score the .phn transcripts of this directory (sorted by name, batched by '
                    '--batch-size; ids or --vocab symbols, the files of --transcribe-wav-dir as they are) against the references of '
                    '--score-ref-dir by Levenshtein alignment on the GPU: <logdir>/<name>/per.csv (file,ref_tokens,hyp_tokens,correct,sub,del,ins,per), '
                    'confusion.npy, confusions.csv, phones.csv; no config, no checkpoint, no model')
parser.add_argument('--score-ref-dir', default=None, type=str, help='--score-phn-dir: the directory of the reference transcripts, <key>.phn for every '
                    'scored file (key: its name up to the first ".", without one trailing "-pred")')
parser.add_argument('--score-ignore', default=None, type=str, help='--score-phn-dir: comma-separated ids dropped from both sides (default 0,1,2: the '
                    'three special tokens; 0,1,2,42 reproduces the filter of cal_per, which also drops the last phone of the reference\'s vocabulary)')
parser.add_argument('--score-nbest', action='store_true', help='--score-phn-dir: score every line of a hypothesis file (the paths of --top-paths) and add '
                    'nbest_per,nbest_path to per.csv: the lowest error over the paths and the first path that attains it')
parser.add_argument('--score-ali', action='store_true', help='--score-phn-dir: also write the alignment of every file as <key>.ops (REF / HYP / OP lines)')
parser.add_argument('--abx-ali-dir', default=None, type=str, help='score a representation by the ABX phone-discrimination error on the GPU: every '
                    '<stem>.ali of this directory (the files of --align-wav-dir) gives the phone boundaries of --abx-wav-dir/<stem>.wav; writes '
                    '<logdir>/<name>/abx.csv (phone_a,phone_b,cells,triples,error) and abx_phones.csv (phone,tokens,items,too_short,too_long)')
parser.add_argument('--abx-wav-dir', default=None, type=str, help='--abx-ali-dir: the directory of the waveforms')
parser.add_argument('--abx-feat', default=None, choices=('mfcc', 'mel', 'latent', 'code'), help='--abx-ali-dir: the representation scored: MFCC '
                    '(default) or clean mel (no checkpoint, no model), or the speech-encoder latents / codebook posteriors of the model of '
                    '--load (the synthetic weights without it)')
parser.add_argument('--abx-metric', default=None, choices=('angular', 'kl', 'euclid'), help='--abx-ali-dir: the frame distance under the DTW '
                    '(default angular; kl for --abx-feat code)')
parser.add_argument('--abx-context', default=None, choices=('triphone', 'none'), help='--abx-ali-dir: compare tokens that share speaker, previous '
                    'and next symbol (triphone, default; the utterance\'s edge is a symbol of its own) or the speaker alone (none)')
parser.add_argument('--abx-spk-map', default=None, type=str, help='--abx-ali-dir: a key,speaker CSV (key: the file\'s stem); without it all files '
                    'are one speaker.  ABX is taken within speaker unless --abx-mode says otherwise')
parser.add_argument('--abx-ignore', default=None, type=str, help='--abx-ali-dir: comma-separated symbols that are never items (they still count as '
                    'context)')
parser.add_argument('--abx-max-items', default=None, type=int, help='--abx-ali-dir: the most tokens of one phone in one cell; above it a seeded '
                    'subsample (--seed) is scored (default 50)')
parser.add_argument('--abx-min-frames', default=None, type=int, help='--abx-ali-dir: tokens of fewer feature rows are dropped (default 1; tokens '
                    'of more than 64 rows always are)')
parser.add_argument('--abx-mode', default=None, choices=('within', 'across', 'both'), help='--abx-ali-dir: where X comes from: the speaker of A and '
                    'B (within, default), another speaker of the same context (across: abx_across.csv with phone_a,phone_b,groups,triples,error and '
                    'abx_across_speakers.csv with speaker,groups,error), or one run after the other (both); across and both need --abx-spk-map')
parser.add_argument('--abx-max-gb', default=None, type=float, help='--abx-mode across|both: the most GiB of distance matrices and pair tables '
                    '(default 8); above it the run is refused')
parser.add_argument('--abx-codebook', default=None, type=str, help='--abx-ali-dir: a (K, D) float32 .npy table of centroids (what --kmeans-out '
                    'writes); every feature row is replaced by its nearest centroid before the items are cut (discrete-unit ABX)')
parser.add_argument('--kmeans-wav-dir', default=None, type=str, help='fit a k-means codebook to the frames of the .wav files of this directory on '
                    'the GPU (sorted by name, batched by --batch-size): --kmeans-out FILE.npy, <logdir>/<name>/kmeans.csv '
                    '(restart,iter,inertia,shift,empty) and kmeans_units.csv (unit,frames)')
parser.add_argument('--kmeans-out', default=None, type=str, help='--kmeans-wav-dir: the .npy file the (K, D) float32 codebook is written to')
parser.add_argument('--kmeans-feat', default=None, choices=('mfcc', 'mel', 'latent'), help='--kmeans-wav-dir / --units-wav-dir: the frames '
                    'clustered: MFCC (default) and mel need no checkpoint and no model; latent is the speech encoder of --load')
parser.add_argument('--kmeans-k', default=None, type=int, help='--kmeans-wav-dir: the number of centroids (default 50, at most 4096)')
parser.add_argument('--kmeans-iters', default=None, type=int, help='--kmeans-wav-dir: the most Lloyd iterations of a fit (default 100)')
parser.add_argument('--kmeans-tol', default=None, type=float, help='--kmeans-wav-dir: a fit stops when the squared move of the centroids is at most '
                    'this times the mean per-column variance of the frames (default 1e-4)')
parser.add_argument('--kmeans-init', default=None, choices=('++', 'sample'), help='--kmeans-wav-dir: k-means++ seeding (default) or K distinct frames, '
                    'both drawn from --seed')
parser.add_argument('--kmeans-restarts', default=None, type=int, help='--kmeans-wav-dir: fits from the seeds --seed, --seed + 1, ..; the one of '
                    'lowest inertia is written (default 1)')
parser.add_argument('--kmeans-max-gb', default=None, type=float, help='--kmeans-wav-dir: the most GiB of packed frames (default 8), computed from '
                    'the .wav headers; above it the run is refused before the device is touched')
parser.add_argument('--units-wav-dir', default=None, type=str, help='write the k-means unit sequence of every .wav file of this directory under '
                    '--units-codebook as <logdir>/<name>/<stem>.phn (ids 3 + unit, consecutive repeats merged, the score -mean squared distance)')
parser.add_argument('--units-codebook', default=None, type=str, help='--units-wav-dir: the (K, D) float32 .npy codebook of --kmeans-out')
parser.add_argument('--units-frames', action='store_true', help='--units-wav-dir: also write the unmerged frame-level units as <stem>-units.npy (int32)')
parser.add_argument('--stoi-wav-dir', default=None, type=str, help='score the processed .wav files of this directory (sorted by name, batched by '
                    '--batch-size; 16-bit mono PCM of any rate the resampler takes) against their time-aligned recordings in --stoi-ref-dir by STOI and '
                    'ESTOI on the GPU: <logdir>/<name>/stoi.csv (file,samples,frames,kept,segments,stoi,estoi); no config, no checkpoint, no model')
parser.add_argument('--stoi-ref-dir', default=None, type=str, help='--stoi-wav-dir: the directory of the recordings, <key>.wav for every processed '
                    'file (key: its name up to the first ".", without one trailing "-pred"), at the rate of its processed file')
parser.add_argument('--stoi-max-len-diff', default=None, type=float, help='--stoi-wav-dir: the most seconds the two files of a pair may differ in '
                    'length; the longer one is cut at its end (default 0.05: three decoder frames and a vocoder\'s partial hop)')
parser.add_argument('--stoi-align', action='store_true', help='--stoi-wav-dir: search each pair\'s integer delay at the files\' own rate within '
                    '+-(--stoi-max-delay) seconds on the GPU and score the overlap it leaves; <logdir>/<name>/delay.csv '
                    '(file,delay_samples,delay_s,coef), positive: the processed file is late')
parser.add_argument('--stoi-max-delay', default=None, type=float, help='--stoi-align: the search bound in seconds (default 0.05; at most 16384 '
                    'samples at the files\' rate); the two lengths of a pair may then differ by --stoi-max-len-diff plus this')
parser.add_argument('--stoi-sdr', action='store_true', help='--stoi-wav-dir: also write <logdir>/<name>/sdr.csv (file,samples,si_sdr,snr,gain_db) on '
                    'the same samples: the aligned overlap with --stoi-align, delay 0 without')
parser.add_argument('--async-stats', action='store_true', help='training: no host read of loss / gradient norm inside a step (read when logged; '
                    'a NaN gradient norm skips the update on the device)')


# Flags of the reference (main.py:23-33) with nothing to do on this path (--gen-wav outside --gen-specgram), and those whose solver files are
# absent from the reference tree itself (main.py:49-60 import bin/asr_decode.py, bin/gen_gt_specgram.py,
# bin/train_asr.py, none of which exist): accepted by the parser so that existing launch lines keep working.
IGNORED_FLAGS = ('debug', 'no_pin', 'store_best_per', 'gen_wav')
MISSING_SOLVERS = {'asr_decode': 'bin/asr_decode.py', 'gen_gt_specgram': 'bin/gen_gt_specgram.py',
                   'asr_only': 'bin/train_asr.py'}


def parse_args(argv=None):
    """The reference's command lines parse unchanged (ref: main.py:14-41); returns the same `paras`
    attributes it sets (`gpu`, `pin_memory` -- inverted there as here, main.py:40 --, `verbose`)."""
    paras = parser.parse_args(argv)
    setattr(paras, 'gpu', not paras.cpu)
    setattr(paras, 'pin_memory', False if paras.cpu else paras.no_pin)
    setattr(paras, 'verbose', not paras.no_msg)
    for flag, path in MISSING_SOLVERS.items():
        if getattr(paras, flag):
            parser.error('--%s: the reference dispatches this mode to %s, which is not part of the reference tree; '
                         'only the default (training) and --gen-specgram modes exist' % (flag.replace('_', '-'), path))
    if paras.unpair_wav_dir is not None and (paras.tts_only or paras.gen_specgram):
        parser.error('--unpair-wav-dir feeds the unpaired batches of the two cycles; it does not combine with --%s'
                     % ('tts-only' if paras.tts_only else 'gen-specgram'))
    if paras.corpus:
        for flag in ('unpair_wav_dir', 'gen_specgram', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir', 'resample_wav_dir',
                     'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'loudness_wav_dir'):
            if getattr(paras, flag):
                parser.error('--corpus trains on the splits of data.corpus (the unpaired one included); it does not combine with --%s'
                             % flag.replace('_', '-'))
        if paras.config is None:
            parser.error('--corpus needs --config (its data.corpus and data.audio)')
        if paras.corpus_max_gb is not None and not 0.0 < paras.corpus_max_gb < float('inf'):
            parser.error('--corpus-max-gb must be finite and positive')
        if paras.max_frames is not None and paras.max_frames < 1:
            parser.error('--max-frames must be >= 1')
    elif paras.corpus_max_gb is not None or paras.max_frames is not None:
        parser.error('--corpus-max-gb and --max-frames belong to --corpus; they need that flag')
    if paras.dev_batches < (-1 if paras.corpus else 0) or (paras.valid_step is not None and paras.valid_step < 1):
        parser.error('--dev-batches must be >= 0 (with --corpus: -1 walks the whole dev split) and --valid-step >= 1')
    if paras.dev_batches != 0 and (paras.tts_only or paras.gen_specgram):
        parser.error('--dev-batches validates the two cycles (VqvaeTrainer); it does not combine with --%s'
                     % ('tts-only' if paras.tts_only else 'gen-specgram'))
    if paras.transcribe_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir'):
            if getattr(paras, flag):
                parser.error('--transcribe-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--transcribe-wav-dir does not combine with --dev-batches')
        if not (1 <= paras.top_paths <= paras.beam_width <= 128):
            parser.error('--transcribe-wav-dir needs 1 <= --top-paths <= --beam-width <= 128')
    if paras.align_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir'):
            if getattr(paras, flag):
                parser.error('--align-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--align-wav-dir does not combine with --dev-batches')
    elif paras.phn_dir is not None:
        parser.error('--phn-dir names the transcripts of --align-wav-dir; it needs that flag')
    if paras.vocode_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir'):
            if getattr(paras, flag):
                parser.error('--vocode-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--vocode-dir does not combine with --dev-batches')
    elif paras.vocode_feat is not None:
        parser.error('--vocode-feat names the files --vocode-dir reads; it needs that flag')
    if paras.vocode_feat is None:
        paras.vocode_feat = 'spec'
    if (paras.resample and paras.unpair_wav_dir is None and paras.transcribe_wav_dir is None and paras.align_wav_dir is None and not paras.corpus
            and paras.loudness_wav_dir is None and paras.abx_ali_dir is None and paras.kmeans_wav_dir is None and paras.units_wav_dir is None):
        parser.error('--resample converts the files of --unpair-wav-dir, --transcribe-wav-dir or --align-wav-dir, or the splits of --corpus; it needs one '
                     'of them')
    if paras.resample_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir'):
            if getattr(paras, flag):
                parser.error('--resample-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--resample-wav-dir does not combine with --dev-batches')
        if paras.resample_out is None:
            parser.error('--resample-wav-dir needs --resample-out DIR (the directory to write)')
        if os.path.realpath(paras.resample_out) == os.path.realpath(paras.resample_wav_dir):
            parser.error('--resample-out must not be the directory --resample-wav-dir reads')
        if paras.resample_rate is not None and paras.resample_rate < 1:
            parser.error('--resample-rate must be a positive number of Hz')
        if paras.resample_rate is None and paras.config is None:
            parser.error('--resample-wav-dir needs --resample-rate N or --config (its data.audio.sample_rate)')
    elif paras.resample_out is not None or paras.resample_rate is not None:
        parser.error('--resample-out and --resample-rate belong to --resample-wav-dir; they need that flag')
    if paras.feat_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir'):
            if getattr(paras, flag):
                parser.error('--feat-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--feat-wav-dir does not combine with --dev-batches')
        if paras.config is None or paras.feat is None:
            parser.error('--feat-wav-dir needs --config (its data.audio) and --feat mfcc|mel|linear')
        if paras.min_segment_len is not None and paras.segment_file is None:
            parser.error('--min-segment-len belongs to --segment-file; it needs that flag')
        if paras.min_segment_len is not None and paras.min_segment_len < 1:
            parser.error('--min-segment-len must be >= 1')
    elif paras.feat is not None or paras.segment_file is not None or paras.min_segment_len is not None:
        parser.error('--feat, --segment-file and --min-segment-len belong to --feat-wav-dir; they need that flag')
    if paras.min_segment_len is None:
        paras.min_segment_len = 2
    if paras.mcd_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir'):
            if getattr(paras, flag):
                parser.error('--mcd-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--mcd-wav-dir does not combine with --dev-batches')
        if paras.config is None or paras.mcd_ref_dir is None:
            parser.error('--mcd-wav-dir needs --config (its data.audio) and --mcd-ref-dir DIR (the recordings)')
    elif paras.mcd_ref_dir is not None or paras.mcd_path:
        parser.error('--mcd-ref-dir and --mcd-path belong to --mcd-wav-dir; they need that flag')
    elif paras.mcd_f0:
        parser.error('--mcd-f0 belongs to --mcd-wav-dir; it needs that flag')
    if not (paras.feat == 'f0' or paras.mcd_f0) and any(v is not None for v in (paras.f0_min, paras.f0_max, paras.f0_threshold)):
        parser.error('--f0-min, --f0-max and --f0-threshold set the pitch tracker of --feat f0 and --mcd-f0; they need one of them')
    paras.f0_min = 60.0 if paras.f0_min is None else paras.f0_min
    paras.f0_max = 500.0 if paras.f0_max is None else paras.f0_max
    paras.f0_threshold = 0.15 if paras.f0_threshold is None else paras.f0_threshold
    if not (0.0 < paras.f0_min < paras.f0_max) or not (0.0 < paras.f0_threshold <= 1.0):
        parser.error('--f0-min, --f0-max and --f0-threshold need 0 < --f0-min < --f0-max and 0 < --f0-threshold <= 1')
    if paras.synth_phn_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir'):
            if getattr(paras, flag):
                parser.error('--synth-phn-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--synth-phn-dir does not combine with --dev-batches')
        if paras.config is None:
            parser.error('--synth-phn-dir needs --config (its model and data.audio)')
        if paras.synth_sid is not None and paras.synth_sid < 0:
            parser.error('--synth-sid must be >= 0')
        for flag in ('end_patience', 'end_max_jump'):
            v = getattr(paras, flag)
            if v is not None and v < 1:
                parser.error('--%s must be >= 1' % flag.replace('_', '-'))
        if paras.max_frames_per_phone is not None and not 0.0 < paras.max_frames_per_phone < float('inf'):
            parser.error('--max-frames-per-phone must be finite and positive')
    elif (paras.synth_sid is not None or paras.end_patience is not None or paras.end_max_jump is not None
          or paras.max_frames_per_phone is not None):
        parser.error('--synth-sid, --end-patience, --end-max-jump and --max-frames-per-phone belong to --synth-phn-dir; they need that flag')
    if paras.synth_sid is None:
        paras.synth_sid = 0
    if paras.end_patience is None:
        paras.end_patience = 3
    if paras.end_max_jump is None:
        paras.end_max_jump = 4
    if paras.stoi_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'loudness_wav_dir', 'score_phn_dir',
                     'abx_ali_dir', 'corpus'):
            if getattr(paras, flag):
                parser.error('--stoi-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        for flag in ('trim_silence', 'normalize_loudness'):
            if getattr(paras, flag):
                parser.error('--stoi-wav-dir does not combine with --%s: changing the two sides separately destroys the alignment the measure needs'
                             % flag.replace('_', '-'))
        if paras.dev_batches != 0:
            parser.error('--stoi-wav-dir does not combine with --dev-batches')
        if paras.stoi_ref_dir is None:
            parser.error('--stoi-wav-dir needs --stoi-ref-dir DIR (the recordings)')
        paras.stoi_max_len_diff = 0.05 if paras.stoi_max_len_diff is None else paras.stoi_max_len_diff
        if not 0.0 <= paras.stoi_max_len_diff < float('inf'):
            parser.error('--stoi-max-len-diff must be finite and at least 0 seconds')
        if paras.stoi_max_delay is not None and not paras.stoi_align:
            parser.error('--stoi-max-delay belongs to --stoi-align; it needs that flag')
        if paras.stoi_align:
            paras.stoi_max_delay = 0.05 if paras.stoi_max_delay is None else paras.stoi_max_delay
            if not 0.0 <= paras.stoi_max_delay < float('inf'):
                parser.error('--stoi-max-delay must be finite and at least 0 seconds')
    elif paras.stoi_ref_dir is not None or paras.stoi_max_len_diff is not None:
        parser.error('--stoi-ref-dir and --stoi-max-len-diff belong to --stoi-wav-dir; they need that flag')
    elif paras.stoi_align or paras.stoi_sdr or paras.stoi_max_delay is not None:
        parser.error('--stoi-align, --stoi-max-delay and --stoi-sdr belong to --stoi-wav-dir; they need that flag')
    if paras.trim_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_silence'):
            if getattr(paras, flag):
                parser.error('--trim-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--trim-wav-dir does not combine with --dev-batches')
        if paras.trim_out is None or paras.config is None:
            parser.error('--trim-wav-dir needs --trim-out DIR (the directory to write) and --config (its data.audio)')
        if os.path.realpath(paras.trim_out) == os.path.realpath(paras.trim_wav_dir):
            parser.error('--trim-out must not be the directory --trim-wav-dir reads')
    elif paras.trim_out is not None:
        parser.error('--trim-out belongs to --trim-wav-dir; it needs that flag')
    if paras.trim_silence:
        if paras.align_wav_dir is not None:
            parser.error('--trim-silence does not combine with --align-wav-dir: its times refer to the untrimmed file')
        if paras.segment_file is not None:
            parser.error('--trim-silence does not combine with --segment-file: its times refer to the untrimmed file')
        if not (paras.corpus or any(getattr(paras, f) is not None for f in ('unpair_wav_dir', 'transcribe_wav_dir', 'mcd_wav_dir', 'feat_wav_dir',
                                                                            'loudness_wav_dir', 'abx_ali_dir', 'kmeans_wav_dir', 'units_wav_dir'))):
            parser.error('--trim-silence trims what --corpus, --unpair-wav-dir, --transcribe-wav-dir, --mcd-wav-dir or --feat-wav-dir load; it needs one '
                         'of them')
    elif paras.trim_wav_dir is None and any(v is not None for v in (paras.trim_top_db, paras.trim_frame_length, paras.trim_hop, paras.trim_pad_ms)):
        parser.error('--trim-top-db, --trim-frame-length, --trim-hop and --trim-pad-ms set --trim-silence or --trim-wav-dir; they need one of them')
    paras.trim_top_db = 60.0 if paras.trim_top_db is None else paras.trim_top_db
    paras.trim_frame_length = 2048 if paras.trim_frame_length is None else paras.trim_frame_length
    paras.trim_hop = 512 if paras.trim_hop is None else paras.trim_hop
    paras.trim_pad_ms = 0.0 if paras.trim_pad_ms is None else paras.trim_pad_ms
    if not 0.0 < paras.trim_top_db < float('inf') or not 1 <= paras.trim_hop <= paras.trim_frame_length <= 8192 or not 0.0 <= paras.trim_pad_ms < float('inf'):
        parser.error('--trim-top-db must be finite and positive, 1 <= --trim-hop <= --trim-frame-length <= 8192 and --trim-pad-ms finite and >= 0')
    if paras.loudness_wav_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'score_phn_dir', 'normalize_loudness'):
            if getattr(paras, flag):
                parser.error('--loudness-wav-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--loudness-wav-dir does not combine with --dev-batches')
        if paras.config is None:
            parser.error('--loudness-wav-dir needs --config (its data.audio.sample_rate)')
        if paras.loudness_out is not None and os.path.realpath(paras.loudness_out) == os.path.realpath(paras.loudness_wav_dir):
            parser.error('--loudness-out must not be the directory --loudness-wav-dir reads')
    elif paras.loudness_out is not None:
        parser.error('--loudness-out belongs to --loudness-wav-dir; it needs that flag')
    if paras.normalize_loudness:
        if paras.align_wav_dir is not None:
            parser.error('--normalize-loudness does not combine with --align-wav-dir in this version (times would not change; the listed modes only)')
        if paras.segment_file is not None:
            parser.error('--normalize-loudness does not combine with --segment-file in this version (times would not change; the listed modes only)')
        writes = paras.vocode_dir is not None or (paras.gen_wav and (paras.gen_specgram or paras.synth_phn_dir is not None))
        if not (paras.corpus or writes or any(getattr(paras, f) is not None for f in ('unpair_wav_dir', 'transcribe_wav_dir', 'mcd_wav_dir', 'feat_wav_dir', 'abx_ali_dir', 'kmeans_wav_dir', 'units_wav_dir'))):
            parser.error('--normalize-loudness normalises what --corpus, --unpair-wav-dir, --transcribe-wav-dir, --feat-wav-dir or --mcd-wav-dir load and what '
                         '--gen-specgram --gen-wav, --vocode-dir or --synth-phn-dir --gen-wav write; it needs one of them')
    elif paras.loudness_wav_dir is None and any(v is not None for v in (paras.loudness_target, paras.loudness_peak, paras.loudness_max_gain)):
        parser.error('--loudness-target, --loudness-peak and --loudness-max-gain set --normalize-loudness or --loudness-wav-dir; they need one of them')
    paras.loudness_target = -23.0 if paras.loudness_target is None else paras.loudness_target
    paras.loudness_peak = -1.0 if paras.loudness_peak is None else paras.loudness_peak
    paras.loudness_max_gain = 30.0 if paras.loudness_max_gain is None else paras.loudness_max_gain
    if not -70.0 <= paras.loudness_target <= 0.0:
        parser.error('--loudness-target must lie in [-70, 0] LUFS')
    if not float('-inf') < paras.loudness_peak <= 0.0:
        parser.error('--loudness-peak must be finite and at most 0 dBFS')
    if not 0.0 <= paras.loudness_max_gain < float('inf'):
        parser.error('--loudness-max-gain must be finite and at least 0 dB')
    if paras.score_phn_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'trim_silence', 'corpus'):
            if getattr(paras, flag):
                parser.error('--score-phn-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches != 0:
            parser.error('--score-phn-dir does not combine with --dev-batches')
        if paras.score_ref_dir is None:
            parser.error('--score-phn-dir needs --score-ref-dir DIR (the reference transcripts)')
        try:
            paras.score_ignore = tuple(int(t) for t in (paras.score_ignore if paras.score_ignore is not None else '0,1,2').split(',') if t.strip())
        except ValueError:
            parser.error('--score-ignore takes comma-separated integer ids (got %r)' % paras.score_ignore)
        if len(paras.score_ignore) > 64 or any(not 0 <= t < 2 ** 31 for t in paras.score_ignore):
            parser.error('--score-ignore takes at most 64 ids in [0, 2^31)')
    elif paras.score_ref_dir is not None or paras.score_ignore is not None or paras.score_nbest or paras.score_ali:
        parser.error('--score-ref-dir, --score-ignore, --score-nbest and --score-ali belong to --score-phn-dir; they need that flag')
    abx_flags = ('abx_wav_dir', 'abx_feat', 'abx_metric', 'abx_context', 'abx_spk_map', 'abx_ignore', 'abx_max_items', 'abx_min_frames')
    if paras.abx_ali_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'loudness_wav_dir', 'score_phn_dir', 'corpus'):
            if getattr(paras, flag):
                parser.error('--abx-ali-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches != 0:
            parser.error('--abx-ali-dir does not combine with --dev-batches')
        if paras.config is None or paras.abx_wav_dir is None:
            parser.error('--abx-ali-dir needs --config (its data.audio and model) and --abx-wav-dir DIR (the waveforms)')
        paras.abx_feat = paras.abx_feat or 'mfcc'
        paras.abx_metric = paras.abx_metric or ('kl' if paras.abx_feat == 'code' else 'angular')
        paras.abx_context = paras.abx_context or 'triphone'
        paras.abx_ignore = tuple(s.strip() for s in (paras.abx_ignore or '').split(',') if s.strip())
        paras.abx_max_items = 50 if paras.abx_max_items is None else paras.abx_max_items
        paras.abx_min_frames = 1 if paras.abx_min_frames is None else paras.abx_min_frames
        if paras.abx_max_items < 2 or not 1 <= paras.abx_min_frames <= 64:
            parser.error('--abx-max-items must be >= 2 and --abx-min-frames in [1, 64]')
        if paras.abx_max_gb is not None and (paras.abx_mode in (None, 'within') or not 0.0 < paras.abx_max_gb < float('inf')):
            parser.error('--abx-max-gb takes a positive number of GiB and belongs to --abx-mode across or both')
        paras.abx_mode = paras.abx_mode or 'within'
        paras.abx_max_gb = 8.0 if paras.abx_max_gb is None else paras.abx_max_gb
        if paras.abx_mode != 'within' and paras.abx_spk_map is None:
            parser.error('--abx-mode %s takes X from another speaker: it needs --abx-spk-map FILE (key,speaker) with at least two speakers' % paras.abx_mode)
    elif paras.abx_mode is not None or paras.abx_max_gb is not None:
        parser.error('--abx-mode and --abx-max-gb belong to --abx-ali-dir; they need that flag')
    elif any(getattr(paras, f) is not None for f in abx_flags):
        parser.error('--abx-wav-dir, --abx-feat, --abx-metric, --abx-context, --abx-spk-map, --abx-ignore, --abx-max-items and --abx-min-frames belong to '
                     '--abx-ali-dir; they need that flag')
    elif paras.abx_codebook is not None:
        parser.error('--abx-codebook belongs to --abx-ali-dir; it needs that flag')
    if paras.abx_codebook is not None and paras.abx_ali_dir is not None and paras.abx_feat == 'code':
        parser.error('--abx-codebook quantises feature rows; it does not combine with --abx-feat code')
    unit_tools = [f for f in ('kmeans_wav_dir', 'units_wav_dir') if getattr(paras, f) is not None]
    for tool in unit_tools:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir', 'build_lm_phn_dir', 'vocode_dir',
                     'resample_wav_dir', 'feat_wav_dir', 'mcd_wav_dir', 'synth_phn_dir', 'trim_wav_dir', 'loudness_wav_dir', 'score_phn_dir',
                     'stoi_wav_dir', 'abx_ali_dir', 'corpus') + (('units_wav_dir',) if tool == 'kmeans_wav_dir' else ()):
            if getattr(paras, flag):
                parser.error('--%s does not combine with --%s' % (tool.replace('_', '-'), flag.replace('_', '-')))
        if paras.dev_batches > 0:
            parser.error('--%s does not combine with --dev-batches' % tool.replace('_', '-'))
    kmeans_flags = ('kmeans_out', 'kmeans_k', 'kmeans_iters', 'kmeans_tol', 'kmeans_init', 'kmeans_restarts', 'kmeans_max_gb')
    if paras.kmeans_wav_dir is not None:
        if paras.config is None or paras.kmeans_out is None:
            parser.error('--kmeans-wav-dir needs --config (its data.audio and model) and --kmeans-out FILE.npy (the codebook to write)')
        paras.kmeans_k = 50 if paras.kmeans_k is None else paras.kmeans_k
        paras.kmeans_iters = 100 if paras.kmeans_iters is None else paras.kmeans_iters
        paras.kmeans_tol = 1e-4 if paras.kmeans_tol is None else paras.kmeans_tol
        paras.kmeans_restarts = 1 if paras.kmeans_restarts is None else paras.kmeans_restarts
        paras.kmeans_max_gb = 8.0 if paras.kmeans_max_gb is None else paras.kmeans_max_gb
        if not 1 <= paras.kmeans_k <= 4096 or paras.kmeans_iters < 1 or paras.kmeans_restarts < 1:
            parser.error('--kmeans-k must lie in [1, 4096], --kmeans-iters and --kmeans-restarts must be >= 1')
        if not 0.0 <= paras.kmeans_tol < float('inf') or not 0.0 < paras.kmeans_max_gb < float('inf'):
            parser.error('--kmeans-tol must be finite and >= 0, --kmeans-max-gb a positive number of GiB')
    elif any(getattr(paras, f) is not None for f in kmeans_flags):
        parser.error('--kmeans-out, --kmeans-k, --kmeans-iters, --kmeans-tol, --kmeans-init, --kmeans-restarts and --kmeans-max-gb belong to '
                     '--kmeans-wav-dir; they need that flag')
    if paras.units_wav_dir is not None:
        if paras.config is None or paras.units_codebook is None:
            parser.error('--units-wav-dir needs --config (its data.audio and model) and --units-codebook FILE.npy (the table of --kmeans-out)')
    elif paras.units_codebook is not None or paras.units_frames:
        parser.error('--units-codebook and --units-frames belong to --units-wav-dir; they need that flag')
    if paras.kmeans_feat is not None and not unit_tools:
        parser.error('--kmeans-feat belongs to --kmeans-wav-dir or --units-wav-dir; it needs one of them')
    if paras.gen_wav_feat != 'linear' and not ((paras.gen_specgram or paras.synth_phn_dir is not None) and paras.gen_wav):
        parser.error('--gen-wav-feat chooses what --gen-specgram --gen-wav vocodes; it needs both flags')
    if paras.build_lm_phn_dir is not None:
        for flag in ('gen_specgram', 'tts_only', 'unpair_wav_dir', 'transcribe_wav_dir', 'align_wav_dir'):
            if getattr(paras, flag):
                parser.error('--build-lm-phn-dir does not combine with --%s' % flag.replace('_', '-'))
        if paras.dev_batches > 0:
            parser.error('--build-lm-phn-dir does not combine with --dev-batches')
        if paras.lm is None or paras.lm_order is None:
            parser.error('--build-lm-phn-dir needs --lm FILE (the table to write) and --lm-order N')
        if not 1 <= paras.lm_order <= 4:
            parser.error('--build-lm-phn-dir needs 1 <= --lm-order <= 4')
        paras.lm_classes = 43 if paras.lm_classes is None else paras.lm_classes
        if paras.lm_classes < 2 or paras.lm_classes ** paras.lm_order > 2 ** 26:
            parser.error('--lm-classes must be >= 2 with --lm-classes ^ --lm-order <= 2^26')
        if paras.lm_smooth is not None and not (0.0 <= paras.lm_smooth < float('inf')):
            parser.error('--lm-smooth must be finite and >= 0')
        if paras.lm_weight is not None or paras.ins_bonus is not None:
            parser.error('--lm-weight and --ins-bonus belong to --transcribe-wav-dir --lm; --build-lm-phn-dir writes probabilities')
    else:
        if paras.lm_order is not None or paras.lm_smooth is not None:
            parser.error('--lm-order and --lm-smooth belong to --build-lm-phn-dir; they need that flag')
        if paras.lm_classes is not None:
            parser.error('--lm-classes belongs to --build-lm-phn-dir; it needs that flag')
        if paras.lm is not None and paras.transcribe_wav_dir is None:
            parser.error('--lm names the n-gram table of --transcribe-wav-dir or --build-lm-phn-dir; it needs one of them')
        if paras.lm is None and (paras.lm_weight is not None or paras.ins_bonus is not None):
            parser.error('--lm-weight and --ins-bonus weight the table of --lm; they need that flag')
        for flag in ('lm_weight', 'ins_bonus'):
            v = getattr(paras, flag)
            if v is not None and not float('-inf') < v < float('inf'):
                parser.error('--%s must be finite' % flag.replace('_', '-'))
    if paras.lm_weight is None:
        paras.lm_weight = 0.5
    if paras.ins_bonus is None:
        paras.ins_bonus = 0.0
    if paras.lm_smooth is None:
        paras.lm_smooth = 1.0
    if paras.verbose:
        for flag in IGNORED_FLAGS:
            if flag == 'gen_wav' and (paras.gen_specgram or paras.synth_phn_dir is not None):
                continue             # read by gen_specgram (bin/gen_specgram.py:114-126), as in the reference, and by --synth-phn-dir
            if flag == 'store_best_per' and paras.dev_batches != 0:
                continue             # read by VqvaeTrainer.validate (bin/train_vqvae.py:376-382)
            if getattr(paras, flag):
                print('[INFO] --%s accepted for compatibility; it has no effect on this path' % flag.replace('_', '-'))
    return paras


# (attribute of paras, class of semi_tts_amd.solver): the modes that do not train; the first one whose flag is given runs
TOOLS = (('resample_wav_dir', 'Resampler'), ('trim_wav_dir', 'Trimmer'), ('loudness_wav_dir', 'LoudnessWriter'), ('vocode_dir', 'Vocoder'),
         ('feat_wav_dir', 'FeatureWriter'), ('mcd_wav_dir', 'McdScorer'), ('stoi_wav_dir', 'StoiScorer'), ('abx_ali_dir', 'AbxScorer'),
         ('kmeans_wav_dir', 'KMeansTrainer'), ('units_wav_dir', 'UnitWriter'),
         ('score_phn_dir', 'PhnScorer'), ('synth_phn_dir', 'Synthesiser'), ('transcribe_wav_dir', 'Transcriber'), ('align_wav_dir', 'Aligner'),
         ('gen_specgram', 'SpecgramGenerator'))


def main(argv=None):
    paras = parse_args(argv)
    if paras.build_lm_phn_dir is not None:                  # host only: no config, no seed, no device
        from semi_tts_amd.ngram import build_lm_from_phn_dir
        from semi_tts_amd.solver import read_vocab
        print(build_lm_from_phn_dir(paras.build_lm_phn_dir, paras.lm, paras.lm_order, V=paras.lm_classes, smooth=paras.lm_smooth,
                                    vocab=read_vocab(paras.vocab) if paras.vocab else None)['summary'])
        return
    if paras.resample_wav_dir is not None and paras.config is None:      # (the rate was given: this mode reads nothing else of a config)
        config = None
        paras.batch_size = paras.batch_size or 8
    elif paras.score_phn_dir is not None:                                # (transcripts against transcripts: no config is read)
        config = None
        paras.batch_size = paras.batch_size or 64
    elif paras.stoi_wav_dir is not None:                                 # (waveforms against waveforms at their own rates: no config is read)
        config = None
        paras.batch_size = paras.batch_size or 32
    else:
        config = yaml.load(open(paras.config, 'r'), Loader=yaml.FullLoader)
    if paras.batch_size is None:
        paras.batch_size = config['data']['corpus'].get('batch_size', 8)
    random.seed(paras.seed)
    np.random.seed(paras.seed)
    torch.manual_seed(paras.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(paras.seed)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:      # one process per GPU (torch.distributed.run), RCCL over xGMI
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl')
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    tool = next((name for flag, name in TOOLS if getattr(paras, flag) not in (None, False)), None)
    if tool is not None:
        import semi_tts_amd.solver
        Solver, mode = getattr(semi_tts_amd.solver, tool), 'test'
    elif paras.tts_only:
        from semi_tts_amd.solver import TtsTrainer as Solver
        mode = 'train'
    else:                                                    # ref: main.py:61-63
        from semi_tts_amd.solver import VqvaeTrainer as Solver
        mode = 'train'
    solver = Solver(config, paras, mode)
    solver.load_data()
    solver.set_model()
    solver.exec()


if __name__ == '__main__':
    main()
