"""Shared helpers for the parity tests (test infrastructure; may import the oracle)."""
import json
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(REPO, 'gpurun_out', 'parity_report.jsonl')


def report(test, **vals):
    """append one line of measured errors to gpurun_out/parity_report.jsonl (best effort)"""
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, 'a') as f:
            f.write(json.dumps(dict(test=test, **{k: (float(v) if not isinstance(v, (str, int)) else v)
                                                   for k, v in vals.items()})) + '\n')
    except OSError:
        pass


U = 2.0 ** -24          # float32 unit roundoff
SENTINEL = -12345.6789


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """float32 tensor as its bit pattern (bitwise comparison that also holds for NaN)"""
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guarded(rows, cols, ld, dev, pad_rows=2, off=3, fill=SENTINEL):
    """(buffer, view): a (rows, cols) view with leading dimension ld inside a buffer filled with `fill` (a sentinel, or NaN so that a
    read outside the view poisons the result) with guard rows above and below and guard columns left (off) and right (ld - off - cols)"""
    assert ld >= cols + off
    buf = torch.full((rows + 2 * pad_rows, ld), fill, device=dev)
    return buf, buf[pad_rows:pad_rows + rows, off:off + cols]


def guard_ok(buf, view_mask_fn, fill=SENTINEL):
    """every element of buf outside the view still holds the fill value, bit for bit"""
    keep = view_mask_fn(torch.zeros(buf.shape, dtype=torch.bool))
    return bool((bits(buf)[~keep] == bits(torch.tensor([fill], dtype=torch.float32))[0]).all())


def inside(rows, cols, pad_rows=2, off=3):
    def f(m):
        m[pad_rows:pad_rows + rows, off:off + cols] = True
        return m
    return f


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


FWD_ATTN = ('whole', 'pre_fin', 'fin_split', 'pq_fin', 'pq_rng')      # bits 0..2 of an st_decoder_fwd_forms word
FWD_PROD = ('none', 'own', 'pq_fin', 'pq_pre')                        # bits 4..5


def fwd_forms(word):
    """(attention form, host of the decoder cell's partial gate product, flags) of an st_decoder_fwd_forms word
    (Decoder._last_fwd_forms); flags is a subset of {'tf', 'defer', 'pre_in_pq', 'pair'}"""
    assert word is not None and word >= 0, word
    flags = {n for b, n in ((8, 'tf'), (9, 'defer'), (10, 'pre_in_pq'), (11, 'pair')) if word >> b & 1}
    return FWD_ATTN[word & 7], FWD_PROD[(word >> 4) & 3], flags


def coin_source(coins):
    it = iter(np.asarray(coins, dtype=np.float64).tolist())
    return lambda: next(it)


def split_masks(masks, hp, training, tf_rate, B, Bt, steps, step_src, P):
    """Re-arrange dropout masks recorded from the reference (in its draw order) into the
    explicit-mask dict the HIP Decoder accepts.  Draw order (src/module.py): teacher prenet
    (2), go-frame prenet (2), then per step: query dropout, decoder dropout (training only),
    prenet of the own output (2; all rows, or only the rows without a teacher)."""
    it = iter(masks)
    out = {}
    if training and hp.get('enc_dropout', 0.0) > 0:      # the encoder's conv blocks come first, (B, C, L) in the reference
        out['enc'] = [next(it).transpose(1, 2).contiguous() for _ in range(hp.get('enc_n_conv', 3))]
    pd = hp['prenet_dropout'] > 0
    if tf_rate != 0.0 and pd:
        out['teacher'] = [next(it), next(it)]
    if pd and hp.get('prenet_norm_type'):
        out['go'] = [next(it), next(it)]         # a normalised prenet maps the zero go frame to relu(beta ...): the masks matter
    elif pd:
        next(it), next(it)                       # go frame: prenet(0) == 0 whatever the mask
    own = torch.ones(steps, 2, B, P)
    q, d = [], []
    for t in range(steps):
        if training and hp['query_dropout'] > 0:
            q.append(next(it))
        if training and hp['dec_dropout'] > 0:
            d.append(next(it))
        if pd:
            if step_src[t] == -1:
                own[t, 0], own[t, 1] = next(it), next(it)
            elif Bt < B:
                own[t, 0, Bt:], own[t, 1, Bt:] = next(it), next(it)
    rest = list(it)
    assert not rest, 'unconsumed reference dropout masks: %d' % len(rest)
    if pd:
        out['own'] = own
    if q:
        out['q'] = torch.stack(q)
    if d:
        out['d'] = torch.stack(d)
    return out


def decoder_fp64_reference(W, memory, teacher, spk, hp, tf_rate=0.0, unpair_max_frame=None, training=False, seed=11, grad=False):
    """oracle.tts_oracle.decoder_forward in float64 on float64 copies of the weights `W` ('decoder.'-prefixed) and inputs.  The dropout
    masks are drawn in float32 from a generator seeded with `seed` and kept in draw order, so that split_masks can replay them through
    the HIP path (and DropoutSource('list', ...) through a float32 run of the oracle).  `teacher`: an int (free running) or a tensor;
    hp: the decoder section plus n_mels.  grad=True makes the float64 weights, memory and speaker embedding leaves that require grad.
    Returns (outs, masks, Wd, memory64, spk64) with outs = (mel, alignment, stop)."""
    from oracle import tts_oracle as O

    class Drop64(O.DropoutSource):
        def __call__(self, x, p, training):
            if (not training) or p == 0.0:
                return x
            keep = torch.full(x.shape, 1.0 - p, dtype=torch.float32)
            mk = torch.bernoulli(keep, generator=self.gen) / (1.0 - p)
            self.used.append(mk)
            return x * mk.double()

    torch.set_default_dtype(torch.float64)       # the oracle creates its zero states in the default dtype
    try:
        Wd = {k: v.double().requires_grad_(grad) for k, v in W.items()}
        mem_r, spk_r = memory.double().requires_grad_(grad), spk.double().requires_grad_(grad)
        drop = Drop64('rng', generator=torch.Generator().manual_seed(seed))
        with torch.set_grad_enabled(grad):
            outs = O.decoder_forward(Wd, mem_r, teacher if isinstance(teacher, int) else teacher.double(), spk_r, hp, tf_rate,
                                     unpair_max_frame, training, drop, lambda: 0.0)
    finally:
        torch.set_default_dtype(torch.float32)
    return outs, drop.used, Wd, mem_r, spk_r


def masks_to(masks, device):
    out = {}
    for k, v in masks.items():
        out[k] = [m.to(device).contiguous() for m in v] if isinstance(v, list) else v.to(device).contiguous()
    return out


def tiny_tacotron(meta, weights, device):
    """build the HIP Tacotron2 with the tiny fixture configuration and load the reference weights"""
    from semi_tts_amd.tts import Tacotron2
    cfg = meta['cfg']
    paras = json.loads(json.dumps(cfg['paras']))
    m = Tacotron2(cfg['n_mels'], cfg['linear_dim'], cfg['in_embed_dim'], cfg['spkr_embed_dim'], paras)
    m.load_state_dict(weights)
    return m.to(device)


FULL_CFG = {
    'encoder': dict(enc_n_conv=3, enc_kernel_size=5, enc_rnn_layer=1, enc_embed_dim=512, enc_dropout=0.0),
    'decoder': dict(n_frames_per_step=3, prenet_dim=256, prenet_dropout=0.5, query_rnn_dim=1024, dec_rnn_dim=1024,
                    query_dropout=0.1, dec_dropout=0.1, attn_dim=256, n_location_filters=32,
                    location_kernel_size=31, loc_aware=True, use_summed_weights=True, drop_dec_in=0.0),
    'separate_postnet': True,
}


def full_tacotron(device, seed=1234, prenet_dropout=0.0):
    """full-size Tacotron2 (the `model.decoder` section of the shipped YAMLs) with synthetic weights"""
    from semi_tts_amd.tts import Tacotron2
    from semi_tts_amd.synthetic import load_synthetic
    cfg = json.loads(json.dumps(FULL_CFG))
    cfg['decoder']['prenet_dropout'] = prenet_dropout
    m = Tacotron2(80, 1025, 64, 128, cfg)
    load_synthetic(m, seed)
    return m.to(device).eval()


def full_hp(prenet_dropout=0.0):
    hp = dict(FULL_CFG['decoder'])
    hp['prenet_dropout'] = prenet_dropout
    hp['n_mels'] = 80
    hp['enc_dropout'] = 0.0
    return hp


def tiny_vqvae(meta, weights, device, strict=False):
    """HIP VQVAE for the H1 fixture: the phoneme-attribute table comes from the fixture (data), not from a file"""
    from semi_tts_amd.vqvae import VQVAE
    cfg = json.loads(json.dumps(meta['model']))
    proj = cfg['codebook'].get('proj_attr')
    cfg['codebook']['proj_attr'] = None
    m = VQVAE(meta['audio']['num_mels'], meta['audio']['num_freq'], meta['vocab_size'], meta['n_spkr'], **cfg)
    if 'codebook.phn_attr.weight' in weights:
        cb = m.codebook
        attr = weights['codebook.phn_attr.weight']
        cb.use_phn_attr = True
        cb.phn_attr = torch.nn.Embedding.from_pretrained(attr.clone(), freeze=True, padding_idx=0)
        cb.proj_attr = torch.nn.Linear(attr.shape[1], proj)
        cb.learnable_table = torch.nn.Parameter(torch.zeros(meta['vocab_size'], cfg['codebook']['latent_dim'] - proj))
    missing = m.load_state_dict(weights, strict=False)
    assert not [k for k in missing.missing_keys if not (k.startswith('asr.') and not strict)], missing.missing_keys
    assert not (strict and missing.unexpected_keys), missing.unexpected_keys
    return m.to(device)
