"""Every forward form of the decode loop (st_decoder_forward) on the GPU at small decoder sizes, against float64.
Needs a real MI355X: pytest -m gpu

The cases are decoder_fwd_cases.CASES; tests/test_decoder_fwd_forms_host.py proves on the host that they reach every attention form,
every host of the decoder cell's partial gate product, 1 / 2 / 4 / 8 fin parts, every flag and several cuts of the cell's reduction.
Here each case runs through a fresh `Decoder` with the case's knobs, and

  * the loop must have taken the forms the table names (Decoder._last_fwd_forms): a case that quietly took another form fails;
  * mel, alignment and stop are compared with oracle.tts_oracle.decoder_forward in float64 on the same weights, inputs and dropout
    masks (drawn by the oracle, replayed through `_masks`).  The yardstick is the same oracle in float32 on the CPU against its float64
    self: |hip - fp64|max <= BOUND_FACTOR * max(|cpu fp32 - fp64|max, YARD_FLOOR) for each output -- the factor and the floor of
    test_c2_with_scaled_recurrent_weights, near 8e-6 at these sizes;
  * every output is finite, a second run is bit-identical, and for a batch that does not fill its tiles of 16 rows the same rows in
    reversed order give the same results row by row within the same bound (padding rows and lanes cannot hide an error);
  * the pairs the project states to be bit-identical are: the cell's partial product beside pq + fin against a launch of its own;
  * the training loop hands its kernels buffers nobody has zeroed (ops.uninit: the step tapes of an unpadded batch, S and the location
    features of every step): with those filled with NaN first the outputs are bitwise the same -- nothing reads what nobody wrote.

Training cases compare the forward only (the gradients of these forms: test_gpu_attn_bwd.py), run through the differentiable path so
that the deferred projection and the paired cells are really taken.
"""
import pytest
import torch

import decoder_fwd_cases as FC
from helpers import decoder_fp64_reference, fwd_forms, masks_to, maxdiff, report, split_masks

pytestmark = pytest.mark.gpu

BOUND_FACTOR = 8        # x the CPU float32 oracle's own error: head-room for another summation order (each case's ratio: parity_report.jsonl)
YARD_FLOOR = 1e-6
OUTS = ('mel', 'align', 'stop')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def hp_of(c):
    d = FC.DIMS[c['dims']]
    # prenet dropout 0.5: the own-output mask path is live in the free-running and partial cases; query / decoder dropout act in training
    return dict(n_frames_per_step=FC.COMMON['r'], prenet_dim=d['P'], prenet_dropout=0.5, query_rnn_dim=d['Q'], dec_rnn_dim=d['D'],
                query_dropout=0.1, dec_dropout=0.1, attn_dim=d['A'], n_location_filters=FC.COMMON['F'],
                location_kernel_size=FC.COMMON['K'], loc_aware=True, use_summed_weights=True, drop_dec_in=0.0)


def new_decoder(c):
    from semi_tts_amd.module import Decoder
    return Decoder(FC.COMMON['n_mels'], enc_embed_dim=FC.DIMS[c['dims']]['E'], spkr_embed_dim=FC.COMMON['S'], **hp_of(c))


_WEIGHTS, _REFS, _RUNS = {}, {}, {}


def weights_of(c):
    """Decoder's own initialisation under a fixed seed, once per dims set and gain (the two LSTM cells' weights x gain)"""
    key = (c['dims'], c['gain'])
    if key not in _WEIGHTS:
        torch.manual_seed(5)
        dec = new_decoder(c)
        with torch.no_grad():
            for cell in (dec.query_rnn, dec.dec_rnn):
                cell.weight_ih.mul_(c['gain'])
                cell.weight_hh.mul_(c['gain'])
        _WEIGHTS[key] = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    return _WEIGHTS[key]


def reference_of(c):
    """inputs, the oracle's masks, its float64 outputs and the float32 yardstick of a case: computed once, shared by the cases that
    differ in knobs only, never modified"""
    from oracle import tts_oracle as O
    from semi_tts_amd.module import plan_decode
    key = tuple(c[k] for k in ('dims', 'B', 'L', 'steps', 'mode', 'Bt', 'gain'))
    if key in _REFS:
        return _REFS[key]
    B, L, r, n_mels = c['B'], c['L'], FC.COMMON['r'], FC.COMMON['n_mels']
    training, steps, src, Bt, Tt = FC.step_plan(c)
    g = torch.Generator().manual_seed(1000 * B + L)
    memory = torch.randn(B, L, FC.DIMS[c['dims']]['E'], generator=g)
    spk = torch.randn(B, FC.COMMON['S'], generator=g)
    free = c['mode'] == 'free'
    teacher = steps * r if free else torch.rand(Bt, Tt * r, n_mels, generator=g)
    tf_rate = 0.0 if free else 1.0
    unpair = steps * r if c['Bt'] is not None else None
    # the step plan the table's host half assumed is the one Decoder.forward makes
    assert plan_decode(free, teacher if free else Tt * r, Bt, B, r, tf_rate, 0.0, unpair, lambda: 0.0) == (steps, src)
    hpo = dict(hp_of(c), n_mels=n_mels)
    W = {'decoder.' + k: v for k, v in weights_of(c).items()}
    outs, used, *_ = decoder_fp64_reference(W, memory, teacher, spk, hpo, tf_rate, unpair, training, seed=11)
    with torch.no_grad():
        outs32 = O.decoder_forward(W, memory, teacher, spk, hpo, tf_rate, unpair, training, O.DropoutSource('list', masks=used), lambda: 0.0)
    assert all(o.dtype == torch.float64 for o in outs) and all(o.dtype == torch.float32 for o in outs32)
    masks = split_masks(used, hpo, training, tf_rate, B, Bt, steps, src, hpo['prenet_dim'])
    ref = dict(memory=memory, spk=spk, teacher=teacher, tf_rate=tf_rate, unpair=unpair, training=training, masks=masks,
               out=dict(zip(OUTS, outs)), yard={n: maxdiff(a, b) for n, a, b in zip(OUTS, outs32, outs)})
    ref['bound'] = {n: BOUND_FACTOR * max(y, YARD_FLOOR) for n, y in ref['yard'].items()}
    _REFS[key] = ref
    return ref


def flip_masks(masks):
    """the masks of the batch in reversed row order"""
    dim = dict(teacher=0, own=2, q=1, d=1)
    return {k: [m.flip(dim[k]) for m in v] if isinstance(v, list) else v.flip(dim[k]) for k, v in masks.items()}


def run_hip(c, ref, dev, reverse=False):
    """the case through a fresh Decoder (knob changes and a degraded hand-off cannot leak into another case); returns the three outputs
    (in the case's own row order) and the planner's word of the loop that ran"""
    dec = new_decoder(c)
    dec.load_state_dict(weights_of(c))
    dec = dec.to(dev)
    dec.train(ref['training'])
    for k, v in FC.knobs_of(c).items():
        assert hasattr(dec, k), k
        setattr(dec, k, v)
    order = (lambda t: t.flip(0)) if reverse else (lambda t: t)
    masks = masks_to(flip_masks(ref['masks']) if reverse else ref['masks'], dev)
    teacher = ref['teacher'] if isinstance(ref['teacher'], int) else order(ref['teacher']).to(dev)
    with torch.set_grad_enabled(ref['training']):      # training: the differentiable path (tapes kept, projection deferred)
        outs = dec(order(ref['memory']).to(dev), None, teacher, order(ref['spk']).to(dev), tf_rate=ref['tf_rate'],
                   unpair_max_frame=ref['unpair'], _masks=masks)
    if ref['training']:
        assert all(o.grad_fn is not None for o in outs[::2])
    torch.cuda.synchronize()
    return {n: order(o.detach()) for n, o in zip(OUTS, outs)}, dec._last_fwd_forms


def first_run(c, dev):
    """(outputs, word) of the case's first run, kept for the bit-identity pairs"""
    if c['id'] not in _RUNS:
        _RUNS[c['id']] = run_hip(c, reference_of(c), dev)
    return _RUNS[c['id']]


@pytest.mark.parametrize('c', FC.CASES, ids=FC.IDS)
def test_form_against_float64(dev, c):
    ref = reference_of(c)
    got, word = first_run(c, dev)
    assert (fwd_forms(word), (word >> 12) & 15, word >> 16) == (c['want'], c['fp'], c['k0']), hex(word)
    B, L, steps, r = c['B'], c['L'], c['steps'], FC.COMMON['r']
    assert got['mel'].shape == (B, steps * r, FC.COMMON['n_mels']) and got['align'].shape == (B, steps, L) and got['stop'].shape == (B, steps * r)
    errs = {n: maxdiff(got[n], ref['out'][n]) for n in OUTS}
    ratio = max(errs[n] / ref['bound'][n] * BOUND_FACTOR for n in OUTS)
    report('decoder_fwd_form', case=c['id'], forms='%s/%s' % c['want'][:2], ratio=ratio, **errs, **{'yard_' + n: ref['yard'][n] for n in OUTS})
    print(c['id'], errs, ref['yard'], 'ratio %.3g' % ratio)
    for n in OUTS:
        assert bool(torch.isfinite(got[n]).all()), n
        assert errs[n] <= ref['bound'][n], (n, errs[n], ref['yard'][n])
    again, word2 = run_hip(c, ref, dev)
    assert word2 == word
    for n in OUTS:
        assert torch.equal(again[n], got[n]), n
    if B % 16 != 0 and B > 1 and c['Bt'] is None:
        # the same rows at other batch positions (row b at B - 1 - b: other lanes of the 16-row tiles, the padding rows elsewhere)
        flipped, word3 = run_hip(c, ref, dev, reverse=True)
        assert word3 == word
        for n in OUTS:
            assert bool(torch.isfinite(flipped[n]).all()), n
            e = maxdiff(flipped[n], ref['out'][n])
            assert e <= ref['bound'][n], (n, 'reversed rows', e, ref['yard'][n])
            assert maxdiff(flipped[n], got[n]) <= ref['bound'][n], (n, 'reversed rows against the first run')


@pytest.mark.parametrize('a,b', FC.BIT_IDENTICAL, ids=['%s-%s' % p for p in FC.BIT_IDENTICAL])
def test_hosted_product_is_bitwise_the_launch_of_its_own(dev, a, b):
    """the cell's partial gate product beside pq + fin (pq_fin / pq_fin) and as a launch of its own behind the two-launch attention step
    (pre_fin / own), at the same cut: the same arithmetic, so the same bits"""
    (ga, wa), (gb, wb) = first_run(FC.BY_ID[a], dev), first_run(FC.BY_ID[b], dev)
    assert fwd_forms(wa)[:2] == ('pq_fin', 'pq_fin') and fwd_forms(wb)[:2] == ('pre_fin', 'own') and wa >> 16 == wb >> 16
    for n in OUTS:
        assert torch.equal(ga[n], gb[n]), n


UNINIT = ['M16_train_b32_l11', 'M16_train_b32_l130', 'MID_train_b32_l11', 'M16_train_b20_l11', 'M16_train_unpaired', 'M16_train_whole']


@pytest.mark.parametrize('name', UNINIT)
def test_training_forms_read_nothing_unwritten(dev, name):
    """B = 32 at M16 / MID pads nothing, so the teacher-forced training loop takes its step tapes without a fill (and S and the location
    features of every step in any case).  With every such buffer NaN first (ops.POISON_UNINIT) the forward is bitwise the clean one.  The
    hosted product of these sizes reduces 7 or 11 k-blocks: its waves issue loads past that range, which must come back as zeros for the
    activations too -- what lies behind them in the tape is the context of the second batch tile, not yet written at that point."""
    from semi_tts_amd import ops
    c = FC.BY_ID[name]
    got, word = first_run(c, dev)
    old = ops.POISON_UNINIT
    ops.POISON_UNINIT = True
    try:
        poisoned, word2 = run_hip(c, reference_of(c), dev)
    finally:
        ops.POISON_UNINIT = old
    assert word2 == word
    for n in OUTS:
        assert bool(torch.isfinite(poisoned[n]).all()), n
        assert torch.equal(poisoned[n], got[n]), n
