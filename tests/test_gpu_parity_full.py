"""Full-size parity of the HIP path in the configurations that are actually benchmarked and shipped
(round-2 additions; needs a real MI355X: pytest -m gpu):

  * the `Postnet` class on device against the reference-recorded fixture;
  * BASELINE config 5: the whole 355-step free-running trajectory (B=64, L=171) against the oracle,
    with the per-step error curve written to gpurun_out/parity_report.jsonl;
  * BASELINE config 2 exactly as bench.py times it: hipGraph replay of the decode loop, prenet dropout 0.5
    with the ORACLE's masks replayed through GraphedDecoder.own_mask, prenet layer 1 fused into the
    projection launch;
  * one C2-size training step (B=32, 258 frames, L=43): loss, global gradient norm and every parameter
    gradient against CPU autograd through the oracle;
  * C2 with the recurrent weights scaled x2.5 (non-contractive dynamics: fp32-vs-fp64 CPU error grows to
    1e-5 over 86 steps) to see real error accumulation instead of summation-order noise.

Tolerances: north star = 1e-3 max-abs on mel; the measured values are reported and much smaller.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, REPO
from helpers import full_hp, full_tacotron, fwd_forms, masks_to, maxdiff, report, split_masks

pytestmark = pytest.mark.gpu

from oracle import tts_oracle as O   # noqa: E402
from oracle import vq_oracle as VQ   # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a GPU'
    from semi_tts_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _weights(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def _step_curve(a, b, steps):
    """max-abs difference per decode step of two (B, steps*r, n_mels) tensors"""
    d = (a.detach().cpu().double() - b.detach().cpu().double()).abs()
    return d.view(d.shape[0], steps, -1).amax(dim=(0, 2))


# ------------------------------------------------------------------------------------ a14
def test_postnet_class_against_reference_golden(dev):
    """The 5-conv `Postnet` class (src/module.py:53-82; constructed by no config) on the HIP path against what
    the real reference produced for the same weights and input (eval mode: BatchNorm folded into the conv)."""
    from semi_tts_amd.module import Postnet
    W, A, _ = load_golden('conv_postnet_tiny')
    m = Postnet(8, 16, 5, 5, 0.0)
    m.load_state_dict(W)
    m = m.to(dev).eval()
    with torch.no_grad():
        y = m(A['x'].to(dev))
    err = maxdiff(y, A['y'])
    report('postnet_class', err=err)
    assert y.shape == A['y'].shape and err < 1e-5
    # ragged shape against the oracle: T not a multiple of the tile, B = 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 37, 8, generator=g)
    with torch.no_grad():
        y2 = m(x.to(dev))
    assert maxdiff(y2, O.conv_postnet_forward(W, x)) < 1e-5


# ------------------------------------------------------------------------------------ C5, whole trajectory
def test_long_form_c5_full_trajectory_against_oracle(dev):
    """BASELINE config 5 (B=64, L=171, (1026+40)//3 = 355 decode steps), free running, prenet dropout 0:
    the whole trajectory against the oracle -- the case where a per-step error could accumulate."""
    from semi_tts_amd.synthetic import synthetic_batch
    m = full_tacotron(dev, seed=5)
    B, L, T = 64, 171, 1066
    steps = T // 3
    txt, spk, _ = synthetic_batch(B, L, 3, seed=9)
    txt, spk = torch.from_numpy(txt), torch.from_numpy(spk)
    with torch.no_grad():
        mem = m.encoder(txt.to(dev), None)
        mel, align, stop = m.decoder(mem, None, T, spk.to(dev), tf_rate=0.0)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        mel_r, al_r, st_r = O.decoder_forward(_weights(m), mem.cpu(), T, spk, full_hp(0.0))
    curve = _step_curve(mel, mel_r, steps)
    errs = dict(mel=maxdiff(mel, mel_r), align=maxdiff(align, al_r), stop=maxdiff(stop, st_r))
    report('c5_full_trajectory', steps=steps, mel_first=float(curve[0]), mel_mid=float(curve[steps // 2]),
           mel_last=float(curve[-1]), curve_every_25=json.dumps([float('%.2e' % v) for v in curve[::25]]), **errs)
    assert mel.shape == (B, 1065, 80) and align.shape == (B, 355, L)
    assert errs['mel'] < 1e-3 and errs['align'] < 1e-4 and errs['stop'] < 1e-3          # north star
    assert errs['mel'] < 5e-5                                                            # measured: ~1e-6


# ------------------------------------------------------------------------------------ C2 exactly as benchmarked
def test_c2_bench_configuration_graph_replay_with_oracle_masks(dev):
    """What bench.py times: GraphedDecoder replay (hipGraph of the 86-step loop, packed weights cached, prenet layer 1
    fused into the proj launch) with prenet dropout 0.5.  The oracle draws the masks (the reference's draw order),
    they are replayed through GraphedDecoder.own_mask, and the outputs must agree."""
    from semi_tts_amd.module import plan_decode
    from semi_tts_amd.runtime import GraphedDecoder
    from semi_tts_amd.synthetic import synthetic_batch
    B, L, T = 32, 43, 258
    m = full_tacotron(dev, seed=1234, prenet_dropout=0.5)
    txt, spk, _ = synthetic_batch(B, L, T, seed=100)
    txt, spk = torch.from_numpy(txt), torch.from_numpy(spk)
    with torch.no_grad():
        mem = m.encoder(txt.to(dev), None).contiguous()
    hp = full_hp(0.5)
    drop = O.DropoutSource('rng', generator=torch.Generator().manual_seed(3))
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        mel_r, al_r, st_r = O.decoder_forward(_weights(m), mem.cpu(), T, spk, hp, tf_rate=0.0, training=False, drop=drop)
    steps, src = plan_decode(True, T, B, B, 3, 0.0, 0.0, None)
    masks = split_masks(drop.used, hp, False, 0.0, B, B, steps, src, hp['prenet_dim'])
    gd = GraphedDecoder(m.decoder, B, L, T, dev)
    gd.capture()
    assert m.decoder.fuse_prenet and gd.own_mask is not None
    gd.own_mask.copy_(masks['own'].to(dev))
    mel, align, stop = gd(mem, spk.to(dev), redraw=False)
    torch.cuda.synchronize()
    curve = _step_curve(mel, mel_r, steps)
    errs = dict(mel=maxdiff(mel, mel_r), align=maxdiff(align, al_r), stop=maxdiff(stop, st_r))
    report('c2_bench_config', mel_last_step=float(curve[-1]), **errs)
    assert errs['mel'] < 1e-3 and errs['align'] < 1e-4 and errs['stop'] < 1e-3          # north star
    assert errs['mel'] < 5e-5
    # a second replay with the same masks is bit-identical; eager with the same masks too
    mel_a = mel.clone()
    mel_b = gd(redraw=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(mel_a, mel_b)
    with torch.no_grad():
        mel_e = m.decoder(mem, None, T, spk.to(dev), tf_rate=0.0, _masks={'own': gd.own_mask})[0]
    assert torch.equal(mel_e, mel_a)


# ------------------------------------------------------------------------------------ C2 with expanding dynamics
def test_c2_with_scaled_recurrent_weights(dev):
    """LSTM weights x2.5: the synthetic U(+-sqrt(3/fan_in)) weights are contractive, so every other full-size test sees
    only summation-order noise (1e-7).  With gain 2.5 the fp32 CPU oracle itself drifts 1e-5 from its float64 self over
    86 steps; the HIP path must stay within the same order of the fp32 oracle (bound: the north star's 1e-3)."""
    from semi_tts_amd.synthetic import synthetic_batch
    B, L, T = 32, 43, 258
    m = full_tacotron(dev, seed=99)
    with torch.no_grad():
        for cell in (m.decoder.query_rnn, m.decoder.dec_rnn):
            cell.weight_ih.mul_(2.5)
            cell.weight_hh.mul_(2.5)
    txt, spk, _ = synthetic_batch(B, L, T)
    txt, spk = torch.from_numpy(txt), torch.from_numpy(spk)
    with torch.no_grad():
        mem = m.encoder(txt.to(dev), None)
        mel, align, stop = m.decoder(mem, None, T, spk.to(dev), tf_rate=0.0)
    W = _weights(m)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        mel_r, al_r, _ = O.decoder_forward(W, mem.cpu(), T, spk, full_hp(0.0))
        torch.set_default_dtype(torch.float64)
        try:
            mel_d, _, _ = O.decoder_forward({k: v.double() for k, v in W.items()}, mem.cpu().double(), T, spk.double(),
                                            full_hp(0.0))
        finally:
            torch.set_default_dtype(torch.float32)
    c_hip, c_cpu = _step_curve(mel, mel_d, 86), _step_curve(mel_r, mel_d, 86)
    errs = dict(mel_vs_fp32_oracle=maxdiff(mel, mel_r), hip_vs_fp64=float(c_hip.max()), cpu_fp32_vs_fp64=float(c_cpu.max()),
                align=maxdiff(align, al_r))
    report('c2_gain2p5', hip_curve=json.dumps([float('%.1e' % v) for v in c_hip[::10]]),
           cpu_curve=json.dumps([float('%.1e' % v) for v in c_cpu[::10]]), **errs)
    assert errs['mel_vs_fp32_oracle'] < 1e-3 and errs['hip_vs_fp64'] < 1e-3
    # the HIP path accumulates error no faster than the CPU fp32 path does (x8 head-room for run-to-run variation)
    assert errs['hip_vs_fp64'] < 8 * max(errs['cpu_fp32_vs_fp64'], 1e-6)


# ------------------------------------------------------------------------------------ C2-size training step
def test_c2_training_step_against_oracle_autograd(dev):
    """One paired training step at BASELINE config 2 size through the trainer's own path (VQVAE.text_to_speech ->
    freq_loss(mel) + freq_loss(linear) -> backward -> global grad norm), tf_rate 1, all dropouts and batch-statistics
    BatchNorm active, against CPU fp32 autograd through the oracle replaying the same masks.
    ref: bin/train_vqvae.py:219-223,270; src/solver.py:138-151; src/util.py:80-126."""
    import yaml
    from semi_tts_amd import autograd as AG
    from semi_tts_amd.optim import clip_grad_norm_
    from semi_tts_amd.synthetic import load_synthetic, synthetic_train_batch
    from semi_tts_amd.vqvae import VQVAE
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    mcfg = cfg['model']
    mcfg['codebook'].update(phn_attr_pth='', proj_attr=None)          # the attribute csv lives in the reference tree
    sr, n_mels = cfg['data']['audio']['sample_rate'], cfg['data']['audio']['num_mels']
    m = VQVAE(80, 1025, 43, 109, **mcfg)
    load_synthetic(m, 321)
    m = m.to(dev).train()
    text, sid, mel, linear = synthetic_train_batch(32, 256, 3, seed=17)
    B, T = mel.shape[0], mel.shape[1]
    steps = T // 3
    hp = dict(mcfg['decoder']['decoder'], n_mels=80, enc_dropout=mcfg['decoder']['encoder']['enc_dropout'])

    # ---- oracle: fp32 CPU autograd
    W = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    Wt = {k[4:]: v.requires_grad_(v.is_floating_point() and 'running_' not in k) for k, v in W.items() if k.startswith('tts.')}
    table = W['codebook.learnable_table'].requires_grad_()
    spk_table = W['spkr_embed.weight'].requires_grad_()
    drop = O.DropoutSource('rng', generator=torch.Generator().manual_seed(23))
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    lat = VQ.l2_inference({'learnable_table': table}, text)
    # Tacotron2.forward with separate_postnet = true (every shipped config): the postnet sees mel.detach()  (src/tts.py:47-50)
    enc_r = O.encoder_forward(Wt, lat, 'encoder.', True, hp['enc_dropout'], drop, None)
    mel_r, al_r, _ = O.decoder_forward(Wt, enc_r, mel, spk_table[sid], hp, 1.0, None, True, drop, lambda: 0.0)
    lin_r = O.postnet_forward(Wt, mel_r.detach(), True, None)
    loss_r = O.freq_loss(mel_r, mel, sr, n_mels) + O.freq_loss(lin_r, linear, sr, n_mels)
    loss_r.backward()
    ref_g = {'tts.' + k: v.grad for k, v in Wt.items() if v.requires_grad and v.grad is not None}
    ref_g['codebook.learnable_table'] = table.grad
    ref_g['spkr_embed.weight'] = spk_table.grad
    gn_ref = float(torch.sqrt(sum((g.double() ** 2).sum() for g in ref_g.values())))

    # ---- HIP: same masks
    masks = masks_to(split_masks(drop.used, hp, True, 1.0, B, B, steps, list(range(steps)), hp['prenet_dim']), dev)
    mel_p, lin_p, align, *_ = m.text_to_speech(text.to(dev), sid.to(dev), None, None, None, None, mel.to(dev), None, 1.0,
                                               _masks=masks)
    f = lambda p, l: AG.freq_loss(p, l, sr, n_mels, 'mse', True, True)
    loss = f(mel_p, mel.to(dev)) + f(lin_p, linear.to(dev))
    loss.backward()
    gn = float(clip_grad_norm_([p for p in m.parameters() if p.grad is not None], 1e9))
    named = dict(m.named_parameters())
    # Gradients are compared three ways.  A ReLU / max-pool whose input is within round-off of zero can land on the other side of
    # the kink than in the CPU run, which changes ONE term of a gradient sum by 100 % (measured with tools/debug_train_grads.py:
    # tts.encoder.convs.1.1.bias has a median element error of 2e-11, a 99.9th percentile of 9e-11 and ONE element off by 6e-7 =
    # 1.5 % of the tensor's scale).  So: the 99.9th-percentile element error and the relative L2 error are bounded tightly, the
    # single worst element loosely.
    worst, worst_k, worst_p999, worst_l2, n = 0.0, '', 0.0, 0.0, 0
    for k, g in ref_g.items():
        assert named[k].grad is not None, 'missing gradient for ' + k
        scale = float(g.abs().max())
        if scale < 1e-9:
            continue
        d = (named[k].grad.detach().cpu().double() - g.double()).abs().flatten()
        e = float(d.max()) / scale
        p999 = float(d.kthvalue(max(1, int(0.999 * d.numel())))[0]) / scale
        l2 = float(d.norm() / g.double().norm())
        worst_p999, worst_l2 = max(worst_p999, p999), max(worst_l2, l2)
        n += 1
        if e > worst:
            worst, worst_k = e, k
        assert p999 < 5e-3 and l2 < 5e-3 and e < 0.1, (k, e, p999, l2)
    errs = dict(mel=maxdiff(mel_p, mel_r), lin=maxdiff(lin_p, lin_r), align=maxdiff(align, al_r),
                loss=abs(float(loss.detach()) - float(loss_r.detach())), loss_ref=float(loss_r.detach()),
                grad_norm=gn, grad_norm_ref=gn_ref, worst_grad_relerr=worst, worst_p999_relerr=worst_p999, worst_rel_l2=worst_l2,
                n_grads=n)
    report('c2_train_step', worst_grad=worst_k, **errs)
    assert errs['mel'] < 1e-3 and errs['lin'] < 1e-3 and errs['align'] < 1e-4
    assert errs['loss'] < 1e-5 * max(1.0, abs(errs['loss_ref']))
    assert abs(gn - gn_ref) < 1e-3 * gn_ref
    assert n >= 95


def test_postnet_class_training_mode_against_reference_golden(dev):
    """The `Postnet` class in TRAINING mode (batch-statistics BatchNorm + nn.Dropout(0.5) after every block, src/module.py:53-82):
    forward with the reference's recorded masks, the running statistics after the step, and the gradients of y.pow(2).sum()
    against what the real reference produced (tools/gen_golden.py postnet_class_train_case)"""
    from semi_tts_amd.module import Postnet
    W, A, _ = load_golden('conv_postnet_train')
    m = Postnet(8, 16, 5, 5, 0.5)
    m.load_state_dict(W)
    m = m.to(dev).train()
    x = A['x'].to(dev).requires_grad_(True)
    y = m(x, _masks=[t.to(dev) for t in A['masks']])
    e_y = maxdiff(y, A['y'])
    y.pow(2).sum().backward()
    e_dx = maxdiff(x.grad, A['dx'])
    sd = m.state_dict()
    e_run = max(maxdiff(sd[k].float(), v.float()) for k, v in A['after'].items())
    scale = max(float(v.abs().max()) for v in A['grad'].values())
    e_g = max(maxdiff(p.grad, A['grad'][k]) for k, p in m.named_parameters())
    report('postnet_class_train', err_y=e_y, err_dx=e_dx, err_running=e_run, err_grad=e_g, grad_scale=scale)
    assert e_y < 2e-5 and e_run < 1e-5
    assert e_dx < 2e-4 * max(1.0, float(A['dx'].abs().max())) and e_g < 2e-4 * max(1.0, scale)
    # without explicit masks the module draws its own (device RNG): finite, and about half of the last block's outputs dropped
    y2 = m(A['x'].to(dev))
    assert bool(torch.isfinite(y2).all()) and 0.3 < float((y2 == 0).float().mean()) < 0.7


def test_c2_training_step_with_poisoned_uninitialised_buffers(dev):
    """The training loops hand their step tapes and slab workspaces to the kernels UNINITIALISED where every element is written before
    it is read (no padding at C2 sizes: B and every width a multiple of 16).  With those buffers filled with NaN first
    (ops.POISON_UNINIT) the step must give the same gradients bit for bit: nothing reads what nobody wrote."""
    import yaml
    from semi_tts_amd import autograd as AG, ops
    from semi_tts_amd.synthetic import load_synthetic, synthetic_train_batch
    from semi_tts_amd.vqvae import VQVAE
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    mcfg = cfg['model']
    mcfg['codebook'].update(phn_attr_pth='', proj_attr=None)
    sr, n_mels = cfg['data']['audio']['sample_rate'], cfg['data']['audio']['num_mels']
    text, sid, mel, linear = (t.to(dev) for t in synthetic_train_batch(32, 256, 3, seed=17))

    def run(poison):
        m = VQVAE(80, 1025, 43, 109, **mcfg)
        load_synthetic(m, 321)
        m = m.to(dev).train()
        old = ops.POISON_UNINIT
        ops.POISON_UNINIT = poison
        try:
            torch.manual_seed(5)
            mel_p, lin_p, *_ = m.text_to_speech(text, sid, None, None, None, None, mel, None, 1.0)
            f = lambda p, l: AG.freq_loss(p, l, sr, n_mels, 'mse', True, True)
            (f(mel_p, mel) + f(lin_p, linear)).backward()
        finally:
            ops.POISON_UNINIT = old
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    g0, g1 = run(False), run(True)
    assert set(g0) == set(g1) and len(g0) > 100
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


def test_postnet_branch_on_a_second_stream_gives_bitwise_the_serial_step(dev):
    """separate_postnet (src/tts.py:47-50): the postnet sees mel_pred.detach(), so CBHG forward + linear freq_loss + CBHG backward neither
    feed nor wait for the decoder's backward through time.  TtsTrainer runs that branch on a second HIP stream beside the main chain
    (Tacotron2.postnet_side) and joins before the clip: losses, gradient norm and EVERY weight after two steps must equal the serial
    order bit for bit (no kernel's result depends on what runs beside it; the queued weight-gradient products leave on the stream their
    operands were produced on) -- config-3 model at B = 8, 66 frames."""
    import yaml
    from argparse import Namespace
    from semi_tts_amd.solver import TtsTrainer
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    outs = []
    for side in (False, True):
        paras = Namespace(batch_size=8, frames=64, n_batches=1, seed=3, verbose=False, max_step=2, load=None)
        tr = TtsTrainer(cfg, paras, 'train').load_data().set_model()
        tr.postnet_side = side
        torch.manual_seed(7)
        batch = [t.to(dev) for t in tr.batches[0]]
        sts = [tr.train_step(*batch) for _ in range(2)]
        torch.cuda.synchronize()
        assert (tr.model.tts.postnet_stream is not None) == side
        outs.append(([(float(s['loss']), float(s['mel_loss']), float(s['linear_loss']), float(s['grad_norm'])) for s in sts],
                     {k: v.detach().clone() for k, v in tr.model.state_dict().items()}))
    (s0, w0), (s1, w1) = outs
    assert s0 == s1, (s0, s1)
    assert all(x == x for t in s1 for x in t)
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k


@pytest.mark.parametrize('B,dims', [(16, dict(prenet_dim=128, query_rnn_dim=512, dec_rnn_dim=512, attn_dim=128)),
                                    (48, dict(prenet_dim=256, query_rnn_dim=512, dec_rnn_dim=1024, attn_dim=256)),
                                    (32, dict(prenet_dim=200, query_rnn_dim=520, dec_rnn_dim=520, attn_dim=64)),       # not multiples of 16: no fused BPTT loop
                                    (20, dict(prenet_dim=256, query_rnn_dim=1024, dec_rnn_dim=1024, attn_dim=256))])   # pad rows (B % 16 != 0)
def test_training_step_with_poisoned_uninitialised_buffers_at_other_dimensions(dev, B, dims):
    """Advisor (round 5): the step tapes are handed over UNINITIALISED only where every element is written before it is read -- which
    depends on which loop the library takes for the dimensions (the fused BPTT loop needs Q, D, E + Q multiples of 16 ...; the six-launch
    loop reads a zero slot behind the last step).  The library is asked beforehand (st_decoder_bwd_fuse_dims) and refuses fuse_pw where
    it cannot honour it.  With every such buffer filled with NaN first (ops.POISON_UNINIT) the gradients must be bitwise those of the
    clean run at other batch sizes and at dimensions that take the generic loops."""
    import yaml
    from semi_tts_amd import autograd as AG, ops
    from semi_tts_amd.synthetic import load_synthetic, synthetic_train_batch
    from semi_tts_amd.vqvae import VQVAE
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    mcfg = cfg['model']
    mcfg['codebook'].update(phn_attr_pth='', proj_attr=None)
    mcfg['decoder']['decoder'].update(dims)
    sr, n_mels = cfg['data']['audio']['sample_rate'], cfg['data']['audio']['num_mels']
    text, sid, mel, linear = (t.to(dev) for t in synthetic_train_batch(B, 30, 3, seed=19))

    def run(poison):
        m = VQVAE(80, 1025, 43, 109, **mcfg)
        load_synthetic(m, 321)
        m = m.to(dev).train()
        old = ops.POISON_UNINIT
        ops.POISON_UNINIT = poison
        try:
            torch.manual_seed(5)
            mel_p, lin_p, *_ = m.text_to_speech(text, sid, None, None, None, None, mel, None, 1.0)
            f = lambda p, l: AG.freq_loss(p, l, sr, n_mels, 'mse', True, True)
            (f(mel_p, mel) + f(lin_p, linear)).backward()
        finally:
            ops.POISON_UNINIT = old
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    g0, g1 = run(False), run(True)
    assert set(g0) == set(g1) and len(g0) > 100
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


def test_decoder_loops_replayed_from_graphs_give_bitwise_the_eager_steps(dev):
    """The two C++ loops of a training step come back with bit-identical arguments step after step (the allocator repeats its addresses);
    the library captures them into hipGraphs at the second sighting and replays them (loop_graph.h).  Twelve steps with the replay on must
    equal twelve steps with it off bit for bit -- losses, gradient norms, every weight -- and the counters must show replays of both loops."""
    import ctypes as C
    import yaml
    from argparse import Namespace
    from semi_tts_amd import _lib
    from semi_tts_amd.solver import TtsTrainer
    lib = _lib.load()
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config', 'semi-single-spkr-paired-data.yaml')))
    outs = []
    prev = lib.st_loop_graphs_enable(1)
    try:
        for on in (0, 1):
            lib.st_loop_graphs_enable(on)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()           # (the allocator repeats its addresses once it has settled: start both runs from the same empty state)
            f0, b0 = (C.c_long * 3)(), (C.c_long * 3)()
            lib.st_loop_graph_stats(f0, b0)
            paras = Namespace(batch_size=32, frames=64, n_batches=1, seed=3, verbose=False, max_step=12, load=None)
            tr = TtsTrainer(cfg, paras, 'train').load_data().set_model()
            tr.async_stats = True
            torch.manual_seed(7)
            batch = [t.to(dev) for t in tr.batches[0]]
            sts = [tr.train_step(*batch) for _ in range(12)]
            tr.drain_stats()
            torch.cuda.synchronize()
            f1, b1 = (C.c_long * 3)(), (C.c_long * 3)()
            lib.st_loop_graph_stats(f1, b1)
            outs.append(([(float(s['loss']), float(s['grad_norm'])) for s in sts], {k: v.detach().clone() for k, v in tr.model.state_dict().items()},
                         (f1[0] - f0[0], b1[0] - b0[0], f1[1] - f0[1], b1[1] - b0[1])))
    finally:
        lib.st_loop_graphs_enable(prev)
    (s0, w0, c0), (s1, w1, c1) = outs
    assert c0 == (0, 0, 0, 0), c0                      # off: nothing captured, nothing replayed
    assert c1[0] >= 1 and c1[1] >= 1 and c1[2] >= 1 and c1[3] >= 1, c1      # on: both loops captured and replayed
    assert s0 == s1, (s0, s1)
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k


# ------------------------------------------------------------------------------------ the decoder cell's dependency split (round 6)
def test_decoder_gate_split_at_every_cut_agrees_with_the_whole_cell_and_the_oracle(dev):
    """Decoder.split_gates: a suffix of the decoder cell's gate reduction [ctx | AdaIN(h_q(t)) | h_d(t-1)] rides beside the pq / fin launch, the
    cell launch reduces the columns in front of the cut (st_decoder_io.gate_part / gate_part_k).  C2 shape, 20 free-running steps, prenet
    dropout 0: every cut -- the library's rule (half, 1280) and 512 / 1024 / 1536 / 2048 -- agrees with the unsplit step to fp32 re-association
    and with the oracle to the north-star tolerance; the two-launch form of the attention step issues the same product as a launch of its own
    and is bit-identical to the hosted form; a cut that is not a multiple of 16 or inside the context columns is refused."""
    import ctypes as C
    from semi_tts_amd import _lib
    from semi_tts_amd._lib import StDecoderDims
    from semi_tts_amd.synthetic import synthetic_batch
    m = full_tacotron(dev, seed=31)
    dec = m.decoder
    B, L, T = 32, 43, 60
    txt, spk, _ = synthetic_batch(B, L, 3, seed=12)
    txt, spk = torch.from_numpy(txt), torch.from_numpy(spk)
    with torch.no_grad():
        mem = m.encoder(txt.to(dev), None)
    d = StDecoderDims(B=B, L=L, E=512, n_mels=80, r=3, P=256, Q=1024, D=1024, A=128)
    assert _lib.load().st_decoder_gate_split_k(C.byref(d)) == 1280 == dec.gate_split_k()

    def run(split, k=0, pq_in_fin=True):
        dec.split_gates, dec.split_cell_k, dec.attn_pq_in_fin = split, k, pq_in_fin
        with torch.no_grad():
            out = [t.clone() for t in dec(mem, None, T, spk.to(dev), tf_rate=0.0)]
        # the form that ran: the product beside pq + fin, in a launch of its own beside the two-launch attention, or none
        want = ('pq_fin', 'pq_fin' if split else 'none') if pq_in_fin else ('pre_fin', 'own' if split else 'none')
        assert fwd_forms(dec._last_fwd_forms)[:2] == want, hex(dec._last_fwd_forms)
        assert dec._last_fwd_forms >> 16 == ((k or 1280) // 16 if split else 0)
        return out
    try:
        whole = run(False)
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
        with torch.no_grad():
            mel_r, al_r, st_r = O.decoder_forward(_weights(m), mem.cpu(), T, spk, full_hp(0.0))
        worst = 0.0
        for k in (0, 512, 1024, 1536, 2048):
            got = run(True, k)
            e = max(maxdiff(a, b) for a, b in zip(got, whole))
            worst = max(worst, e)
            assert e < 2e-5, (k, e)
            assert maxdiff(got[0], mel_r) < 5e-5 and maxdiff(got[1], al_r) < 1e-4 and maxdiff(got[2], st_r) < 1e-3, k
            again = run(True, k)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), k
            if k in (0, 1024):
                two = run(True, k, pq_in_fin=False)          # the product as a launch of its own
                assert all(torch.equal(a, b) for a, b in zip(got, two)), k
        report('decoder_gate_split_cuts', worst_vs_whole_cell=worst)
        for bad in (1000, 256, 2560):
            with pytest.raises(RuntimeError):
                run(True, bad)
    finally:
        dec.split_gates, dec.split_cell_k, dec.attn_pq_in_fin = True, 0, True


def test_training_loop_with_the_gate_split_agrees_with_the_unsplit_loop(dev):
    """The same split in the teacher-forced loop (Decoder.split_gates_train: the product rides beside the query projection + attention pre
    part, the paired cell launch adds the slab): outputs and every gradient of the full-size decoder agree with the unsplit loop to fp32
    re-association, and the split loop reproduces itself bit for bit."""
    m = full_tacotron(dev, seed=4321, prenet_dropout=0.5).train()
    dec = m.decoder
    B, L, steps = 32, 43, 6
    r, n_mels = dec.n_frames_per_step, dec.n_mels
    g = torch.Generator().manual_seed(1)
    mem0, spk0 = torch.randn(B, L, 512, generator=g).to(dev), torch.randn(B, 128, generator=g).to(dev)
    teacher = torch.rand(B, steps * r, n_mels, generator=g).to(dev)
    douts = None
    res = []
    try:
        for split in (False, True, True):
            dec.split_gates_train = split
            for p in dec.parameters():
                p.grad = None
            torch.manual_seed(77)
            mem, spk = mem0.clone().requires_grad_(), spk0.clone().requires_grad_()
            mel, align, stop = dec(mem, None, teacher, spk, tf_rate=1.0)
            assert fwd_forms(dec._last_fwd_forms)[:2] == ('pre_fin', 'pq_pre' if split else 'none'), hex(dec._last_fwd_forms)
            if douts is None:
                douts = [torch.randn(t.shape, generator=g).to(dev) for t in (mel, align, stop)]
            torch.autograd.backward([mel, align, stop], douts)
            res.append(dict(mel=mel.detach().clone(), align=align.detach().clone(), dmem=mem.grad.clone(), dspk=spk.grad.clone(),
                            **{k: p.grad.clone() for k, p in dec.named_parameters() if p.grad is not None}))
    finally:
        dec.split_gates_train = True
    whole, split, again = res
    assert len(whole) > 20
    worst = 0.0
    for k, v in whole.items():
        e = float((split[k] - v).abs().max() / v.abs().max().clamp_min(1e-12))
        worst = max(worst, e)
        assert e < 2e-5, (k, e)
        assert torch.equal(split[k], again[k]), k
    report('training_gate_split', worst_rel=worst, n=len(whole))
