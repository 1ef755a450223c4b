"""The refusals of the model-free scoring and signal ops, pinned to the letter: the full text of every ValueError, which refusal wins when
an input is wrong in two ways, and that a good input gets as far as the library.  No device: _lib.load is patched to raise, and a meta
tensor (or a flagged host tensor, where two different buffers or two devices are needed) stands in for a device tensor.

The table was written against ops.py at 064bfb2, where the functions below hold 127 `raise ValueError` statements (75 in the scoring
ops from ctc_greedy_edit_distance to edit_align, 52 in the signal ops from f0_yin to wave_gather; a search for the two words finds 128,
one of them in abx_count's docstring).  test_every_refusal_is_pinned finds the statements of whatever module holds the functions now
and fails on one that no row reaches; the one refusal that cannot be reached without a device is named in UNREACHED."""
import ast
import inspect
import textwrap

import pytest
import torch

F32, F64, I64, I32, I16 = torch.float32, torch.float64, torch.int64, torch.int32, torch.int16
REACHED = 'reached the device'


def M(*shape, dtype=F32):
    """a meta tensor: shape, dtype, strides and a device, no memory"""
    return torch.zeros(*shape, dtype=dtype, device='meta')


def H(*shape, dtype=F32):
    """a host tensor flagged to pass for a device tensor: a second 'device', and buffers with addresses of their own"""
    t = torch.zeros(*shape, dtype=dtype)
    t.stands_in = True
    return t


@pytest.fixture
def no_device(monkeypatch):
    from semi_tts_amd import _lib

    def load(*a, **k):
        raise AssertionError(REACHED)
    monkeypatch.setattr(_lib, 'load', load)
    # the checks read .is_cuda / .device / .shape / .dtype / .stride() only
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type in ('cuda', 'meta') or getattr(self, 'stands_in', False)))


P, TX = M(2, 4, 5), M(2, 3, dtype=I64)                                           # posteriors (B, T, V) and transcripts (B, L)
X, Y = M(2, 5, 3), M(2, 6, 3)                                                    # dtw's two sides
FE, IS, IL, PA, PB = M(10, 4), M(3, dtype=I32), M(3, dtype=I32), M(2, dtype=I32), M(2, dtype=I32)       # dtw_pairs' operands
DM, BK = M(9), M(2, 6, dtype=I64)                                                # abx_count's
AL = M(2, 5, 4)                                                                  # attn_endpoint's alignment (B, S, L)
HY, HL = M(2, 4, dtype=I64), M(2, dtype=I32)                                     # hyp_edit_distance's
EH, EL, ER = M(2, 3, 4, dtype=I64), [[4, 1, 0], [2, 2, 2]], M(2, 5, dtype=I64)   # edit_align's
FB = (M(8, dtype=I32), M(8, dtype=I32), M(8, dtype=I32), M(40))                  # a banded mel filterbank
W160, OL = M(160), dict(off=[0, 100], lens=[100, 60])                            # a packed batch of two utterances
F0 = dict(OL, hop=20, W=80, tau_min=5, tau_max=40, sample_rate=2000.0, threshold=0.15, T_pad=6)
FX, FY, PATH, PLEN = M(2, 5), M(2, 6), M(2, 10, 2, dtype=I32), M(2, dtype=I32)   # f0_path_scores'
TR = dict(OL, frame_length=40, hop=20, top_db=30.0)
W4K, LD = M(4000), dict(off=[0, 2000], lens=[2000, 1700], sr=16000)              # loudness at 16 kHz: hops of 1600 samples
WG = dict(off=[0, 2000], lens=[2000, 1700], stats=M(2, 8))
W1K, ST = M(1000), dict(off=[0, 500], lens=[500, 400])                           # stoi_batch: 2 frames in the longer signal
PR = dict(xoff=[0, 500], xlens=[500, 400], yoff=[0, 300], ylens=[300, 700])      # xcorr_delay's / sisdr_batch's pairs
S8, D8 = H(8), H(8)                                                              # wave_gather's two buffers

# (function, positional arguments, keyword arguments, the whole message, '' / 'order': wrong in two ways / 'good')
TABLE = [
    # ------------------------------------------------------------------------------------------------ ctc_greedy_edit_distance
    ('ctc_greedy_edit_distance', (None, TX, ()), {}, 'ctc_greedy_edit_distance: prob and text must be tensors', ''),
    ('ctc_greedy_edit_distance', (torch.zeros(2, 4, 5), TX, ()), {}, 'ctc_greedy_edit_distance: prob and text must be on one GPU (got cpu, meta)', ''),
    ('ctc_greedy_edit_distance', (M(2, 4, 5, dtype=F64), TX, ()), {}, 'ctc_greedy_edit_distance: prob must be (B, T, V) float32 or (B, T) int64 (got (2, 4, 5) torch.float64)', ''),
    ('ctc_greedy_edit_distance', (M(2, 4), TX, ()), {}, 'ctc_greedy_edit_distance: prob must be (B, T, V) float32 or (B, T) int64 (got (2, 4) torch.float32)', ''),
    ('ctc_greedy_edit_distance', (P, M(2, 3, dtype=I32), ()), {}, 'ctc_greedy_edit_distance: text must be (B, L) int64 (got (2, 3) torch.int32)', ''),
    ('ctc_greedy_edit_distance', (P, M(3, 3, dtype=I64), ()), {}, 'ctc_greedy_edit_distance: 2 utterances of prob, 3 of text (at least one)', ''),
    ('ctc_greedy_edit_distance', (M(1, 4097, 5), M(1, 3, dtype=I64), ()), {}, 'ctc_greedy_edit_distance: T=4097, V=5, L=3, 0 ignored ids outside 1 <= T <= 4096, 1 <= V <= 10240, 1 <= L <= 1024, <= 64 ignored ids', ''),
    ('ctc_greedy_edit_distance', (P, TX, (2 ** 31,)), {}, 'ctc_greedy_edit_distance: ignored ids must fit int32', ''),
    ('ctc_greedy_edit_distance', (M(2, 4, 5, dtype=F64), M(2, 3, dtype=I32), ()), {}, 'ctc_greedy_edit_distance: prob must be (B, T, V) float32 or (B, T) int64 (got (2, 4, 5) torch.float64)', 'order'),
    ('ctc_greedy_edit_distance', (P, TX, (0,)), {}, REACHED, 'good'),
    ('ctc_greedy_edit_distance', (M(2, 4, dtype=I64), TX, ()), dict(want_hyp=True), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ ctc_beam_search
    ('ctc_beam_search', (torch.zeros(2, 4, 5),), {}, 'ctc_beam_search: prob must be a (B, T, V) float32 GPU tensor (got (2, 4, 5) torch.float32 on cpu)', ''),
    ('ctc_beam_search', (None,), {}, 'ctc_beam_search: prob must be a (B, T, V) float32 GPU tensor (got NoneType)', ''),
    ('ctc_beam_search', (M(2, 4, 1),), {}, 'ctc_beam_search: B=2, T=4, V=1 outside B >= 1, 1 <= T <= 4096, 2 <= V <= 1024', ''),
    ('ctc_beam_search', (P,), dict(beam_width=129), 'ctc_beam_search: need 1 <= top_paths <= beam_width <= 128 (beam_width 129, top_paths 1)', ''),
    ('ctc_beam_search', (P,), dict(top_paths=17), 'ctc_beam_search: need 1 <= top_paths <= beam_width <= 128 (beam_width 16, top_paths 17)', ''),
    ('ctc_beam_search', (P,), dict(blank=5), 'ctc_beam_search: blank 5 outside [0, 5)', ''),
    ('ctc_beam_search', (P,), dict(eps=-1.0), 'ctc_beam_search: eps must be >= 0 (got -1.0)', ''),
    ('ctc_beam_search', (P,), dict(eps=float('nan')), 'ctc_beam_search: eps must be >= 0 (got nan)', ''),
    ('ctc_beam_search', (P,), dict(bonus=torch.zeros(5, 5)), 'ctc_beam_search: bonus must be a contiguous (V^(order-1), V) float32 tensor on the device of prob (got (5, 5) torch.float32 on cpu)', ''),
    ('ctc_beam_search', (P,), dict(bonus=[[0.0]]), 'ctc_beam_search: bonus must be a contiguous (V^(order-1), V) float32 tensor on the device of prob (got list)', ''),
    ('ctc_beam_search', (P,), dict(bonus=M(7, 5)), 'ctc_beam_search: a bonus table of shape (7, 5) is no (V^(order-1), V) table for V = 5, 1 <= order <= 4', ''),
    ('ctc_beam_search', (P,), dict(bonus=M(5, 4)), 'ctc_beam_search: a bonus table of shape (5, 4) is no (V^(order-1), V) table for V = 5, 1 <= order <= 4', ''),
    ('ctc_beam_search', (P,), dict(bonus=M(5, 5), order=3), 'ctc_beam_search: order 3, but the bonus table of shape (5, 5) has order 2', ''),
    ('ctc_beam_search', (M(1, 4, 1024),), dict(bonus=M(1024 * 1024, 1024)), 'ctc_beam_search: V^order = 1024^3 table elements, at most 2^26', ''),
    ('ctc_beam_search', (P,), dict(bonus=M(5, 5), bos=5), 'ctc_beam_search: bos 5 outside [0, 5)', ''),
    ('ctc_beam_search', (P,), dict(order=2), 'ctc_beam_search: order 2 without a bonus table', ''),
    ('ctc_beam_search', (P,), dict(lengths=M(2)), 'ctc_beam_search: lengths must be (B,) integers on the device of prob (got (2,) torch.float32 on meta)', ''),
    ('ctc_beam_search', (P,), dict(lengths=M(3, dtype=I32)), 'ctc_beam_search: lengths must be (B,) integers on the device of prob (got (3,) torch.int32 on meta)', ''),
    ('ctc_beam_search', (P,), dict(lengths=[1, 5]), 'ctc_beam_search: lengths must be 2 integers in [0, 4] (got [1, 5])', ''),
    ('ctc_beam_search', (P,), dict(lengths=torch.tensor([1, 2, 3])), 'ctc_beam_search: lengths must be 2 integers in [0, 4] (got [1, 2, 3])', ''),
    ('ctc_beam_search', (P,), dict(lengths=[1.0, 2.0]), 'ctc_beam_search: lengths must be 2 integers in [0, 4] (got [1.0, 2.0])', ''),
    ('ctc_beam_search', (P,), dict(lengths=M(2, dtype=torch.bool)), 'ctc_beam_search: lengths must be (B,) integers on the device of prob (got (2,) torch.bool on meta)', ''),
    ('ctc_beam_search', (M(2, 4, 1),), dict(beam_width=0), 'ctc_beam_search: B=2, T=4, V=1 outside B >= 1, 1 <= T <= 4096, 2 <= V <= 1024', 'order'),
    ('ctc_beam_search', (P,), {}, REACHED, 'good'),
    ('ctc_beam_search', (P,), dict(lengths=[4, 0]), REACHED, 'good'),
    ('ctc_beam_search', (P,), dict(lengths=M(2, dtype=I64), log_input=True), REACHED, 'good'),
    ('ctc_beam_search', (P,), dict(bonus=M(25, 5), order=3, bos=4), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ ctc_forced_align
    ('ctc_forced_align', (torch.zeros(2, 4, 5), TX), {}, 'ctc_forced_align: prob must be a (B, T, V) float32 GPU tensor (got (2, 4, 5) torch.float32 on cpu)', ''),
    ('ctc_forced_align', ('x', TX), {}, 'ctc_forced_align: prob must be a (B, T, V) float32 GPU tensor (got str)', ''),
    ('ctc_forced_align', (P, torch.zeros(2, 3, dtype=I64)), {}, 'ctc_forced_align: text must be a (B, L) int64 tensor on the device of prob (got (2, 3) torch.int64 on cpu)', ''),
    ('ctc_forced_align', (P, None), {}, 'ctc_forced_align: text must be a (B, L) int64 tensor on the device of prob (got NoneType)', ''),
    ('ctc_forced_align', (P, M(3, 3, dtype=I64)), {}, 'ctc_forced_align: 2 utterances of prob, 3 of text', ''),
    ('ctc_forced_align', (M(2, 4, 1), TX), {}, 'ctc_forced_align: B=2, T=4, V=1, L=3 outside B >= 1, 1 <= T <= 4096, 2 <= V <= 10240, 1 <= L <= 1024', ''),
    ('ctc_forced_align', (P, TX), dict(blank=-1), 'ctc_forced_align: blank -1 outside [0, 5)', ''),
    ('ctc_forced_align', (P, TX), dict(eps=float('nan')), 'ctc_forced_align: eps must be >= 0 (got nan)', ''),
    ('ctc_forced_align', (P, TX), dict(lengths=M(2)), 'ctc_forced_align: lengths must be (B,) integers on the device of prob (got (2,) torch.float32 on meta)', ''),
    ('ctc_forced_align', (P, TX), dict(text_lengths=M(2, 2, dtype=I32)), 'ctc_forced_align: text_lengths must be (B,) integers on the device of prob (got (2, 2) torch.int32 on meta)', ''),
    ('ctc_forced_align', (P, TX), dict(lengths=[5, 1]), 'ctc_forced_align: lengths must be 2 integers in [0, 4] (got [5, 1])', ''),
    ('ctc_forced_align', (P, TX), dict(text_lengths=[1, 4]), 'ctc_forced_align: text_lengths must be 2 integers in [0, 3] (got [1, 4])', ''),
    ('ctc_forced_align', (P, TX), dict(lengths=torch.tensor([1])), 'ctc_forced_align: lengths must be 2 integers in [0, 4] (got [1])', ''),
    ('ctc_forced_align', (P, TX), dict(blank=9, lengths=[9, 9]), 'ctc_forced_align: blank 9 outside [0, 5)', 'order'),
    ('ctc_forced_align', (P, TX), {}, REACHED, 'good'),
    ('ctc_forced_align', (P, TX), dict(lengths=[4, 1], text_lengths=M(2, dtype=I32)), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ dtw
    ('dtw', (torch.zeros(2, 5, 3), Y), {}, 'dtw: x must be a (B, T, D) float32 GPU tensor (got (2, 5, 3) torch.float32 on cpu)', ''),
    ('dtw', (X, None), {}, 'dtw: y must be a (B, T, D) float32 GPU tensor (got NoneType)', ''),
    ('dtw', (X, H(2, 6, 3)), {}, 'dtw: x on meta, y on cpu', ''),
    ('dtw', (X, M(3, 6, 3)), {}, 'dtw: x is (2, 5, 3), y is (3, 6, 3): the pairs and the columns must match', ''),
    ('dtw', (M(2, 4097, 3), Y), {}, 'dtw: B=2, Tx=4097, Ty=6, D=3 outside B >= 1, 1 <= Tx, Ty <= 4096, D >= 1', ''),
    ('dtw', (X, Y), dict(cols=3), 'dtw: cols must be a pair (d0, d1) (got 3)', ''),
    ('dtw', (X, Y), dict(cols=(0, 1, 2)), 'dtw: cols must be a pair (d0, d1) (got (0, 1, 2))', ''),
    ('dtw', (X, Y), dict(cols=(2, 1)), 'dtw: cols [2, 1) outside 0 <= d0 < d1 <= D = 3, at most 64 columns', ''),
    ('dtw', (X, Y), dict(scale=0.0), 'dtw: scale must be finite and positive (got 0.0)', ''),
    ('dtw', (M(2, 5, 6)[:, :, ::2], Y), {}, 'dtw: x has strides (30, 6, 2): the last dimension needs stride 1 and rows at least d1 = 3 floats apart', ''),
    ('dtw', (X, Y), dict(x_len=M(2)), 'dtw: x_len must be (B,) integers on the device of x (got (2,) torch.float32 on meta)', ''),
    ('dtw', (X, Y), dict(y_len=M(3, dtype=I32)), 'dtw: y_len must be (B,) integers on the device of x (got (3,) torch.int32 on meta)', ''),
    ('dtw', (X, Y), dict(x_len=[6, 1]), 'dtw: x_len must be 2 integers in [0, 5] (got [6, 1])', ''),
    ('dtw', (X, Y), dict(y_len=[1, 7]), 'dtw: y_len must be 2 integers in [0, 6] (got [1, 7])', ''),
    ('dtw', (X, Y), dict(y_len=torch.tensor([-1, 2])), 'dtw: y_len must be 2 integers in [0, 6] (got [-1, 2])', ''),
    ('dtw', (X, M(3, 6, 3)), dict(scale=-1.0), 'dtw: x is (2, 5, 3), y is (3, 6, 3): the pairs and the columns must match', 'order'),
    ('dtw', (X, Y), {}, REACHED, 'good'),
    ('dtw', (X, Y), dict(x_len=[5, 0], y_len=M(2, dtype=I32), cols=(1, 3), want_path=False), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ dtw_pairs
    ('dtw_pairs', (torch.zeros(10, 4), IS, IL, PA, PB), {}, 'dtw_pairs: feat must be a (n_rows, D) float32 GPU tensor (got (10, 4) torch.float32 on cpu)', ''),
    ('dtw_pairs', (None, IS, IL, PA, PB), {}, 'dtw_pairs: feat must be a (n_rows, D) float32 GPU tensor (got NoneType)', ''),
    ('dtw_pairs', (M(10, 513), IS, IL, PA, PB), {}, 'dtw_pairs: feat is (10, 513): n_rows >= 1 and 1 <= D <= 512', ''),
    ('dtw_pairs', (M(10, 8)[:, ::2], IS, IL, PA, PB), {}, 'dtw_pairs: feat has strides (8, 2): the columns need stride 1 and the rows at least D = 4 floats apart', ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(metric='cos'), "dtw_pairs: metric 'cos' is none of ['angular', 'euclid', 'kl']", ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(metric=3), "dtw_pairs: metric 3 is none of ['angular', 'euclid', 'kl']", ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(metric=True), "dtw_pairs: metric True is none of ['angular', 'euclid', 'kl']", ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(max_len=65), 'dtw_pairs: max_len must be an integer in [1, 64] (got 65)', ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(max_len=2.0), 'dtw_pairs: max_len must be an integer in [1, 64] (got 2.0)', ''),
    ('dtw_pairs', (FE, M(3, dtype=I64), IL, PA, PB), {}, 'dtw_pairs: item_start must be a contiguous 1-d int32 tensor on the device of the features (got (3,) torch.int64 on meta)', ''),
    ('dtw_pairs', (FE, IS, IL, PA, [0, 1]), {}, 'dtw_pairs: pair_b must be a contiguous 1-d int32 tensor on the device of the features (got list)', ''),
    ('dtw_pairs', (FE, IS, M(2, dtype=I32), PA, PB), {}, 'dtw_pairs: 3 item starts, 2 item lengths: at least one item, as many of each', ''),
    ('dtw_pairs', (FE, IS, IL, PA, M(3, dtype=I32)), {}, 'dtw_pairs: 2 first items, 3 second items: at least one pair, below 2^31, as many of each', ''),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(metric='cos', max_len=0), "dtw_pairs: metric 'cos' is none of ['angular', 'euclid', 'kl']", 'order'),
    ('dtw_pairs', (FE, IS, IL, PA, PB), {}, REACHED, 'good'),
    ('dtw_pairs', (FE, IS, IL, PA, PB), dict(metric=2, max_len=1, want_cost=True), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ abx_count
    ('abx_count', (torch.zeros(9), BK), {}, 'abx_count: dmat must be a contiguous 1-d float32 GPU tensor (got (9,) torch.float32 on cpu)', ''),
    ('abx_count', ([0.0], BK), {}, 'abx_count: dmat must be a contiguous 1-d float32 GPU tensor (got list)', ''),
    ('abx_count', (DM, M(2, 6, dtype=I32)), {}, 'abx_count: blk must be a contiguous 2-d int64 tensor on the device of the features (got (2, 6) torch.int32 on meta)', ''),
    ('abx_count', (DM, M(2, 5, dtype=I64)), {}, 'abx_count: blk is (2, 5) over 9 distances: (NB, 6) with NB >= 1, at least one distance', ''),
    ('abx_count', (M(9, dtype=F64), M(2, 5, dtype=I64)), {}, 'abx_count: dmat must be a contiguous 1-d float32 GPU tensor (got (9,) torch.float64 on meta)', 'order'),
    ('abx_count', (DM, BK), {}, REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ attn_endpoint
    ('attn_endpoint', (torch.zeros(2, 5, 4), [4, 3]), {}, 'attn_endpoint: align must be a (B, S, L) float32 GPU tensor (got (2, 5, 4) torch.float32 on cpu)', ''),
    ('attn_endpoint', (None, [4, 3]), {}, 'attn_endpoint: align must be a (B, S, L) float32 GPU tensor (got NoneType)', ''),
    ('attn_endpoint', (M(2, 5, 2049), [4, 3]), {}, 'attn_endpoint: B=2, S=5, L=2049 outside B >= 1, 1 <= S <= 4096, 1 <= L <= 2048', ''),
    ('attn_endpoint', (AL, [4, 3]), dict(patience=0), 'attn_endpoint: patience must be an integer >= 1 (got 0)', ''),
    ('attn_endpoint', (AL, [4, 3]), dict(max_jump=True), 'attn_endpoint: max_jump must be an integer >= 1 (got True)', ''),
    ('attn_endpoint', (M(2, 5, 8)[:, :, ::2], [4, 3]), {}, 'attn_endpoint: align has strides (40, 8, 2): the last dimension needs stride 1 and rows at least L = 4 floats apart', ''),
    ('attn_endpoint', (AL, M(2)), {}, 'attn_endpoint: enc_len must be (B,) integers on the device of align (got (2,) torch.float32 on meta)', ''),
    ('attn_endpoint', (AL, [0, 4]), {}, 'attn_endpoint: enc_len must be 2 integers in [1, 4] (got [0, 4])', ''),
    ('attn_endpoint', (AL, [4, 5]), {}, 'attn_endpoint: enc_len must be 2 integers in [1, 4] (got [4, 5])', ''),
    ('attn_endpoint', (AL, torch.tensor([4])), {}, 'attn_endpoint: enc_len must be 2 integers in [1, 4] (got [4])', ''),
    ('attn_endpoint', (AL, None), {}, 'attn_endpoint: enc_len must be 2 integers in [1, 4] (got None)', ''),
    ('attn_endpoint', (AL, [0, 0]), dict(patience=0), 'attn_endpoint: patience must be an integer >= 1 (got 0)', 'order'),
    ('attn_endpoint', (AL, [4, 1]), {}, REACHED, 'good'),
    ('attn_endpoint', (AL, M(2, dtype=I32)), dict(patience=1, max_jump=1), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ hyp_edit_distance
    ('hyp_edit_distance', (None, HL, TX, ()), {}, 'hyp_edit_distance: hyp, hyp_len and text must be tensors', ''),
    ('hyp_edit_distance', (torch.zeros(2, 4, dtype=I64), HL, TX, ()), {}, 'hyp_edit_distance: hyp, hyp_len and text must be on one GPU (got cpu, meta, meta)', ''),
    ('hyp_edit_distance', (M(2, 4, dtype=I32), HL, TX, ()), {}, 'hyp_edit_distance: hyp and text must be 2-D int64 (got (2, 4) torch.int32, (2, 3) torch.int64)', ''),
    ('hyp_edit_distance', (HY, M(2, dtype=I64), TX, ()), {}, 'hyp_edit_distance: hyp_len must be (2,) int32 (got (2,) torch.int64)', ''),
    ('hyp_edit_distance', (HY, HL, M(3, 3, dtype=I64), ()), {}, 'hyp_edit_distance: 2 hypotheses, 3 transcripts (at least one)', ''),
    ('hyp_edit_distance', (M(2, 4097, dtype=I64), HL, TX, ()), {}, 'hyp_edit_distance: Lh=4097, L=3, 0 ignored ids outside 1 <= Lh <= 4096, 1 <= L <= 1024, <= 64 ignored ids', ''),
    ('hyp_edit_distance', (HY, HL, TX, (2 ** 31,)), {}, 'hyp_edit_distance: ignored ids must fit int32', ''),
    ('hyp_edit_distance', (M(2, 4, dtype=I32), M(2, dtype=I64), TX, ()), {}, 'hyp_edit_distance: hyp and text must be 2-D int64 (got (2, 4) torch.int32, (2, 3) torch.int64)', 'order'),
    ('hyp_edit_distance', (HY, HL, TX, (0, 1)), {}, REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ edit_align
    ('edit_align', (torch.zeros(2, 3, 4, dtype=I64), EL, ER), {}, 'edit_align: hyp must be an int64 GPU tensor (got (2, 3, 4) torch.int64 on cpu)', ''),
    ('edit_align', (EH, EL, None), {}, 'edit_align: ref must be an int64 GPU tensor (got NoneType)', ''),
    ('edit_align', (EH, EL, H(2, 5, dtype=I64)), {}, 'edit_align: hyp on meta, ref on cpu', ''),
    ('edit_align', (M(2, 4, dtype=I64), EL, ER), {}, 'edit_align: hyp must be (B, N, Lh) and ref (B, Lr) (got (2, 4), (2, 5))', ''),
    ('edit_align', (EH, EL, M(3, 5, dtype=I64)), {}, 'edit_align: 2 utterances of hypotheses, 3 references: they must match', ''),
    ('edit_align', (M(2, 0, 4, dtype=I64), EL, ER), {}, 'edit_align: B=2, N=0 outside B >= 1, N >= 1, B N <= 2^24', ''),
    ('edit_align', (M(2, 3, 1025, dtype=I64), EL, ER), {}, 'edit_align: Lh=1025, Lr=5 outside 1 <= Lh, Lr <= 1024', ''),
    ('edit_align', (EH, EL, ER), dict(n_classes=0), 'edit_align: n_classes must be an integer in [1, 1024] (got 0)', ''),
    ('edit_align', (EH, EL, ER), dict(n_classes=1.5), 'edit_align: n_classes must be an integer in [1, 1024] (got 1.5)', ''),
    ('edit_align', (EH, EL, ER), dict(ignore=5), 'edit_align: ignore must be a sequence of integer ids (got 5)', ''),
    ('edit_align', (EH, EL, ER), dict(ignore=range(65)), 'edit_align: 65 ignored ids, at most 64', ''),
    ('edit_align', (EH, EL, ER), dict(ignore=(-2 ** 31 - 1,)), 'edit_align: ignored ids must fit int32', ''),
    ('edit_align', (EH, EL, ER), dict(confusion=M(3, 3, dtype=I32)), 'edit_align: confusion must be a contiguous (2, 2) int32 tensor on the device of hyp (got (3, 3) torch.int32 on meta)', ''),
    ('edit_align', (EH, EL, ER), dict(confusion='x'), 'edit_align: confusion must be a contiguous (2, 2) int32 tensor on the device of hyp (got str)', ''),
    ('edit_align', (EH, M(2, 3), ER), {}, 'edit_align: hyp_len must be (2, 3) integers on the device of hyp (got (2, 3) torch.float32 on meta)', ''),
    ('edit_align', (EH, [[5, 0, 0], [0, 0, 0]], ER), {}, 'edit_align: hyp_len must be (2, 3) integers in [0, 4] (got [[5, 0, 0], [0, 0, 0]])', ''),
    ('edit_align', (EH, EL, ER), dict(ref_len=M(3, dtype=I32)), 'edit_align: ref_len must be (2,) integers on the device of hyp (got (3,) torch.int32 on meta)', ''),
    ('edit_align', (EH, EL, ER), dict(ref_len=[6, 1]), 'edit_align: ref_len must be (2,) integers in [0, 5] (got [6, 1])', ''),
    ('edit_align', (EH, None, ER), {}, 'edit_align: hyp_len must be (2, 3) integers in [0, 4] (got None)', ''),
    ('edit_align', (EH, [[5, 0, 0], [0, 0, 0]], ER), dict(n_classes=0), 'edit_align: n_classes must be an integer in [1, 1024] (got 0)', 'order'),
    ('edit_align', (EH, EL, ER), {}, REACHED, 'good'),
    ('edit_align', (EH, EL, ER), dict(ref_len=[5, 0], ignore=(0,), n_classes=3, confusion=True, want_ali=False), REACHED, 'good'),
    ('edit_align', (EH, M(2, 3, dtype=I32), ER), dict(confusion=M(2, 2, dtype=I32)), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ vocoder, features, resampling
    # (these refuse by assertion, not by ValueError: only that good input gets to the library is pinned)
    ('stft_fwd', (M(2, 400), 64, 16, 64), {}, REACHED, 'good'),
    ('istft', (M(2, 5, 33, 2), 64, 16, 64), {}, REACHED, 'good'),
    ('griffin_lim', (M(2, 5, 33), M(2, 33, 5), 64, 16, 64), {}, REACHED, 'good'),
    ('mel_to_linear', (M(2, 5, 8), M(8, 33)), {}, REACHED, 'good'),
    ('griffin_lim_batch', (M(2, 5, 8), M(2, 33, 5), 64, 16, 64), dict(basis=M(8, 33), frames=M(2, dtype=I32)), REACHED, 'good'),
    ('audio_features', (W160, [0, 100], [100, 60], 64, 64, 16, 0.97, FB, 8), {}, REACHED, 'good'),
    ('feature_noise', (16, 0, 1, 'meta'), {}, REACHED, 'good'),
    ('audio_mfcc', (W160, [0, 100], [100, 60], 64, 64, 16, 0.97, FB, M(4, 8), 9), {}, REACHED, 'good'),
    ('segment_gather', (M(2, 8, 4), M(3, dtype=I32), M(3, dtype=I32), M(3, dtype=I32), 5), {}, REACHED, 'good'),
    ('resample_batch', (W160, [0, 100], [100, 60], 2, 1, M(1, dtype=I32), M(1, 9), 0, 0), {}, REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ f0_yin
    ('f0_yin', (W160,), dict(F0, hop=2.5), 'f0_yin: hop must be an integer (got 2.5)', ''),
    ('f0_yin', (W160,), dict(F0, W=True), 'f0_yin: W must be an integer (got True)', ''),
    ('f0_yin', (W160,), dict(F0, hop=0), 'f0_yin: hop 0 below 1', ''),
    ('f0_yin', (W160,), dict(F0, tau_min=1), 'f0_yin: lags [1, 40] outside 2 <= tau_min < tau_max <= 1024', ''),
    ('f0_yin', (W160,), dict(F0, W=2049), 'f0_yin: window W = 2049 outside [1, 2048]', ''),
    ('f0_yin', (W160,), dict(F0, threshold=0.0), 'f0_yin: threshold must lie in (0, 1] (got 0.0)', ''),
    ('f0_yin', (W160,), dict(F0, sample_rate=float('inf')), 'f0_yin: sample_rate must be finite and positive (got inf)', ''),
    ('f0_yin', (W160,), dict(F0, lens=[100, 0]), 'f0_yin: lens must be B >= 1 integers in [1, 2^31) (got [100, 0])', ''),
    ('f0_yin', (W160,), dict(F0, lens=[100.0, 60.0]), 'f0_yin: lens must be B >= 1 integers in [1, 2^31) (got [100.0, 60.0])', ''),
    ('f0_yin', (W160,), dict(F0, lens=[], off=[]), 'f0_yin: lens must be B >= 1 integers in [1, 2^31) (got [])', ''),
    ('f0_yin', (torch.zeros(160),), F0, 'f0_yin: x must be a packed 1-D contiguous float32 GPU tensor (got (160,) torch.float32 on cpu)', ''),
    ('f0_yin', (None,), F0, 'f0_yin: x must be a packed 1-D contiguous float32 GPU tensor (got NoneType)', ''),
    ('f0_yin', (W160,), dict(F0, off=[0, 101]), 'f0_yin: an utterance lies outside the 160 packed samples (off [0, 101], lens [100, 60])', ''),
    ('f0_yin', (W160,), dict(F0, T_pad=5), 'f0_yin: T_pad 5 below the 6 frames of the longest utterance', ''),
    ('f0_yin', (W160,), dict(F0, hop=0, threshold=2.0), 'f0_yin: hop 0 below 1', 'order'),
    ('f0_yin', (torch.zeros(160),), dict(F0, lens=[100, 0]), 'f0_yin: lens must be B >= 1 integers in [1, 2^31) (got [100, 0])', 'order'),
    ('f0_yin', (W160,), F0, REACHED, 'good'),
    ('f0_yin', (W160,), dict(F0, tau_min=2, tau_max=1024, W=2048, with_aper=True), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ f0_path_scores
    ('f0_path_scores', (torch.zeros(2, 5), FY, PATH, PLEN), {}, 'f0_path_scores: f0_x must be a (B, T) float32 GPU tensor (got (2, 5) torch.float32 on cpu)', ''),
    ('f0_path_scores', (FX, None, PATH, PLEN), {}, 'f0_path_scores: f0_y must be a (B, T) float32 GPU tensor (got NoneType)', ''),
    ('f0_path_scores', (FX, M(3, 6), PATH, PLEN), {}, 'f0_path_scores: f0_x is (2, 5) on meta, f0_y is (3, 6) on meta: B >= 1 pairs of at least one frame on one device', ''),
    ('f0_path_scores', (M(2, 10)[:, ::2], FY, PATH, PLEN), {}, 'f0_path_scores: f0_x has strides (10, 2): a row needs unit stride', ''),
    ('f0_path_scores', (FX, FY, M(2, 9, 2, dtype=I32), PLEN), {}, 'f0_path_scores: path must be the contiguous (B, Tx + Ty - 1, 2) = (2, 10, 2) int32 tensor of metrics.dtw on the device of the tracks (got (2, 9, 2) torch.int32 on meta)', ''),
    ('f0_path_scores', (FX, FY, None, PLEN), {}, 'f0_path_scores: path must be the contiguous (B, Tx + Ty - 1, 2) = (2, 10, 2) int32 tensor of metrics.dtw on the device of the tracks (got NoneType)', ''),
    ('f0_path_scores', (FX, FY, PATH, M(2, dtype=I64)), {}, 'f0_path_scores: path_len must be the (B,) int32 tensor of metrics.dtw on the device of the tracks (got (2,) torch.int64 on meta)', ''),
    ('f0_path_scores', (FX, FY, PATH, [3, 4]), {}, 'f0_path_scores: path_len must be the (B,) int32 tensor of metrics.dtw on the device of the tracks (got list)', ''),
    ('f0_path_scores', (FX, M(3, 6), None, PLEN), {}, 'f0_path_scores: f0_x is (2, 5) on meta, f0_y is (3, 6) on meta: B >= 1 pairs of at least one frame on one device', 'order'),
    ('f0_path_scores', (FX, FY, PATH, PLEN), {}, REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ trim_silence
    ('trim_silence', (W160,), dict(TR, hop=2.5), 'trim_silence: hop must be an integer (got 2.5)', ''),
    ('trim_silence', (W160,), dict(TR, max_iv=True), 'trim_silence: max_iv must be an integer (got True)', ''),
    ('trim_silence', (W160,), dict(TR, hop=41), 'trim_silence: needs 1 <= hop <= frame_length <= 8192 (hop 41, frame_length 40)', ''),
    ('trim_silence', (W160,), dict(TR, top_db='x'), "trim_silence: top_db must be a finite number (got 'x')", ''),
    ('trim_silence', (W160,), dict(TR, top_db=float('nan')), 'trim_silence: top_db must be a finite number (got nan)', ''),
    ('trim_silence', (W160,), dict(TR, top_db=0.0), 'trim_silence: top_db 0.0 gives the ratio 1.0; it must lie strictly inside (0, 1) in float32', ''),
    ('trim_silence', (W160,), dict(TR, top_db=1000), 'trim_silence: top_db 1000 gives the ratio 0.0; it must lie strictly inside (0, 1) in float32', ''),
    ('trim_silence', (W160,), dict(TR, pad=-1), 'trim_silence: pad -1 outside [0, 2^31)', ''),
    ('trim_silence', (W160,), dict(TR, max_iv=2 ** 30), 'trim_silence: max_iv 1073741824 outside [0, 2^30)', ''),
    ('trim_silence', (W160,), dict(TR, lens=[100, 0]), 'trim_silence: lens must be B >= 1 integers in [1, 2^31) (got [100, 0])', ''),
    ('trim_silence', (W160,), dict(TR, lens=[[100, 60]]), 'trim_silence: lens must be B >= 1 integers in [1, 2^31) (got [[100, 60]])', ''),
    ('trim_silence', (torch.zeros(160),), TR, 'trim_silence: x must be a packed 1-D contiguous float32 GPU tensor (got (160,) torch.float32 on cpu)', ''),
    ('trim_silence', (M(160, dtype=F64),), TR, 'trim_silence: x must be a packed 1-D contiguous float32 GPU tensor (got (160,) torch.float64 on meta)', ''),
    ('trim_silence', (W160,), dict(TR, off=[0, 101]), 'trim_silence: an utterance lies outside the 160 packed samples (off [0, 101], lens [100, 60])', ''),
    ('trim_silence', (W160,), dict(TR, T_pad=5), 'trim_silence: T_pad 5 below the 6 frames of the longest utterance', ''),
    ('trim_silence', (W160,), dict(TR, hop=0, pad=-1), 'trim_silence: needs 1 <= hop <= frame_length <= 8192 (hop 0, frame_length 40)', 'order'),
    ('trim_silence', (None,), dict(TR, off=[0, 101]), 'trim_silence: x must be a packed 1-D contiguous float32 GPU tensor (got NoneType)', 'order'),
    ('trim_silence', (W160,), TR, REACHED, 'good'),
    ('trim_silence', (W160,), dict(TR, pad=3, max_iv=2, T_pad=7, energy=M(2, 7)), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ loudness
    ('loudness', (W4K,), dict(LD, sr=7999), 'loudness: the sample rate must be an integer in [8000, 48000] (got 7999)', ''),
    ('loudness', (W4K,), dict(LD, sr=16000.0), 'loudness: the sample rate must be an integer in [8000, 48000] (got 16000.0)', ''),
    ('loudness', (W4K,), dict(LD, peak_db=float('inf')), 'loudness: peak_db must be a finite number (got inf)', ''),
    ('loudness', (W4K,), dict(LD, max_gain_db='x'), "loudness: max_gain_db must be a finite number (got 'x')", ''),
    ('loudness', (W4K,), dict(LD, target=float('inf')), 'loudness: target must be a finite number, or None / NaN to measure only (got inf)', ''),
    ('loudness', (W4K,), dict(LD, target=True), 'loudness: target must be a finite number, or None / NaN to measure only (got True)', ''),
    ('loudness', (W4K,), dict(LD, lens=[[1]]), 'loudness: lens must be 1 .. 64 integers, one call takes no more utterances (got shape (1, 1), int64)', ''),
    ('loudness', (W4K,), dict(LD, lens=[1.0, 2.0]), 'loudness: lens must be 1 .. 64 integers, one call takes no more utterances (got shape (2,), float64)', ''),
    ('loudness', (W4K,), dict(LD, lens=[1] * 65, off=[0] * 65), 'loudness: lens must be 1 .. 64 integers, one call takes no more utterances (got shape (65,), int64)', ''),
    ('loudness', (W4K,), dict(LD, lens=[2000, 0]), 'loudness: every length must lie in [1, 2^31) (got [2000, 0])', ''),
    ('loudness', (W4K,), dict(LD, H_pad=0), 'loudness: H_pad 0 below the 1 hops of the longest utterance', ''),
    ('loudness', (W4K,), dict(LD, H_pad=1.0), 'loudness: H_pad 1.0 below the 1 hops of the longest utterance', ''),
    ('loudness', (torch.zeros(4000),), LD, 'loudness: x must be a packed 1-D contiguous float32 GPU tensor (got (4000,) torch.float32 on cpu)', ''),
    ('loudness', ('x',), LD, 'loudness: x must be a packed 1-D contiguous float32 GPU tensor (got str)', ''),
    ('loudness', (W4K,), dict(LD, off=[0, 2301]), 'loudness: an utterance lies outside the 4000 packed samples (off [0, 2301], lens [2000, 1700])', ''),
    ('loudness', (W4K,), dict(LD, off=[0]), 'loudness: an utterance lies outside the 4000 packed samples (off [0], lens [2000, 1700])', ''),
    ('loudness', (W4K,), dict(LD, sr=1, lens=[2000, 0]), 'loudness: the sample rate must be an integer in [8000, 48000] (got 1)', 'order'),
    ('loudness', (torch.zeros(4000),), dict(LD, H_pad=0), 'loudness: H_pad 0 below the 1 hops of the longest utterance', 'order'),
    ('loudness', (W4K,), LD, REACHED, 'good'),
    ('loudness', (W4K,), dict(LD, target=-23.0, H_pad=3), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ wave_gain
    ('wave_gain', (W4K,), dict(WG, lens=[2000, 0]), 'wave_gain: lens must be 1 .. 64 integers in [1, 2^31) (got [2000, 0])', ''),
    ('wave_gain', (W4K,), dict(WG, lens=[[2000, 1700]]), 'wave_gain: lens must be 1 .. 64 integers in [1, 2^31) (got [[2000, 1700]])', ''),
    ('wave_gain', (torch.zeros(4000),), WG, 'wave_gain: x must be a packed 1-D contiguous float32 GPU tensor (got (4000,) torch.float32 on cpu)', ''),
    ('wave_gain', (W4K,), dict(WG, off=[-1, 2000]), 'wave_gain: an utterance lies outside the 4000 packed samples (off [-1, 2000], lens [2000, 1700])', ''),
    ('wave_gain', (W4K,), dict(WG, stats=M(2, 7)), 'wave_gain: stats must be the contiguous (2, 8) float32 tensor of loudness() on meta', ''),
    ('wave_gain', (W4K,), dict(WG, stats=None), 'wave_gain: stats must be the contiguous (2, 8) float32 tensor of loudness() on meta', ''),
    ('wave_gain', (W4K,), dict(WG, out=M(4000, dtype=I16)), 'wave_gain: out must be a contiguous 1-D torch.float32 tensor of 4000 samples on meta', ''),
    ('wave_gain', (W4K,), dict(WG, out=M(4000), pcm16=True), 'wave_gain: out must be a contiguous 1-D torch.int16 tensor of 4000 samples on meta', ''),
    ('wave_gain', (W4K,), dict(WG, lens=[2000, 0], stats=None), 'wave_gain: lens must be 1 .. 64 integers in [1, 2^31) (got [2000, 0])', 'order'),
    ('wave_gain', (W4K,), WG, REACHED, 'good'),
    ('wave_gain', (W4K,), dict(WG, out=M(4000, dtype=I16), pcm16=True), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ stoi_batch
    ('stoi_batch', (W1K, M(1000)), dict(ST, lens=[[1]]), 'stoi_batch: lens must be 0 .. 64 integers, one call takes no more pairs (got shape (1, 1), int64)', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, lens=[1.5]), 'stoi_batch: lens must be 0 .. 64 integers, one call takes no more pairs (got shape (1,), float64)', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, lens=[1] * 65, off=[0] * 65), 'stoi_batch: lens must be 0 .. 64 integers, one call takes no more pairs (got shape (65,), int64)', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, lens=[0], off=[0]), 'stoi_batch: every length must lie in [1, 4194304] (got [0])', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, lens=[2 ** 22 + 1], off=[0]), 'stoi_batch: every length must lie in [1, 4194304] (got [4194305])', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, F_pad=1), 'stoi_batch: F_pad 1 below the 2 frames of the longest signal (at least 1)', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, F_pad=2.0), 'stoi_batch: F_pad 2.0 below the 2 frames of the longest signal (at least 1)', ''),
    ('stoi_batch', (W1K, torch.zeros(1000)), ST, "stoi_batch: y must be a packed 1-D contiguous float32 tensor of x's size on x's device (got (1000,) torch.float32 on cpu)", ''),
    ('stoi_batch', (W1K, None), ST, "stoi_batch: y must be a packed 1-D contiguous float32 tensor of x's size on x's device (got NoneType)", ''),
    ('stoi_batch', (None, M(1000)), ST, "stoi_batch: y must be a packed 1-D contiguous float32 tensor of x's size on x's device (got (1000,) torch.float32 on meta)", ''),
    ('stoi_batch', (M(1000, dtype=F64), M(1000)), ST, 'stoi_batch: x must be a packed 1-D contiguous float32 GPU tensor (got (1000,) torch.float64 on meta)', ''),
    ('stoi_batch', (W1K, M(1000)), dict(ST, off=[0, 601]), 'stoi_batch: an utterance lies outside the 1000 packed samples (off [0, 601], lens [500, 400])', ''),
    ('stoi_batch', (W1K, None), dict(ST, lens=[0], off=[0]), 'stoi_batch: every length must lie in [1, 4194304] (got [0])', 'order'),
    ('stoi_batch', (W1K, M(1000)), ST, REACHED, 'good'),
    ('stoi_batch', (W1K, M(1000)), dict(off=[], lens=[], want_parts=True), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ xcorr_delay
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, xlens=[[1]]), 'xcorr_delay: the lengths of x must be 0 .. 64 integers, one call takes no more pairs (got shape (1, 1), int64)', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, ylens=[1.5, 2.5]), 'xcorr_delay: the lengths of y must be 0 .. 64 integers, one call takes no more pairs (got shape (2,), float64)', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, xlens=[0, 1]), 'xcorr_delay: every length of x must lie in [1, 4194304] (got [0, 1])', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, ylens=[2 ** 22 + 1, 1]), 'xcorr_delay: every length of y must lie in [1, 4194304] (got [4194305, 1])', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, ylens=[300], yoff=[0]), 'xcorr_delay: 2 references and 1 processed signals: one of each per pair', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=16385), 'xcorr_delay: max_lag must be an integer in [0, 16384] (got 16385)', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=1.0), 'xcorr_delay: max_lag must be an integer in [0, 16384] (got 1.0)', ''),
    ('xcorr_delay', (torch.zeros(1000),), dict(PR, y=M(1000), max_lag=100), 'xcorr_delay: x must be a packed 1-D contiguous float32 GPU tensor (got (1000,) torch.float32 on cpu)', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=None, max_lag=100), "xcorr_delay: y must be a packed 1-D contiguous float32 tensor on x's device", ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000, dtype=F64), max_lag=100), 'xcorr_delay: x must be a packed 1-D contiguous float32 GPU tensor (got (1000,) torch.float64 on meta)', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, yoff=[0, 301]), 'xcorr_delay: an utterance lies outside the 1000 packed samples (off [0, 301], lens [300, 700])', ''),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=-1, xlens=[0, 1]), 'xcorr_delay: every length of x must lie in [1, 4194304] (got [0, 1])', 'order'),
    ('xcorr_delay', (W1K,), dict(PR, y=M(1000), max_lag=100, want_corr=True), REACHED, 'good'),
    ('xcorr_delay', (W1K,), dict(xoff=[], xlens=[], y=M(1000), yoff=[], ylens=[], max_lag=0), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ sisdr_batch
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), xlens=[[1]]), 'sisdr_batch: the lengths of x must be 0 .. 64 integers, one call takes no more pairs (got shape (1, 1), int64)', ''),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), ylens=[300, 0]), 'sisdr_batch: every length of y must lie in [1, 4194304] (got [300, 0])', ''),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), xlens=[500], xoff=[0]), 'sisdr_batch: 1 references and 2 processed signals: one of each per pair', ''),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), delay=M(2, dtype=I64)), "sisdr_batch: delay must be None or a contiguous (2,) int32 tensor on x's device (got (2,) torch.int64 on meta)", ''),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), delay=[0, 0]), "sisdr_batch: delay must be None or a contiguous (2,) int32 tensor on x's device (got list)", ''),
    ('sisdr_batch', (None,), dict(PR, y=M(1000), delay=M(2, dtype=I32)), "sisdr_batch: delay must be None or a contiguous (2,) int32 tensor on x's device (got (2,) torch.int32 on meta)", ''),
    ('sisdr_batch', (W1K,), dict(PR, y=torch.zeros(1000)), "sisdr_batch: y must be a packed 1-D contiguous float32 tensor on x's device", ''),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), xoff=[0, 601]), 'sisdr_batch: an utterance lies outside the 1000 packed samples (off [0, 601], lens [500, 400])', ''),
    ('sisdr_batch', (torch.zeros(1000),), dict(PR, y=M(1000), delay=[0, 0]), "sisdr_batch: delay must be None or a contiguous (2,) int32 tensor on x's device (got list)", 'order'),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000)), REACHED, 'good'),
    ('sisdr_batch', (W1K,), dict(PR, y=M(1000), delay=M(2, dtype=I32), zero_mean=False), REACHED, 'good'),
    # ------------------------------------------------------------------------------------------------ wave_gather
    ('wave_gather', (S8, [0], D8, [0], [0]), {}, 'wave_gather: lens must be 0 .. 64 integers in [1, 4194304] (got [0])', ''),
    ('wave_gather', (S8, [0], D8, [0], [[1]]), {}, 'wave_gather: lens must be 0 .. 64 integers in [1, 4194304] (got [[1]])', ''),
    ('wave_gather', (S8, [0], D8, [0], [1.0]), {}, 'wave_gather: lens must be 0 .. 64 integers in [1, 4194304] (got [1.0])', ''),
    ('wave_gather', (S8, [0, 1], D8, [0], [5]), {}, 'wave_gather: src_off and dst_off must hold 1 integers each', ''),
    ('wave_gather', (S8, [0], D8, [0.0], [5]), {}, 'wave_gather: src_off and dst_off must hold 1 integers each', ''),
    ('wave_gather', (torch.zeros(8), [0], D8, [0], [5]), {}, 'wave_gather: src must be a contiguous 1-D float32 GPU tensor (got (8,) torch.float32 on cpu)', ''),
    ('wave_gather', (S8, [0], None, [0], [5]), {}, 'wave_gather: dst must be a contiguous 1-D float32 GPU tensor (got NoneType)', ''),
    ('wave_gather', (S8, [0], S8, [0], [5]), {}, 'wave_gather: src and dst must be two different buffers on one device', ''),
    ('wave_gather', (S8, [0], M(8), [0], [5]), {}, 'wave_gather: src and dst must be two different buffers on one device', ''),
    ('wave_gather', (S8, [4], D8, [0], [5]), {}, 'wave_gather: a span lies outside its buffer (src 8 samples, dst 8; src_off [4], dst_off [0], lens [5])', ''),
    ('wave_gather', (S8, [0], D8, [-1], [5]), {}, 'wave_gather: a span lies outside its buffer (src 8 samples, dst 8; src_off [0], dst_off [-1], lens [5])', ''),
    ('wave_gather', (None, [0], D8, [0], [0]), {}, 'wave_gather: lens must be 0 .. 64 integers in [1, 4194304] (got [0])', 'order'),
    ('wave_gather', (S8, [0, 3], D8, [3, 0], [5, 3]), {}, REACHED, 'good'),
]


def _run(row):
    from semi_tts_amd import ops
    name, args, kwargs = row[:3]
    with pytest.raises((ValueError, AssertionError)) as e:
        getattr(ops, name)(*args, **kwargs)
    return e


@pytest.mark.parametrize('i', range(len(TABLE)))
def test_message(no_device, i):
    row = TABLE[i]
    e = _run(row)
    assert str(e.value) == row[3]
    assert isinstance(e.value, AssertionError) == (row[4] == 'good') == (row[3] == REACHED)


def test_every_function_has_an_order_case_and_a_good_case():
    kinds = {}
    for name, _, _, _, kind in TABLE:
        kinds.setdefault(name, set()).add(kind)
    assert len(kinds) == 28
    for name, k in kinds.items():
        assert 'good' in k, name
        assert k == {'good'} or {'', 'order'} <= k, name             # (the functions that refuse by assertion have the good case alone)


# the `raise ValueError` that no row reaches without a device, as (function, its format string): the reason
UNREACHED = {
    ('trim_silence', 'trim_silence: energy must be a contiguous (%d, %d) float32 tensor on %s'):
        'trim_silence loads the library before it looks at `energy`: the refusal comes after the point where these tests stop',
}


def _refusals():
    """{(file, first line, last line): (function, format string)} of every `raise ValueError` in the functions of the table and in the
    helpers of their module(s) that they call.  _p, stream_handle and check are the hot path's, shared with it, and stay outside."""
    from semi_tts_amd import ops
    sites, seen, todo = {}, set(), [getattr(ops, name) for name in sorted({row[0] for row in TABLE})]
    while todo:
        fn = todo.pop()
        if fn in seen:
            continue
        seen.add(fn)
        mod, base = inspect.getmodule(fn), fn.__code__.co_firstlineno - 1
        for node in ast.walk(ast.parse(textwrap.dedent(inspect.getsource(fn)))):
            if isinstance(node, ast.Raise) and isinstance(node.exc, ast.Call) and getattr(node.exc.func, 'id', None) == 'ValueError':
                fmt = [c.value for c in ast.walk(node.exc) if isinstance(c, ast.Constant) and isinstance(c.value, str)][0]
                sites[(fn.__code__.co_filename, base + node.lineno, base + node.end_lineno)] = (fn.__name__, fmt)
            elif isinstance(node, ast.Name) and node.id not in ('_p', 'stream_handle', 'check'):
                callee = getattr(mod, node.id, None)
                if inspect.isfunction(callee) and callee.__module__ in ('semi_tts_amd.ops', 'semi_tts_amd.toolops'):
                    todo.append(callee)
    return sites


def test_every_refusal_is_pinned(no_device):
    sites = _refusals()
    assert len(sites) >= 60                                           # (the walk found the statements)
    hit = set()
    for row in TABLE:
        e = _run(row)
        if isinstance(e.value, ValueError):
            tb = e.tb
            while tb.tb_next is not None:
                tb = tb.tb_next
            where = [s for s in sites if s[0] == tb.tb_frame.f_code.co_filename and s[1] <= tb.tb_lineno <= s[2]]
            assert len(where) == 1, (row[:3], tb.tb_frame.f_code.co_filename, tb.tb_lineno)
            hit.add(where[0])
    assert sorted(sites[s] for s in set(sites) - hit) == sorted(UNREACHED)


# every name of ops that does not begin with two underscores, at 064bfb2.  The three copies of one lengths check that the move to one set
# of argument checks folds -- _ca_lengths, _dtw_lengths, _ea_lengths, which nothing outside ops.py uses -- are the only names left out.
NAMES = [
 'ABX_MAX_D', 'ABX_MAX_LEN', 'ABX_METRICS', 'ACT', 'AE_MAX_L', 'AE_MAX_S', 'C', 'CA_MAX_L', 'CA_MAX_T', 'CA_MAX_V', 'CA_MIN_V', 'CB_MAX_ORDER',
 'CB_MAX_T', 'CB_MAX_TABLE', 'CB_MAX_V', 'CB_MAX_W', 'CB_MIN_V', 'CTC_MAX_TOKENS', 'CTC_TC', 'DTW_MAX_D', 'DTW_MAX_T', 'EA_MAX_IGNORE', 'EA_MAX_L',
 'EA_MAX_V', 'F0_MAX_SPAN', 'F0_MAX_TAU', 'F0_MAX_W', 'F0_RUN', 'FEATURES_MAX_BATCH', 'GED_MAX_IGNORE', 'GED_MAX_L', 'GED_MAX_T', 'GED_MAX_V',
 'GL_CLIP', 'GL_INV_PREEMPHASIS', 'Graph', 'LOUDNESS_FLAGS', 'LOUDNESS_MAX_SR', 'LOUDNESS_MIN_SR', 'LOUDNESS_TABLE_DOUBLES', 'LOUDNESS_THREADS',
 'LSTM_ONE_LAUNCH', 'LSTM_PACKED', 'LSTM_PERSIST', 'LSTM_STEP', 'LSTM_W_NATURAL', 'LSTM_W_PACKED_T', 'LSTM_W_T', 'MEL_MAX', 'MEL_TO_LINEAR_TILE',
 'MFCC_MIN_FRAMES', 'PERSIST_CU_RESERVE', 'POISON_UNINIT', 'RESAMPLE_MAX_STAGE_FLOATS', 'RESAMPLE_MAX_TABLE_FLOATS', 'RESAMPLE_TILE', 'SISDR_CHUNK',
 'STOI_BANDS', 'STOI_BAND_EDGES', 'STOI_CHUNK', 'STOI_FRAME', 'STOI_FS', 'STOI_HOP', 'STOI_MAX_BATCH', 'STOI_MAX_LEN', 'STOI_NFFT', 'STOI_SEG',
 'STOI_SENTINEL', 'StGemmEpilogue', 'StSeg', 'Starved', 'TRIM_CHUNK', 'TRIM_MAX_FRAME_LENGTH', 'TRIM_MAX_SPAN', 'TRIM_RUN', 'WGRAD_DEFER',
 'WGRAD_QMAX', 'XCORR_CHUNK', 'XCORR_LAG_TILE', 'XCORR_MAX_BATCH', 'XCORR_MAX_CHUNKS', 'XCORR_MAX_LAG', 'XCORR_MAX_LEN', '_DEGRADED', '_GRAD_SINK',
 '_G_COUNT', '_G_TASK', '_IGNORE_DEV', '_LAYOUTS', '_PERSIST_STATUS', '_ParamLayouts', '_SIDE_PENDING', '_SIDE_STREAMS', '_WQ', '_WQ_PENDING',
 '_WQ_TASK', '_abx_ints', '_alias', '_audio_ws', '_bn_bank_segs', '_chunks', '_colreduce_ws', '_cur_device', '_dev_index', '_dtw_side', '_f0_check',
 '_fin_job', '_graph_task', '_host_off_lens', '_host_ptr', '_lib', '_loudness_check', '_lstm_run', '_lstm_weights', '_ngram_order_of', '_p',
 '_pair_args', '_pair_check', '_persist_bwd_headroom', '_queue_wgrads', '_raw_stream', '_seg', '_segs', '_stoi_check', '_stream_override',
 '_tap_major', '_trim_check', '_wave_args', '_wave_chunk', '_wave_operands', '_wgrad_job_outputs', 'abx_count', 'act_bwd', 'attn_endpoint',
 'attn_fin', 'attn_fin_split', 'attn_pre', 'attn_pre_job', 'attn_step', 'audio_features', 'audio_mfcc', 'bn_apply', 'bn_bank_bwd', 'bn_bank_bwd_sync',
 'bn_bank_fwd', 'bn_bank_fwd_sync', 'bn_bwd', 'bn_bwd_apply', 'bn_bwd_reduce', 'bn_norm', 'bn_norm_res_mask', 'bn_stats', 'bn_stats_record',
 'bn_sync_merge', 'capturing', 'cat_params', 'check', 'check_handoff', 'check_persist_status', 'colsum', 'contextmanager', 'copy2d', 'copy3d',
 'ctc_beam_search', 'ctc_forced_align', 'ctc_greedy_edit_distance', 'ctc_loss', 'degrade', 'device_info', 'dtw', 'dtw_pairs', 'dx_weight',
 'edit_align', 'f0_path_scores', 'f0_run_length', 'f0_yin', 'feature_noise', 'fill_', 'flush_wgrads', 'frame_lengths', 'gather_rows', 'gemm',
 'gemm_flush', 'gemm_wgrad', 'gemm_wgrad_batch', 'gemm_wgrad_split', 'grad_first', 'grad_slot', 'griffin_lim', 'griffin_lim_batch', 'gru_seq',
 'gru_seq_bwd', 'handoff_starved', 'highway_bwd', 'highway_fwd', 'highway_ht_bwd', 'highway_ht_fwd', 'highway_stack', 'hyp_edit_distance', 'istft',
 'join_side', 'kb16', 'layer_norm', 'layer_norm_bwd', 'linear_small', 'log_softmax', 'log_softmax_bwd', 'loudness', 'loudness_hop',
 'loudness_run_length', 'lstm_cell', 'lstm_cell_job', 'lstm_cell_packed', 'lstm_cell_packed_part', 'lstm_layer', 'lstm_layer_bwd', 'lstm_plan',
 'mean_rows', 'mel_to_linear', 'mt_copy', 'np', 'os', 'pack_weight', 'pack_weight_t', 'packed_linear_job', 'packed_product', 'partial_product',
 'persist_starved', 'persist_status', 'pool_prev_bwd', 'pool_prev_fwd', 'query_attn_fin', 'query_attn_rng', 'resample_batch', 'resample_lds_floats',
 'rowscale_combine', 'scatter_add_rows', 'seg', 'segment_gather', 'set_grad_sink', 'side_pending', 'side_stream', 'sisdr_batch', 'skinny_linear',
 'skinny_linear_packed', 'skinny_linear_packed_attnpre', 'softmax_argmax', 'softmax_bwd', 'stft_fwd', 'stoi_batch', 'stoi_frames', 'stream_handle',
 't16_floats', 't16_view', 'tile_rows', 'torch', 'trim_ratio', 'trim_run_length', 'trim_silence', 'uninit', 'untile_rows', 'untile_tape',
 'use_stream', 'vq_build_table', 'vq_l2', 'vq_mfma_shape', 'vq_pack_table', 'wave_gain', 'wave_gather', 'xcorr_chunk_len', 'xcorr_delay', 'zeros',
]


def test_ops_keeps_its_names():
    from semi_tts_amd import ops
    assert len(NAMES) == len(set(NAMES))
    assert [n for n in NAMES if not hasattr(ops, n)] == []
