"""Thin torch-tensor front end over the C ABI (include/semitts.h).

PyTorch is used only for device memory and stream handles: every function here takes
contiguous fp32 (or int64 index) CUDA/HIP tensors, passes raw device pointers to
libsemitts_hip.so and returns.  There is no eager/CPU fallback -- a CPU tensor raises.
"""
import os
import ctypes as C
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib
from ._lib import StSeg, StGemmEpilogue, check

ACT = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3}

# Debug aid (tests): buffers that are handed to the kernels UNINITIALISED because every element is written before it is read (step tapes
# of the training loops, slab workspaces) are filled with NaN first -- a read of something nobody wrote then shows up in the result.
POISON_UNINIT = False


def uninit(*shape, device, dtype=torch.float32):
    """torch.empty for a buffer whose every element the kernels write before reading it (NaN-filled under POISON_UNINIT)"""
    t = torch.empty(*shape, device=device, dtype=dtype)
    if POISON_UNINIT:
        t.fill_(float('nan'))
    return t

_stream_override = None


def zeros(*shape, device, dtype=torch.float32):
    """torch.zeros through the library's fill launch (a kernel trace of a step then shows no ATen fill; same launch count)"""
    t = torch.empty(*shape, device=device, dtype=dtype)
    if dtype == torch.float32 and t.numel() > 0:
        return fill_(t, 0.0)
    return t.zero_()


def stream_handle():
    """hipStream_t (as int) all st_* calls are issued on: torch's current stream unless overridden."""
    if _stream_override is not None:
        return _stream_override
    # (the raw handle straight from the C side: torch.cuda.current_stream() builds a Stream object through four Python layers -- 10 us a
    # call, ~60 calls per training step and thread, once the host's time per step mattered: DESIGN 3.4)
    return _raw_stream(_cur_device())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)
if _raw_stream is None or _cur_device is None:                 # (an older torch: the public way)
    _raw_stream = lambda _dev: torch.cuda.current_stream().cuda_stream
    _cur_device = lambda: 0


def capturing():
    """st_* calls are being issued on an overridden stream (a hipGraph capture): nothing may read results back now"""
    return _stream_override is not None


class Starved(RuntimeError):
    """a launch whose workgroups hand data to each other was scheduled without all of them resident (a shared or CU-masked GPU):
    its outputs are NaN.  Callers that can, fall back to the multi-launch form and run again (degrade())."""


_DEGRADED = set()


def degrade(what, detail):
    """log -- once per kind -- that an in-launch hand-off was starved and its multi-launch form takes over for the rest of the process"""
    if what not in _DEGRADED:
        _DEGRADED.add(what)
        import warnings
        warnings.warn('semi_tts_amd: %s: the launch was starved of compute units (another tenant or a CU mask on this GPU); falling back '
                      'to %s for the rest of this process' % (what, detail), RuntimeWarning, stacklevel=3)


def handoff_starved(status):
    """True (and the word cleared) if an in-launch hand-off of the decode loop timed out since the word was last cleared.  Reads one
    device word (synchronises)."""
    if status is None:
        return False
    v = int(status.item())
    if v != 0:
        status.zero_()
    return v != 0


def check_handoff(status):
    """Raise if an in-launch hand-off of the decode loop timed out since the word was last cleared (st_decoder_io.handoff_status):
    the waiting workgroups were not co-resident with their producers -- the outputs of that forward are poisoned with NaN.
    Reads one device word (synchronises) and clears it."""
    if status is None:
        return
    v = int(status.item())
    if v != 0:
        status.zero_()
        raise Starved('decode loop: an in-launch hand-off of the processed query timed out (status word 0x%x): the launch was '
                           'starved of compute units; the outputs of this forward are invalid.  Set decoder.attn_pq_in_fin = False '
                           'to run the query projection and the attention as two launches.' % v)


@contextmanager
def use_stream(handle):
    global _stream_override
    prev, _stream_override = _stream_override, handle
    try:
        yield
    finally:
        _stream_override = prev


_SIDE_STREAMS = {}
_SIDE_PENDING = []


def side_stream(device):
    """a second HIP stream per device for work that is independent of the main chain (the detached postnet branch of a training step)"""
    key = str(device)
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return s


def side_pending(event=None):
    """announce (event) / clear (None) side-stream work in flight: kernels that need every compute unit to themselves -- the one-launch
    BiLSTM layers, whose workgroups wait for each other inside the launch -- make their stream wait for it first (join_side)"""
    del _SIDE_PENDING[:]
    if event is not None:
        _SIDE_PENDING.append(event)


def join_side():
    for ev in _SIDE_PENDING:
        torch.cuda.current_stream().wait_event(ev)


def _p(t, dtype=torch.float32):
    """device pointer of a tensor (None -> NULL) after checking it is usable by the kernels"""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('semi_tts_amd: the HIP path needs device tensors (got a CPU tensor); there is no CPU fallback')
    if t.dtype != dtype:
        raise RuntimeError('semi_tts_amd: expected %s, got %s' % (dtype, t.dtype))
    return t.data_ptr()


def _seg(x, w, k=None, ldx=None, ldw=None):
    s = StSeg()
    s.x, s.w = _p(x), _p(w)
    s.k = int(k if k is not None else w.shape[-1])
    s.ldx = int(ldx if ldx is not None else x.stride(-2) if x.dim() > 1 else s.k)
    s.ldw = int(ldw if ldw is not None else w.stride(-2) if w.dim() > 1 else s.k)
    return s


def _segs(pairs):
    arr = (StSeg * len(pairs))()
    for i, s in enumerate(pairs):
        arr[i] = s
    return arr


# ---------------------------------------------------------------------------------------------
def lstm_cell(segs, b_ih, b_hh, c_prev, h_out, c_out, mask=None, pre=None, ldpre=0, gates_out=None,
              ldh=None, ldc=None, ldc_prev=None):
    """segs: list of StSeg (see seg()).  h_out/c_out (B,H) views; writes in place."""
    lib = _lib.load()
    B, H = h_out.shape[0], h_out.shape[-1]
    arr = _segs(segs)
    check(lib.st_lstm_cell_fwd(arr, len(segs), _p(b_ih), _p(b_hh), _p(pre), int(ldpre),
                               _p(c_prev), int(ldc_prev if ldc_prev is not None else (c_prev.stride(0) if c_prev is not None else H)),
                               _p(mask), _p(h_out), int(ldh if ldh is not None else h_out.stride(0)),
                               _p(c_out), int(ldc if ldc is not None else c_out.stride(0)),
                               _p(gates_out), B, H, stream_handle()), 'st_lstm_cell_fwd')


seg = _seg


def skinny_linear(segs, y, bias=None, act=None, mask=None, n_split=0, y2=None, rep=0, N=None):
    lib = _lib.load()
    B = y.shape[0]
    N = int(N if N is not None else y.shape[-1])
    arr = _segs(segs)
    check(lib.st_skinny_linear_fwd(arr, len(segs), _p(bias), ACT[act], _p(mask), int(mask.stride(0)) if mask is not None else 0,
                                   _p(y), int(y.stride(0)), int(n_split), _p(y2), int(y2.stride(0)) if y2 is not None else 0,
                                   int(rep), B, N, stream_handle()), 'st_skinny_linear_fwd')
    return y


def linear_small(x, w, bias=None, act=None, mask=None, out=None):
    """y = act(x W^T + b) * mask for a small number of rows (B <= a few dozen)."""
    if out is None:
        out = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.float32)
    return skinny_linear([_seg(x, w)], out, bias, act, mask)


def attn_step(pq, pm, memory, w_prev, w_cum_prev, w_out, w_cum_out, loc_conv_w, loc_lin_w, v, ctx,
              h_q=None, ada_std=None, ada_mean=None, h_adapt=None):
    B, L, E = memory.shape
    job = _lib.StAttnStepJob()
    job.pq, job.pm, job.memory = _p(pq), _p(pm), _p(memory)
    job.w_prev, job.ld_wprev, job.w_cum_prev = _p(w_prev), int(w_prev.stride(0)), _p(w_cum_prev)
    job.w_out, job.ld_wout, job.w_cum_out = _p(w_out), int(w_out.stride(0)), _p(w_cum_out)
    job.loc_conv_w, job.loc_lin_w, job.v = _p(loc_conv_w), _p(loc_lin_w), _p(v)
    job.ctx, job.ld_ctx = _p(ctx), int(ctx.stride(0))
    if h_q is not None:
        job.h_q, job.ld_hq, job.Q = _p(h_q), int(h_q.stride(0)), h_q.shape[-1]
    job.ada_std, job.ada_mean, job.h_adapt = _p(ada_std), _p(ada_mean), _p(h_adapt)
    job.L, job.A, job.E, job.F, job.K = L, pm.shape[-1], E, loc_conv_w.shape[0], loc_conv_w.shape[2]
    check(_lib.load().st_attn_step_fwd(C.byref(job), B, stream_handle()), 'st_attn_step_fwd')


def attn_pre(pm, w_prev, w_cum_prev, loc_conv_w, loc_lin_w, s_buf=None, parts=1):
    """S = pm + W_l conv([w_prev; w_cum_prev]): the part of the attention step that only needs the previous weights"""
    B, L, A = pm.shape
    F_, _, K = loc_conv_w.shape
    if s_buf is None:
        s_buf = torch.empty(B, L, A, device=pm.device, dtype=torch.float32)
    job = attn_pre_job(pm, w_prev, w_cum_prev, loc_conv_w, loc_lin_w, s_buf, parts)
    check(_lib.load().st_attn_pre_fwd(C.byref(job), B, stream_handle()), 'st_attn_pre_fwd')
    return s_buf


def attn_pre_job(pm, w_prev, w_cum_prev, loc_conv_w, loc_lin_w, s_buf, parts=1):
    """StAttnPreJob of one step (the arguments of attn_pre)"""
    B, L, A = pm.shape
    F_, _, K = loc_conv_w.shape
    return _lib.StAttnPreJob(pm=_p(pm), w_prev=_p(w_prev), ld_wprev=int(w_prev.stride(0)), w_cum_prev=_p(w_cum_prev), loc_conv_w=_p(loc_conv_w),
                             loc_lin_w=_p(loc_lin_w), s_buf=_p(s_buf), L=L, A=A, F=F_, K=K, parts=int(parts))


def _fin_job(s_buf, memory, w_cum_prev, v, w_out, w_cum_out, parts, F_=0, K=0, ctx=None, ctx_t16=None, status=None):
    """StAttnFinJob of one step: the context goes to `ctx` (natural (B, E)) and / or `ctx_t16` (a T16 buffer of (B, E))"""
    B, L, E = memory.shape
    job = _lib.StAttnFinJob()
    job.s_buf, job.memory, job.w_cum_prev = _p(s_buf), _p(memory), _p(w_cum_prev)
    job.w_out, job.ld_wout, job.w_cum_out, job.v = _p(w_out), int(w_out.stride(0)), _p(w_cum_out), _p(v)
    if ctx_t16 is not None:
        job.ctx_dst[0] = t16_view(ctx_t16, K=E)
        job.n_ctx_dst = 1
    if ctx is not None:
        job.ctx, job.ld_ctx = _p(ctx), int(ctx.stride(0))
    job.parts, job.L, job.A, job.E, job.F, job.K = int(parts), L, s_buf.shape[-1], E, int(F_), int(K)
    job.status = _p(status, torch.int32)
    return job


def attn_fin(pq, s_buf, memory, w_cum_prev, v, w_out, w_cum_out, ctx, F_, K, parts=1, ctx_t16=None):
    job = _fin_job(s_buf, memory, w_cum_prev, v, w_out, w_cum_out, parts, F_, K, ctx=ctx, ctx_t16=ctx_t16)
    check(_lib.load().st_attn_fin_fwd(_p(pq), C.byref(job), memory.shape[0], stream_handle()), 'st_attn_fin_fwd')


def attn_fin_split(pq, s_buf, memory, w_cum_prev, v, w_out, w_cum_out, ctx, parts):
    """the fin part over `parts` position ranges + a combine launch (long texts): st_attn_fin_split_fwd"""
    lib = _lib.load()
    B, L, E = memory.shape
    ws = torch.empty(int(lib.st_attn_fin_split_workspace_floats(B, E, int(parts))), device=memory.device, dtype=torch.float32)
    job = _fin_job(s_buf, memory, w_cum_prev, v, w_out, w_cum_out, parts, ctx=ctx)
    check(lib.st_attn_fin_split_fwd(_p(pq), C.byref(job), _p(ws), B, stream_handle()), 'st_attn_fin_split_fwd')


def query_attn_fin(packed_wq, h_q_t16, Q, s_buf, memory, w_cum_prev, v, w_out, w_cum_out, ctx_t16, F_, K, parts=2, epoch=1, granules=None):
    """query projection + attention fin part in ONE launch (pq handed over inside the launch): st_query_attn_fin_fwd.
    h_q_t16 / ctx_t16: T16 buffers of (B, Q) / (B, E); `granules` (B, 2 A floats) must be zero before the first epoch."""
    B, A = memory.shape[0], s_buf.shape[-1]
    if granules is None:
        granules = torch.zeros(B, 2 * A, device=memory.device, dtype=torch.float32)
    job = _fin_job(s_buf, memory, w_cum_prev, v, w_out, w_cum_out, parts, F_, K, ctx_t16=ctx_t16)
    hv = t16_view(h_q_t16, K=Q)
    check(_lib.load().st_query_attn_fin_fwd(_p(packed_wq), C.byref(hv), 16 * kb16(Q), _p(granules), int(epoch), C.byref(job), B, None,
                                            stream_handle()), 'st_query_attn_fin_fwd')
    return granules


def query_attn_rng(packed_wq, h_q_t16, Q, s_buf, memory, w_cum_prev, v, w_out, w_cum_out, ctx_t16, parts, epoch=1, granules=None,
                   xchg=None, status=None):
    """query projection + attention fin part over `parts` position ranges + combine in ONE launch: st_query_attn_rng_fwd.
    `granules` (B, 2 A floats) and `xchg` must be zero before the first epoch; returns them."""
    lib = _lib.load()
    B, L, E = memory.shape
    A = s_buf.shape[-1]
    if granules is None:
        granules = torch.zeros(B, 2 * A, device=memory.device, dtype=torch.float32)
    if xchg is None:
        xchg = torch.zeros(2 * int(lib.st_attn_rng_xchg_words(B, E, int(parts))), device=memory.device, dtype=torch.float32)
    job = _fin_job(s_buf, memory, w_cum_prev, v, w_out, w_cum_out, parts, ctx_t16=ctx_t16, status=status)
    hv = t16_view(h_q_t16, K=Q)
    check(lib.st_query_attn_rng_fwd(_p(packed_wq), C.byref(hv), 16 * kb16(Q), _p(granules), _p(xchg), int(epoch), C.byref(job), B,
                                    stream_handle()), 'st_query_attn_rng_fwd')
    return granules, xchg


class _ParamLayouts:
    """Cached re-layouts of PARAMETERS (a layout change only: mode 0 = Conv1d weight (N, Cin, KT) -> tap-major (N, KT, Cin), the forward
    implicit-GEMM operand; mode 1 = (N, Cin, KT) -> (Cin, KT, N) with the taps reversed, the weight of the input-gradient conv, for
    KT = 1 the transpose of a Linear weight).  Keyed on (storage address, shape, mode); an entry holds a detached alias of the
    parameter (same storage and version counter) and is valid while the version counter has not moved.  When ANY entry is found
    stale (the optimiser has stepped), ALL entries are refreshed by ONE launch (st_relayout_batch): training re-lays out ~40 weights
    per step, one torch copy each in round 2.  Entries nobody asked for during the last 8 epochs (steps) are dropped -- except those a
    hipGraph capture has seen (the graph holds the buffer's address; a refresh rewrites it in place, so a replay after a weight
    update reads the new layout)."""
    MAX_ENTRIES = 1024

    def __init__(self):
        self.entries = {}       # key -> [alias, dst, version, (N, Cin, KT), epoch of the last use, pinned(, row stride of dst)]
        self.cats = {}          # key -> (dst, keys of its parts in `entries`): see get_cat
        self.table = None       # device descriptor table of the entries
        self.blk_desc = None    # descriptor index of every workgroup of the refresh launch
        self.count = 0
        self.total_blocks = 0
        self.dirty = True
        self.refreshes = 0      # launches
        self.epoch = 0          # stale-triggered refreshes (~ optimisation steps)

    def get(self, w, mode):
        key = (w.data_ptr(), tuple(w.shape), mode)
        e = self.entries.get(key)
        if e is not None:
            e[4] = self.epoch
            if capturing():
                e[5] = True                  # a hipGraph now holds this buffer's address: the entry is never dropped (and refreshed in place)
            if e[2] != e[0]._version:
                self.epoch += 1              # (a weight has moved: a new optimisation step -- entries age by these, not by launches)
                e[4] = self.epoch
                self.refresh()
            return e[1]
        N, Cin = int(w.shape[0]), int(w.shape[1])
        KT = int(w.shape[2]) if w.dim() == 3 else 1
        assert w.is_contiguous() and w.dtype == torch.float32
        if len(self.entries) >= self.MAX_ENTRIES:          # (inference-only processes never refresh: bound the table by age)
            for k in [k for k in sorted(self.entries, key=lambda k: self.entries[k][4]) if not self.entries[k][5]][:self.MAX_ENTRIES // 2]:
                del self.entries[k]
        dst = torch.empty((N, KT, Cin) if mode == 0 else (Cin, KT, N), device=w.device, dtype=torch.float32)
        self.entries[key] = [w.detach(), dst, -1, (N, Cin, KT), self.epoch, capturing()]
        self.dirty = True
        self.refresh()
        return dst

    def get_cat(self, ws, mode, pad_to=0):
        """Several parameters of equal Cin laid out side by side as ONE operand: mode 0 -> (sum N, Cin), their rows one after the other
        (the weight of one forward product in place of len(ws); 1-D parameters: their concatenation); mode 1 -> (Cin, sum N), their
        transposes as column blocks (the weight of one input-gradient product).  Same caching and the same single refresh launch as get()."""
        key = (tuple(w.data_ptr() for w in ws), tuple(tuple(w.shape) for w in ws), mode, 'cat', int(pad_to))
        c = self.cats.get(key)
        if c is not None and all(k in self.entries for k in c[1]):
            stale = False
            for k in c[1]:
                e = self.entries[k]
                e[4] = self.epoch
                if capturing():
                    e[5] = True
                stale = stale or e[2] != e[0]._version
            if stale:
                self.epoch += 1
                for k in c[1]:
                    self.entries[k][4] = self.epoch
                self.refresh()
            return c[0]
        one_d = ws[0].dim() == 1
        Ns = [int(w.shape[0]) for w in ws]
        Cin = 1 if one_d else int(ws[0].shape[1])
        assert all(w.is_contiguous() and w.dtype == torch.float32 and w.dim() == ws[0].dim() and (one_d or int(w.shape[1]) == Cin) for w in ws)
        Nt = sum(Ns)
        if pad_to:      # mode 1 only: (Cin, pad_to) with ZERO columns past sum N (a reduction axis padded to whole 16-byte pieces)
            assert mode == 1 and not one_d and pad_to >= Nt
            Nt_alloc = int(pad_to)
            dst = torch.zeros(Cin, Nt_alloc, device=ws[0].device, dtype=torch.float32)
        else:
            Nt_alloc = Nt
            dst = torch.empty((Nt,) if one_d else ((Nt, Cin) if mode == 0 else (Cin, Nt)), device=ws[0].device, dtype=torch.float32)
        keys, off = [], 0
        for w, N in zip(ws, Ns):
            part = dst[off:off + N] if (mode == 0 or one_d) else dst[:, off:off + N]
            k = (w.data_ptr(), tuple(w.shape), mode, 'part', dst.data_ptr(), off)
            self.entries[k] = [w.detach(), part, -1, (N, Cin, 1), self.epoch, capturing(), Nt_alloc if (mode == 1 and not one_d) else 0]
            keys.append(k)
            off += N
        self.cats[key] = (dst, keys)
        self.dirty = True
        self.refresh()
        return dst

    def refresh(self):
        lib = _lib.load()
        self.refreshes += 1
        drop = [k for k, e in self.entries.items() if self.epoch - e[4] > 8 and not e[5]]
        for k in drop:
            del self.entries[k]
            self.dirty = True
        if drop:
            self.cats = {k: c for k, c in self.cats.items() if all(pk in self.entries for pk in c[1])}
        if not self.entries:
            return
        if self.dirty:
            dev = next(iter(self.entries.values()))[1].device
            assert all(e[1].device == dev for e in self.entries.values()), 'parameter layouts of several devices in one process'
            arr = (_lib.StRelayoutDesc * len(self.entries))()
            blk, owner = 0, []
            for j, (d, (key, e)) in enumerate(zip(arr, self.entries.items())):
                N, Cin, KT = e[3]
                d.src, d.dst, d.N, d.Cin, d.KT, d.mode, d.blk0 = e[0].data_ptr(), e[1].data_ptr(), N, Cin, KT, key[2], blk
                d.ld_dst = e[6] if len(e) > 6 else 0
                nb = int(lib.st_relayout_blocks(N, Cin, KT))
                owner += [j] * nb
                blk += nb
            self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            self.blk_desc = torch.tensor(owner, dtype=torch.int32).to(dev)        # the descriptor of every workgroup
            self.count, self.total_blocks, self.dirty = len(self.entries), blk, False
        check(lib.st_relayout_batch(_p(self.table, torch.uint8), self.count, self.total_blocks, _p(self.blk_desc, torch.int32), stream_handle()),
              'st_relayout_batch')
        for e in self.entries.values():
            e[2] = e[0]._version


_LAYOUTS = _ParamLayouts()


def _tap_major(w):
    """Conv1d weight (N, Cin, KT) -> (N, KT, Cin) contiguous (layout change of a PARAMETER; a k-block of the implicit GEMM is then
    16-byte loadable).  Cached per tensor object and version: inference converts a weight once, training once per step -- and then
    all weights in one launch (_ParamLayouts)."""
    if w.is_contiguous() and w.is_cuda and w.dtype == torch.float32:
        return _LAYOUTS.get(w, 0)
    return w.detach().permute(0, 2, 1).contiguous()


def dx_weight(w):
    """the weight operand of the input-gradient product of a conv / linear layer with parameter w ((N, Cin, KT) or (N, Cin)):
    returns (weight, tap_major) for ops.gemm -- the cached (Cin, KT, N) tap-reversed form when the tap-major kernel can take it,
    otherwise torch's permute / flip copy in the Conv1d layout"""
    KT = w.shape[2] if w.dim() == 3 else 1
    N = w.shape[0]
    if w.is_contiguous() and w.is_cuda and w.dtype == torch.float32 and (KT == 1 or (N % 4 == 0 and N >= 16)):
        wt = _LAYOUTS.get(w, 1)
        return (wt.view(wt.shape[0], N), False) if KT == 1 else (wt, True)
    return (w.permute(1, 0, 2).flip(2) if w.dim() == 3 else w.t()).contiguous(), False


def gemm(a, w, out=None, *, Bn=None, Tin=None, Tout=None, pad=0, stride=1, coff=0, bias=None, act_pre=None,
         bn=None, bn_eps=1e-5, act_post=None, res=None, highway_h=None, mask=None, pool_prev=False, w_tap_major=False,
         collect=None):
    """C = epilogue(conv1d / linear).  a: (Bn, Tin, Cin) or (M, Cin) channels-last; w: torch Linear
    (N, Cin) or Conv1d (N, Cin, KT) weight -- or, with w_tap_major, a conv weight already in the tap-major (N, KT, Cin) layout
    (ops.dx_weight).  bn = (mean, var, weight, bias) tensors.  collect: a list -- the job is appended to it instead of being
    launched (ops.gemm_flush(list) then runs all collected jobs, sharing launches where the kernels allow)."""
    lib = _lib.load()
    if a.dim() == 3:
        Bn_, Tin_, Cin = a.shape
    else:
        Bn_, Tin_, Cin = 1, a.shape[0], a.shape[1]
    Bn = Bn or Bn_
    Tin = Tin or Tin_
    KT = (w.shape[1] if w_tap_major else w.shape[2]) if w.dim() == 3 else 1
    N = w.shape[0]
    if w_tap_major:
        assert w.dim() == 3 and w.shape[2] == Cin and w.is_contiguous() and KT > 1 and Cin % 4 == 0
    if Tout is None:
        Tout = (Tin + 2 * pad - KT) // stride + 1
    lda = a.stride(-2)
    if out is None:
        shape = (Bn, Tout, N) if a.dim() == 3 else (Bn * Tout, N)
        out = torch.empty(shape, device=a.device, dtype=torch.float32)
    ldc = out.stride(-2)
    ep = StGemmEpilogue()
    ep.bias = _p(bias)
    ep.act_pre = ACT[act_pre]
    if bn is not None:
        ep.bn_mean, ep.bn_var, ep.bn_w, ep.bn_b = _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3])
    ep.bn_eps = float(bn_eps)
    ep.act_post = ACT[act_post]
    ep.res = _p(res)
    ep.ldres = int(res.stride(-2)) if res is not None else 0
    ep.highway_h = _p(highway_h)
    ep.ldhw = int(highway_h.stride(-2)) if highway_h is not None else 0
    ep.mask = _p(mask)
    ep.ldmask = int(mask.stride(-2)) if mask is not None else 0
    if w_tap_major:
        ep.w_tap_major = 1
    elif KT > 1 and Cin % 4 == 0 and Cin >= 16:
        w = _tap_major(w)
        ep.w_tap_major = 1
    if pool_prev and ep.w_tap_major and a.dim() == 3 and a.is_contiguous() and stride == 1 and a.data_ptr() % 16 == 0 and \
            (Bn, Tin) == (a.shape[0], a.shape[1]):
        # the LDS-DMA kernel cannot take a maximum on the way into LDS: the pooled input becomes a tensor of its own (one elementwise
        # launch, ~10 us for the CBHG's (32, 258, 640) bank output) and the conv runs on the fast kernel (52 against 84 us)
        a, pool_prev = pool_prev_fwd(a), False
    slabs = int(lib.st_gemm_splitk_slabs(int(Bn), int(Tout), int(Cin), int(N), int(KT)))
    ws = None
    if slabs > 1:         # small grid, long reduction: partial products per k range + a finish pass (st_gemm_epilogue.splitk_ws)
        ws = torch.empty(slabs * Bn * Tout * N, device=a.device, dtype=torch.float32)
        ep.splitk_ws, ep.splitk_slabs = _p(ws), slabs
    if collect is not None:
        job = _lib.StGemmJob()
        job.A, job.lda, job.W, job.C, job.ldc, job.coff = _p(a), int(lda), _p(w), _p(out), int(ldc), int(coff)
        job.Bn, job.Tin, job.Tout, job.Cin, job.N, job.KT = int(Bn), int(Tin), int(Tout), int(Cin), int(N), int(KT)
        job.pad, job.stride, job.pool_prev, job.ep = int(pad), int(stride), 1 if pool_prev else 0, ep
        collect.append((job, (a, w, out, ws, bias, bn, res, highway_h, mask)))       # (the tensors stay alive until the flush)
        return out
    check(lib.st_gemm_fwd(_p(a), int(lda), _p(w), _p(out), int(ldc), int(coff), int(Bn), int(Tin), int(Tout),
                          int(Cin), int(N), int(KT), int(pad), int(stride), 1 if pool_prev else 0, C.byref(ep), stream_handle()),
          'st_gemm_fwd')
    return out


def highway_stack(x, layers):
    """eval-mode highway stack in one launch; layers: [(W_H, b_H, W_T, b_T), ...] torch Linear parameters.  None when the shape is
    not one the kernel takes (the caller then runs the layers as GEMM pairs)."""
    lib = _lib.load()
    Cn = int(x.shape[-1])
    if not (x.is_contiguous() and lib.st_highway_stack_supported(Cn, len(layers))) or any(
            tuple(w.shape) != (Cn, Cn) or not w.is_contiguous() for l in layers for w in (l[0], l[2])):
        return None
    n = len(layers)
    arr = lambda k: (C.c_void_p * n)(*[_p(l[k]) for l in layers])
    y = torch.empty_like(x)
    M = x.numel() // Cn
    check(lib.st_highway_stack_fwd(_p(x), Cn, arr(0), arr(1), arr(2), arr(3), n, _p(y), Cn, int(M), Cn, stream_handle()),
          'st_highway_stack_fwd')
    return y


def gemm_flush(collected):
    """run the jobs gathered by ops.gemm(..., collect=list) -- st_gemm_fwd_batch: one launch for up to eight jobs of the pipelined
    kernel (the conv bank), separate launches otherwise"""
    if not collected:
        return
    arr = (_lib.StGemmJob * len(collected))(*[j for j, _ in collected])
    check(_lib.load().st_gemm_fwd_batch(arr, len(collected), stream_handle()), 'st_gemm_fwd_batch')
    del collected[:]


def _colreduce_ws(M, N, device):
    n = int(_lib.load().st_colreduce_workspace_floats(int(M), int(N)))
    return torch.empty(n, device=device, dtype=torch.float32)


def bn_stats(x2d, coff, N, run_mean=None, run_var=None, momentum=0.1, batches_tracked=None):
    """per-column batch statistics of x2d[:, coff:coff+N] (+ running-stat update in place, + `num_batches_tracked` += 1)"""
    lib = _lib.load()
    M = x2d.shape[0]
    mean = torch.empty(N, device=x2d.device, dtype=torch.float32)
    var = torch.empty(N, device=x2d.device, dtype=torch.float32)
    check(lib.st_bn_stats(_p(x2d), int(x2d.stride(0)), int(coff), M, N, _p(mean), _p(var), _p(run_mean), _p(run_var),
                          float(momentum), _p(batches_tracked, torch.int64), _p(_colreduce_ws(M, N, x2d.device)), stream_handle()),
          'st_bn_stats')
    return mean, var


def bn_stats_record(x2d, coff, N, batches_tracked=None):
    """SyncBN, local half: (mean[N], M2[N], row count) of this rank's rows of x2d[:, coff:coff+N], as one (2N + 1) record"""
    M = x2d.shape[0]
    rec = torch.empty(2 * N + 1, device=x2d.device, dtype=torch.float32)
    check(_lib.load().st_bn_stats_record(_p(x2d), int(x2d.stride(0)), int(coff), M, N, _p(rec), _p(batches_tracked, torch.int64),
                                         _p(_colreduce_ws(M, N, x2d.device)), stream_handle()), 'st_bn_stats_record')
    return rec


def bn_sync_merge(rec, N, run_mean=None, run_var=None, momentum=0.1):
    """SyncBN, merged half: the gathered (world, 2N + 1) records -> (mean, var, 1 / global row count) of the global batch in one
    launch (+ running-stat update in place)"""
    world = rec.shape[0]
    assert rec.is_contiguous() and rec.shape[1] == 2 * N + 1
    out = torch.empty(2 * N + 1, device=rec.device, dtype=torch.float32)
    mean, var, inv_total = out[:N], out[N:2 * N], out[2 * N:]
    check(_lib.load().st_bn_sync_merge(_p(rec), world, N, _p(mean), _p(var), _p(run_mean), _p(run_var), float(momentum), _p(inv_total),
                                       stream_handle()), 'st_bn_sync_merge')
    return mean, var, inv_total


def layer_norm(x2d, gamma, beta, eps, want_stats=False):
    """nn.LayerNorm over the last dimension of (M, N) rows -> y [, mean (M), rstd (M)]"""
    M, N = x2d.shape
    y = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    mean = torch.empty(M, device=x2d.device, dtype=torch.float32) if want_stats else None
    rstd = torch.empty(M, device=x2d.device, dtype=torch.float32) if want_stats else None
    check(_lib.load().st_layer_norm_fwd(_p(x2d), int(x2d.stride(0)), _p(gamma), _p(beta), float(eps), _p(y), N, _p(mean), _p(rstd), M, N,
                                        stream_handle()), 'st_layer_norm_fwd')
    return (y, mean, rstd) if want_stats else y


def layer_norm_bwd(dy2d, x2d, gamma, mean, rstd):
    """-> (dx, dy * xhat): d gamma = colsum(dy * xhat), d beta = colsum(dy)"""
    M, N = x2d.shape
    dx = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    dyxhat = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    check(_lib.load().st_layer_norm_bwd(_p(dy2d), int(dy2d.stride(0)), _p(x2d), int(x2d.stride(0)), _p(gamma), _p(mean), _p(rstd),
                                        _p(dx), N, _p(dyxhat), M, N, stream_handle()), 'st_layer_norm_bwd')
    return dx, dyxhat


def log_softmax(x):
    N = x.shape[-1]
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().st_log_softmax_fwd(_p(x), _p(y), x.numel() // N, N, stream_handle()), 'st_log_softmax_fwd')
    return y


def log_softmax_bwd(dy, y):
    N = y.shape[-1]
    dx = torch.empty_like(y)
    check(_lib.load().st_log_softmax_bwd(_p(dy.contiguous()), _p(y), _p(dx), y.numel() // N, N, stream_handle()), 'st_log_softmax_bwd')
    return dx


def bn_apply(x2d, coff, N, mean, var, w, b, eps, act=None):
    lib = _lib.load()
    check(lib.st_bn_apply(_p(x2d), int(x2d.stride(0)), int(coff), x2d.shape[0], N, _p(mean), _p(var), _p(w), _p(b),
                          float(eps), ACT[act], stream_handle()), 'st_bn_apply')


LSTM_PERSIST = True      # bidirectional LSTM layers as one launch for all steps where st_lstm_seq_variant takes the shape (the jobs' allow_persist)
_PERSIST_STATUS = {}


def _dev_index(device):
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def persist_status(device):
    """the device word the one-launch recurrent layers report a starved launch in (bit 1); see check_persist_status"""
    key = _dev_index(device)
    t = _PERSIST_STATUS.get(key)
    if t is None:
        t = _PERSIST_STATUS[key] = torch.zeros(1, device=torch.device('cuda', key), dtype=torch.int32)
    return t


def persist_starved(device=None):
    """True (and the word cleared) if a one-launch recurrent layer gave up waiting for its neighbour workgroups since the last check.
    Reads one device word per device (synchronises)."""
    hit = False
    for key, t in list(_PERSIST_STATUS.items()):
        if device is not None and key != _dev_index(device):
            continue
        if int(t.item()):
            t.zero_()
            hit = True
    return hit


def check_persist_status(device=None):
    """Raise if a one-launch recurrent layer gave up waiting for its neighbour workgroups since the last check (the launch was starved
    of compute units; the rows it produced are NaN).  Reads one device word per device (synchronises) and clears it."""
    for key, t in list(_PERSIST_STATUS.items()):
        if device is not None and key != _dev_index(device):
            continue
        v = int(t.item())
        if v:
            t.zero_()
            raise Starved('one-launch LSTM layer: a wait for the hidden state timed out (status word 0x%x): the launch was starved '
                               'of compute units and its outputs are NaN.  Set semi_tts_amd.ops.LSTM_PERSIST = False to run the layer '
                               'as one launch per time step.' % v)


LSTM_STEP, LSTM_PACKED, LSTM_ONE_LAUNCH = 0, 1, 2        # ST_LSTM_STEP / _PACKED / _PERSIST of include/semitts.h
LSTM_W_NATURAL, LSTM_W_T, LSTM_W_PACKED_T = 0, 1, 2      # ST_LSTM_W_*


def lstm_plan(backward, ndir, x, cols, H, aligned_ops, cu_reserve=0):
    """st_lstm_seq_variant for the (B, T, >= cols[d] + H) output (forward) or output gradient (backward) x: the form the layer takes, the
    weight layout and workspace it needs.  aligned_ops: the operands of the ST_LSTM_AL_* bits, in bit order."""
    B, T = x.shape[:2]
    if x.stride(2) != 1 or x.stride(0) != T * x.stride(1):
        raise ValueError('semi_tts_amd: LSTM layer: a (B, T, ld) tensor with strides (T * ld, ld, 1) is needed, got %s' % (tuple(x.stride()),))
    q = _lib.StLstmSeqQuery(int(bool(backward)), ndir, B, T, H, int(x.stride(1)), (C.c_int * 2)(*cols),
                            sum(1 << i for i, t in enumerate(aligned_ops) if t.data_ptr() % 16 == 0), 1 if LSTM_PERSIST else 0, 0, cu_reserve)
    plan = _lib.StLstmSeqPlan()
    if _lib.load().st_lstm_seq_variant(C.byref(q), C.byref(plan)):
        raise ValueError('semi_tts_amd: no LSTM layer form takes ndir=%d B=%d T=%d H=%d ld=%d cols=%s' % (ndir, B, T, H, x.stride(1), tuple(cols)))
    return plan


def _lstm_weights(w_hhs):
    if not all(w.is_contiguous() for w in w_hhs):
        raise ValueError('semi_tts_amd: LSTM layer: the recurrent weights must be contiguous')
    return [w.detach() for w in w_hhs]


def _lstm_run(entry, j, plan, device):
    if plan.form == LSTM_ONE_LAUNCH:
        join_side()               # (its workgroups wait for each other inside the launch: nothing else may hold compute units meanwhile)
        j.status = _p(persist_status(device), torch.int32)
    ws = torch.empty(plan.ws_floats, device=device, dtype=torch.float32) if plan.ws_floats else None
    j.ws = _p(ws)
    check(getattr(_lib.load(), entry)(C.byref(j), stream_handle()), entry)


def lstm_layer(xprojs, w_hhs, b_hhs, out, gates_tapes=None, c_tapes=None, reverse=False, ocols=None):
    """One nn.LSTM layer over its input projections xprojs[d] (B,T,4H), ndir = len(xprojs) directions: out(:, :, ocols[d] : ocols[d]+H) =
    h of direction d (default: direction d in columns [d H, (d+1) H)).  One direction walks forward in time, or backward with `reverse`;
    of two, the second walks backward.  One launch for the whole layer where st_lstm_seq_variant says so, else one launch per time step."""
    ndir = len(xprojs)
    B, T, H4 = xprojs[0].shape
    H = H4 // 4
    w_hhs = _lstm_weights(w_hhs)
    j = _lib.StLstmSeqJob(ndir=ndir, reverse=1 if reverse else 0, out=_p(out), ldo=int(out.stride(1)), B=B, T=T, H=H,
                          allow_persist=1 if LSTM_PERSIST else 0)
    for d in range(ndir):
        j.xproj[d], j.w_hh[d], j.b_hh[d], j.ocol[d] = _p(xprojs[d]), _p(w_hhs[d]), _p(b_hhs[d]), d * H if ocols is None else int(ocols[d])
        j.gates_tape[d] = _p(gates_tapes[d]) if gates_tapes is not None else None
        j.c_tape[d] = _p(c_tapes[d]) if c_tapes is not None else None
    plan = lstm_plan(False, ndir, out, j.ocol, H, [out] + w_hhs)
    _lstm_run('st_lstm_seq_fwd', j, plan, out.device)


PERSIST_CU_RESERVE = int(os.environ.get('ST_PERSIST_CU_RESERVE', '32'))      # compute units left to RCCL's channels beside the one-launch BiLSTM backward


def _persist_bwd_headroom():
    """Compute units the one-launch BiLSTM backward must leave free.  It needs all of its workgroups co-resident, and under data
    parallelism the decoder's gradient buckets are all-reduced by RCCL kernels on another stream exactly while the encoder's BiLSTM
    backward runs (advisor, round 5): with more than one rank and asynchronous buckets in flight the launch leaves PERSIST_CU_RESERVE
    compute units free, or the per-step form runs instead (a starved launch costs a skipped step and switches LSTM_PERSIST off for good)."""
    sink = _GRAD_SINK
    if sink is None or not getattr(sink, '_active', False) or not any(w is not None for w in getattr(sink, 'works', ())):
        return 0
    try:
        import torch.distributed as dist
        return PERSIST_CU_RESERVE if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 else 0
    except Exception:
        return 0


def lstm_layer_bwd(dout, gates_tapes, c_tapes, w_hhs, reverse=False, dcols=None):
    """Backward through time of lstm_layer: dout (B,T,>= dcols[d]+H) -> [dxproj of direction d (B,T,4H)].  w_hhs: the W_hh parameters
    (4H, H); the layout the form st_lstm_seq_variant chooses needs (transposed, packed) is built here."""
    ndir = len(gates_tapes)
    T, B, _, H = gates_tapes[0].shape
    w_hhs = _lstm_weights(w_hhs)
    dx = list(torch.empty(ndir, B, T, 4 * H, device=dout.device, dtype=torch.float32).unbind(0))      # (back to back: one sentinel fill)
    j = _lib.StLstmSeqBwdJob(ndir=ndir, reverse=1 if reverse else 0, dout=_p(dout), ldd=int(dout.stride(1)), B=B, T=T, H=H,
                             allow_persist=1 if LSTM_PERSIST else 0, cu_reserve=_persist_bwd_headroom() if LSTM_PERSIST and ndir == 2 else 0)
    for d in range(ndir):
        j.dcol[d], j.gates_tape[d], j.c_tape[d], j.dxproj[d] = d * H if dcols is None else int(dcols[d]), _p(gates_tapes[d]), _p(c_tapes[d]), _p(dx[d])
    plan = lstm_plan(True, ndir, dout, j.dcol, H, [dout] + list(gates_tapes) + list(c_tapes) + dx, j.cu_reserve)
    if plan.weights == LSTM_W_T:
        ws_w = [dx_weight(w)[0] for w in w_hhs]                 # W_hh^T (H, 4H)
    elif plan.weights == LSTM_W_PACKED_T:
        ws_w = [pack_weight_t([w]) for w in w_hhs]              # W_hh^T in MFMA order: N = H, K = 4H
    else:
        ws_w = w_hhs
    j.weights = plan.weights
    for d in range(ndir):
        j.w[d] = _p(ws_w[d])
    _lstm_run('st_lstm_seq_bwd', j, plan, dout.device)
    return dx


def gru_seq(gi_f, gi_b, w_hh_f, w_hh_b, b_hh_f, b_hh_b, out, tape=None):
    lib = _lib.load()
    B, T, H3 = gi_f.shape
    ndir = 2 if gi_b is not None else 1
    check(lib.st_gru_seq_fwd(_p(gi_f), _p(gi_b), _p(w_hh_f), _p(w_hh_b), _p(b_hh_f), _p(b_hh_b), _p(out),
                             int(out.stride(1)), _p(tape), B, T, H3 // 3, ndir, stream_handle()), 'st_gru_seq_fwd')


def gru_seq_bwd(dout, out, tape, w_hh_f, w_hh_b):
    """returns (dgi_f, dgi_b, dgh_f, dgh_b), each (B,T,3H)"""
    ndir, B, T, _, H = tape.shape
    mk = lambda: torch.empty(B, T, 3 * H, device=dout.device, dtype=torch.float32)
    dgi_f, dgh_f = mk(), mk()
    dgi_b, dgh_b = (mk(), mk()) if ndir == 2 else (None, None)
    check(_lib.load().st_gru_seq_bwd(_p(dout), int(dout.stride(1)), _p(out), int(out.stride(1)), _p(tape), _p(w_hh_f),
                                     _p(w_hh_b), _p(dgi_f), _p(dgi_b), _p(dgh_f), _p(dgh_b), B, T, H, ndir,
                                     stream_handle()), 'st_gru_seq_bwd')
    return dgi_f, dgi_b, dgh_f, dgh_b


def vq_build_table(learnable, attr=None, attr_w=None, attr_b=None):
    lib = _lib.load()
    V, Dl = learnable.shape
    Da = attr_w.shape[0] if attr_w is not None else 0
    table = torch.empty(V, Dl + Da, device=learnable.device, dtype=torch.float32)
    check(lib.st_vq_build_table(_p(learnable), Dl, _p(attr), attr.shape[1] if attr is not None else 0, _p(attr_w),
                                _p(attr_b), Da, _p(table), V, stream_handle()), 'st_vq_build_table')
    return table


def gather_rows(table, idx):
    lib = _lib.load()
    V, D = table.shape
    idx = idx.contiguous()
    out = torch.empty(tuple(idx.shape) + (D,), device=table.device, dtype=torch.float32)
    check(lib.st_gather_rows(_p(table), _p(idx, torch.int64), _p(out), idx.numel(), D, V, stream_handle()), 'st_gather_rows')
    return out


def vq_mfma_shape(D, V):
    """shapes the matrix-core nearest-code search takes (st_vq_pack_table / st_vq_l2_packed_fwd)"""
    return D <= 64 and D % 4 == 0 and V <= 1024


def vq_pack_table(table):
    """MFMA-order copy of a (V, D) code table: made once per table version (embed.L2Embedding caches it), not per lookup"""
    lib = _lib.load()
    V, D = table.shape
    packed = torch.empty(int(lib.st_vq_l2_workspace_floats(D, V)), device=table.device, dtype=torch.float32)
    check(lib.st_vq_pack_table(_p(table), _p(packed), D, V, stream_handle()), 'st_vq_pack_table')
    return packed


def vq_l2(x, table, temp, scalar_kernel=False, packed=None):
    """scalar_kernel=True (tests): the LDS-table kernel instead of the matrix-core one; packed: vq_pack_table(table)"""
    lib = _lib.load()
    lead, D = x.shape[:-1], x.shape[-1]
    V = table.shape[0]
    n = x.numel() // D
    p = torch.empty(tuple(lead) + (V,), device=x.device, dtype=torch.float32)
    idx = torch.empty(tuple(lead), device=x.device, dtype=torch.int64)
    out = torch.empty_like(x)
    if packed is not None and not scalar_kernel:
        check(lib.st_vq_l2_packed_fwd(_p(x), _p(table), _p(packed), _p(temp), _p(p), _p(idx, torch.int64), _p(out), n, D, V,
                                      stream_handle()), 'st_vq_l2_packed_fwd')
        return p, idx, out
    ws = None if scalar_kernel else torch.empty(int(lib.st_vq_l2_workspace_floats(D, V)), device=x.device, dtype=torch.float32)
    check(lib.st_vq_l2_fwd(_p(x), _p(table), _p(temp), _p(p), _p(idx, torch.int64), _p(out), _p(ws), n, D, V, stream_handle()),
          'st_vq_l2_fwd')
    return p, idx, out


def softmax_bwd(p, dp, scale=1.0, relu_scale=None, want_rowsum=False):
    """dz = s * p * (dp - sum(dp * p, -1)) with s = scale * relu(relu_scale[0]); optionally also dz.sum(-1)"""
    V = p.shape[-1]
    n = p.numel() // V
    dz = torch.empty_like(p)
    rs = torch.empty(p.shape[:-1], device=p.device, dtype=torch.float32) if want_rowsum else None
    check(_lib.load().st_softmax_bwd(_p(p), _p(dp), _p(relu_scale), float(scale), _p(dz), _p(rs), n, V, stream_handle()), 'st_softmax_bwd')
    return (dz, rs) if want_rowsum else dz


def rowscale_combine(a, alpha, x=None, r=None, beta=0.0, c=None):
    """alpha * a + beta * r[:, None] * x (+ c), all (M, D) row-major"""
    M, D = a.shape
    out = torch.empty_like(a)
    check(_lib.load().st_rowscale_combine(_p(a), float(alpha), _p(x), _p(r), float(beta), _p(c), _p(out), M, D, stream_handle()),
          'st_rowscale_combine')
    return out


CTC_MAX_TOKENS, CTC_TC = 127, 16      # st_ctc_loss: the longest transcript (one thread per blank-extended state), the frames per tile


def ctc_loss(prob, text, eps, want_grad=True, log_input=False, in_len=None, dprob=None):
    """-> (loss scalar tensor, d loss / d prob or None); see st_ctc_loss (log_input: prob holds log-probabilities).
    in_len: (B,) int32 device tensor, utterance b uses its first clamp(in_len[b], 0, T) frames (st_ctc_loss_len); None: every frame.
    dprob: a caller's (B, T, V) buffer for the gradient (every element is written)."""
    lib = _lib.load()
    B, T, V = prob.shape
    L = text.shape[1]
    loss = torch.empty((), device=prob.device, dtype=torch.float32)
    if dprob is not None:
        if tuple(dprob.shape) != (B, T, V) or not dprob.is_contiguous():
            raise ValueError('ctc_loss: dprob must be a contiguous (B, T, V) buffer')
    elif want_grad:
        dprob = torch.empty_like(prob)
    ws = torch.empty(int(lib.st_ctc_workspace_floats(B, T)), device=prob.device, dtype=torch.float32)
    if in_len is None:
        check(lib.st_ctc_loss(_p(prob), _p(text, torch.int64), float(eps), _p(loss), _p(dprob), _p(ws), B, T, V, L, 1 if log_input else 0,
                              stream_handle()), 'st_ctc_loss')
    else:
        if tuple(in_len.shape) != (B,) or not in_len.is_contiguous():
            raise ValueError('ctc_loss: in_len must be a contiguous (B,) int32 tensor')
        check(lib.st_ctc_loss_len(_p(prob), _p(text, torch.int64), _p(in_len, torch.int32), float(eps), _p(loss), _p(dprob), _p(ws),
                                  B, T, V, L, 1 if log_input else 0, stream_handle()), 'st_ctc_loss_len')
    return loss, dprob


def frame_lengths(x=None, pad_value=0.0, div=1, text=None, r=1):
    """(B,) int32 frame counts for ctc_loss(in_len=...), on the device, one launch, no host read (see st_frame_lengths):
    x (B, T, D) fp32 -> (frames of x[b] not entirely == pad_value) // div;
    text (B, L) int64 (x None) -> 1 + (len6 + len6 % r) // div with len6 = 6 * nonzero(text[b]): the text-first branch"""
    if (x is None) == (text is None):
        raise ValueError('frame_lengths: either x or text')
    src = x if x is not None else text
    if src.dim() != (3 if x is not None else 2) or not src.is_contiguous():
        raise ValueError('frame_lengths: a contiguous (B, T, D) spectrogram or (B, L) text')
    B = src.shape[0]
    out = torch.empty(B, device=src.device, dtype=torch.int32)
    if x is not None:
        check(_lib.load().st_frame_lengths(_p(x), B, x.shape[1], x.shape[2], float(pad_value), None, 0, 1, int(div), _p(out, torch.int32),
                                           stream_handle()), 'st_frame_lengths')
    else:
        check(_lib.load().st_frame_lengths(None, B, 0, 0, 0.0, _p(text, torch.int64), text.shape[1], int(r), int(div), _p(out, torch.int32),
                                           stream_handle()), 'st_frame_lengths')
    return out


GED_MAX_T, GED_MAX_V, GED_MAX_L, GED_MAX_IGNORE = 4096, 10240, 1024, 64      # st_ctc_greedy_edit_distance's limits
_IGNORE_DEV = {}


def ctc_greedy_edit_distance(prob, text, ignore, want_hyp=False):
    """greedy CTC transcript of `prob` and its edit distance to `text`, per utterance (see st_ctc_greedy_edit_distance):
    prob (B, T, V) fp32 posteriors / log-posteriors, or (B, T) int64 ids already argmaxed (st_ids_edit_distance); text (B, L) int64;
    ignore: the ids dropped from both sides.  -> (dist, ref_len) int32 (B,) device tensors [+ (hyp (B, T) int64, hyp_len (B,) int32)
    with want_hyp].  One launch, no host read.  Anything the kernel would refuse raises ValueError before the launch."""
    if not (torch.is_tensor(prob) and torch.is_tensor(text)):
        raise ValueError('ctc_greedy_edit_distance: prob and text must be tensors')
    if not (prob.is_cuda and text.is_cuda and prob.device == text.device):
        raise ValueError('ctc_greedy_edit_distance: prob and text must be on one GPU (got %s, %s)' % (prob.device, text.device))
    ids = prob.dim() == 2
    if ids and prob.dtype != torch.int64 or not ids and (prob.dim() != 3 or prob.dtype != torch.float32):
        raise ValueError('ctc_greedy_edit_distance: prob must be (B, T, V) float32 or (B, T) int64 (got %s %s)'
                         % (tuple(prob.shape), prob.dtype))
    if text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('ctc_greedy_edit_distance: text must be (B, L) int64 (got %s %s)' % (tuple(text.shape), text.dtype))
    B, T = prob.shape[:2]
    V = 0 if ids else prob.shape[2]
    L = text.shape[1]
    ignore = tuple(int(i) for i in ignore)
    if text.shape[0] != B or B < 1:
        raise ValueError('ctc_greedy_edit_distance: %d utterances of prob, %d of text (at least one)' % (B, text.shape[0]))
    if not (1 <= T <= GED_MAX_T and (ids or 1 <= V <= GED_MAX_V) and 1 <= L <= GED_MAX_L and len(ignore) <= GED_MAX_IGNORE):
        raise ValueError('ctc_greedy_edit_distance: T=%d, V=%d, L=%d, %d ignored ids outside 1 <= T <= %d, 1 <= V <= %d, 1 <= L <= %d, '
                         '<= %d ignored ids' % (T, V, L, len(ignore), GED_MAX_T, GED_MAX_V, GED_MAX_L, GED_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('ctc_greedy_edit_distance: ignored ids must fit int32')
    dev = prob.device
    ign = _IGNORE_DEV.get((dev, ignore))
    if ign is None:
        ign = _IGNORE_DEV[(dev, ignore)] = torch.tensor(ignore if ignore else [0], dtype=torch.int32).to(dev)
    prob, text = prob.contiguous(), text.contiguous()
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    ref_len = torch.empty(B, device=dev, dtype=torch.int32)
    hyp = torch.empty(B, T, device=dev, dtype=torch.int64) if want_hyp else None
    hyp_len = torch.empty(B, device=dev, dtype=torch.int32) if want_hyp else None
    lib = _lib.load()
    if ids:
        check(lib.st_ids_edit_distance(_p(prob, torch.int64), B, T, _p(text, torch.int64), L, _p(ign, torch.int32), len(ignore),
                                       _p(dist, torch.int32), _p(ref_len, torch.int32), _p(hyp, torch.int64), _p(hyp_len, torch.int32),
                                       stream_handle()), 'st_ids_edit_distance')
    else:
        check(lib.st_ctc_greedy_edit_distance(_p(prob), B, T, V, _p(text, torch.int64), L, _p(ign, torch.int32), len(ignore),
                                              _p(dist, torch.int32), _p(ref_len, torch.int32), _p(hyp, torch.int64), _p(hyp_len, torch.int32),
                                              stream_handle()), 'st_ctc_greedy_edit_distance')
    return (dist, ref_len, hyp, hyp_len) if want_hyp else (dist, ref_len)


CB_MAX_T, CB_MIN_V, CB_MAX_V, CB_MAX_W = 4096, 2, 1024, 128          # st_ctc_beam_search's limits
from .ngram import MAX_ORDER as CB_MAX_ORDER, MAX_TABLE as CB_MAX_TABLE, order_of as _ngram_order_of   # noqa: E402  (st_ctc_beam_search_lm's limits)


def ctc_beam_search(prob, lengths=None, beam_width=16, top_paths=1, blank=0, log_input=False, eps=1e-10, bonus=None, order=None, bos=1):
    """CTC prefix beam search of prob (B, T, V) fp32 on one GPU (see st_ctc_beam_search).  lengths: None (all T frames), or (B,) integer
    frame counts -- a host tensor / sequence is checked against [0, T] here, a device tensor is taken as it is (the kernel clamps it).
    -> (hyp (B, top_paths, T) int64 0-padded, hyp_len (B, top_paths) int32, score (B, top_paths) float32) device tensors; one launch,
    no host read.  bonus: None (st_ctc_beam_search, the acoustic search), or the fused n-gram table of st_ctc_beam_search_lm: a contiguous
    (V^(order-1), V) float32 tensor on the device of prob (order: None = from the shape; bos: the start id of the empty prefix's
    context); its values are not read here.  Anything the kernel would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(prob) or not prob.is_cuda or prob.dim() != 3 or prob.dtype != torch.float32:
        raise ValueError('ctc_beam_search: prob must be a (B, T, V) float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(prob.shape), prob.dtype, prob.device) if torch.is_tensor(prob) else type(prob).__name__))
    B, T, V = prob.shape
    W, N, blank = int(beam_width), int(top_paths), int(blank)
    if B < 1 or not (1 <= T <= CB_MAX_T and CB_MIN_V <= V <= CB_MAX_V):
        raise ValueError('ctc_beam_search: B=%d, T=%d, V=%d outside B >= 1, 1 <= T <= %d, %d <= V <= %d' % (B, T, V, CB_MAX_T, CB_MIN_V, CB_MAX_V))
    if not (1 <= W <= CB_MAX_W and 1 <= N <= W):
        raise ValueError('ctc_beam_search: need 1 <= top_paths <= beam_width <= %d (beam_width %d, top_paths %d)' % (CB_MAX_W, W, N))
    if not 0 <= blank < V:
        raise ValueError('ctc_beam_search: blank %d outside [0, %d)' % (blank, V))
    if not eps >= 0.0:
        raise ValueError('ctc_beam_search: eps must be >= 0 (got %r)' % (eps,))
    dev = prob.device
    if bonus is not None:
        if not torch.is_tensor(bonus) or not bonus.is_cuda or bonus.device != dev or bonus.dim() != 2 or bonus.dtype != torch.float32 \
                or not bonus.is_contiguous():
            raise ValueError('ctc_beam_search: bonus must be a contiguous (V^(order-1), V) float32 tensor on the device of prob (got %s)'
                             % ('%s %s on %s' % (tuple(bonus.shape), bonus.dtype, bonus.device) if torch.is_tensor(bonus)
                                else type(bonus).__name__))
        found = _ngram_order_of(bonus.shape[0], V) if bonus.shape[1] == V else None
        if found is None:
            raise ValueError('ctc_beam_search: a bonus table of shape %s is no (V^(order-1), V) table for V = %d, 1 <= order <= %d'
                             % (tuple(bonus.shape), V, CB_MAX_ORDER))
        if order is not None and int(order) != found:
            raise ValueError('ctc_beam_search: order %r, but the bonus table of shape %s has order %d' % (order, tuple(bonus.shape), found))
        order, bos = found, int(bos)
        if V ** order > CB_MAX_TABLE:
            raise ValueError('ctc_beam_search: V^order = %d^%d table elements, at most 2^26' % (V, order))
        if not 0 <= bos < V:
            raise ValueError('ctc_beam_search: bos %d outside [0, %d)' % (bos, V))
    elif order is not None:
        raise ValueError('ctc_beam_search: order %r without a bonus table' % (order,))
    if lengths is not None:
        if torch.is_tensor(lengths) and lengths.is_cuda:
            if lengths.device != dev or lengths.shape != (B,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError('ctc_beam_search: lengths must be (B,) integers on the device of prob (got %s %s on %s)'
                                 % (tuple(lengths.shape), lengths.dtype, lengths.device))
        else:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths)
            if host.shape != (B,) or host.dtype.kind not in 'iu' or (host < 0).any() or (host > T).any():
                raise ValueError('ctc_beam_search: lengths must be %d integers in [0, %d] (got %s)' % (B, T, host.tolist()))
        lengths = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    lib = _lib.load()
    prob = prob.contiguous()
    hyp = torch.empty(B, N, T, device=dev, dtype=torch.int64)
    hyp_len = torch.empty(B, N, device=dev, dtype=torch.int32)
    score = torch.empty(B, N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_ctc_beam_workspace_bytes(B, T, W)), device=dev, dtype=torch.uint8)
    if bonus is None:
        check(lib.st_ctc_beam_search(_p(prob), B, T, V, _p(lengths, torch.int32), W, N, blank, 1 if log_input else 0, float(eps),
                                     _p(hyp, torch.int64), _p(hyp_len, torch.int32), _p(score), _p(ws, torch.uint8), stream_handle()),
              'st_ctc_beam_search')
    else:
        check(lib.st_ctc_beam_search_lm(_p(prob), B, T, V, _p(lengths, torch.int32), W, N, blank, 1 if log_input else 0, float(eps),
                                        _p(bonus), order, bos, _p(hyp, torch.int64), _p(hyp_len, torch.int32), _p(score),
                                        _p(ws, torch.uint8), stream_handle()), 'st_ctc_beam_search_lm')
    return hyp, hyp_len, score


CA_MAX_T, CA_MIN_V, CA_MAX_V, CA_MAX_L = 4096, 2, 10240, 1024          # st_ctc_forced_align's limits


def _ca_lengths(name, x, B, hi, dev):
    """lengths / text_lengths of ctc_forced_align: None, or (B,) integers -- a host tensor / sequence is checked against [0, hi] here, a
    device tensor is taken as it is (the kernel clamps it) -> int32 device tensor or None"""
    if x is None:
        return None
    if torch.is_tensor(x) and x.is_cuda:
        if x.device != dev or x.shape != (B,) or x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError('ctc_forced_align: %s must be (B,) integers on the device of prob (got %s %s on %s)'
                             % (name, tuple(x.shape), x.dtype, x.device))
    else:
        host = np.asarray(x.cpu() if torch.is_tensor(x) else x)
        if host.shape != (B,) or host.dtype.kind not in 'iu' or (host < 0).any() or (host > hi).any():
            raise ValueError('ctc_forced_align: %s must be %d integers in [0, %d] (got %s)' % (name, B, hi, host.tolist()))
    return torch.as_tensor(x).to(dev, torch.int32).contiguous()


def ctc_forced_align(prob, text, lengths=None, text_lengths=None, blank=0, log_input=False, eps=1e-10):
    """CTC forced alignment (Viterbi) of text (B, L) int64 to prob (B, T, V) fp32 on one GPU (see st_ctc_forced_align).  lengths /
    text_lengths: None (all T frames / all L entries), or (B,) integers -- a host tensor / sequence is checked against [0, T] / [0, L]
    here, a device tensor is taken as it is (the kernel clamps it).  The targets are the non-blank entries of each row of text.
    -> (score (B,) float32, path (B, T) int32, tok_start (B, L) int32, tok_end (B, L) int32) device tensors; one launch, no host read.
    Anything the kernel would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(prob) or not prob.is_cuda or prob.dim() != 3 or prob.dtype != torch.float32:
        raise ValueError('ctc_forced_align: prob must be a (B, T, V) float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(prob.shape), prob.dtype, prob.device) if torch.is_tensor(prob) else type(prob).__name__))
    dev = prob.device
    if not torch.is_tensor(text) or not text.is_cuda or text.device != dev or text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('ctc_forced_align: text must be a (B, L) int64 tensor on the device of prob (got %s)'
                         % ('%s %s on %s' % (tuple(text.shape), text.dtype, text.device) if torch.is_tensor(text) else type(text).__name__))
    B, T, V = prob.shape
    L, blank = text.shape[1], int(blank)
    if text.shape[0] != B:
        raise ValueError('ctc_forced_align: %d utterances of prob, %d of text' % (B, text.shape[0]))
    if B < 1 or not (1 <= T <= CA_MAX_T and CA_MIN_V <= V <= CA_MAX_V and 1 <= L <= CA_MAX_L):
        raise ValueError('ctc_forced_align: B=%d, T=%d, V=%d, L=%d outside B >= 1, 1 <= T <= %d, %d <= V <= %d, 1 <= L <= %d'
                         % (B, T, V, L, CA_MAX_T, CA_MIN_V, CA_MAX_V, CA_MAX_L))
    if not 0 <= blank < V:
        raise ValueError('ctc_forced_align: blank %d outside [0, %d)' % (blank, V))
    if not eps >= 0.0:
        raise ValueError('ctc_forced_align: eps must be >= 0 (got %r)' % (eps,))
    lengths = _ca_lengths('lengths', lengths, B, T, dev)
    text_lengths = _ca_lengths('text_lengths', text_lengths, B, L, dev)
    lib = _lib.load()
    prob, text = prob.contiguous(), text.contiguous()
    score = torch.empty(B, device=dev, dtype=torch.float32)
    path = torch.empty(B, T, device=dev, dtype=torch.int32)
    tok_start = torch.empty(B, L, device=dev, dtype=torch.int32)
    tok_end = torch.empty(B, L, device=dev, dtype=torch.int32)
    nbytes = int(lib.st_ctc_align_workspace_bytes(B, T, L))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_ctc_forced_align(_p(prob), B, T, V, _p(lengths, torch.int32), _p(text, torch.int64), L, _p(text_lengths, torch.int32),
                                  blank, 1 if log_input else 0, float(eps), _p(score), _p(path, torch.int32), _p(tok_start, torch.int32),
                                  _p(tok_end, torch.int32), _p(ws, torch.uint8), stream_handle()), 'st_ctc_forced_align')
    return score, path, tok_start, tok_end


DTW_MAX_T, DTW_MAX_D = 4096, 64          # st_dtw_batch's limits


def _dtw_side(name, t):
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError('dtw: %s must be a (B, T, D) float32 GPU tensor (got %s)'
                         % (name, '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))


def _dtw_lengths(name, v, B, hi, dev):
    """x_len / y_len of dtw: as _ca_lengths (None, host integers checked against [0, hi], or a device tensor the kernel clamps)"""
    if v is None:
        return None
    if torch.is_tensor(v) and v.is_cuda:
        if v.device != dev or v.shape != (B,) or v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError('dtw: %s must be (B,) integers on the device of x (got %s %s on %s)' % (name, tuple(v.shape), v.dtype, v.device))
    else:
        host = np.asarray(v.cpu() if torch.is_tensor(v) else v)
        if host.shape != (B,) or host.dtype.kind not in 'iu' or (host < 0).any() or (host > hi).any():
            raise ValueError('dtw: %s must be %d integers in [0, %d] (got %s)' % (name, B, hi, host.tolist()))
    return torch.as_tensor(v).to(dev, torch.int32).contiguous()


def dtw(x, y, x_len=None, y_len=None, cols=None, scale=1.0, want_path=True):
    """Dynamic time warping of x (B, Tx, D) against y (B, Ty, D), fp32 on one GPU, pair by pair (see st_dtw_batch): Euclidean frame
    distance over the columns cols = (d0, d1) (None: all D) times `scale`, unweighted symmetric steps, ties to the diagonal, then
    (i-1, j).  Any batch / row strides (the last dimension has stride 1: a column window of a wider tensor is passed as cols, not as
    a slice).  x_len / y_len: None (all rows), or (B,) integers -- a host tensor / sequence is checked against [0, Tx] / [0, Ty] here,
    a device tensor is taken as it is (the kernel clamps it).
    -> (total (B,) float32, path_len (B,) int32, path (B, Tx + Ty - 1, 2) int32 or None when want_path is false) device tensors;
    one launch, no host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    _dtw_side('x', x)
    _dtw_side('y', y)
    dev = x.device
    if y.device != dev:
        raise ValueError('dtw: x on %s, y on %s' % (x.device, y.device))
    B, Tx, D = x.shape
    Ty = y.shape[1]
    if y.shape[0] != B or y.shape[2] != D:
        raise ValueError('dtw: x is %s, y is %s: the pairs and the columns must match' % (tuple(x.shape), tuple(y.shape)))
    if B < 1 or not (1 <= Tx <= DTW_MAX_T and 1 <= Ty <= DTW_MAX_T) or D < 1:
        raise ValueError('dtw: B=%d, Tx=%d, Ty=%d, D=%d outside B >= 1, 1 <= Tx, Ty <= %d, D >= 1' % (B, Tx, Ty, D, DTW_MAX_T))
    if cols is None:
        cols = (0, D)
    try:
        d0, d1 = (int(c) for c in cols)
    except (TypeError, ValueError):
        raise ValueError('dtw: cols must be a pair (d0, d1) (got %r)' % (cols,))
    if not (0 <= d0 < d1 <= D and d1 - d0 <= DTW_MAX_D):
        raise ValueError('dtw: cols [%d, %d) outside 0 <= d0 < d1 <= D = %d, at most %d columns' % (d0, d1, D, DTW_MAX_D))
    scale = float(scale)
    if not 0.0 < scale < float('inf'):
        raise ValueError('dtw: scale must be finite and positive (got %r)' % (scale,))
    strides = []
    for name, t in (('x', x), ('y', y)):
        sb, st = (t.stride(0) if B > 1 else 0), (t.stride(1) if t.shape[1] > 1 else max(t.stride(1), d1))     # (a 1-long dimension's stride is free)
        if (t.stride(2) != 1 and D > 1) or st < d1 or sb < 0:
            raise ValueError('dtw: %s has strides %s: the last dimension needs stride 1 and rows at least d1 = %d floats apart'
                             % (name, tuple(t.stride()), d1))
        strides.append((sb, st))
    x_len = _dtw_lengths('x_len', x_len, B, Tx, dev)
    y_len = _dtw_lengths('y_len', y_len, B, Ty, dev)
    lib = _lib.load()
    total = torch.empty(B, device=dev, dtype=torch.float32)
    path_len = torch.empty(B, device=dev, dtype=torch.int32)
    path = torch.empty(B, Tx + Ty - 1, 2, device=dev, dtype=torch.int32) if want_path else None
    nbytes = int(lib.st_dtw_workspace_bytes(B, Tx, Ty))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_dtw_batch(_p(x), strides[0][0], strides[0][1], _p(x_len, torch.int32), Tx, _p(y), strides[1][0], strides[1][1],
                           _p(y_len, torch.int32), Ty, B, d0, d1, scale, _p(total), _p(path_len, torch.int32), _p(path, torch.int32),
                           _p(ws, torch.uint8), stream_handle()), 'st_dtw_batch')
    return total, path_len, path


ABX_MAX_LEN, ABX_MAX_D = 64, 512         # st_dtw_pairs' limits
ABX_METRICS = {'euclid': 0, 'angular': 1, 'kl': 2}


def _abx_ints(what, name, t, dev, dtype=torch.int32, dim=1):
    if (not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dim() != dim or t.dtype != dtype or not t.is_contiguous()):
        raise ValueError('%s: %s must be a contiguous %d-d %s tensor on the device of the features (got %s)'
                         % (what, name, dim, str(dtype).replace('torch.', ''),
                            '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))


def dtw_pairs(feat, item_start, item_len, pair_a, pair_b, metric='angular', max_len=ABX_MAX_LEN, want_cost=False):
    """Path-normalised DTW distance of P pairs of items of one packed feature buffer, one wave a pair (see st_dtw_pairs): feat (n_rows, D)
    float32 on one GPU with unit column stride (a column slice of a wider tensor keeps its row stride); item q is the rows
    [item_start[q], item_start[q] + item_len[q]); pair p is item pair_a[p] against item pair_b[p] -- four contiguous int32 device tensors.
    metric: 'euclid', 'angular' or 'kl' (or its number).  max_len: the longest item the launch takes (it sizes LDS; at most 64).
    -> dist (P,) float32, or (dist, cost (P,) float32, path_len (P,) int32) with want_cost; NaN / 0 for a pair the kernel refuses (a bad
    index, a length outside [1, max_len], rows outside feat, a NaN among its rows).  One launch, no host read.  Anything the C entry
    point would refuse raises ValueError before the device is touched."""
    if not torch.is_tensor(feat) or not feat.is_cuda or feat.dim() != 2 or feat.dtype != torch.float32:
        raise ValueError('dtw_pairs: feat must be a (n_rows, D) float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(feat.shape), feat.dtype, feat.device) if torch.is_tensor(feat) else type(feat).__name__))
    dev = feat.device
    n_rows, D = feat.shape
    if n_rows < 1 or not 1 <= D <= ABX_MAX_D:
        raise ValueError('dtw_pairs: feat is %s: n_rows >= 1 and 1 <= D <= %d' % (tuple(feat.shape), ABX_MAX_D))
    st = feat.stride(0) if n_rows > 1 else max(feat.stride(0), D)          # (a 1-long dimension's stride is free)
    if (feat.stride(1) != 1 and D > 1) or st < D:
        raise ValueError('dtw_pairs: feat has strides %s: the columns need stride 1 and the rows at least D = %d floats apart'
                         % (tuple(feat.stride()), D))
    if isinstance(metric, str):
        if metric not in ABX_METRICS:
            raise ValueError('dtw_pairs: metric %r is none of %s' % (metric, sorted(ABX_METRICS)))
        metric = ABX_METRICS[metric]
    if isinstance(metric, bool) or not isinstance(metric, (int, np.integer)) or int(metric) not in ABX_METRICS.values():
        raise ValueError('dtw_pairs: metric %r is none of %s' % (metric, sorted(ABX_METRICS)))
    if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or not 1 <= int(max_len) <= ABX_MAX_LEN:
        raise ValueError('dtw_pairs: max_len must be an integer in [1, %d] (got %r)' % (ABX_MAX_LEN, max_len))
    for name, t in (('item_start', item_start), ('item_len', item_len), ('pair_a', pair_a), ('pair_b', pair_b)):
        _abx_ints('dtw_pairs', name, t, dev)
    n_items, P = item_start.shape[0], pair_a.shape[0]
    if n_items < 1 or item_len.shape[0] != n_items:
        raise ValueError('dtw_pairs: %d item starts, %d item lengths: at least one item, as many of each'
                         % (n_items, item_len.shape[0]))
    if P < 1 or pair_b.shape[0] != P or P >= 2 ** 31:
        raise ValueError('dtw_pairs: %d first items, %d second items: at least one pair, below 2^31, as many of each' % (P, pair_b.shape[0]))
    lib = _lib.load()
    dist = torch.empty(P, device=dev, dtype=torch.float32)
    cost = torch.empty(P, device=dev, dtype=torch.float32) if want_cost else None
    path_len = torch.empty(P, device=dev, dtype=torch.int32) if want_cost else None
    check(lib.st_dtw_pairs(_p(feat), n_rows, D, st, _p(item_start, torch.int32), _p(item_len, torch.int32), n_items, _p(pair_a, torch.int32),
                           _p(pair_b, torch.int32), P, int(metric), int(max_len), _p(dist), _p(cost), _p(path_len, torch.int32),
                           stream_handle()), 'st_dtw_pairs')
    return (dist, cost, path_len) if want_cost else dist


def abx_count(dmat, blk):
    """ABX triple counts from finished distances (see st_abx_count): dmat, a contiguous 1-d float32 GPU tensor holding the dense symmetric
    matrices of the cells end to end; blk (NB, 6) int64 on the same device, rows (mat_off, n_c, a_lo, a_hi, b_lo, b_hi).
    -> count (NB, 4) int64 = (wrong, tied, nan, triples) per block, a device tensor; one launch, exact, no host read.  Bad arguments
    raise ValueError before the device is touched."""
    if not torch.is_tensor(dmat) or not dmat.is_cuda or dmat.dim() != 1 or dmat.dtype != torch.float32 or not dmat.is_contiguous():
        raise ValueError('abx_count: dmat must be a contiguous 1-d float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(dmat.shape), dmat.dtype, dmat.device) if torch.is_tensor(dmat) else type(dmat).__name__))
    _abx_ints('abx_count', 'blk', blk, dmat.device, torch.int64, 2)
    NB = blk.shape[0]
    if blk.shape[1] != 6 or NB < 1 or NB >= 2 ** 31 or dmat.shape[0] < 1:
        raise ValueError('abx_count: blk is %s over %d distances: (NB, 6) with NB >= 1, at least one distance' % (tuple(blk.shape), dmat.shape[0]))
    lib = _lib.load()
    count = torch.empty(NB, 4, device=dmat.device, dtype=torch.int64)
    check(lib.st_abx_count(_p(dmat), dmat.shape[0], _p(blk, torch.int64), NB, _p(count, torch.int64), stream_handle()), 'st_abx_count')
    return count


AE_MAX_S, AE_MAX_L = 4096, 2048          # st_attn_endpoint's limits


def attn_endpoint(align, enc_len, patience=3, max_jump=4):
    """End of speech and alignment diagnostics of align (B, S, L), fp32 on one GPU, utterance by utterance (see st_attn_endpoint).
    Any batch / row strides with unit stride in L (a sliced view is read where it lies).  enc_len: (B,) real phones per utterance -- a
    host sequence / tensor is checked against [1, L] here, a device tensor is taken as it is (the kernel clamps it).
    -> (stats (B, 6) int32 = (end, reached, n_back, n_skip, covered, nonfinite), focus (B,) float32, peak (B, S) int32,
    dur (B, L) int32) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError before the
    device is touched."""
    if not torch.is_tensor(align) or not align.is_cuda or align.dim() != 3 or align.dtype != torch.float32:
        raise ValueError('attn_endpoint: align must be a (B, S, L) float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(align.shape), align.dtype, align.device) if torch.is_tensor(align) else type(align).__name__))
    dev = align.device
    B, S, L = align.shape
    if B < 1 or not (1 <= S <= AE_MAX_S and 1 <= L <= AE_MAX_L):
        raise ValueError('attn_endpoint: B=%d, S=%d, L=%d outside B >= 1, 1 <= S <= %d, 1 <= L <= %d' % (B, S, L, AE_MAX_S, AE_MAX_L))
    for name, v in (('patience', patience), ('max_jump', max_jump)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 2 ** 31 - 1:
            raise ValueError('attn_endpoint: %s must be an integer >= 1 (got %r)' % (name, v))
    sb, st = (align.stride(0) if B > 1 else 0), (align.stride(1) if S > 1 else max(align.stride(1), L))     # (a 1-long dimension's stride is free)
    if (align.stride(2) != 1 and L > 1) or st < L or sb < 0:
        raise ValueError('attn_endpoint: align has strides %s: the last dimension needs stride 1 and rows at least L = %d floats apart'
                         % (tuple(align.stride()), L))
    if torch.is_tensor(enc_len) and enc_len.is_cuda:
        if enc_len.device != dev or enc_len.shape != (B,) or enc_len.dtype.is_floating_point or enc_len.dtype == torch.bool:
            raise ValueError('attn_endpoint: enc_len must be (B,) integers on the device of align (got %s %s on %s)'
                             % (tuple(enc_len.shape), enc_len.dtype, enc_len.device))
    else:
        host = np.asarray(enc_len.cpu() if torch.is_tensor(enc_len) else enc_len)
        if host.shape != (B,) or host.dtype.kind not in 'iu' or (host < 1).any() or (host > L).any():
            raise ValueError('attn_endpoint: enc_len must be %d integers in [1, %d] (got %s)' % (B, L, host.tolist()))
    enc_len = torch.as_tensor(enc_len).to(dev, torch.int32).contiguous()
    lib = _lib.load()
    # one allocation, carved into the four contiguous outputs (the call is latency-bound: three more torch.empty cost as much as the kernel)
    flat = torch.empty(B * (7 + S + L), device=dev, dtype=torch.int32)
    stats, focus = flat[:6 * B].view(B, 6), flat[6 * B:7 * B].view(torch.float32)
    peak, dur = flat[7 * B:(7 + S) * B].view(B, S), flat[(7 + S) * B:].view(B, L)
    check(lib.st_attn_endpoint(_p(align), sb, st, _p(enc_len, torch.int32), B, S, L, int(patience), int(max_jump), _p(stats, torch.int32),
                               _p(focus), _p(peak, torch.int32), _p(dur, torch.int32), stream_handle()), 'st_attn_endpoint')
    return stats, focus, peak, dur


def hyp_edit_distance(hyp, hyp_len, text, ignore):
    """edit distance of transcripts that are already collapsed (a beam search's) to `text`, per utterance (see st_hyp_edit_distance):
    hyp (B, Lh) int64 with hyp_len (B,) int32 tokens each, text (B, L) int64, ignore: the ids dropped from both sides.  -> (dist,
    ref_len) int32 (B,) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError first."""
    if not all(torch.is_tensor(x) for x in (hyp, hyp_len, text)):
        raise ValueError('hyp_edit_distance: hyp, hyp_len and text must be tensors')
    if not (hyp.is_cuda and hyp.device == hyp_len.device == text.device):
        raise ValueError('hyp_edit_distance: hyp, hyp_len and text must be on one GPU (got %s, %s, %s)' % (hyp.device, hyp_len.device, text.device))
    if hyp.dim() != 2 or hyp.dtype != torch.int64 or text.dim() != 2 or text.dtype != torch.int64:
        raise ValueError('hyp_edit_distance: hyp and text must be 2-D int64 (got %s %s, %s %s)'
                         % (tuple(hyp.shape), hyp.dtype, tuple(text.shape), text.dtype))
    B, Lh = hyp.shape
    L = text.shape[1]
    if hyp_len.shape != (B,) or hyp_len.dtype != torch.int32:
        raise ValueError('hyp_edit_distance: hyp_len must be (%d,) int32 (got %s %s)' % (B, tuple(hyp_len.shape), hyp_len.dtype))
    ignore = tuple(int(i) for i in ignore)
    if text.shape[0] != B or B < 1:
        raise ValueError('hyp_edit_distance: %d hypotheses, %d transcripts (at least one)' % (B, text.shape[0]))
    if not (1 <= Lh <= GED_MAX_T and 1 <= L <= GED_MAX_L and len(ignore) <= GED_MAX_IGNORE):
        raise ValueError('hyp_edit_distance: Lh=%d, L=%d, %d ignored ids outside 1 <= Lh <= %d, 1 <= L <= %d, <= %d ignored ids'
                         % (Lh, L, len(ignore), GED_MAX_T, GED_MAX_L, GED_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('hyp_edit_distance: ignored ids must fit int32')
    dev = hyp.device
    ign = _IGNORE_DEV.get((dev, ignore))
    if ign is None:
        ign = _IGNORE_DEV[(dev, ignore)] = torch.tensor(ignore if ignore else [0], dtype=torch.int32).to(dev)
    hyp, hyp_len, text = hyp.contiguous(), hyp_len.contiguous(), text.contiguous()
    dist = torch.empty(B, device=dev, dtype=torch.int32)
    ref_len = torch.empty(B, device=dev, dtype=torch.int32)
    check(_lib.load().st_hyp_edit_distance(_p(hyp, torch.int64), _p(hyp_len, torch.int32), B, Lh, _p(text, torch.int64), L,
                                           _p(ign, torch.int32), len(ignore), _p(dist, torch.int32), _p(ref_len, torch.int32),
                                           stream_handle()), 'st_hyp_edit_distance')
    return dist, ref_len


EA_MAX_L, EA_MAX_V, EA_MAX_IGNORE = 1024, 1024, 64          # st_edit_align's limits


def _ea_lengths(name, v, shape, hi, dev):
    """hyp_len / ref_len of edit_align: host integers checked against [0, hi], or a device tensor the kernel clamps"""
    if torch.is_tensor(v) and v.is_cuda:
        if v.device != dev or tuple(v.shape) != shape or v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError('edit_align: %s must be %s integers on the device of hyp (got %s %s on %s)'
                             % (name, shape, tuple(v.shape), v.dtype, v.device))
    else:
        host = np.asarray(v.cpu() if torch.is_tensor(v) else v)
        if host.shape != shape or host.dtype.kind not in 'iu' or (host < 0).any() or (host > hi).any():
            raise ValueError('edit_align: %s must be %s integers in [0, %d] (got %s)' % (name, shape, hi, host.tolist()))
    return torch.as_tensor(v).to(dev, torch.int32).contiguous()


def edit_align(hyp, hyp_len, ref, ref_len=None, ignore=(), n_classes=1, confusion=None, want_ali=True):
    """Levenshtein alignment with its trace-back, pair by pair on one GPU (see st_edit_align): hyp (B, N, Lh) int64 transcripts of
    hyp_len (B, N) tokens, N paths per utterance, against ref (B, Lr) int64 of ref_len (B,) tokens (None: all Lr); a host sequence of
    lengths is checked against [0, L] here, a device tensor is taken as it is (the kernel clamps it).  ignore: the ids dropped from
    both sides.  confusion: None, a (n_classes + 1, n_classes + 1) int32 device tensor that path 0 of every utterance is added into, or
    True for a zeroed one made here.
    -> (counts (B, N, 4) int32 = correct, substitutions, deletions, insertions; ali_len (B, N) int32; ali (B, N, Lr + Lh, 2) int32 or
    None when want_ali is false; the confusion tensor or None) device tensors; one launch, no host read.  Anything the kernel would refuse raises ValueError before
    the device is touched."""
    for name, t in (('hyp', hyp), ('ref', ref)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int64:
            raise ValueError('edit_align: %s must be an int64 GPU tensor (got %s)'
                             % (name, '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    dev = hyp.device
    if ref.device != dev:
        raise ValueError('edit_align: hyp on %s, ref on %s' % (hyp.device, ref.device))
    if hyp.dim() != 3 or ref.dim() != 2:
        raise ValueError('edit_align: hyp must be (B, N, Lh) and ref (B, Lr) (got %s, %s)' % (tuple(hyp.shape), tuple(ref.shape)))
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    if ref.shape[0] != B:
        raise ValueError('edit_align: %d utterances of hypotheses, %d references: they must match' % (B, ref.shape[0]))
    if B < 1 or N < 1 or B * N > 2 ** 24:
        raise ValueError('edit_align: B=%d, N=%d outside B >= 1, N >= 1, B N <= 2^24' % (B, N))
    if not (1 <= Lh <= EA_MAX_L and 1 <= Lr <= EA_MAX_L):
        raise ValueError('edit_align: Lh=%d, Lr=%d outside 1 <= Lh, Lr <= %d' % (Lh, Lr, EA_MAX_L))
    V = n_classes
    if isinstance(V, bool) or not isinstance(V, (int, np.integer)) or not 1 <= int(V) <= EA_MAX_V:
        raise ValueError('edit_align: n_classes must be an integer in [1, %d] (got %r)' % (EA_MAX_V, V))
    V = int(V)
    try:
        ignore = tuple(int(i) for i in ignore)
    except (TypeError, ValueError):
        raise ValueError('edit_align: ignore must be a sequence of integer ids (got %r)' % (ignore,))
    if len(ignore) > EA_MAX_IGNORE:
        raise ValueError('edit_align: %d ignored ids, at most %d' % (len(ignore), EA_MAX_IGNORE))
    if any(not -2 ** 31 <= i < 2 ** 31 for i in ignore):
        raise ValueError('edit_align: ignored ids must fit int32')
    if confusion is not None and confusion is not True:
        if (not torch.is_tensor(confusion) or not confusion.is_cuda or confusion.device != dev or confusion.dtype != torch.int32
                or tuple(confusion.shape) != (V + 1, V + 1) or not confusion.is_contiguous()):
            raise ValueError('edit_align: confusion must be a contiguous (%d, %d) int32 tensor on the device of hyp (got %s)'
                             % (V + 1, V + 1, '%s %s on %s' % (tuple(confusion.shape), confusion.dtype, confusion.device)
                                if torch.is_tensor(confusion) else type(confusion).__name__))
    hyp_len = _ea_lengths('hyp_len', hyp_len, (B, N), Lh, dev)
    ref_len = None if ref_len is None else _ea_lengths('ref_len', ref_len, (B,), Lr, dev)
    lib = _lib.load()
    ign = _IGNORE_DEV.get((dev, ignore))
    if ign is None:
        ign = _IGNORE_DEV[(dev, ignore)] = torch.tensor(ignore if ignore else [0], dtype=torch.int32).to(dev)
    hyp, ref = hyp.contiguous(), ref.contiguous()
    if confusion is True:
        confusion = torch.zeros(V + 1, V + 1, device=dev, dtype=torch.int32)
    # one allocation, carved into the outputs (the call is latency-bound)
    AL = Lr + Lh
    flat = torch.empty(B * N * (5 + (2 * AL if want_ali else 0)), device=dev, dtype=torch.int32)
    counts, ali_len = flat[:4 * B * N].view(B, N, 4), flat[4 * B * N:5 * B * N].view(B, N)
    ali = flat[5 * B * N:].view(B, N, AL, 2) if want_ali else None
    nbytes = int(lib.st_edit_align_workspace_bytes(B * N, Lr, Lh))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    check(lib.st_edit_align(_p(hyp, torch.int64), _p(hyp_len, torch.int32), B, N, Lh, _p(ref, torch.int64), _p(ref_len, torch.int32), Lr,
                            _p(ign, torch.int32), len(ignore), V, _p(counts, torch.int32), _p(ali_len, torch.int32), _p(ali, torch.int32),
                            _p(confusion, torch.int32), _p(ws, torch.uint8), stream_handle()), 'st_edit_align')
    return counts, ali_len, ali, confusion


def softmax_argmax(logits):
    lib = _lib.load()
    V = logits.shape[-1]
    n = logits.numel() // V
    p = torch.empty_like(logits)
    idx = torch.empty(logits.shape[:-1], device=logits.device, dtype=torch.int64)
    check(lib.st_softmax_argmax(_p(logits), _p(p), _p(idx, torch.int64), n, V, stream_handle()), 'st_softmax_argmax')
    return p, idx


def fill_(t, v):
    check(_lib.load().st_fill(_p(t), float(v), t.numel(), stream_handle()), 'st_fill')
    return t


def copy2d(dst, src, rows, cols, ldd=None, lds=None):
    check(_lib.load().st_copy2d(_p(dst), int(ldd if ldd is not None else dst.stride(0)), _p(src),
                                int(lds if lds is not None else src.stride(0)), rows, cols, stream_handle()), 'st_copy2d')


def mean_rows(src):
    B, T, D = src.shape
    dst = torch.empty(B, D, device=src.device, dtype=torch.float32)
    check(_lib.load().st_mean_rows(_p(src), _p(dst), B, T, D, stream_handle()), 'st_mean_rows')
    return dst


# --------------------------------------------------------------------------------------------- backward blocks
def bn_norm(x2d, xoff, N, mean, var, w, b, eps, act=None, out=None, yoff=0):
    """out-of-place BatchNorm normalisation (training forward keeps x2d for the backward)"""
    M = x2d.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    check(_lib.load().st_bn_norm_fwd(_p(x2d), int(x2d.stride(0)), int(xoff), _p(out), int(out.stride(0)), int(yoff), M, N,
                                     _p(mean), _p(var), _p(w), _p(b), float(eps), ACT[act], stream_handle()), 'st_bn_norm_fwd')
    return out


def bn_norm_res_mask(x2d, mean, var, w, b, eps, act=None, res2d=None, mask2d=None, want_t=True):
    """-> (t, y): t = act(BatchNorm(x)) kept for the backward (None unless want_t), y = (t + res) * mask -- one launch (ConvLayer's tail,
    src/module.py:641-646).  Contiguous (M, N) operands."""
    M, N = x2d.shape
    y = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    t = torch.empty(M, N, device=x2d.device, dtype=torch.float32) if want_t and (res2d is not None or mask2d is not None) else None
    check(_lib.load().st_bn_norm_res_mask_fwd(_p(x2d), _p(t), _p(y), M, N, _p(mean), _p(var), _p(w), _p(b), float(eps), ACT[act],
                                              _p(res2d), _p(mask2d), stream_handle()), 'st_bn_norm_res_mask_fwd')
    return (t if t is not None else (y if want_t else None)), y


# ------------------------------------------------------------------------- where parameter gradients are written
_GRAD_SINK = None


def set_grad_sink(sink, only_if=None):
    """`sink.claim(param)` -> tensor or None decides where the kernels that produce parameter gradients write them: under data
    parallelism parallel.GradReducer hands out the parameter's slot in its all-reduce bucket, so the gradient is born in the
    communication buffer (no accumulate launch, no copy).  only_if: clear only when that sink is the registered one."""
    global _GRAD_SINK
    if only_if is not None and _GRAD_SINK is not only_if:
        return
    _GRAD_SINK = sink


def grad_slot(param):
    """the tensor the gradient of `param` should be written to (same shape), or None: allocate as usual"""
    s = _GRAD_SINK
    if s is None or param is None:
        return None
    return s.claim(param)


def mt_copy(dsts, srcs):
    """dsts[i] <- srcs[i] (contiguous fp32 device tensors of equal sizes) in a handful of multi-tensor launches"""
    import ctypes as C
    n = len(dsts)
    dp = (C.c_void_p * n)(*[t.data_ptr() for t in dsts])
    sp = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    sz = (C.c_long * n)(*[t.numel() for t in dsts])
    check(_lib.load().st_mt_copy(dp, sp, sz, n, stream_handle()), 'st_mt_copy')


def gemm_wgrad_split(dc, a, split, w0=None, w1=None, b0=None, b1=None, with_db=False):
    """gemm_wgrad of a Linear over concatenated inputs, cut at input column `split`: (dW0 (N, split), dW1 (N, Cin - split)[, db, db'])
    -- the gradients of [W_ih | W_hh] (and b_ih, b_hh: equal) of an LSTM cell leave the product's fixed-order slab sum as the
    parameters' own gradient tensors (w0 / w1 / b0 / b1: the parameters, asked for their grad_slot)"""
    lib = _lib.load()
    M, Cin = a.shape
    N = dc.shape[-1]
    f32 = dict(device=a.device, dtype=torch.float32)
    d0, d1 = grad_slot(w0), grad_slot(w1)
    d0 = d0 if d0 is not None else torch.empty(N, split, **f32)
    d1 = d1 if d1 is not None else torch.empty(N, Cin - split, **f32)
    db = dbd = None
    if with_db:
        db, dbd = grad_slot(b0), grad_slot(b1)
        db = db if db is not None else torch.empty(N, **f32)
        dbd = dbd if dbd is not None else torch.empty(N, **f32)
    nws = int(lib.st_gemm_wgrad_workspace_floats(1, int(M), int(Cin), int(N), 1))
    ws = torch.empty(nws, **f32)
    check(lib.st_gemm_wgrad_split(_p(dc), int(dc.stride(-2)), 0, _p(a), int(a.stride(-2)), _p(d0), int(split), _p(d1),
                                  _p(db), _p(dbd), _p(ws), int(M), int(Cin), int(N), 0, stream_handle()), 'st_gemm_wgrad_split')
    return (d0, d1, db, dbd) if with_db else (d0, d1)


# Weight gradients are leaves of the backward pass: nothing later in it reads them.  Inside an autograd backward the products marked
# `later=True` are therefore only QUEUED (their output tensors exist at once, and are what the Function returns); the queue leaves as
# batched launches (st_gemm_wgrad_batch: one product launch + one slab-sum launch per 16 small products instead of two launches each,
# and small products share the chip) when it is full, before a gradient bucket is handed to the all-reduce (parallel.GradReducer),
# and from an engine callback at the end of the backward pass -- before `backward()` returns.  ST_WGRAD_DEFER=0: every product at once.
# A queued product must be the ONLY thing that has touched its parameter's gradient when it finally runs (it overwrites): the sites ask
# `grad_first(*params)` -- True when this is the first gradient contribution to each of them in this backward pass -- and queue only
# then; a later contribution to a parameter whose first one is still queued (the prenet's weights under partial teacher forcing: the
# decoder's own-output path and the teacher path) sends the queue out first and runs at once, so autograd's in-place accumulate finds
# both written.
_WQ = []
_WQ_TASK = -1
_WQ_PENDING = set()
_G_TASK = -1
_G_COUNT = {}
WGRAD_DEFER = os.environ.get('ST_WGRAD_DEFER', '1') != '0'
WGRAD_QMAX = 16


def _graph_task():
    f = getattr(torch._C, '_current_graph_task_id', None)
    return f() if f is not None else -1


def flush_wgrads():
    """launch the queued weight-gradient products (a no-op when there are none)"""
    global _WQ
    if _WQ:
        jobs, _WQ = _WQ, []
        _WQ_PENDING.clear()
        cur = stream_handle()
        streams = []
        for j in jobs:
            if j.get('_stream', cur) not in streams:
                streams.append(j.get('_stream', cur))
        for h in streams:
            group = [j for j in jobs if j.get('_stream', cur) == h]
            if h == cur:
                gemm_wgrad_batch(group)
            else:
                with use_stream(h):
                    gemm_wgrad_batch(group)


def grad_first(*params):
    """announce a gradient contribution to each of `params` (None entries ignored) by the calling backward function; True when it is
    the first one to every one of them in this backward pass and all of them are leaves (the returned gradient goes straight to
    `.grad`, nothing reads it on the way) -- the condition for handing the product to the queue (`later=`).  Outside a backward
    pass: False."""
    global _G_TASK
    tid = _graph_task() if WGRAD_DEFER else -1
    if tid == -1:
        return False
    if tid != _G_TASK:
        _G_TASK = tid
        _G_COUNT.clear()
    first = True
    for q in params:
        if q is None:
            continue
        k = q.data_ptr()
        n = _G_COUNT.get(k, 0) + 1
        _G_COUNT[k] = n
        if n > 1:
            first = False
            if k in _WQ_PENDING:
                flush_wgrads()
        if not q.is_leaf:                 # (computed from parameters by torch ops: their backward reads the gradient at once)
            first = False
        # a parameter that already HAS a gradient (a second backward() without zero_grad -- gradient accumulation --, or
        # zero_grad(set_to_none=False)) makes AccumulateGrad run `grad += new` the moment the function returns, and a tensor hook reads
        # the gradient there as well: both before a queued product would have written it.  Such a product is launched at once.
        elif q.grad is not None or q._backward_hooks:
            first = False
    return first


def _queue_wgrads(jobs, params=()):
    """jobs (dicts of gemm_wgrad_batch, outputs allocated) onto the queue; False outside a backward pass (the caller launches them)"""
    global _WQ_TASK
    tid = _graph_task() if WGRAD_DEFER else -1
    if tid == -1:
        return False
    if _WQ and _WQ_TASK != tid:
        _WQ.clear()                       # (left by a backward pass that raised: their tensors belong to a step that is gone)
        _WQ_PENDING.clear()
    if not _WQ:
        _WQ_TASK = tid
        torch.autograd.Variable._execution_engine.queue_callback(flush_wgrads)
    h = stream_handle()
    for j in jobs:
        j['_stream'] = h                  # (launched later, perhaps by another thread: on the stream its operands were produced on)
    _WQ.extend(jobs)
    _WQ_PENDING.update(q.data_ptr() for q in params if q is not None)
    if len(_WQ) >= WGRAD_QMAX:
        flush_wgrads()
    return True


def _alias(t):
    """a second tensor object over the same memory: autograd adopts a returned gradient as `.grad` only when nobody else holds that
    OBJECT (otherwise it clones it on the spot -- here before the queued product has written it)"""
    return None if t is None else t.view(t.shape)


def _wgrad_job_outputs(j):
    """fill in `out` / `db_out` of a job dict (fresh tensors where the caller named none); returns (dW, db or None)"""
    dc, a = j['dc'], j['a']
    Cin = a.shape[-1]
    KT = int(j.get('KT', 1))
    N = j.get('N') if j.get('N') is not None else dc.shape[-1]
    if j.get('out') is None:
        j['out'] = torch.empty((N, Cin, KT) if KT > 1 else (N, Cin), device=a.device, dtype=torch.float32)
    if j.get('with_db') and j.get('db_out') is None:
        j['db_out'] = torch.empty(N, device=a.device, dtype=torch.float32)
    return j['out'], (j['db_out'] if j.get('with_db') else None)


def gemm_wgrad_batch(jobs, later=False, params=()):
    """[gemm_wgrad(dc, a, KT, pad, Bn=, Tin=, Tout=, N=, out=, with_db=, db_out=) for each job dict] as ONE product launch and ONE slab-sum
    launch per 16 where the kernels allow (st_gemm_wgrad_batch: bit for bit the separate calls); returns [(dW, db or None)].
    later: inside a backward pass the jobs only join the queue (see above); pass `later=grad_first(*params)` and the same `params`."""
    from ._lib import StWgradJob
    if later:
        outs = [_wgrad_job_outputs(j) for j in jobs]
        if _queue_wgrads(jobs, params):
            return [(_alias(dw), _alias(db)) for dw, db in outs]
    lib = _lib.load()
    n = len(jobs)
    arr = (StWgradJob * n)()
    outs = []
    for i, j in enumerate(jobs):
        dc, a = j['dc'], j['a']
        if a.dim() == 3:
            Bn_, Tin_, Cin = a.shape
        else:
            Bn_, Tin_, Cin = 1, a.shape[0], a.shape[1]
        KT = int(j.get('KT', 1))
        Bn = j.get('Bn') or Bn_
        Tin = j.get('Tin') or Tin_
        Tout = j.get('Tout')
        if Tout is None:
            Tout = dc.shape[1] if dc.dim() == 3 else dc.shape[0] // Bn
        N = j.get('N') if j.get('N') is not None else dc.shape[-1]
        out = j.get('out')
        if out is None:
            out = torch.empty((N, Cin, KT) if KT > 1 else (N, Cin), device=a.device, dtype=torch.float32)
        db = None
        if j.get('with_db'):
            db = j.get('db_out')
            if db is None:
                db = torch.empty(N, device=a.device, dtype=torch.float32)
        q = arr[i]
        q.dC, q.lddc, q.dcoff, q.A, q.lda, q.dW, q.db = _p(dc), int(dc.stride(-2)), 0, _p(a), int(a.stride(-2)), _p(out), _p(db)
        q.Bn, q.Tin, q.Tout, q.Cin, q.N, q.KT, q.pad = int(Bn), int(Tin), int(Tout), int(Cin), int(N), KT, int(j.get('pad', 0))
        outs.append((out, db))
    ws = torch.empty(int(lib.st_gemm_wgrad_batch_workspace_floats(arr, n)), device=jobs[0]['a'].device, dtype=torch.float32)
    check(lib.st_gemm_wgrad_batch(arr, n, _p(ws), stream_handle()), 'st_gemm_wgrad_batch')
    return outs


def gemm_wgrad(dc, a, KT=1, pad=0, *, Bn=None, Tin=None, Tout=None, dcoff=0, N=None, pool_prev=False, out=None,
               accumulate=False, with_db=False, db_out=None, later=False, params=()):
    """dW (N, Cin[, KT]) of C = conv1d/linear(a, W): dc (Bn, Tout, >=dcoff+N) or (M, .), a (Bn, Tin, Cin) or (M, Cin).
    with_db: returns (dW, db) with db = the column sums of dc (the bias gradient), formed inside the same launches.
    out / db_out: where to write them (grad_slot of the parameters), else fresh tensors.
    later (= grad_first(*params), with the same `params`: the parameters whose gradients this writes): inside a backward pass the
    product may be queued and launched with others (flush_wgrads); the caller must not write to `dc` / `a` afterwards."""
    if later and WGRAD_DEFER and not pool_prev and not accumulate and dcoff == 0 and _graph_task() != -1:
        j = dict(dc=dc, a=a, KT=KT, pad=pad, Bn=Bn, Tin=Tin, Tout=Tout, N=N, out=out, with_db=with_db, db_out=db_out)
        dw, db = _wgrad_job_outputs(j)
        if _queue_wgrads([j], params):
            return (_alias(dw), _alias(db)) if with_db else _alias(dw)
        out, db_out = dw, db
    lib = _lib.load()
    if a.dim() == 3:
        Bn_, Tin_, Cin = a.shape
    else:
        Bn_, Tin_, Cin = 1, a.shape[0], a.shape[1]
    Bn = Bn or Bn_
    Tin = Tin or Tin_
    if Tout is None:
        Tout = dc.shape[1] if dc.dim() == 3 else dc.shape[0] // Bn
    N = N if N is not None else dc.shape[-1] - dcoff
    if out is None:
        out = torch.empty((N, Cin, KT) if KT > 1 else (N, Cin), device=a.device, dtype=torch.float32)
    nws = int(lib.st_gemm_wgrad_workspace_floats(int(Bn), int(Tout), int(Cin), int(N), int(KT)))
    ws = torch.empty(nws, device=a.device, dtype=torch.float32)
    if with_db:
        db = db_out if db_out is not None else torch.empty(N, device=a.device, dtype=torch.float32)
        check(lib.st_gemm_wgrad_db(_p(dc), int(dc.stride(-2)), int(dcoff), _p(a), int(a.stride(-2)), _p(out), _p(db), _p(ws), int(Bn),
                                   int(Tin), int(Tout), int(Cin), int(N), int(KT), int(pad), 1 if pool_prev else 0,
                                   1 if accumulate else 0, stream_handle()), 'st_gemm_wgrad_db')
        return out, db
    check(lib.st_gemm_wgrad(_p(dc), int(dc.stride(-2)), int(dcoff), _p(a), int(a.stride(-2)), _p(out), _p(ws), int(Bn),
                            int(Tin), int(Tout), int(Cin), int(N), int(KT), int(pad), 1 if pool_prev else 0,
                            1 if accumulate else 0, stream_handle()), 'st_gemm_wgrad')
    return out


def colsum(x2d, N=None, xoff=0, y2d=None, yoff=0, out=None, accumulate=False):
    M = x2d.shape[0]
    N = N if N is not None else x2d.shape[1] - xoff
    if out is None:
        out = torch.empty(N, device=x2d.device, dtype=torch.float32)
    check(_lib.load().st_colsum(_p(x2d), int(x2d.stride(0)), int(xoff), _p(y2d), int(y2d.stride(0)) if y2d is not None else 0,
                                int(yoff), M, N, _p(out), 1 if accumulate else 0, _p(_colreduce_ws(M, N, x2d.device)),
                                stream_handle()), 'st_colsum')
    return out


def act_bwd(dout2d, out2d, act, mask2d=None, dpre=None):
    M, N = dout2d.shape
    if dpre is None:
        dpre = torch.empty(M, N, device=dout2d.device, dtype=torch.float32)
    check(_lib.load().st_act_bwd(_p(dout2d), int(dout2d.stride(0)), _p(out2d), int(out2d.stride(0)) if out2d is not None else 0,
                                 ACT[act], _p(mask2d), int(mask2d.stride(0)) if mask2d is not None else 0, _p(dpre),
                                 int(dpre.stride(0)), M, N, stream_handle()), 'st_act_bwd')
    return dpre


def bn_bwd(dy2d, y2d, act, x2d, mean, var, w, eps, need_wb=True):
    """returns dx, dw, db for y = act(BN_train(x))"""
    M, N = x2d.shape
    dx = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    dw = torch.empty(N, device=x2d.device, dtype=torch.float32) if need_wb else None
    db = torch.empty(N, device=x2d.device, dtype=torch.float32) if need_wb else None
    ws = _colreduce_ws(M, N, x2d.device)
    check(_lib.load().st_bn_bwd(_p(dy2d), int(dy2d.stride(0)), 0, _p(y2d), int(y2d.stride(0)) if y2d is not None else 0, 0,
                                ACT[act], _p(x2d), int(x2d.stride(0)), 0, _p(mean), _p(var), _p(w), float(eps), M, N,
                                _p(dx), N, 0, _p(dw), _p(db), 0, _p(ws), stream_handle()), 'st_bn_bwd')
    return dx, dw, db


def bn_bwd_reduce(dy2d, y2d, act, x2d, mean, var, eps, mask2d=None):
    """-> s (2N): [sum dyb, sum dyb * xhat] over the local rows; mask2d: dy is multiplied by it on the way in (st_bn_norm_res_mask_fwd's backward)"""
    M, N = x2d.shape
    s = torch.empty(2 * N, device=x2d.device, dtype=torch.float32)
    ws = _colreduce_ws(M, N, x2d.device)
    if mask2d is not None:
        check(_lib.load().st_bn_bwd_reduce_masked(_p(dy2d), int(dy2d.stride(0)), _p(mask2d), int(mask2d.stride(0)), _p(y2d),
                                                  int(y2d.stride(0)) if y2d is not None else 0, ACT[act], _p(x2d), int(x2d.stride(0)),
                                                  _p(mean), _p(var), float(eps), M, N, _p(s), _p(ws), stream_handle()), 'st_bn_bwd_reduce_masked')
        return s
    check(_lib.load().st_bn_bwd_reduce(_p(dy2d), int(dy2d.stride(0)), 0, _p(y2d), int(y2d.stride(0)) if y2d is not None else 0, 0,
                                       ACT[act], _p(x2d), int(x2d.stride(0)), 0, _p(mean), _p(var), float(eps), M, N, _p(s), _p(ws),
                                       stream_handle()), 'st_bn_bwd_reduce')
    return s


def bn_bwd_apply(dy2d, y2d, act, x2d, mean, var, w, eps, s, Mstat, inv_total=None, mask2d=None, want_dres=None):
    """inv_total (device scalar, bn_sync_merge): s holds sums over all ranks' rows, divide them by the global count.
    want_dres is not None: the masked form -> (dx, dres or None) with dres = dy * mask (the gradient of a residual input)"""
    M, N = x2d.shape
    dx = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    if want_dres is not None:
        dres = torch.empty(M, N, device=x2d.device, dtype=torch.float32) if want_dres else None
        check(_lib.load().st_bn_bwd_apply_masked(_p(dy2d), int(dy2d.stride(0)), _p(mask2d), int(mask2d.stride(0)) if mask2d is not None else 0,
                                                 _p(y2d), int(y2d.stride(0)) if y2d is not None else 0, ACT[act], _p(x2d), int(x2d.stride(0)),
                                                 _p(mean), _p(var), _p(w), float(eps), M, N, _p(s), int(Mstat), _p(inv_total), _p(dx), N,
                                                 _p(dres), N, stream_handle()), 'st_bn_bwd_apply_masked')
        return dx, dres
    if inv_total is not None:
        check(_lib.load().st_bn_bwd_apply_sync(_p(dy2d), int(dy2d.stride(0)), 0, _p(y2d), int(y2d.stride(0)) if y2d is not None else 0, 0,
                                               ACT[act], _p(x2d), int(x2d.stride(0)), 0, _p(mean), _p(var), _p(w), float(eps), M, N,
                                               _p(s), _p(inv_total), _p(dx), N, 0, stream_handle()), 'st_bn_bwd_apply_sync')
        return dx
    check(_lib.load().st_bn_bwd_apply(_p(dy2d), int(dy2d.stride(0)), 0, _p(y2d), int(y2d.stride(0)) if y2d is not None else 0, 0,
                                      ACT[act], _p(x2d), int(x2d.stride(0)), 0, _p(mean), _p(var), _p(w), float(eps), M, N, _p(s),
                                      int(Mstat), _p(dx), N, 0, stream_handle()), 'st_bn_bwd_apply')
    return dx


def highway_fwd(H, Tg, x):
    y = torch.empty_like(x)
    check(_lib.load().st_highway_fwd(_p(H), _p(Tg), _p(x), _p(y), x.numel(), stream_handle()), 'st_highway_fwd')
    return y


def highway_bwd(dy, H, x, Tg):
    dH, dT, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    check(_lib.load().st_highway_bwd(_p(dy), _p(H), _p(x), _p(Tg), _p(dH), _p(dT), _p(dx), x.numel(), stream_handle()),
          'st_highway_bwd')
    return dH, dT, dx


def _bn_bank_segs(xs, bns, means, vars_, dxs=None, sums=None, update_running=True):
    import ctypes as C
    n = len(xs)
    segs = (_lib.StBnBankSeg * n)()
    for k, (x, bn) in enumerate(zip(xs, bns)):
        sg = segs[k]
        sg.x, sg.ldx, sg.T = _p(x), int(x.stride(-2)), int(x.shape[1])
        sg.w, sg.b = _p(bn.weight), _p(bn.bias)
        if update_running and bn.running_mean is not None:
            sg.run_mean, sg.run_var = _p(bn.running_mean), _p(bn.running_var)
            sg.batches_tracked = _p(bn.num_batches_tracked, torch.int64)
        assert bn.momentum is not None, 'BatchNorm1d(momentum=None) (cumulative average) is not what the reference builds'
        sg.momentum, sg.eps = float(bn.momentum), float(bn.eps)
        sg.mean, sg.var = _p(means[k]), _p(vars_[k])
        if dxs is not None:
            sg.dx, sg.lddx, sg.sums = _p(dxs[k]), int(dxs[k].stride(-2)), _p(sums[k])
    return segs


def bn_bank_fwd(xs, bns, Tout):
    """K BatchNorm1d layers (batch statistics, running statistics updated) of K tensors (Bn, T_k, N) -> the bank (Bn, Tout, K N) and the
    (K, 2, N) statistics: 3 launches (st_bn_bank_fwd)"""
    lib = _lib.load()
    n, (Bn, _, N) = len(xs), xs[0].shape
    dev = xs[0].device
    stats = torch.empty(n, 2, N, device=dev, dtype=torch.float32)
    Y = torch.empty(Bn, Tout, n * N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_bn_bank_workspace_floats(n, int(Bn * max(x.shape[1] for x in xs)), int(N))), device=dev, dtype=torch.float32)
    segs = _bn_bank_segs(xs, bns, [stats[k, 0] for k in range(n)], [stats[k, 1] for k in range(n)])
    check(lib.st_bn_bank_fwd(segs, n, int(Bn), int(N), _p(Y), n * int(N), int(Tout), _p(ws), stream_handle()), 'st_bn_bank_fwd')
    return Y, stats


def bn_bank_fwd_sync(xs, bns, Tout):
    """bn_bank_fwd under SyncBN: this rank's records -> ONE all-gather -> merge -> normalise.  Returns the bank, the (K, 2, N) global
    statistics and inv_total (K) = 1 / global row count per segment."""
    from . import parallel
    lib = _lib.load()
    n, (Bn, _, N) = len(xs), xs[0].shape
    dev = xs[0].device
    stats = torch.empty(n, 2, N, device=dev, dtype=torch.float32)
    Y = torch.empty(Bn, Tout, n * N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_bn_bank_workspace_floats(n, int(Bn * max(x.shape[1] for x in xs)), int(N))), device=dev, dtype=torch.float32)
    segs = _bn_bank_segs(xs, bns, [stats[k, 0] for k in range(n)], [stats[k, 1] for k in range(n)])
    rec = torch.empty(n, 2 * N + 1, device=dev, dtype=torch.float32)
    check(lib.st_bn_bank_stats_record(segs, n, int(Bn), int(N), _p(rec), _p(ws), stream_handle()), 'st_bn_bank_stats_record')
    allrec = parallel.all_gather_(rec).contiguous()                       # (world, n, 2N + 1)
    inv_total = torch.empty(n, device=dev, dtype=torch.float32)
    check(lib.st_bn_bank_sync_merge(segs, n, int(Bn), int(N), _p(allrec), int(allrec.shape[0]), _p(inv_total), stream_handle()),
          'st_bn_bank_sync_merge')
    check(lib.st_bn_bank_norm(segs, n, int(Bn), int(N), _p(Y), n * int(N), int(Tout), stream_handle()), 'st_bn_bank_norm')
    return Y, stats, inv_total


def bn_bank_bwd_sync(dY, xs, bns, stats, inv_total, relu_in):
    """backward of bn_bank_fwd_sync: local sums -> ONE all-reduce -> apply.  Returns (dxs, LOCAL sums (K, 2, N)): the parameter gradients
    keep this rank's sums (the gradient reducer averages them over the ranks), dx uses the global ones."""
    from . import parallel
    lib = _lib.load()
    n, (Bn, _, N) = len(xs), xs[0].shape
    dev = xs[0].device
    dxs = [torch.empty_like(x) for x in xs]
    local = torch.empty(n, 2, N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_bn_bank_workspace_floats(n, int(Bn * max(x.shape[1] for x in xs)), int(N))), device=dev, dtype=torch.float32)
    means, vars_ = [stats[k, 0] for k in range(n)], [stats[k, 1] for k in range(n)]
    segs = _bn_bank_segs(xs, bns, means, vars_, dxs, [local[k] for k in range(n)], update_running=False)
    check(lib.st_bn_bank_bwd_reduce(segs, n, int(Bn), int(N), _p(dY), int(dY.stride(-2)), int(dY.shape[1]), _p(ws), stream_handle()),
          'st_bn_bank_bwd_reduce')
    glob = local.clone()
    parallel.all_reduce_sum_(glob)
    segs = _bn_bank_segs(xs, bns, means, vars_, dxs, [glob[k] for k in range(n)], update_running=False)
    check(lib.st_bn_bank_bwd_apply(segs, n, int(Bn), int(N), _p(dY), int(dY.stride(-2)), int(dY.shape[1]), 1 if relu_in else 0, _p(inv_total),
                                   stream_handle()), 'st_bn_bank_bwd_apply')
    return dxs, local


def bn_bank_bwd(dY, xs, bns, stats, relu_in):
    """backward of bn_bank_fwd: dx_k over every row of segment k (through the ReLU in front of the norm when relu_in) and the (K, 2, N)
    sums (d bias, d weight): 3 launches"""
    lib = _lib.load()
    n, (Bn, _, N) = len(xs), xs[0].shape
    dev = xs[0].device
    dxs = [torch.empty_like(x) for x in xs]
    sums = torch.empty(n, 2, N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.st_bn_bank_workspace_floats(n, int(Bn * max(x.shape[1] for x in xs)), int(N))), device=dev, dtype=torch.float32)
    segs = _bn_bank_segs(xs, bns, [stats[k, 0] for k in range(n)], [stats[k, 1] for k in range(n)], dxs, [sums[k] for k in range(n)],
                         update_running=False)
    check(lib.st_bn_bank_bwd(segs, n, int(Bn), int(N), _p(dY), int(dY.stride(-2)), int(dY.shape[1]), 1 if relu_in else 0, _p(ws),
                             stream_handle()), 'st_bn_bank_bwd')
    return dxs, sums


def cat_params(ws, transposed=False, pad_to=0):
    """parameters side by side as one GEMM operand (cached per weight version, refreshed with the other layouts in one launch)"""
    return _LAYOUTS.get_cat(list(ws), 1 if transposed else 0, pad_to)


def highway_ht_fwd(ht, x):
    M, Cn = x.shape
    y = torch.empty_like(x)
    check(_lib.load().st_highway_ht_fwd(_p(ht), _p(x), _p(y), int(M), int(Cn), stream_handle()), 'st_highway_ht_fwd')
    return y


def highway_ht_bwd(dy, ht, x):
    M, Cn = x.shape
    dht, dxd = torch.empty_like(ht), torch.empty_like(x)
    check(_lib.load().st_highway_ht_bwd(_p(dy), _p(ht), _p(x), _p(dht), _p(dxd), int(M), int(Cn), stream_handle()), 'st_highway_ht_bwd')
    return dht, dxd


def pool_prev_fwd(x):
    """MaxPool1d(2, stride 1, padding 1)(x)[:T] of a contiguous channels-last (B, T, C) tensor as a tensor of its own (C % 4 == 0)"""
    Bn, T, Cc = x.shape
    y = torch.empty_like(x)
    check(_lib.load().st_pool_prev_fwd(_p(x), _p(y), int(Bn), int(T), int(Cc), stream_handle()), 'st_pool_prev_fwd')
    return y


def pool_prev_bwd(dy_pooled, x):
    Bn, T, Cc = x.shape
    dx = torch.empty_like(x)
    check(_lib.load().st_pool_prev_bwd(_p(dy_pooled), _p(x), _p(dx), Bn, T, Cc, stream_handle()), 'st_pool_prev_bwd')
    return dx


def copy3d(dst, src, Bn, T, Cc, accumulate=False):
    """dst[b, t, :Cc] (+)= src[b, t, :Cc]; both (Bn, T, >=Cc) views with unit channel stride"""
    assert dst.stride(-1) == 1 and src.stride(-1) == 1
    check(_lib.load().st_copy3d(_p(dst), int(dst.stride(0)), int(dst.stride(1)), _p(src), int(src.stride(0)),
                                int(src.stride(1)), Bn, T, Cc, 1 if accumulate else 0, stream_handle()), 'st_copy3d')
    return dst


def scatter_add_rows(dout, idx, V):
    D = dout.shape[-1]
    idx = idx.contiguous()
    dtable = torch.empty(V, D, device=dout.device, dtype=torch.float32)
    fill_(dtable, 0.0)
    check(_lib.load().st_scatter_add_rows(_p(dout), _p(idx, torch.int64), _p(dtable), idx.numel(), D, V, stream_handle()),
          'st_scatter_add_rows')
    return dtable


# --------------------------------------------------------------------------------------------- packed operands
def t16_floats(B, K):
    return int(_lib.load().st_t16_floats(int(B), int(K)))


def pack_weight(ws, ks, N, lstm_H=0, ldws=None):
    """ws: list of (N, k_s) weight slices (views of torch weights); returns the P16 buffer"""
    lib = _lib.load()
    n = len(ws)
    karr = (C.c_int * n)(*[int(k) for k in ks])
    ldarr = (C.c_int * n)(*[int(ld) for ld in (ldws or [w.stride(0) for w in ws])])
    warr = (C.c_void_p * n)(*[_p(w) for w in ws])
    size = int(lib.st_packed_weight_floats(karr, n, int(N), int(lstm_H)))
    out = torch.empty(size, device=ws[0].device, dtype=torch.float32)
    check(lib.st_pack_weight(warr, ldarr, karr, n, int(N), int(lstm_H), _p(out), stream_handle()), 'st_pack_weight')
    return out


def pack_weight_t(ws):
    """P16 buffer of torch.cat(ws, 1).t() -- ws: list of (K, cols_s) matrices (row stride >= cols_s); no cat / transpose copy"""
    lib = _lib.load()
    n = len(ws)
    K = int(ws[0].shape[0])
    assert all(int(w.shape[0]) == K and w.stride(1) == 1 for w in ws)
    cols = [int(w.shape[1]) for w in ws]
    carr = (C.c_int * n)(*cols)
    ldarr = (C.c_int * n)(*[int(w.stride(0)) for w in ws])
    warr = (C.c_void_p * n)(*[_p(w) for w in ws])
    karr = (C.c_int * 1)(K)
    size = int(lib.st_packed_weight_floats(karr, 1, sum(cols), 0))
    out = torch.empty(size, device=ws[0].device, dtype=torch.float32)
    check(lib.st_pack_weight_t(warr, ldarr, carr, n, K, _p(out), stream_handle()), 'st_pack_weight_t')
    return out


def kb16(k):
    return (int(k) + 15) // 16


def t16_view(buf, kb_stride=None, kb0=0, K=None):
    """StT16View over a T16 buffer (kb_stride defaults to the k-blocks of a (B, K) buffer)"""
    v = _lib.StT16View()
    v.base = _p(buf)
    v.kb_stride = int(kb_stride if kb_stride is not None else kb16(K))
    v.kb0 = int(kb0)
    return v


def tile_rows(x, out=None, kb_stride=None, kb0=0):
    """natural (B, K) -> T16 (optionally into the k-block range kb0.. of a wider buffer)"""
    B, K = x.shape
    if out is None:
        out = torch.zeros(t16_floats(B, K), device=x.device, dtype=torch.float32)
    v = t16_view(out, kb_stride if kb_stride is not None else kb16(K), kb0)
    check(_lib.load().st_tile_rows(_p(x), int(x.stride(0)), C.byref(v), B, K, stream_handle()), 'st_tile_rows')
    return out


def untile_rows(x_t16, B, K, kb_stride=None, kb0=0):
    out = torch.empty(B, K, device=x_t16.device, dtype=torch.float32)
    v = t16_view(x_t16, kb_stride if kb_stride is not None else kb16(K), kb0)
    check(_lib.load().st_untile_rows(C.byref(v), _p(out), K, B, K, stream_handle()), 'st_untile_rows')
    return out


def untile_tape(flat, slots, Bp, kb_stride, segs):
    """T16 step tape (slots x [Bp/16][kb_stride][64][4]) -> natural (slots, Bp, sum(k)); segs = [(kb0, k), ...].
    Consecutive slots are consecutive batch tiles, so one launch per segment un-tiles every step."""
    width = sum(k for _, k in segs)
    out = torch.empty(slots, Bp, width, device=flat.device, dtype=torch.float32)
    merged = []          # segments that follow each other in whole k-blocks are one run in both layouts: one launch for the run
    for kb0, k in segs:
        if merged and merged[-1][1] % 16 == 0 and merged[-1][0] + merged[-1][1] // 16 == kb0:
            merged[-1] = (merged[-1][0], merged[-1][1] + k)
        else:
            merged.append((kb0, k))
    col = 0
    for kb0, k in merged:
        v = t16_view(flat, kb_stride, kb0)
        check(_lib.load().st_untile_rows(C.byref(v), _p(out) + 4 * col, width, slots * Bp, k, stream_handle()), 'st_untile_rows')
        col += k
    return out


def lstm_cell_job(packed_w, x_view, Kpad, b_ih, b_hh, c_prev, h_dst0, c_out, B, H, h_dst1=None, mask=None,
                  gates_out=None, ada_std=None, ada_mean=None, hadapt_dst=None, part=None, w_kbs=0):
    """StLstmCellPackedJob; x_view / *_dst: StT16View (see t16_view); Kpad = 16 * (k-blocks to reduce over).  `part` (B, 4H): the cell runs over
    its LEADING Kpad columns and adds this slab of the products over the others; w_kbs = k-blocks per row tile of the whole packed matrix"""
    job = _lib.StLstmCellPackedJob(packed_w=_p(packed_w), x=x_view, K=int(Kpad), b_ih=_p(b_ih), b_hh=_p(b_hh), c_prev=_p(c_prev), ldc_prev=H,
                                   mask=_p(mask), h_dst0=h_dst0, c_out=_p(c_out), ldc=H, gates_out=_p(gates_out), ada_std=_p(ada_std),
                                   ada_mean=_p(ada_mean), B=int(B), H=int(H), part=_p(part), w_kbs=int(w_kbs))
    if h_dst1 is not None:
        job.h_dst1 = h_dst1
    if hadapt_dst is not None:
        job.hadapt_dst = hadapt_dst
    return job


def lstm_cell_packed(packed_w, x_view, Kpad, b_ih, b_hh, c_prev, h_dst0, c_out, B, H, h_dst1=None, mask=None,
                     gates_out=None, ada_std=None, ada_mean=None, hadapt_dst=None):
    job = lstm_cell_job(packed_w, x_view, Kpad, b_ih, b_hh, c_prev, h_dst0, c_out, B, H, h_dst1, mask, gates_out, ada_std, ada_mean, hadapt_dst)
    check(_lib.load().st_lstm_cell_packed_fwd(C.byref(job), stream_handle()), 'st_lstm_cell_packed_fwd')


def lstm_cell_packed_part(packed_w, w_kbs, x_view, Kpad, part, b_ih, b_hh, c_prev, h_dst0, c_out, B, H, h_dst1=None, mask=None, gates_out=None):
    """the cell over its LEADING Kpad columns + the slab `part` (B, 4H) of the products over the others"""
    assert part is not None
    job = lstm_cell_job(packed_w, x_view, Kpad, b_ih, b_hh, c_prev, h_dst0, c_out, B, H, h_dst1, mask, gates_out, part=part, w_kbs=w_kbs)
    check(_lib.load().st_lstm_cell_packed_fwd(C.byref(job), stream_handle()), 'st_lstm_cell_packed_fwd')


def partial_product(packed_w, w_kbs, kb0, KB, x_view, N, part, B):
    """part (B, N) = x[:, kb0 .. kb0 + KB) W[:, kb0 .. kb0 + KB)^T over a k-block range of a P16 matrix (st_partial_product_fwd); x_view.kb0 =
    the range's first k-block in the T16 buffer"""
    job = _lib.StPartialProductJob(packed_w=_p(packed_w), w_kbs=int(w_kbs), kb0=int(kb0), KB=int(KB), x=x_view, N=int(N), part=_p(part))
    check(_lib.load().st_partial_product_fwd(C.byref(job), int(B), stream_handle()), 'st_partial_product_fwd')
    return part


def packed_product(packed_w, x_view, Kpad, y, ldy, B, N):
    """StPackedProduct: y (B, N) = x W^T on packed operands (x_view: StT16View, Kpad = 16 * (k-blocks to reduce over); y may be None where the
    entry point allows it)"""
    return _lib.StPackedProduct(packed_w=_p(packed_w), x=x_view, K=int(Kpad), y=_p(y), ldy=int(ldy), B=int(B), N=int(N))


def packed_linear_job(packed_w, x_view, Kpad, B, N, y=None, y_dst=None, bias=None, act=None, mask=None,
                      n_split=0, y2=None, rep=0, n_split2=0, act2=None, mask2=None, y3_dst=None):
    """StPackedLinearJob (the arguments of skinny_linear_packed)"""
    ld = lambda t: int(t.stride(0)) if t is not None else 0
    job = _lib.StPackedLinearJob(p=packed_product(packed_w, x_view, Kpad, y, ld(y), B, N), bias=_p(bias), act=ACT[act], mask=_p(mask), ldmask=ld(mask),
                                 n_split=int(n_split), y2=_p(y2), ldy2=ld(y2), rep=int(rep),
                                 n_split2=int(n_split2), act2=ACT[act2], mask2=_p(mask2), ldmask2=ld(mask2))
    if y_dst is not None:
        job.y_dst = y_dst
    if y3_dst is not None:
        job.y3_dst = y3_dst
    return job


def skinny_linear_packed(packed_w, x_view, Kpad, B, N, **kw):
    job = packed_linear_job(packed_w, x_view, Kpad, B, N, **kw)
    check(_lib.load().st_skinny_linear_packed_fwd(C.byref(job), stream_handle()), 'st_skinny_linear_packed_fwd')


def skinny_linear_packed_attnpre(job, pre, part=None):
    """the linear `job` (packed_linear_job) with the attention-pre job `pre` (attn_pre_job) as extra workgroups of the same launch and,
    optionally, a hosted partial product `part` (StPartialProductJob) behind them: st_skinny_linear_packed_attnpre_fwd"""
    if part is not None:
        pre.part = C.addressof(part)
    check(_lib.load().st_skinny_linear_packed_attnpre_fwd(C.byref(job), C.byref(pre), stream_handle()), 'st_skinny_linear_packed_attnpre_fwd')


# --------------------------------------------------------------------------------------------- graphs
class Graph:
    """Records every st_* call issued inside `with g.capture():` on a private HIP stream into a
    hipGraph; `g.launch()` replays it on torch's current stream.  Every tensor touched inside the
    capture must stay alive as long as the graph is replayed: either allocated beforehand and kept
    by the caller, or allocated inside `with g.memory():` -- a private torch memory pool owned by
    this object, so that a buffer freed after the capture is never handed to anybody else (run the
    same code once inside `g.memory()` BEFORE the capture: the pool then serves the capture's
    allocations from its cache; a hipMalloc is not allowed while capturing)."""

    def __init__(self):
        self.lib = _lib.load()
        self.exec = None
        self._stream = C.c_void_p()
        check(self.lib.st_stream_create(C.byref(self._stream)), 'st_stream_create')
        self.pool = torch.cuda.MemPool()
        persist_status(torch.device('cuda', torch.cuda.current_device()))      # (allocated OUTSIDE the private pool: it outlives this graph)

    @contextmanager
    def memory(self):
        with torch.cuda.use_mem_pool(self.pool):
            yield

    @contextmanager
    def capture(self):
        torch.cuda.synchronize()
        check(self.lib.st_graph_begin(self._stream), 'st_graph_begin')
        ok = False
        try:
            with use_stream(self._stream.value):
                yield
            ok = True
        finally:
            ex = C.c_void_p()
            rc = self.lib.st_graph_end(self._stream, C.byref(ex))
            if ok:
                check(rc, 'st_graph_end')
                self.exec = ex

    def launch(self):
        check(self.lib.st_graph_launch(self.exec, stream_handle()), 'st_graph_launch')

    def __del__(self):
        try:
            if self.exec is not None:
                self.lib.st_graph_destroy(self.exec)
            self.lib.st_stream_destroy(self._stream)
        except Exception:
            pass


def device_info():
    lib = _lib.load()
    ncu, lds = C.c_int(), C.c_int()
    name = C.create_string_buffer(128)
    check(lib.st_device_info(C.byref(ncu), C.byref(lds), name, 128), 'st_device_info')
    return {'n_cu': ncu.value, 'lds_bytes': lds.value, 'name': name.value.decode()}


# --------------------------------------------------------------------------------------------- Griffin-Lim vocoder (src/audio.py)
def _audio_ws(fn, B, T, n_fft, hop, win, device):
    n = fn(B, T, n_fft, hop, win)
    if n == 0:
        raise RuntimeError('semi_tts_amd: bad STFT dimensions B=%d T=%d n_fft=%d hop=%d win=%d' % (B, T, n_fft, hop, win))
    return torch.empty(n, device=device, dtype=torch.float32)


def stft_fwd(x, n_fft, hop, win):
    """torch.stft(x (B, L), n_fft, hop, win, hann_window(win), center=True, pad_mode='reflect', onesided) on the HIP kernel:
    -> (B, T, n_fft // 2 + 1, 2) float32, frame-major (re, im), T = 1 + L // hop."""
    assert x.dim() == 2 and x.is_contiguous()
    B, L = x.shape
    spec = torch.empty(B, 1 + L // hop, n_fft // 2 + 1, 2, device=x.device, dtype=torch.float32)
    check(_lib.load().st_stft_fwd(_p(x), _p(spec), B, L, n_fft, hop, win, stream_handle()), 'st_stft_fwd')
    return spec


def istft(spec, n_fft, hop, win):
    """inverse of stft_fwd (lib/istft.py semantics, no `length`): spec (B, T, n_fft // 2 + 1, 2) -> (B, hop * (T - 1))"""
    assert spec.dim() == 4 and spec.shape[2] == n_fft // 2 + 1 and spec.shape[3] == 2 and spec.is_contiguous()
    B, T = spec.shape[:2]
    lib = _lib.load()
    ws = _audio_ws(lib.st_istft_workspace_floats, B, T, n_fft, hop, win, spec.device)
    x = torch.empty(B, hop * (T - 1), device=spec.device, dtype=torch.float32)
    check(lib.st_istft(_p(spec), _p(x), B, T, n_fft, hop, win, _p(ws), stream_handle()), 'st_istft')
    return x


GL_INV_PREEMPHASIS, GL_CLIP = 1, 2


def griffin_lim(feat, phases, n_fft, hop, win, n_iter=30, normalized=False, power=1.0, post=0):
    """griffin_lim_batch() on a linear spectrogram with one frame count: feat (B, T, F) in any strides (the decoder's (B, T, F) output
    or a transposed (B, F, T) magnitude), phases (B, F, T) contiguous -> waveform (B, hop * (T - 1)).  post: GL_INV_PREEMPHASIS | GL_CLIP."""
    return griffin_lim_batch(feat, phases, n_fft, hop, win, n_iter=n_iter, normalized=normalized, power=power, post=post)


MEL_TO_LINEAR_TILE = 16          # frames per workgroup of st_mel_to_linear (MEL_TILE in audio.hip): the tests straddle it
MEL_MAX = 256                    # most mel bins st_mel_to_linear takes (MEL_MAX in audio.hip)


def mel_to_linear(mel, basis, normalized=True, take_abs=False):
    """st_mel_to_linear: mel (B, T, n_mels) in any strides, basis (n_mels, F) contiguous (the transposed pseudo-inverse of the mel
    filterbank) -> (B, T, F) = sum_m basis[m, k] a[b, t, m], a the denormalised amplitude of mel (normalized) or mel itself;
    take_abs stores the magnitude Griffin-Lim takes."""
    assert mel.dim() == 3 and basis.dim() == 2 and basis.is_contiguous() and basis.shape[0] == mel.shape[2]
    B, T, n_mels = mel.shape
    F = basis.shape[1]
    lin = torch.empty(B, T, F, device=mel.device, dtype=torch.float32)
    sb, st, sm = mel.stride()
    check(_lib.load().st_mel_to_linear(_p(mel), sb, st, sm, _p(basis), _p(lin), B, T, n_mels, F, int(bool(normalized)),
                                       int(bool(take_abs)), stream_handle()), 'st_mel_to_linear')
    return lin


def griffin_lim_batch(feat, phases, n_fft, hop, win, n_iter=30, normalized=False, power=1.0, post=0, basis=None, frames=None):
    """st_griffin_lim_batch, the one vocoder entry: utterances of one length or of their own, linear or mel input.  feat (B, T, F)
    linear in any strides, or (B, T, n_mels) with basis (n_mels, F) as mel_to_linear() takes it; phases (B, F, T) contiguous; frames:
    device int32 (B,) frame counts (None: T for all).  -> waveform (B, hop * (T - 1)), row b filled on [0, hop * (frames[b] - 1))
    and zero after.  feat rows and phase columns beyond an utterance's frames are never read."""
    F = n_fft // 2 + 1
    assert feat.dim() == 3 and feat.shape[2] == (F if basis is None else basis.shape[0])
    B, T, n_in = feat.shape
    assert phases.shape == (B, F, T) and phases.is_contiguous()
    assert basis is None or (basis.shape == (n_in, F) and basis.is_contiguous())
    assert frames is None or (frames.shape == (B,) and frames.dtype == torch.int32 and frames.is_contiguous() and frames.is_cuda)
    lib = _lib.load()
    ws = _audio_ws(lib.st_gl_batch_workspace_floats, B, T, n_fft, hop, win, feat.device)
    wav = torch.empty(B, hop * (T - 1), device=feat.device, dtype=torch.float32)
    sb, st, sf = feat.stride()
    job = _lib.StGlJob(feat=_p(feat), sb=sb, st=st, sf=sf, n_in=n_in, basis=_p(basis), normalized=int(bool(normalized)), power=float(power),
                       phases=_p(phases), frames=_p(frames, torch.int32), wav=_p(wav), B=B, T=T, n_iter=int(n_iter), post=int(post))
    check(lib.st_griffin_lim_batch(C.byref(job), C.byref(_lib.StFraming(n_fft, win, hop)), _p(ws), stream_handle()), 'st_griffin_lim_batch')
    return wav


# --------------------------------------------------------------------------------------------- feature extraction (src/audio.py)
FEATURES_MAX_BATCH = 64          # utterances per st_audio_features call (its per-utterance metadata travels by value)


def _chunks(B):
    """(first utterance, count) of every call a batch of B utterances is issued in"""
    return [(b0, min(FEATURES_MAX_BATCH, B - b0)) for b0 in range(0, B, FEATURES_MAX_BATCH)]


def _host_ptr(a, b0):
    """address of row b0 of a contiguous host array (None stays None)"""
    return None if a is None else a.ctypes.data + b0 * a.itemsize


def _host_off_lens(off, lens):
    return np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int32)


def _wave_operands(x, n_fft, win, hop, fb):
    """the operands st_audio_features and st_audio_mfcc share: (StWaveBatch without its per-call off / len / B, StFraming, StMelBank)"""
    assert x.dim() == 1 and x.is_contiguous()
    fs, fc, fo, fw = fb
    return (_lib.StWaveBatch(x=_p(x), n_samples=x.numel()), _lib.StFraming(n_fft, win, hop),
            _lib.StMelBank(start=_p(fs, torch.int32), cnt=_p(fc, torch.int32), off=_p(fo, torch.int32), w=_p(fw), n_mels=fs.shape[0]))


def _wave_chunk(w, off, lens, b0, nb):
    """points the StWaveBatch `w` (modified in place) at utterances [b0, b0 + nb) and returns a reference to it"""
    w.off, w.len, w.B = _host_ptr(off, b0), _host_ptr(lens, b0), nb
    return C.byref(w)


def audio_features(x, off, lens, n_fft, win, hop, preemph, fb, T_pad, with_linear=True, aug_win=None, aug_hop=None, Ta_pad=None,
                   snr_db=None, noise=None, seed=0):
    """st_audio_features on a ragged batch: x the packed float32 waveforms (device), utterance b = x[off[b]:off[b] + lens[b]];
    fb = (start, count, offset, weights) device tensors of the banded mel filterbank.  -> (mel (B, T_pad, n_mels),
    linear (B, T_pad, n_fft // 2 + 1) or None, aug (B, Ta_pad, n_mels) or None); the augmented mel when aug_win / aug_hop (per
    utterance) are given, with noise at snr_db[b] (NaN: none) from `noise` (packed like x) or the built-in generator of `seed`.
    Batches above FEATURES_MAX_BATCH are issued in chunks of it; the generator is keyed on the position in the whole batch
    (feature_noise(n, b, seed) is utterance b's noise whatever B is)."""
    assert noise is None or (noise.shape == x.shape and noise.is_contiguous())
    w, fr, bank = _wave_operands(x, n_fft, win, hop, fb)
    n_mels, F = bank.n_mels, n_fft // 2 + 1
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    use_aug = aug_win is not None
    dev = x.device
    mel = torch.empty(B, T_pad, n_mels, device=dev, dtype=torch.float32)
    lin = torch.empty(B, T_pad, F, device=dev, dtype=torch.float32) if with_linear else None
    aug = torch.empty(B, Ta_pad, n_mels, device=dev, dtype=torch.float32) if use_aug else None
    if use_aug:
        aug_win = np.ascontiguousarray(aug_win, dtype=np.int32)
        aug_hop = np.ascontiguousarray(aug_hop, dtype=np.int32)
    if snr_db is not None:
        snr_db = np.ascontiguousarray(snr_db, dtype=np.float32)
    lib = _lib.load()
    ws = torch.empty(lib.st_features_workspace_floats(min(B, FEATURES_MAX_BATCH)), device=dev, dtype=torch.float32)
    a = _lib.StFeatAug(noise=_p(noise), seed=int(seed) & (2 ** 64 - 1), Ta_pad=Ta_pad or 0)
    for b0, nb in _chunks(B):
        a.win, a.hop, a.snr_db, a.utt0, a.out = _host_ptr(aug_win, b0), _host_ptr(aug_hop, b0), _host_ptr(snr_db, b0), b0, _p(aug[b0:]) if use_aug else None
        check(lib.st_audio_features(_wave_chunk(w, off, lens, b0, nb), C.byref(fr), float(preemph), C.byref(bank), C.byref(a), _p(mel[b0:]),
                                    _p(lin[b0:]) if with_linear else None, T_pad, _p(ws), stream_handle()), 'st_audio_features')
    return mel, lin, aug


def feature_noise(n, utt, seed, device):
    """the built-in noise generator of st_audio_features: (n,) standard normals of (seed, utterance utt, sample index)"""
    out = torch.empty(n, device=device, dtype=torch.float32)
    check(_lib.load().st_feature_noise(_p(out), n, utt, int(seed) & (2 ** 64 - 1), stream_handle()), 'st_feature_noise')
    return out


MFCC_MIN_FRAMES = 9              # fewest frames per utterance st_audio_mfcc takes: the width of the derivative filters


def audio_mfcc(x, off, lens, n_fft, win, hop, preemph, fb, dct, T_pad, with_mel=False):
    """st_audio_mfcc on a ragged batch packed as for audio_features: dct (n_mfcc, n_mels) float32 on the device (audio.mfcc_dct);
    win / hop: the MFCC framing.  -> (mfcc (B, T_pad, 3 * n_mfcc): cepstra, first and second derivatives; mel (B, T_pad, n_mels) at
    that framing, or None without with_mel).  Batches above FEATURES_MAX_BATCH are issued in chunks of it."""
    w, fr, bank = _wave_operands(x, n_fft, win, hop, fb)
    n_mels = bank.n_mels
    assert dct.dim() == 2 and dct.shape[1] == n_mels and dct.is_contiguous()
    n_mfcc = dct.shape[0]
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    out = torch.empty(B, T_pad, 3 * n_mfcc, device=x.device, dtype=torch.float32)
    mel = torch.empty(B, T_pad, n_mels, device=x.device, dtype=torch.float32) if with_mel else None
    lib = _lib.load()
    for b0, nb in _chunks(B):
        check(lib.st_audio_mfcc(_wave_chunk(w, off, lens, b0, nb), C.byref(fr), float(preemph), C.byref(bank), _p(dct), n_mfcc, _p(out[b0:]),
                                _p(mel[b0:]) if with_mel else None, T_pad, stream_handle()), 'st_audio_mfcc')
    return out, mel


def segment_gather(feat, seg_utt, seg_start, seg_len, max_len):
    """st_segment_gather: feat (B, T_pad, D) float32 on the device, rows contiguous; seg_utt / seg_start / seg_len: device int32 (S,).
    -> (S, max_len, D): row i < seg_len[s] of segment s = feat[seg_utt[s], seg_start[s] + i], every other row 0."""
    assert feat.dim() == 3 and feat.stride(2) == 1
    B, T_pad, D = feat.shape
    S = seg_utt.shape[0]
    for a in (seg_utt, seg_start, seg_len):
        assert a.shape == (S,) and a.dtype == torch.int32 and a.is_contiguous() and a.device == feat.device
    out = torch.empty(S, max_len, D, device=feat.device, dtype=torch.float32)
    check(_lib.load().st_segment_gather(_p(feat), feat.stride(0), feat.stride(1), B, T_pad, D, _p(seg_utt, torch.int32),
                                        _p(seg_start, torch.int32), _p(seg_len, torch.int32), S, int(max_len), _p(out), stream_handle()),
          'st_segment_gather')
    return out


# --------------------------------------------------------------------------------------------- sample-rate conversion
RESAMPLE_TILE = 1024                 # outputs per workgroup of st_resample_batch (RS_TILE in resample.hip): the tests straddle it
RESAMPLE_MAX_TABLE_FLOATS = 9216     # LDS floats of the staged table: min(n, RESAMPLE_TILE) rows of (taps | 1) + 1 (RS_MAX_TABLE)
RESAMPLE_MAX_STAGE_FLOATS = 6912     # LDS floats of a tile's input span (RS_MAX_STAGE)


def resample_lds_floats(o, n, taps, first_min, first_max):
    """(staged table floats, staged input floats) of one st_resample_batch workgroup at the ratio o / n: what the two limits bound"""
    return min(n, RESAMPLE_TILE) * ((taps | 1) + 1), ((RESAMPLE_TILE - 1) * o + n - 1) // n + first_max - first_min + taps


def resample_batch(x, off, lens, o, n, first, table, first_min, first_max, out=None):
    """st_resample_batch on a ragged batch: x the packed waveforms on the device, float32 or int16 PCM (scaled by 1 / 32768 in the
    kernel); utterance b = x[off[b]:off[b] + lens[b]].  first (n,) int32 and table (n, taps) float32: the device copies of
    audio.resample_table(); first_min / first_max the bounds of first.  -> (y, out_off, out_lens): the packed float32 output
    (`out`, a contiguous 1-D float32 device tensor of exactly the summed output lengths, or a new one), utterance b =
    y[out_off[b]:out_off[b] + out_lens[b]], out_lens[b] = ceil(n lens[b] / o).  Batches above FEATURES_MAX_BATCH are issued in
    chunks of it."""
    assert x.dim() == 1 and x.is_contiguous() and x.dtype in (torch.float32, torch.int16)
    assert table.dim() == 2 and table.shape[0] == n and table.is_contiguous() and table.dtype == torch.float32
    assert first.shape == (n,) and first.dtype == torch.int32 and first.is_contiguous()
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    out_lens = (lens.astype(np.int64) * n + o - 1) // o
    out_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(out_lens)[:-1]]), dtype=np.int64)
    total = int(out_lens.sum())
    if out is None:
        out = torch.empty(total, device=x.device, dtype=torch.float32)
    assert out.dim() == 1 and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == total and out.device == x.device
    lib = _lib.load()
    for b0, nb in _chunks(B):
        check(lib.st_resample_batch(_p(x, x.dtype), int(x.dtype == torch.int16), x.numel(), _host_ptr(off, b0), _host_ptr(lens, b0), nb,
                                    int(o), int(n), table.shape[1], int(first_min), int(first_max), _p(first, torch.int32), _p(table),
                                    _p(out), total, _host_ptr(out_off, b0), stream_handle()), 'st_resample_batch')
    return out, out_off, out_lens


# --------------------------------------------------------------------------------------------- pitch (st_f0_yin, st_f0_path_scores)
F0_MAX_TAU, F0_MAX_W = 1024, 2048    # st_f0_yin's limits
F0_RUN, F0_MAX_SPAN = 8, 10240       # frames a workgroup takes from one staged span, and the samples such a span may hold (f0.hip)


def f0_run_length(hop, W, tau_max):
    """the consecutive frames one st_f0_yin workgroup takes at this framing (st_f0_run_length): the tests straddle it"""
    r = F0_RUN
    while r > 1 and (r - 1) * int(hop) + int(W) + int(tau_max) > F0_MAX_SPAN:
        r -= 1
    return r


def _f0_check(lens, hop, W, tau_min, tau_max, sample_rate, threshold):
    """every refusal of st_f0_yin that does not need the buffers, raised before any device is touched"""
    for name, v in (('hop', hop), ('W', W), ('tau_min', tau_min), ('tau_max', tau_max)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('f0_yin: %s must be an integer (got %r)' % (name, v))
    if hop < 1:
        raise ValueError('f0_yin: hop %d below 1' % hop)
    if not 2 <= tau_min < tau_max <= F0_MAX_TAU:
        raise ValueError('f0_yin: lags [%d, %d] outside 2 <= tau_min < tau_max <= %d' % (tau_min, tau_max, F0_MAX_TAU))
    if not 1 <= W <= F0_MAX_W:
        raise ValueError('f0_yin: window W = %d outside [1, %d]' % (W, F0_MAX_W))
    threshold, sample_rate = float(threshold), float(sample_rate)
    if not 0.0 < threshold <= 1.0:
        raise ValueError('f0_yin: threshold must lie in (0, 1] (got %r)' % (threshold,))
    if not 0.0 < sample_rate < float('inf'):
        raise ValueError('f0_yin: sample_rate must be finite and positive (got %r)' % (sample_rate,))
    lens = np.asarray(lens)
    if lens.ndim != 1 or lens.shape[0] < 1 or lens.dtype.kind not in 'iu' or (lens < 1).any() or (lens >= 2 ** 31).any():
        raise ValueError('f0_yin: lens must be B >= 1 integers in [1, 2^31) (got %s)' % (lens.tolist(),))


def f0_yin(x, off, lens, hop, W, tau_min, tau_max, sample_rate, threshold, T_pad, with_aper=False):
    """st_f0_yin on a ragged batch packed as for audio_features: x the packed float32 waveforms on the device, utterance b =
    x[off[b]:off[b] + lens[b]].  -> (f0 (B, T_pad) in Hz, 0 on unvoiced frames and on the rows past 1 + lens[b] // hop; aper (B, T_pad),
    the normalised difference at the chosen lag, or None without with_aper).  Batches above FEATURES_MAX_BATCH are issued in chunks
    of it.  Anything the kernel would refuse raises ValueError before the device is touched."""
    _f0_check(lens, hop, W, tau_min, tau_max, sample_rate, threshold)
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('f0_yin: x must be a packed 1-D contiguous float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x).__name__))
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    if off.shape != (B,) or (off < 0).any() or (off + lens > x.numel()).any():
        raise ValueError('f0_yin: an utterance lies outside the %d packed samples (off %s, lens %s)' % (x.numel(), off.tolist(), lens.tolist()))
    T_pad = int(T_pad)
    if T_pad < 1 + int(lens.max()) // hop:
        raise ValueError('f0_yin: T_pad %d below the %d frames of the longest utterance' % (T_pad, 1 + int(lens.max()) // hop))
    lib = _lib.load()
    f0 = torch.empty(B, T_pad, device=x.device, dtype=torch.float32)
    aper = torch.empty(B, T_pad, device=x.device, dtype=torch.float32) if with_aper else None
    w = _lib.StWaveBatch(x=_p(x), n_samples=x.numel())
    for b0, nb in _chunks(B):
        check(lib.st_f0_yin(_wave_chunk(w, off, lens, b0, nb), int(hop), int(W), int(tau_min), int(tau_max), float(sample_rate), float(threshold),
                            _p(f0[b0:]), _p(aper[b0:]) if with_aper else None, T_pad, stream_handle()), 'st_f0_yin')
    return f0, aper


def f0_path_scores(f0_x, f0_y, path, path_len):
    """st_f0_path_scores: f0_x (B, Tx) and f0_y (B, Ty) float32 tracks on one GPU (unit stride along a row, any row stride), path
    (B, P, 2) int32 and path_len (B,) int32 on the same device.  THE PATH MUST COME FROM metrics.dtw / metrics.mcd over sequences of
    Tx and Ty rows (P = Tx + Ty - 1): the kernel reads its first path_len entries as indices without checking them.
    -> (counts (B, 4) int32 = (n_pairs, n_both, n_vuv, n_gross), sums (B, 2) float32 = (sum c^2, sum c) in cents over the both-voiced
    pairs) device tensors; one launch, no host read.  Anything else raises ValueError before the device is touched."""
    for name, t in (('f0_x', f0_x), ('f0_y', f0_y)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError('f0_path_scores: %s must be a (B, T) float32 GPU tensor (got %s)'
                             % (name, '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    dev = f0_x.device
    B, Tx = f0_x.shape
    Ty = f0_y.shape[1]
    if f0_y.device != dev or f0_y.shape[0] != B or B < 1 or Tx < 1 or Ty < 1:
        raise ValueError('f0_path_scores: f0_x is %s on %s, f0_y is %s on %s: B >= 1 pairs of at least one frame on one device'
                         % (tuple(f0_x.shape), f0_x.device, tuple(f0_y.shape), f0_y.device))
    strides = []
    for name, t in (('f0_x', f0_x), ('f0_y', f0_y)):
        sb = t.stride(0) if B > 1 else 0
        if (t.stride(1) != 1 and t.shape[1] > 1) or sb < 0:
            raise ValueError('f0_path_scores: %s has strides %s: a row needs unit stride' % (name, tuple(t.stride())))
        strides.append(sb)
    if (not torch.is_tensor(path) or not path.is_cuda or path.device != dev or path.dtype != torch.int32
            or tuple(path.shape) != (B, Tx + Ty - 1, 2) or not path.is_contiguous()):
        raise ValueError('f0_path_scores: path must be the contiguous (B, Tx + Ty - 1, 2) = (%d, %d, 2) int32 tensor of metrics.dtw on the device '
                         'of the tracks (got %s)' % (B, Tx + Ty - 1, '%s %s on %s' % (tuple(path.shape), path.dtype, path.device)
                                                     if torch.is_tensor(path) else type(path).__name__))
    if (not torch.is_tensor(path_len) or not path_len.is_cuda or path_len.device != dev or path_len.dtype != torch.int32
            or tuple(path_len.shape) != (B,) or not path_len.is_contiguous()):
        raise ValueError('f0_path_scores: path_len must be the (B,) int32 tensor of metrics.dtw on the device of the tracks (got %s)'
                         % ('%s %s on %s' % (tuple(path_len.shape), path_len.dtype, path_len.device) if torch.is_tensor(path_len)
                            else type(path_len).__name__))
    lib = _lib.load()
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    sums = torch.empty(B, 2, device=dev, dtype=torch.float32)
    check(lib.st_f0_path_scores(_p(f0_x), strides[0], Tx, _p(f0_y), strides[1], Ty, _p(path, torch.int32), _p(path_len, torch.int32), B,
                                Tx + Ty - 1, _p(counts, torch.int32), _p(sums), stream_handle()), 'st_f0_path_scores')
    return counts, sums


# --------------------------------------------------------------------------------------------- silence trimming (st_trim_silence)
TRIM_MAX_FRAME_LENGTH = 8192         # st_trim_silence's limit
TRIM_RUN, TRIM_MAX_SPAN = 16, 12288  # frames a workgroup takes from one staged span, and the samples such a span may hold (trim.hip)
TRIM_CHUNK = 256                     # frames per step of the decision launch: the tests straddle it


def trim_run_length(frame_length, hop):
    """the consecutive frames one st_trim_silence workgroup takes at this framing (st_trim_run_length): the tests straddle it"""
    r = TRIM_RUN
    while r > 1 and (r - 1) * int(hop) + int(frame_length) > TRIM_MAX_SPAN:
        r -= 1
    return r


def trim_ratio(top_db):
    """the threshold ratio of st_trim_silence: 10^(-top_db / 10) in double, rounded once to float32"""
    return float(np.float32(10.0 ** (-float(top_db) / 10.0)))


def _trim_check(lens, frame_length, hop, top_db, pad=0, max_iv=0):
    """every refusal of st_trim_silence that does not need the buffers, raised before any device is touched"""
    for name, v in (('frame_length', frame_length), ('hop', hop), ('pad', pad), ('max_iv', max_iv)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('trim_silence: %s must be an integer (got %r)' % (name, v))
    if not 1 <= hop <= frame_length <= TRIM_MAX_FRAME_LENGTH:
        raise ValueError('trim_silence: needs 1 <= hop <= frame_length <= %d (hop %d, frame_length %d)' % (TRIM_MAX_FRAME_LENGTH, hop, frame_length))
    if isinstance(top_db, bool) or not isinstance(top_db, (int, float, np.integer, np.floating)) or not np.isfinite(top_db):
        raise ValueError('trim_silence: top_db must be a finite number (got %r)' % (top_db,))
    if not 0.0 < trim_ratio(top_db) < 1.0:
        raise ValueError('trim_silence: top_db %r gives the ratio %r; it must lie strictly inside (0, 1) in float32'
                         % (top_db, trim_ratio(top_db)))
    if not 0 <= pad < 2 ** 31:
        raise ValueError('trim_silence: pad %d outside [0, 2^31)' % pad)
    if not 0 <= max_iv < 2 ** 30:
        raise ValueError('trim_silence: max_iv %d outside [0, 2^30)' % max_iv)
    lens = np.asarray(lens)
    if lens.ndim != 1 or lens.shape[0] < 1 or lens.dtype.kind not in 'iu' or (lens < 1).any() or (lens >= 2 ** 31).any():
        raise ValueError('trim_silence: lens must be B >= 1 integers in [1, 2^31) (got %s)' % (lens.tolist(),))


def trim_silence(x, off, lens, frame_length, hop, top_db, pad=0, max_iv=0, T_pad=None, energy=None):
    """st_trim_silence on a ragged batch packed as for audio_features: x the packed float32 waveforms on the device, utterance b =
    x[off[b]:off[b] + lens[b]] (the offsets need not be cumulative).  -> device tensors (energy (B, T_pad) float32, 0 on the rows past
    1 + lens[b] // hop; bounds (B, 4) int32 = (start, end, non-silent frames, flags); intervals (B, max_iv, 2) int32 and n_iv (B,)
    int32, or None, None with max_iv = 0).  T_pad None: the longest utterance's frames.  Batches above FEATURES_MAX_BATCH are
    issued in chunks of it.  energy: a contiguous (B, T_pad) float32 tensor on x's device to write the energies into (default: a new one).
    Anything the kernel would refuse raises ValueError before the device is touched."""
    _trim_check(lens, frame_length, hop, top_db, pad, max_iv)
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('trim_silence: x must be a packed 1-D contiguous float32 GPU tensor (got %s)'
                         % ('%s %s on %s' % (tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x).__name__))
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    if off.shape != (B,) or (off < 0).any() or (off + lens > x.numel()).any():
        raise ValueError('trim_silence: an utterance lies outside the %d packed samples (off %s, lens %s)' % (x.numel(), off.tolist(), lens.tolist()))
    frames = 1 + int(lens.max()) // hop
    T_pad = frames if T_pad is None else int(T_pad)
    if T_pad < frames:
        raise ValueError('trim_silence: T_pad %d below the %d frames of the longest utterance' % (T_pad, frames))
    lib = _lib.load()
    dev = x.device
    if energy is None:
        energy = torch.empty(B, T_pad, device=dev, dtype=torch.float32)
    elif not (torch.is_tensor(energy) and energy.shape == (B, T_pad) and energy.dtype == torch.float32 and energy.is_contiguous() and energy.device == dev):
        raise ValueError('trim_silence: energy must be a contiguous (%d, %d) float32 tensor on %s' % (B, T_pad, dev))
    bounds = torch.empty(B, 4, device=dev, dtype=torch.int32)
    iv = torch.empty(B, max_iv, 2, device=dev, dtype=torch.int32) if max_iv else None
    n_iv = torch.empty(B, device=dev, dtype=torch.int32) if max_iv else None
    ratio = trim_ratio(top_db)
    w = _lib.StWaveBatch(x=_p(x), n_samples=x.numel())
    for b0, nb in _chunks(B):
        check(lib.st_trim_silence(_wave_chunk(w, off, lens, b0, nb), int(frame_length), int(hop), ratio, int(pad), int(max_iv), _p(energy[b0:]),
                                  T_pad, _p(bounds[b0:], torch.int32), _p(iv[b0:], torch.int32) if max_iv else None,
                                  _p(n_iv[b0:], torch.int32) if max_iv else None, stream_handle()), 'st_trim_silence')
    return energy, bounds, iv, n_iv


# --------------------------------------------------------------------------------------------- loudness (st_loudness_batch, st_wave_gain)
LOUDNESS_MIN_SR, LOUDNESS_MAX_SR = 8000, 48000     # st_loudness_batch's limits
LOUDNESS_THREADS = 256                             # runs a hop is cut into (loudness.hip)
LOUDNESS_TABLE_DOUBLES = 152 + 256 * 16            # ST_LOUDNESS_TABLE_DOUBLES
LOUDNESS_FLAGS = {'nonfinite': 1, 'short': 2, 'silent': 4, 'peak_limited': 8, 'gain_limited': 16}


def loudness_hop(sr):
    """samples of a 100 ms hop at this rate: (sr + 5) // 10"""
    return (int(sr) + 5) // 10


def loudness_run_length(sr):
    """the samples one st_loudness_batch thread owns at this rate (st_loudness_run_length): the tests straddle it"""
    return (loudness_hop(sr) + LOUDNESS_THREADS - 1) // LOUDNESS_THREADS


def _loudness_check(lens, sr, target=None, peak_db=-1.0, max_gain_db=30.0, H_pad=None):
    """every refusal of st_loudness_batch that does not need the buffers, raised before any device is touched -> (hop, H_pad)"""
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or not LOUDNESS_MIN_SR <= sr <= LOUDNESS_MAX_SR:
        raise ValueError('loudness: the sample rate must be an integer in [%d, %d] (got %r)' % (LOUDNESS_MIN_SR, LOUDNESS_MAX_SR, sr))
    for name, v in (('peak_db', peak_db), ('max_gain_db', max_gain_db)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError('loudness: %s must be a finite number (got %r)' % (name, v))
    if target is not None and (isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)) or np.isinf(target)):
        raise ValueError('loudness: target must be a finite number, or None / NaN to measure only (got %r)' % (target,))
    lens = np.asarray(lens)
    if lens.ndim != 1 or not 1 <= lens.shape[0] <= FEATURES_MAX_BATCH or lens.dtype.kind not in 'iu':
        raise ValueError('loudness: lens must be 1 .. %d integers, one call takes no more utterances (got %s)'
                         % (FEATURES_MAX_BATCH, 'shape %s, %s' % (lens.shape, lens.dtype)))
    if (lens < 1).any() or (lens >= 2 ** 31).any():
        raise ValueError('loudness: every length must lie in [1, 2^31) (got %s)' % (lens.tolist(),))
    hop = loudness_hop(sr)
    hops = int(lens.max()) // hop
    if H_pad is None:
        H_pad = max(1, hops)
    if isinstance(H_pad, bool) or not isinstance(H_pad, (int, np.integer)) or H_pad < hops or H_pad >= 2 ** 31:
        raise ValueError('loudness: H_pad %r below the %d hops of the longest utterance' % (H_pad, hops))
    return hop, int(H_pad)


def _wave_args(what, x, off, lens):
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('%s: x must be a packed 1-D contiguous float32 GPU tensor (got %s)'
                         % (what, '%s %s on %s' % (tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x).__name__))
    B = len(lens)
    off, lens = _host_off_lens(off, lens)
    if off.shape != (B,) or (off < 0).any() or (off + lens > x.numel()).any():
        raise ValueError('%s: an utterance lies outside the %d packed samples (off %s, lens %s)' % (what, x.numel(), off.tolist(), lens.tolist()))
    return off, lens


def loudness(x, off, lens, sr, target=None, peak_db=-1.0, max_gain_db=30.0, H_pad=None):
    """st_loudness_batch (ITU-R BS.1770-4 integrated loudness; the definition is in include/semitts.h) on a ragged batch packed as for
    audio_features: x the packed float32 waveforms on the device, utterance b = x[off[b]:off[b] + lens[b]], at most FEATURES_MAX_BATCH
    of them (the callers above split).  -> device tensors (hop_energy (B, H_pad) float32, stats (B, 8) float32 = (L_I, momentary
    maximum, relative gate, sample peak, ungated, gain, 0, 0), counts (B, 4) int32 = (blocks, above the absolute gate, above the
    relative gate, flags)).  target None (or NaN): measure only, gain 1.  H_pad None: the longest utterance's hops (at least 1).
    Four launches, no host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    hop, H_pad = _loudness_check(lens, sr, target, peak_db, max_gain_db, H_pad)
    off, lens = _wave_args('loudness', x, off, lens)
    from .audio import kweight_tables                          # (here: audio imports this module)
    lib = _lib.load()
    dev = x.device
    tab = kweight_tables(sr, dev)
    B = len(lens)
    hop_energy = torch.empty(B, H_pad, device=dev, dtype=torch.float32)
    stats = torch.empty(B, 8, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    ws = torch.empty(B * (H_pad + 1) * 9, device=dev, dtype=torch.float64)
    w = _lib.StWaveBatch(x=_p(x), n_samples=x.numel())
    check(lib.st_loudness_batch(_wave_chunk(w, off, lens, 0, B), int(sr), _p(tab, torch.float64), float('nan') if target is None else float(target),
                                float(peak_db), float(max_gain_db), _p(hop_energy), H_pad, _p(stats), _p(counts, torch.int32),
                                _p(ws, torch.float64), stream_handle()), 'st_loudness_batch')
    return hop_energy, stats, counts


def wave_gain(x, off, lens, stats, out=None, pcm16=False):
    """st_wave_gain: utterance b of the packed batch times the gain stats[b, 5] of `loudness`, read on the device (no host read).
    pcm16 False -> float32, one product a sample, written into `out` (a packed buffer like x; x itself is allowed: in place; default a
    new buffer of zeros).  pcm16 True -> int16, rint(clip(x g, -1, 1) * 32767) as audio.write_wav, into `out` (int16, x's size) or a
    new buffer of zeros.  Samples outside the utterances are not written.  At most FEATURES_MAX_BATCH utterances a call."""
    lens_a = np.asarray(lens)
    if lens_a.ndim != 1 or not 1 <= lens_a.shape[0] <= FEATURES_MAX_BATCH or lens_a.dtype.kind not in 'iu' or (lens_a < 1).any() or (lens_a >= 2 ** 31).any():
        raise ValueError('wave_gain: lens must be 1 .. %d integers in [1, 2^31) (got %s)' % (FEATURES_MAX_BATCH, lens_a.tolist()))
    off, lens = _wave_args('wave_gain', x, off, lens)
    B = len(lens)
    dt = torch.int16 if pcm16 else torch.float32
    if not (torch.is_tensor(stats) and stats.is_cuda and stats.device == x.device and stats.dtype == torch.float32 and tuple(stats.shape) == (B, 8)
            and stats.is_contiguous()):
        raise ValueError('wave_gain: stats must be the contiguous (%d, 8) float32 tensor of loudness() on %s' % (B, x.device))
    if out is None:
        out = torch.zeros(x.numel(), device=x.device, dtype=dt)
    elif not (torch.is_tensor(out) and out.device == x.device and out.dtype == dt and out.dim() == 1 and out.numel() == x.numel() and out.is_contiguous()):
        raise ValueError('wave_gain: out must be a contiguous 1-D %s tensor of %d samples on %s' % (dt, x.numel(), x.device))
    lib = _lib.load()
    w = _lib.StWaveBatch(x=_p(x), n_samples=x.numel())
    check(lib.st_wave_gain(_wave_chunk(w, off, lens, 0, B), _p(stats), None if pcm16 else _p(out), _p(out, torch.int16) if pcm16 else None,
                           stream_handle()), 'st_wave_gain')
    return out


# --------------------------------------------------------------------------------------------- intelligibility (st_stoi_batch)
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT = 10000, 256, 128, 512
STOI_BANDS, STOI_SEG = 15, 30
STOI_MAX_BATCH = 64                  # st_stoi_batch's limits: pairs a call ...
STOI_MAX_LEN = 1 << 22               # ... and samples of the longest signal (7 minutes at 10 kHz)
STOI_CHUNK = 256                     # frames per step of the selection launch's scan: the tests straddle it
STOI_SENTINEL = 1e-5                 # both scores of a pair with fewer than 30 band frames (pystoi's convention)
STOI_BAND_EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
                   (109, 138), (138, 174), (174, 219))


def stoi_frames(L):
    """F of an L-sample signal at 10 kHz: the frames i with 128 i < L - 256 (strict, as the authors' code); 0 when L <= 256"""
    L = int(L)
    return (L - STOI_FRAME + STOI_HOP - 1) // STOI_HOP if L > STOI_FRAME else 0


def _stoi_check(lens, F_pad=None):
    """every refusal of st_stoi_batch that does not need the buffers, raised before any device is touched -> F_pad"""
    lens = np.asarray(lens)
    if lens.ndim != 1 or not 0 <= lens.shape[0] <= STOI_MAX_BATCH or (lens.shape[0] and lens.dtype.kind not in 'iu'):
        raise ValueError('stoi_batch: lens must be 0 .. %d integers, one call takes no more pairs (got %s)'
                         % (STOI_MAX_BATCH, 'shape %s, %s' % (lens.shape, lens.dtype)))
    if lens.shape[0] and ((lens < 1).any() or (lens > STOI_MAX_LEN).any()):
        raise ValueError('stoi_batch: every length must lie in [1, %d] (got %s)' % (STOI_MAX_LEN, lens.tolist()))
    frames = max([1] + [stoi_frames(v) for v in lens])
    if F_pad is None:
        F_pad = frames
    if isinstance(F_pad, bool) or not isinstance(F_pad, (int, np.integer)) or F_pad < frames or F_pad >= 2 ** 24:
        raise ValueError('stoi_batch: F_pad %r below the %d frames of the longest signal (at least 1)' % (F_pad, frames))
    return int(F_pad)


def stoi_batch(x, y, off, lens, F_pad=None, want_parts=False):
    """st_stoi_batch (STOI and ESTOI; the definition is in include/semitts.h) on a ragged batch of pairs at 10 kHz: x the packed float32
    clean signals on the device, y the processed ones packed the same way (x's size), pair b = x / y[off[b]:off[b] + lens[b]], at most
    STOI_MAX_BATCH of them (metrics.stoi splits).  -> device tensors (score (B, 2) float32 = (STOI, ESTOI), counts (B, 4) int32 =
    (frames F, kept K, band frames M, segments S), and with want_parts energy (B, F_pad) float32, kept (B, F_pad) int32 with -1 past K,
    bands (B, 2, 15, F_pad) float32 with 0 past M; None, None, None without).  F_pad None: the longest signal's frames (at least 1).
    B = 0 launches nothing.  No host read.  Anything the kernel would refuse raises ValueError before the device is touched."""
    F_pad = _stoi_check(lens, F_pad)
    if not torch.is_tensor(y) or not torch.is_tensor(x) or y.shape != x.shape or y.device != x.device or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError('stoi_batch: y must be a packed 1-D contiguous float32 tensor of x\'s size on x\'s device (got %s)'
                         % ('%s %s on %s' % (tuple(y.shape), y.dtype, y.device) if torch.is_tensor(y) else type(y).__name__))
    off, lens = _wave_args('stoi_batch', x, off, lens)
    lib = _lib.load()
    dev = x.device
    B = len(lens)
    score = torch.empty(B, 2, device=dev, dtype=torch.float32)
    counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
    energy = torch.empty(B, F_pad, device=dev, dtype=torch.float32) if want_parts else None
    kept = torch.empty(B, F_pad, device=dev, dtype=torch.int32) if want_parts else None
    bands = torch.empty(B, 2, STOI_BANDS, F_pad, device=dev, dtype=torch.float32) if want_parts else None
    if B == 0:
        return score, counts, energy, kept, bands
    ws = torch.empty(int(lib.st_stoi_workspace_floats(B, F_pad)), device=dev, dtype=torch.float32)
    w = _lib.StWaveBatch(x=_p(x), n_samples=x.numel())
    check(lib.st_stoi_batch(_wave_chunk(w, off, lens, 0, B), _p(y), _p(score), _p(counts, torch.int32), F_pad, _p(energy), _p(kept, torch.int32),
                            _p(bands), _p(ws), stream_handle()), 'st_stoi_batch')
    return score, counts, energy, kept, bands


# --------------------------------------------------------------------------------------------- alignment (st_xcorr_delay, st_sisdr_batch, st_wave_gather)
XCORR_MAX_BATCH = 64                 # st_xcorr_delay's limits: pairs a call ...
XCORR_MAX_LEN = 1 << 22              # ... samples of the longest signal of either side ...
XCORR_MAX_LAG = 16384                # ... and the search bound D (+-0.34 s at 48 kHz)
XCORR_CHUNK = 1024                   # samples of a staged piece, the smallest chunk of x: the tests straddle it
XCORR_LAG_TILE = 2048                # lags a workgroup owns: the tests straddle it
XCORR_MAX_CHUNKS = 32                # chunks of the longest signal: past 32 * 1024 samples the chunk grows
SISDR_CHUNK = 8192                   # samples a workgroup of st_sisdr_batch's first launch sums


def xcorr_chunk_len(L):
    """samples of one chunk of an L-sample reference: XCORR_CHUNK times the smallest factor that leaves at most XCORR_MAX_CHUNKS chunks"""
    return XCORR_CHUNK * ((int(L) + XCORR_CHUNK * XCORR_MAX_CHUNKS - 1) // (XCORR_CHUNK * XCORR_MAX_CHUNKS))


def _pair_check(what, xlens, ylens, max_lag=0):
    """every refusal of st_xcorr_delay / st_sisdr_batch that does not need the buffers, raised before any device is touched"""
    xl, yl = np.asarray(xlens), np.asarray(ylens)
    for name, v in (('x', xl), ('y', yl)):
        if v.ndim != 1 or not 0 <= v.shape[0] <= XCORR_MAX_BATCH or (v.shape[0] and v.dtype.kind not in 'iu'):
            raise ValueError('%s: the lengths of %s must be 0 .. %d integers, one call takes no more pairs (got %s)'
                             % (what, name, XCORR_MAX_BATCH, 'shape %s, %s' % (v.shape, v.dtype)))
        if v.shape[0] and ((v < 1).any() or (v > XCORR_MAX_LEN).any()):
            raise ValueError('%s: every length of %s must lie in [1, %d] (got %s)' % (what, name, XCORR_MAX_LEN, v.tolist()))
    if xl.shape[0] != yl.shape[0]:
        raise ValueError('%s: %d references and %d processed signals: one of each per pair' % (what, xl.shape[0], yl.shape[0]))
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= XCORR_MAX_LAG:
        raise ValueError('%s: max_lag must be an integer in [0, %d] (got %r)' % (what, XCORR_MAX_LAG, max_lag))


def _pair_args(what, x, xoff, xlens, y, yoff, ylens):
    xoff, xlens = _wave_args(what, x, xoff, xlens)
    if not torch.is_tensor(y) or y.device != x.device:
        raise ValueError('%s: y must be a packed 1-D contiguous float32 tensor on x\'s device' % what)
    yoff, ylens = _wave_args(what, y, yoff, ylens)
    wx, wy = _lib.StWaveBatch(x=_p(x), n_samples=x.numel()), _lib.StWaveBatch(x=_p(y), n_samples=y.numel())
    B = len(xlens)
    return _wave_chunk(wx, xoff, xlens, 0, B), _wave_chunk(wy, yoff, ylens, 0, B), (wx, wy, xoff, xlens, yoff, ylens)


def xcorr_delay(x, xoff, xlens, y, yoff, ylens, max_lag, want_corr=False):
    """st_xcorr_delay (the definition is in include/semitts.h): the integer delay of B pairs by direct float64 cross-correlation over
    the lags [-max_lag, max_lag].  x, y: two packed float32 device buffers, pair b = x[xoff[b]:xoff[b] + xlens[b]] against
    y[yoff[b]:yoff[b] + ylens[b]] (the lengths may differ, the offsets need not be cumulative), at most XCORR_MAX_BATCH pairs
    (metrics.delay splits).  -> device tensors (delay (B,) int32, positive: y is late; coef (B,) float32; corr (B, 2 max_lag + 1)
    float64 with want_corr, else None).  B = 0 launches nothing.  No host read.  Anything the kernel would refuse raises ValueError
    before the device is touched."""
    _pair_check('xcorr_delay', xlens, ylens, max_lag)
    px, py, keep = _pair_args('xcorr_delay', x, xoff, xlens, y, yoff, ylens)
    lib = _lib.load()
    dev, B, D = x.device, len(keep[3]), int(max_lag)
    delay = torch.empty(B, device=dev, dtype=torch.int32)
    coef = torch.empty(B, device=dev, dtype=torch.float32)
    corr = torch.empty(B, 2 * D + 1, device=dev, dtype=torch.float64) if want_corr else None
    if B == 0:
        return delay, coef, corr
    max_len = int(max(keep[3].max(), keep[5].max()))
    ws = torch.empty(int(lib.st_xcorr_workspace_bytes(B, max_len, D)) // 8, device=dev, dtype=torch.float64)
    check(lib.st_xcorr_delay(px, py, D, _p(delay, torch.int32), _p(coef), _p(corr, torch.float64), _p(ws, torch.float64), stream_handle()),
          'st_xcorr_delay')
    return delay, coef, corr


def sisdr_batch(x, xoff, xlens, y, yoff, ylens, delay=None, zero_mean=True):
    """st_sisdr_batch (the definition is in include/semitts.h): SI-SDR, SNR and gain of B pairs on the overlap a delay leaves.  x, y as
    for xcorr_delay.  delay: None (0) or a DEVICE int32 tensor (B,), read on the device only: the caller checks its values where they
    come from the host.  -> device tensors (score (B, 3) float32 = (SI-SDR dB, SNR dB, gain dB), sums (B, 6) float64 = (n, sum x, sum y,
    sum x^2, sum y^2, sum x y)).  B = 0 launches nothing.  No host read."""
    _pair_check('sisdr_batch', xlens, ylens)
    B = len(xlens)
    if delay is not None and not (torch.is_tensor(delay) and delay.is_cuda and delay.dtype == torch.int32 and tuple(delay.shape) == (B,)
                                  and delay.is_contiguous() and torch.is_tensor(x) and delay.device == x.device):
        raise ValueError('sisdr_batch: delay must be None or a contiguous (%d,) int32 tensor on x\'s device (got %s)'
                         % (B, '%s %s on %s' % (tuple(delay.shape), delay.dtype, delay.device) if torch.is_tensor(delay) else type(delay).__name__))
    px, py, keep = _pair_args('sisdr_batch', x, xoff, xlens, y, yoff, ylens)
    lib = _lib.load()
    dev = x.device
    score = torch.empty(B, 3, device=dev, dtype=torch.float32)
    sums = torch.empty(B, 6, device=dev, dtype=torch.float64)
    if B == 0:
        return score, sums
    max_len = int(max(keep[3].max(), keep[5].max()))
    ws = torch.empty(int(lib.st_sisdr_workspace_bytes(B, max_len)) // 8, device=dev, dtype=torch.float64)
    check(lib.st_sisdr_batch(px, py, _p(delay, torch.int32), int(bool(zero_mean)), _p(sums, torch.float64), _p(score), _p(ws, torch.float64),
                             stream_handle()), 'st_sisdr_batch')
    return score, sums


def wave_gather(src, src_off, dst, dst_off, lens):
    """st_wave_gather: dst[dst_off[b]:dst_off[b] + lens[b]] = src[src_off[b]:src_off[b] + lens[b]] for at most XCORR_MAX_BATCH spans in one
    launch; src, dst: two different contiguous 1-D float32 buffers on one device; nothing else of dst is written.  -> dst"""
    la = np.asarray(lens)
    if la.ndim != 1 or not 0 <= la.shape[0] <= XCORR_MAX_BATCH or (la.shape[0] and (la.dtype.kind not in 'iu' or (la < 1).any() or (la > XCORR_MAX_LEN).any())):
        raise ValueError('wave_gather: lens must be 0 .. %d integers in [1, %d] (got %s)' % (XCORR_MAX_BATCH, XCORR_MAX_LEN, la.tolist()))
    B = la.shape[0]
    so, do = np.asarray(src_off), np.asarray(dst_off)
    if so.shape != (B,) or do.shape != (B,) or (B and (so.dtype.kind not in 'iu' or do.dtype.kind not in 'iu')):
        raise ValueError('wave_gather: src_off and dst_off must hold %d integers each' % B)
    for name, t in (('src', src), ('dst', dst)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('wave_gather: %s must be a contiguous 1-D float32 GPU tensor (got %s)'
                             % (name, '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    if src.device != dst.device or src.data_ptr() == dst.data_ptr():
        raise ValueError('wave_gather: src and dst must be two different buffers on one device')
    if B == 0:
        return dst
    so, do = np.ascontiguousarray(so, dtype=np.int64), np.ascontiguousarray(do, dtype=np.int64)
    la = np.ascontiguousarray(la, dtype=np.int32)
    if (so < 0).any() or (so + la > src.numel()).any() or (do < 0).any() or (do + la > dst.numel()).any():
        raise ValueError('wave_gather: a span lies outside its buffer (src %d samples, dst %d; src_off %s, dst_off %s, lens %s)'
                         % (src.numel(), dst.numel(), so.tolist(), do.tolist(), la.tolist()))
    lib = _lib.load()
    check(lib.st_wave_gather(_p(src), src.numel(), so.ctypes.data, _p(dst), dst.numel(), do.ctypes.data, la.ctypes.data, B, stream_handle()),
          'st_wave_gather')
    return dst
