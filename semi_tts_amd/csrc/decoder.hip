// decoder.hip -- the autoregressive decode loop of Decoder.forward, issued natively.
//
// ref: src/module.py:184-206 (loop + next-input policy) and :216-288 (one step).
// Once per forward the six weight matrices the loop streams every step are packed into MFMA
// lane order (skinny_packed.hip, "P16"); all per-step activations live in the tiled "T16"
// layout, written that way by their producers.  Per step the loop enqueues, in dependency order:
//   1. query LSTM cell      x = [dec_in | ctx_{t-1} | h_q] (ONE tiled buffer per step), fused AdaIN of the new h_q
//   2. query projection     pq = W_q h_q
//   3. attention step       energies, softmax, context, cumulative weights   (attention.hip)
//   4. decoder LSTM cell    x = [ctx_t | adapted h_q | h_d]
//   5. proj + gate          [h_d | ctx_t] -> r mel frames + stop logit
//   6. next input           teacher frame (tiled copy) and/or prenet(own output) (2 launches)
// There is no host synchronisation, allocation or blocking copy inside, so the whole loop
// can be captured into a hipGraph (st_graph_begin/st_graph_end) and replayed as one launch.
// State lives in caller-owned tapes indexed by step; nothing is overwritten, so the same
// buffers are the saved tensors of the backward pass.
#include "st_common.h"
#include "loop_graph.h"
#include <cstdlib>

namespace {

// zero up to twelve buffers in one launch (blockIdx.y = buffer): the tapes' initial slots and the hand-off words of a forward
struct ZeroArgs { float* p[12]; size_t floats[12]; int n; };
__global__ __launch_bounds__(256) void zero_regions_kernel(const ZeroArgs a) {
    float* __restrict__ p = a.p[blockIdx.y];
    const size_t n = a.floats[blockIdx.y];
    const size_t n4 = (((uintptr_t)p & 15u) == 0) ? n / 4 : 0;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) reinterpret_cast<f32x4*>(p)[i] = z;
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.0f;
}

}  // namespace

extern "C" size_t st_packed_weight_floats(const int* k, int nseg, int N, int lstm_H);
extern "C" size_t st_t16_floats(int B, int K);

namespace {

struct PackedLayout {   // offsets (floats) of the six packed matrices inside the packed buffer
    size_t q, pq, d, pg, p0, p1, total;
};

PackedLayout packed_layout(const st_decoder_dims* d) {
    PackedLayout o;
    const int in_dim = d->r * d->n_mels;
    size_t p = 0;
    { int k[3] = {d->P, d->E, d->Q}; o.q = p; p += st_packed_weight_floats(k, 3, 4 * d->Q, d->Q); }
    { int k[1] = {d->Q}; o.pq = p; p += st_packed_weight_floats(k, 1, d->A, 0); }
    { int k[3] = {d->E, d->Q, d->D}; o.d = p; p += st_packed_weight_floats(k, 3, 4 * d->D, d->D); }
    { int k[2] = {d->D, d->E}; o.pg = p; p += st_packed_weight_floats(k, 2, in_dim + 1 + (d->fuse_pre0 ? d->P : 0), 0); }
    { int k[1] = {in_dim}; o.p0 = p; p += st_packed_weight_floats(k, 1, d->P, 0); }
    { int k[1] = {d->P}; o.p1 = p; p += st_packed_weight_floats(k, 1, d->P, 0); }
    o.total = p;
    return o;
}

inline int kb16(int k) { return (k + 15) >> 4; }

struct StepViews {   // k-block geometry of the three step-input buffers
    int q_kbs, q_ctx, q_h;        // xq = [dec_in | ctx | h_q]
    int d_kbs, d_ha, d_h;         // xd = [ctx | hadapt | h_d]
    int o_kbs, o_ctx;             // xo = [h_d | ctx]
    size_t q_floats, d_floats, o_floats;
};

StepViews step_views(const st_decoder_dims* d) {
    StepViews v;
    const int bt = (d->B + 15) >> 4;
    v.q_ctx = kb16(d->P); v.q_h = v.q_ctx + kb16(d->E); v.q_kbs = v.q_h + kb16(d->Q);
    v.d_ha = kb16(d->E); v.d_h = v.d_ha + kb16(d->Q); v.d_kbs = v.d_h + kb16(d->D);
    v.o_ctx = kb16(d->D); v.o_kbs = v.o_ctx + kb16(d->E);
    v.q_floats = (size_t)bt * v.q_kbs * 256; v.d_floats = (size_t)bt * v.d_kbs * 256; v.o_floats = (size_t)bt * v.o_kbs * 256;
    return v;
}

// dec_in_{s} = teacher frame min(s-1, Tt-1) for every step s = 1..steps-1 and row b < Bt, written straight into the
// dec_in k-blocks of the xq tape (slot s) in T16 order: one launch instead of one st_tile_rows per step
__global__ __launch_bounds__(256) void tile_teacher_kernel(const float* teacher_pre, int Tt, float* xq_tape, size_t slot_floats,
                                                           int q_kbs, int steps, int Bt, int P) {
    const size_t total = (size_t)(steps - 1) * Bt * P;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % P);
        const size_t sb = i / P;
        const int b = (int)(sb % Bt), s = (int)(sb / Bt) + 1;
        const int frame = s - 1 < Tt ? s - 1 : Tt - 1;
        const float v = teacher_pre[((size_t)b * Tt + frame) * P + k];
        xq_tape[(size_t)s * slot_floats + (((size_t)(b >> 4) * q_kbs + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (b & 15)) * 4 + (k & 3)] = v;
    }
}

int prenet_own(const st_decoder_weights* w, const st_decoder_dims* d, const st_decoder_io* io, const PackedLayout& pl, const StepViews& sv,
               int t, bool layer1_done, void* stream) {
    // dec_in_{t+1} = prenet(mel_t) for every row                ref: src/module.py:192,:197-198,:205-206
    const int in_dim = d->r * d->n_mels;
    const size_t BP = (size_t)d->B * d->P;
    const float* m1 = io->prenet_mask ? io->prenet_mask + ((size_t)t * 2 + 0) * BP : nullptr;
    const float* m2 = io->prenet_mask ? io->prenet_mask + ((size_t)t * 2 + 1) * BP : nullptr;
    st_t16_view mel = {io->mel_t16, kb16(in_dim), 0};
    st_t16_view pre1 = {io->pre1_t16 + (size_t)t * io->pre1_step_floats, kb16(d->P), 0};
    int rc = 0;
    if (d->prenet_norm) {
        // normalised prenet (Linear -> LayerNorm / BatchNorm1d -> ReLU -> dropout, src/module.py:337-339,508-521): the Linear's
        // output stays in natural layout, the norm launch applies norm + ReLU + mask and writes the T16 operand of the next product
        st_t16_view next_n = {io->xq_tape + (size_t)(t + 1) * sv.q_floats, sv.q_kbs, 0};
        const st_t16_view* dsts[2] = {&pre1, &next_n};
        const st_t16_view* srcs[2] = {&mel, &pre1};
        const float* pw[2] = {io->packed + pl.p0, io->packed + pl.p1};
        const int Ks[2] = {16 * kb16(in_dim), 16 * kb16(d->P)};
        const float* ms[2] = {m1, m2};
        // the rows that feed back: all of them on an own-output step, the ones without a teacher otherwise -- the batch of a
        // BatchNorm1d step (the products run over every row; rows < b0 of the next input come from the teacher afterwards)
        const int b0 = io->step_src[t] == -1 ? 0 : io->Bt;
        for (int l = 0; l < 2; ++l) {
            float* y = io->pre_nat_tape ? io->pre_nat_tape + ((size_t)t * 2 + l) * BP : io->pre_nat;
            const st_packed_linear_job lj = st_plain_linear_job(pw[l], *srcs[l], Ks[l], y, d->P, d->B, d->P);
            rc = st_skinny_linear_packed_fwd(&lj, stream);
            if (rc) return rc;
            rc = st_prenet_norm_fwd(y, d->P, d->prenet_norm, w->pre_norm_w[l], w->pre_norm_b[l], w->pre_norm_rm[l], w->pre_norm_rv[l],
                                    w->pre_norm_nbt[l], w->pre_norm_eps, w->pre_norm_momentum, ms[l], d->P, dsts[l], b0, d->B, d->P, stream);
            if (rc) return rc;
        }
        return 0;
    }
    // a prenet layer: relu(x W^T) * mask -> a T16 destination only
    auto layer = [&](const float* packed_w, const st_t16_view& x, int K, const float* mask, const st_t16_view& dst) {
        st_packed_linear_job lj = st_plain_linear_job(packed_w, x, K, nullptr, 0, d->B, d->P);
        lj.act = ST_ACT_RELU; lj.mask = mask; lj.ldmask = d->P; lj.y_dst = dst;
        return st_skinny_linear_packed_fwd(&lj, stream);
    };
    if (!layer1_done) rc = layer(io->packed + pl.p0, mel, 16 * kb16(in_dim), m1, pre1);
    if (rc) return rc;
    st_t16_view next = {io->xq_tape + (size_t)(t + 1) * sv.q_floats, sv.q_kbs, 0};
    return layer(io->packed + pl.p1, pre1, 16 * kb16(d->P), m2, next);
}

}  // namespace

extern "C" int st_decoder_gate_split_k(const st_decoder_dims* d) {
    if (!d) return 0;
    const StepViews sv = step_views(d);
    int hosted = (sv.d_kbs / 2) / 16 * 16;                 // k-blocks that ride beside pq / fin: half the reduction, whole rounds of 16
    if (hosted < 16 || hosted > sv.d_kbs - sv.d_ha) hosted = sv.d_kbs - sv.d_ha;
    return 16 * (sv.d_kbs - hosted);
}

extern "C" size_t st_decoder_packed_floats(const st_decoder_dims* d) { return d ? packed_layout(d).total : 0; }

extern "C" int st_decoder_pack(const st_decoder_weights* w, const st_decoder_dims* d, float* packed, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(w && d && packed, "st_decoder_pack: null pointer");
    const PackedLayout pl = packed_layout(d);
    const int in_dim = d->r * d->n_mels;
    st_pack_job j[6];
    memset(j, 0, sizeof(j));
    auto seg = [&](st_pack_job& q, int s, const float* wp, int ld, int k) { q.w[s] = wp; q.ldw[s] = ld; q.k[s] = k; q.nseg = s + 1; };
    // query LSTM: K = [dec_in (P) | ctx (E) | h_q (Q)]                       ref: src/module.py:227-228
    seg(j[0], 0, w->q_w_ih, d->P + d->E, d->P); seg(j[0], 1, w->q_w_ih + d->P, d->P + d->E, d->E); seg(j[0], 2, w->q_w_hh, d->Q, d->Q);
    j[0].N = 4 * d->Q; j[0].lstm_H = d->Q; j[0].packed = packed + pl.q;
    seg(j[1], 0, w->attn_query_w, d->Q, d->Q); j[1].N = d->A; j[1].packed = packed + pl.pq;
    // decoder LSTM: K = [ctx (E) | adapted h_q (Q) | h_d (D)]                 ref: src/module.py:275-277
    seg(j[2], 0, w->d_w_ih, d->E + d->Q, d->E); seg(j[2], 1, w->d_w_ih + d->E, d->E + d->Q, d->Q); seg(j[2], 2, w->d_w_hh, d->D, d->D);
    j[2].N = 4 * d->D; j[2].lstm_H = d->D; j[2].packed = packed + pl.d;
    // proj (+) gate: K = [h_d (D) | ctx (E)]                                  ref: src/module.py:282-287
    seg(j[3], 0, w->projgate_w, d->D + d->E, d->D); seg(j[3], 1, w->projgate_w + d->D, d->D + d->E, d->E);
    j[3].N = in_dim + 1 + (d->fuse_pre0 ? d->P : 0); j[3].packed = packed + pl.pg;
    seg(j[4], 0, w->prenet_w0, in_dim, in_dim); j[4].N = d->P; j[4].packed = packed + pl.p0;
    seg(j[5], 0, w->prenet_w1, d->P, d->P); j[5].N = d->P; j[5].packed = packed + pl.p1;
    return st_pack_weight_batch(j, 6, stream);       // one launch for the six (they were ~10 us each)
}

extern "C" size_t st_decoder_tape_floats(const st_decoder_dims* d, int which) {
    if (!d) return 0;
    const StepViews sv = step_views(d);
    return which == 0 ? sv.q_floats : (which == 1 ? sv.d_floats : sv.o_floats);
}

namespace {

// How the decode loop issues its steps, decided once per forward (st_decoder_fwd_forms reports it).  Host arithmetic only: no HIP call,
// no device memory read; step_src is the one host array it looks into.  `cus` = the device's compute units, `rng_capacity` = the
// workgroups of the one-launch range form (pk_attnrng_kernel) the device holds at once: the forms whose workgroups wait for each other
// inside a launch need all of them resident.
enum FwdAttn {          // steps 2 + 3: query projection and attention
    ATTN_WHOLE,         //   pq launch, then the whole attention step
    ATTN_PRE_FIN,       //   pq launch, then the fin part from S (the pre part ran in the proj launch of the step before, or in the pq launch)
    ATTN_FIN_SPLIT,     //   pq launch, then the fin part over position ranges + a combine launch (long texts)
    ATTN_PQ_FIN,        //   pq + fin part as one launch (pq handed over inside the launch as granules)
    ATTN_PQ_RNG         //   pq + fin part over position ranges + combine as one launch (long texts)
};
enum FwdProd {          // where the decoder cell's partial gate product (io->gate_part) runs
    PROD_NONE,          //   nowhere: the cell reduces its whole K
    PROD_OWN,           //   in a launch of its own before the cell
    PROD_PQ_FIN,        //   beside the pq + fin launch
    PROD_PQ_PRE         //   beside the pq + attention-pre launch (step 0 has no pre part: a launch of its own there)
};
struct FwdForms {
    bool pure_tf;       // every next input is a teacher frame for every row: the inputs of all steps are tiled before the loop
    bool defer;         // no proj (+) gate launch per step: the caller computes mel / stop of all steps after the loop
    bool pre_in_pq;     // the attention pre part of step t rides in the pq launch of step t (else in the proj launch of step t-1)
    bool pair_cells;    // the decoder cell of step t and the query cell of step t+1 as one launch
    FwdAttn attn;
    FwdProd prod;
    int fin_parts;      // workgroups per utterance of the fin part (ATTN_PRE_FIN, ATTN_PQ_FIN)
    int pq_pre_parts;   // ... of the pre part inside the pq launch
    int d_k0;           // k-blocks of the decoder cell's reduction that stay in the cell launch (with a partial product)
};

FwdForms fwd_forms(const st_decoder_dims* d, const st_decoder_io* io, int cus, int rng_capacity) {
    FwdForms f;
    const int B = d->B, L = d->L, E = d->E, Q = d->Q, D = d->D, A = d->A, BT = (B + 15) / 16;
    // pure teacher forcing (every next input is teacher frame min(t, Tt-1), all rows have a teacher): the inputs of all
    // steps are tiled into the tape up front, and with io->defer_proj the projection is left to the caller (one GEMM
    // over all steps instead of one launch per step -- no step's input depends on an earlier output)
    f.pure_tf = io->teacher_pre && io->Bt == B && io->Tt > 0;
    for (int t = 0; t + 1 < io->steps && f.pure_tf; ++t) f.pure_tf = io->step_src[t] == (t < io->Tt ? t : io->Tt - 1);
    f.defer = io->defer_proj != 0;
    // teacher-forced training (deferred projection): [decoder cell of t | query cell of t+1] as one launch
    f.pair_cells = f.defer && f.pure_tf && io->pair_cells;
    // Attention in two parts (io->attn_s_buf set by the host): the location part of step t+1 ("pre": conv + W_l + processed
    // memory -> S) only needs the attention weights of step t, so it rides as extra workgroups of a small launch that runs
    // anyway -- the proj launch of step t when the loop has one, otherwise (deferred projection = teacher-forced training) the
    // query-projection launch of step t+1 itself.  The attention launch then starts from S ("fin").
    // Measured and removed: early LSTM inputs on a second stream, as side jobs of the small launches, and as
    // distributed side jobs over four launches of the step -- all slower than the plain chain of dependent launches.
    const bool split_attn = io->attn_s_buf != nullptr;
    f.pre_in_pq = split_attn && f.defer;
    const int fp_req = io->attn_fin_parts;
    f.fin_parts = (fp_req == 2 || fp_req == 4 || fp_req == 8) && E % (4 * fp_req) == 0 ? fp_req : 1;
    // long texts: the fin part split over position ranges + a combine launch (see at_split_kernel) ...
    const int sp = io->attn_split_parts;
    const bool fin_split = split_attn && io->attn_split_ws && sp >= 2 && sp <= 64 && A % 4 == 0 && A <= 256 && E % 4 == 0 &&
                           E / 4 <= 512 && 512 % (E / 4) == 0 && (L + sp - 1) / sp <= 512;
    // ... or, when the device holds all its workgroups at once, query projection + fin part over position ranges + combine as ONE launch
    const bool fin_rng = fin_split && !f.pre_in_pq && io->pq_granules && io->attn_xchg && sp <= 8 && A % 16 == 0 && E % (4 * sp) == 0 &&
                         E / sp <= 256 && (sp - 1) * ((L + sp - 1) / sp) < L && (A / 16) * BT + B * sp <= rng_capacity;
    // query projection + attention fin part as one launch with an in-launch hand-off of pq (st_query_attn_fin_fwd): needs the split
    // attention step and every workgroup of the launch resident at once
    const bool fuse_pq_fin = !fin_split && split_attn && !f.pre_in_pq && io->pq_granules && A % 16 == 0 && A <= 256 && E % 4 == 0 &&
                             (A / 16) * BT + B * f.fin_parts <= cus;
    f.attn = !split_attn ? ATTN_WHOLE : fin_rng ? ATTN_PQ_RNG : fin_split ? ATTN_FIN_SPLIT : fuse_pq_fin ? ATTN_PQ_FIN : ATTN_PRE_FIN;
    // io->gate_part: the decoder cell's gate products over [AdaIN(h_q(t)) | h_d(t-1)] -- known before the attention of step t runs -- ride
    // beside the pq / fin launch; the cell launch reduces the context columns and adds the slab.  Measured (round 6, two boxes, A/B in
    // one process): 2.71 -> 2.79 and 2.78 -> 2.84 M mel-frames/s.  The same for the query cell, or the two halves at two sites, LOSE
    // (DESIGN.md section 3.5): a hosted product costs ~7 us + 3 us per 1024 columns whatever its host's length.
    // (the other forms of the attention step issue the partial product as a launch of its own: same arithmetic bit for bit, so a starved
    // hand-off that degrades to the two-launch form changes nothing but the speed)
    // Teacher-forced training (deferred projection) has the same split: there the product rides beside the query projection + attention pre
    // part of the step (its operands come from the paired cell launch of the step before), the paired launch adds the slab.
    const bool split_d = io->gate_part && (!f.defer || f.pre_in_pq) && B > 16 && B <= 32 && D % 16 == 0 && (D / 4) % 2 == 0 &&
                         E % 16 == 0 && Q % 16 == 0 && st_aligned16(io->gate_part);
    // (two attention-pre workgroups per utterance beside the product: with four, 16 + 128 + 128 workgroups would not fit the device in one round)
    const int pre_parts_split = io->attn_pre_parts > 2 ? 2 : io->attn_pre_parts;
    const bool split_pre = split_d && f.pre_in_pq && A <= 16 * 128 &&
                           ((A + 15) / 16) * BT + B * (pre_parts_split > 1 ? pre_parts_split : 1) + (4 * D) / 32 <= cus;
    f.pq_pre_parts = split_pre ? pre_parts_split : io->attn_pre_parts;
    if (!split_d) f.prod = PROD_NONE;
    else if (split_pre) f.prod = PROD_PQ_PRE;
    else if (fuse_pq_fin && (A / 16) * BT + B * f.fin_parts + (4 * D) / 32 <= cus) f.prod = PROD_PQ_FIN;
    else f.prod = PROD_OWN;
    // ... how much of it: measured at C2 (hosted 512 / 768 / 1024 / 1280 / 1536 / 2048 columns: 2.78 / 2.83 / 2.88 / 2.89 / 2.86 / 2.81 M
    // mel-frames/s, whole rounds of 16 k-blocks for the 8 waves x 2 only -- 1088 ... 1408 in steps of 64 all lose to 1280): the cell keeps half.
    f.d_k0 = (io->gate_part_k ? io->gate_part_k : st_decoder_gate_split_k(d)) / 16;
    return f;
}

}  // namespace

int pk_attnrng_capacity();      // (skinny_packed.hip)

extern "C" int st_decoder_fwd_forms(const st_decoder_dims* d, const st_decoder_io* io, int cus, int rng_capacity) {
    if (!d || !io || (io->steps > 1 && !io->step_src)) return -1;
    const FwdForms f = fwd_forms(d, io, cus > 0 ? cus : st_device_cus(), rng_capacity > 0 ? rng_capacity : pk_attnrng_capacity());
    return (int)f.attn | ((int)f.prod << 4) | (f.pure_tf ? 1 << 8 : 0) | (f.defer ? 1 << 9 : 0) | (f.pre_in_pq ? 1 << 10 : 0) |
           (f.pair_cells ? 1 << 11 : 0) | (f.fin_parts << 12) | ((f.prod != PROD_NONE ? f.d_k0 & 0xfff : 0) << 16);
}

static int decoder_forward_issue(const st_decoder_weights* w, const st_decoder_dims* d, const st_decoder_io* io, void* stream);

static stlg::Cache g_fwd_graphs;
extern "C" void st_loop_graph_stats(long* fwd3, long* bwd3);      // (defined in decoder_bwd.hip: {replays, captures, eager} of both loops)
extern "C" void stx_fwd_loop_graph_stats(long* out3) {
    std::lock_guard<std::mutex> lock(g_fwd_graphs.mu);
    out3[0] = g_fwd_graphs.replays; out3[1] = g_fwd_graphs.captures; out3[2] = g_fwd_graphs.eager;
}

extern "C" int st_decoder_forward(const st_decoder_weights* w, const st_decoder_dims* d, const st_decoder_io* io,
                                  void* stream) {
    (void)hipGetLastError();  // drop stale errors left by other HIP users of this thread
    ST_CHECK_ARG(w && d && io, "st_decoder_forward: null struct pointer");
    // the teacher-forced loop of a training step (tapes kept, projection deferred) comes back with bit-identical arguments step after step:
    // captured at the second sighting, replayed with one launch afterwards (loop_graph.h)
    if (io->defer_proj && io->steps > 0 && io->step_src && stlg::enabled(d->B)) {
        st_decoder_io key_io = *io;
        key_io.step_src = nullptr;                       // (a host array: its CONTENTS are part of the key, not its address)
        uint64_t key = stlg::fnv(stlg::FNV0, w, sizeof(*w));
        key = stlg::fnv(key, d, sizeof(*d));
        key = stlg::fnv(key, &key_io, sizeof(key_io));
        key = stlg::fnv(key, io->step_src, sizeof(int) * (size_t)io->steps);
        stlg::Entry* e = nullptr;
        hipStream_t issue_on = (hipStream_t)stream;
        const int mode = stlg::begin(g_fwd_graphs, key, (hipStream_t)stream, &e, &issue_on);
        if (mode == 1) return 0;
        int rc = decoder_forward_issue(w, d, io, (void*)issue_on);
        if (mode == 2) {
            rc = stlg::end(g_fwd_graphs, e, (hipStream_t)stream, rc);
            if (rc == -5) st_set_error("st_decoder_forward: capturing the loop into a hipGraph failed");
        }
        return rc;
    }
    return decoder_forward_issue(w, d, io, stream);
}

static int decoder_forward_issue(const st_decoder_weights* w, const st_decoder_dims* d, const st_decoder_io* io, void* stream) {
    ST_CHECK_ARG(w && d && io, "st_decoder_forward: null struct pointer");
    const int B = d->B, L = d->L, E = d->E, P = d->P, Q = d->Q, D = d->D, A = d->A;
    const int steps = io->steps;
    const int in_dim = d->r * d->n_mels;
    ST_CHECK_ARG(B > 0 && L > 0 && steps > 0 && in_dim > 0, "st_decoder_forward: B=%d L=%d steps=%d", B, L, steps);
    ST_CHECK_ARG(io->memory && io->pm && io->ada_std && io->ada_mean && io->step_src && io->packed,
                 "st_decoder_forward: null input");
    ST_CHECK_ARG(io->mel_out && io->align_out && io->stop_out, "st_decoder_forward: null output");
    ST_CHECK_ARG(io->xq_tape && io->xd_tape && io->xo_tape && io->cq_tape && io->cd_tape && io->wcum_tape &&
                 io->pq_buf && io->pre1_t16 && io->mel_t16 && io->zero_row, "st_decoder_forward: null tape/scratch");
    ST_CHECK_ARG(d->prenet_norm >= 0 && d->prenet_norm <= 3 && (!d->prenet_norm || (!d->fuse_pre0 && io->pre_nat && w->pre_norm_w[0] &&
                 w->pre_norm_w[1] && w->pre_norm_b[0] && w->pre_norm_b[1])), "st_decoder_forward: normalised prenet needs pre_nat, the norm weights and fuse_pre0 = 0");
    for (int t = 0; t + 1 < steps; ++t) {
        const int src = io->step_src[t];
        ST_CHECK_ARG(!d->fuse_pre0 || src == -1, "st_decoder_forward: fuse_pre0 needs every next input to be the own output");
        ST_CHECK_ARG(src >= -2 && (src < 0 || (io->teacher_pre && src < io->Tt)), "st_decoder_forward: step_src[%d]=%d invalid", t, src);
        ST_CHECK_ARG(src != -2 || io->teacher_mean, "st_decoder_forward: step_src[%d]=-2 without teacher_mean", t);
        ST_CHECK_ARG(src == -1 || (io->Bt > 0 && io->Bt <= B), "st_decoder_forward: Bt=%d invalid", io->Bt);
    }
    const StepViews sv = step_views(d);
    ST_CHECK_ARG(io->gate_part_k == 0 || !io->gate_part || (io->gate_part_k % 16 == 0 && io->gate_part_k >= 16 * sv.d_ha && io->gate_part_k < 16 * sv.d_kbs),
                 "st_decoder_forward: gate_part_k = %d must be a multiple of 16 in [%d, %d)", io->gate_part_k, 16 * sv.d_ha, 16 * sv.d_kbs);
    FwdForms f = fwd_forms(d, io, st_device_cus(), pk_attnrng_capacity());
    ST_CHECK_ARG(!f.defer || (f.pure_tf && !d->fuse_pre0), "st_decoder_forward: defer_proj needs pure teacher forcing");
    // Ablation (timing experiments only: tools/gpu_ablate.sh builds a SEPARATE library with -DST_ABLATE and times the loop with the
    // launches of the bit mask ST_SKIP left out; the outputs are garbage then).  Bits: 0 query cell, 1 query projection, 2 attention,
    // 3 decoder cell (paired or not), 4 proj (+) gate, 5 own-output prenet, 6 the attention pre part inside the proj launch, 7 the proj
    // launch over a quarter of its reduction.  Bit 1 or bit 2 skips a merged pq + fin launch.  A skipped launch takes the partial product
    // it hosts with it, and so does bit 3: the cell then reduces its whole K.
#ifdef ST_ABLATE
    const int skip = getenv("ST_SKIP") ? atoi(getenv("ST_SKIP")) : 0;
    if ((skip & 8) || (f.prod == PROD_PQ_FIN && (skip & 6)) || (f.prod == PROD_PQ_PRE && (skip & 2))) f.prod = PROD_NONE;
#define ST_SKIPPED(bit) (skip & (1 << (bit)))
#else
#define ST_SKIPPED(bit) 0
#endif
    hipStream_t st = (hipStream_t)stream;
    const PackedLayout pl = packed_layout(d);
    const size_t BQ = (size_t)B * Q, BD = (size_t)B * D, BL = (size_t)B * L;
    // The tiled tapes are handed in zero-filled (torch.zeros): slot 0 of xq / the h_d part of xd slot 0
    // are the initial zero state (src/module.py:290-303) and dec_in_0 = prenet(go frame) = 0 (:161,:183).
    // (one launch for all of them, together with the hand-off words: eight memset nodes were 25 us of every forward)
    ZeroArgs za;
    memset(&za, 0, sizeof(za));
    auto zero = [&](void* p, size_t bytes) { za.p[za.n] = (float*)p; za.floats[za.n] = bytes / sizeof(float); ++za.n; };
    zero(io->cq_tape, BQ * sizeof(float));
    zero(io->cd_tape, BD * sizeof(float));
    zero(io->wcum_tape, BL * sizeof(float));
    zero(io->zero_row, BL * sizeof(float));
    zero(io->xq_tape, sv.q_floats * sizeof(float));
    zero(io->xd_tape, sv.d_floats * sizeof(float));
    if (io->attn_loc_tape) zero(io->attn_loc_tape, BL * d->F * sizeof(float));      // (slot 0: no step writes it -- there is no history yet)
    // the granule words of the in-launch hand-offs, zeroed before the first step (a memset node when the loop is captured: a replay must
    // not see the tags of the previous one)
    const int sp_parts = io->attn_split_parts;
    if (f.attn == ATTN_PQ_FIN || f.attn == ATTN_PQ_RNG) zero(io->pq_granules, (size_t)B * A * sizeof(unsigned long long));
    if (f.attn == ATTN_PQ_RNG) zero(io->attn_xchg, st_attn_rng_xchg_words(B, E, sp_parts) * sizeof(unsigned long long));
    {
        size_t most = 0;
        for (int i = 0; i < za.n; ++i) most = za.floats[i] > most ? za.floats[i] : most;
        size_t blocks = (most / 4 + 255) / 256 + 1;
        if (blocks > 256) blocks = 256;
        hipLaunchKernelGGL(zero_regions_kernel, dim3((unsigned)blocks, za.n), dim3(256), 0, st, za);
        ST_LAUNCH_CHECK();
    }
    if (io->dec_in0) {      // dec_in_0 = prenet(go frame) of a normalised prenet (a plain one gives the zeros the tape holds already)
        st_t16_view xq0 = {io->xq_tape, sv.q_kbs, 0};
        int rc0 = st_tile_rows(io->dec_in0, P, &xq0, B, P, stream);
        if (rc0) return rc0;
    }
    if (f.pure_tf && steps > 1) {
        const size_t total = (size_t)(steps - 1) * B * P;
        size_t blocks = (total + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(tile_teacher_kernel, dim3((unsigned)blocks), dim3(256), 0, st, io->teacher_pre, io->Tt, io->xq_tape,
                           sv.q_floats, sv.q_kbs, steps, B, P);
        ST_LAUNCH_CHECK();
    }

    const size_t ldmel = (size_t)steps * in_dim;
    const int ldal = steps * L;
    const int Kq = 16 * sv.q_kbs, Kd = 16 * sv.d_kbs, Ko = 16 * sv.o_kbs;
    st_partial_product_job pj_d;      // the tail of the decoder cell's gate product (f.prod), wherever it runs
    memset(&pj_d, 0, sizeof(pj_d));
    pj_d.packed_w = io->packed + pl.d; pj_d.w_kbs = sv.d_kbs; pj_d.kb0 = f.d_k0; pj_d.KB = sv.d_kbs - f.d_k0; pj_d.N = 4 * D; pj_d.part = io->gate_part;
    const bool part = f.prod != PROD_NONE;      // the decoder cell reduces its first d_k0 k-blocks and adds the slab
    // the two cells of step t (1. and 4. below)
    auto cell_q = [&](int t) {      // x = xq_t, h_q_t -> xq_{t+1}[h part], AdaIN(h_q_t) -> xd_t[hadapt part]
        st_lstm_cell_packed_job j;
        memset(&j, 0, sizeof(j));
        j.packed_w = io->packed + pl.q; j.x = st_t16_view{io->xq_tape + (size_t)t * sv.q_floats, sv.q_kbs, 0}; j.K = Kq;
        j.b_ih = w->q_b_ih; j.b_hh = w->q_b_hh;
        j.c_prev = io->cq_tape + (size_t)t * BQ; j.ldc_prev = Q; j.mask = io->q_mask ? io->q_mask + (size_t)t * BQ : nullptr;
        j.h_dst0 = st_t16_view{io->xq_tape + (size_t)(t + 1) * sv.q_floats, sv.q_kbs, sv.q_h};
        j.c_out = io->cq_tape + (size_t)(t + 1) * BQ; j.ldc = Q;
        j.gates_out = io->gates_q_tape ? io->gates_q_tape + (size_t)t * 4 * BQ : nullptr;
        j.ada_std = io->ada_std; j.ada_mean = io->ada_mean; j.hadapt_dst = st_t16_view{io->xd_tape + (size_t)t * sv.d_floats, sv.d_kbs, sv.d_ha};
        j.B = B; j.H = Q;
        return j;
    };
    auto cell_d = [&](int t) {      // x = xd_t, h_d_t -> xd_{t+1}[h part], xo_t[h part]
        st_lstm_cell_packed_job j;
        memset(&j, 0, sizeof(j));
        j.packed_w = io->packed + pl.d; j.x = st_t16_view{io->xd_tape + (size_t)t * sv.d_floats, sv.d_kbs, 0}; j.K = Kd;
        j.b_ih = w->d_b_ih; j.b_hh = w->d_b_hh;
        if (part) { j.K = 16 * f.d_k0; j.part = io->gate_part; j.w_kbs = sv.d_kbs; }
        j.c_prev = io->cd_tape + (size_t)t * BD; j.ldc_prev = D; j.mask = io->d_mask ? io->d_mask + (size_t)t * BD : nullptr;
        j.h_dst0 = st_t16_view{io->xd_tape + (size_t)(t + 1) * sv.d_floats, sv.d_kbs, sv.d_h};
        j.h_dst1 = st_t16_view{io->xo_tape + (size_t)t * sv.o_floats, sv.o_kbs, 0};
        j.c_out = io->cd_tape + (size_t)(t + 1) * BD; j.ldc = D;
        j.gates_out = io->gates_d_tape ? io->gates_d_tape + (size_t)t * 4 * BD : nullptr;
        j.B = B; j.H = D;
        return j;
    };
    // the attention pre part of step t (needs only the weights of step t-1): beside the pq launch of step t or the proj launch of step t-1
    auto pre_job = [&](int t, int parts) {
        return st_attn_pre_job{io->pm, io->align_out + (size_t)(t - 1) * L, ldal, io->wcum_tape + (size_t)t * BL,
                               w->attn_loc_conv_w, w->attn_loc_lin_w,
                               f.attn != ATTN_WHOLE ? io->attn_s_buf + (size_t)t * io->attn_s_step_floats : nullptr, L, A, d->F, d->K,
                               parts, io->attn_loc_tape ? io->attn_loc_tape + (size_t)t * BL * d->F : nullptr, nullptr};
    };
    int rc = 0;
    for (int t = 0; t < steps; ++t) {
        float* xq_next = io->xq_tape + (size_t)(t + 1) * sv.q_floats;
        float* xd = io->xd_tape + (size_t)t * sv.d_floats;
        float* xo = io->xo_tape + (size_t)t * sv.o_floats;
        pj_d.x = st_t16_view{xd, sv.d_kbs, f.d_k0};

        // 1. query LSTM (+ AdaIN of the new hidden state)                ref: :227-231, :267-269
        //    h_q_t -> xq_{t+1}[h part] (next step's recurrent input, also the query projection's input)
        //    adapted h_q_t -> xd_t[hadapt part]
        st_t16_view hq_dst = {xq_next, sv.q_kbs, sv.q_h};
        // (pair_cells: the query cell of step t > 0 ran beside the decoder cell of step t-1, see step 4)
        if (!(f.pair_cells && t > 0) && !ST_SKIPPED(0)) {
            const st_lstm_cell_packed_job jq = cell_q(t);
            rc = st_lstm_cell_packed_fwd(&jq, stream);
            if (rc) return rc;
        }

        // 2. processed query (the merged forms issue it with step 3)    ref: :380
        if (f.attn != ATTN_PQ_FIN && f.attn != ATTN_PQ_RNG && !ST_SKIPPED(1)) {
            const st_packed_linear_job pq = st_plain_linear_job(io->packed + pl.pq, hq_dst, 16 * kb16(Q), io->pq_buf, A, B, A);
            if (f.pre_in_pq && t > 0) {   // attention pre part of THIS step rides along (needs only the weights of step t-1)
                st_attn_pre_job job = pre_job(t, f.pq_pre_parts);
                if (f.prod == PROD_PQ_PRE) job.part = &pj_d;      // ... and the tail of the decoder cell's gate product of this step
                rc = st_skinny_linear_packed_attnpre_fwd(&pq, &job, stream);
            } else
                rc = st_skinny_linear_packed_fwd(&pq, stream);
            if (rc) return rc;
        }

        // 3. attention + state update                                    ref: :256-264, :371-407
        //    ctx_t -> xq_{t+1}[ctx part], xd_t[ctx part], xo_t[ctx part]
        st_t16_view ctx_dst[3] = {{xq_next, sv.q_kbs, sv.q_ctx}, {xd, sv.d_kbs, 0}, {xo, sv.o_kbs, sv.o_ctx}};
        // S of this step: written by the pre part (step 0: no history yet, S = pm)
        const float* s_t = t == 0 || f.attn == ATTN_WHOLE ? io->pm : io->attn_s_buf + (size_t)t * io->attn_s_step_floats;
        auto fin_job = [&](int parts) {      // the fin part of the step, in whichever launch it runs
            st_attn_fin_job fj;
            memset(&fj, 0, sizeof(fj));
            fj.s_buf = s_t; fj.memory = io->memory; fj.w_cum_prev = io->wcum_tape + (size_t)t * BL;
            fj.w_out = io->align_out + (size_t)t * L; fj.ld_wout = ldal; fj.w_cum_out = io->wcum_tape + (size_t)(t + 1) * BL; fj.v = w->attn_v;
            for (int c = 0; c < 3; ++c) fj.ctx_dst[c] = ctx_dst[c];
            fj.status = io->handoff_status;
            fj.n_ctx_dst = 3; fj.parts = parts; fj.L = L; fj.A = A; fj.E = E; fj.F = d->F; fj.K = d->K;
            return fj;
        };
        switch (f.attn) {
        case ATTN_WHOLE:
            if (!ST_SKIPPED(2)) {
                st_attn_step_job sj;
                memset(&sj, 0, sizeof(sj));
                sj.pq = io->pq_buf; sj.pm = io->pm; sj.memory = io->memory;
                sj.w_prev = t == 0 ? io->zero_row : io->align_out + (size_t)(t - 1) * L; sj.ld_wprev = t == 0 ? L : ldal;
                sj.w_cum_prev = io->wcum_tape + (size_t)t * BL;
                sj.w_out = io->align_out + (size_t)t * L; sj.ld_wout = ldal; sj.w_cum_out = io->wcum_tape + (size_t)(t + 1) * BL;
                sj.loc_conv_w = w->attn_loc_conv_w; sj.loc_lin_w = w->attn_loc_lin_w; sj.v = w->attn_v;
                for (int c = 0; c < 3; ++c) sj.ctx_dst[c] = ctx_dst[c];
                sj.n_ctx_dst = 3; sj.L = L; sj.A = A; sj.E = E; sj.F = d->F; sj.K = d->K;
                rc = st_attn_step_fwd(&sj, B, stream);
            }
            break;
        case ATTN_PRE_FIN:
            if (!ST_SKIPPED(2)) {
                const st_attn_fin_job fj = fin_job(f.fin_parts);
                rc = st_attn_fin_fwd(io->pq_buf, &fj, B, stream);
            }
            break;
        case ATTN_FIN_SPLIT:
            if (!ST_SKIPPED(2)) {
                const st_attn_fin_job fj = fin_job(sp_parts);
                rc = st_attn_fin_split_fwd(io->pq_buf, &fj, io->attn_split_ws, B, stream);
            }
            break;
        case ATTN_PQ_FIN:       // 2 + 3 as one launch: the fin workgroups wait for pq inside the launch (granule hand-off)
            if (!(ST_SKIPPED(1) || ST_SKIPPED(2))) {
                const st_attn_fin_job fj = fin_job(f.fin_parts);
                rc = st_query_attn_fin_fwd(io->packed + pl.pq, &hq_dst, 16 * kb16(Q), io->pq_granules, (unsigned)(t + 1), &fj, B,
                                           f.prod == PROD_PQ_FIN ? &pj_d : nullptr, stream);
            }
            break;
        case ATTN_PQ_RNG:       // 2 + 3 + combine as one launch (long texts)
            if (!(ST_SKIPPED(1) || ST_SKIPPED(2))) {
                const st_attn_fin_job fj = fin_job(sp_parts);
                rc = st_query_attn_rng_fwd(io->packed + pl.pq, &hq_dst, 16 * kb16(Q), io->pq_granules, io->attn_xchg, (unsigned)(t + 1), &fj, B, stream);
            }
            break;
        }
        if (rc) return rc;

        // 4. decoder LSTM: h_d_t -> xd_{t+1}[h part], xo_t[h part]        ref: :275-280
        if (f.prod == PROD_OWN || (f.prod == PROD_PQ_PRE && t == 0)) {     // (no launch of this step hosts the product: one of its own, same arithmetic)
            rc = st_partial_product_fwd(&pj_d, B, stream);
            if (rc) return rc;
        }
        if (!ST_SKIPPED(3)) {
            const st_lstm_cell_packed_job jd = cell_d(t);
            if (f.pair_cells && t + 1 < steps) {
                // teacher forcing: the query cell of step t+1 needs ctx_t, h_q_t and a teacher frame -- not h_d_t.  Both cells in one launch.
                const st_lstm_cell_packed_job jq = cell_q(t + 1);
                rc = st_lstm_cell_packed_pair_fwd(&jd, &jq, stream);
            } else
                rc = st_lstm_cell_packed_fwd(&jd, stream);
            if (rc) return rc;
        }

        // 5. mel frames + stop logit (+ prenet layer 1 of the next input when fused)   ref: :282-287
        st_t16_view xo_v = {xo, sv.o_kbs, 0};
        st_t16_view mel_dst = {io->mel_t16, kb16(in_dim), 0};
        st_t16_view pre1_dst = {io->pre1_t16 + (size_t)t * io->pre1_step_floats, kb16(P), 0};
        const bool fuse = d->fuse_pre0 != 0;
        if (f.defer) continue;         // mel / stop of all steps come from one GEMM over the xo tape (caller)
        const bool split_attn = f.attn != ATTN_WHOLE;
        const st_attn_pre_job job = pre_job(t + 1, io->attn_pre_parts);
        if (!ST_SKIPPED(4)) {
            // mel (B, in_dim) natural (+ T16 for the prenet launches when they follow), the stop logit repeated per frame, and, fused, prenet
            // layer 1 of the next input as the third range
            st_packed_linear_job pg = st_plain_linear_job(io->packed + pl.pg, xo_v, ST_SKIPPED(7) ? Ko / 4 : Ko, io->mel_out + (size_t)t * in_dim,
                                                          (int)ldmel, B, in_dim + 1 + (fuse ? P : 0));
            pg.bias = w->projgate_b;
            if (!fuse) pg.y_dst = mel_dst;
            pg.n_split = in_dim; pg.y2 = io->stop_out + (size_t)t * d->r; pg.ldy2 = steps * d->r; pg.rep = d->r;
            pg.n_split2 = fuse ? in_dim + 1 : 0; pg.act2 = ST_ACT_RELU;
            pg.mask2 = io->prenet_mask ? io->prenet_mask + (size_t)t * 2 * B * P : nullptr; pg.ldmask2 = P;
            if (fuse) pg.y3_dst = pre1_dst;
            rc = st_skinny_linear_packed_attnpre_fwd(&pg, split_attn && t + 1 < steps && !ST_SKIPPED(6) ? &job : nullptr, stream);
            if (rc) return rc;
        }

        // 6. next decoder input -> xq_{t+1}[dec_in part]                 ref: :190-206
        if (t + 1 < steps) {
            const int src = io->step_src[t];
            st_t16_view next = {xq_next, sv.q_kbs, 0};
            if ((src == -1 || io->Bt < B) && !ST_SKIPPED(5)) {    // rows without a teacher feed their own output back
                rc = prenet_own(w, d, io, pl, sv, t, fuse, stream);
                if (rc) return rc;
            }
            // (pure teacher forcing: tiled for all steps before the loop)
            if (!f.pure_tf && src >= 0) rc = st_tile_rows(io->teacher_pre + (size_t)src * P, io->Tt * P, &next, io->Bt, P, stream);
            else if (!f.pure_tf && src == -2) rc = st_tile_rows(io->teacher_mean, P, &next, io->Bt, P, stream);
            if (rc) return rc;
        } else if (d->prenet_norm == 3 && (io->step_src[t] == -1 || io->Bt < B)) {
            // the reference forms the next input after the LAST step too (:192,:197-198,:205-206).  Nothing reads it, but a training-mode
            // BatchNorm1d moves its running statistics (and counts the batch) once more: same launches into slot `steps` of the tape
            rc = prenet_own(w, d, io, pl, sv, t, false, stream);
            if (rc) return rc;
        }
    }
    return 0;
}
