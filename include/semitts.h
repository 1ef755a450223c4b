/* semitts.h -- C ABI of libsemitts_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the Tacotron-style TTS decode hot path and the VQ codebook lookup of
 * ttaoREtw/semi-tts.  The reference has NO native/FFI layer (it is pure PyTorch, SURVEY.md
 * section 8b): each entry point below replaces the torch.nn / torch.nn.functional call(s)
 * of the reference cited next to it (`ref:` = path:line under the reference tree).  The
 * Python host (the .py files of semi_tts_amd/) binds these with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous row-major fp32 (or int64 where said);
 *    the caller (PyTorch) owns every buffer; the library allocates nothing persistent
 *    except graphs/streams explicitly created through st_graph_* / st_stream_*;
 *  - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and is
 *    hipGraph-capturable (no host sync, no malloc, no blocking memcpy inside);
 *  - return value 0 = success; negative = error, text via st_last_error() (thread-local);
 *  - "ld*" arguments are row strides in elements.
 */
#ifndef SEMITTS_H
#define SEMITTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 1

/* activation codes */
#define ST_ACT_NONE 0
#define ST_ACT_RELU 1
#define ST_ACT_TANH 2
#define ST_ACT_SIGMOID 3

const char* st_last_error(void);
int st_abi_version(void);
/* number of compute units / device name of the current device (diagnostics for bench.py) */
int st_device_info(int* n_cu, int* lds_bytes, char* name, int name_len);

/* ------------------------------------------------------------------ streams and graphs */
/* HIP stream + hipGraph plumbing so that a launch-bound sequence of st_* calls (the 86..355
 * step decode loop) is recorded once and replayed as ONE graph launch. */
int st_stream_create(void** stream_out);
int st_stream_destroy(void* stream);
int st_stream_sync(void* stream);
int st_graph_begin(void* stream);                       /* hipStreamBeginCapture            */
int st_graph_end(void* stream, void** graph_exec_out);  /* EndCapture + Instantiate         */
int st_graph_launch(void* graph_exec, void* stream);
int st_graph_destroy(void* graph_exec);
/* HIP-event timing on a given stream (bench.py measures kernels on the stream they run on) */
int st_event_create(void** ev_out);
int st_event_record(void* ev, void* stream);
int st_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* syncs on ev_stop */
int st_event_destroy(void* ev);

/* ------------------------------------------------------------------ skinny (small-batch) ops
 * Weight-streaming kernels for M = batch <= a few dozen rows: the weight matrix is the MFMA
 * A operand (16 rows per workgroup, K split over the waves of the workgroup), the batch is
 * the MFMA N dimension, so every weight byte is read from HBM exactly once per call.
 * The logical input is the concatenation of up to 3 segments x_s (B, k_s) with row stride
 * ldx_s, multiplied by W_s (N, k_s) with row stride ldw_s (slices of torch weights).
 */
typedef struct st_seg {
    const float* x; /* (B, k) activations                       */
    const float* w; /* (N, k) weight slice, torch [out][in]     */
    int ldx;
    int ldw;
    int k;
} st_seg;

/* One LSTMCell step, fused gate GEMM + pointwise (+ hidden-state dropout).
 * ref: nn.LSTMCell src/module.py:127-128,133-134 called :228,:277; nn.Dropout :230,:279;
 *      nn.LSTM time step src/module.py:458-460 (with `pre` = x W_ih^T + b_ih + b_hh).
 * gates(b, g*H+u) = sum_s x_s W_s^T + b_ih + b_hh + pre ; order (i,f,g,o)
 * c' = s(f) c + s(i) tanh(g);  h' = s(o) tanh(c');  h_out = h' * mask (mask already scaled by 1/(1-p))
 * b_ih, b_hh, pre, mask, gates_out may be NULL.  gates_out (B,4,H) receives the ACTIVATED
 * gates (i,f,g,o) for the backward pass.  c_prev/c_out and h_out are (B,H) with row strides
 * ldc / ldh (so they can point into a (B,T,H) sequence tensor). */
int st_lstm_cell_fwd(const st_seg* segs, int nseg, const float* b_ih, const float* b_hh,
                     const float* pre, int ldpre, const float* c_prev, int ldc_prev,
                     const float* mask, float* h_out, int ldh, float* c_out, int ldc,
                     float* gates_out, int B, int H, void* stream);

/* y(b, n) = act(sum_s x_s W_s^T + bias) * mask      (B small)
 * ref: Linear wrapper src/module.py:500-522 (prenet :337-339, query_layer :380,
 *      pseudo_latent_mean/std :268-269).
 * If n_split > 0 the output columns n >= n_split go to y2 instead, each value repeated
 * `rep` times: the proj (+) gate_layer pair of src/module.py:285-287 in one launch
 * (y = mel (B, r*n_mels), y2 = stop (B, r)). */
int st_skinny_linear_fwd(const st_seg* segs, int nseg, const float* bias, int act,
                         const float* mask, int ldmask, float* y, int ldy,
                         int n_split, float* y2, int ldy2, int rep,
                         int B, int N, void* stream);

/* ------------------------------------------------------------------ pre-packed operands (decode loop)
 * A global load whose lanes touch 16 different cache lines per quarter-wave (the natural MFMA
 * operand pattern over row-major data) sustains ~18 B/clk per CU on MI355X; 1 KiB-contiguous
 * wave loads sustain ~90-140 B/clk (tools/mb).  The decode loop therefore keeps its operands
 * in MFMA lane order in HBM:
 *   P16 (weights):      [row tile of 16][k block of 16][lane 0..63][4 floats]
 *   T16 (activations):  [batch tile of 16][k block of 16][lane 0..63][4 floats]
 *   element (r, k) of a block lives at lane 16*((k>>2)&3) + (r&15), component k&3.
 * Rows/columns beyond the logical shape are zero.  T16 destinations must be zero-filled by the
 * caller once (kernels only write logical elements). */
typedef struct st_t16_view {   /* a k-block range [kb0, kb0 + ceil(k/16)) of a T16 buffer */
    float* base;      /* start of the T16 buffer                                     */
    int kb_stride;    /* k-blocks per batch tile of the WHOLE buffer                 */
    int kb0;          /* first k-block of this view                                  */
} st_t16_view;
/* CONTRACT (finite neighbours): a product that takes more than one batch tile per workgroup (st_packed_fwd_variant: nb > 1)
 * reads its activation operand through ONE descriptor over all the batch tiles it spans.  When the reduced
 * range is not a multiple of the load group (16 k-blocks), the k-blocks that FOLLOW the view's range in every spanned batch tile but
 * the last are loaded too and multiplied with weight blocks that read as zero.  0 * finite adds exactly 0; 0 * Inf or 0 * NaN would
 * poison the sum.  So EVERY k-block of the batch tiles an operand spans -- the other views of the same T16 buffer, pad rows and pad
 * columns included -- must hold finite values: allocate T16 buffers zero-filled, never uninitialised. */
/* Several logical activations that one consumer multiplies with ONE packed weight matrix share one
 * T16 buffer (e.g. [dec_in | ctx | h_q] for the query LSTM): each producer writes its k-block range
 * of every consumer's buffer, so a consumer streams exactly one contiguous activation run. */

size_t st_packed_weight_floats(const int* k, int nseg, int N, int lstm_H); /* size of a P16 buffer */
size_t st_t16_floats(int B, int K);                                        /* size of a T16 buffer */
/* Pack up to 3 K-segments w[s] (N, k[s]) (row stride ldw[s], torch [out][in]) into one P16 buffer
 * whose K axis is the concatenation of the segments (each padded to a multiple of 16).
 * lstm_H > 0: N == 4*lstm_H and the 16 rows of tile t are the (i,f,g,o) rows of hidden units
 * 4t..4t+3 (so the cell update is workgroup-local). */
int st_pack_weight(const float* const* w, const int* ldw, const int* k, int nseg, int N, int lstm_H,
                   float* packed, void* stream);
/* ... for up to eight matrices in ONE launch (the six matrices of st_decoder_pack were six launches of ~10 us per forward / weight update) */
typedef struct st_pack_job { const float* w[3]; int ldw[3]; int k[3]; int nseg; int N; int lstm_H; float* packed; } st_pack_job;
int st_pack_weight_batch(const st_pack_job* jobs, int n, void* stream);
/* P16 image of the TRANSPOSE of the column concatenation [w[0] | w[1] | ...] (each (K, cols[s]), row stride ldw[s]): N = sum cols,
 * one segment of K columns -- what st_pack_weight would make of torch.cat(w, 1).t().contiguous(), without those two copies
 * (the BPTT loop's W^T operands: backward of nn.LSTMCell / Linear, src/module.py:247-283). */
int st_pack_weight_t(const float* const* w, const int* ldw, const int* cols, int nseg, int K, float* packed, void* stream);
int st_tile_rows(const float* src, int ld, const st_t16_view* dst, int B, int K, void* stream);   /* natural -> T16 */
int st_untile_rows(const st_t16_view* src, float* dst, int ld, int B, int K, void* stream);       /* T16 -> natural */
/* st_lstm_cell_fwd on packed operands: x = K logical columns starting at view x.  The new hidden
 * state goes to up to two T16 destinations; optionally also the AdaIN-adapted hidden state
 * hadapt = ada_std * (h_out - ada_mean)  (ada_* natural (B,H)).
 * ref: as st_lstm_cell_fwd, AdaIN src/module.py:268-269 */
typedef struct st_lstm_cell_packed_job {
    const float* packed_w; st_t16_view x; int K;
    const float* b_ih; const float* b_hh;
    const float* c_prev; int ldc_prev; const float* mask;
    st_t16_view h_dst0; st_t16_view h_dst1;      /* h_dst1.base may be NULL */
    float* c_out; int ldc; float* gates_out;
    const float* ada_std; const float* ada_mean; st_t16_view hadapt_dst;   /* hadapt_dst.base may be NULL */
    int B, H;
    const float* part; int w_kbs;   /* optional: K covers the LEADING k-blocks of a matrix packed with w_kbs k-blocks per row tile; the gate
                                     * products over the others arrive as the (B, 4 H) slab `part`, written by an st_partial_product_job of an
                                     * earlier launch, and are added to the reduced gates.  16 < B <= 32, H / 4 even.  NULL: the whole cell.
                                     * ref: nn.LSTMCell, src/module.py:275-280 */
} st_lstm_cell_packed_job;
int st_lstm_cell_packed_fwd(const st_lstm_cell_packed_job* job, void* stream);
/* Two independent cells in ONE launch: under teacher forcing the decoder cell of step t and the query cell of step t+1 both only wait
 * for the attention of step t (src/module.py:216-288 with a teacher frame as the next input).  Falls back to one launch per cell for
 * shapes the 2-D tiled kernel does not take. */
int st_lstm_cell_packed_pair_fwd(const st_lstm_cell_packed_job* j0, const st_lstm_cell_packed_job* j1, void* stream);
/* The operands of every packed weight-streaming product: y (B, N) = x W^T, x = K logical columns starting at view x (by value, as in
 * st_lstm_cell_packed_job), W a P16 buffer of N rows, y natural with row stride ldy >= N.  The K-split partial products
 * (st_skinny_partial_attn_*, st_partial_product_fwd) keep arguments of their own: their output is S slabs, not a (y, ldy) pair. */
typedef struct st_packed_product {
    const float* packed_w; st_t16_view x; int K;
    float* y; int ldy;
    int B, N;
} st_packed_product;
/* st_skinny_linear_fwd on packed operands; output natural (p.y) and/or T16 (y_dst).  A zero-initialised job with only `p` set is the
 * plain product y = x W^T. */
typedef struct st_packed_linear_job {
    st_packed_product p;                            /* p.y may be NULL when y_dst.base is given */
    const float* bias; int act; const float* mask; int ldmask;   /* v = act(x W^T + bias) * mask(b, n), as st_skinny_linear_fwd */
    st_t16_view y_dst;                              /* .base NULL = none (as h_dst1 of the cell job) */
    int n_split; float* y2; int ldy2; int rep;      /* n_split > 0: columns n >= n_split go to y2[b, (n - n_split) * rep + j], j < rep,
                                                     * instead (y = mel, y2 = stop.  ref: proj (+) gate_layer src/module.py:285-287) */
    /* optional third row range [n_split2, N), n_split2 >= n_split: v = act2(v) * mask2(b, n - n_split2) -> y3_dst column n - n_split2
     * (used to emit prenet layer 1 of the next step from the same launch as proj/gate) */
    int n_split2; int act2; const float* mask2; int ldmask2; st_t16_view y3_dst;
} st_packed_linear_job;
int st_skinny_linear_packed_fwd(const st_packed_linear_job* job, void* stream);

/* ------------------------------------------------------------------ location-sensitive attention
 * One decode step for the whole batch, one workgroup per utterance.
 * ref: Attention.energy/.forward src/module.py:371-407 and the state update :262-264,
 *      AdaIN :267-269 (std/mean hoisted out of the loop).
 *   loc   = W_loclin . conv1d(stack[w_prev, w_cum]; 2->F, k=K, pad (K-1)/2)      (L,A)
 *   e_l   = v . tanh(pq + loc_l + pm_l)
 *   w     = softmax_L(e)  (no mask)             -> w_out ; w_cum_out = w + w_cum_prev
 *   ctx   = sum_l w_l memory_l                  -> ctx (B,E)
 *   if h_q != NULL: h_adapt = ada_std * (h_q - ada_mean)                          (B,Q)
 * pq (B,A) = query_layer(h_q) is produced by st_skinny_linear_fwd. */
typedef struct st_attn_step_job {
    const float* pq; const float* pm; const float* memory;
    const float* w_prev; int ld_wprev; const float* w_cum_prev;
    float* w_out; int ld_wout; float* w_cum_out;
    const float* loc_conv_w; const float* loc_lin_w; const float* v;
    st_t16_view ctx_dst[3]; int n_ctx_dst;   /* the context goes to up to 3 T16 destinations (the decode loop) ... */
    float* ctx; int ld_ctx;                  /* ... and / or to a natural (B, E) one */
    const float* h_q; int ld_hq; const float* ada_std; const float* ada_mean; float* h_adapt; int Q;   /* optional AdaIN; not together
                                              * with T16 destinations (the decode loop fuses it into the query LSTM epilogue) */
    int L, A, E, F, K;
} st_attn_step_job;
int st_attn_step_fwd(const st_attn_step_job* job, int B, void* stream);
/* The same step in two launches.  `pre` only needs the PREVIOUS step's attention weights: location conv and
 * S(b,l,:) = pm(b,l,:) + W_l conv([w_prev; w_cum_prev])(l) -> s_buf (B,L,A); it can run while the rest of the decode step
 * does (st_skinny_linear_packed_attnpre_fwd runs it as extra workgroups of the proj launch).  `fin` = energies
 * v . tanh(pq + S), softmax, cumulative weights, context.  (pq + W_l cf) + pm becomes pq + (pm + W_l cf): fp32
 * re-association only.  Both take their job struct, declared below: st_attn_pre_job, st_attn_fin_job. */
/* st_skinny_linear_packed_fwd plus, as extra workgroups of the same launch (one per utterance), st_attn_pre_fwd for the NEXT
 * decode step: the proj (+) gate launch of step t leaves most compute units idle and the attention weights of step t are
 * already known, so S of step t+1 is ready when its attention launch starts. */
struct st_partial_product_job;
typedef struct st_attn_pre_job {
    const float* pm; const float* w_prev; int ld_wprev; const float* w_cum_prev;
    const float* loc_conv_w; const float* loc_lin_w; float* s_buf;
    int L, A, F, K;
    int parts;      /* workgroups per utterance (ranges of positions): a power of two from 2 to 64; any other value runs as 1 */
    float* cf_out;  /* optional (B, L, F): the location features of the step, kept for the backward pass */
    /* optional: a K-split partial product (st_partial_product_job, below) on the compute units the launch leaves idle -- teacher-forced
     * training hosts the tail of the decoder cell's gate reduction beside the query projection + attention pre part (B = 17..32; the
     * launch then has N / 16 x 2 + B x parts + job->N / 32 workgroups) */
    const struct st_partial_product_job* part;
} st_attn_pre_job;
int st_attn_pre_fwd(const st_attn_pre_job* job, int B, void* stream);   /* the pre part as a launch of its own: no cf_out, no part */
int st_skinny_linear_packed_attnpre_fwd(const st_packed_linear_job* job, const st_attn_pre_job* pre, void* stream);   /* pre NULL or without s_buf: the linear alone */
/* The launch(es) a forward product on packed operands takes, from shapes alone (touches no memory; the launchers decide through the
 * same code).  mode: ST_PK_MODE_CELL st_lstm_cell_packed_fwd (n = H), ST_PK_MODE_LINEAR st_skinny_linear_packed_fwd /
 * st_skinny_linear_packed_attnpre_fwd (n = N), ST_PK_MODE_CELL_PAIR st_lstm_cell_packed_pair_fwd (jobs (B, n = H) and (B1, n1 = H1)).
 * Linear only: pre_parts > 0 -- an attention-pre job with that many workgroups per utterance rides along (pre_A, pre_F its dims,
 * pre_aligned: pm, loc_lin_w and s_buf 16-byte aligned); part_n > 0 -- and a hosted partial product of part_n rows.
 * Fills out[0] (out[0..1] for a pair that falls back to one launch per cell) and returns the number of launches, or -1 for a refusal.
 *   family: the kernel; nb: batch tiles per workgroup; grid_x, grid_y: the grid (attention-pre forms: one-dimensional, the linear's
 *   workgroups, then B * pre_parts attention workgroups, then part_n / 32 of the partial product); vec: the attention-pre workgroups
 *   use 16-byte loads.
 * The linear picks the fewest batch tiles per workgroup (at most 4, and at most ceil(B / 16)) that keep the grid within 512. */
#define ST_PK_MODE_CELL 0
#define ST_PK_MODE_LINEAR 1
#define ST_PK_MODE_CELL_PAIR 2
#define ST_PK_KERNEL 0          /* pk_kernel<mode, nb>: one row tile x nb batch tiles per workgroup */
#define ST_PK_LSTM_RT2 1        /* pk_lstm_rt2_kernel<nb>: two row tiles x nb batch tiles */
#define ST_PK_LSTM_RT2_PAIR 2   /* pk_lstm_rt2_pair_kernel: two cells, nb = 1 */
#define ST_PK_ATTNPRE 3         /* pk_attnpre_kernel<nb, vec> */
#define ST_PK_ATTNPRE_PART 4    /* pk_attnpre_part_kernel<1, vec> */
typedef struct st_packed_fwd_query { int mode; int B, n; int B1, n1; int pre_parts, pre_A, pre_F, pre_aligned; int part_n; } st_packed_fwd_query;
typedef struct st_packed_fwd_launch { int family, nb, grid_x, grid_y, vec; } st_packed_fwd_launch;
int st_packed_fwd_variant(const st_packed_fwd_query* q, st_packed_fwd_launch* out);

/* st_skinny_linear_packed_fwd (no bias / activation, natural y) whose output columns [n0, n0 + H) are dh of an LSTM cell: the pointwise
 * half of that cell's backward step (st_lstm_cell_bwd_pointwise with dh0 = those columns of y) runs in the EPILOGUE of the product
 * instead of as a launch of its own.  The BPTT of the decode loop uses it twice per step: dgates_d(t) . [W_ih_d | W_hh_d] makes
 * dh_d(t-1) in its last D columns, and W_q^T dpq(t) makes the attention's share of dh_q(t).  Every row stride a multiple of 4, every
 * base 16-byte aligned, n0 a multiple of 16.  ref: backward of nn.LSTMCell src/module.py:228,:277 */
typedef struct st_lstm_pw_job {
    int n0, H;
    const float* dh1; int ld1;                        /* optional addend (B rows) */
    const float* dh2; int ld2; const float* scale2;   /* optional addend * scale2 (B, H) */
    const float* mask;                                /* optional (B, H) */
    const float* gates;                               /* (B, 4, H) activated (i, f, g, o) */
    const float* c; int ldc; const float* c_prev; int ldcp;
    float* dc;                                        /* (B, H) in: dL/dc_t, out: dL/dc_{t-1} */
    float* dgates; int ldg;                           /* (B, 4H) out */
    st_t16_view dgates_t16;                           /* optional second copy in T16 (K = 4H) */
    int dh1_slabs; long dh1_slab_stride;              /* > 1: dh1 is the first of that many slabs (dh1_slab_stride floats apart) of a K-split
                                                       * product (st_skinny_partial_attn_*): the addend is their sum, in slab order */
} st_lstm_pw_job;
int st_skinny_linear_packed_lstm_bwd_fwd(const st_packed_product* p, const st_lstm_pw_job* job, void* stream);

/* The fin part for LONG texts: every utterance split over `parts` (2..64) ranges of positions -- local softmax statistics and an
 * un-normalised partial context per range (flash-decoding style), then a combine launch.  S and the memory rows are read once in
 * total; st_attn_fin_fwd re-reads S in each of its context slices and one compute unit has to pull ~2 L A 4 bytes (12 us at
 * L = 171).  Same arithmetic as softmax(e) @ memory up to fp32 rounding (~1e-7).  workspace: B * parts * (4 + E) floats.
 * (st_attn_fin_split_fwd, declared with the fin job below: job->parts = 2..64; F, K and status are unused there) */
size_t st_attn_fin_split_workspace_floats(int B, int E, int parts);
/* Query projection + attention fin part in ONE launch: pq = W_q h_q (ref: src/module.py:380) is computed by the first workgroups
 * and handed to the fin workgroups of the same launch (st_attn_fin_fwd's work: :389-406, :262-264) as 8-byte
 * {value, tag} words in `granules` ((B, A) 64-bit words, device memory, ZEROED by the caller before the first step of a
 * forward); `epoch` = decode step + 1 (never 0) is the tag this launch writes and waits for.  The fin workgroups request S, v
 * and the memory rows while pq is being computed: one kernel boundary and one exposed load round trip less per decode step.
 * Needs A % 16 == 0, A <= 256 and (A / 16) * ceil(B / 16) + B * parts workgroups resident at once (<= compute units); when that
 * does not hold the call fails and the caller uses st_skinny_linear_packed_fwd + st_attn_fin_fwd. */
typedef struct st_attn_fin_job {
    const float* s_buf; const float* memory; const float* w_cum_prev;
    float* w_out; int ld_wout; float* w_cum_out; const float* v;
    st_t16_view ctx_dst[3]; int n_ctx_dst;
    int parts;          /* workgroups per utterance: each takes E / parts context dims and repeats the energies + softmax; 1, 2, 4 or 8
                         * with E % (4 * parts) == 0 */
    int L, A, E, F, K;
    unsigned* status;   /* optional device word: bit 0 is set when a fin workgroup gave up waiting for its granules (the query is
                         * then poisoned with NaN as well); never cleared by the library -- the caller zeroes and reads it */
    float* ctx; int ld_ctx;   /* optional natural (B, E) context output, beside or instead of the T16 destinations */
} st_attn_fin_job;
int st_attn_fin_fwd(const float* pq, const st_attn_fin_job* job, int B, void* stream);   /* the fin part as a launch of its own, pq (B, A) */
int st_attn_fin_split_fwd(const float* pq, const st_attn_fin_job* job, float* workspace, int B, void* stream);
/* The launch a forward attention call takes, from shapes and operand alignment alone (touches no memory; the launchers decide through
 * the same code).  part: 0 st_attn_step_fwd, 1 st_attn_pre_fwd, 2 st_attn_fin_fwd, 3 st_attn_fin_split_fwd.  parts: the job's `parts`
 * (ignored by part 0).  aligned: ST_ATTN_AL_* bits of the operands that are 16-byte aligned (set the bits of operands the part does
 * not take).  Returns 0 and fills *out, or a refusal (out then holds what was decided before it):
 *   vec: the 16-byte-load kernel (at_kernel<true, part>), else the scalar one;  wl_vec: W_l is fetched with 16-byte loads;
 *   s_mfma: the pre part forms S on the matrix cores;  kp32: the conv reads 32-tap filter rows (K <= 32), else the generic loop;
 *   lds_bytes: dynamic LDS of a workgroup;  opt_in: the launch raises the kernel's dynamic-LDS limit first (> 64 KiB);
 *   workgroups: of the launch (part 3: of the range launch; the combine launch adds B);
 *   parts, Lp: part 1 -- position ranges per utterance as run (a power of two from 2 to 64, anything else 1) and positions per range
 *   (a multiple of 12); part 2 -- context slices, L; part 3 -- ranges that hold positions (trailing empty ones are dropped), ceil(L / parts);
 *   L_64k, L_160k: parts 0..2, the last L whose image stays within 64 KiB (no opt-in) and within 160 KiB (not refused) at these dims. */
#define ST_ATTN_AL_PM 1
#define ST_ATTN_AL_PQ 2
#define ST_ATTN_AL_V 4
#define ST_ATTN_AL_WL 8
#define ST_ATTN_AL_MEM 16
#define ST_ATTN_AL_S 32
#define ST_ATTN_AL_WS 64           /* the workspace of part 3 */
#define ST_ATTN_R_DIMS (-1)        /* a dimension <= 0, or no such part */
#define ST_ATTN_R_K_EVEN (-2)      /* the location kernel size must be odd */
#define ST_ATTN_R_E (-3)           /* E must be a multiple of 4, at most 2048 */
#define ST_ATTN_R_ALIGN (-4)       /* memory (always), pm / pq / v / S (A % 4 == 0), every operand of part 3 */
#define ST_ATTN_R_LDS (-5)         /* the image exceeds 160 KiB */
#define ST_ATTN_R_PARTS (-6)       /* part 2: 1, 2, 4 or 8 with E % (4 parts) == 0; part 3: 2..64 */
#define ST_ATTN_R_RANGE_DIMS (-7)  /* part 3: A a multiple of 4 in 4..256, E / 4 a divisor of 512 */
#define ST_ATTN_R_LP (-8)          /* part 3: more than 512 positions per range */
typedef struct st_attn_fwd_query { int part; int B, L, A, E, F, K; int parts; unsigned aligned; } st_attn_fwd_query;
typedef struct st_attn_fwd_plan { int vec, wl_vec, s_mfma, kp32; long lds_bytes; int opt_in, workgroups, parts, Lp, L_64k, L_160k; } st_attn_fwd_plan;
int st_attn_fwd_variant(const st_attn_fwd_query* q, st_attn_fwd_plan* out);
/* A partial product part (B, N) = x[:, kb0 .. kb0 + KB) W[:, kb0 .. kb0 + KB)^T over a k-block range of a P16 matrix (w_kbs k-blocks per row
 * tile; LSTM row order when the matrix is a cell's) and of a T16 activation buffer (x.kb0 = the range's first k-block in it): two row tiles
 * and both batch tiles per workgroup (16 < B <= 32, N % 32 == 0), N / 32 workgroups. */
typedef struct st_partial_product_job {
    const float* packed_w; int w_kbs; int kb0; int KB;
    st_t16_view x;
    int N;
    float* part;
} st_partial_product_job;
/* The query projection + fin launch; `part` (may be NULL) is such a job beside it in the same launch (every workgroup on a compute unit of
 * its own: (A / 16) ceil(B / 16) + B * parts + N / 32 <= compute units).  The decode step's use: the part of nn.LSTMCell's gate product
 * (ref: src/module.py:275-280) whose operands do not depend on the attention of the step runs WHILE the attention runs. */
int st_query_attn_fin_fwd(const float* packed_wq, const st_t16_view* h_q, int Q, unsigned long long* granules, unsigned epoch,
                          const st_attn_fin_job* job, int B, const st_partial_product_job* part, void* stream);
/* ... and the job as a launch of its own: what the decode loop issues in its two-launch pq / fin form (a starved hand-off degrades to it),
 * so that both forms compute the same arithmetic bit for bit */
int st_partial_product_fwd(const st_partial_product_job* job, int B, void* stream);
/* Long texts (the fin part is bound by what ONE compute unit pulls in: S and the memory rows of an utterance): the same launch with the
 * fin part over `job->parts` (2..8) POSITION ranges per utterance -- local softmax statistics and an un-normalised partial context per
 * range, as st_attn_fin_split_fwd -- and the combine INSIDE the launch: the ranges of an utterance exchange (max, sum, partial context)
 * as 8-byte {value, tag} granules through `xchg` (st_attn_rng_xchg_words(B, E, parts) 64-bit words, zero before the first epoch of a
 * forward) and each finishes E / parts context dims and the weights of its own positions.  One launch instead of three.
 * Needs E % (4 * parts) == 0, E / parts <= 256 and every workgroup resident at once: st_query_attn_rng_fits(B, A, parts) != 0
 * (occupancy query of the kernel x compute units); otherwise use the two / three launch forms.  No natural output: job->ctx must be NULL. */
int st_query_attn_rng_fits(int B, int A, int parts);
size_t st_attn_rng_xchg_words(int B, int E, int parts);
int st_query_attn_rng_fwd(const float* packed_wq, const st_t16_view* h_q, int Q, unsigned long long* granules,
                          unsigned long long* xchg, unsigned epoch, const st_attn_fin_job* job, int B, void* stream);
/* Diagnostics: one wave runs the consumer side of that hand-off on `granules` (A 64-bit {value, tag} words) as they are and writes
 * the A values to `out` -- or NaN, with bit 0 of *status set, after `max_spins` polls without every tag == epoch (the failure
 * path of a starved launch, which the scheduler never produces on an idle device). */
int st_handoff_wait_selftest(const unsigned long long* granules, unsigned epoch, int A, unsigned* status, float* out,
                             int max_spins, void* stream);

/* ------------------------------------------------------------------ dense GEMM / conv1d (many rows)
 * C(m, coff + n) = epilogue( sum_tap sum_ci A(row(m) * stride + tap - pad, ci) * W(n, ci, tap) )
 * channels-last activations: A is (Bn * Tin, Cin) with row stride lda, C is (Bn * Tout, N)
 * with row stride ldc; rows of one utterance never read across its [0,Tin) range (zero pad).
 * W is the torch Conv1d weight (N, Cin, KT) or, with KT == 1, the torch Linear weight (N, Cin).
 * epilogue: v += bias[n]; v = act_pre(v); if bn_mean: v = (v - bn_mean[n]) / sqrt(bn_var[n] + eps)
 *           * bn_w[n] + bn_b[n]; v = act_post(v); if highway_h: v = highway_h(m,n) * v +
 *           res(m,n) * (1 - v) else if res: v += res(m,n); if mask: v *= mask(m,n)
 * pool_prev != 0: A(row, ci) is replaced by max(A(row, ci), A(row - 1, ci)) (row-1 inside the
 * utterance), i.e. MaxPool1d(2, stride 1, padding 1)[:T] fused into the load.
 * ref: Conv1d+BatchNorm1d+ReLU src/module.py:421-431; BatchNormConv1d :527-538; CBHG bank /
 *      maxpool / projections / pre_highway / Highway :597-611, :541-555; nn.Linear src/tts.py:34;
 *      memory_layer src/module.py:306; prenet over the whole teacher :178-179; the strided / residual
 *      ConvLayer of the speech encoder src/module.py:627-648. */
typedef struct st_gemm_epilogue {
    const float* bias;
    int act_pre;
    const float* bn_mean; const float* bn_var; const float* bn_w; const float* bn_b; float bn_eps;
    int act_post;
    const float* res; int ldres;
    const float* highway_h; int ldhw;
    const float* mask; int ldmask;
    int w_tap_major;   /* KT > 1 only: W is given as (N, KT, Cin) -- taps outermost, so a k-block of weights is contiguous (16-byte
                        * loads) -- instead of the torch Conv1d layout (N, Cin, KT) */
    float* splitk_ws;  /* optional workspace of splitk_slabs * (Bn * Tout) * N floats: the reduction is split over splitk_slabs =
                        * st_gemm_splitk_slabs(...) (> 1) groups of workgroups whose partial products a finish pass adds in a
                        * fixed order before the epilogue (small grids with long reductions: the encoder convs) */
    int splitk_slabs;
} st_gemm_epilogue;
int st_gemm_splitk_slabs(int Bn, int Tout, int Cin, int N, int KT);   /* 1 = no split */

int st_gemm_fwd(const float* A, int lda, const float* W, float* C, int ldc, int coff,
                int Bn, int Tin, int Tout, int Cin, int N, int KT, int pad, int stride, int pool_prev,
                const st_gemm_epilogue* ep, void* stream);

/* Several independent st_gemm_fwd jobs in one launch: the K convolutions of the CBHG conv bank read the same input
 * (`[conv1d(x)[:, :, :T] for conv1d in self.conv1d_banks]`, src/module.py:590-598).  Each job holds the arguments of st_gemm_fwd
 * (the epilogue by value).  Jobs the pipelined kernel takes without pooling or split-K share launches (8 jobs each, longest
 * reduction first); otherwise the jobs run one after the other -- the results are those of n st_gemm_fwd calls either way. */
typedef struct st_gemm_job {
    const float* A; int lda; const float* W; float* C; int ldc; int coff;
    int Bn, Tin, Tout, Cin, N, KT, pad, stride, pool_prev;
    st_gemm_epilogue ep;
} st_gemm_job;
int st_gemm_fwd_batch(const st_gemm_job* jobs, int n, void* stream);
/* What st_gemm_fwd / st_gemm_fwd_batch would launch for these arguments (host only: pointers are looked at for their alignment, never
 * read; negative on bad arguments).  st_gemm_fwd_variant = kernel | slabs << 8 | finish << 16 with
 *   kernel: 0-2 the LDS-DMA kernel with 64x64 / 32x64 / 64x32 tiles; 3 + 4 VW + 2 PL + (MT == 1): the pipelined kernel (VW: 16-byte
 *           weight pieces, PL: fused max-pool, MT == 1: 32-row tiles); 11 / 12: its element-wise form for rows that are not 16-byte
 *           addressable (weights adjacent in ci / torch Conv1d layout); 13 / 14: the one-block kernel with / without 16-byte weights;
 *   slabs:  split-K slab count (1 = none);  finish: 0 none, 1 four columns per thread (compile-time slab count), 2 the same with a
 *           run-time count, 3 one column per thread (N % 4 != 0).
 * st_gemm_fwd_batch_variant = OR of: 1 separate st_gemm_fwd calls, 2 / 4 batched LDS-DMA launches with 64x32 / 64x64 tiles,
 * 8 batched pipelined launches. */
int st_gemm_fwd_variant(const float* A, int lda, const float* W, const float* C, int ldc, int coff,
                        int Bn, int Tin, int Tout, int Cin, int N, int KT, int pad, int stride, int pool_prev,
                        const st_gemm_epilogue* ep);
int st_gemm_fwd_batch_variant(const st_gemm_job* jobs, int n);

/* The highway stack of the CBHG in one launch (eval mode): n_layers times y = relu(W_H x + b_H) * T + x * (1 - T), T = sigmoid(W_T x + b_T),
 * x (M, C) rows; w_h / w_t: n_layers pointers to torch Linear weights (C, C), b_h / b_t: their biases (NULL entries = no bias).
 * Bit-identical to 2 n_layers st_gemm_fwd launches with the highway epilogue.  st_highway_stack_supported: C % 16 == 0, C <= 80, <= 8 layers.
 * ref: Highway.forward src/module.py:541-555, CBHG.forward :609-611. */
int st_highway_stack_supported(int C, int n_layers);
int st_highway_stack_fwd(const float* x, int ldx, const float* const* w_h, const float* const* b_h, const float* const* w_t,
                         const float* const* b_t, int n_layers, float* y, int ldy, int M, int C, void* stream);

/* per-column statistics over M rows (training-mode BatchNorm): mean, biased variance, and
 * the running-stat update  run = (1-mom) run + mom * {mean, unbiased var}; batches_tracked (optional, one int64 on the device:
 * nn.BatchNorm1d.num_batches_tracked) is incremented by the same launch.
 * ref: nn.BatchNorm1d in training mode, src/module.py:429,:531 */
int st_bn_stats(const float* X, int ldx, int coff, int M, int N, float* mean_out, float* var_out,
                float* run_mean, float* run_var, float momentum, long long* batches_tracked, float* ws, void* stream);
/* nn.LayerNorm over the last dimension of (M, N) rows: y = (x - mean) / sqrt(var + eps) * gamma + beta (biased variance, two passes
 * as ATen); mean_out / rstd_out (M) optional, kept for the backward.  ref: the speech encoder's `layer_norm` src/asr.py:38-39,58; the
 * normalised prenet Linear src/module.py:508-521 */
int st_layer_norm_fwd(const float* x, int ldx, const float* gamma, const float* beta, float eps, float* y, int ldy,
                      float* mean_out, float* rstd_out, int M, int N, void* stream);
/* dx of the above; dyxhat (optional, (M, N) contiguous) = dy * xhat, whose column sum is d gamma (d beta = column sum of dy) */
int st_layer_norm_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* mean,
                      const float* rstd, float* dx, int lddx, float* dyxhat, int M, int N, void* stream);
/* log_softmax over the last dimension of (M, N) contiguous rows and its backward dx = dy - exp(y) * sum_n dy.
 * ref: ASRPostnet.forward src/asr.py:80 */
int st_log_softmax_fwd(const float* x, float* y, int M, int N, void* stream);
int st_log_softmax_bwd(const float* dy, const float* y, float* dx, int M, int N, void* stream);
/* One normalised prenet layer of a decode step after its Linear (the reference's Linear wrapper with norm_type, applied to the
 * (B, P) rows of ONE step: src/module.py:192,:508-521,:337-339): dst (T16) = relu(norm(y)) * mask.
 * mode 1: LayerNorm over the P columns; mode 2: BatchNorm1d with running statistics (eval); mode 3: BatchNorm1d with the
 * statistics of the step's rows, running statistics updated in place (momentum, unbiased variance), batches_tracked += 1.
 * Rows b0 .. B-1 are normalised and written (y, mask and dst are indexed by the absolute row): with a partial teacher the
 * reference's prenet sees the rows WITHOUT a teacher only (src/module.py:197-198,205-206), which is the batch of its BatchNorm1d. */
int st_prenet_norm_fwd(const float* y, int ldy, int mode, const float* gamma, const float* beta, float* run_mean,
                       float* run_var, long long* batches_tracked, float eps, float momentum, const float* mask, int ldmask,
                       const st_t16_view* dst, int b0, int B, int P, void* stream);
/* Backward of that layer, in place: dn (rows, P) = gradient at the norm's output (ReLU / mask backward applied) -> gradient at the
 * Linear's output y (rows, P); this step's sums are ADDED to dgamma / dbeta (P).  Statistics are recomputed from y (mode 2: the
 * running ones).  What torch autograd derives for nn.LayerNorm / nn.BatchNorm1d on a (rows, P) input. */
int st_prenet_norm_bwd(float* dn, int ld, const float* y, int ldy, int mode, const float* gamma, const float* run_mean,
                       const float* run_var, float eps, float* dgamma, float* dbeta, int rows, int P, void* stream);
/* X(m, coff+n) = act((X - mean) / sqrt(var + eps) * w + b), in place */
int st_bn_apply(float* X, int ldx, int coff, int M, int N, const float* mean, const float* var,
                const float* w, const float* b, float eps, int act, void* stream);

/* out-of-place variant of st_bn_apply (training keeps the pre-normalisation tensor for the backward) */
int st_bn_norm_fwd(const float* X, int ldx, int xoff, float* Y, int ldy, int yoff, int M, int N,
                   const float* mean, const float* var, const float* w, const float* b, float eps, int act,
                   void* stream);

/* ------------------------------------------------------------------ backward building blocks (training, H1)
 * Input gradient of st_gemm_fwd = st_gemm_fwd itself on dC with the weight transposed and tap-flipped
 * (W'(ci, n, t) = W(n, ci, KT-1-t), pad' = KT-1-pad, Tin/Tout swapped).
 * ref: what torch autograd derives for nn.Conv1d / nn.Linear / nn.BatchNorm1d / activations used at
 * src/module.py:421-431,:527-538,:541-555,:597-611 and src/tts.py:34. */
/* dW(n, ci, tap) (+)= sum_rows dC(row, dcoff+n) * A(row + tap - pad, ci)   [torch weight layout (N, Cin, KT)]
 * ws: st_gemm_wgrad_workspace_floats() floats of scratch (row-split partial slabs, added in fixed order) */
size_t st_gemm_wgrad_workspace_floats(int Bn, int Tout, int Cin, int N, int KT);
int st_gemm_wgrad(const float* dC, int lddc, int dcoff, const float* A, int lda, float* dW, float* ws,
                  int Bn, int Tin, int Tout, int Cin, int N, int KT, int pad, int pool_prev, int accumulate, void* stream);
/* st_gemm_wgrad + the bias gradient db[n] = sum over all (Bn * Tout) rows of dC[:, dcoff + n] in the same launches (no st_colsum
 * next to the product): backward of nn.Linear / nn.Conv1d with bias. */
int st_gemm_wgrad_db(const float* dC, int lddc, int dcoff, const float* A, int lda, float* dW, float* db, float* ws,
                     int Bn, int Tin, int Tout, int Cin, int N, int KT, int pad, int pool_prev, int accumulate, void* stream);
/* out(n) (+)= sum_m X(m, xoff+n) [* Y(m, yoff+n)]      (bias gradients, AdaIN statistics gradients) */
int st_colsum(const float* X, int ldx, int xoff, const float* Y, int ldy, int yoff, int M, int N,
              float* out, int accumulate, float* ws, void* stream);
/* scratch of the row-split column reductions st_bn_stats(_record) / st_colsum / st_bn_bwd_reduce: <= 128 chunk partials + the result, (2, N) each */
size_t st_colreduce_workspace_floats(int M, int N);
/* dpre = dout * mask * act'(out)   (out = the activated forward value; mask may be NULL) */
int st_act_bwd(const float* dout, int ldd, const float* out, int ldo, int act, const float* mask, int ldm,
               float* dpre, int ldp, int M, int N, void* stream);
/* BatchNorm backward with batch statistics, y = act((x - mean)/sqrt(var+eps)*w + b), in two halves so that a data-parallel caller can
 * all-reduce the two sums in between (SyncBN):
 *   reduce: s[0:N] = sum_rows dyb (= d bias), s[N:2N] = sum_rows dyb * xhat (= d weight) over the M local rows, dyb = dy [* mask] * act'(y);
 *           ws: st_colreduce_workspace_floats(M, N) floats.
 *   apply:  dx = w/sigma * (dyb - s1/Mstat - xhat * s2/Mstat) [, dres = dy * mask].  Mstat = the rows behind mean / var / s; under SyncBN
 *           the caller all-reduces s across ranks between the calls and passes inv_total (mean / var are then the global batch's too).
 * Both halves read the same job.  Both refuse (-22, before any launch) a NULL job, NULL dy / x / mean / var / s, M <= 0, N <= 0, and
 * act != ST_ACT_NONE with NULL y; reduce also NULL ws; apply also NULL dx, and Mstat < M without inv_total. */
typedef struct st_bn_bwd_job {
    const float* dy;   int ldd;        /* (M, N) rows; a column slice comes as pointer + stride */
    const float* y;    int ldy;        /* act(BN(x)) kept by the forward; NULL iff act == ST_ACT_NONE */
    int act;
    const float* x;    int ldx;
    const float* mean; const float* var; const float* w;   /* w NULL = 1 */
    float eps;
    int M, N;
    const float* mask; int ldm;        /* NULL, or dy is multiplied by it on the way in */
    float* s;                          /* (2N): reduce writes (sum dyb, sum dyb*xhat); apply reads them */
    int Mstat;                         /* apply: rows behind mean/var/s; ignored when inv_total is given */
    const float* inv_total;            /* apply: NULL, or device scalar 1/(global rows) of st_bn_sync_merge */
    float* dx;   int lddx;             /* apply: out */
    float* dres; int lddr;             /* apply: NULL, or out = dy * mask (gradient of the residual input) */
} st_bn_bwd_job;
int st_bn_bwd_reduce(const st_bn_bwd_job* job, float* ws, void* stream);
int st_bn_bwd_apply(const st_bn_bwd_job* job, void* stream);
/* ConvLayer's tail in training (ref: src/module.py:641-646: BatchNorm -> activation -> (+ x) -> dropout) as ONE launch behind the conv:
 * Tact (M, N) = act(BatchNorm(X)) with the given batch statistics, kept for the backward (NULL: not written), Y (M, N) = (Tact + res) * mask
 * (res, mask: NULL = absent).  Contiguous rows of N floats, N % 4 == 0, 16-byte aligned.  Replaces nn.BatchNorm1d + torch.tanh + `+` +
 * nn.Dropout of the reference (one launch instead of BatchNorm apply, add, bernoulli_, div_, mul). */
int st_bn_norm_res_mask_fwd(const float* X, float* Tact, float* Y, int M, int N, const float* mean, const float* var,
                            const float* w, const float* b, float eps, int act, const float* res, const float* mask, void* stream);
/* The backward of that tail is st_bn_bwd_reduce / st_bn_bwd_apply with the job's `mask` (dy is multiplied by it on the way in, no launch
 * of its own), `y` = the kept Tact, and `dres` (the gradient of the residual input; NULL: no residual). */
/* SyncBN (the data-parallel form of the BatchNorm1d layers above; the reference trains on one device, ref: src/module.py:434-455,
 * so this is the path's own multi-GPU extension) with the row counts kept on the device:
 *   st_bn_stats_record   rec (2N + 1) = (mean[N], M2[N], row count) of this rank's rows -- what the ranks all-gather;
 *   st_bn_sync_merge     the gathered records (world, 2N + 1) -> mean / biased variance of the global batch, merged in rank order
 *                        (identical on every rank), running statistics updated with the unbiased variance over the global count,
 *                        *inv_total_out = 1 / (global row count);
 *   st_bn_bwd_apply      with the job's inv_total: s summed over all ranks and divided by the global count read from *inv_total. */
int st_bn_stats_record(const float* X, int ldx, int coff, int M, int N, float* rec, long long* batches_tracked, float* ws, void* stream);
int st_bn_sync_merge(const float* rec, int world, int N, float* mean_out, float* var_out, float* run_mean, float* run_var,
                     float momentum, float* inv_total_out, void* stream);
/* Highway combine y = H*T + x*(1-T) and its backward dH = dy*T, dT = dy*(H-x), dx_direct = dy*(1-T)
 * ref: src/module.py:551-554 */
int st_highway_fwd(const float* H, const float* Tgate, const float* x, float* y, size_t total, void* stream);
/* One Highway layer on the PRE-activations of its two Linear layers side by side, ht (M, 2C) = [W_H x + b_H | W_T x + b_T] (one
 * N = 2C product instead of two): y = relu(h) * sigmoid(t) + x * (1 - sigmoid(t)) (src/module.py:551-554), and its backward:
 * dht (M, 2C) = gradients at the two pre-activations (the operand of ONE input-gradient product and ONE weight-gradient product),
 * dx_direct (M, C) = dy * (1 - T). */
/* The K BatchNorm1d layers of a conv bank (K independent layers of equal width N over K tensors of (Bn, T_k, N) rows, src/module.py:590-598)
 * as one launch per phase.  Segment k: x (Bn * T_k rows, stride ldx), statistics over ALL its rows (the reference normalises the T + 1
 * positions of an even-k conv before trimming to T); the normalised rows t < Tout go to columns [k N, (k + 1) N) of Y (Bn * Tout rows, stride
 * ldy) -- the concatenated bank, no torch.cat.  Backward: dY (same geometry) -> dx_k over all rows of each segment (rows t >= Tout see
 * dy = 0), optionally through the ReLU in FRONT of the norm (relu_in: x_k = relu(conv), so the factor is x > 0), and (s1, s2) = (d bias, d weight).
 * Both entries read one st_bn_bank_job and run the stages in `stages`: forward ST_BN_STATS | ST_BN_NORM (rec == NULL: 3 launches); under SyncBN
 * ST_BN_STATS with rec (this rank's (mean, M2, row count) per segment -> rec (nseg, 2N + 1), the batch counted; mean / var not needed) ->
 * [all-gather] -> ST_BN_MERGE (allrec (world, nseg, 2N + 1) -> global mean / var, running statistics, inv_total[k] = 1 / global rows) -> ST_BN_NORM.
 * Backward ST_BN_REDUCE | ST_BN_APPLY; under SyncBN ST_BN_REDUCE (local sums -> segs[k].sums) -> [all-reduce] -> ST_BN_APPLY (sums = the global ones).
 * Other `stages`, or a stage without what it reads or writes: -22 before any launch.  ws: st_bn_bank_workspace_floats(nseg, max rows, N). */
#define ST_BN_BANK_MAX 16
typedef struct st_bn_bank_seg {
    const float* x; int ldx; int T;                /* rows b * T + t, b < Bn */
    const float* w; const float* b;                /* weight, bias (N) or NULL */
    float* run_mean; float* run_var; long long* batches_tracked; float momentum, eps;   /* updated in place by the forward (NULL = none) */
    float* mean; float* var;                       /* (N) out of STATS / MERGE, in of NORM and the backward */
    float* dx; int lddx;                           /* APPLY: out, Bn * T rows */
    float* sums;                                   /* REDUCE: out (2, N) = (sum dy, sum dy xhat) = (d bias, d weight); APPLY: in */
} st_bn_bank_seg;
typedef struct st_bn_bank_job {
    const st_bn_bank_seg* segs; int nseg; int Bn, N;
    float* Y; const float* dY; int ld; int Tout;   /* the concatenated bank (forward out / backward in), its row stride, frames kept */
    int relu_in;                                   /* APPLY: dx through the ReLU in front of the norm */
    float* rec; const float* allrec; int world;    /* SyncBN: this rank's records out; the gathered records in */
    float* inv_total; float* ws;                   /* inv_total (nseg): written by MERGE, read by APPLY; NULL = local row counts */
} st_bn_bank_job;
enum { ST_BN_STATS = 1, ST_BN_MERGE = 2, ST_BN_NORM = 4, ST_BN_REDUCE = 1, ST_BN_APPLY = 2 };   /* stages of _fwd; of _bwd */
size_t st_bn_bank_workspace_floats(int nseg, int max_rows, int N);
int st_bn_bank_fwd(const st_bn_bank_job* job, int stages, void* stream);
int st_bn_bank_bwd(const st_bn_bank_job* job, int stages, void* stream);
int st_highway_ht_fwd(const float* ht, const float* x, float* y, int M, int C, void* stream);
int st_highway_ht_bwd(const float* dy, const float* ht, const float* x, float* dht, float* dx_direct, int M, int C, void* stream);
int st_highway_bwd(const float* dy, const float* H, const float* x, const float* Tgate,
                   float* dH, float* dT, float* dx_direct, size_t total, void* stream);
/* y(b,t,:) = max(x(b,t-1,:), x(b,t,:)), y(b,0,:) = x(b,0,:): nn.MaxPool1d(2, stride=1, padding=1)(x)[:, :, :T] of the CBHG,
 * src/module.py:600, on contiguous channels-last (Bn, T, C) tensors, C % 4 == 0 (the input of the LDS-DMA conv kernel; the
 * register-staged kernel fuses the same maximum into its loads: pool_prev of st_gemm_fwd) */
int st_pool_prev_fwd(const float* x, float* y, int Bn, int T, int C, void* stream);
/* backward of the fused MaxPool1d(2,1,1)[:T]: dx(b,t,c) from the gradient w.r.t. the pooled tensor */
int st_pool_prev_bwd(const float* dy_pooled, const float* x, float* dx, int Bn, int T, int C, void* stream);
/* dst(b,t,:) (+)= src(b,t,:) with arbitrary (b,t) strides (elements) */
int st_copy3d(float* dst, long dst_sb, long dst_st, const float* src, long src_sb, long src_st,
              int Bn, int T, int C, int accumulate, void* stream);
/* dtable(v, :) += sum of dout(r, :) over the rows with idx(r) == v, in row order (deterministic, no atomics)
 * ref: backward of F.embedding src/embed.py:97-101 */
int st_scatter_add_rows(const float* dout, const int64_t* idx, float* dtable, int n, int D, int V, void* stream);

/* ------------------------------------------------------------------ recurrent sequence layers */
/* One nn.LSTM layer (ndir = 1, or 2 for bidirectional=True) over a full sequence, lengths ignored, zero initial state.
 * xproj[d] (B,T,4H) = x W_ih[d]^T + b_ih[d] (from st_gemm_fwd; b_hh is added in the cell), out(b, t, ocol[d] : ocol[d]+H) = h_t of
 * direction d.  Of two directions, 0 walks t = s and 1 walks t = T-1-s; one direction walks backward with `reverse`.  Training:
 * gates_tape[d] (T,B,4,H) receives the activated gates and c_tape[d] (T,B,H) every cell state (both indexed by time step).
 * The backward takes dout(b, t, dcol[d] : dcol[d]+H) to dxproj[d] (B,T,4H) (= gradient of the input projection incl. both biases); the
 * caller finishes with dW_hh = st_gemm_wgrad(dxproj, out shifted by one step) and db = st_colsum(dxproj).
 * st_lstm_seq_variant is the one place a form is chosen (host arithmetic only; -1: null pointer, or a shape no form takes):
 *   ST_LSTM_STEP     one launch per time step (backward: a pointwise and a W_hh^T launch, w = W_hh^T (H,4H): ST_LSTM_W_T).
 *                    ws_floats: forward (2 ndir + 1) B H, backward 2 ndir B H.
 *   ST_LSTM_PACKED   backward, ndir == 2, H % 16 == 0, ld and col multiples of 4 and every ST_LSTM_AL_* operand 16-byte aligned (else
 *                    ST_LSTM_STEP): one launch per time step, dgates(s) . W_hh with the pointwise backward of step s-1
 *                    in its epilogue; w = st_pack_weight_t of W_hh (N = H, K = 4H): ST_LSTM_W_PACKED_T.  ws_floats: 2 B H +
 *                    4 st_t16_floats(B, 4H), ws 16-byte aligned.
 *   ST_LSTM_PERSIST  ndir == 2: ALL time steps in ONE launch, its workgroups resident at once on cus - cu_reserve compute units (cus == 0:
 *                    this device's).  The plain (4H,H) weights (ST_LSTM_W_NATURAL) and the cell states / dL/dc stay in registers; the
 *                    hand-over between steps is polled straight out of out / dxproj, which the entry first fills with a sentinel (every
 *                    word is written exactly once: the data is the flag).  Forward: H = 64, 128, 256 or 512, B <= 64, disjoint output
 *                    columns.  Backward: H = 32, 64, 128 or 256.  ld and col multiples of 4, every ST_LSTM_AL_* operand of the pass 16-byte
 *                    aligned, allow_persist != 0.  *status (optional device word): bit 1 set when a wait timed out -- the launch was
 *                    starved of compute units, the affected rows are NaN.  The plan names the launch: grid, block, rt row tiles, nkb
 *                    k-blocks per wave, rg batch rows per workgroup (backward), xcd_map (forward); 0 for the other forms.
 * The run entry points plan from the job itself and refuse one whose `weights` is not the plan's or whose ws is NULL while ws_floats > 0.
 * ref: nn.LSTM src/module.py:432-438,:458-460 and its backward */
#define ST_LSTM_STEP 0
#define ST_LSTM_PACKED 1
#define ST_LSTM_PERSIST 2
#define ST_LSTM_W_NATURAL 0
#define ST_LSTM_W_T 1
#define ST_LSTM_W_PACKED_T 2
#define ST_LSTM_AL_OUT 1           /* forward: out, and w_hh[d] (<< d) */
#define ST_LSTM_AL_W0 2
#define ST_LSTM_AL_DOUT 1          /* backward: dout, and gates_tape[d], c_tape[d], dxproj[d] (<< d) */
#define ST_LSTM_AL_GATES0 2
#define ST_LSTM_AL_C0 8
#define ST_LSTM_AL_DX0 32
typedef struct st_lstm_seq_job {
    int ndir, reverse;                /* ndir 1 or 2; reverse only with ndir == 1 */
    const float *xproj[2], *w_hh[2], *b_hh[2];
    float* out; int ldo; int ocol[2];
    float *gates_tape[2], *c_tape[2]; /* NULL in inference */
    int B, T, H;
    float* ws;                        /* plan.ws_floats floats */
    unsigned* status;                 /* one-launch form only */
    int allow_persist, cu_reserve;
} st_lstm_seq_job;
typedef struct st_lstm_seq_bwd_job {
    int ndir, reverse;
    const float* dout; int ldd; int dcol[2];
    const float *gates_tape[2], *c_tape[2];
    const float* w[2];                /* in the layout plan.weights names */
    int weights;                      /* ST_LSTM_W_*: what w[] holds */
    float* dxproj[2];
    int B, T, H;
    float* ws; unsigned* status; int allow_persist, cu_reserve;
} st_lstm_seq_bwd_job;
/* ld, col: ldo, ocol (forward) or ldd, dcol (backward) */
typedef struct st_lstm_seq_query { int backward, ndir, B, T, H, ld, col[2]; unsigned aligned; int allow_persist, cus, cu_reserve; } st_lstm_seq_query;
typedef struct st_lstm_seq_plan { int form, weights; size_t ws_floats; int grid_x, grid_y, grid_z, block, rt, nkb, rg, xcd_map; } st_lstm_seq_plan;
int st_lstm_seq_variant(const st_lstm_seq_query* q, st_lstm_seq_plan* out);
int st_lstm_seq_fwd(const st_lstm_seq_job* j, void* stream);
int st_lstm_seq_bwd(const st_lstm_seq_bwd_job* j, void* stream);
/* Pointwise half of one LSTM cell backward step (shared by the encoder BiLSTM and the decoder's two cells):
 * dh = (dh0 + dh1 + dh2 * scale2) * mask;  from dh and the carried dc (B,H, updated in place to dL/dc_{t-1})
 * to dgates (B,4H) w.r.t. the pre-activation gates in torch order (i,f,g,o).  dh1, dh2, scale2, mask, c_prev
 * may be NULL; dgates_t16 (optional): a second copy of dgates in the T16 tile layout (K = 4H), the operand of
 * st_skinny_linear_packed_fwd over the packed W^T.  ref: backward of nn.LSTMCell src/module.py:228,:277 */
int st_lstm_cell_bwd_pointwise(const float* dh0, int ld0, const float* dh1, int ld1, const float* dh2, int ld2,
                               const float* scale2, const float* mask, const float* gates, const float* c, int ldc,
                               const float* c_prev, int ldcp, float* dc, float* dgates, int ldg,
                               const st_t16_view* dgates_t16, int B, int H, void* stream);
/* Two LSTM cells / two plain linears of the same shape in ONE launch (the two directions of a bidirectional layer at their own time
 * steps): arrays of two, one segment each */
int st_lstm_cell_pair_fwd(const st_seg* segs2, const float* const* b_hh2, const float* const* pre2, int ldpre,
                          const float* const* c_prev2, int ldc_prev, float* const* h_out2, int ldh,
                          float* const* c_out2, int ldc, float* const* gates_out2, int B, int H, void* stream);
int st_skinny_linear_pair_fwd(const st_seg* segs2, float* const* y2, int ldy, int B, int N, void* stream);
/* nn.GRU, ndir directions in one launch (direction 1 runs time-reversed), one workgroup per
 * (utterance, direction) keeps W_hh rows in registers and h in LDS for all T steps.
 * gi[d] (B,T,3H) = x W_ih[d]^T + b_ih[d] (from st_gemm_fwd); out(b, t, d*H : (d+1)*H) = h_t.
 * Training: tape (ndir,B,T,4,H) receives (r, z, n, W_hn h + b_hn) per step; NULL in inference.
 * ref: nn.GRU src/module.py:585-586,:617 */
int st_gru_seq_fwd(const float* gi_fwd, const float* gi_bwd, const float* w_hh_fwd, const float* w_hh_bwd,
                   const float* b_hh_fwd, const float* b_hh_bwd, float* out, int ldo, float* tape,
                   int B, int T, int H, int ndir, void* stream);
/* Backward through time of st_gru_seq_fwd, again one workgroup per (utterance, direction) with W_hh^T columns
 * in registers: dout (B,T,>=ndir*H) -> dgi[d] (B,T,3H) (gradient of gi) and dgh[d] (B,T,3H) (gradient of
 * W_hh h + b_hh).  The caller finishes with dW_hh = st_gemm_wgrad(dgh, out shifted by one step), db_hh = colsum. */
int st_gru_seq_bwd(const float* dout, int ldd, const float* out, int ldo, const float* tape,
                   const float* w_hh_fwd, const float* w_hh_bwd, float* dgi_fwd, float* dgi_bwd,
                   float* dgh_fwd, float* dgh_bwd, int B, int T, int H, int ndir, void* stream);
/* The kernel st_gru_seq_fwd (backward = 0) or st_gru_seq_bwd (backward = 1) launches for hidden size H, from H alone: ST_GRU_TRI
 * (H <= 84: three lanes per hidden unit split the reduction), ST_GRU_QUAD (forward, H <= 128: one lane per gate row, four lanes per unit),
 * ST_GRU_REG32 (backward, H <= 128: W_hh columns in registers, padded to 128), ST_GRU_GENERAL (H <= 341: W_hh read from memory each
 * step) -- or -1: no kernel takes H (H < 1, or 3H > 1024), and both calls refuse it. */
#define ST_GRU_TRI 0
#define ST_GRU_QUAD 1
#define ST_GRU_REG32 2
#define ST_GRU_GENERAL 3
int st_gru_seq_variant(int H, int backward);

/* ------------------------------------------------------------------ VQ codebook */
/* table(v, :) = cat[learnable(v, 0:Dl), attr(v,:) W_attr^T + b_attr]      (V, Dl + Da)
 * ref: L2Embedding.embedding / forward src/embed.py:87-94,109-112 */
int st_vq_build_table(const float* learnable, int Dl, const float* attr, int n_attr,
                      const float* attr_w, const float* attr_b, int Da, float* table, int V, void* stream);
/* out(n, :) = table(idx(n), :)   ref: F.embedding src/embed.py:97-101,:134,:181-183 */
int st_gather_rows(const float* table, const int64_t* idx, float* out, int n, int D, int V, void* stream);
/* Nearest-code search.  x (n, D), table (V, D):
 *   sim = relu(temp) * -(|x|^2 + |e|^2 - 2 x.e) ; p = softmax_V(sim) ; idx = argmax_V(p)
 *   (first maximum wins) ; out = (x + table[idx]) - x   (straight-through forward value)
 * ref: L2Embedding.forward src/embed.py:105-147, neg_batch_l2 :208-213 */
int st_vq_l2_fwd(const float* x, const float* table, const float* temp, float* p_code,
                 int64_t* idx, float* out, float* workspace, int n, int D, int V, void* stream);
/* The same search with the table's MFMA-order copy made ONCE per table version instead of on every call (the table only changes
 * with the weights): st_vq_pack_table fills `packed` (st_vq_l2_workspace_floats(D, V) floats; D <= 64, D % 4 == 0, V <= 1024),
 * st_vq_l2_packed_fwd searches with it.  Same results as st_vq_l2_fwd bit for bit. */
int st_vq_pack_table(const float* table, float* packed, int D, int V, void* stream);
int st_vq_l2_packed_fwd(const float* x, const float* table, const float* packed, const float* temp, float* p_code,
                        int64_t* idx, float* out, int n, int D, int V, void* stream);
/* workspace: st_vq_l2_workspace_floats(D, V) floats (the table re-packed into MFMA operand order + |e|^2 per code) selects the
 * matrix-core kernel (D <= 64, D % 4 == 0, V <= 1024; exact-fp32 MFMA keeps the dimension-ascending dot product, so the indices
 * are those of the scalar kernel); NULL or another shape runs the scalar kernel (table staged in LDS). */
size_t st_vq_l2_workspace_floats(int D, int V);
/* Backward pieces of the codebook lookup (what autograd derives for src/embed.py:105-147 and :187-205):
 *   st_softmax_bwd:       dz(n, v) = s * p(n, v) * (dp(n, v) - sum_v' dp(n, v') p(n, v')),  s = scale * (relu_scale ? max(relu_scale[0], 0) : 1);
 *                         rowsum (optional) = sum_v dz(n, v)
 *   st_rowscale_combine:  out(m, d) = alpha * a(m, d) + beta * r(m) * x(m, d) + c(m, d)   (x/r and c optional) -- with a = dz E or
 *                         dz^T X from the GEMM entry points this forms dX = 2 (dz E) - 2 X rowsum + dnew_latent and
 *                         dE = 2 (dz^T X) - 2 E colsum + scatter_add(dnew_latent) of sim = -relu(temp) (|x|^2 + |e|^2 - 2 x.e). */
int st_softmax_bwd(const float* p, const float* dp, const float* relu_scale, float scale, float* dz, float* rowsum,
                   int n, int V, void* stream);
int st_rowscale_combine(const float* a, float alpha, const float* x, const float* r, float beta, const float* c,
                        float* out, int M, int D, void* stream);
/* Run-length merge of VQ codes with blank filtering (ref: VQVAE.mean_forward src/vqvae.py:218-257): per utterance,
 * consecutive frames with the same argmax code (runs capped at max_frames_per_phn+1 frames) are replaced by the
 * mean of their latents, runs of code 0 are dropped.  out (B, T, D) must be ZERO on entry (rows >= lens(b) stay
 * zero = the reference's pad_sequence); lens (B) int32 = kept segments per utterance (0 = all-blank utterance:
 * the reference returns None for the batch); frame_seg (B,T) int32 / frame_w (B,T) = segment of every frame
 * (-1 = dropped) and 1/len, the saved tensors of st_vq_mean_bwd. */
int st_vq_mean_fwd(const float* p_code, const float* latent, float* out, int* lens, int* frame_seg, float* frame_w,
                   int B, int T, int D, int V, int max_frames_per_phn, void* stream);
/* dlatent(b,t,:) = dout(b, seg(t), :) / len(seg(t)); dout is (B, n_seg_rows, D) */
int st_vq_mean_bwd(const float* dout, int n_seg_rows, const int* frame_seg, const float* frame_w, float* dlatent,
                   int B, int T, int D, void* stream);
/* softmax + argmax over rows of logits (n, V) -> p (n, V), idx (n)
 * ref: SeperateEmbedding.forward src/embed.py:190-193 */
int st_softmax_argmax(const float* logits, float* p, int64_t* idx, int n, int V, void* stream);

/* ------------------------------------------------------------------ the decode loop
 * Decoder.forward's `for t in range(decode_steps)` (src/module.py:184-206) issued natively:
 * per step  query LSTM -> query projection -> attention (+AdaIN) -> decoder LSTM -> proj/gate
 * [-> prenet of the own output when the next input is not a teacher frame].
 * All per-step state lives in caller-owned "tapes" indexed by step (slot 0 = initial zeros),
 * which double as the saved tensors of the backward pass.
 */
typedef struct st_decoder_weights {
    const float* prenet_w0;      /* decoder.prenet.layers.0.linear.weight (P, r*n_mels)   */
    const float* prenet_w1;      /* decoder.prenet.layers.1.linear.weight (P, P)          */
    const float* q_w_ih;         /* decoder.query_rnn.weight_ih (4Q, P+E)                  */
    const float* q_w_hh;         /* decoder.query_rnn.weight_hh (4Q, Q)                    */
    const float* q_b_ih; const float* q_b_hh;
    const float* attn_query_w;   /* decoder.attn.query_layer.linear.weight (A, Q)          */
    const float* attn_v;         /* decoder.attn.v.linear.weight (1, A)                    */
    const float* attn_loc_conv_w;/* decoder.attn.loc_conv.conv.weight (F, 2, K)            */
    const float* attn_loc_lin_w; /* decoder.attn.loc_linear.linear.weight (A, F)           */
    const float* d_w_ih;         /* decoder.dec_rnn.weight_ih (4D, E+Q)                    */
    const float* d_w_hh;         /* decoder.dec_rnn.weight_hh (4D, D)                      */
    const float* d_b_ih; const float* d_b_hh;
    const float* projgate_w;     /* cat[proj.linear.weight; gate_layer.linear.weight] (r*n_mels+1, D+E) */
    const float* projgate_b;     /* cat[proj.linear.bias; gate_layer.linear.bias]                      */
    /* normalised prenet (st_decoder_dims.prenet_norm != 0; the reference's Linear wrapper with norm_type, src/module.py:508-521):
     * per layer the norm's weight / bias and, for BatchNorm1d, its running statistics and batch counter */
    const float* pre_norm_w[2]; const float* pre_norm_b[2];
    float* pre_norm_rm[2]; float* pre_norm_rv[2]; long long* pre_norm_nbt[2];
    float pre_norm_eps, pre_norm_momentum;
} st_decoder_weights;

typedef struct st_decoder_dims {
    int B, L, E, n_mels, r, P, Q, D, A, F, K;
    /* fuse_pre0 != 0 (free-running inference only: every next input is prenet(own output)):
     * projgate_w/_b carry P extra rows  W_pre0 . W_proj  /  W_pre0 . b_proj, so the proj/gate launch
     * also emits relu(prenet layer 1) of the next step (same function, re-associated in fp32). */
    int fuse_pre0;
    /* 0: plain prenet.  1 LayerNorm / 2 BatchNorm1d (eval) / 3 BatchNorm1d (training: statistics of a step's B rows) between
     * each prenet Linear and its ReLU (st_prenet_norm_fwd): the own-output prenet of the loop then runs as Linear, norm launch,
     * Linear, norm launch; fuse_pre0 must be 0 and st_decoder_io.pre_nat given */
    int prenet_norm;
} st_decoder_dims;

typedef struct st_decoder_io {
    const float* memory;      /* (B, L, E)  encoder output                                  */
    const float* pm;          /* (B, L, A)  memory_layer(memory)        src/module.py:306   */
    const float* ada_std;     /* (B, Q) relu(pseudo_latent_std(spkr))   src/module.py:268   */
    const float* ada_mean;    /* (B, Q) pseudo_latent_mean(spkr)        src/module.py:269   */
    /* next-input policy, decided by the host exactly as src/module.py:190-206:
     * step_src[t] (HOST array, `steps` entries) tells where dec_in of step t+1 comes from:
     *   -1 = prenet(own output) for every row; -2 = teacher mean (rows < Bt) ; >= 0 = teacher
     *   frame index `take_frame` (rows < Bt); rows >= Bt always use prenet(own output).   */
    const int* step_src;
    const float* teacher_pre; /* (Bt, Tt, P) prenet(teacher) or NULL     src/module.py:178-179 */
    const float* teacher_mean;/* (Bt, P) teacher_pre.mean(1) or NULL     src/module.py:194   */
    int Bt, Tt;
    const float* prenet_mask; /* (steps, 2, B, P) scaled masks for prenet(own output) after step t, or NULL */
    const float* q_mask;      /* (steps, B, Q) scaled hidden-state dropout masks or NULL   */
    const float* d_mask;      /* (steps, B, D) */
    int steps;
    /* outputs */
    float* mel_out;           /* (B, steps*r, n_mels) */
    float* align_out;         /* (B, steps, L)        */
    float* stop_out;          /* (B, steps*r)         */
    /* packed weights: st_decoder_packed_floats() floats, filled by st_decoder_pack() */
    const float* packed;
    /* tapes.  The step inputs live in three T16 buffers per step, handed in ZERO-FILLED:
     *   xq_tape: steps+1 slots of T16 (B, P+E+Q)  slot t = [dec_in_t | ctx_{t-1} | h_q_{t-1}]
     *   xd_tape: steps+1 slots of T16 (B, E+Q+D)  slot t = [ctx_t | adapted h_q_t | h_d_{t-1}]
     *   xo_tape: steps   slots of T16 (B, D+E)    slot t = [h_d_t | ctx_t]
     * (each logical piece padded to a multiple of 16 columns; slot size = st_t16_floats(B, padded sum)).
     * cq/cd/wcum are natural (steps+1, B, dim); slot 0 = initial zero state. */
    float* xq_tape; float* xd_tape; float* xo_tape;
    float* cq_tape; float* cd_tape; float* wcum_tape;
    float* pq_buf;            /* (B, A) scratch, natural */
    float* pre1_t16;          /* T16 (B,P) scratch (prenet layer-1 output), zero-filled */
    float* mel_t16;           /* T16 (B, r*n_mels) scratch (own output as the prenet input), zero-filled */
    float* zero_row;          /* (B, max(L,1)) zeros (w_prev of step 0) -- zeroed by the callee */
    float* gates_q_tape;      /* (steps, B, 4, Q) or NULL (training) */
    float* gates_d_tape;      /* (steps, B, 4, D) or NULL */
    float* attn_s_buf;        /* (B,L,A) or NULL: split the attention step -- its location conv + W_l part for step t+1 runs inside
                               * the proj (+) gate launch of step t (st_skinny_linear_packed_attnpre_fwd), the attention launch
                               * itself starts from S (free-running fused-prenet inference) */
    int attn_pre_parts;       /* workgroups per utterance of the pre part (a power of two up to 64; anything else runs as 1) */
    int attn_fin_parts;       /* workgroups per utterance of the fin part (0/1, 2, 4, 8; E % (4*parts) == 0) */
    int defer_proj;           /* pure teacher forcing only: skip the per-step proj (+) gate launch; the caller computes mel /
                               * stop for all steps with one GEMM over xo_tape afterwards (mel_out / stop_out untouched) */
    int pre1_step_floats;     /* > 0: pre1_t16 is a tape of `steps` slots of that many floats (training keeps the prenet
                               * layer-1 output of every own-output feedback for the backward); 0: one scratch slot */
    int attn_s_step_floats;   /* > 0: attn_s_buf is a tape, slot t = S of step t (B*L*A floats apart), kept for the backward */
    float* attn_loc_tape;     /* optional (steps, B, L, F): location features of every step (slot 0, which no step writes, is zeroed by the callee) */
    float* attn_split_ws;     /* optional, st_attn_fin_split_workspace_floats(B, E, attn_split_parts) floats: long texts run the fin part
                               * split over attn_split_parts position ranges + a combine launch (st_attn_fin_split_fwd) */
    int attn_split_parts;
    unsigned long long* pq_granules;   /* optional (B, A) 64-bit words: with attn_s_buf, the query projection and the attention fin
                                        * part of a step run as ONE launch (st_query_attn_fin_fwd); zeroed by the callee per forward */
    const float* dec_in0;              /* optional (B, P) natural: the input of step 0 = prenet(go frame).  NULL = zeros, which is what a
                                        * plain prenet makes of the all-zero go frame (src/module.py:161,183); a normalised prenet does not */
    float* pre_nat;                    /* (B, P) scratch, natural layout: the Linear output of a normalised prenet layer (prenet_norm != 0) */
    unsigned long long* attn_xchg;     /* optional, st_attn_rng_xchg_words(B, E, attn_split_parts) 64-bit words: with pq_granules and
                                        * attn_split_parts in 2..8, long texts run query projection + fin part over position ranges +
                                        * combine as ONE launch per step (st_query_attn_rng_fwd) when it fits the device; zeroed by the
                                        * callee per forward */
    unsigned* handoff_status;          /* optional device word for pq_granules: bit 0 = an in-launch hand-off timed out (a starved launch:
                                        * the waiting workgroups were not co-resident with their producers).  Sticky; owned, zeroed and
                                        * read by the caller after the forward -- a time-out is an ERROR, not a NaN to find later */
    int pair_cells;                    /* != 0 (with defer_proj, i.e. pure teacher forcing): the decoder cell of step t and the query cell of
                                        * step t+1 share one launch (st_lstm_cell_packed_pair_fwd) -- neither needs the other's output */
    float* pre_nat_tape;               /* optional (steps, 2, B, P): with prenet_norm, the Linear outputs of both prenet layers of every
                                        * own-output feedback are kept here (instead of pre_nat) for the backward */
    float* gate_part;                  /* optional (B, 4 D) scratch: in the one-launch pq + fin form (pq_granules) with 16 < B <= 32 the decoder
                                        * cell's gate products over operands that are known BEFORE the attention runs -- the tail of the cell's
                                        * reduction [ctx | AdaIN(h_q(t)) | h_d(t-1)] from column gate_part_k on -- ride beside the pq / fin launch
                                        * on compute units it leaves idle (st_query_attn_fin_fwd with `part`); the cell launch then reduces the first
                                        * gate_part_k columns and adds this slab (st_lstm_cell_packed_job.part).  fp32 re-association only.
                                        * NULL = off */
    int gate_part_k;                   /* the cell's own share of the reduction: a multiple of 16 in [kb16(E) * 16, K_d); 0 = the callee's rule
                                        * (st_decoder_gate_split_k: half of the reduction in whole rounds of 16 k-blocks -- C2: 1280 of 2560,
                                        * measured best of 512 ... 2048) */
} st_decoder_io;

/* the default of st_decoder_io.gate_part_k for these dimensions */
int st_decoder_gate_split_k(const st_decoder_dims* d);
size_t st_decoder_packed_floats(const st_decoder_dims* d);
/* floats of ONE slot of xq_tape (which = 0), xd_tape (1), xo_tape (2) */
size_t st_decoder_tape_floats(const st_decoder_dims* d, int which);
/* pack the six matrices the loop streams every step (once per forward / per weight update) */
int st_decoder_pack(const st_decoder_weights* w, const st_decoder_dims* d, float* packed, void* stream);
int st_decoder_forward(const st_decoder_weights* w, const st_decoder_dims* d, const st_decoder_io* io,
                       void* stream);
/* which forms st_decoder_forward will take for these dimensions and buffers, on a device with `cus` compute units that holds
 * `rng_capacity` workgroups of the one-launch range form at once (<= 0: this device's, which is what st_decoder_forward uses).  Host
 * arithmetic only.  Bits 0..2 the attention step (with the query projection): 0 whole step in one launch, 1 pre part elsewhere + fin
 * launch, 2 fin over position ranges + combine launch, 3 pq + fin as one launch, 4 pq + fin over position ranges + combine as one
 * launch; bits 4..5 where the decoder cell's partial gate product (gate_part) runs: 0 nowhere, 1 a launch of its own, 2 beside pq + fin,
 * 3 beside pq + attention pre (step 0: its own launch); bit 8 pure teacher forcing, bit 9 deferred projection, bit 10 the attention pre
 * part inside the pq launch, bit 11 paired cells; bits 12..15 the fin part's workgroups per utterance; bits 16..27 the k-blocks the
 * cell keeps with a partial product (0 without one).  -1 for a null pointer. */
int st_decoder_fwd_forms(const st_decoder_dims* d, const st_decoder_io* io, int cus, int rng_capacity);

/* ------------------------------------------------------------------ decoder backward (training, teacher forcing)
 * ref: what torch autograd derives for Decoder.forward / decode_one_step, src/module.py:184-288 */
/* Backward of one attention step: the one description of it, taken by the stand-alone launch below and by the launches that host the step
 * beside a product of the BPTT loop (st_skinny_linear_packed_lstm_bwd_attn_bwd, st_skinny_partial_attn_bwd; backward of
 * src/module.py:247-283).  The location features and tanh are recomputed from the saved weights, or S = pm + W_l loc of the step is given
 * (s_in, (B,L,A), e.g. kept by the forward): then loc_t is not written and may be NULL.
 * dctx / dw_direct: up to three addends each (row strides ld_*; a NULL addend is absent); dcum (B,L) carries dL/dcum_t across steps
 * (+ dcum_add).  Outputs needed by the recurrence: dpq (B,A) -- with dpq_t16.base also as a second copy in the T16 tile layout (K = A),
 * the operand of the packed W_q^T product that follows -- and dhist (B,2,L) = gradient w.r.t. [w_{t-1}; cum_{t-1}] through the location
 * conv.  Everything that is a sum over steps is left to the caller: the kernel writes this step's slices ds_t (B,L,A), loc_t / dloc_t
 * (B,L,F), hist_t (B,L,2) channels-last, dctx_t (B,E), dv_t (B,A), from which dpm = sum_t ds, dW_l = ds^T loc, dW_c = conv weight
 * gradient of (dloc, hist), dmem[b] = w^T dctx, dv = sum dv_t. */
typedef struct st_attn_bwd_job {
    const float* pq; const float* pm; const float* memory;
    const float* w_prev; int ld_wprev; const float* w_cum_prev; const float* w; int ld_w;
    const float* loc_conv_w; const float* loc_lin_w; const float* v;
    const float* dctx[3]; int ld_dctx[3]; int n_dctx;
    const float* dw_direct[3]; int ld_dw[3]; int n_dw;
    float* dcum; const float* dcum_add; int ld_dcum_add;
    float* dpq; st_t16_view dpq_t16; float* dhist; float* ds_t; float* loc_t; float* dloc_t; float* hist_t;
    float* dctx_t; float* dv_t; const float* s_in;
    int B, L, A, E, F, K;
    /* parts > 1 (2 or 4; 0 / 1 = the whole step in one workgroup per utterance): `parts` workgroups per utterance, each taking A / parts
     * attention dims of the energy gradient; ds_t / dpq / dv_t / dctx_t are complete afterwards, the location-feature gradient only as
     * `parts` partial sums in dloc_part (parts, B, L, F).  dhist / dloc_t / hist_t are NOT written and dcum is read-only (it must hold
     * the total gradient w.r.t. cum_t; dcum_add must be NULL): the caller runs st_attn_hist_job next, which forms them. */
    int parts; float* dloc_part;
    /* up to three more addends of the context gradient, behind dctx[0 .. n_dctx): the slabs of a K-split product (the gradient w.r.t.
     * ctx_{t} inside dxq_{t+1} when that launch ran in the partial form) */
    const float* dctx_more[3]; int ld_dctx_more[3]; int n_dctx_more;
} st_attn_bwd_job;
/* one attention-step backward, one workgroup per utterance (the whole step); job->s_in NULL: S is recomputed and loc_t written;
 * job->dpq_t16.base NULL: no T16 copy of dpq; job->parts must be 0 or 1 (the split forms exist only hosted) */
int st_attn_step_bwd(const st_attn_bwd_job* job, void* stream);

/* dmem(b,l,:) = sum_t align(b,t,l) * dctx_tape(t,b,:)   (gradient of the encoder memory through the contexts) */
int st_attn_dmem(const float* align, const float* dctx_tape, float* dmem, int B, int steps, int L, int E, void* stream);

typedef struct st_decoder_bwd_weights {   /* transposed copies prepared by the caller (layout only) */
    const float* q_w_cat_t;        /* [W_ih_q | W_hh_q]^T   (P+E+Q, 4Q)   (may be NULL when the packed form below is given) */
    const float* d_w_cat_t;        /* [W_ih_d | W_hh_d]^T   (E+Q+D, 4D)   (likewise) */
    const float* attn_query_w_t;   /* W_q^T                 (Q, A)        (may be NULL when the loop runs with fuse_pw) */
    const float* q_w_cat_t_p16;    /* optional: q_w_cat_t packed by st_pack_weight (N = P+E+Q, K = 4Q); NULL = natural kernels */
    const float* d_w_cat_t_p16;    /* optional: d_w_cat_t packed (N = E+Q+D, K = 4D) */
    const float* attn_query_w_t_p16;   /* optional: W_q^T packed (N = Q, K = A): with the two above and st_decoder_bwd_io.fuse_pw the loop runs
                                        * the cells' pointwise backward in the epilogues of its products (4 launches per step instead of 6) */
    const float* attn_v; const float* attn_loc_conv_w; const float* attn_loc_lin_w;
} st_decoder_bwd_weights;

/* All step-indexed tensors are natural row-major with Bp >= B rows per step slot (Bp = B rounded up to 16,
 * the row count of the un-tiled forward tapes; rows >= B are zero). */
typedef struct st_decoder_bwd_io {
    const float* memory; const float* pm; const float* ada_std;   /* (B,L,E) (B,L,A) (B,Q) */
    const float* align;            /* (B, steps, L) forward output            */
    const float* wcum_tape;        /* (steps+1, B, L)                         */
    const float* cq_tape; const float* cd_tape;             /* (steps+1, B, Q / D) */
    const float* gates_q_tape; const float* gates_d_tape;   /* (steps, B, 4, Q / D) activated gates */
    const float* q_mask; const float* d_mask;               /* (steps, B, Q / D) or NULL */
    const float* pq_all;           /* (steps, Bp, A)  = W_q h_q_t, recomputed by the caller */
    int steps; int Bp;
    const float* dxo;              /* (steps, Bp, D+E) = [dmel_t | dstop_t] [W_proj ; W_gate] */
    const float* dalign;           /* (B, steps, L) or NULL */
    float* dgq; float* dgd;        /* (steps, Bp, 4Q / 4D) out: pre-activation gate gradients */
    float* dxq; float* dxd;        /* (steps+1, Bp, P+E+Q / E+Q+D) out; slot `steps` must be zero */
    float* dpq;                    /* (steps, Bp, A) out */
    float* ds_tape; float* loc_tape; float* dloc_tape;   /* (steps, B, L, A / F / F) out, see st_attn_step_bwd */
    float* hist_tape; float* dctx_tape; float* dv_tape;  /* (steps, B, L, 2), (steps, B, E), (steps, B, A) out */
    float* dcq; float* dcd;        /* (B,Q) (B,D) scratch, zero on entry */
    float* dhist[2];               /* (B,2,L) x 2 scratch, zero on entry */
    float* dcum;                   /* (B,L) scratch, zero on entry */
    float* dhq_attn;               /* (B,Q) scratch */
    float* dgq_t16; float* dgd_t16;   /* st_t16_floats(B, 4Q / 4D) scratch, ZERO on entry; needed with the packed weights */
    /* own-output feedback (scheduled sampling: step_src[t] == -1 for all rows; unpaired rows: rows >= Bt always):
     * dec_in_{t+1} = prenet(mel_t) for those rows, so the gradient w.r.t. dec_in_{t+1} flows back into mel_t and the
     * projection gradient of step t can only be formed inside the loop.  All NULL / 0 for pure teacher forcing. */
    const int* step_src; int Bt;      /* host array (steps entries) as given to st_decoder_forward */
    float* dY;                        /* (steps, Bp, r*n_mels+1) [dmel_t | dstop_t]; gets the feedback gradient ADDED */
    float* dxo_rw;                    /* = dxo, written per step in this mode */
    const float* wpg_t;               /* [W_proj ; W_gate]^T   (D+E, r*n_mels+1) */
    const float* pre_w1_t; const float* pre_w0_t;   /* prenet W1^T (P,P), W0^T (r*n_mels, P) */
    const float* own_mask;            /* (steps, 2, B, P) or NULL */
    const float* xq_nat;              /* (steps+1, Bp, P+E+Q) un-tiled forward tape (dec_in = first P columns) */
    const float* pre1_nat;            /* (steps, Bp, P) un-tiled prenet layer-1 outputs */
    float* d2_tape; float* dp1_tape;  /* (steps, Bp, P) out, zero on entry: gradients at the two prenet layers (-> dW1, dW0) */
    float* tmp_p; float* tmp_in;      /* (B, P), (B, r*n_mels) scratch */
    int fuse_pw;                      /* != 0 (pure teacher forcing, packed weights incl. attn_query_w_t_p16): pointwise LSTM backward in the
                                       * epilogues of dgates_d . W (for step t-1) and of W_q^T dpq (for step t); needs dgd_t16_b and dpq_t16 */
    float* dgd_t16_b;                 /* second st_t16_floats(B, 4D) buffer, zero on entry (the epilogue writes step t-1 while step t is read) */
    float* dpq_t16;                   /* st_t16_floats(B, A) scratch, zero on entry */
    int need_dxq0;                    /* != 0: also form dxq of step 0 (the gradient of dec_in_0 = prenet(go frame), which only a
                                       * normalised prenet makes non-constant) */
    const float* attn_s_tape;         /* optional (steps, B, L, A): S_t = pm + W_l loc_t saved by the forward (slot 0 unused: S_0 =
                                       * pm).  Then loc_tape is an INPUT (the forward's attn_loc_tape) and the attention backward
                                       * neither recomputes the location conv nor the W_l product. */
    int overlap_attn;                 /* != 0 (with fuse_pw and attn_s_tape): the decoder cell's product of step t-1 and the attention backward
                                       * of step t share one launch -- the decoder cell's recurrence runs one step ahead of the attention /
                                       * query chain (3 launches per step on the critical path instead of 4) */
    /* own-output feedback through a NORMALISED prenet (st_decoder_dims.prenet_norm of the forward; 0 = plain): the forward's
     * pre_nat_tape, the norm weights (and, mode 2, running statistics) of the two layers, and (P) accumulators for their gradients,
     * zero on entry.  d2_tape / dp1_tape then hold the gradients at the two Linear outputs. */
    int prenet_norm;
    const float* pre_y_tape;          /* (steps, 2, B, P) */
    const float* pre_norm_w[2]; const float* pre_norm_rm[2]; const float* pre_norm_rv[2];
    float pre_norm_eps;
    float* dpre_norm_w[2]; float* dpre_norm_b[2];
    /* attn_parts = 2 or 4 (with overlap_attn; 0 / 1 = off): the hosted attention backward of a step runs as that many workgroups per
     * utterance (st_attn_bwd_job.parts) and the step's W_q^T dpq launch hosts the st_attn_hist_job; dloc_part (attn_parts, B, L, F) scratch */
    int attn_parts; float* dloc_part;
    /* with attn_parts = 2 and 16 < B <= 32: (dxd_splits, B, E+Q+D) scratch -- the decoder cell's product of the hosted launch runs K-split
     * (st_skinny_partial_attn_bwd) and is summed, with its pointwise epilogue, in the step's W_q^T dpq launch (st_partial_sum_job); NULL = off */
    float* dxd_part; int dxd_splits;
    /* ... and (steps + 1, dxq_splits, B, P+E+Q) slabs: the query cell's product dgates_q . [W_ih | W_hh] K-split as well; dxq then only receives
     * step 0 (need_dxq0) and the callers sum the slabs' first P columns for the teacher gradient.  NULL = off.  dxq_splits <= 4. */
    float* dxq_part; int dxq_splits;
} st_decoder_bwd_io;
/* 1 when the dimensions allow the fused BPTT loop (st_decoder_bwd_io.fuse_pw: the pointwise halves of the two LSTM cells' backward steps,
 * ref: src/module.py:227-231,275-280, in the epilogues of the loop's products): Q, D, E + Q multiples of 16, A and the input widths of the
 * three products multiples of 4.  A caller asks BEFORE it decides to hand its step tapes over uninitialised; st_decoder_backward then
 * fails (instead of falling back to the six-launch loop, which reads a zero slot) when fuse_pw is set and cannot be honoured. */
int st_decoder_bwd_fuse_dims(const st_decoder_dims* d);
/* which forms st_decoder_backward will take for these dimensions and buffers: bit 0 split attention backward, bit 1 partial decoder-cell
 * product, bit 2 partial query-cell product (dxq_part holds the gradient w.r.t. the query cell's inputs as slabs), bit 3 the fused loop
 * (io.fuse_pw and dimensions st_decoder_bwd_fuse_dims takes), bit 4 the overlapped loop (fused, overlap_attn, attn_s_tape); bits 8..11 the
 * attention workgroups per utterance (1, 2 or 4), bits 12..15 the decoder cell's K-split slabs (0 without the partial product), bits
 * 16..19 the query cell's (0 without it) */
int st_decoder_bwd_forms(const st_decoder_dims* d, const st_decoder_bwd_io* io);
/* What a split attention backward (st_attn_bwd_job.parts > 1) leaves behind, one workgroup per utterance: dloc = the partial sums added in
 * part order -> dloc_t (B, L, F); hist_t (B, L, 2) = [w_{t-1}, cum_{t-1}]; dhist (B, 2, L) = the gradient w.r.t. that history through the
 * location conv (the transposed convolution of dloc with loc_conv_w (F, 2, K)); dcum (B, L; may be NULL) += dhist(:, 1, :), the gradient
 * carried along cum_t = cum_{t-1} + w_t.  Backward of src/module.py:235-237,384-385 (stack / conv1d / transpose). */
typedef struct st_attn_hist_job {
    const float* dloc_part; int parts;
    const float* loc_conv_w;
    const float* w_prev; int ld_wprev; const float* w_cum_prev;
    float* dloc_t; float* hist_t; float* dhist; float* dcum;
    int B, L, F, K;
} st_attn_hist_job;
/* two st_skinny_linear_packed_lstm_bwd_fwd of one shape in one launch (arrays of two; p2[d].y may be NULL: the product is only consumed
 * by its epilogue); products whose K, B, N or ldy differ are refused */
int st_skinny_linear_packed_lstm_bwd_pair_fwd(const st_packed_product* p2, const st_lstm_pw_job* job2, void* stream);
/* st_skinny_linear_packed_lstm_bwd_fwd + st_attn_step_bwd in ONE launch: the attention backward of BPTT step t beside the decoder cell's
 * backward product of step t-1 (the decoder cell's recurrence does not depend on the attention / query chain of the same step).  job may
 * be NULL (the plain product); ab->s_in must be given (the forward kept S) */
int st_skinny_linear_packed_lstm_bwd_attn_bwd(const st_packed_product* p, const st_lstm_pw_job* job, const st_attn_bwd_job* ab, void* stream);
/* 1 when the attention backward's 48-position block (+ a hosting product's 8 KB) fits the LDS for these dims: what parts > 1 needs */
int st_attn_bwd_wide_fits(int L, int A, int E, int F, int K);
/* The launch an attention-step backward takes, from shapes alone (touches no memory): hosted = 0 st_attn_step_bwd (parts must be
 * 1), 1 st_skinny_linear_packed_lstm_bwd_attn_bwd beside a product of N outputs for B rows, 2 st_skinny_partial_attn_bwd; has_s: the
 * forward's S is given (s_in); loc_lin_w only for its alignment.  Returns kernel | wide << 4 | opt_in << 5 | s << 6 | wl_fast << 7 |
 * mem_pf << 8 --
 *   kernel: 0 plain, 1 hosted, 2 hosted fallback to two launches (the other bits: the plain launch), 3 dual (parts 2, both batch
 *           tiles of a product row tile in one 16-wave workgroup), 4 NB2 (ST_AB_NB2), 5 generic parts 2 (ST_AB_NO_DUAL, or not 16 < B <= 32),
 *           6 lean split parts 4, 7 partial product, 8 partial product with 16-wave workgroups (ST_PART_KW16);
 *   wide: the 48-position block (else 16); opt_in: the dynamic LDS exceeds the kernel's default limit and is raised first (the plain
 *   launch: > 64 KiB); s: the kernel starts from S; wl_fast: F == 32 and W_l 16-byte aligned; mem_pf: E <= 512 (memory rows prefetched)
 * -- or a refusal: -1 bad dims, -2 the plain launch needs more than 160 KiB of LDS, -3 hosted without S, -4 parts not possible (not 2 or
 * 4, A does not split, or the lean image does not fit), -5 not the partial form's two-part job or rows */
int st_attn_bwd_variant(int L, int A, int E, int F, int K, int has_s, int parts, int hosted, int B, int N, const float* loc_lin_w);
/* K-split partial product for 16 < B <= 32 rows: part(s, b, n) = sum over the s-th of S equal ranges of k of x(b, k) W(n, k) -- two row
 * tiles and both batch tiles per workgroup (half the bytes per output of st_skinny_linear_packed_fwd, whose workgroups each re-read a
 * whole batch tile of x), N / 32 * S workgroups; N % 32 == 0, (K / 16) % S == 0; part (S, B, N).  With `ab` (an st_attn_bwd_job with
 * parts = 2) the split attention backward of a BPTT step runs beside it in the same launch, as in
 * st_skinny_linear_packed_lstm_bwd_attn_bwd.  The slabs are added -- in split order -- by an st_partial_sum_job of the caller's next launch:
 *   y(b, n) = sum_s part(s, b, n), and for the columns [pw->n0, pw->n0 + pw->H) the pointwise LSTM backward of st_lstm_pw_job on them
 * (pw may be NULL).  Backward of nn.LSTMCell's product, ref: src/module.py:277 (dgates . [W_ih | W_hh]). */
typedef struct st_partial_sum_job {
    const float* part; int S; int N;
    float* y; int ldy;
    const st_lstm_pw_job* pw;
} st_partial_sum_job;
int st_skinny_partial_attn_bwd(const float* packed_w, const st_t16_view* x, int K, float* part, int S, int B, int N,
                               const st_attn_bwd_job* ab, void* stream);
/* the partial product with an st_attn_hist_job beside it (BPTT launch 3, dgates_q . [W_ih | W_hh], in the partial form: its consumers -- the
 * next attention backward's context addend and the query cell's dh1 addend -- take the S slabs as they are, st_attn_bwd_job.dctx_more and
 * st_lstm_pw_job.dh1_slabs) */
int st_skinny_partial_attn_hist(const float* packed_w, const st_t16_view* x, int K, float* part, int S, int B, int N,
                                const st_attn_hist_job* hist, void* stream);
/* st_skinny_linear_packed_lstm_bwd_fwd with an st_attn_hist_job and an st_partial_sum_job beside it in the same launch (the BPTT step's
 * W_q^T dpq product, which occupies half of the compute units); hist may be NULL */
int st_skinny_linear_packed_lstm_bwd_attn_hist_sum(const st_packed_product* p, const st_lstm_pw_job* job, const st_attn_hist_job* hist,
                                                   const st_partial_sum_job* sum, void* stream);
/* y = x W^T (no epilogue) with an st_attn_hist_job beside it: the BPTT step's dgates_q . [W_ih | W_hh] launch leaves 32 compute units idle
 * for 9 us -- the history part of the step's split attention backward hides there completely */
int st_skinny_linear_packed_attn_hist(const st_packed_product* p, const st_attn_hist_job* hist, void* stream);
int st_decoder_backward(const st_decoder_bwd_weights* w, const st_decoder_dims* d, const st_decoder_bwd_io* io, void* stream);
/* The two loops of a training step (st_decoder_forward with defer_proj, st_decoder_backward) are called with bit-identical arguments step after
 * step once the caller's allocator repeats its addresses: at the second sighting of an argument set the loop's launches are captured into a
 * hipGraph (thread-local capture on the calling stream) and replayed with one launch whenever the set comes back; other sets run eagerly.
 * OFF unless asked for (ST_LOOP_GRAPHS=1, st_loop_graphs_enable): it saves host time (0.8 ms of a C2 step), which the measured steps are not bound by.  st_loop_graph_stats: {replays, captures, eager calls} of the forward / backward loop (either may be NULL). */
void st_loop_graph_stats(long* fwd3, long* bwd3);
/* the replay at run time: 1 on, 0 off, -1 re-read ST_LOOP_GRAPHS; returns the previous setting */
int st_loop_graphs_enable(int on);
/* dY(t, b, :) = [dmel(b, t*r .. t*r+r-1, :) | sum_j dstop(b, t*r+j)]   (steps, Bp) rows of r*n_mels+1 values, row stride ld floats
 * (a stride rounded up to a multiple of 4, pad columns zero, puts the two products over dY on the 16-byte kernels); NULL = zeros */
int st_decoder_pack_dout(const float* dmel, const float* dstop, float* dY, int ld, int B, int Bp, int steps, int r, int n_mels,
                         void* stream);
/* the forward twin (teacher forcing with the deferred projection): Y (steps, Bp) rows [mel_t | stop_t] of stride ld -> mel (B, steps*r, n_mels)
 * and stop (B, steps*r), a step's stop value repeated r times.  ref: src/module.py:283-287 */
int st_decoder_unpack_out(const float* Y, float* mel, float* stop, int B, int Bp, int steps, int r, int n_mels, int ld, void* stream);
/* gradient of prenet(teacher) under plain teacher forcing (step t + 1 reads frame t, src/module.py:190-206): dteacher (Bt, Tt, P) = the dec_in
 * columns of dxq_{t+1}, summed over the S slabs of dxq_part (steps + 1, S, Bp, XQw) in slab order; frames t >= steps - 1: zeros */
int st_decoder_dteacher_sum(const float* dxq_part, float* dteacher, int S, int Bp, int XQw, int Bt, int Tt, int P, int steps, void* stream);
/* AdaIN statistics gradients (ref: src/module.py:267-269): adapted_t = std * (h_q_t - mean)
 * dstd = sum_t dadapt_t * (h_q_t - mean), dmean = -std * sum_t dadapt_t; *_step_stride / *_ld in elements */
int st_adain_bwd(const float* dadapt, long da_step_stride, int da_ld, const float* hq, long hq_step_stride, int hq_ld,
                 const float* ada_std, const float* ada_mean, float* dstd, float* dmean, int B, int Q, int steps, void* stream);

/* CTC loss of the paired ASR branch (ref: torch.nn.CTCLoss() as called by compute_ctcloss, bin/train_vqvae.py:430-444, with
 * paras.actual_len = False): lp = log(prob + eps), targets = the non-zero tokens of text (B, L) in order, every one of the T
 * frames counts, blank = 0, loss = mean_b(nll_b / max(S_b, 1)).  prob (B, T, V) posteriors over the codebook.  One call gives the
 * loss (device scalar) and, when dprob != NULL, d loss / d prob (the backward scales it by the incoming scalar: st_scale_by).
 * ws: st_ctc_workspace_floats(B, T) floats.  Transcripts of up to 127 tokens, at most 10240 classes.
 * log_input != 0: `prob` already holds log-probabilities (ASRPostnet's log_softmax, src/asr.py:80; compute_ctcloss(..., apply_log=False),
 * bin/train_vqvae.py:212) and the gradient is with respect to them; eps is ignored.
 * A token outside [0, V) makes that utterance's loss and gradient NaN (torch raises; the device cannot). */
size_t st_ctc_workspace_floats(int B, int T);
int st_ctc_loss(const float* prob, const int64_t* text, float eps, float* loss, float* dprob, float* ws,
                int B, int T, int V, int L, int log_input, void* stream);

/* st_ctc_loss with per-utterance frame counts (paras.actual_len = True, bin/train_vqvae.py:436-444): in_len (B) int32 on the device, or
 * NULL (= st_ctc_loss, bit for bit).  Utterance b uses the frames t < T_b = clamp(in_len[b], 0, T): alpha runs to T_b - 1, beta starts there,
 * the nll is read there.  Every gradient row t >= T_b is written as exact +0, for an infeasible utterance too (torch.nn.CTCLoss); an
 * infeasible utterance gives +inf and NaN rows for t < T_b.  T_b = 0: +inf when the utterance has tokens, 0 when it has none, all rows 0.
 * Targets stay "the non-zero tokens in order".  With actual_len the reference passes the padded 2-D targets and takes the first S_b of each
 * row; the two agree when a row's zeros are all at its end, which is how the corpus loader pads. */
int st_ctc_loss_len(const float* prob, const int64_t* text, const int32_t* in_len, float eps, float* loss, float* dprob, float* ws,
                    int B, int T, int V, int L, int log_input, void* stream);

/* The frame counts st_ctc_loss_len takes, computed on the device in one launch (no host read).
 * x != NULL (compute_ctcloss, bin/train_vqvae.py:437-438): x (B, T, D) fp32,
 *   out[b] = (number of frames t whose D values are not all == pad_value) / div     -- such frames anywhere, not only trailing ones.
 * x == NULL (the text-first branch, bin/train_vqvae.py:238-240): text (B, L) int64,
 *   len6 = 6 * (number of non-zero tokens of row b);  out[b] = 1 + (len6 + len6 % r) / div.
 * out (B) int32.  div >= 1, r >= 1. */
int st_frame_lengths(const float* x, int B, int T, int D, float pad_value, const int64_t* text, int L, int r, int div, int32_t* out,
                     void* stream);

/* greedy CTC transcript and its edit distance to the reference transcript (ref: src/util.py:169-181, cal_per -- which copies the argmax to
 * the host and runs a Python loop and editdistance.eval per utterance).  Per utterance b of prob (B, T, V), text (B, L) int64:
 *   p[t] = argmax_v prob[b, t, v] over all T frames (ties: the first maximal index; a NaN is the maximum, the first NaN wins: torch.argmax);
 *   hyp  = p[t] where t == 0 or p[t] != p[t-1] (runs collapse FIRST), then every id of ignore[0 .. n_ignore) dropped;
 *   ref  = text[b, :] with every ignored id dropped, wherever it sits;
 *   dist[b] = Levenshtein(hyp, ref) with unit costs (editdistance.eval), ref_len[b] = len(ref) (int32).
 * hyp (B, T) int64: the transcript left-aligned, padded with 0, and hyp_len (B) int32 -- both NULL, or both given.
 * Integer arithmetic only, no atomics: exact and bitwise repeatable.  One launch, no host read.
 * Limits (-22 past them): 1 <= T <= 4096, 1 <= V <= 10240, 1 <= L <= 1024, 0 <= n_ignore <= 64.
 * st_ids_edit_distance: the same with pred (B, T) int64 ids already argmaxed (cal_per's 2-D input); no V. */
int st_ctc_greedy_edit_distance(const float* prob, int B, int T, int V, const int64_t* text, int L,
                                const int32_t* ignore, int n_ignore,
                                int32_t* dist, int32_t* ref_len, int64_t* hyp /* NULL = not written */, int32_t* hyp_len /* NULL */,
                                void* stream);
int st_ids_edit_distance(const int64_t* pred, int B, int T, const int64_t* text, int L, const int32_t* ignore, int n_ignore,
                         int32_t* dist, int32_t* ref_len, int64_t* hyp, int32_t* hyp_len, void* stream);
/* st_hyp_edit_distance: the same distance for hypotheses that are already transcripts (st_ctc_beam_search's): hyp (B, Lh) int64, utterance
 * b's tokens hyp[b, 0 .. hyp_len[b]) (hyp_len (B) int32, clamped to [0, Lh]), the ignored ids dropped from both sides, runs NOT collapsed
 * ("a <blank> a" stays two tokens).  Limits: 1 <= Lh <= 4096, 1 <= L <= 1024, 0 <= n_ignore <= 64. */
int st_hyp_edit_distance(const int64_t* hyp, const int32_t* hyp_len, int B, int Lh, const int64_t* text, int L, const int32_t* ignore,
                         int n_ignore, int32_t* dist, int32_t* ref_len, void* stream);

/* CTC prefix beam search (the ASR side's transcription; the reference's --asr-decode solver is absent from its tree).
 * prob (B, T, V) fp32: log-probability log(prob + eps) when log_input == 0 (compute_ctcloss(apply_log=True), bin/train_vqvae.py:430-433),
 * prob itself when log_input != 0 (ASRPostnet's log_softmax).  Utterance b reads frames [0, lengths[b]) (lengths (B) int32 on the device,
 * NULL = all T; clamped to [0, T]); nothing beyond is read for its value, so NaN there changes nothing.
 * Each prefix carries (log p_blank, log p_nonblank) and scores their logaddexp.  Start: the empty prefix, p_blank = log 1, p_nonblank = -inf.
 * Per frame every prefix of the beam makes candidates: its stay (blank into p_blank, its last symbol repeated into p_nonblank) and one
 * extension per non-blank symbol c (fed by p_blank alone when c is its last symbol).  An extension equal to a prefix of the beam is
 * merged into that prefix's stay (exact sequence identity, never a hash).  The W best candidates form the next beam.
 * Order: score descending, then candidate index ascending; the index counts the stays first in slot order, then the extensions by
 * (slot, symbol).  Outputs, the N best prefixes after the last frame in that order: hyp (B, N, T) int64 label ids 0-padded, hyp_len (B, N)
 * int32, score (B, N) fp32 natural-log prefix probability.  lengths[b] == 0: one empty hypothesis of score 0.  A NaN log-probability in the
 * valid frames: every path of the utterance has length 0 and score NaN.  Fewer than N distinct prefixes: the surplus paths have length 0 and
 * score -inf.  No float atomics; an utterance's result depends on it alone (bitwise repeatable, independent of B).
 * Limits (-22 past them): 1 <= T <= 4096, 2 <= V <= 1024, 1 <= W <= 128, 1 <= N <= W, 0 <= blank < V.  ws:
 * st_ctc_beam_workspace_bytes(B, T, W) bytes (the prefix tree; no initialisation needed).  One launch, no host read. */
size_t st_ctc_beam_workspace_bytes(int B, int T, int W);
int st_ctc_beam_search(const float* prob, int B, int T, int V, const int32_t* lengths /* NULL = all T */, int W, int N, int blank,
                       int log_input, float eps, int64_t* hyp /* (B, N, T), 0-padded */, int32_t* hyp_len /* (B, N) */,
                       float* score /* (B, N) */, void* ws, void* stream);
/* st_ctc_beam_search_lm: the same search with an n-gram table fused into the candidate scoring.  Everything above holds (candidates,
 * merge rule, order and tie-break, outputs, NaN rule, limits, workspace, one launch, no host read, no float atomics, result independent of
 * B), with one addition.  bonus (V^(order-1), V) fp32 on the device, row-major: row r = sum_i ctx[i] V^(order-2-i) of the last order-1
 * symbols ctx (the reference's NgramPrior layout, src/lm.py:233-290), one row for order 1.  Every prefix carries its row: the empty prefix
 * row 0 when order == 1, else the row of (0, ..., 0, bos) -- NgramPrior's start, zeros then the start id.  Extending prefix A by symbol c
 * adds bonus[row(A) V + c] to the extension's log-probability -- one fp32 addition, after lp[c] -- and the new prefix has row
 * (row(A) V + c) mod V^(order-1) (0 for order 1).  Stays add nothing.  The bonus is a function of the prefix alone, so an extension merged
 * into a stay carries the same total as that stay, and a prefix scores log(its CTC prefix probability) + the sum of its extension bonuses:
 * that fused score is what `score` reports.  The column bonus[:, blank] is never read.  -inf entries are legal (a forbidden transition:
 * the candidate exists with score -inf, as structurally impossible candidates do); NaN and +inf are outside the contract and the table is
 * NOT checked here (the Python layers refuse them for host arrays; a device table is trusted).
 * Extra limits (-22 past them): 1 <= order <= 4, V^order <= 2^26 table elements, 0 <= bos < V, bonus != NULL. */
int st_ctc_beam_search_lm(const float* prob, int B, int T, int V, const int32_t* lengths /* NULL = all T */, int W, int N, int blank,
                          int log_input, float eps, const float* bonus /* (V^(order-1), V) */, int order, int bos,
                          int64_t* hyp /* (B, N, T), 0-padded */, int32_t* hyp_len /* (B, N) */, float* score /* (B, N) */, void* ws,
                          void* stream);

/* CTC forced alignment: the single most probable CTC alignment of a transcript (Viterbi over the blank-expanded targets), its
 * log-probability, the label of every frame and the frame span of every target token.  (The reference has no aligner: its AudioConverter
 * reads phone boundaries "found by MFA" from a segment_file, src/audio.py:310-327.)
 * lp[t][v] = log(prob[b,t,v] + eps) in fp32 when log_input == 0, prob[b,t,v] itself otherwise.  Utterance b reads frames [0, lengths[b])
 * (lengths (B) int32 on the device, NULL = all T; clamped to [0, T]); nothing beyond is read for its value.
 * Targets: the entries of text[b, 0 .. text_lengths[b]) (int32 on the device, NULL = all L; clamped to [0, L]) that are not `blank`, in
 * order -- with blank = 0 and text_lengths = NULL the targets st_ctc_loss trains on.  S targets give the states
 * ext = [blank, y0, blank, y1, ..., blank], n = 2 S + 1.
 * Start: a[0] = lp[0][blank], a[1] = lp[0][y0], the rest -inf.  Step: a'[s] = best + lp[t][ext[s]] (one fp32 addition), best the maximum of
 * a[s], a[s-1] and -- only when ext[s] != blank and ext[s] != ext[s-2] -- a[s-2].  Ties: the stay wins, then s-1, then s-2 (a candidate
 * replaces the best only when strictly greater).  End: the larger of a[n-1] and a[n-2], n-1 on a tie; the path is traced back from there.
 * Outputs: score (B) the end value; path (B, T) int32, path[b,t] = ext[state_t] for t < length, -1 beyond; tok_start / tok_end (B, L) int32:
 * the first frame and one past the last frame spent in state 2k+1, -1 for k >= S.
 * Without raising: S = 0 gives the all-blank path (score sum of lp[t][blank]; 0 when the length is 0 too).  A target outside [0, V): score
 * NaN.  Otherwise, infeasible (length < S + the number of adjacent equal targets; any S > 0 at length 0): score -inf.  Otherwise, a NaN among
 * the log-probabilities of the valid frames in the columns of ext: score NaN.  In all three cases path and the spans are -1 everywhere.
 * Integers and fp32 max / add only, no float atomics: an utterance's result depends on it alone (bitwise repeatable, independent of B and of
 * what lies past its lengths).  One launch, no host read.
 * Limits (-22 past them): B >= 1, 1 <= T <= 4096, 2 <= V <= 10240, 1 <= L <= 1024, 0 <= blank < V.
 * ws: st_ctc_align_workspace_bytes(B, T, L) bytes, no initialisation needed -- 0 (ws may be NULL) when the 2-bit back-pointers of a
 * (T, 2 L + 1) trellis fit LDS, which the shipped shapes do. */
size_t st_ctc_align_workspace_bytes(int B, int T, int L);
int st_ctc_forced_align(const float* prob, int B, int T, int V, const int32_t* lengths /* NULL = all T */,
                        const int64_t* text /* (B, L) */, int L, const int32_t* text_lengths /* NULL = all L */,
                        int blank, int log_input, float eps,
                        float* score /* (B) */, int32_t* path /* (B, T) */,
                        int32_t* tok_start /* (B, L) */, int32_t* tok_end /* (B, L) */, void* ws, void* stream);

/* Dynamic time warping of B ragged pairs of feature sequences: the cheapest monotone path through the grid of frame distances, its cost
 * and the path (the warp under mel-cepstral distortion, semi_tts_amd.metrics.mcd; the reference has no such measure).
 * x(b, i, k) = x[b x_sb + i x_st + k], likewise y; strides in floats.  Only the columns k in [d0, d1) are read.  Pair b is the first
 * n = x_len[b] rows of x against the first m = y_len[b] rows of y (lengths (B) int32 on the device, NULL = all Tx / Ty; clamped to
 * [0, Tx] / [0, Ty]); nothing beyond is read for its value.
 * Cost: d(i, j) = scale * sqrtf(sum_{k = d0}^{d1 - 1} (x[i,k] - y[j,k])^2), the sum in fp32 over ascending k (whether the compiler
 * contracts it to fma is not specified).  Recurrence: D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), predecessors outside
 * the grid absent, D(0, 0) = d(0, 0); the addition is ONE fp32 add of the chosen predecessor and d.  Ties: the diagonal wins, then
 * (i-1, j), then (i, j-1) (a candidate replaces the best only when strictly smaller).  This is the unweighted symmetric step pattern.
 * Outputs: total (B) = D(n-1, m-1); path_len (B) = P, the cells on the path traced back from (n-1, m-1); path (B, Tx + Ty - 1, 2) int32,
 * path[b, p, :] = (i_p, j_p) for p < P in forward order from (0, 0) to (n-1, m-1), -1 for p >= P.  path == NULL: only total and path_len.
 * Without raising: n == 0 or m == 0, or a NaN among the read columns of the valid rows of either side: total NaN, path_len 0, path -1
 * everywhere.  (Infinite inputs are outside the contract: the path is still a valid one, its cost may be NaN.)
 * fp32 compare / add only, no float atomics: a pair's outputs depend on that pair alone (bitwise repeatable, independent of B, of the
 * pair's position in the batch and of what lies beyond its lengths, NaN included).  One launch (the trace-back is part of it), no host read.
 * Limits (-22 past them): B >= 1, 1 <= Tx, Ty <= 4096, 0 <= d0 < d1, d1 - d0 <= 64, x_st and y_st >= d1, x_sb and y_sb >= 0, scale finite
 * and positive.
 * ws: st_dtw_workspace_bytes(B, Tx, Ty) bytes, no initialisation needed -- 0 (ws may be NULL) when the 2-bit back-pointers of a
 * (Tx, Ty) grid fit LDS beside the three rolling diagonals, which utterances of a few seconds at a 10 ms hop do. */
size_t st_dtw_workspace_bytes(int B, int Tx, int Ty);
int st_dtw_batch(const float* x, long x_sb, long x_st, const int32_t* x_len /* NULL = all Tx */, int Tx,
                 const float* y, long y_sb, long y_st, const int32_t* y_len /* NULL = all Ty */, int Ty,
                 int B, int d0, int d1, float scale,
                 float* total /* (B) */, int32_t* path_len /* (B) */, int32_t* path /* (B, Tx + Ty - 1, 2) or NULL */,
                 void* ws, void* stream);

/* Where an utterance ends, read off the decoder's attention, and the alignment diagnostics of the same pass (the model has no trained
 * stop gate: the reference decodes to the length of the ground-truth mel; semi_tts_amd.metrics.attention_endpoints, main.py --synth-phn-dir).
 * align(b, t, j) = align[b a_sb + t a_st + j], strides in floats, unit stride in j; all L columns of all S rows are read.  n = enc_len[b]
 * ((B) int32 on the device, clamped to [1, L]) is the count of real phones of utterance b.
 * Peak: peak[t] = the lowest column among the maxima of row t over all L columns; a NaN entry never wins, a row without a non-NaN entry
 * has peak 0.  maxw[t] = that maximum, 0 for such a row.
 * End: flag[t] = peak[t] >= n - 1.  t0 = the smallest t with t + K <= S and flag[t .. t + K - 1] all set (K = patience).  With such a
 * t0: end = t0 + K, reached = 1; without: end = S, reached = 0 (a run of fewer than K flags that touches step S - 1 is no detection).
 * Over the steps [0, end): focus = the fp32 mean of maxw; n_back = the t >= 1 with peak[t] < peak[t-1]; n_skip = the t >= 1 with
 * peak[t] > peak[t-1] + max_jump; dur[j] = the steps with peak == j, for every j < L; covered = the j < n with dur[j] > 0.
 * nonfinite = 1 when any entry of the S rows is NaN or +-inf, else 0.
 * Outputs: stats (B, 6) int32 = (end, reached, n_back, n_skip, covered, nonfinite); focus (B); peak (B, S) int32, all S steps;
 * dur (B, L) int32.  No output needs initialising.
 * Integer compares and LDS integer atomics; the focus sum has a fixed order that depends on `end` alone: every output of an utterance
 * is bitwise repeatable and independent of B, of its position in the batch and of the other utterances (NaN included).
 * One launch (one workgroup per utterance), no workspace, no host read.
 * Limits (-22 past them): B >= 1, 1 <= S <= 4096, 1 <= L <= 2048, a_st >= L, a_sb >= 0, patience >= 1, max_jump >= 1. */
int st_attn_endpoint(const float* align, long a_sb, long a_st, const int32_t* enc_len /* (B) */,
                     int B, int S, int L, int patience, int max_jump,
                     int32_t* stats /* (B, 6) */, float* focus /* (B) */,
                     int32_t* peak /* (B, S) */, int32_t* dur /* (B, L) */, void* stream);

/* The trainer's scalar arithmetic on loss values as one launch (ref: bin/train_vqvae.py:208-233: total_loss = asr_weight * asr_loss +
 * tts_weight * (mel_loss + linear_loss) + unpair_speech_weight * ... -- a chain of one-element torch kernels there):
 * *outs[j] = sum_i W[j * n + i] * *xs[i] for j < m (m <= 4 outputs, n <= ST_SCALAR_MAX terms, W on the host; in rows j > 0 a zero weight means the term is not a member of that sum).
 * st_scalar_fanout is the backward of output 0: out[i] = w[i] * *dout. */
#define ST_SCALAR_MAX 8
int st_scalar_combine(const float* const* xs, int n, const float* W, int m, float* const* outs, void* stream);
int st_scalar_fanout(const float* dout, const float* w, int n, float* out, void* stream);

/* ------------------------------------------------------------------ trainer loss
 * loss = w_all*crit(pred,label) + w_low*crit(low n_low bins) + w_diff*crit(first differences along T), crit = MSE or
 * (l1 != 0) mean absolute error; writes the scalar to *loss and d loss / d pred to dpred (B,T,D).  ws: st_freq_loss_workspace_floats() floats (one partial sum per workgroup).
 * ref: freq_loss src/util.py:80-126 (mel: w = 1, 0, 0.5; linear with low-band emphasis: w = 0.5, 0.5, 0) */
size_t st_freq_loss_workspace_floats(void);
int st_freq_loss(const float* pred, const float* label, float* loss, float* dpred, float* ws,
                 int B, int T, int D, int n_low, float w_all, float w_low, float w_diff, int l1, void* stream);
/* Several st_gemm_wgrad / st_gemm_wgrad_db (db may be NULL per job; no pooling, no accumulation) as ONE product launch and ONE slab-sum launch
 * when every job takes the LDS-DMA form (16-byte addressable rows, N and Cin multiples of 4, Cin >= 16) on 64-tiles; otherwise one after the
 * other.  Each job keeps its own slab count and summation order: bit for bit the results of the separate calls.  For the K weight
 * gradients of the CBHG conv bank (80 x 80 x k: eight launches that each leave most of the chip idle) and the two directions of a
 * recurrent layer.  ws: st_gemm_wgrad_batch_workspace_floats(jobs, n) floats.  ref: backward of src/module.py:590-598. */
typedef struct st_wgrad_job {
    const float* dC; int lddc, dcoff; const float* A; int lda; float* dW; float* db;
    int Bn, Tin, Tout, Cin, N, KT, pad;
} st_wgrad_job;
size_t st_gemm_wgrad_batch_workspace_floats(const st_wgrad_job* jobs, int n);
int st_gemm_wgrad_batch(const st_wgrad_job* jobs, int n, float* ws, void* stream);
/* What st_gemm_wgrad[_db] (with_db) / st_gemm_wgrad_split (with_split) would launch (host only: pointers are looked at for their
 * alignment, never read; negative on bad arguments): product | sum << 8 | Z << 16 with
 *   product: 0 the few-channel kernel, 1 LDS-DMA 64-tiles, 2 LDS-DMA 128-tiles on 16-row chunks, 3 / 4 register-staged 64 / 128-tiles;
 *            + 8 folded (channel, tap) columns, + 16 Linear rows, + 32 fused max-pool, + 64 written straight to dW (one slab);
 *   sum:     0 none, 1 one thread per element, 2 slab groups met in LDS (many slabs), 3 with the bias-gradient slabs, 4 the same
 *            cut into two outputs;  Z: slab count.
 * st_gemm_wgrad_batch_variant: codes[i] = 1 + the group launch job i of st_gemm_wgrad_batch joins, 0 when it runs as a call of its
 * own; returns the number of group launches. */
int st_gemm_wgrad_variant(const float* dC, int lddc, int dcoff, const float* A, int lda, int Bn, int Tin, int Tout, int Cin,
                          int N, int KT, int pad, int pool_prev, int accumulate, int with_db, int with_split);
int st_gemm_wgrad_batch_variant(const st_wgrad_job* jobs, int n, int* codes);
/* st_gemm_wgrad[_db] of a Linear over CONCATENATED inputs (KT = 1; M rows), the result cut at input column `split`:
 * dW0 (N, split) and dW1 (N, Cin - split) are the gradients of the two weights whose columns the product saw side by side -- an
 * nn.LSTMCell fed with [x | h] has gates = [W_ih | W_hh] [x | h]^T (ref: src/module.py:227-231,275-280), so the BPTT weight gradient
 * over the step tapes lands in the two parameters' own gradient tensors (under data parallelism: in their all-reduce bucket slots)
 * instead of one tensor that two copies then cut up.  db (may be NULL) = column sums of dC; db_dup (may be NULL) receives the same
 * sums once more (b_ih and b_hh have equal gradients). */
int st_gemm_wgrad_split(const float* dC, int lddc, int dcoff, const float* A, int lda, float* dW0, int split, float* dW1,
                        float* db, float* db_dup, float* ws, int M, int Cin, int N, int accumulate, void* stream);
/* y = x * (*scalar)   (scalar on the device: the incoming gradient of a scalar loss) */
int st_scale_by(const float* x, const float* scalar, float* y, size_t n, void* stream);

/* ------------------------------------------------------------------ optimiser step (multi-tensor)
 * ref: BaseSolver.backward src/solver.py:138-151 (clip_grad_norm_ 5.0, optimizer.step()), torch.optim.Adam as built by
 * src/optim.py.  The pointer arrays are HOST arrays of device pointers (nt tensors, n[t] elements each); the
 * kernels take them through their arguments, a few launches for ~100 tensors. */
long st_mt_table_misses(void);   /* diagnostics: block maps built and uploaded so far (once per set of tensor addresses; the multi-tensor
                                    * launches below read their tensor list from a cached device-side table) */
size_t st_mt_blocks(const long* n, int nt);                   /* floats of `partials` st_mt_grad_norm needs */
/* *norm_out (device) = sqrt(sum_t sum_i g_t[i]^2), fixed summation order */
int st_mt_grad_norm(float* const* g, const long* n, int nt, float* partials, float* norm_out, void* stream);
/* g *= max_norm / (norm + 1e-6) when that is < 1 (torch.nn.utils.clip_grad_norm_); norm is a device scalar */
int st_mt_clip_scale(float* const* g, const long* n, int nt, const float* norm, float max_norm, void* stream);
/* The same pair for gradients that are still the SUM over `world` data-parallel ranks (pre_scale = 1 / world): *norm_out =
 * pre_scale * sqrt(sum g^2) = the norm of the AVERAGED gradients, and the clip launch multiplies every gradient by
 * pre_scale * min(1, max_norm / (norm + 1e-6)) -- the average of the all-reduce costs no launch of its own (ref: the reference
 * clips the single-process gradient, src/solver.py:145; data parallelism is this path's extension). */
int st_mt_grad_norm_scaled(float* const* g, const long* n, int nt, float* partials, float* norm_out, float pre_scale, void* stream);
int st_mt_clip_scale_pre(float* const* g, const long* n, int nt, const float* norm, float max_norm, float pre_scale, void* stream);
/* dst_t[i] = src_t[i] for nt tensors in a handful of launches (gradients that autograd allocated elsewhere are gathered into their
 * all-reduce bucket by one call per bucket) */
int st_mt_copy(float* const* dst, float* const* src, const long* n, int nt, void* stream);
/* Host arithmetic only (like st_gemm_fwd_variant / st_packed_fwd_variant: no device, nothing behind the sizes is touched): the launches
 * the KERNEL-ARGUMENT form makes for a size list -- the form taken during a stream capture, when no device-side table can be made.
 * kind 0: the optimiser passes (norm, clip, Adam: 24 tensor slots, 640 blocks of 32768 floats per launch); kind 1: st_mt_copy (96 slots,
 * 512 blocks of 4096 floats).  Returns the number of launches and writes blocks[i] / tensors[i] (blocks and tensor slots of launch i; a
 * tensor cut across launches takes a slot in each) for the first `cap` of them; 0 for a list of empty tensors; negative for a refusal
 * (bad arguments, or a tensor too long for the 16-bit chunk index).  The launchers run the same splitting code. */
int st_mt_launch_plan(const long* n, int nt, int kind, int* blocks, int* tensors, int cap);
/* torch.optim.Adam (no weight decay, no amsgrad): m = m + (g-m)(1-b1); v = b2 v + (1-b2) g^2;
 * p -= step_size * m / (sqrt(v)/bias_correction2_sqrt + eps), step_size = lr / (1 - b1^t).  The betas travel as doubles: the kernel
 * multiplies by (float)b2 and by (float)(1.0 - b), each rounded once from the double as torch's Adam rounds them (1.0f - (float)0.999
 * would be 0.00099998713, 1.3e-5 away from the 0.001 on g^2) */
int st_mt_adam(float* const* p, float* const* g, float* const* m, float* const* v, const long* n, int nt,
               double beta1, double beta2, float eps, float step_size, float bias_correction2_sqrt, void* stream);
/* st_mt_adam that leaves parameters and moments untouched when *guard_norm (a device scalar: the gradient norm st_mt_grad_norm wrote)
 * is NaN or inf -- BaseSolver.backward's `if math.isnan(grad_norm): ... else: self.optimizer.step()` (src/solver.py:147-150) decided
 * on the device, so a training loop need not wait for the norm on the host every step.  guard_norm NULL = st_mt_adam. */
int st_mt_adam_guarded(float* const* p, float* const* g, float* const* m, float* const* v, const long* n, int nt,
                       double beta1, double beta2, float eps, float step_size, float bias_correction2_sqrt,
                       const float* guard_norm, void* stream);

/* ------------------------------------------------------------------ small utilities */
int st_fill(float* p, float v, size_t n, void* stream);

/* Re-layouts of many PARAMETERS in one launch: what `w.permute(0, 2, 1).contiguous()` (mode 0: Conv1d weight (N, Cin, KT) -> tap-major
 * (N, KT, Cin), the forward implicit-GEMM operand) and `w.permute(1, 0, 2).flip(2)` in tap-major form (mode 1: -> (Cin, KT, N) with the
 * taps reversed, the weight of the input-gradient conv; KT = 1: the transpose of a Linear weight) do one torch copy at a time.
 * `table_dev` is a DEVICE array of n descriptors ordered by blk0; descriptor d owns workgroups [blk0, blk0 + st_relayout_blocks(N, Cin, KT)).
 * Replaces the per-weight layout copies in front of torch's conv / linear backward (src/module.py: every Conv1d / Linear). */
typedef struct st_relayout_desc {
    const float* src; float* dst;
    int N, Cin, KT, mode;
    int blk0;
    int ld_dst;     /* mode 1 only: row stride of dst in floats (0 = N): the layout lands in a column block of a wider matrix (the
                     * transposes of several Linear weights side by side = the weight of ONE input-gradient product) */
} st_relayout_desc;
int st_relayout_blocks(int N, int Cin, int KT);
/* blk_desc_dev: optional DEVICE array of total_blocks ints, the descriptor index of every workgroup (NULL: each workgroup searches the table) */
int st_relayout_batch(const st_relayout_desc* table_dev, int n, int total_blocks, const int* blk_desc_dev, void* stream);
int st_copy2d(float* dst, int ldd, const float* src, int lds, int rows, int cols, void* stream);
/* dst(b, :) = mean over t of src(b, t, :)    ref: teacher.mean(dim=1) src/module.py:194 */
int st_mean_rows(const float* src, float* dst, int B, int T, int D, void* stream);

/* ------------------------------------------------------------------ Griffin-Lim vocoder (linear spectrogram -> waveform)
 * Replaces AudioProcessor.specgram_to_waveform / _griffin_lim / _stft / _istft / _inv_preemphasis (ref: src/audio.py:179-192,
 * 208-262, 274-288) for the linear branch of feat_to_wave (:397-407).  STFT conventions of the reference: center=True,
 * pad_mode='reflect', onesided, unnormalised, periodic Hann window of `win` samples zero-padded to n_fft at offset
 * (n_fft - win) / 2; the iSTFT divides the overlap-add by the window-square envelope and trims n_fft / 2 at both ends (no
 * `length`: hop * (T - 1) samples; lib/istft.py).  Supported: n_fft in {512, 1024, 2048, 4096}, 0 < 2 * hop <= win <= n_fft,
 * signals longer than n_fft / 2 samples (anything else returns -22).  Spectra are frame-major (B, T, n_fft / 2 + 1) complex
 * (re, im interleaved): the (B, F, T) tensor of torch.stft transposed.  No atomics: results are bitwise repeatable.  The first
 * call on a device uploads the FFT twiddle tables (computed in double on the host) and may not be inside a stream capture. */
/* the framing of every entry point of this family; a refusal names the framing first, then batch / frames (T < 2), then a short signal */
typedef struct st_framing { int n_fft, win, hop; } st_framing;
size_t st_istft_workspace_floats(int B, int T, int n_fft, int hop, int win);
/* spec (B, 1 + L / hop, n_fft / 2 + 1, 2) = torch.stft(x (B, L), ...)    ref: AudioProcessor._stft src/audio.py:234-246 */
int st_stft_fwd(const float* x, float* spec, int B, int L, int n_fft, int hop, int win, void* stream);
/* x (B, hop * (T - 1)) = istft(spec (B, T, n_fft / 2 + 1, 2))    ref: AudioProcessor._istft src/audio.py:248-262, lib/istft.py
 * ws: st_istft_workspace_floats() floats.  3 launches. */
int st_istft(const float* spec, float* x, int B, int T, int n_fft, int hop, int win, float* ws, void* stream);
/* lin (B, T, F) contiguous = the mel -> linear product of melspecgram_to_specgram (ref: src/audio.py:194-205):
 * lin[b, t, k] = sum_m basis[m, k] a[b, t, m], mel(b, t, m) = mel[b * sb + t * st + m * sm] (strides in floats), basis (n_mels, F)
 * row-major = pinverse(mel filterbank) transposed (computed by the caller, once).  normalized = 1: a = _db_to_amp(_denormalize(mel)
 * + REF_LEVEL_DB), the expressions of the Griffin-Lim kernels; 0: a = mel.  take_abs = 1 stores |lin| (what _griffin_lim takes, :217);
 * 0 the signed product the reference method returns.  Supported: 1 <= n_mels <= 256, F = n_fft / 2 + 1 of a supported n_fft
 * (anything else returns -22).  One launch; each output is an fmaf chain over ascending m: bitwise independent of batch and tiling. */
int st_mel_to_linear(const float* mel, long sb, long st, long sm, const float* basis, float* lin, int B, int T, int n_mels, int F,
                     int normalized, int take_abs, void* stream);
/* Griffin-Lim, the one vocoder entry: wav (B, hop * (T - 1)) after n_iter iterations (ref: _griffin_lim src/audio.py:208-226,
 * GFL_ITER = 30), from linear or mel input, for utterances of one frame count or of their own.
 * feat(b, t, f) = feat[b * sb + t * st + f * sf] (strides in floats; the decoder's (B, T, F) is sb = T F, st = F, sf = 1).
 * basis == NULL, n_in == n_fft / 2 + 1: feat is the linear spectrogram.  normalized = 1: it is the normalised spectrogram and the
 * magnitude is _db_to_amp(_denormalize(feat) + REF_LEVEL_DB) ** power (:186-188, :281-288); 0: feat is the magnitude.
 * basis != NULL, n_in == n_mels: feat is the mel spectrogram (B, T, n_mels) through the same strides; the magnitude is
 * |mel -> linear product| (one more launch, into the workspace) and power must be 1 (the reference's mel branch is isAmp, :402-408).
 * phases: initial phases (B, F, T) contiguous (:214-216, drawn by the caller).  post: bit 0 = inverse pre-emphasis y[n] = x[n] +
 * 0.97 y[n-1] (the literal of :274-276, scipy.signal.lfilter([1], [1, -0.97])), bit 1 = clip to [-1, 1] (:192).
 * frames: DEVICE int32 array of B frame counts, or NULL for T everywhere (the uniform kernels: one envelope, no per-utterance clamp).
 * Utterance b has T_b = frames[b] frames and L_b = hop * (T_b - 1) samples: reflect padding, overlap-add, envelope, inverse
 * pre-emphasis and clip are those of a T_b-frame utterance vocoded alone (bitwise).  Storage keeps the strides of T: feat rows and
 * phase columns t >= T_b are never read; wav is (B, hop * (T - 1)), row b written on [0, L_b) and zero after.  The kernels clamp
 * frames[b] into [n_fft / 2 / hop + 2, T] (the fewest frames the reflect padding takes; T itself is checked), so no value indexes
 * outside the workspace; validating frames is the caller's.  ws: st_gl_batch_workspace_floats() floats.  n_iter + 3 launches (+ 1: mel). */
typedef struct st_gl_job {
    const float* feat; long sb, st, sf; int n_in; const float* basis;       /* basis NULL: feat is linear, n_in = n_fft / 2 + 1 */
    int normalized; float power; const float* phases; const int* frames;   /* frames NULL: T for every utterance */
    float* wav; int B, T, n_iter, post;
} st_gl_job;
size_t st_gl_batch_workspace_floats(int B, int T, int n_fft, int hop, int win);
int st_griffin_lim_batch(const st_gl_job* job, const st_framing* fr, float* ws, void* stream);

/* ------------------------------------------------------------------ feature extraction (waveforms -> normalised spectrograms)
 * Host arrays (B entries, read before the call returns): off, len, and win / hop / snr_db of st_feat_aug; all else is on the device. */
/* ragged batch of packed float32 waveforms: utterance b is x[off[b] .. off[b] + len[b]) of the n_samples in x; B <= 64 */
typedef struct st_wave_batch { const float* x; long n_samples; const long* off; const int* len; int B; } st_wave_batch;
/* banded mel filterbank (Slaney / area-normalised): mel[m] = sum_j |X|[start[m] + j] * w[off[m] + j], j < cnt[m] */
typedef struct st_mel_bank { const int* start; const int* cnt; const int* off; const float* w; int n_mels; } st_mel_bank;
/* the augmented framing of st_audio_features (a NULL st_feat_aug* or out == NULL: none).  out (B, Ta_pad, n_mels) is the augmented
 * mel: its own framing win[b] / hop[b] (the time-stretched win / hop of src/audio.py:366-373), and s = x + coeff_b n with coeff_b =
 * sqrt(sum x^2 / sum n^2 * 10^(-snr_db[b] / 10)) over the utterance (snr_db null, or NaN for an utterance: no noise).  n: `noise`,
 * packed like x, or, when null, the built-in counter-based generator (Philox4x32-10, standard normal by Box-Muller) of (seed,
 * utt0 + b, sample index): no noise buffer exists.  utt0 is the position of this call's first utterance in the caller's whole batch
 * (0 for a batch issued in one call): a batch above 64 issued in several calls then draws the noise st_feature_noise() gives for
 * each utterance's position in the batch.  Only the generator reads utt0; the arrays and the output rows are relative to this call. */
typedef struct st_feat_aug { const int* win; const int* hop; const float* snr_db; const float* noise;
                             unsigned long long seed; int utt0; float* out; int Ta_pad; } st_feat_aug;
/* Replaces AudioProcessor.extract_feature_from_waveform (ref: src/audio.py:156-177) and AudioConverter.wave_to_feat's feature
 * and augmentation steps (:329-395, add_noise / snr_coeff :409-416, :434-437) for a ragged batch.  Each frame is the torch.stft
 * frame (same conventions as st_stft_fwd, reflect padding at the utterance's own length) of the pre-emphasised signal y[0] = s[0],
 * y[i] = s[i] - preemph * s[i-1] (preemph 0: none), built on the fly; the magnitude |X| gives linear = norm(|X|) and mel[m] =
 * norm(the band sum of st_mel_bank) with norm(a) = clamp((20 log10(max(a, 1e-5)) - 20 + 100) / 100, 0, 1) (_amp_to_db, _normalize).
 * Outputs are time-major: mel (B, T_pad, n_mels), linear (B, T_pad, n_fft / 2 + 1) (null: not written), frames t >= 1 + len[b] / hop
 * written as 0 (SPEC_PAD_VALUE), T_pad >= 1 + max len / hop; likewise aug->out with Ta_pad at the augmented framing.
 * Supported: n_fft in {512, 1024, 2048, 4096}, 0 < 2 * hop <= win <= n_fft for both framings, len[b] > n_fft / 2, B <= 64
 * (anything else returns -22, before any device call).  ws: st_features_workspace_floats(B) floats.  One launch (clean + augmented
 * framings as the two z-slices of one grid), plus one before it for the per-utterance power sums when there is noise.  No atomics:
 * bitwise repeatable for a given seed. */
size_t st_features_workspace_floats(int B);
int st_audio_features(const st_wave_batch* w, const st_framing* fr, float preemph, const st_mel_bank* fb, const st_feat_aug* aug,
                      float* mel, float* linear, int T_pad, float* ws, void* stream);
/* out[i] = the built-in generator's standard normal for (seed, utterance utt, sample i), i < n (for tests) */
int st_feature_noise(float* out, long n, int utt, unsigned long long seed, void* stream);
/* MFCC with derivatives (ref: AudioProcessor.extract_mfcc_from_waveform, src/audio.py:119-154) for a ragged batch (st_wave_batch):
 * out (B, T_pad, 3 * n_mfcc).  Frame t of utterance b is the frame of st_audio_features' clean framing
 * (same pre-emphasis, reflect padding, window, filterbank and norm) at the caller's framing -- the reference's MFCC framing is
 * win = int(0.025 sr), hop = int(0.010 sr) in the model's n_fft.  Columns [0, n_mfcc): c[k] = sum_m dct[k, m] mel[m] over the
 * NORMALISED [0, 1] mel (librosa.feature.mfcc(S=mel, n_mfcc) = scipy.fftpack.dct(mel, axis=0, type=2, norm='ortho')[:n_mfcc]; the
 * reference hands it the normalised mel, kept here), dct (n_mfcc, n_mels) row-major on the device, tabulated by the caller:
 * dct[k, m] = sqrt(2 / n_mels) cos(pi (2 m + 1) k / (2 n_mels)), row 0 divided by sqrt(2).  Each c[k] is one fmaf chain over
 * ascending m.  Columns [n_mfcc, 2 n_mfcc) and [2 n_mfcc, 3 n_mfcc): librosa.feature.delta(c) and delta(c, order=2) =
 * scipy.signal.savgol_filter(c, 9, deriv=o, polyorder=o, axis=time, mode='interp'), which is the 9-tap filter with its centre
 * clamped into [4, T_b - 5]: with tc = min(max(t, 4), T_b - 5),
 *     delta[t] = sum_{j=-4..4} (j / 60) c[tc + j],   delta2[t] = sum_j w2[j] c[tc + j],  w2 = (28, 7, -8, -17, -20, -17, -8, 7, 28) / 462
 * (order 2 is the second derivative of c, not a delta of the delta), each one fmaf chain over ascending j.  T_b = 1 + len[b] / hop;
 * rows t >= T_b are written as 0, T_pad >= max T_b.  mel_out (B, T_pad, n_mels) (null: not written): the normalised mel at this
 * framing.  A frame's bits depend on neither the batch nor the position in it.  Supported (anything else returns -22): n_fft in
 * {512, 1024, 2048, 4096}, 0 < 2 * hop <= win <= n_fft, len[b] > n_fft / 2, 1 <= n_mfcc <= n_mels <= 256, len[b] >= 8 * hop (T_b >= 9:
 * librosa refuses a width above the frame count), B <= 64.  Two launches (frames, then derivatives); no atomics, no workspace. */
int st_audio_mfcc(const st_wave_batch* w, const st_framing* fr, float preemph, const st_mel_bank* fb, const float* dct, int n_mfcc,
                  float* out, float* mel_out, int T_pad, void* stream);
/* Phone segments (ref: AudioProcessor.segment, src/audio.py:94-117): out (S, max_len, D) contiguous, 16-byte aligned, from
 * feat (B, T_pad, D) with feat(b, t, d) = feat[b * sb + t * st + d] (strides in floats, st >= D).  Row i < seg_len[s] of segment s
 * is feat[seg_utt[s], seg_start[s] + i, :] copied exactly; every other row is 0.  seg_utt, seg_start, seg_len: DEVICE int32 arrays
 * of S entries.  The utterance index is clamped into [0, B) and the frame index into [0, T_pad), so a wrong table cannot index
 * outside feat.  S == 0 or max_len == 0 returns 0 without a launch.  One launch, 16-byte stores, any D. */
int st_segment_gather(const float* feat, long sb, long st, int B, int T_pad, int D, const int* seg_utt, const int* seg_start,
                      const int* seg_len, int S, int max_len, float* out, void* stream);

/* ------------------------------------------------------------------ sample-rate conversion (waveforms -> waveforms)
 * Not a step of the reference (its AudioProcessor.load refuses a foreign rate, src/audio.py:70-77, and leaves conversion to an
 * offline tool).  Windowed-sinc interpolation with a Hann window (the default of torchaudio.functional.resample:
 * lowpass_filter_width lpw = 6, rolloff 0.99) for the ratio o / n = orig_sr / new_sr in lowest terms.  With base = min(o, n) *
 * rolloff, W = lpw * o / base and tau_m = m o / n:
 *     y[m] = (base / o) sum_{i : |i - tau_m| < W} sinc(pi base (i - tau_m) / o) cos^2(pi base (i - tau_m) / (2 lpw o)) x[i],
 * x[i] = 0 outside [0, L), m = 0 .. ceil(n L / o) - 1.  The weights depend on the phase p = m mod n only: the host tabulates
 * them (semi_tts_amd.audio.resample_table: float64, rounded once) as table (n, taps), row p holding the weights (scale included)
 * of x[floor(tau_m) + first[p] + k], k < taps, zero where |i - tau| >= W.  The kernel forms
 *     y[m] = fma(table[p][taps-1], x[..], ... fma(table[p][0], x[floor(tau_m) + first[p]], 0))
 * one chain in ascending tap order, so a sample's bits do not depend on the tile, the batch or the position in it.
 * x: the packed input, float32 or (pcm16 != 0) int16 PCM scaled by 1 / 32768 in the kernel (exact); utterance b is
 * x[off[b] .. off[b] + len[b]) and is written to y[out_off[b] .. out_off[b] + ceil(n len[b] / o)); nothing else of y is written.
 * Host arrays: off, len, out_off (B entries, read before the call returns); first (n ints) and table are on the device.
 * first_min / first_max: bounds of first[] (the kernel clamps its reads into the staged span, so an inconsistent `first` cannot
 * index outside it).  Limits (anything else returns -22): B <= 64, len[b] >= 1, o n < 2^31, min(n, 1024) * ((taps | 1) + 1) <=
 * 9216 floats of staged table and ceil(1023 o / n) + first_max - first_min + taps <= 6912 staged input samples: one workgroup
 * (1024 outputs of one utterance) holds both in LDS, at most 63 KB.  One launch, no atomics, no workspace. */
int st_resample_batch(const void* x, int pcm16, long n_samples, const long* off, const int* len, int B, int o, int n, int taps,
                      int first_min, int first_max, const int* first, const float* table, float* y, long n_out, const long* out_off,
                      void* stream);

/* ------------------------------------------------------------------ pitch (waveforms -> F0 tracks) and F0 figures along a warp
 * Not a step of the reference (it has no pitch tracker).  st_f0_yin is the YIN estimator (de Cheveigne & Kawahara 2002, steps 2 - 5)
 * on the RAW waveform (no pre-emphasis) of a ragged batch (st_wave_batch, B <= 64).
 * Frames.  Utterance b with L = len[b] samples x[0 .. L) has the frames t = 0 .. T - 1, T = 1 + L / hop (the MFCC frame count at
 * hop = hop_length_mfcc: a DTW path over MFCC rows indexes F0 rows directly).  Frame t starts at s0 = t hop - W / 2 (integer
 * division) and reads the W + tau_max samples x[s0 .. s0 + W + tau_max), with x[i] = 0 for i outside [0, L).
 * Difference function, the DIRECT form in fp32:  d(tau) = sum_{j = 0}^{W - 1} (x[s0 + j] - x[s0 + j + tau])^2,  tau = 0 .. tau_max,
 * every term non-negative, formed as one chain acc = fmaf(e, e, acc), e = x[s0 + j] - x[s0 + j + tau], over ascending j.  (The
 * autocorrelation / FFT form r(0) + r_tau(0) - 2 r(tau) cancels and is not used.)
 * Cumulative-mean-normalised difference:  c(tau) = sum_{k = 1}^{tau} d(k) (an fp32 prefix sum whose order depends on tau_max alone),
 * d'(0) = 1,  d'(tau) = d(tau) * tau / c(tau) (one fp32 product, one correctly rounded quotient), or 1 where c(tau) = 0 (digital silence).
 * Search.  tau0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold.  Without one the frame is unvoiced: f0 = 0,
 * aper = min_{tau in [tau_min, tau_max]} d'(tau).  Otherwise tau* = the smallest tau >= tau0 with tau = tau_max or d'(tau + 1) >= d'(tau).
 * Parabolic refinement with a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1): when tau* < tau_max and a > b,
 * delta = 0.5 (a - c) / ((a - b) + (c - b)) (the denominator a - 2b + c, positive by construction; delta in (-0.5, 0.5]); otherwise
 * delta = 0.  f0 = sample_rate / (tau* + delta), aper = b.
 * Outputs: f0 (B, T_pad) in Hz, aper (B, T_pad) or NULL; rows t >= T up to T_pad are written 0.  A NaN or an infinity among the
 * samples a frame reads makes that frame's f0 and aper NaN, and only that frame's.  A frame depends on its utterance alone: bitwise
 * repeatable, independent of B, of the position in the batch and of T_pad.  One launch, no workspace, no atomics, no host read.
 * Limits (-22 past them, before any device call): 1 <= B <= 64, every len >= 1, hop >= 1, 2 <= tau_min < tau_max <= 1024,
 * 1 <= W <= 2048, T_pad >= the largest T, 0 < threshold <= 1 (finite), sample_rate finite and positive.
 * st_f0_run_length: the consecutive frames one workgroup takes from one staged span at this framing (8, fewer when 7 hop + W + tau_max
 * would pass 10240 samples; 0 outside the limits) -- for tests that straddle it. */
int st_f0_run_length(int hop, int W, int tau_max);
int st_f0_yin(const st_wave_batch* w, int hop, int W, int tau_min, int tau_max, float sample_rate, float threshold,
              float* f0 /* (B, T_pad) */, float* aper /* (B, T_pad) or NULL */, int T_pad, void* stream);

/* F0 figures of B pairs of tracks along a warp: f0_x(b, i) = f0_x[b x_sb + i], i < Tx, likewise f0_y (strides in floats); path
 * (B, P, 2) int32 and path_len (B) exactly as st_dtw_batch writes them (P = its Tx + Ty - 1; -1 past path_len).  Only the first
 * path_len[b] (clamped to [0, P]) entries are read; an index outside [0, Tx) x [0, Ty) among them is NOT checked.
 * A frame is voiced iff f0 > 0 (NaN: unvoiced).  counts (B, 4) int32 = (n_pairs = path_len, n_both = pairs with both sides voiced,
 * n_vuv = pairs whose voicing differs, n_gross = both-voiced pairs with |fx - fy| > 0.2 fy, compared in float64).  sums (B, 2) fp32 =
 * (sum c^2, sum c) over the both-voiced pairs, c = 1200 log2(fx / fy) cents evaluated in float64 and rounded once to fp32.
 * Summation order: thread tid of 256 adds its entries p = tid, tid + 256, ... in ascending p (c^2 by fmaf) into fp32 partials; the 64
 * partials of a wave combine by the xor butterfly (lane offsets 32, 16, 8, 4, 2, 1), the four wave sums as (w0 + w1) + (w2 + w3):
 * bitwise repeatable.  path_len 0 gives zeros.  One launch, one workgroup per pair.  Limits (-22): B, Tx, Ty, P >= 1, strides >= 0. */
int st_f0_path_scores(const float* f0_x, long x_sb, int Tx, const float* f0_y, long y_sb, int Ty,
                      const int32_t* path /* (B, P, 2) */, const int32_t* path_len /* (B) */, int B, int P,
                      int32_t* counts /* (B, 4) */, float* sums /* (B, 2) */, void* stream);

/* ------------------------------------------------------------------ silence trimming (waveforms -> sample bounds, non-silent intervals)
 * Not a step of the reference (it leaves trimming to an offline tool).  The definition is that of librosa.effects.trim / split with
 * ref = max, center = True and zero padding, on the RAW waveform of a ragged batch (st_wave_batch, B <= 64).
 * Frames.  Utterance b with L = len[b] samples x[0 .. L) has the frames t = 0 .. T - 1, T = 1 + L / hop.  Frame t reads the
 * frame_length samples x[t hop - frame_length / 2 + j], j < frame_length (integer division), with x[i] = 0 for i outside [0, L) --
 * never a neighbouring utterance's samples of the packed buffer.
 * Energy.  energy[b, t] = (sum_j x^2) / frame_length in fp32; rows t >= T up to T_pad are written 0.  Summation order: with
 * j = 64 q + l, lane l < 64 forms ONE chain acc = fmaf(x, x, acc) over its j in ascending q; the 64 partials combine by the xor
 * butterfly (lane offsets 32, 16, 8, 4, 2, 1); the quotient by frame_length is one correctly rounded division.  A frame's bits depend
 * on its utterance's samples and the framing alone: not on B, the position in the batch, T_pad or what lies next to the utterance.
 * A NaN or an infinity among the samples makes exactly the frames that read it NaN / inf (IEEE), as in the pitch tracker above.
 * Decision.  e_t = max(energy_t, 1e-10f), ref = max_t e_t; frame t is non-silent iff e_t > ref * ratio (one fp32 product, a strict
 * comparison), ratio = 10^(-top_db / 10) computed in double by the caller and rounded once.  0 < ratio < 1, so the loudest frame is
 * always non-silent and digital silence is kept whole.  (Should the product round up to ref itself -- a ratio within 2^-23 of 1 --
 * the frames with e_t = ref count as non-silent, as they would with the exact product.)
 * bounds[b] = (start, end, n_nonsilent, flags): with f0 / f1 the first / last non-silent frame, start = max(0, f0 hop - pad),
 * end = min(L, (f1 + 1) hop + pad).  An utterance with any non-finite energy gets (0, L, -1, 1) and n_iv = 0, every interval entry
 * -1; the other utterances of the batch are unaffected.
 * intervals (when not NULL): the maximal runs of non-silent frames [fa, fb] as (fa hop, min(L, (fb + 1) hop)), ascending, pad NOT
 * applied; n_iv[b] (when not NULL) the true number of runs, even above max_iv; entries past min(n_iv, max_iv) are written -1.
 * Two launches (energies: a workgroup stages the span of a run of consecutive frames in LDS once; decision: one workgroup per
 * utterance), no atomics, no workspace beyond `energy`, no host read: bitwise repeatable.
 * Limits (-22 past them, before any device call): 1 <= B <= 64, every len >= 1, 1 <= hop <= frame_length <= 8192, T_pad >= the
 * largest T, 0 < ratio < 1 (finite), pad >= 0, max_iv >= 0 and max_iv == 0 exactly when intervals is NULL.
 * st_trim_run_length: the consecutive frames one workgroup takes from one staged span at this framing (16, fewer when
 * 15 hop + frame_length would pass 12288 samples; 0 outside the limits) -- for tests that straddle it. */
int st_trim_run_length(int frame_length, int hop);
int st_trim_silence(const st_wave_batch* w, int frame_length, int hop, float ratio, int pad, int max_iv,
                    float* energy /* (B, T_pad) */, int T_pad, int32_t* bounds /* (B, 4) */,
                    int32_t* intervals /* (B, max_iv, 2) or NULL */, int32_t* n_iv /* (B) or NULL */, void* stream);

/* ------------------------------------------------------------------ transcript scoring (Levenshtein alignment with its trace-back)
 * Not a step of the reference (its cal_per returns a distance only).  hyp (B, N, Lh) int64 holds N >= 1 transcripts per utterance, already
 * collapsed (st_ctc_beam_search's paths), of hyp_len (B, N) tokens; ref (B, Lr) int64 of ref_len (B) tokens (NULL: all Lr).  Lengths
 * are clamped into [0, L] by the kernel.  The ignored ids (at most 64) are dropped from both sides wherever they sit, as in
 * st_hyp_edit_distance; r[0 .. n) is the filtered reference and h[0 .. m) the filtered hypothesis of pair p = b N + k.
 * Definition.  D(i, 0) = i, D(0, j) = j, D(i, j) = min(D(i-1, j-1) + [r_i != h_j], D(i-1, j) + 1, D(i, j-1) + 1).  The alignment is
 * the trace-back from (n, m): at (i, j) with i, j > 0 the diagonal if D(i-1, j-1) + [r_i != h_j] = D(i, j), else the deletion
 * (i-1, j) if D(i-1, j) + 1 = D(i, j), else the insertion (i, j-1); on the border the one move that exists.  This fixes one alignment.
 * counts[p] = (correct, substitutions, deletions, insertions): dist = S + D + I, n = C + S + D, m = C + S + I.  ali_len[p] =
 * C + S + D + I.  ali[p] (when not NULL): the aligned pairs in forward order as (reference token, hypothesis token), -1 for a gap
 * (tokens as their low 32 bits), (-1, -1) past ali_len.  confusion (when not NULL) is ADDED into, never zeroed: path k = 0 of each
 * utterance adds 1 to [r, h] for a correct or substituted pair, to [r, V] for a deletion and to [V, h] for an insertion; a pair
 * with a token outside [0, V) is aligned and counted like any other but touches no cell.  The additions are integer atomics, exact
 * in any order.  counts and ali depend on their pair alone and are bitwise repeatable.  An empty side gives all deletions or all
 * insertions (all zeros when both are empty).
 * ws: st_edit_align_workspace_bytes(B N, Lr, Lh) bytes, no initialisation needed -- 0 (ws may be NULL) when the 2-bit moves of a
 * pair fit the LDS of a CU beside its tokens (Lh <= 256, or Lr <= 563 at Lh = 1024).
 * One launch, one wave per pair, no host read.  Limits (-22 past them, before anything is launched): B, N >= 1,
 * 1 <= Lh, Lr <= 1024, 1 <= V <= 1024, 0 <= n_ignore <= 64. */
size_t st_edit_align_workspace_bytes(int pairs, int Lr, int Lh);
int st_edit_align(const int64_t* hyp /* (B, N, Lh) */, const int32_t* hyp_len /* (B, N) */, int B, int N, int Lh,
                  const int64_t* ref /* (B, Lr) */, const int32_t* ref_len /* (B) or NULL */, int Lr, const int32_t* ignore, int n_ignore,
                  int V, int32_t* counts /* (B, N, 4) */, int32_t* ali_len /* (B, N) */, int32_t* ali /* (B, N, Lr + Lh, 2) or NULL */,
                  int32_t* confusion /* (V + 1, V + 1) or NULL */, void* ws, void* stream);

/* ------------------------------------------------------------------ loudness (ITU-R BS.1770-4 / EBU R 128 integrated loudness, gain)
 * Not a step of the reference (its features are absolute levels: a quieter recording is a different input).  Mono, channel 0, the RAW
 * waveform (no pre-emphasis) of a ragged batch (st_wave_batch, B <= 64).  Utterance b is x[0 .. L), L = len[b]; its filter state
 * starts at zero and it never sees a neighbouring utterance's samples of the packed buffer.  Out of scope: multichannel weighting,
 * true (oversampled) peak, loudness range (EBU Tech 3342) and short-term loudness.
 * K-weighting at the sample rate fs: two biquads, coefficients computed by the caller in float64.
 *   Stage 1 (shelf): f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *   Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b = (Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2) / a0,
 *   a = (1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0).
 *   Stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0 formulas; b = (1, -2, 1) exactly,
 *   a = (1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0).
 *   At fs = 48000 these are the standard's table to its 14 printed digits.  A 0 dBFS 997 Hz sine reads -3.0103 LKFS there and -2.970
 *   at 16 kHz (the bilinear warp).
 * Hops and blocks.  hop = (fs + 5) / 10 samples (integer division, 100 ms); H = L / hop full hops, the tail is not metered.
 * e[h] = sum of y^2 over hop h of the filtered signal y.  Block j = 0 .. H - 4: z_j = (e[j] + e[j+1] + e[j+2] + e[j+3]) / (4 hop),
 * l_j = -0.691 + 10 log10 z_j.
 * Gating.  A = { j : l_j > -70 }; Gr = -0.691 + 10 log10(mean of z over A) - 10; R = { j in A : l_j > Gr }; the integrated loudness
 * L_I = -0.691 + 10 log10(mean of z over R).  Both comparisons are strict.
 * Arithmetic.  The recurrence, its carry across threads and hops and the sums of squares are float64 on the device; e[h] is rounded
 * once to fp32 into hop_energy, and blocks, gates and statistics are formed in float64 FROM those fp32 values, each result rounded once.
 * Outputs.  hop_energy (B, H_pad): e[h], rows h >= H written 0.
 *   stats (B, 8) fp32: 0 L_I; 1 max_j l_j (momentary maximum); 2 Gr; 3 the sample peak max |x| over all L samples, tail included;
 *   4 the ungated loudness over all blocks; 5 the gain g; 6, 7 zero.
 *   counts (B, 4) int32: (max(H - 3, 0), |A|, |R|, flags).
 *   flags: 1 a non-finite sample -- slots 0 .. 4 NaN, g = 1, |A| = |R| = 0, hop_energy NaN from the hop that holds it on (IEEE), the
 *   other utterances untouched; 2 H < 4, no block -- slots 0, 1, 2, 4 NaN, g = 1; 4 A is empty -- L_I = Gr = -inf, g = 1;
 *   8 the gain is limited by the peak ceiling; 16 the gain is limited by max_gain_db (of 8 and 16 the one that binds; 8 on a tie).
 * Gain.  g = min(10^((target - L_I) / 20), 10^(peak_db / 20) / peak, 10^(max_gain_db / 20)) in float64 on the device, rounded once.
 * target NaN: measure only, g = 1 and neither 8 nor 16.
 * tables: ST_LOUDNESS_TABLE_DOUBLES float64 values on the device, with r = st_loudness_run_length(fs), pad = 256 r - hop and A the 4 x 4
 * state matrix of the cascade in DF2-transposed form, state (shelf s1, shelf s2, high-pass s1, high-pass s2), matrices row-major:
 *   [0, 8) b0 b1 b2 a1 a2 of stage 1, a1 a2 of stage 2, 0;  [8, 136) A^(r 2^k), k < 8;  [136, 152) A^hop;
 *   [152, 152 + 256 * 16) A^max(0, t r - pad), t < 256.
 * ws: B (H_pad + 1) 9 doubles, no initialisation needed.
 * Four launches (run end states and peaks; the carry over the hops, one wave per utterance; hop energies; gating and gain, one
 * workgroup per utterance), no atomics, no host read: every output depends on its utterance's samples, fs and the three gain arguments
 * alone -- not on B, the position in the batch, H_pad or the neighbours -- and is bitwise repeatable.
 * Limits (-22 past them, before any device call): 1 <= B <= 64, every len >= 1, 8000 <= fs <= 48000, H_pad >= the largest H, finite
 * peak_db and max_gain_db, target finite or NaN.
 * st_loudness_run_length: the samples r = ceil(hop / 256) one thread owns at this rate (4 .. 19; 0 outside the limits) -- for tests
 * that straddle it.
 * st_wave_gain: out[off[b] + i] = x[off[b] + i] * g_b, ONE fp32 product, g_b = stats[8 b + 5] read on the device (no host read between
 * the meter and the gain).  out_f32 (n_samples floats, packed as x) may be x itself; out_i16 (n_samples int16, packed as x) is
 * rint(clip((double)(x g), -1, 1) * 32767), a 16-bit .wav writer's formula.  Either may be NULL, not both.  Samples of the buffers
 * outside the utterances are not touched.  Limits as above (B, len). */
#define ST_LOUDNESS_TABLE_DOUBLES (152 + 256 * 16)
int st_loudness_run_length(int fs);
int st_loudness_batch(const st_wave_batch* w, int fs, const double* tables, double target, double peak_db, double max_gain_db,
                      float* hop_energy /* (B, H_pad) */, int H_pad, float* stats /* (B, 8) */, int32_t* counts /* (B, 4) */,
                      double* ws, void* stream);
int st_wave_gain(const st_wave_batch* w, const float* stats /* (B, 8) */, float* out_f32, int16_t* out_i16, void* stream);

/* ------------------------------------------------------------------ ABX phone discrimination: pairwise DTW of short items, triple counts
 * Not a step of the reference (it scores no representation); the measure of ZeroSpeech / Libri-light (semi_tts_amd.metrics.abx,
 * main.py --abx-ali-dir).
 * st_dtw_pairs: the path-normalised DTW distance of P pairs of items of one packed feature buffer.  feat(r, k) = feat[r st + k], n_rows
 * rows of D columns, row stride st >= D floats.  Item q is the rows [item_start[q], item_start[q] + item_len[q]) (device int32, n_items
 * entries); pair p is item a = pair_a[p] (n rows) against item b = pair_b[p] (m rows) (device int32, P entries).
 * Frame distance d(i, j) of row i of a (x) and row j of b (y), fp32, sums over ascending k (fma contraction not specified):
 *   ST_ABX_EUCLID   sqrtf(sum_k (x_k - y_k)^2) -- st_dtw_batch's distance at scale 1.
 *   ST_ABX_ANGULAR  u = x / ||x|| (x times the rounded reciprocal of sqrtf(sum x_k^2), one reciprocal a row; a zero row stays zero),
 *                   d = (2 / pi) atan2f(||u - v||, ||u + v||), in [0, 1]: the angle, in the form that keeps its digits for near-parallel
 *                   frames (acos of an fp32 cosine loses half of them there).  A zero row is at 0.5 from a non-zero row, at 0 from a zero row.
 *   ST_ABX_KL       0.5 sum_k (x_k - y_k) (logf(x_k + 1e-10) - logf(y_k + 1e-10)), the symmetrised KL divergence of two probability
 *                   rows with the project's log(p + 1e-10); a negative entry makes the pair NaN.
 * Recurrence and ties as st_dtw_batch: D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), ONE fp32 add; the diagonal wins, then
 * (i-1, j), then (i, j-1) (a candidate replaces the best only when strictly smaller).  The path length is carried beside the cost:
 * L(0, 0) = 1, L(i, j) = L(chosen predecessor) + 1 -- the length of the path a trace-back would find; no back-pointers exist.
 * Outputs: cost (P) = D(n-1, m-1) and path_len (P) = L(n-1, m-1) (either may be NULL); dist (P) = cost / (float)path_len, one correctly
 * rounded fp32 division (the DTW of ABXpy / Libri-light's ABX evaluation).
 * Without raising, dist and cost NaN and path_len 0 for a pair with: an item index outside [0, n_items); an item_len outside
 * [1, max_len]; an item reaching outside [0, n_rows); a NaN among the rows of either item.  Nothing outside feat is read in any case.
 * A pair depends on its two items alone: bitwise repeatable, independent of P, of its position in the list, of the other pairs, of
 * max_len and of the rows that belong to neither item.  d(a, b) and d(b, a) have the same cost, but under exact ties they may differ in
 * path_len (the rule prefers (i-1, j) to (i, j-1), which swaps with the sides) and hence in dist.
 * Limits (-22 past them): P >= 1, n_items >= 1, n_rows >= 1, 1 <= D <= 512, 1 <= max_len <= 64, metric one of the three, st >= D.
 * One launch (the waves stride over the pairs when P passes one grid), no workspace, no atomics, no host read. */
#define ST_ABX_EUCLID 0
#define ST_ABX_ANGULAR 1
#define ST_ABX_KL 2
int st_dtw_pairs(const float* feat, long n_rows, int D, long st, const int32_t* item_start, const int32_t* item_len, int n_items,
                 const int32_t* pair_a, const int32_t* pair_b, int P, int metric, int max_len,
                 float* dist /* (P) */, float* cost /* (P) or NULL */, int32_t* path_len /* (P) or NULL */, void* stream);

/* st_abx_count: ABX triple counts from finished distances.  dmat: dmat_len floats, the dense symmetric (n_c, n_c) matrices of the
 * cells laid end to end (the diagonal is never read).  blk (NB, 6) int64 on the device: (mat_off, n_c, a_lo, a_hi, b_lo, b_hi) -- the
 * matrix of the block's cell starts at dmat[mat_off]; classes a and b are the local index ranges [a_lo, a_hi) and [b_lo, b_hi), clamped
 * into [0, n_c] (an inverted range is empty).  count (NB, 4) int64 = (wrong, tied, nan, triples) over all X, A in a with A != X (by
 * index) and all B in b: nan = the triples with a NaN in d(A, X) or d(B, X), counted nowhere else; wrong = #{d(A, X) > d(B, X)};
 * tied = #{d(A, X) == d(B, X)}; triples = n_a (n_a - 1) n_b.  d(., X) is read from row X of the matrix.
 * A block whose matrix does not lie inside dmat (mat_off < 0, n_c < 0 or above 2^20, mat_off + n_c^2 > dmat_len) reads nothing and
 * gets -1 in all four columns.  Integer sums, no atomics: exact and repeatable.  One launch, one workgroup a block (blocks with more
 * triples than threads are strided over).  Limits (-22): NB >= 1, dmat_len >= 1. */
int st_abx_count(const float* dmat, long dmat_len, const int64_t* blk /* (NB, 6) */, int NB, int64_t* count /* (NB, 4) */, void* stream);

/* st_abx_across: across-speaker ABX from finished distances -- A and B of one speaker, X of another (Libri-light's second figure).
 * dmat as for st_abx_count, one dense (n_c, n_c) matrix per CONTEXT whose items are ordered by (speaker, label, index), so a
 * (speaker, label) run is an index range; entries between items of one speaker are never read.
 * grp (NG, 8) int64 on the device: (mat_off, n_c, a_lo, a_hi, b_lo, b_hi, xr_lo, xr_hi) -- A runs over [a_lo, a_hi), B over
 * [b_lo, b_hi) (same speaker, another label), and xr[xr_lo .. xr_hi) of xr (NX, 2) int64 are the ranges (x_lo, x_hi) of label a for the
 * speakers of the context in ascending speaker order, a list all groups of one (context, a) share.  All ranges are clamped into
 * [0, n_c] and an inverted range is empty; the entry that equals (a_lo, a_hi) after clamping is the group's own speaker and is skipped.
 * Per X range: the triples (A, B, X), n_a n_b n_x of them; wrong = d(A, X) > d(B, X), tied = ==, nan = either is NaN (counted nowhere
 * else), d(., X) read from row X; pair score = (wrong + tied / 2) / (triples - nan) in float64, absent when nothing is left.
 * err (NG) float64 = the mean of the present pair scores: their sum taken sequentially in list order, one division by their number;
 * NaN without one.  count (NG, 5) int64 = (wrong, tied, nan, triples, x_speakers): the first four summed over all ranges but the
 * group's own, x_speakers the number of present pair scores.
 * A group whose matrix does not lie inside dmat (as for st_abx_count) or whose xr_lo or xr_hi lies outside [0, NX] reads nothing and
 * gets -1 in all five columns and NaN; xr_hi <= xr_lo is an empty list.  Integer partial sums, no atomics, a fixed order: bitwise
 * repeatable and independent of NG, of the group's position and of the other groups.  One launch, one wave a group (groups wider
 * than a wave are strided over), no workspace, no host read.  Limits (-22): NG >= 1, dmat_len >= 1, NX >= 1, no null pointer; n_c as
 * for st_abx_count. */
int st_abx_across(const float* dmat, long dmat_len, const int64_t* grp /* (NG, 8) */, int NG, const int64_t* xr /* (NX, 2) */, long NX,
                  double* err /* (NG) */, int64_t* count /* (NG, 5) */, void* stream);

/* ------------------------------------------------------------------ intelligibility: STOI and ESTOI of (clean, processed) waveform pairs
 * Not a step of the reference (it scores no waveform).  STOI: Taal, Hendriks, Heusdens, Jensen 2011; ESTOI: Jensen, Taal 2016
 * (semi_tts_amd.metrics.stoi, main.py --stoi-wav-dir).  Both signals of a pair are at 10 kHz, time-aligned and of one length: x is a
 * ragged batch (st_wave_batch, 0 <= B <= 64) of clean signals, y a second packed buffer with the SAME offsets and lengths that holds
 * the processed ones.  A pair never sees a neighbour's samples of the packed buffers.
 * Window.  w[n] = 0.5 - 0.5 cos(2 pi (n + 1) / 257), n < 256 (hanning(258) without its two zeros), computed in double, rounded once.
 * Frames.  Frame i starts at 128 i for every i with 128 i < L - 256 (strict, as the authors' code): F = st_stoi_frames(L) of them,
 * 0 when L <= 256.
 * Silent frames.  energy[b, i] = ||w x_i||_2 in fp32 (rows i >= F up to F_pad written 0): the products w[j] x[j] are rounded, lane
 * l < 64 forms ONE chain acc = fmaf(v, v, acc) over j = l, l + 64, l + 128, l + 192, the 64 partials combine by the xor butterfly
 * (offsets 32 .. 1) and the root is one sqrtf.  Frame i is kept iff e_i + EPS > 0.01f (max_i e_i + EPS) with EPS = 2^-52: the 40 dB
 * range below the loudest frame of 20 log10(e + EPS), without the logarithm; one fp32 product, a strict comparison.  The clean signal
 * alone decides.  kept[b, k], k < K, are the kept frame indices in ascending order; entries k >= K up to F_pad are -1.
 * Bands.  The kept windowed frames of each side, overlap-added at hop 128 in kept order, give (K - 1) 128 + 256 samples; that signal
 * is framed by the same rule (M = K - 1 frames: the strict bound drops the last one), windowed again, zero-padded to 512 and
 * transformed.  It is never written to memory: output frame m is gathered from the kept frames m - 1, m, m + 1.  Band j < 15 is
 * sqrtf of the sum of |X[k]|^2 over the bins [lo_j, hi_j) nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid k 10000 / 512:
 * (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219).
 * bands[b, side, j, m] (side 0 clean, 1 processed); columns m >= M up to F_pad are written 0.
 * Segments.  Segment s = 0 .. M - 30 holds the columns [s, s + 30) of both sides; S = M - 29 of them, 0 when M < 30.
 * STOI.  Per segment and band, with x, y the two rows: c = ||x|| / (||y|| + EPS), y' = min(c y, (1 + 10^(15 / 20)) x) (a NaN stays a
 * NaN); both rows minus their means, each divided by (its norm + EPS); d = the sum of the products over all bands and segments / (15 S).
 * ESTOI.  Per segment the rows of x and of y minus their means and divided by (norm + EPS), then the columns likewise;
 * d_e = the sum of the products / (30 S).  Both correlations are formed in float64 on the device from the fp32 bands, the segments
 * are summed in a fixed order and each score is rounded once.
 * Outputs.  score (B, 2) = (d, d_e); counts (B, 4) int32 = (F, K, M, S).  S = 0 (too short, or too few kept frames): both scores are
 * the sentinel 1e-5f.  A non-finite frame norm of the clean signal: K = M = S = 0, every kept entry -1, both scores NaN.  A non-finite
 * sample of y inside a kept frame makes both scores NaN through the arithmetic.  Digital silence on either side scores 0.
 * energy, kept, bands: each may be NULL (the workspace holds it then).
 * ws: st_stoi_workspace_floats(B, F_pad) floats, 8-byte aligned, no initialisation needed.
 * Five launches (frame norms: a workgroup stages the span of 16 consecutive frames in LDS once; selection: one workgroup per pair,
 * a block scan over chunks of 256 frames; bands: one wave per (output frame, side, pair); correlations: one wave per (pair, segment);
 * the sum over segments: one wave per pair), three when F_pad <= 30, none when B = 0.  No atomics, no allocation, no host read: every
 * output of a pair depends on its samples alone -- not on B, the position in the batch, F_pad or the neighbours -- and is bitwise
 * repeatable.  The first call on a device uploads the twiddle and window tables and may not be inside a stream capture.
 * Limits (-22 past them, before any device call): 0 <= B <= 64, 1 <= len <= 2^22 = 4194304, F_pad >= max(1, the largest F).
 * st_stoi_frames: F of a signal of len samples (-1 outside the limits). */
int st_stoi_frames(int len);
size_t st_stoi_workspace_floats(int B, int F_pad);
int st_stoi_batch(const st_wave_batch* x, const float* y, float* score /* (B, 2) */, int32_t* counts /* (B, 4) */, int F_pad,
                  float* energy /* (B, F_pad) or NULL */, int32_t* kept /* (B, F_pad) or NULL */,
                  float* bands /* (B, 2, 15, F_pad) or NULL */, float* ws, void* stream);

/* ------------------------------------------------------------------ waveform alignment: integer-delay search, SI-SDR / SNR, span copy
 * Not a step of the reference.  What lets st_stoi_batch score pairs that are shifted against each other (semi_tts_amd.metrics.delay,
 * si_sdr, align_pairs; main.py --stoi-align, --stoi-sdr).  x is a ragged batch of references, y a SECOND st_wave_batch of processed
 * signals with its own buffer, offsets and lengths; B is the same on both sides, Lx = x->len[b] and Ly = y->len[b] may differ.  A pair
 * never sees a neighbour's samples of the packed buffers.
 * st_xcorr_delay.  For pair b and every lag d in [-D, D], D = max_lag:
 *   r[b, d] = sum over n of x[n] y[n + d],  max(0, -d) <= n < min(Lx, Ly - d)   (0 for an empty range)
 * the plain cross-correlation in its direct form: not normalised per lag, not GCC-PHAT, no FFT.  A positive d: y is late by d samples.
 * Each product is (double)x * (double)y, which is exact (24 + 24 bits), and the products are accumulated in float64.  The samples of x
 * are cut into chunks of 1024 m samples, m = ceil(Lx / 32768) (at most 32 chunks); a lag's chunk sum is ONE chain of fma over ascending
 * n, and the chunk sums are added in ascending order.  The cut depends on the pair's own Lx alone.  On input that is a multiple of 2^-15
 * with magnitude at most 1 (16-bit PCM / 32768) every product is a multiple of 2^-30 and a sum of 2^22 of them stays below 2^53 units:
 * r is then EXACT, whatever the order.
 * Outputs.  delay (B) int32: the lag of the largest r; ties go to the smallest |d|, then to the non-negative one (the order 0, +1, -1,
 * +2, -2, ...); the argmax by that rule also when every r is 0 or negative.  coef (B) float32 = r[d*] / sqrt(sum x^2 * sum y^2), the
 * sums over the whole signals in float64 (fma chains, a fixed order; exact on PCM input), the quotient rounded once; 0 / 0 is NaN.
 * corr (B, 2 D + 1) float64 or NULL: the whole r, column d + D.  If any r[b, d] is NaN, delay[b] = 0 and coef[b] = NaN.
 * ws: st_xcorr_workspace_bytes(B, max_len, D) bytes (max_len: the longest signal of either side), 8-byte aligned, no initialisation
 * needed: B * min(32, ceil(max_len / 1024)) * (2 D + 1) float64.
 * Two launches (partials: grid (tiles of 2048 lags, chunks, pairs), a piece of 1024 samples of x and the span of y it meets staged
 * in LDS as float64, a register tile of 8 lags x 8 samples a thread; finish: one workgroup per pair), none when B = 0.
 * st_sisdr_batch.  delay: a DEVICE int32 (B) or NULL for 0 (it is not read on the host: any value is taken).  The scored span of pair
 * b is the overlap the delay d leaves: d >= 0: x from 0, y from d; d < 0: x from -d, y from 0; n = min(Lx - x0, Ly - y0) samples.
 * sums (B, 6) float64 = (n, sum x, sum y, sum x^2, sum y^2, sum x y) over the span, float64 sums of exact terms in a fixed order
 * (chunks of 8192 samples, then the chunks): exact on PCM input.  score (B, 3) float32 = (SI-SDR dB, SNR dB, gain dB), evaluated on the
 * device in float64 from the sums, every operation rounded on its own (no contraction), each figure rounded once:
 *   zero_mean != 0: Cxx = Sxx - (Sx Sx) / n, Cyy = Syy - (Sy Sy) / n, Cxy = Sxy - (Sx Sy) / n;  zero_mean == 0: C = S
 *   si_sdr = 10 log10((Cxy Cxy) / (Cxx Cyy - Cxy Cxy))            (Le Roux, Wisdom, Erdogan, Hershey 2019)
 *   snr    = 10 log10(Cxx / ((Cxx - 2 Cxy) + Cyy))
 *   gain   = 20 log10 |Cxy / Cxx|
 * IEEE semantics are kept: y = a x with zero_mean = 0 gives +inf; a silent reference gives NaN (0 / 0) in SI-SDR and gain and -inf
 * (log10 0) in SNR.  n <= 0 (the delay is longer than a side):
 * the three scores are NaN and the six sums 0.
 * ws: st_sisdr_workspace_bytes(B, max_len) bytes, 8-byte aligned.  Two launches (chunk partials; one wave per pair), none when B = 0.
 * st_wave_gather.  dst[dst_off[b] + i] = src[src_off[b] + i], i < len[b], for B spans in ONE launch (src_off, dst_off, len: host
 * arrays, as st_wave_batch's); nothing else of dst is written.  src and dst are different buffers.  It gives the two overlaps an
 * alignment leaves, which start at different places of their buffers, the one common layout st_stoi_batch requires.
 * No atomics, no allocation, no host read anywhere: every output of a pair depends on its own samples, lengths and D alone -- not on
 * B, the position in the batch or the neighbours -- and is bitwise repeatable.
 * Limits (-22 past them, before any device call): 0 <= B <= 64, 1 <= len <= 2^22 = 4194304 on both sides, 0 <= max_lag <= 16384
 * (+-0.34 s at 48 kHz), every span inside its buffer.  The workspace functions return 0 outside the limits. */
size_t st_xcorr_workspace_bytes(int B, int max_len, int max_lag);
int st_xcorr_delay(const st_wave_batch* x, const st_wave_batch* y, int max_lag, int32_t* delay /* (B) */, float* coef /* (B) */,
                   double* corr /* (B, 2 max_lag + 1) or NULL */, void* ws, void* stream);
size_t st_sisdr_workspace_bytes(int B, int max_len);
int st_sisdr_batch(const st_wave_batch* x, const st_wave_batch* y, const int32_t* delay /* device (B) or NULL */, int zero_mean,
                   double* sums /* (B, 6) */, float* score /* (B, 3) */, void* ws, void* stream);
int st_wave_gather(const float* src, long src_n, const long* src_off, float* dst, long dst_n, const long* dst_off, const int* len, int B,
                   void* stream);

/* ------------------------------------------------------------------ k-means over frame features: units without transcripts or a codebook
 * Not a step of the reference (it clusters nothing); the discrete-unit baseline of ZeroSpeech / HuBERT (semi_tts_amd.kmeans,
 * main.py --kmeans-wav-dir, --units-wav-dir, --abx-codebook).  One operand struct for every call: N rows of D columns, row n at
 * x + n ld, ld >= D floats, so a column slice of a wider buffer is taken as it is.  cent is a contiguous (K, D) table.
 * Limits of every entry point (-22 past them, before any launch): 1 <= D <= 256, 1 <= K <= 4096, 1 <= N, N ld < 2^40, no null pointer.
 *
 * st_kmeans_assign: idx[n] (int32) = the smallest k that attains the minimum over k of d(n, k), dist[n] = that minimum, with
 *   d(n, k) = max(0, (|x_n|^2 + |c_k|^2) - 2 x_n.c_k) in fp32 -- the expanded form: the three sums are fmaf chains over ascending d,
 *   the sum of the two norms is one rounded add, the last step one fmaf.  Exact whenever every intermediate is (small integers); else
 *   |d - ||x - c||^2| <= (D + 3) 2^-24 (||x|| + ||c||)^2 to first order, which loses digits when a column's mean dwarfs its spread.
 *   The centroids are visited in ascending k and a later one wins only when strictly smaller.  A row holding a NaN or an infinity (or whose |x|^2
 *   overflows fp32) gets idx = -1 and dist = NaN.  One launch, no workspace, no atomics: a row's result depends on that row and the table alone.
 *
 * st_kmeans_update: cent_out, count and stats from an assignment.  A point with idx outside [0, K) (the -1 of a NaN row) is no
 *   member.  count[k] (int32) = the members of k; cent_out[k, d] = (float)(S / (double)count[k]) with S the float64 sum of the members'
 *   x[n, d], or cent_in[k, d] when count[k] = 0.  stats (4 doubles) = (sum of dist over the members; sum over k, d of
 *   (cent_out - cent_in)^2 in float64; clusters with count 0; points that are no member).
 *   Order of every sum, a function of (N, K, idx) alone: a cluster's members in ascending n are cut into slabs of 256; a slab is summed
 *   from 0 in that order; the slabs are added in ascending order.  dist: per chunk of 1024 points, thread t of 256 adds its points
 *   t, t + 256, .. in that order and a binary tree over the threads (t with t + s, s = 128 .. 1) joins them; the chunks and the per-cluster
 *   shifts (each the sum over ascending d) are joined alike over 1024 threads.  No floating-point atomics; integer atomics only for
 *   the LDS histograms, whose result does not depend on their order: two runs give the same bits.
 *   ws: st_kmeans_update_workspace_bytes(N, D, K) bytes (0 outside the limits), 16-byte aligned.  Seven launches, no host read.
 *
 * st_kmeans_relocate: the e-th cluster with count[k] = 0 (ascending k) takes the row of the e-th member point in the order (dist
 *   descending, n ascending); with fewer member points than such clusters the rest of cent is left alone.  cent (K, D) is changed in
 *   place; the donors' clusters are not adjusted.  One launch of one workgroup, a pass over the points per empty cluster: the rare path.
 *
 * st_kmeans_pp_step / st_kmeans_pp_pick: k-means++ (Arthur, Vassilvitskii 2007) without a host read between the picks.  Device state:
 *   mind (N) float32, filled with +inf by the caller; part (st_kmeans_chunks(N)) doubles; picks (K) int32; totals (K) doubles; flag (1)
 *   int32, zeroed by the caller; u (K) doubles in [0, 1).  The caller issues pick(0), step(0), pick(1), step(1), .., pick(K-1), step(K-1).
 *   step(j): p = picks[j]; cent[j] = row p; mind[n] = min(mind[n], sum_d (x[n, d] - x[p, d])^2) (fp32, the direct form, an fmaf chain
 *     over ascending d: exactly 0 for a copy of row p), NaN for a row holding one; part[c] = the sum of the weights of chunk c of 1024
 *     points, a point's weight being mind where mind > 0 and 0 elsewhere (float64, the tree of st_kmeans_update's dist).
 *   pick(0): picks[0] = floor(u[0] N).  pick(j): total = the sum of part; cum = the float64 running sum of the weights over ascending
 *     n (the chunks before a point's own taken from part); picks[j] = the first n whose weight is positive and cum[n] > u[j] total, or
 *     the last n of positive weight when rounding leaves none; totals[j] = total.  total = 0 (fewer distinct rows than centres) sets
 *     flag[0] = 1 and picks[j] = 0; the caller reads the flag once at the end.  On integer data every sum is exact and the picks are
 *     those of a sequential float64 scan.  One launch each. */
typedef struct st_kmeans_data { const float* x; long ld; int N; int D; } st_kmeans_data;
int st_kmeans_assign(const st_kmeans_data* x, const float* cent /* (K, D) */, int K, int32_t* idx /* (N) */, float* dist /* (N) */, void* stream);
size_t st_kmeans_update_workspace_bytes(int N, int D, int K);
int st_kmeans_update(const st_kmeans_data* x, const int32_t* idx, const float* dist, const float* cent_in, int K, float* cent_out /* (K, D) */,
                     int32_t* count /* (K) */, double* stats /* (4) */, void* ws, void* stream);
int st_kmeans_relocate(const st_kmeans_data* x, const int32_t* idx, const float* dist, const int32_t* count, int K, float* cent /* (K, D) */,
                       void* stream);
long st_kmeans_chunks(int N);
int st_kmeans_pp_step(const st_kmeans_data* x, const int32_t* picks, int j, int K, float* mind, double* part, float* cent, void* stream);
int st_kmeans_pp_pick(const st_kmeans_data* x, const float* mind, const double* part, const double* u, int j, int K, int32_t* picks,
                      double* totals, int32_t* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMITTS_H */
