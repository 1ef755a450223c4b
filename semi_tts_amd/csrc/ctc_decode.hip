// ctc_decode.hip -- CTC prefix beam search (contract: st_ctc_beam_search in include/semitts.h).
//
// One workgroup of 256 threads per utterance; the beam lives in LDS, the prefix tree in the workspace.  Per frame:
//   1. log-probabilities of the frame into LDS (NaN anywhere -> the utterance's result is NaN, the loop stops);
//   2. the nb "stay" candidates, each with the one extension merged into it: B's parent prefix is in the beam at slot link(B), so
//      "A + c == B" holds exactly when link(B) == A and last(B) == c.  Those (A, c) extensions are masked in a W x V bitmap;
//   3. the nb new beam entries are the W best of the nb + nb (V - 1) candidates: an MSB-first radix select (8 bits a pass) on an
//      order-preserving integer key of the score finds the W-th key, a block scan compacts the winners in candidate order, a rank
//      sort over the <= W winners orders them by (score desc, candidate index asc);
//   4. the new entries' links: an extension of A points to A's new stay slot; a stay inherits its old parent's new stay slot.  A
//      stay whose parent was NOT in the old beam may find it among the new extensions: that is decided by comparing the two
//      prefixes symbol by symbol through the prefix tree (rare, and it stops at the first difference or the first common node).
// Every prefix that ever enters the beam as an extension gets a node (parent node, symbol) in the workspace; the N outputs are
// read back along those chains.  Only integer LDS atomics (histogram counts, bitmap bits), no float atomics: results are bitwise repeatable.
//
// LM fusion (st_ctc_beam_search_lm, the LM = true instantiation): every slot carries the row `ctx` of its n-gram context; an extension of
// slot s by c scores (.. + lp[c]) + bonus[ctx[s] V + c] in the three places an extension's score is formed (the merge of step 2, the keys
// of step 3, the new entry of step 4), always through ext_score(), so the three agree bit for bit.  The table is read through L2 where
// the score is formed: copying the nb live rows into LDS once a frame was built and measured, and was worth 1 % at most.
// LM = false compiles to the kernel without any of it.
#include <type_traits>
#include "st_common.h"

namespace {

constexpr int CB_NT = 256, CB_MAX_T = 4096, CB_MAX_V = 1024, CB_MIN_V = 2, CB_MAX_W = 128;
constexpr int CB_MASK_WORDS = CB_MAX_W * CB_MAX_V / 32;
constexpr int CB_MAX_ORDER = 4, CB_MAX_TABLE = 1 << 26;   // LM fusion: n-gram order, elements of the (V^(order-1), V) table

__device__ __forceinline__ float cb_lae(float a, float b) {     // log(exp a + exp b); -inf, -inf -> -inf
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (n == -INFINITY) return m;
    return m + log1pf(expf(n - m));
}

// a total order on non-NaN floats as unsigned integers (larger score -> larger key); -0 and +0 map to one key.  Every score's key is
// >= key(-inf) = 0x007fffff, so 0 marks "not a candidate" (a merged extension).
__device__ __forceinline__ unsigned cb_key(float s) {
    const unsigned u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inclusive/exclusive block scan of one int per thread; returns the exclusive prefix, *total = the block sum.  scr >= 4 ints.
__device__ __forceinline__ int cb_scan(int x, int* scr, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int s = x;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    if (lane == 63) scr[w] = s;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < CB_NT / 64; ++k) { if (k < w) off += scr[k]; tot += scr[k]; }
    __syncthreads();
    *total = tot;
    return off + s - x;
}

struct CbBeam {                  // one beam (double-buffered in LDS)
    float pb[CB_MAX_W], pnb[CB_MAX_W];
    int last[CB_MAX_W], link[CB_MAX_W], node[CB_MAX_W], len[CB_MAX_W];
};
struct CbBeamLm : CbBeam {       // with LM fusion: the table row of each prefix's context
    int ctx[CB_MAX_W];
};

// what the fused kernel takes on top (nothing for LM = false): bonus (ctx_mod, V) fp32, ctx_mod = V^(order-1); ctx0 the empty prefix's row
template <bool LM> struct CbLmArgs {};
template <> struct CbLmArgs<true> { const float* bonus; int ctx_mod, ctx0; };

template <bool LM>
__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(const float* __restrict__ prob, int T, int V, const int32_t* __restrict__ lengths,
                                                         int W, int N, int blank, int log_input, float eps, int64_t* __restrict__ hyp,
                                                         int32_t* __restrict__ hyp_len, float* __restrict__ score, int2* __restrict__ ws,
                                                         CbLmArgs<LM> lm) {
    using Beam = std::conditional_t<LM, CbBeamLm, CbBeam>;
    __shared__ Beam bm[2];
    __shared__ float lp[CB_MAX_V];
    __shared__ float tot[CB_MAX_W];                       // score of each slot of the current beam
    __shared__ float cpb[CB_MAX_W], cpnb[CB_MAX_W];       // stay candidates (merges included)
    __shared__ unsigned skey[CB_MAX_W];
    __shared__ unsigned mask[CB_MASK_WORDS];              // (slot, symbol) extensions merged into a stay
    __shared__ int hist[256];
    __shared__ int sel_idx[CB_MAX_W], order[CB_MAX_W], stay_slot[CB_MAX_W];
    __shared__ unsigned sel_key[CB_MAX_W];
    __shared__ int scr[CB_NT / 64];
    __shared__ int s_nan, s_digit, s_k;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = lengths ? min(max(lengths[b], 0), T) : T;   // (the host checks lengths it can see; the device clamps)
    int2* nodes = ws + (size_t)b * ((size_t)T * W + 1);   // node 0 = the empty prefix; frame t's new entries take 1 + t W + slot
    const int Vm = V - 1;
    if (tid == 0) {
        bm[0].pb[0] = 0.0f; bm[0].pnb[0] = -INFINITY;
        bm[0].last[0] = -1; bm[0].link[0] = -1; bm[0].node[0] = 0; bm[0].len[0] = 0;
        tot[0] = 0.0f;
        if constexpr (LM) bm[0].ctx[0] = lm.ctx0;
        s_nan = 0;
        nodes[0] = make_int2(-1, -1);
    }
    int nb = 1, cur = 0;
    __syncthreads();
    for (int t = 0; t < Tb; ++t) {
        Beam& o = bm[cur];
        Beam& n = bm[cur ^ 1];
        // ---- 1. the frame's log-probabilities
        const float* row = prob + ((size_t)b * T + t) * V;
        for (int v = tid; v < V; v += CB_NT) {
            const float x = row[v];
            const float l = log_input ? x : logf(x + eps);
            if (l != l) s_nan = 1;
            lp[v] = l;
        }
        for (int k = tid; k < (nb * V + 31) / 32; k += CB_NT) mask[k] = 0u;
        __syncthreads();
        if (s_nan) break;
        // the score of slot s extended by c; with LM one more fp32 addition, after lp[c]
        auto ext_score = [&](int s, int c) -> float {
            const float e = (c == o.last[s] ? o.pb[s] : tot[s]) + lp[c];
            if constexpr (LM) return e + lm.bonus[(size_t)o.ctx[s] * V + c];
            else return e;
        };
        // ---- 2. stays, with the merged extension A + last(B) of A = link(B)
        if (tid < nb) {
            const int s = tid, c = o.last[s], a = o.link[s];
            const float spb = tot[s] + lp[blank];
            float spnb = c >= 0 ? o.pnb[s] + lp[c] : -INFINITY;
            if (a >= 0) {
                spnb = cb_lae(spnb, ext_score(a, c));
                const int bit = a * V + c;
                atomicOr(&mask[bit >> 5], 1u << (bit & 31));
            }
            cpb[s] = spb; cpnb[s] = spnb;
            skey[s] = cb_key(cb_lae(spb, spnb));
            stay_slot[s] = -1;
        }
        __syncthreads();
        const int M = nb + nb * Vm;
        auto cand_key = [&](int i) -> unsigned {
            if (i < nb) return skey[i];
            const int j = i - nb, s = j / Vm, r = j - s * Vm, c = r < blank ? r : r + 1;
            const int bit = s * V + c;
            if (mask[bit >> 5] & (1u << (bit & 31))) return 0u;
            return cb_key(ext_score(s, c));
        };
        // ---- 3a. how many candidates are real (M minus the merged ones), then the W-th key by radix select
        int n_real;
        {
            int cnt = 0;
            for (int i = tid; i < M; i += CB_NT) cnt += cand_key(i) != 0u;
            cb_scan(cnt, scr, &n_real);
        }
        const int nb_new = min(W, n_real);
        unsigned thr = 1u;                                // keys > thr ... (all real ones when they all fit)
        int k_eq = 0x7fffffff;                            // ... and of the keys == thr, the first k_eq in candidate order
        if (n_real > W) {
            unsigned prefix = 0u, pmask = 0u;
            int k = nb_new;                               // rank (1-based) of the wanted key among those matching the prefix
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[tid] = 0;
                __syncthreads();
                for (int i = tid; i < M; i += CB_NT) {
                    const unsigned key = cand_key(i);
                    if (key != 0u && (key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
                }
                __syncthreads();
                // suffix sums over the digits, high digit first: thread d holds digit 255 - d
                const int h = hist[255 - tid];
                int above_total;
                const int above = cb_scan(h, scr, &above_total);          // keys with a larger digit
                if (above < k && above + h >= k) { s_digit = 255 - tid; s_k = k - above; }
                __syncthreads();
                prefix |= (unsigned)s_digit << shift;
                pmask |= 255u << shift;
                k = s_k;
            }
            thr = prefix;
            k_eq = k;
        }
        // ---- 3b. compaction in candidate order: thread tid takes the contiguous indices [i0, i1)
        {
            const int ch = (M + CB_NT - 1) / CB_NT, i0 = min(M, tid * ch), i1 = min(M, i0 + ch);
            int gt = 0, eq = 0;
            for (int i = i0; i < i1; ++i) {
                const unsigned key = cand_key(i);
                gt += key > thr;
                eq += key == thr;
            }
            int n_gt, n_eq;
            const int gt_before = cb_scan(gt, scr, &n_gt);
            int eq_before = cb_scan(eq, scr, &n_eq);
            int pos = gt_before + min(eq_before, k_eq);
            for (int i = i0; i < i1; ++i) {
                const unsigned key = cand_key(i);
                if (key > thr || (key == thr && eq_before++ < k_eq)) { sel_idx[pos] = i; sel_key[pos] = key; ++pos; }
            }
        }
        __syncthreads();
        // ---- 3c. order the survivors: score descending, candidate index ascending
        if (tid < nb_new) {
            const unsigned ki = sel_key[tid];
            const int ii = sel_idx[tid];
            int rank = 0;
            for (int j = 0; j < nb_new; ++j) {
                const unsigned kj = sel_key[j];
                rank += kj > ki || (kj == ki && sel_idx[j] < ii);
            }
            order[rank] = ii;
        }
        __syncthreads();
        // ---- 4. the new beam
        if (tid < nb_new) {
            const int r = tid, i = order[r];
            if (i < nb) {
                n.pb[r] = cpb[i]; n.pnb[r] = cpnb[i];
                n.last[r] = o.last[i]; n.node[r] = o.node[i]; n.len[r] = o.len[i];
                if constexpr (LM) n.ctx[r] = o.ctx[i];
                stay_slot[i] = r;
            } else {
                const int j = i - nb, s = j / Vm, rr = j - s * Vm, c = rr < blank ? rr : rr + 1;
                const int id = 1 + t * W + r;
                n.pb[r] = -INFINITY;
                n.pnb[r] = ext_score(s, c);
                n.last[r] = c; n.len[r] = o.len[s] + 1; n.node[r] = id;
                if constexpr (LM) n.ctx[r] = (o.ctx[s] * V + c) % lm.ctx_mod;       // (< V^order <= 2^26: no overflow; order 1: always 0)
                nodes[id] = make_int2(o.node[s], c);
            }
        }
        __syncthreads();
        if (tid < nb_new) {
            const int r = tid, i = order[r];
            if (i < nb) n.link[r] = o.link[i] >= 0 ? stay_slot[o.link[i]] : -1;
            else n.link[r] = stay_slot[(i - nb) / Vm];
        }
        __syncthreads();
        // a stay B whose parent was not in the old beam: is the parent one of the new extensions E?  (len(E) == len(B) - 1 and
        // last(E) == the symbol before last(B), then the exact comparison along the prefix tree; at most one E matches)
        for (int p = tid; p < nb_new * nb_new; p += CB_NT) {
            const int r = p / nb_new, e = p - r * nb_new;
            if (order[r] >= nb || order[e] < nb || n.link[r] >= 0 || n.len[r] < 2 || n.len[e] != n.len[r] - 1) continue;
            int x = nodes[n.node[r]].x, y = n.node[e];   // B's parent node, E's node
            bool same = true;
            while (x != y) {
                if (x <= 0 || y <= 0) { same = false; break; }   // (one chain at the root first: not the same length)
                const int2 nx = nodes[x], ny = nodes[y];
                if (nx.y != ny.y) { same = false; break; }
                x = nx.x; y = ny.x;
            }
            // (written while other threads read n.link[r] in the guard above: benign -- at most one E can match B, and a reader that sees
            // the new value skips a pair that could not match anyway)
            if (same) n.link[r] = e;
        }
        __syncthreads();
        if (tid < nb_new) tot[tid] = cb_lae(n.pb[tid], n.pnb[tid]);
        nb = nb_new;
        cur ^= 1;
        __syncthreads();
    }
    // ---- outputs: path k < N along its node chain (thread k walks path k), 0-padded
    const Beam& f = bm[cur];
    const bool nan = s_nan != 0;
    for (int k = 0; k < N; ++k) {
        const int L = (nan || k >= nb) ? 0 : f.len[k];
        int64_t* hk = hyp + ((size_t)b * N + k) * T;
        for (int t = L + tid; t < T; t += CB_NT) hk[t] = 0;
    }
    if (tid < N) {
        const int k = tid, L = (nan || k >= nb) ? 0 : f.len[k];
        int64_t* hk = hyp + ((size_t)b * N + k) * T;
        int x = L > 0 ? f.node[k] : 0;
        for (int pos = L - 1; pos >= 0; --pos) {
            const int2 nx = nodes[x];
            hk[pos] = nx.y;
            x = nx.x;
        }
        hyp_len[(size_t)b * N + k] = L;
        score[(size_t)b * N + k] = nan ? NAN : (k < nb ? tot[k] : -INFINITY);
    }
}

}  // namespace

extern "C" size_t st_ctc_beam_workspace_bytes(int B, int T, int W) {
    if (B <= 0 || T <= 0 || W <= 0) return 0;
    return (size_t)B * ((size_t)T * W + 1) * sizeof(int2);
}

extern "C" int st_ctc_beam_search(const float* prob, int B, int T, int V, const int32_t* lengths, int W, int N, int blank, int log_input,
                                  float eps, int64_t* hyp, int32_t* hyp_len, float* score, void* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(prob && hyp && hyp_len && score && ws && B > 0, "st_ctc_beam_search: bad arguments");
    ST_CHECK_ARG(T >= 1 && T <= CB_MAX_T, "st_ctc_beam_search: 1..%d frames (T=%d)", CB_MAX_T, T);
    ST_CHECK_ARG(V >= CB_MIN_V && V <= CB_MAX_V, "st_ctc_beam_search: %d..%d classes (V=%d)", CB_MIN_V, CB_MAX_V, V);
    ST_CHECK_ARG(W >= 1 && W <= CB_MAX_W, "st_ctc_beam_search: beam width 1..%d (W=%d)", CB_MAX_W, W);
    ST_CHECK_ARG(N >= 1 && N <= W, "st_ctc_beam_search: 1 <= N <= W (N=%d, W=%d)", N, W);
    ST_CHECK_ARG(blank >= 0 && blank < V, "st_ctc_beam_search: blank %d outside [0, %d)", blank, V);
    hipLaunchKernelGGL(ctc_beam_kernel<false>, dim3(B), dim3(CB_NT), 0, (hipStream_t)stream, prob, T, V, lengths, W, N, blank, log_input, eps,
                       hyp, hyp_len, score, reinterpret_cast<int2*>(ws), CbLmArgs<false>{});
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_ctc_beam_search_lm(const float* prob, int B, int T, int V, const int32_t* lengths, int W, int N, int blank, int log_input,
                                     float eps, const float* bonus, int order, int bos, int64_t* hyp, int32_t* hyp_len, float* score, void* ws,
                                     void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(prob && hyp && hyp_len && score && ws && B > 0, "st_ctc_beam_search_lm: bad arguments");
    ST_CHECK_ARG(T >= 1 && T <= CB_MAX_T, "st_ctc_beam_search_lm: 1..%d frames (T=%d)", CB_MAX_T, T);
    ST_CHECK_ARG(V >= CB_MIN_V && V <= CB_MAX_V, "st_ctc_beam_search_lm: %d..%d classes (V=%d)", CB_MIN_V, CB_MAX_V, V);
    ST_CHECK_ARG(W >= 1 && W <= CB_MAX_W, "st_ctc_beam_search_lm: beam width 1..%d (W=%d)", CB_MAX_W, W);
    ST_CHECK_ARG(N >= 1 && N <= W, "st_ctc_beam_search_lm: 1 <= N <= W (N=%d, W=%d)", N, W);
    ST_CHECK_ARG(blank >= 0 && blank < V, "st_ctc_beam_search_lm: blank %d outside [0, %d)", blank, V);
    ST_CHECK_ARG(bonus != nullptr, "st_ctc_beam_search_lm: no bonus table");
    ST_CHECK_ARG(order >= 1 && order <= CB_MAX_ORDER, "st_ctc_beam_search_lm: order 1..%d (order=%d)", CB_MAX_ORDER, order);
    ST_CHECK_ARG(bos >= 0 && bos < V, "st_ctc_beam_search_lm: bos %d outside [0, %d)", bos, V);
    long long rows = 1;
    for (int k = 1; k < order; ++k) rows *= V;            // (<= 1024^3: no overflow)
    ST_CHECK_ARG(rows * V <= CB_MAX_TABLE, "st_ctc_beam_search_lm: V^order = %lld table elements, at most %d", rows * V, CB_MAX_TABLE);
    hipLaunchKernelGGL(ctc_beam_kernel<true>, dim3(B), dim3(CB_NT), 0, (hipStream_t)stream, prob, T, V, lengths, W, N, blank, log_input, eps,
                       hyp, hyp_len, score, reinterpret_cast<int2*>(ws), CbLmArgs<true>{bonus, (int)rows, order == 1 ? 0 : bos});
    ST_LAUNCH_CHECK();
    return 0;
}
