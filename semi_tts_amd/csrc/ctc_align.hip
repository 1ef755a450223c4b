// ctc_align.hip -- CTC forced alignment: the Viterbi path of a transcript through the posteriors (contract: st_ctc_forced_align in
// include/semitts.h).
//
// One workgroup of 256 threads per utterance.  The states ext = [blank, y0, blank, y1, ..., blank] and two ping-pong copies of the
// Viterbi values live in LDS; thread tid owns the states tid, tid + 256, ... (NS of them, a template parameter chosen from L) and keeps
// its own values in registers, so a frame costs it one LDS read of the two lower neighbours, a compare / select chain, ONE fp32
// addition, one LDS write and one LDS-only barrier (st_lds_barrier: the ping-pong makes a second one unnecessary).
// The gathers lp[t][ext[s]] are requested D frames ahead, a block of D frames at a time, from clamped addresses (never conditional),
// so the frame chain never waits for global memory.
// Back-pointers take 2 bits: a thread packs 16 frames of one state into a word.  The words go to LDS when the whole table fits the
// 64 KiB carve (BP_LDS) and to the workspace otherwise.  Thread 0 walks the back-pointers into a state path in LDS, then all threads
// write `path` and the token spans in parallel.  Integers and fp32 max / add only, no float atomics: bitwise repeatable.
#include "st_common.h"

namespace {

constexpr int CA_NT = 256, CA_MAX_T = 4096, CA_MAX_V = 10240, CA_MIN_V = 2, CA_MAX_L = 1024;
constexpr size_t CA_LDS_BUDGET = 64 * 1024 - 128;     // dynamic carve; the statics below are a few dozen bytes

// dynamic LDS in 4-byte words: ext[nmax] | A[2][nmax + 2] | state path (T int16) | back-pointer words (BP_LDS)
__host__ __device__ inline size_t ca_fixed_words(int T, int L) { const size_t nmax = 2 * (size_t)L + 1; return nmax + 2 * (nmax + 2) + ((size_t)T + 1) / 2; }
__host__ __device__ inline size_t ca_bp_words(int T, int L) { return (((size_t)T + 15) / 16) * (2 * (size_t)L + 1); }
inline bool ca_bp_in_lds(int T, int L) { return (ca_fixed_words(T, L) + ca_bp_words(T, L)) * 4 <= CA_LDS_BUDGET; }

template <int NS, int D, bool BP_LDS>
__global__ __launch_bounds__(CA_NT) void ctc_align_kernel(const float* __restrict__ prob, int T, int V, const int32_t* __restrict__ lengths,
                                                          const int64_t* __restrict__ text, int L, const int32_t* __restrict__ text_lengths,
                                                          int blank, int log_input, float eps, float* __restrict__ score,
                                                          int32_t* __restrict__ path, int32_t* __restrict__ tok_start,
                                                          int32_t* __restrict__ tok_end, unsigned* ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned ca_dyn[];
    __shared__ int scr[CA_NT / 64];
    __shared__ int s_bad, s_rep, s_nan;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nmax = 2 * L + 1;
    int* ext = reinterpret_cast<int*>(ca_dyn);
    float* A0 = reinterpret_cast<float*>(ca_dyn + nmax);
    float* A1 = A0 + nmax + 2;
    short* spath = reinterpret_cast<short*>(ca_dyn + nmax + 2 * (nmax + 2));
    unsigned* bp;
    if constexpr (BP_LDS) bp = ca_dyn + ca_fixed_words(T, L);
    else bp = ws + (size_t)b * ca_bp_words(T, L);
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    const int tl = text_lengths ? min(max(text_lengths[b], 0), L) : L;
    if (tid == 0) { s_bad = 0; s_rep = 0; s_nan = 0; }

    // ---- the targets: the non-blank entries of text[b, 0 .. tl), compacted in order (thread tid takes a contiguous chunk)
    const int64_t* row = text + (size_t)b * L;
    const int ch = (tl + CA_NT - 1) / CA_NT, i0 = min(tl, tid * ch), i1 = min(tl, i0 + ch);
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += row[i] != (int64_t)blank;
    int S, off;
    {
        const int lane = tid & 63, w = tid >> 6;
        int s = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(s, d);
            if (lane >= d) s += y;
        }
        if (lane == 63) scr[w] = s;
        __syncthreads();
        int o = 0, tot = 0;
        for (int k = 0; k < CA_NT / 64; ++k) { if (k < w) o += scr[k]; tot += scr[k]; }
        S = tot;
        off = o + s - cnt;
    }
    const int n = 2 * S + 1;
    bool bad = false;
    for (int i = i0; i < i1; ++i) {
        const int64_t y = row[i];
        if (y == (int64_t)blank) continue;
        const bool in = y >= 0 && y < (int64_t)V;
        bad |= !in;
        ext[2 * off + 1] = in ? (int)y : blank;
        ++off;
    }
    if (bad) s_bad = 1;
    for (int s = 2 * tid; s < n; s += 2 * CA_NT) ext[s] = blank;
    for (int s = tid; s < n + 2; s += CA_NT) { A0[s] = s == 2 ? 0.0f : -INFINITY; A1[s] = -INFINITY; }   // A[2 + s]; the virtual frame -1: state 0 at log 1
    __syncthreads();
    {
        int rep = 0;
        for (int k = 1 + tid; k < S; k += CA_NT) rep += ext[2 * k + 1] == ext[2 * k - 1];
        if (rep) atomicAdd(&s_rep, rep);
    }
    __syncthreads();
    const bool refused = s_bad != 0, infeasible = len < S + s_rep;

    if (!refused && !infeasible) {      // (uniform)
        int e[NS];
        bool valid[NS], skip[NS];
        float mine[NS];
        unsigned w[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int s = tid + j * CA_NT;
            valid[j] = s < n;
            e[j] = valid[j] ? ext[s] : blank;
            skip[j] = valid[j] && s >= 2 && e[j] != blank && e[j] != ext[max(s - 2, 0)];
            mine[j] = s == 0 ? 0.0f : -INFINITY;
            w[j] = 0u;
        }
        const float* base = prob + (size_t)b * T * V;
        const int last = max(len - 1, 0);
        float nx[D][NS];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) nx[i][j] = base[(size_t)min(i, last) * V + e[j]];
        bool nan = false;
        for (int t0 = 0; t0 < len; t0 += D) {
            float cur[D][NS];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const float x = nx[i][j];
                    const float l = log_input ? x : logf(x + eps);
                    nan |= l != l && valid[j] && t0 + i < len;
                    cur[i][j] = l;
                }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) nx[i][j] = base[(size_t)min(t0 + D + i, last) * V + e[j]];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int t = t0 + i;
                if (t < len) {          // (uniform)
                    const float* Ac = (t & 1) ? A1 : A0;
                    float* An = (t & 1) ? A0 : A1;
                    const int sh = 2 * (t & 15);
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const int s = tid + j * CA_NT;
                        if (valid[j]) {
                            const float a2r = Ac[s], a1 = Ac[s + 1];          // states s - 2 and s - 1 (A is shifted by 2)
                            const float a2 = skip[j] ? a2r : -INFINITY;
                            float best = mine[j];
                            unsigned p = 0u;
                            if (a1 > best) { best = a1; p = 1u; }
                            if (a2 > best) { best = a2; p = 2u; }
                            mine[j] = best + cur[i][j];
                            An[s + 2] = mine[j];
                            w[j] = (sh == 0 ? 0u : w[j]) | (p << sh);
                            if (sh == 30) bp[(size_t)(t >> 4) * n + s] = w[j];
                        }
                    }
                    st_lds_barrier();
                }
            }
        }
        if (len > 0 && (len & 15) != 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (valid[j]) bp[(size_t)((len - 1) >> 4) * n + tid + j * CA_NT] = w[j];
        }
        if (nan) s_nan = 1;
    }
    __syncthreads();        // (also publishes the workspace form's back-pointer words to thread 0)
    const bool ok = !refused && !infeasible && s_nan == 0;
    if (tid == 0) {
        const float* Af = (len & 1) ? A1 : A0;
        int s = n - 1;
        if (n > 1 && Af[2 + n - 2] > Af[2 + n - 1]) s = n - 2;
        score[b] = (refused || s_nan) ? NAN : (infeasible ? -INFINITY : Af[2 + s]);
        if (ok && len > 0) {
            spath[len - 1] = (short)s;
            size_t at = ~(size_t)0;
            unsigned word = 0u;
            for (int t = len - 1; t > 0; --t) {
                const size_t idx = (size_t)(t >> 4) * n + s;
                if (idx != at) { word = bp[idx]; at = idx; }
                s -= (int)((word >> (2 * (t & 15))) & 3u);
                spath[t - 1] = (short)s;
            }
        }
    }
    __syncthreads();
    int32_t* pb = path + (size_t)b * T;
    int32_t* ts = tok_start + (size_t)b * L;
    int32_t* te = tok_end + (size_t)b * L;
    for (int t = tid; t < T; t += CA_NT) pb[t] = (ok && t < len) ? ext[spath[t]] : -1;
    for (int k = tid; k < L; k += CA_NT)
        if (!ok || k >= S) { ts[k] = -1; te[k] = -1; }
    if (ok) {
        for (int t = tid; t < len; t += CA_NT) {
            const int s = spath[t];
            if (!(s & 1)) continue;
            if (t == 0 || spath[t - 1] != s) ts[s >> 1] = t;
            if (t == len - 1 || spath[t + 1] != s) te[s >> 1] = t + 1;
        }
    }
}

template <int NS, int D>
void ca_launch(bool lds, size_t bytes, int B, hipStream_t st, const float* prob, int T, int V, const int32_t* lengths, const int64_t* text, int L,
               const int32_t* text_lengths, int blank, int log_input, float eps, float* score, int32_t* path, int32_t* tok_start,
               int32_t* tok_end, unsigned* ws) {
    if (lds)
        hipLaunchKernelGGL((ctc_align_kernel<NS, D, true>), dim3(B), dim3(CA_NT), bytes, st, prob, T, V, lengths, text, L, text_lengths, blank,
                           log_input, eps, score, path, tok_start, tok_end, ws);
    else
        hipLaunchKernelGGL((ctc_align_kernel<NS, D, false>), dim3(B), dim3(CA_NT), bytes, st, prob, T, V, lengths, text, L, text_lengths, blank,
                           log_input, eps, score, path, tok_start, tok_end, ws);
}

}  // namespace

extern "C" size_t st_ctc_align_workspace_bytes(int B, int T, int L) {
    if (B <= 0 || T <= 0 || L <= 0 || ca_bp_in_lds(T, L)) return 0;
    return (size_t)B * ca_bp_words(T, L) * sizeof(unsigned);
}

extern "C" int st_ctc_forced_align(const float* prob, int B, int T, int V, const int32_t* lengths, const int64_t* text, int L,
                                   const int32_t* text_lengths, int blank, int log_input, float eps, float* score, int32_t* path,
                                   int32_t* tok_start, int32_t* tok_end, void* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(prob && text && score && path && tok_start && tok_end && B > 0, "st_ctc_forced_align: bad arguments");
    ST_CHECK_ARG(T >= 1 && T <= CA_MAX_T, "st_ctc_forced_align: 1..%d frames (T=%d)", CA_MAX_T, T);
    ST_CHECK_ARG(V >= CA_MIN_V && V <= CA_MAX_V, "st_ctc_forced_align: %d..%d classes (V=%d)", CA_MIN_V, CA_MAX_V, V);
    ST_CHECK_ARG(L >= 1 && L <= CA_MAX_L, "st_ctc_forced_align: 1..%d transcript entries (L=%d)", CA_MAX_L, L);
    ST_CHECK_ARG(blank >= 0 && blank < V, "st_ctc_forced_align: blank %d outside [0, %d)", blank, V);
    const bool lds = ca_bp_in_lds(T, L);
    ST_CHECK_ARG(lds || ws, "st_ctc_forced_align: T=%d, L=%d needs the workspace of st_ctc_align_workspace_bytes", T, L);
    const size_t bytes = (ca_fixed_words(T, L) + (lds ? ca_bp_words(T, L) : 0)) * 4;
    hipStream_t st = (hipStream_t)stream;
    unsigned* w = reinterpret_cast<unsigned*>(ws);
    const int nmax = 2 * L + 1;          // states per thread: NS = ceil(nmax / 256); gathers requested D frames ahead
#define CA_GO(NS, D) ca_launch<NS, D>(lds, bytes, B, st, prob, T, V, lengths, text, L, text_lengths, blank, log_input, eps, score, path, tok_start, tok_end, w)
    if (nmax <= CA_NT) CA_GO(1, 8);
    else if (nmax <= 2 * CA_NT) CA_GO(2, 8);
    else if (nmax <= 4 * CA_NT) CA_GO(4, 4);
    else CA_GO(9, 4);
#undef CA_GO
    ST_LAUNCH_CHECK();
    return 0;
}
