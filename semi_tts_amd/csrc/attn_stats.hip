// attn_stats.hip -- where an utterance ends, read off the decoder's attention, and the alignment diagnostics of the same pass
// (contract: st_attn_endpoint in include/semitts.h).
//
// One workgroup of 256 threads (4 waves) per utterance, five phases separated by barriers:
//   1. peaks.  Wave w takes the rows w, w + 4, ...; lane l reads the columns l, l + 64, ... of a row (coalesced along L) and keeps the
//      largest non-NaN value with its column (strictly greater replaces: the lowest column of a lane wins), then six xor-shuffle steps
//      merge the 64 (value, column) pairs, a tie going to the lower column.  peak[t] and maxw[t] go to LDS.
//   2. end.  Thread i owns the steps [i seg, (i + 1) seg), seg = ceil(S / 256).  z_i = its last step whose peak is short of the last
//      phone; an inclusive max-scan over the threads (shuffles inside a wave, four wave totals through LDS) gives every thread the
//      last such step before its own, and a second walk over its steps finds the first t with K flagged steps ending at it;
//      end = the smallest t + 1 (LDS atomicMin), S when there is none.
//   3. counts over [0, end).  Steps strided over the threads: dur[peak[t]] += 1, backward jumps and skips (LDS integer atomics, one
//      per thread and counter), and the focus sum: thread i adds maxw[i], maxw[i + 256], ... in ascending order, a wave sums its 64
//      partials by xor-shuffles, thread 0 adds the four wave sums in order.  The order depends on `end` alone: bitwise repeatable.
//   4. covered = phones j < n with dur[j] > 0; peak and dur leave LDS for global memory, coalesced.
//   5. thread 0 writes the six integers and the focus.
// LDS: peak int32[4096] | maxw float[4096] | dur int32[2048] = 40 KiB static, whatever S and L are (three workgroups of 4 waves fit a
// CU; the batch has at most a few dozen utterances, so occupancy is not what limits it).  The kernel reads B S L floats once and does
// a few operations on each: it is bound by the latency of its dependent load -> shuffle chains and its barriers, not by bandwidth.
#include <math.h>
#include "st_common.h"

namespace {

constexpr int AE_NT = 256, AE_WAVES = AE_NT / ST_WAVE, AE_MAX_S = 4096, AE_MAX_L = 2048;
constexpr int AE_NONE = 0x7fffffff;         // "no non-NaN entry seen yet" in the column half of a (value, column) pair

// b replaces a when it holds an entry and a holds none, or a larger value, or the same value at a lower column
__device__ __forceinline__ void ae_merge(float& v, int& c, float ov, int oc) {
    const bool take = oc != AE_NONE && (c == AE_NONE || ov > v || (ov == v && oc < c));
    if (take) { v = ov; c = oc; }
}

__global__ __launch_bounds__(AE_NT) void attn_endpoint_kernel(const float* __restrict__ align, long a_sb, long a_st,
                                                              const int32_t* __restrict__ enc_len, int S, int L, int patience, int max_jump,
                                                              int32_t* __restrict__ stats, float* __restrict__ focus,
                                                              int32_t* __restrict__ peak, int32_t* __restrict__ dur) {
    __shared__ int s_peak[AE_MAX_S];
    __shared__ float s_maxw[AE_MAX_S];
    __shared__ int s_dur[AE_MAX_L];
    __shared__ int s_wlast[AE_WAVES];
    __shared__ float s_wsum[AE_WAVES];
    __shared__ int s_end, s_back, s_skip, s_cov, s_nonfinite;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int n = min(max(enc_len[b], 1), L);
    const float* ab = align + (size_t)b * a_sb;

    for (int j = tid; j < L; j += AE_NT) s_dur[j] = 0;
    if (tid == 0) { s_end = S + 1; s_back = 0; s_skip = 0; s_cov = 0; s_nonfinite = 0; }
    st_lds_barrier();                               // (phase 1 of another wave may set s_nonfinite)

    // ---- 1. the peak of every row
    bool bad = false;
    for (int t = wave; t < S; t += AE_WAVES) {
        const float* row = ab + (size_t)t * a_st;
        float v = 0.0f;
        int c = AE_NONE;
        for (int j = lane; j < L; j += ST_WAVE) {
            const float x = row[j];
            bad |= !(fabsf(x) < INFINITY);          // NaN or +-inf
            if (x == x && (c == AE_NONE || x > v)) { v = x; c = j; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off, ST_WAVE);
            const int oc = __shfl_xor(c, off, ST_WAVE);
            ae_merge(v, c, ov, oc);
        }
        if (lane == 0) {
            s_peak[t] = c == AE_NONE ? 0 : c;
            s_maxw[t] = c == AE_NONE ? 0.0f : v;
        }
    }
    if (bad) s_nonfinite = 1;
    __syncthreads();

    // ---- 2. the first run of `patience` steps whose peak has reached the last phone
    const int seg = (S + AE_NT - 1) / AE_NT, lo = min(tid * seg, S), hi = min(lo + seg, S);
    int last = -1;                                  // the last step before hi (so far: of this thread's own) that is not flagged
    for (int t = lo; t < hi; ++t)
        if (s_peak[t] < n - 1) last = t;
#pragma unroll
    for (int off = 1; off < ST_WAVE; off <<= 1) {
        const int o = __shfl_up(last, off, ST_WAVE);
        if (lane >= off) last = max(last, o);
    }
    if (lane == ST_WAVE - 1) s_wlast[wave] = last;
    int carry = __shfl_up(last, 1, ST_WAVE);        // exclusive: the threads before this one
    if (lane == 0) carry = -1;
    __syncthreads();
    for (int w = 0; w < wave; ++w) carry = max(carry, s_wlast[w]);
    for (int t = lo; t < hi; ++t) {
        if (s_peak[t] < n - 1) carry = t;
        else if (t - carry >= patience) { atomicMin(&s_end, t + 1); break; }
    }
    __syncthreads();
    const int reached = s_end <= S ? 1 : 0, end = reached ? s_end : S;

    // ---- 3. durations, jumps and the focus sum over [0, end)
    int back = 0, skip = 0;
    float sum = 0.0f;
    for (int t = tid; t < end; t += AE_NT) {
        const int p = s_peak[t];
        atomicAdd(&s_dur[p], 1);
        if (t >= 1) {
            const int d = p - s_peak[t - 1];
            back += d < 0;
            skip += d > max_jump;
        }
        sum += s_maxw[t];
    }
    if (back) atomicAdd(&s_back, back);
    if (skip) atomicAdd(&s_skip, skip);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, ST_WAVE);
    if (lane == 0) s_wsum[wave] = sum;
    __syncthreads();

    // ---- 4. coverage; peak and dur to global memory
    int cov = 0;
    for (int j = tid; j < n; j += AE_NT) cov += s_dur[j] > 0;
    if (cov) atomicAdd(&s_cov, cov);
    for (int t = tid; t < S; t += AE_NT) peak[(size_t)b * S + t] = s_peak[t];
    for (int j = tid; j < L; j += AE_NT) dur[(size_t)b * L + j] = s_dur[j];
    __syncthreads();

    // ---- 5. the row of integers and the focus
    if (tid == 0) {
        int32_t* st = stats + (size_t)b * 6;
        st[0] = end;
        st[1] = reached;
        st[2] = s_back;
        st[3] = s_skip;
        st[4] = s_cov;
        st[5] = s_nonfinite;
        float total = s_wsum[0];
#pragma unroll
        for (int w = 1; w < AE_WAVES; ++w) total += s_wsum[w];
        focus[b] = total / (float)end;
    }
}

}  // namespace

extern "C" int st_attn_endpoint(const float* align, long a_sb, long a_st, const int32_t* enc_len, int B, int S, int L, int patience, int max_jump,
                                int32_t* stats, float* focus, int32_t* peak, int32_t* dur, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(align && enc_len && stats && focus && peak && dur && B >= 1, "st_attn_endpoint: bad arguments");
    ST_CHECK_ARG(S >= 1 && S <= AE_MAX_S && L >= 1 && L <= AE_MAX_L, "st_attn_endpoint: 1..%d steps and 1..%d phones (S=%d, L=%d)", AE_MAX_S,
                 AE_MAX_L, S, L);
    ST_CHECK_ARG(a_st >= L && a_sb >= 0, "st_attn_endpoint: row stride %ld below L = %d, or negative batch stride %ld", a_st, L, a_sb);
    ST_CHECK_ARG(patience >= 1 && max_jump >= 1, "st_attn_endpoint: patience and max_jump must be >= 1 (got %d, %d)", patience, max_jump);
    hipLaunchKernelGGL(attn_endpoint_kernel, dim3(B), dim3(AE_NT), 0, (hipStream_t)stream, align, a_sb, a_st, enc_len, S, L, patience, max_jump,
                       stats, focus, peak, dur);
    ST_LAUNCH_CHECK();
    return 0;
}
