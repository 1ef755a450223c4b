// dtw.hip -- dynamic time warping of ragged pairs of feature sequences: the cheapest monotone path through the grid of frame
// distances, its cost and the path itself (contract: st_dtw_batch in include/semitts.h).
//
// One workgroup of 256 threads per pair sweeps the anti-diagonals i + j = c.  A cell needs D(i-1, j-1) from diagonal c - 2 and
// D(i-1, j), D(i, j-1) from diagonal c - 1, so three rolling diagonals indexed by i live in LDS (3 Tx floats) and a diagonal costs one
// LDS-only barrier (st_lds_barrier: a thread of diagonal c + 1 overwrites diagonal c - 2, which nobody reads after that barrier).
// Thread tid takes the cells at positions tid, tid + 256, ... of a diagonal (position p is row ilo + p, ilo = max(0, c - (m - 1))):
// consecutive lanes read consecutive rows of x and of y, which are staged in LDS at an odd row stride (no bank conflict) when they fit
// (ROWS_LDS) and read through L2 otherwise.  The distance d(i, j) is formed on the fly; no n x m float matrix exists anywhere.
// Back-pointers take 2 bits, indexed by (diagonal, position): the four lanes of a quad gather their codes by two DPP steps and the
// first stores one byte, so no two threads share a store.  The bytes go to LDS when the table fits beside the diagonals (BP_LDS) and
// to the workspace otherwise.  Thread 0 walks the back-pointers from (n-1, m-1) into a reversed list in LDS, then all threads write
// `path` in forward order.  fp32 compare / add only, no atomics on floats: bitwise repeatable.
#include <math.h>
#include "st_common.h"

namespace {

constexpr int DT_NT = 256, DT_MAX_T = 4096, DT_MAX_D = 64;
constexpr size_t DT_LDS_BUDGET = 160 * 1024 - 256;      // dynamic carve of the 160 KiB of a gfx950 CU; the statics below are a few bytes

// dynamic LDS in 4-byte words: diagonals [3][Tx] | reversed path list (Tx + Ty - 1) | back-pointer bytes (BP_LDS) | x rows, y rows (ROWS_LDS)
__host__ __device__ inline int dt_bpd(int Tx, int Ty) { return (min(Tx, Ty) + 3) / 4; }                    // back-pointer bytes per diagonal
__host__ __device__ inline size_t dt_fixed_words(int Tx, int Ty) { return 3 * (size_t)Tx + (size_t)(Tx + Ty - 1); }
__host__ __device__ inline size_t dt_bp_bytes(int Tx, int Ty) { return (((size_t)(Tx + Ty - 1) * dt_bpd(Tx, Ty)) + 15) / 16 * 16; }
__host__ __device__ inline int dt_row_stride(int D) { return D | 1; }
inline bool dt_bp_in_lds(int Tx, int Ty) { return dt_fixed_words(Tx, Ty) * 4 + dt_bp_bytes(Tx, Ty) <= DT_LDS_BUDGET; }
inline size_t dt_rows_words(int Tx, int Ty, int D) { return (size_t)(Tx + Ty) * dt_row_stride(D); }

__device__ __forceinline__ unsigned dt_quad_or(unsigned v) {       // OR over the 4 lanes of a quad (all 64 lanes must be active)
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ST_DPP_QUAD_XOR1, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ST_DPP_QUAD_XOR2, 0xf, 0xf, true);
    return v;
}

// sum_k (x[k] - y[k])^2 in fp32 over ascending k; the loads of 8 (then 4) columns are issued together, the additions stay in order
__device__ __forceinline__ float dt_sqdist(const float* __restrict__ xr, const float* __restrict__ yr, int D) {
    float s = 0.0f;
    int k = 0;
    for (; k + 8 <= D; k += 8) {
        float a[8], c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { a[u] = xr[k + u]; c[u] = yr[k + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const float t = a[u] - c[u]; s += t * t; }
    }
    if (k + 4 <= D) {
        float a[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = xr[k + u]; c[u] = yr[k + u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const float t = a[u] - c[u]; s += t * t; }
        k += 4;
    }
    for (; k < D; ++k) { const float t = xr[k] - yr[k]; s += t * t; }
    return s;
}

template <bool ROWS_LDS, bool BP_LDS>
__global__ __launch_bounds__(DT_NT) void dtw_kernel(const float* __restrict__ x, long x_sb, long x_st, const int32_t* __restrict__ x_len, int Tx,
                                                    const float* __restrict__ y, long y_sb, long y_st, const int32_t* __restrict__ y_len, int Ty,
                                                    int d0, int D, float scale, float* __restrict__ total, int32_t* __restrict__ path_len,
                                                    int32_t* __restrict__ path, unsigned char* ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned dt_dyn[];
    __shared__ int s_nan, s_plen;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = x_len ? min(max(x_len[b], 0), Tx) : Tx;
    const int m = y_len ? min(max(y_len[b], 0), Ty) : Ty;
    const int PL = Tx + Ty - 1, bpd = dt_bpd(Tx, Ty), Ds = dt_row_stride(D);
    float* diag = reinterpret_cast<float*>(dt_dyn);
    unsigned* list = dt_dyn + 3 * (size_t)Tx;
    unsigned char* bp;
    if constexpr (BP_LDS) bp = reinterpret_cast<unsigned char*>(dt_dyn + dt_fixed_words(Tx, Ty));
    else bp = ws + (size_t)b * dt_bp_bytes(Tx, Ty);
    float* xs = reinterpret_cast<float*>(dt_dyn + dt_fixed_words(Tx, Ty)) + (BP_LDS ? dt_bp_bytes(Tx, Ty) / 4 : 0);
    float* ys = xs + (size_t)Tx * Ds;
    const float* xb = x + (size_t)b * x_sb + d0;
    const float* yb = y + (size_t)b * y_sb + d0;
    if (tid == 0) { s_nan = 0; s_plen = 0; }
    __syncthreads();

    // ---- the read columns of the valid rows: NaN check, and the LDS copy at row stride Ds
    const bool empty = n == 0 || m == 0;
    if (!empty) {       // (uniform)
        bool nan = false;
        for (int e = tid; e < n * D; e += DT_NT) {
            const int i = e / D, k = e - i * D;
            const float v = xb[(size_t)i * x_st + k];
            nan |= v != v;
            if constexpr (ROWS_LDS) xs[i * Ds + k] = v;
        }
        for (int e = tid; e < m * D; e += DT_NT) {
            const int j = e / D, k = e - j * D;
            const float v = yb[(size_t)j * y_st + k];
            nan |= v != v;
            if constexpr (ROWS_LDS) ys[j * Ds + k] = v;
        }
        if (nan) s_nan = 1;
    }
    __syncthreads();
    const bool ok = !empty && s_nan == 0;

    if (ok) {           // (uniform)
        float* cur = diag;                  // diagonal c
        float* p1 = diag + Tx;              // diagonal c - 1
        float* p2 = diag + 2 * (size_t)Tx;  // diagonal c - 2
        const unsigned sh = 2u * (tid & 3);
        for (int c = 0; c < n + m - 1; ++c) {
            const int ilo = max(0, c - (m - 1)), ihi = min(n - 1, c), len = ihi - ilo + 1;
            unsigned char* bpc = bp + (size_t)c * bpd;
            for (int q0 = 0; q0 < len; q0 += DT_NT) {       // (uniform trip count: every lane reaches the DPP steps)
                const int p = q0 + tid;
                const bool valid = p < len;
                const int i = min(ilo + p, ihi), j = c - i;
                // the predecessors (clamped addresses, never conditional: the loads go out beside the row loads below)
                const int im = max(i - 1, 0);
                const float dg = p2[im], up = p1[im], left = p1[i];
                float s;
                if constexpr (ROWS_LDS) s = dt_sqdist(xs + i * Ds, ys + j * Ds, D);
                else s = dt_sqdist(xb + (size_t)i * x_st, yb + (size_t)j * y_st, D);
                const float d = scale * sqrtf(s);
                // a cell has all three predecessors, or one (first row / column), or none ((0, 0)): the diagonal, then (i-1, j), then (i, j-1)
                const bool hi = i > 0, hj = j > 0, both = hi && hj;
                float best = both ? dg : (hi ? up : (hj ? left : 0.0f));
                unsigned code = both ? 0u : (hi ? 1u : (hj ? 2u : 0u));
                if (both && up < best) { best = up; code = 1u; }
                if (both && left < best) { best = left; code = 2u; }
                if (valid) cur[i] = best + d;
                const unsigned packed = dt_quad_or(valid ? code << sh : 0u);
                if (valid && sh == 0u) bpc[p >> 2] = (unsigned char)packed;
            }
            st_lds_barrier();
            float* t = p2; p2 = p1; p1 = cur; cur = t;
        }
        // (after the last rotation p1 is the last diagonal)
        if (tid == 0) total[b] = p1[n - 1];
    }
    __syncthreads();        // (also publishes the workspace form's back-pointer bytes to thread 0)
    if (tid == 0) {
        int P = 0;
        if (ok) {
            int i = n - 1, j = m - 1;
            const bool keep = path != nullptr;
            while (P < PL) {        // (a path has at most n + m - 1 cells; the sweep wrote a code for every cell, and only moves that exist)
                if (keep) list[P] = (unsigned)i | ((unsigned)j << 16);
                ++P;
                if (i == 0 && j == 0) break;
                const int c = i + j, p = i - max(0, c - (m - 1));
                const unsigned code = (bp[(size_t)c * bpd + (p >> 2)] >> (2 * (p & 3))) & 3u;
                if (code != 2u && i > 0) --i;
                if (code != 1u && j > 0) --j;
            }
        } else {
            total[b] = NAN;
        }
        path_len[b] = P;
        s_plen = P;
    }
    if (path) {             // (uniform)
        __syncthreads();
        const int P = s_plen;
        int32_t* pb = path + (size_t)b * PL * 2;
        for (int p = tid; p < PL; p += DT_NT) {
            int i = -1, j = -1;
            if (p < P) { const unsigned e = list[P - 1 - p]; i = (int)(e & 0xffffu); j = (int)(e >> 16); }
            pb[2 * p] = i;
            pb[2 * p + 1] = j;
        }
    }
}

template <bool ROWS_LDS, bool BP_LDS>
int dt_launch(size_t lds, int B, hipStream_t st, const float* x, long x_sb, long x_st, const int32_t* x_len, int Tx, const float* y, long y_sb,
              long y_st, const int32_t* y_len, int Ty, int d0, int D, float scale, float* total, int32_t* path_len, int32_t* path,
              unsigned char* ws) {
    static size_t seen = 0;
    if (int rc = st_lds_opt_in(reinterpret_cast<const void*>(dtw_kernel<ROWS_LDS, BP_LDS>), lds, lds > 48 * 1024, seen)) return rc;
    hipLaunchKernelGGL((dtw_kernel<ROWS_LDS, BP_LDS>), dim3(B), dim3(DT_NT), lds, st, x, x_sb, x_st, x_len, Tx, y, y_sb, y_st, y_len, Ty, d0, D,
                       scale, total, path_len, path, ws);
    return 0;
}

}  // namespace

extern "C" size_t st_dtw_workspace_bytes(int B, int Tx, int Ty) {
    if (B <= 0 || Tx <= 0 || Ty <= 0 || Tx > DT_MAX_T || Ty > DT_MAX_T || dt_bp_in_lds(Tx, Ty)) return 0;
    return (size_t)B * dt_bp_bytes(Tx, Ty);
}

extern "C" int st_dtw_batch(const float* x, long x_sb, long x_st, const int32_t* x_len, int Tx, const float* y, long y_sb, long y_st,
                            const int32_t* y_len, int Ty, int B, int d0, int d1, float scale, float* total, int32_t* path_len, int32_t* path,
                            void* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(x && y && total && path_len && B >= 1, "st_dtw_batch: bad arguments");
    ST_CHECK_ARG(Tx >= 1 && Tx <= DT_MAX_T && Ty >= 1 && Ty <= DT_MAX_T, "st_dtw_batch: 1..%d frames a side (Tx=%d, Ty=%d)", DT_MAX_T, Tx, Ty);
    ST_CHECK_ARG(d0 >= 0 && d0 < d1 && d1 - d0 <= DT_MAX_D, "st_dtw_batch: columns [d0, d1) = [%d, %d): 0 <= d0 < d1, at most %d of them", d0, d1,
                 DT_MAX_D);
    ST_CHECK_ARG(x_st >= d1 && y_st >= d1, "st_dtw_batch: row strides %ld, %ld below d1 = %d", x_st, y_st, d1);
    ST_CHECK_ARG(x_sb >= 0 && y_sb >= 0, "st_dtw_batch: negative batch strides %ld, %ld", x_sb, y_sb);
    ST_CHECK_ARG(scale > 0.0f && scale < INFINITY, "st_dtw_batch: scale must be finite and positive (got %g)", (double)scale);
    const int D = d1 - d0;
    const bool bp_lds = dt_bp_in_lds(Tx, Ty);
    ST_CHECK_ARG(bp_lds || ws, "st_dtw_batch: Tx=%d, Ty=%d needs the workspace of st_dtw_workspace_bytes", Tx, Ty);
    size_t lds = dt_fixed_words(Tx, Ty) * 4 + (bp_lds ? dt_bp_bytes(Tx, Ty) : 0);
    const bool rows_lds = lds + dt_rows_words(Tx, Ty, D) * 4 <= DT_LDS_BUDGET;
    if (rows_lds) lds += dt_rows_words(Tx, Ty, D) * 4;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = reinterpret_cast<unsigned char*>(ws);
    int rc;
#define DT_GO(R, P) rc = dt_launch<R, P>(lds, B, st, x, x_sb, x_st, x_len, Tx, y, y_sb, y_st, y_len, Ty, d0, D, scale, total, path_len, path, w)
    if (rows_lds && bp_lds) DT_GO(true, true);
    else if (rows_lds) DT_GO(true, false);
    else if (bp_lds) DT_GO(false, true);
    else DT_GO(false, false);
#undef DT_GO
    if (rc) return rc;
    ST_LAUNCH_CHECK();
    return 0;
}
