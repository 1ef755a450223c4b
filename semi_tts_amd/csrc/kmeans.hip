// kmeans.hip -- k-means over frame features: nearest centroid, centroid update, empty-cluster relocation and k-means++ seeding
// (contracts: st_kmeans_assign, st_kmeans_update, st_kmeans_relocate, st_kmeans_pp_step, st_kmeans_pp_pick in include/semitts.h).
//
// st_kmeans_assign.  The expanded form d = max(0, (|x|^2 + |c|^2) - 2 x.c): one FMA a term where the direct form takes a subtraction and
// an FMA.  A lane owns KM_P points; a workgroup of 256 lanes owns 512.  The centroids pass through LDS in tiles of up to 32 KiB, zero
// padded to a multiple of four columns and of KM_KT rows, |c|^2 beside them (+inf for a padding row, which therefore never wins).  A
// lane keeps a register tile of KM_P x KM_KT dot products; every 16-byte read of the centroid tile is at one address for the whole
// wave (a broadcast, no bank conflict) and feeds KM_P x 4 FMAs.  With D <= KM_DC the lane's rows stay in registers over all tiles
// (the MFCC case, D = 39); a wider row is re-read in chunks of KM_DC columns for every KM_KT centroids (L1 / L2 hits).  All sums run
// over ascending d as fmaf chains, the centroids are visited in ascending k and a candidate wins only when strictly smaller.
//
// st_kmeans_update.  No floating-point atomics and no order that depends on the launch: (1) a histogram of the K clusters per chunk of
// 1024 points in LDS (integer atomics: a count does not depend on their order), and the chunk's sum of dist by a fixed tree;
// (2) an exclusive scan of every cluster's row of chunk counts and (3) of the cluster totals; (4) a stable scatter of the point indices
// -- a point's place is its cluster's start + the members in earlier chunks + its rank among the members of its own chunk -- so
// that a cluster's members stand in ascending n; (5) slabs of 256 members summed in float64 in that order, lanes across d, one slab a
// wave-aligned lane group; (6) per cluster the slabs added in ascending order, the division, the shift; (7) the four statistics by fixed
// trees.  Which workgroup takes which slab changes nothing: a slab is always summed from zero by one lane per column.
//
// st_kmeans_relocate.  The rare path: one workgroup selects the e-th point of the order (dist descending, n ascending) by a full
// pass for every empty cluster -- the candidate after the previous choice -- and copies its row.
//
// st_kmeans_pp_step / st_kmeans_pp_pick.  The step is one workgroup per chunk of 1024 points (direct form sum (x - x_p)^2, which is
// exactly 0 for a copy of x_p) and leaves the chunk's sum of weights; the pick is one workgroup that scans the chunk sums, finds the
// chunk where the running sum passes u * total and scans that chunk's 1024 weights.
#include <math.h>
#include "st_common.h"

namespace {

constexpr int KM_NT = 256, KM_P = 2, KM_KT = 16, KM_DC = 40, KM_PTS = KM_NT * KM_P;
constexpr int KM_TILE_FLOATS = 8192;            // floats of one centroid tile in LDS
constexpr int KM_MAX_D = 256, KM_MAX_K = 4096;
constexpr int KM_CHUNK = 1024, KM_SLAB = 256;   // points of a histogram chunk; members of a summation slab
constexpr int KM_BIG = 1024;                    // threads of the single-workgroup kernels

__host__ __device__ inline int km_tile_rows(int K, int Dp) {
    int r = (KM_TILE_FLOATS / Dp) & ~(KM_KT - 1);
    if (r < KM_KT) r = KM_KT;
    const int kr = (K + KM_KT - 1) & ~(KM_KT - 1);
    return r < kr ? r : kr;
}

__device__ __forceinline__ void km_load_chunk(float (&xv)[KM_DC], const float* __restrict__ xr, int D, int d0) {
#pragma unroll
    for (int j = 0; j < KM_DC / 4; ++j) {
        const int d = d0 + 4 * j, rem = D - d;
        const f32x4 v = rem >= 4 ? st_ld4_u(xr + d) : st_ld4_guard(xr + d, rem);
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[4 * j + u] = v[u];
    }
}

template <bool SINGLE>
__global__ __launch_bounds__(KM_NT) void km_assign_kernel(const float* __restrict__ x, long ld, int N, int D, const float* __restrict__ cent,
                                                          int K, int TKL, int32_t* __restrict__ idx, float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) float km_dyn[];
    const int Dp = (D + 3) & ~3;
    float* cs = km_dyn;                         // (TKL, Dp)
    float* ccs = cs + (size_t)TKL * Dp;         // (TKL)
    const int t = threadIdx.x;
    long n[KM_P];
    const float* xr[KM_P];
    float xv[KM_P][KM_DC], xx[KM_P], best[KM_P];
    int bi[KM_P];
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
        n[p] = (long)blockIdx.x * KM_PTS + p * KM_NT + t;
        xr[p] = x + (n[p] < N ? n[p] : (long)N - 1) * ld;     // (a lane past the end reads the last row and writes nothing)
        xx[p] = 0.0f;
        best[p] = INFINITY;
        bi[p] = 0;
        for (int d0 = 0; d0 < Dp; d0 += KM_DC) {
            km_load_chunk(xv[p], xr[p], D, d0);
#pragma unroll
            for (int u = 0; u < KM_DC; ++u) xx[p] = fmaf(xv[p][u], xv[p][u], xx[p]);
        }
    }
    for (int k0 = 0; k0 < K; k0 += TKL) {
        const int nk = K - k0 < TKL ? K - k0 : TKL;
        const int rows = (nk + KM_KT - 1) & ~(KM_KT - 1);
        __syncthreads();
        for (int e = t; e < rows * Dp; e += KM_NT) {
            const int r = e / Dp, d = e - r * Dp;
            cs[e] = r < nk && d < D ? cent[(size_t)(k0 + r) * D + d] : 0.0f;
        }
        __syncthreads();
        for (int r = t; r < rows; r += KM_NT) {
            float s = 0.0f;
            for (int d = 0; d < D; ++d) s = fmaf(cs[r * Dp + d], cs[r * Dp + d], s);
            ccs[r] = r < nk ? s : INFINITY;
        }
        __syncthreads();
        for (int ks = 0; ks < rows; ks += KM_KT) {
            float acc[KM_P][KM_KT];
#pragma unroll
            for (int p = 0; p < KM_P; ++p)
#pragma unroll
                for (int kk = 0; kk < KM_KT; ++kk) acc[p][kk] = 0.0f;
            for (int d0 = 0; d0 < Dp; d0 += KM_DC) {
                if (!SINGLE) {
#pragma unroll
                    for (int p = 0; p < KM_P; ++p) km_load_chunk(xv[p], xr[p], D, d0);
                }
#pragma unroll
                for (int j = 0; j < KM_DC / 4; ++j) {
                    const int d = d0 + 4 * j;
                    if (d < Dp) {               // (uniform)
#pragma unroll
                        for (int kk = 0; kk < KM_KT; ++kk) {
                            const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (ks + kk) * Dp + d);
#pragma unroll
                            for (int p = 0; p < KM_P; ++p)
#pragma unroll
                                for (int u = 0; u < 4; ++u) acc[p][kk] = fmaf(xv[p][4 * j + u], c[u], acc[p][kk]);
                        }
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < KM_KT; ++kk) {
                const float cc = ccs[ks + kk];
#pragma unroll
                for (int p = 0; p < KM_P; ++p) {
                    const float d = fmaxf(fmaf(-2.0f, acc[p][kk], xx[p] + cc), 0.0f);
                    if (d < best[p]) {
                        best[p] = d;
                        bi[p] = k0 + ks + kk;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
        if (n[p] < N) {
            const bool bad = !(xx[p] < INFINITY);        // a NaN or an infinity among the row's entries (or a norm past fp32)
            idx[n[p]] = bad ? -1 : bi[p];
            dist[n[p]] = bad ? NAN : best[p];
        }
    }
}

// ------------------------------------------------------------------------------------------------ fixed trees and scans of a workgroup
// the sum of one value a thread over NT threads (a power of two): the same pairs in the same order on every run; all threads get it
template <int NT, typename T>
__device__ __forceinline__ T km_block_sum(T v, T* buf) {
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) buf[t] = buf[t] + buf[t + s];
        __syncthreads();
    }
    return buf[0];
}

// exclusive scan of one value a thread (Hillis-Steele over two buffers of NT); total: the sum of all
template <int NT, typename T>
__device__ __forceinline__ T km_block_excl_scan(T v, T* buf /* 2 NT */, T& total) {
    const int t = threadIdx.x;
    __syncthreads();
    T* a = buf;
    T* b = buf + NT;
    a[t] = v;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {
        b[t] = t >= s ? a[t - s] + a[t] : a[t];
        __syncthreads();
        T* c = a; a = b; b = c;
    }
    total = a[NT - 1];
    return a[t] - v;                            // (exact for integers; the float64 users take the inclusive value and subtract nothing)
}

template <int NT>
__device__ __forceinline__ double km_block_incl_scan(double v, double* buf /* 2 NT */, double& total) {
    const int t = threadIdx.x;
    __syncthreads();
    double* a = buf;
    double* b = buf + NT;
    a[t] = v;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {
        b[t] = t >= s ? a[t - s] + a[t] : a[t];
        __syncthreads();
        double* c = a; a = b; b = c;
    }
    total = a[NT - 1];
    return a[t];
}

// ------------------------------------------------------------------------------------------------ update
struct KmWs {
    double* cin;        // (NC) the chunks' sums of dist
    double* part;       // (N / KM_SLAB + K + 1, D) the slabs' sums
    double* shiftk;     // (K)
    int32_t* hist;      // (K, NC) counts, then each row's exclusive scan
    int32_t* start;     // (K + 1)
    int32_t* perm;      // (N)
};

__host__ __device__ inline long km_chunks(long N) { return (N + KM_CHUNK - 1) / KM_CHUNK; }
inline size_t km_part_rows(long N, int K) { return (size_t)(N / KM_SLAB) + (size_t)K + 1; }

inline size_t km_ws_carve(KmWs* w, void* base, long N, int D, int K) {
    const size_t NC = (size_t)km_chunks(N);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 15) & ~(size_t)15; return o; };
    const size_t o_cin = take(NC * 8), o_part = take(km_part_rows(N, K) * D * 8), o_shift = take((size_t)K * 8);
    const size_t o_hist = take((size_t)K * NC * 4), o_start = take(((size_t)K + 1) * 4), o_perm = take((size_t)N * 4);
    if (w) {
        char* b = (char*)base;
        w->cin = (double*)(b + o_cin); w->part = (double*)(b + o_part); w->shiftk = (double*)(b + o_shift);
        w->hist = (int32_t*)(b + o_hist); w->start = (int32_t*)(b + o_start); w->perm = (int32_t*)(b + o_perm);
    }
    return off;
}

__global__ __launch_bounds__(KM_NT) void km_hist_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, int N, int K, long NC,
                                                        int32_t* __restrict__ hist, double* __restrict__ cin) {
    __shared__ int32_t h[KM_MAX_K];
    __shared__ double red[KM_NT];
    const int t = threadIdx.x;
    const long c = blockIdx.x;
    for (int k = t; k < K; k += KM_NT) h[k] = 0;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const long n = c * KM_CHUNK + i * KM_NT + t;
        if (n < N) {
            const int k = idx[n];
            if (k >= 0 && k < K) {
                atomicAdd(&h[k], 1);
                s += (double)dist[n];
            }
        }
    }
    s = km_block_sum<KM_NT>(s, red);
    for (int k = t; k < K; k += KM_NT) hist[(size_t)k * NC + c] = h[k];
    if (t == 0) cin[c] = s;
}

// one workgroup a cluster: its row of chunk counts -> the exclusive scan of the row; start[k] = the row's total (scanned by km_start_kernel)
__global__ __launch_bounds__(KM_NT) void km_rowscan_kernel(int32_t* __restrict__ hist, long NC, int32_t* __restrict__ start) {
    __shared__ int32_t buf[2 * KM_NT];
    const int t = threadIdx.x;
    int32_t* row = hist + (size_t)blockIdx.x * NC;
    int32_t carry = 0;
    for (long c0 = 0; c0 < NC; c0 += KM_NT) {
        const long c = c0 + t;
        const int32_t v = c < NC ? row[c] : 0;
        int32_t tot;
        const int32_t ex = km_block_excl_scan<KM_NT>(v, buf, tot);
        if (c < NC) row[c] = carry + ex;
        carry += tot;
    }
    if (t == 0) start[blockIdx.x] = carry;
}

__global__ __launch_bounds__(KM_BIG) void km_start_kernel(int32_t* __restrict__ start, int K) {
    __shared__ int32_t buf[2 * KM_BIG];
    const int t = threadIdx.x;
    int32_t v[KM_MAX_K / KM_BIG], s = 0;
#pragma unroll
    for (int i = 0; i < KM_MAX_K / KM_BIG; ++i) {
        const int k = t * (KM_MAX_K / KM_BIG) + i;
        v[i] = k < K ? start[k] : 0;
        s += v[i];
    }
    int32_t tot;
    int32_t run = km_block_excl_scan<KM_BIG>(s, buf, tot);
#pragma unroll
    for (int i = 0; i < KM_MAX_K / KM_BIG; ++i) {
        const int k = t * (KM_MAX_K / KM_BIG) + i;
        if (k < K) start[k] = run;
        run += v[i];
    }
    if (t == 0) start[K] = tot;
}

__global__ __launch_bounds__(KM_NT) void km_scatter_kernel(const int32_t* __restrict__ idx, int N, int K, long NC, const int32_t* __restrict__ hist,
                                                           const int32_t* __restrict__ start, int32_t* __restrict__ perm) {
    __shared__ __attribute__((aligned(16))) int32_t ids[KM_CHUNK];
    const int t = threadIdx.x;
    const long c = blockIdx.x;
#pragma unroll
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const long n = c * KM_CHUNK + i * KM_NT + t;
        int k = -1;
        if (n < N) {
            k = idx[n];
            if (k < 0 || k >= K) k = -1;
        }
        ids[i * KM_NT + t] = k;
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const int p = i * KM_NT + t;
        const int k = ids[p];
        if (k < 0) continue;
        int rank = 0, j = 0;
        for (; j + 4 <= p; j += 4) {
            const int4 q = *reinterpret_cast<const int4*>(ids + j);
            rank += (q.x == k) + (q.y == k) + (q.z == k) + (q.w == k);
        }
        for (; j < p; ++j) rank += ids[j] == k;
        const long dst = (long)start[k] + hist[(size_t)k * NC + c] + rank;
        if (dst < N) perm[dst] = (int32_t)(c * KM_CHUNK + p);
    }
}

// the slab's place among the partial sums: unique and ascending over (k, s) (see km_part_rows)
__device__ __forceinline__ size_t km_slab_row(int start_k, int k, int s) { return (size_t)(start_k / KM_SLAB) + (size_t)k + (size_t)s; }

__global__ __launch_bounds__(KM_NT) void km_slabsum_kernel(const float* __restrict__ x, long ld, int D, int lanes, const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ perm, double* __restrict__ part) {
    const int k = blockIdx.x;
    const int s0 = start[k], cnt = start[k + 1] - s0;
    const int nslab = (cnt + KM_SLAB - 1) / KM_SLAB;
    const int G = KM_NT / lanes, g = threadIdx.x / lanes, d = threadIdx.x - g * lanes;
    for (int s = blockIdx.y * G + g; s < nslab; s += gridDim.y * G) {
        const int lo = s * KM_SLAB, hi = lo + KM_SLAB < cnt ? lo + KM_SLAB : cnt;
        if (d < D) {
            double acc = 0.0;
            int i = lo;
            for (; i + 4 <= hi; i += 4) {
                const int n0 = perm[s0 + i], n1 = perm[s0 + i + 1], n2 = perm[s0 + i + 2], n3 = perm[s0 + i + 3];
                const float a0 = x[n0 * ld + d], a1 = x[n1 * ld + d], a2 = x[n2 * ld + d], a3 = x[n3 * ld + d];
                acc += (double)a0; acc += (double)a1; acc += (double)a2; acc += (double)a3;
            }
            for (; i < hi; ++i) acc += (double)x[perm[s0 + i] * ld + d];
            part[km_slab_row(s0, k, s) * D + d] = acc;
        }
    }
}

__global__ __launch_bounds__(KM_NT) void km_finalize_kernel(int D, const int32_t* __restrict__ start, const double* __restrict__ part,
                                                            const float* __restrict__ cent_in, float* __restrict__ cent_out,
                                                            int32_t* __restrict__ count, double* __restrict__ shiftk) {
    __shared__ double sq[KM_MAX_D];
    const int k = blockIdx.x, d = threadIdx.x;
    const int s0 = start[k], cnt = start[k + 1] - s0;
    const int nslab = (cnt + KM_SLAB - 1) / KM_SLAB;
    if (d < D) {
        const float cin = cent_in[(size_t)k * D + d];
        float out = cin;
        if (cnt > 0) {
            double S = 0.0;
            for (int s = 0; s < nslab; ++s) S += part[km_slab_row(s0, k, s) * D + d];
            out = (float)(S / (double)cnt);
        }
        cent_out[(size_t)k * D + d] = out;
        const double df = (double)out - (double)cin;
        sq[d] = df * df;
    }
    __syncthreads();
    if (d == 0) {
        double s = 0.0;
        for (int e = 0; e < D; ++e) s += sq[e];
        shiftk[k] = s;
        count[k] = cnt;
    }
}

__global__ __launch_bounds__(KM_BIG) void km_stats_kernel(int N, int K, long NC, const double* __restrict__ cin, const double* __restrict__ shiftk,
                                                          const int32_t* __restrict__ start, double* __restrict__ stats) {
    __shared__ double red[KM_BIG];
    __shared__ int32_t ired[KM_BIG];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    int32_t e = 0;
    for (long c = t; c < NC; c += KM_BIG) a += cin[c];
    for (int k = t; k < K; k += KM_BIG) {
        b += shiftk[k];
        e += start[k + 1] == start[k];
    }
    a = km_block_sum<KM_BIG>(a, red);
    b = km_block_sum<KM_BIG>(b, red);
    e = km_block_sum<KM_BIG>(e, ired);
    if (t == 0) {
        stats[0] = a;
        stats[1] = b;
        stats[2] = (double)e;
        stats[3] = (double)(N - start[K]);
    }
}

// ------------------------------------------------------------------------------------------------ relocate
// (d, n) stands before (d2, n2) in the order (dist descending, n ascending)
__device__ __forceinline__ bool km_before(float d, int n, float d2, int n2) { return d > d2 || (d == d2 && n < n2); }

__global__ __launch_bounds__(KM_BIG) void km_relocate_kernel(const float* __restrict__ x, long ld, int N, int D, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ dist, const int32_t* __restrict__ count, int K,
                                                             float* __restrict__ cent) {
    __shared__ int32_t empty[KM_MAX_K];
    __shared__ float rd[KM_BIG];
    __shared__ int32_t rn[KM_BIG];
    __shared__ int32_t n_empty;
    const int t = threadIdx.x;
    if (t == 0) {
        int e = 0;
        for (int k = 0; k < K; ++k)
            if (count[k] == 0) empty[e++] = k;
        n_empty = e;
    }
    __syncthreads();
    const int E = n_empty;
    float pd = INFINITY;
    int pn = -1;                                // the previous choice: every (d, n) with n >= 0 stands after (inf, -1)
    for (int e = 0; e < E; ++e) {
        float bd = -1.0f;
        int bn = -1;
        for (long n = t; n < N; n += KM_BIG) {
            const int k = idx[n];
            const float d = dist[n];
            if (k < 0 || k >= K || !(d >= 0.0f)) continue;
            if (km_before(pd, pn, d, (int)n) && (bn < 0 || km_before(d, (int)n, bd, bn))) {
                bd = d;
                bn = (int)n;
            }
        }
        __syncthreads();
        rd[t] = bd;
        rn[t] = bn;
        __syncthreads();
        for (int s = KM_BIG / 2; s > 0; s >>= 1) {
            if (t < s) {
                const float d2 = rd[t + s];
                const int n2 = rn[t + s];
                if (n2 >= 0 && (rn[t] < 0 || km_before(d2, n2, rd[t], rn[t]))) {
                    rd[t] = d2;
                    rn[t] = n2;
                }
            }
            __syncthreads();
        }
        pd = rd[0];
        pn = rn[0];
        if (pn < 0) break;                      // (uniform) fewer points than empty clusters: the rest keep their rows
        if (t < D) cent[(size_t)empty[e] * D + t] = x[pn * ld + t];
    }
}

// ------------------------------------------------------------------------------------------------ k-means++ seeding
__device__ __forceinline__ double km_weight(float m) { return m > 0.0f ? (double)m : 0.0; }

__global__ __launch_bounds__(KM_NT) void km_pp_step_kernel(const float* __restrict__ x, long ld, int N, int D, const int32_t* __restrict__ picks, int j,
                                                           float* __restrict__ mind, double* __restrict__ part, float* __restrict__ cent) {
    __shared__ float xp[KM_MAX_D];
    __shared__ double red[KM_NT];
    const int t = threadIdx.x;
    int p = picks[j];
    p = p < 0 ? 0 : (p >= N ? N - 1 : p);
    if (t < D) {
        xp[t] = x[p * ld + t];
        if (blockIdx.x == 0) cent[(size_t)j * D + t] = xp[t];
    }
    __syncthreads();
    double w = 0.0;
#pragma unroll 1
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const long n = (long)blockIdx.x * KM_CHUNK + i * KM_NT + t;
        if (n < N) {
            const float* xr = x + n * ld;
            float s = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float df = xr[d] - xp[d];
                s = fmaf(df, df, s);
            }
            const float m = s != s ? s : fminf(mind[n], s);
            mind[n] = m;
            w += km_weight(m);
        }
    }
    w = km_block_sum<KM_NT>(w, red);
    if (t == 0) part[blockIdx.x] = w;
}

__global__ __launch_bounds__(KM_NT) void km_pp_pick_kernel(int N, long NC, const float* __restrict__ mind, const double* __restrict__ part,
                                                           const double* __restrict__ u, int j, int32_t* __restrict__ picks,
                                                           double* __restrict__ totals, int32_t* __restrict__ flag) {
    __shared__ double buf[2 * KM_NT];
    __shared__ int c_first, c_last, n_first, n_last;      // (N < 2^31: a chunk index fits an int)
    __shared__ double c_base;
    const int t = threadIdx.x;
    if (j == 0) {
        if (t == 0) {
            long n = (long)floor(u[0] * (double)N);
            picks[0] = (int32_t)(n < 0 ? 0 : (n >= N ? N - 1 : n));
            totals[0] = 0.0;
        }
        return;
    }
    if (t == 0) {
        c_first = (int)NC; c_last = -1; n_first = N; n_last = -1;
    }
    const long per = (NC + KM_NT - 1) / KM_NT;
    const long lo = t * per < NC ? t * per : NC, hi = lo + per < NC ? lo + per : NC;
    double s = 0.0;
    for (long c = lo; c < hi; ++c) s += part[c];
    double total;
    const double base = km_block_incl_scan<KM_NT>(s, buf, total) - s;     // (sums of non-negative terms: the difference is the prefix up to rounding)
    const double thr = u[j] * total;
    if (!(total > 0.0)) {                       // (uniform) fewer distinct rows than centres
        if (t == 0) {
            picks[j] = 0;
            totals[j] = total;
            *flag = 1;
        }
        return;
    }
    double run = t == 0 ? 0.0 : base;
    bool found = false;
    for (long c = lo; c < hi; ++c) {
        const double v = part[c];
        if (v > 0.0) atomicMax(&c_last, (int)c);
        const double e = run + v;
        if (!found && v > 0.0 && e > thr) {      // (a chunk without weight holds no row to draw)
            atomicMin(&c_first, (int)c);
            found = true;
        }
        run = e;
    }
    __syncthreads();
    const bool fallback = c_first >= NC;
    const long cs = fallback ? c_last : c_first;
    if (cs < 0 || cs >= NC) {                   // (uniform; a total that is positive has a positive chunk: kept for the bounds alone)
        if (t == 0) {
            picks[j] = 0;
            totals[j] = total;
            *flag = 1;
        }
        return;
    }
    if (cs >= lo && cs < hi) {                  // the owner of the chosen chunk: the running sum before it
        double r = t == 0 ? 0.0 : base;
        for (long c = lo; c < cs; ++c) r += part[c];
        c_base = r;
    }
    __syncthreads();
    const double cb = c_base;
    double w[KM_CHUNK / KM_NT], ws = 0.0;
#pragma unroll
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const long n = cs * KM_CHUNK + t * (KM_CHUNK / KM_NT) + i;
        w[i] = n < N ? km_weight(mind[n]) : 0.0;
        ws += w[i];
    }
    double ctot;
    double cum = cb + (km_block_incl_scan<KM_NT>(ws, buf, ctot) - ws);
    bool hit = false;
#pragma unroll
    for (int i = 0; i < KM_CHUNK / KM_NT; ++i) {
        const int n = (int)(cs * KM_CHUNK + t * (KM_CHUNK / KM_NT) + i);
        cum += w[i];
        if (w[i] > 0.0) {
            atomicMax(&n_last, n);
            if (!hit && !fallback && cum > thr) {
                atomicMin(&n_first, n);
                hit = true;
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        picks[j] = n_first < N ? n_first : n_last;
        totals[j] = total;
    }
}

int km_check(const st_kmeans_data* x, int K, const char* who) {
    ST_CHECK_ARG(x && x->x, "%s: null data", who);
    ST_CHECK_ARG(x->N >= 1 && x->D >= 1 && x->D <= KM_MAX_D && K >= 1 && K <= KM_MAX_K, "%s: N=%d D=%d K=%d outside N >= 1, 1 <= D <= %d, 1 <= K <= %d",
                 who, x->N, x->D, K, KM_MAX_D, KM_MAX_K);
    ST_CHECK_ARG(x->ld >= x->D && (double)x->N * (double)x->ld < 1099511627776.0, "%s: ld=%ld N=%d: ld >= D and N * ld < 2^40", who, x->ld, x->N);
    return 0;
}

}  // namespace

extern "C" int st_kmeans_assign(const st_kmeans_data* x, const float* cent, int K, int32_t* idx, float* dist, void* stream) {
    if (int rc = km_check(x, K, "st_kmeans_assign")) return rc;
    ST_CHECK_ARG(cent && idx && dist, "st_kmeans_assign: null pointer");
    const int Dp = (x->D + 3) & ~3, TKL = km_tile_rows(K, Dp);
    const size_t lds = ((size_t)TKL * Dp + TKL) * sizeof(float);
    const unsigned grid = (unsigned)(((long)x->N + KM_PTS - 1) / KM_PTS);
    hipStream_t s = (hipStream_t)stream;
    if (Dp <= KM_DC) km_assign_kernel<true><<<grid, KM_NT, lds, s>>>(x->x, x->ld, x->N, x->D, cent, K, TKL, idx, dist);
    else km_assign_kernel<false><<<grid, KM_NT, lds, s>>>(x->x, x->ld, x->N, x->D, cent, K, TKL, idx, dist);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t st_kmeans_update_workspace_bytes(int N, int D, int K) {
    if (N < 1 || D < 1 || D > KM_MAX_D || K < 1 || K > KM_MAX_K) return 0;
    return km_ws_carve(nullptr, nullptr, N, D, K);
}

extern "C" int st_kmeans_update(const st_kmeans_data* x, const int32_t* idx, const float* dist, const float* cent_in, int K, float* cent_out,
                                int32_t* count, double* stats, void* ws, void* stream) {
    if (int rc = km_check(x, K, "st_kmeans_update")) return rc;
    ST_CHECK_ARG(idx && dist && cent_in && cent_out && count && stats && ws, "st_kmeans_update: null pointer");
    ST_CHECK_ARG(st_aligned16(ws), "st_kmeans_update: the workspace must be 16-byte aligned");
    KmWs w;
    km_ws_carve(&w, ws, x->N, x->D, K);
    const long NC = km_chunks(x->N);
    const int lanes = x->D <= 64 ? 64 : (x->D <= 128 ? 128 : 256), G = KM_NT / lanes;
    long Y = ((long)x->N / KM_SLAB + K + (long)K * G - 1) / ((long)K * G);     // slabs per lane group of a cluster, were they spread evenly
    Y = Y < 1 ? 1 : (Y > 1024 ? 1024 : Y);
    hipStream_t s = (hipStream_t)stream;
    km_hist_kernel<<<(unsigned)NC, KM_NT, 0, s>>>(idx, dist, x->N, K, NC, w.hist, w.cin);
    ST_LAUNCH_CHECK();
    km_rowscan_kernel<<<K, KM_NT, 0, s>>>(w.hist, NC, w.start);
    ST_LAUNCH_CHECK();
    km_start_kernel<<<1, KM_BIG, 0, s>>>(w.start, K);
    ST_LAUNCH_CHECK();
    km_scatter_kernel<<<(unsigned)NC, KM_NT, 0, s>>>(idx, x->N, K, NC, w.hist, w.start, w.perm);
    ST_LAUNCH_CHECK();
    km_slabsum_kernel<<<dim3(K, (unsigned)Y), KM_NT, 0, s>>>(x->x, x->ld, x->D, lanes, w.start, w.perm, w.part);
    ST_LAUNCH_CHECK();
    km_finalize_kernel<<<K, KM_NT, 0, s>>>(x->D, w.start, w.part, cent_in, cent_out, count, w.shiftk);
    ST_LAUNCH_CHECK();
    km_stats_kernel<<<1, KM_BIG, 0, s>>>(x->N, K, NC, w.cin, w.shiftk, w.start, stats);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_kmeans_relocate(const st_kmeans_data* x, const int32_t* idx, const float* dist, const int32_t* count, int K, float* cent,
                                  void* stream) {
    if (int rc = km_check(x, K, "st_kmeans_relocate")) return rc;
    ST_CHECK_ARG(idx && dist && count && cent, "st_kmeans_relocate: null pointer");
    km_relocate_kernel<<<1, KM_BIG, 0, (hipStream_t)stream>>>(x->x, x->ld, x->N, x->D, idx, dist, count, K, cent);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" long st_kmeans_chunks(int N) { return N < 1 ? 0 : km_chunks(N); }

extern "C" int st_kmeans_pp_step(const st_kmeans_data* x, const int32_t* picks, int j, int K, float* mind, double* part, float* cent, void* stream) {
    if (int rc = km_check(x, K, "st_kmeans_pp_step")) return rc;
    ST_CHECK_ARG(picks && mind && part && cent && j >= 0 && j < K, "st_kmeans_pp_step: null pointer, or j=%d outside [0, K=%d)", j, K);
    km_pp_step_kernel<<<(unsigned)km_chunks(x->N), KM_NT, 0, (hipStream_t)stream>>>(x->x, x->ld, x->N, x->D, picks, j, mind, part, cent);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_kmeans_pp_pick(const st_kmeans_data* x, const float* mind, const double* part, const double* u, int j, int K, int32_t* picks,
                                 double* totals, int32_t* flag, void* stream) {
    if (int rc = km_check(x, K, "st_kmeans_pp_pick")) return rc;
    ST_CHECK_ARG(mind && part && u && picks && totals && flag && j >= 0 && j < K, "st_kmeans_pp_pick: null pointer, or j=%d outside [0, K=%d)", j, K);
    km_pp_pick_kernel<<<1, KM_NT, 0, (hipStream_t)stream>>>(x->N, km_chunks(x->N), mind, part, u, j, picks, totals, flag);
    ST_LAUNCH_CHECK();
    return 0;
}
