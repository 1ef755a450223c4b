// abx.hip -- the distance engine of the ABX phone-discrimination error: path-normalised DTW of many pairs of short items of one packed
// feature buffer, and the triple counts over finished distance matrices (contracts: st_dtw_pairs, st_abx_count, st_abx_across in
// include/semitts.h).
//
// st_dtw_pairs.  One WAVE per pair, four waves a workgroup, no workgroup barrier: a wave's pair touches only that wave's slice of LDS.
// Phase 1: the 64 lanes go over the n x m cells (lane = cell mod 64) and write the frame distances into the wave's tile in LDS; both
// rows of a cell are read by 16-byte loads and the sums run over ascending k.  For `angular` the reciprocal norm of each of the n + m
// rows is formed once (one lane a row) and kept beside the tile.  A NaN distance (a NaN among the rows; a negative probability under
// `kl`) is voted over the wave and ends the pair.  The tile has the row stride ld = m rounded up to even: in phase 2 lane i reads
// tile[i ld + c - i], consecutive lanes ld - 1 words apart, and an odd distance walks all the banks.
// Phase 2: lane i owns row i and the wave sweeps the anti-diagonals c = i + j.  D(i, j-1) is the lane's own value of the step before,
// D(i-1, j) is the value of the lane above at the step before -- it arrives by ONE DPP wave shift (wave_shr:1 rides on a v_mov; an LDS
// permute would cost its ~100 cycles on every one of the n + m - 1 dependent steps) -- and D(i-1, j-1) is what that shift delivered
// the step before that, kept in a register.  The path length travels beside the cost through the same shift, so there is no
// back-pointer table and no trace-back.  Cells that do not exist hold +inf and never win a comparison; lanes past row n - 1 and
// columns past m - 1 compute values nobody reads (a cell reads from lanes below it and columns before it only).  The distance of the
// next step is fetched from LDS before the chain of this one.
//
// st_abx_count.  One workgroup of 256 threads per block of the table; a thread takes the (X, A) pairs u = tid, tid + 256, ... and runs
// over the B of the block with d(A, X) in a register, reading row X of the symmetric matrix.  Integer partials, a shuffle reduction per
// wave, the four wave sums added by thread 0: exact and repeatable, no atomics.
//
// st_abx_across.  The across-speaker count: a group (context, speaker of A and B, a, b) against the list of label a's index ranges of
// every speaker of the context.  Groups are tiny and very many, so a group is one WAVE's work (see abx_across_kernel).
#include <math.h>
#include "st_common.h"

namespace {

constexpr int AX_WAVES = 4, AX_NT = ST_WAVE * AX_WAVES, AX_MAX_LEN = 64, AX_MAX_D = 512, AX_MAX_GRID = 1 << 20;
constexpr int AX_DPP_WAVE_SHR1 = 0x138;     // lane l reads lane l - 1 over the whole wave; lane 0 keeps `old`
constexpr int AX_CNT_NT = 256;
constexpr long long AX_MAX_NC = 1ll << 20;  // items of one cell: n_a^2 n_b stays below 2^60

__host__ __device__ inline int ax_ld(int m) { return (m + 1) & ~1; }
// floats of LDS per wave: the tile | the reciprocal norms of the n + m rows (angular)
__host__ __device__ inline size_t ax_wave_words(int max_len) { return (size_t)max_len * ax_ld(max_len) + 2 * (size_t)max_len; }

// compiler-level ordering of a wave's own LDS traffic (the hardware serves one wave's LDS instructions in order)
__device__ __forceinline__ void ax_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 1 / ||x||, 0 for a zero row
__device__ __forceinline__ float ax_rnorm(const float* __restrict__ xr, int D) {
    float s = 0.0f;
    int k = 0;
    for (; k + 4 <= D; k += 4) {
        const f32x4 a = st_ld4_u(xr + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += a[u] * a[u];
    }
    for (; k < D; ++k) s += xr[k] * xr[k];
    const float nrm = sqrtf(s);
    return nrm > 0.0f ? __fdiv_rn(1.0f, nrm) : (nrm != nrm ? nrm : 0.0f);
}

struct AxAcc {
    float s, t;
    bool bad;
};

template <int METRIC>
__device__ __forceinline__ void ax_term(AxAcc& acc, float x, float y, float rx, float ry) {
    if constexpr (METRIC == ST_ABX_EUCLID) {
        const float t = x - y;
        acc.s += t * t;
    } else if constexpr (METRIC == ST_ABX_ANGULAR) {
        // the unit vectors are rounded products of their own, never contracted into the difference (fma(x, rx, -v) would leave the
        // rounding error of the product where an item against itself must give 0); __fmul_rn is a plain product to the compiler
        float dm, dp;
        {
#pragma clang fp contract(off)
            const float u = x * rx, v = y * ry;
            dm = u - v;
            dp = u + v;
        }
        acc.s += dm * dm;
        acc.t += dp * dp;
    } else {
        acc.bad |= x < 0.0f || y < 0.0f;
        acc.s += (x - y) * (logf(x + 1e-10f) - logf(y + 1e-10f));
    }
}

template <int METRIC>
__device__ __forceinline__ float ax_frame_dist(const float* __restrict__ xr, const float* __restrict__ yr, int D, float rx, float ry, bool& bad) {
    AxAcc acc{0.0f, 0.0f, false};
    int k = 0;
    for (; k + 4 <= D; k += 4) {
        const f32x4 a = st_ld4_u(xr + k), c = st_ld4_u(yr + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) ax_term<METRIC>(acc, a[u], c[u], rx, ry);
    }
    for (; k < D; ++k) ax_term<METRIC>(acc, xr[k], yr[k], rx, ry);
    float d;
    if constexpr (METRIC == ST_ABX_EUCLID) d = sqrtf(acc.s);
    else if constexpr (METRIC == ST_ABX_ANGULAR) {
        d = 0.63661977236758134f * atan2f(sqrtf(acc.s), sqrtf(acc.t));
        d = d > 1.0f ? 1.0f : d;        // (not fminf: a NaN must stay one)
    } else d = 0.5f * acc.s;
    bad |= acc.bad || d != d;
    return d;
}

__device__ __forceinline__ float ax_shr1(float v, float fill) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), AX_DPP_WAVE_SHR1,
                                                                 0xf, 0xf, false));
}
__device__ __forceinline__ int ax_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, AX_DPP_WAVE_SHR1, 0xf, 0xf, false); }

template <int METRIC>
__global__ __launch_bounds__(AX_NT) void dtw_pairs_kernel(const float* __restrict__ feat, long n_rows, int D, long st,
                                                          const int32_t* __restrict__ item_start, const int32_t* __restrict__ item_len, int n_items,
                                                          const int32_t* __restrict__ pair_a, const int32_t* __restrict__ pair_b, int P, int max_len,
                                                          float* __restrict__ dist, float* __restrict__ cost, int32_t* __restrict__ path_len) {
    extern __shared__ __attribute__((aligned(16))) float ax_dyn[];
    const int lane = threadIdx.x & (ST_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* tile = ax_dyn + (size_t)wave * ax_wave_words(max_len);
    float* rn = tile + (size_t)max_len * ax_ld(max_len);
    for (long p = (long)blockIdx.x * AX_WAVES + wave; p < P; p += (long)gridDim.x * AX_WAVES) {       // (wave-uniform)
        const int a = pair_a[p], b = pair_b[p];
        bool ok = a >= 0 && a < n_items && b >= 0 && b < n_items;
        int n = 0, m = 0;
        long sa = 0, sb = 0;
        if (ok) {
            n = item_len[a]; m = item_len[b];
            sa = item_start[a]; sb = item_start[b];
            ok = n >= 1 && n <= max_len && m >= 1 && m <= max_len && sa >= 0 && sb >= 0 && sa + n <= n_rows && sb + m <= n_rows;
        }
        const int ld = ax_ld(m);
        if (ok) {
            // ---- phase 1: the n x m frame distances
            const float* xa = feat + (size_t)sa * st;
            const float* yb = feat + (size_t)sb * st;
            ax_wave_sync();         // (the sweep of the wave's previous pair has read the tile)
            if constexpr (METRIC == ST_ABX_ANGULAR) {
                for (int r = lane; r < n + m; r += ST_WAVE) rn[r] = ax_rnorm(r < n ? xa + (size_t)r * st : yb + (size_t)(r - n) * st, D);
                ax_wave_sync();
            }
            bool bad = false;
            const float rm = 1.0f / (float)m;
            for (int e = lane; e < n * m; e += ST_WAVE) {
                const int i = (int)(((float)e + 0.5f) * rm), j = e - i * m;       // (e < 4096, m <= 64: the quotient is exact)
                float rx = 0.0f, ry = 0.0f;
                if constexpr (METRIC == ST_ABX_ANGULAR) { rx = rn[i]; ry = rn[n + j]; }
                tile[i * ld + j] = ax_frame_dist<METRIC>(xa + (size_t)i * st, yb + (size_t)j * st, D, rx, ry, bad);
            }
            ok = __ballot(bad) == 0ull;
            ax_wave_sync();
        }
        float c_out = NAN;
        int l_out = 0;
        if (ok) {
            // ---- phase 2: lane i sweeps row i along the anti-diagonals; all 64 lanes run every step (the DPP shift reads its neighbour)
            const float* trow = tile + min(lane, n - 1) * ld;
            float cur = INFINITY, dg = INFINITY;       // D(i, j-1) of the step before; what the shift delivered the step before
            int curL = 0, dgL = 0;
            float dn = trow[0];
            for (int c = 0; c < n + m - 1; ++c) {
                const int j = c - lane;
                const float d = dn;
                dn = trow[min(max(j + 1, 0), m - 1)];
                const float up = ax_shr1(cur, INFINITY);
                const int upL = ax_shr1(curL, 0);
                float best = dg;
                int bl = dgL;
                if (up < best) { best = up; bl = upL; }
                if (cur < best) { best = cur; bl = curL; }
                if (c == 0 && lane == 0) { best = 0.0f; bl = 0; }
                dg = up;
                dgL = upL;
                cur = j >= 0 ? best + d : INFINITY;
                curL = bl + 1;
            }
            const int last = __builtin_amdgcn_readfirstlane(n - 1);
            c_out = st_lane(cur, last);
            l_out = __builtin_amdgcn_readlane(curL, last);
        }
        if (lane == 0) {
            dist[p] = ok ? __fdiv_rn(c_out, (float)l_out) : NAN;
            if (cost) cost[p] = c_out;
            if (path_len) path_len[p] = l_out;
        }
    }
}

template <int METRIC>
int ax_launch(int grid, size_t lds, hipStream_t s, const float* feat, long n_rows, int D, long st, const int32_t* item_start, const int32_t* item_len,
              int n_items, const int32_t* pair_a, const int32_t* pair_b, int P, int max_len, float* dist, float* cost, int32_t* path_len) {
    static size_t seen = 0;
    if (int rc = st_lds_opt_in(reinterpret_cast<const void*>(dtw_pairs_kernel<METRIC>), lds, lds > 48 * 1024, seen)) return rc;
    hipLaunchKernelGGL((dtw_pairs_kernel<METRIC>), dim3(grid), dim3(AX_NT), lds, s, feat, n_rows, D, st, item_start, item_len, n_items, pair_a,
                       pair_b, P, max_len, dist, cost, path_len);
    return 0;
}

__device__ __forceinline__ long long ax_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(AX_CNT_NT) void abx_count_kernel(const float* __restrict__ dmat, long dmat_len, const int64_t* __restrict__ blk, int NB,
                                                              int64_t* __restrict__ count) {
    __shared__ long long part[AX_CNT_NT / ST_WAVE][3];
    const int tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid >> 6;
    for (int q = blockIdx.x; q < NB; q += gridDim.x) {      // (uniform)
        const int64_t* r = blk + (size_t)q * 6;
        const long long off = r[0], nc = r[1];
        const bool ok = nc >= 0 && nc <= AX_MAX_NC && off >= 0 && off <= (long long)dmat_len && nc * nc <= (long long)dmat_len - off;
        long long wrong = 0, tied = 0, nan = 0, triples = -1;
        if (ok) {
            const long long a_lo = ax_clamp(r[2], 0, nc), a_hi = ax_clamp(r[3], 0, nc), b_lo = ax_clamp(r[4], 0, nc), b_hi = ax_clamp(r[5], 0, nc);
            const long long na = a_hi > a_lo ? a_hi - a_lo : 0, nb = b_hi > b_lo ? b_hi - b_lo : 0;
            triples = na * (na - 1) * nb;
            const float* mat = dmat + off;
            for (long long u = tid; u < na * na; u += AX_CNT_NT) {
                const long long x = u / na, a = u - x * na;
                if (a == x) continue;
                const float* row = mat + (a_lo + x) * nc;       // d(., X): the matrix is symmetric
                const float ax = row[a_lo + a];
                const bool ax_nan = ax != ax;
                for (long long b = 0; b < nb; ++b) {
                    const float bx = row[b_lo + b];
                    const bool isnan_ = ax_nan || bx != bx;
                    nan += isnan_ ? 1 : 0;
                    wrong += (!isnan_ && ax > bx) ? 1 : 0;
                    tied += (!isnan_ && ax == bx) ? 1 : 0;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                wrong += __shfl_xor(wrong, d);
                tied += __shfl_xor(tied, d);
                nan += __shfl_xor(nan, d);
            }
        }
        if (lane == 0) { part[wave][0] = wrong; part[wave][1] = tied; part[wave][2] = nan; }
        __syncthreads();
        if (tid == 0) {
            long long s[3] = {0, 0, 0};
            for (int w = 0; w < AX_CNT_NT / ST_WAVE; ++w)
                for (int k = 0; k < 3; ++k) s[k] += part[w][k];
            int64_t* o = count + (size_t)q * 4;
            o[0] = ok ? s[0] : -1; o[1] = ok ? s[1] : -1; o[2] = ok ? s[2] : -1; o[3] = triples;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double ax_lane_f64(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// One WAVE per group, four waves a workgroup, no LDS, no barrier.  A pass hands 64 / W consecutive X ranges of the group's list to
// segments of W lanes each, W the power of two that holds the widest range's n_x n_a (X, A) pairs (64, strided over, past 32 of them);
// a lane keeps d(A, X) in a register and runs over B.  The three counts of a range are summed over its segment by log2 W butterfly
// steps, the segment's first lane forms the float64 pair score, and the scores of a pass are added in lane (= range) order through
// readlane; the totals are per-lane sums reduced over the wave once per group.
__global__ __launch_bounds__(AX_NT) void abx_across_kernel(const float* __restrict__ dmat, long dmat_len, const int64_t* __restrict__ grp, int NG,
                                                           const int64_t* __restrict__ xr, long NX, double* __restrict__ err,
                                                           int64_t* __restrict__ count) {
    const int lane = threadIdx.x & (ST_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long g = (long)blockIdx.x * AX_WAVES + wave; g < NG; g += (long)gridDim.x * AX_WAVES) {       // (wave-uniform)
        const int64_t* r = grp + (size_t)g * 8;
        const long long off = r[0], nc = r[1], s_lo = r[6], s_hi = r[7];
        const bool ok = nc >= 0 && nc <= AX_MAX_NC && off >= 0 && off <= (long long)dmat_len && nc * nc <= (long long)dmat_len - off &&
                        s_lo >= 0 && s_lo <= (long long)NX && s_hi >= 0 && s_hi <= (long long)NX;
        if (!ok) {
            if (lane == 0) {
                for (int k = 0; k < 5; ++k) count[(size_t)g * 5 + k] = -1;
                err[g] = NAN;
            }
            continue;
        }
        const long long a_lo = ax_clamp(r[2], 0, nc), a_hi = ax_clamp(r[3], 0, nc), b_lo = ax_clamp(r[4], 0, nc), b_hi = ax_clamp(r[5], 0, nc);
        const long long na = a_hi > a_lo ? a_hi - a_lo : 0, nb = b_hi > b_lo ? b_hi - b_lo : 0;
        const long long nr = s_hi > s_lo ? s_hi - s_lo : 0;
        const float* mat = dmat + off;
        // the widest range of the list decides the lanes a range gets
        long long widest = 0;
        for (long long k = lane; k < nr; k += ST_WAVE) {
            const long long x_lo = ax_clamp(xr[(size_t)(s_lo + k) * 2], 0, nc), x_hi = ax_clamp(xr[(size_t)(s_lo + k) * 2 + 1], 0, nc);
            const long long nx = (x_lo == a_lo && x_hi == a_hi) || x_hi <= x_lo ? 0 : x_hi - x_lo;
            widest = nx > widest ? nx : widest;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long o = __shfl_xor(widest, d);
            widest = o > widest ? o : widest;
        }
        int lw = 6;                                         // log2 W
        if (widest * na <= 32) {
            lw = 0;
            while ((1 << lw) < (int)(widest * na)) ++lw;
        }
        lw = __builtin_amdgcn_readfirstlane(lw);
        const int W = 1 << lw, seg = lane >> lw, sl = lane & (W - 1), segs = ST_WAVE >> lw;
        long long t_wrong = 0, t_tied = 0, t_nan = 0, t_tri = 0;        // this lane's share of the group's totals
        double sum = 0.0;
        int present = 0;
        for (long long base = 0; base < nr; base += segs) {             // (uniform)
            const long long k = base + seg;
            long long x_lo = 0, nx = 0;
            if (k < nr) {
                x_lo = ax_clamp(xr[(size_t)(s_lo + k) * 2], 0, nc);
                const long long x_hi = ax_clamp(xr[(size_t)(s_lo + k) * 2 + 1], 0, nc);
                nx = (x_lo == a_lo && x_hi == a_hi) || x_hi <= x_lo ? 0 : x_hi - x_lo;      // the group's own speaker; an inverted range
            }
            const long long items = nx * na;
            long long wrong = 0, tied = 0, nan = 0;
            for (long long u = sl; u < items; u += W) {
                const long long x = items <= 0x7fffffffll ? (long long)((unsigned)u / (unsigned)na) : u / na, a = u - x * na;
                const float* row = mat + (x_lo + x) * nc;       // d(., X)
                const float ax = row[a_lo + a];
                const bool ax_nan = ax != ax;
                for (long long b = 0; b < nb; ++b) {
                    const float bx = row[b_lo + b];
                    const bool isnan_ = ax_nan || bx != bx;
                    nan += isnan_ ? 1 : 0;
                    wrong += (!isnan_ && ax > bx) ? 1 : 0;
                    tied += (!isnan_ && ax == bx) ? 1 : 0;
                }
            }
            t_wrong += wrong;
            t_tied += tied;
            t_nan += nan;
            t_tri += sl == 0 ? items * nb : 0;
            for (int d = W >> 1; d >= 1; d >>= 1) {                     // (uniform; the partners stay inside the segment)
                wrong += __shfl_xor(wrong, d);
                tied += __shfl_xor(tied, d);
                nan += __shfl_xor(nan, d);
            }
            const long long valid = items * nb - nan;
            const double score = valid > 0 ? ((double)wrong + 0.5 * (double)tied) / (double)valid : 0.0;
            unsigned long long have = __ballot(sl == 0 && valid > 0);
            while (have) {                                              // ascending lanes are ascending ranges
                const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(have));
                sum += ax_lane_f64(score, src);
                ++present;
                have &= have - 1;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            t_wrong += __shfl_xor(t_wrong, d);
            t_tied += __shfl_xor(t_tied, d);
            t_nan += __shfl_xor(t_nan, d);
            t_tri += __shfl_xor(t_tri, d);
        }
        if (lane == 0) {
            int64_t* o = count + (size_t)g * 5;
            o[0] = t_wrong; o[1] = t_tied; o[2] = t_nan; o[3] = t_tri; o[4] = present;
            err[g] = present > 0 ? sum / (double)present : (double)NAN;
        }
    }
}

}  // namespace

extern "C" int st_dtw_pairs(const float* feat, long n_rows, int D, long st, const int32_t* item_start, const int32_t* item_len, int n_items,
                            const int32_t* pair_a, const int32_t* pair_b, int P, int metric, int max_len, float* dist, float* cost,
                            int32_t* path_len, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(feat && item_start && item_len && pair_a && pair_b && dist, "st_dtw_pairs: bad arguments");
    ST_CHECK_ARG(P >= 1 && n_items >= 1 && n_rows >= 1, "st_dtw_pairs: P=%d pairs of %d items in %ld rows: at least one of each", P, n_items, n_rows);
    ST_CHECK_ARG(D >= 1 && D <= AX_MAX_D, "st_dtw_pairs: 1..%d columns (D=%d)", AX_MAX_D, D);
    ST_CHECK_ARG(st >= D, "st_dtw_pairs: row stride %ld below D = %d", st, D);
    ST_CHECK_ARG(max_len >= 1 && max_len <= AX_MAX_LEN, "st_dtw_pairs: 1..%d rows an item (max_len=%d)", AX_MAX_LEN, max_len);
    ST_CHECK_ARG(metric == ST_ABX_EUCLID || metric == ST_ABX_ANGULAR || metric == ST_ABX_KL, "st_dtw_pairs: metric %d is none of euclid (0), angular (1), kl (2)",
                 metric);
    const size_t lds = AX_WAVES * ax_wave_words(max_len) * sizeof(float);
    const long groups = ((long)P + AX_WAVES - 1) / AX_WAVES;
    const int grid = (int)(groups < AX_MAX_GRID ? groups : AX_MAX_GRID);     // (past that the waves stride over the pairs)
    hipStream_t s = (hipStream_t)stream;
    int rc;
#define AX_GO(M) rc = ax_launch<M>(grid, lds, s, feat, n_rows, D, st, item_start, item_len, n_items, pair_a, pair_b, P, max_len, dist, cost, path_len)
    if (metric == ST_ABX_EUCLID) AX_GO(ST_ABX_EUCLID);
    else if (metric == ST_ABX_ANGULAR) AX_GO(ST_ABX_ANGULAR);
    else AX_GO(ST_ABX_KL);
#undef AX_GO
    if (rc) return rc;
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_abx_count(const float* dmat, long dmat_len, const int64_t* blk, int NB, int64_t* count, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(dmat && blk && count, "st_abx_count: bad arguments");
    ST_CHECK_ARG(NB >= 1 && dmat_len >= 1, "st_abx_count: NB=%d blocks over %ld distances: at least one of each", NB, dmat_len);
    hipLaunchKernelGGL(abx_count_kernel, dim3(NB < AX_MAX_GRID ? NB : AX_MAX_GRID), dim3(AX_CNT_NT), 0, (hipStream_t)stream, dmat, dmat_len, blk, NB,
                       count);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_abx_across(const float* dmat, long dmat_len, const int64_t* grp, int NG, const int64_t* xr, long NX, double* err, int64_t* count,
                             void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(dmat && grp && xr && err && count, "st_abx_across: bad arguments");
    ST_CHECK_ARG(NG >= 1 && dmat_len >= 1 && NX >= 1, "st_abx_across: NG=%d groups and %ld X ranges over %ld distances: at least one of each", NG, NX,
                 dmat_len);
    const long wgs = ((long)NG + AX_WAVES - 1) / AX_WAVES;
    hipLaunchKernelGGL(abx_across_kernel, dim3((unsigned)(wgs < AX_MAX_GRID ? wgs : AX_MAX_GRID)), dim3(AX_NT), 0, (hipStream_t)stream, dmat, dmat_len,
                       grp, NG, xr, NX, err, count);
    ST_LAUNCH_CHECK();
    return 0;
}
