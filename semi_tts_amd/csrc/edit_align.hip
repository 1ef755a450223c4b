// edit_align.hip -- Levenshtein alignment of phone transcripts with its trace-back: correct / substituted / deleted / inserted counts,
// the aligned pairs and a confusion matrix (contract: st_edit_align in include/semitts.h).
//
// One workgroup of ONE wave per (utterance, path) pair.  The wave first compacts the reference and the hypothesis without the ignored
// ids into LDS (a ballot and a population count per 64 tokens).  It then sweeps the rows i = 1 .. n of the table (one reference token a
// row) with the hypothesis columns j = 1 .. m spread over the lanes, lane l owning the CPT consecutive columns 1 + l CPT + k.  As in
// ged_levenshtein (loss.hip) the left dependency of a row is a prefix minimum,
//   X[0] = i,  X[j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1),  D[i][j] = j + min_{k <= j} (X[k] - k),
// taken per lane in its registers and across the lanes with DPP row shifts and scalar lane reads: no barrier and no LDS permute inside
// the sweep.  Once D[i][j] is known the move of the cell is read off D[i-1][j-1], D[i-1][j] and D[i][j] -- the diagonal if it attains
// D[i][j], else the deletion (i-1, j) if that does, else the insertion (i, j-1) -- and stored at 2 bits: a lane's CPT codes fill
// CPT / 4 whole bytes, so no two lanes share a store.  The table (16 CPT bytes a row) lies in LDS when it fits beside the tokens
// (BP_LDS) and in the caller's workspace otherwise.
// Lane 0 walks the codes back from (n, m) into a reversed list in LDS; then all lanes turn the list into `ali` in forward order, count
// the four kinds with a shuffle reduction and, for path 0, add into the confusion matrix with integer atomics (exact in any order).
// Integers only: a pair's counts and alignment depend on that pair alone and are bitwise repeatable.
#include "st_common.h"

namespace {

constexpr int EA_NT = 64, EA_MAX_L = 1024, EA_MAX_V = 1024, EA_MAX_IGNORE = 64;
constexpr int EA_CPT_SMALL = 4, EA_CPT_LARGE = 16;       // columns per lane: Lh <= 256, Lh <= 1024
constexpr size_t EA_LDS_BUDGET = 160 * 1024 - 512;       // dynamic carve of the 160 KiB of a gfx950 CU; the statics below take 256 bytes

inline int ea_cpt(int Lh) { return Lh <= EA_NT * EA_CPT_SMALL ? EA_CPT_SMALL : EA_CPT_LARGE; }
// dynamic LDS: ref int64[Lr] | hyp int64[Lh] | reversed move list uint32[Lr + Lh] | move codes, Lr rows of 16 CPT bytes (BP_LDS)
inline size_t ea_fixed_bytes(int Lr, int Lh) { return 12 * ((size_t)Lr + Lh); }
inline size_t ea_bp_bytes(int Lr, int Lh) { return (size_t)Lr * 16 * ea_cpt(Lh); }
inline bool ea_bp_in_lds(int Lr, int Lh) { return ea_fixed_bytes(Lr, Lh) + ea_bp_bytes(Lr, Lh) <= EA_LDS_BUDGET; }

__device__ __forceinline__ bool ea_ignored(int64_t x, const int* ign, int n_ign) {
    for (int k = 0; k < n_ign; ++k) if (x == (int64_t)ign[k]) return true;
    return false;
}

// dst = src[0 .. len) without the ignored ids, in order; -> its length (every lane).  One wave, 64 tokens a step.
__device__ __forceinline__ int ea_compact(const int64_t* __restrict__ src, int len, const int* ign, int n_ign, int64_t* dst, int lane) {
    int cnt = 0;
    for (int base = 0; base < len; base += EA_NT) {
        const int t = base + lane;
        const bool valid = t < len;
        const int64_t x = valid ? src[t] : 0;
        const bool keep = valid && !ea_ignored(x, ign, n_ign);
        const unsigned long long mask = __ballot(keep);
        if (keep) dst[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = x;
        cnt += __popcll(mask);
    }
    return cnt;
}

// Lane-to-lane moves of the sweep on the VALU itself (DPP row shifts inside a row of 16 lanes, a scalar lane read across the rows)
// instead of LDS permutes, whose latency a lone wave cannot hide: the row sweep is one dependent chain.  All 64 lanes must be active.
constexpr int EA_DPP_ROW_SHR1 = 0x111, EA_DPP_ROW_SHR2 = 0x112, EA_DPP_ROW_SHR4 = 0x114, EA_DPP_ROW_SHR8 = 0x118;

template <int CTRL>
__device__ __forceinline__ int ea_row_shr(int v, int fill) {        // lane l reads lane l - k of its row; `fill` where there is none
    return __builtin_amdgcn_update_dpp(fill, v, CTRL, 0xf, 0xf, false);
}

// the value of lane - 1; `fill` in lane 0
__device__ __forceinline__ int ea_shift1(int v, int fill, int lane) {
    int y = ea_row_shr<EA_DPP_ROW_SHR1>(v, fill);
    const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31), c = __builtin_amdgcn_readlane(v, 47);
    y = lane == 16 ? a : y;
    y = lane == 32 ? b : y;
    y = lane == 48 ? c : y;
    return y;
}

// inclusive prefix minimum over the 64 lanes
__device__ __forceinline__ int ea_scan_min(int v, int lane) {
    v = min(v, ea_row_shr<EA_DPP_ROW_SHR1>(v, INT_MAX));
    v = min(v, ea_row_shr<EA_DPP_ROW_SHR2>(v, INT_MAX));
    v = min(v, ea_row_shr<EA_DPP_ROW_SHR4>(v, INT_MAX));
    v = min(v, ea_row_shr<EA_DPP_ROW_SHR8>(v, INT_MAX));
    const int a = __builtin_amdgcn_readlane(v, 15), b = min(a, __builtin_amdgcn_readlane(v, 31)), c = min(b, __builtin_amdgcn_readlane(v, 47));
    const int row = lane >> 4;
    return min(v, row == 0 ? INT_MAX : row == 1 ? a : row == 2 ? b : c);
}

template <int CPT, bool BP_LDS>
__global__ __launch_bounds__(EA_NT) void edit_align_kernel(const int64_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int N, int Lh,
                                                           const int64_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int Lr,
                                                           const int32_t* __restrict__ ignore, int n_ignore, int V, int32_t* __restrict__ counts,
                                                           int32_t* __restrict__ ali_len, int32_t* __restrict__ ali, int32_t* confusion,
                                                           unsigned char* ws) {
    static_assert(CPT % 4 == 0 && CPT <= 16, "a lane's codes fill whole bytes of one 32-bit word");
    constexpr int RB = 16 * CPT;                    // bytes of move codes per row
    extern __shared__ __attribute__((aligned(16))) unsigned char ea_dyn[];
    __shared__ int ign[EA_MAX_IGNORE];
    __shared__ int s_plen;
    const int p = blockIdx.x, b = p / N, lane = threadIdx.x;
    int64_t* rs = reinterpret_cast<int64_t*>(ea_dyn);
    int64_t* hs = rs + Lr;
    unsigned* list = reinterpret_cast<unsigned*>(hs + Lh);
    unsigned char* bp = BP_LDS ? reinterpret_cast<unsigned char*>(list + Lr + Lh) : ws + (size_t)p * Lr * RB;
    for (int k = lane; k < n_ignore; k += EA_NT) ign[k] = ignore[k];
    __syncthreads();
    const int rl = ref_len ? min(max(ref_len[b], 0), Lr) : Lr;
    const int hl = min(max(hyp_len[p], 0), Lh);
    const int n = ea_compact(ref + (size_t)b * Lr, rl, ign, n_ignore, rs, lane);
    const int m = ea_compact(hyp + (size_t)p * Lh, hl, ign, n_ignore, hs, lane);
    __syncthreads();

    // ---- the sweep: D[k] = D(i, j), j = 1 + lane CPT + k.  Columns past m hold values nobody reads (a cell depends on columns <= j only).
    if (n > 0 && m > 0) {       // (uniform)
        int D[CPT];
        int64_t h[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int j = 1 + lane * CPT + k;
            D[k] = j;                                             // row 0: j insertions
            h[k] = j <= m ? hs[j - 1] : 0;
        }
        int64_t rn = rs[0];
        for (int i = 1; i <= n; ++i) {
            const int64_t r = rn;
            rn = rs[min(i, n - 1)];                               // (the next row's token: its LDS latency hides behind this row)
            const int left = ea_shift1(D[CPT - 1], i - 1, lane);  // D(i-1, j - 1) of this lane's first column; column 0 for lane 0
            int pm = INT_MAX, Y[CPT], dg[CPT];
            int prev = left;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int j = 1 + lane * CPT + k;
                dg[k] = prev + (r != h[k] ? 1 : 0);
                const int X = min(dg[k], D[k] + 1);
                prev = D[k];
                pm = min(pm, X - j);
                Y[k] = pm;                                        // inclusive prefix minimum within the lane
            }
            const int s = ea_scan_min(pm, lane);                  // inclusive prefix minimum over the lanes
            const int e = min(ea_shift1(s, INT_MAX, lane), i);    // ... exclusive, with X[0] - 0 = i of column 0
            unsigned word = 0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int v = 1 + lane * CPT + k + min(e, Y[k]);
                const unsigned code = dg[k] == v ? 0u : (D[k] + 1 == v ? 1u : 2u);       // diagonal, then (i-1, j), then (i, j-1)
                word |= code << (2 * k);
                D[k] = v;
            }
            unsigned char* row = bp + (size_t)(i - 1) * RB;
            if constexpr (CPT == 4) row[lane] = (unsigned char)word;
            else reinterpret_cast<unsigned*>(row)[lane] = word;   // (CPT = 16: little-endian, column 1 + 16 lane + k in byte k / 4)
        }
    }
    __syncthreads();            // (also publishes the workspace form's codes to lane 0)

    // ---- the trace-back from (n, m): entry = move | i << 2 | j << 13 of the cell the move leaves (move 0 diagonal, 1 deletion, 2 insertion)
    if (lane == 0) {
        int i = n, j = m, P = 0;
        while ((i > 0 || j > 0) && P < n + m) {     // (at most n + m moves; each one lowers i + j)
            unsigned mv;
            if (i == 0) mv = 2u;
            else if (j == 0) mv = 1u;
            else mv = (bp[(size_t)(i - 1) * RB + ((j - 1) >> 2)] >> (2 * ((j - 1) & 3))) & 3u;
            if (mv == 3u) mv = 2u;                  // (never stored)
            list[P++] = mv | ((unsigned)i << 2) | ((unsigned)j << 13);
            if (mv != 2u) --i;
            if (mv != 1u) --j;
        }
        s_plen = P;
    }
    __syncthreads();
    const int P = s_plen;

    // ---- forward order: the aligned pairs, the four counts, the confusion cells of path 0
    const int AL = Lr + Lh;
    int32_t* ab = ali ? ali + (size_t)p * AL * 2 : nullptr;
    int32_t* cf = (confusion && p % N == 0) ? confusion : nullptr;
    int c_ok = 0, c_sub = 0, c_del = 0, c_ins = 0;
    for (int q = lane; q < AL; q += EA_NT) {
        int32_t rt = -1, ht = -1;
        if (q < P) {
            const unsigned e = list[P - 1 - q];
            const unsigned mv = e & 3u;
            const int i = (int)((e >> 2) & 0x7ffu), j = (int)(e >> 13);
            const int64_t r64 = mv != 2u ? rs[i - 1] : 0, h64 = mv != 1u ? hs[j - 1] : 0;
            int row = V, col = V;                   // the gap's row / column
            bool in = true;
            if (mv != 2u) { rt = (int32_t)r64; in = in && r64 >= 0 && r64 < V; row = (int)r64; }
            if (mv != 1u) { ht = (int32_t)h64; in = in && h64 >= 0 && h64 < V; col = (int)h64; }
            if (mv == 0u) { if (r64 == h64) ++c_ok; else ++c_sub; }
            else if (mv == 1u) ++c_del;
            else ++c_ins;
            if (cf && in) atomicAdd(cf + (size_t)row * (V + 1) + col, 1);
        }
        if (ab) { ab[2 * q] = rt; ab[2 * q + 1] = ht; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c_ok += __shfl_xor(c_ok, d);
        c_sub += __shfl_xor(c_sub, d);
        c_del += __shfl_xor(c_del, d);
        c_ins += __shfl_xor(c_ins, d);
    }
    if (lane == 0) {
        int32_t* cb = counts + (size_t)p * 4;
        cb[0] = c_ok; cb[1] = c_sub; cb[2] = c_del; cb[3] = c_ins;
        ali_len[p] = P;
    }
}

template <int CPT, bool BP_LDS>
int ea_launch(size_t lds, int pairs, hipStream_t st, const int64_t* hyp, const int32_t* hyp_len, int N, int Lh, const int64_t* ref,
              const int32_t* ref_len, int Lr, const int32_t* ignore, int n_ignore, int V, int32_t* counts, int32_t* ali_len, int32_t* ali,
              int32_t* confusion, unsigned char* ws) {
    static size_t seen = 0;
    if (int rc = st_lds_opt_in(reinterpret_cast<const void*>(edit_align_kernel<CPT, BP_LDS>), lds, lds > 48 * 1024, seen)) return rc;
    hipLaunchKernelGGL((edit_align_kernel<CPT, BP_LDS>), dim3(pairs), dim3(EA_NT), lds, st, hyp, hyp_len, N, Lh, ref, ref_len, Lr, ignore,
                       n_ignore, V, counts, ali_len, ali, confusion, ws);
    return 0;
}

}  // namespace

extern "C" size_t st_edit_align_workspace_bytes(int pairs, int Lr, int Lh) {
    if (pairs <= 0 || Lr <= 0 || Lh <= 0 || Lr > EA_MAX_L || Lh > EA_MAX_L || ea_bp_in_lds(Lr, Lh)) return 0;
    return (size_t)pairs * ea_bp_bytes(Lr, Lh);
}

extern "C" int st_edit_align(const int64_t* hyp, const int32_t* hyp_len, int B, int N, int Lh, const int64_t* ref, const int32_t* ref_len, int Lr,
                             const int32_t* ignore, int n_ignore, int V, int32_t* counts, int32_t* ali_len, int32_t* ali, int32_t* confusion,
                             void* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(hyp && hyp_len && ref && counts && ali_len, "st_edit_align: bad arguments");
    ST_CHECK_ARG(B >= 1 && N >= 1 && (long long)B * N <= (1ll << 24), "st_edit_align: B=%d utterances of N=%d paths: at least one pair, at most %d",
                 B, N, 1 << 24);
    ST_CHECK_ARG(Lh >= 1 && Lh <= EA_MAX_L && Lr >= 1 && Lr <= EA_MAX_L, "st_edit_align: 1..%d tokens a side (Lh=%d, Lr=%d)", EA_MAX_L, Lh, Lr);
    ST_CHECK_ARG(V >= 1 && V <= EA_MAX_V, "st_edit_align: 1..%d classes (V=%d)", EA_MAX_V, V);
    ST_CHECK_ARG(n_ignore >= 0 && n_ignore <= EA_MAX_IGNORE && (n_ignore == 0 || ignore), "st_edit_align: 0..%d ignored ids", EA_MAX_IGNORE);
    const bool bp_lds = ea_bp_in_lds(Lr, Lh);
    ST_CHECK_ARG(bp_lds || ws, "st_edit_align: Lr=%d, Lh=%d needs the workspace of st_edit_align_workspace_bytes", Lr, Lh);
    const size_t lds = ea_fixed_bytes(Lr, Lh) + (bp_lds ? ea_bp_bytes(Lr, Lh) : 0);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = reinterpret_cast<unsigned char*>(ws);
    const int pairs = B * N;
    int rc;
#define EA_GO(C, P) rc = ea_launch<C, P>(lds, pairs, st, hyp, hyp_len, N, Lh, ref, ref_len, Lr, ignore, n_ignore, V, counts, ali_len, ali, confusion, w)
    if (ea_cpt(Lh) == EA_CPT_SMALL) EA_GO(EA_CPT_SMALL, true);          // (12 (Lr + Lh) + 64 Lr <= 80 KiB: always in LDS)
    else if (bp_lds) EA_GO(EA_CPT_LARGE, true);
    else EA_GO(EA_CPT_LARGE, false);
#undef EA_GO
    if (rc) return rc;
    ST_LAUNCH_CHECK();
    return 0;
}
