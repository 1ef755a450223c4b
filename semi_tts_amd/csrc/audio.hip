// audio.hip -- Griffin-Lim vocoder: linear spectrogram -> waveform (ref: src/audio.py:179-262, 274-288), and feature extraction:
// waveforms -> normalised mel / linear spectrograms, clean and augmented (ref: src/audio.py:156-177, 329-395), MFCC with derivatives
// (ref: :119-154) and the phone-segment gather (ref: :94-117)
//
// Every FFT is a real n_fft-point transform done as an (n_fft/2)-point complex Stockham FFT in LDS (radix 4, one radix-2 stage
// when log2(n_fft/2) is odd) plus the real split pass.  Twiddles e^{-2 pi i k / n_fft} come from tables computed in double on the
// host and uploaded once per device.  The time-domain state between launches is the windowed inverse FFT of every frame (its
// `win` support only): the next launch gathers the overlap-add of a frame's neighbours straight from it, so one Griffin-Lim
// iteration (iSTFT -> STFT -> phase projection) is ONE launch of one workgroup per (utterance, frame), with no atomics (every
// result is bitwise repeatable).
#include "st_common.h"
#include <limits.h>
#include <math.h>
#include <mutex>

namespace {

constexpr int GL_THREADS = 256;
constexpr int OLA_THREADS = 1024;
constexpr int OLA_CHUNK = 16;                               // samples per thread per tile of the final overlap-add + de-emphasis
constexpr int OLA_TILE = OLA_THREADS * OLA_CHUNK;
constexpr float INV_PREEMPH = 0.97f;                        // the literal of src/audio.py:276 (not data.audio.preemphasis_coeff)
constexpr float MIN_LEVEL_DB = -100.0f;                     // src/audio.py:17-18
constexpr float REF_LEVEL_DB = 20.0f;

// ------------------------------------------------------------------ twiddle tables, e^{-2 pi i k / N} for k in [0, N)
__device__ float2 g_tw512[512];
__device__ float2 g_tw1024[1024];
__device__ float2 g_tw2048[2048];
__device__ float2 g_tw4096[4096];

template <int N> __device__ __forceinline__ const float2* tw_table();
template <> __device__ __forceinline__ const float2* tw_table<512>() { return g_tw512; }
template <> __device__ __forceinline__ const float2* tw_table<1024>() { return g_tw1024; }
template <> __device__ __forceinline__ const float2* tw_table<2048>() { return g_tw2048; }
template <> __device__ __forceinline__ const float2* tw_table<4096>() { return g_tw4096; }

std::mutex g_tw_mu;
bool g_tw_done[64];

template <int N>
int upload_table(const void* sym) {
    static float2 h[N];
    for (int k = 0; k < N; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)N;
        h[k] = make_float2((float)cos(a), (float)sin(a));
    }
    ST_HIP(hipMemcpyToSymbol(sym, h, sizeof(h)));
    return 0;
}

// First use on a device uploads the four tables (a synchronous copy): that first call may not be inside a stream capture.
int ensure_twiddles(void* stream) {
    int dev = 0;
    ST_HIP(hipGetDevice(&dev));
    ST_CHECK_ARG(dev >= 0 && dev < 64, "audio: device index %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_tw_mu);
    if (g_tw_done[dev]) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    ST_HIP(hipStreamIsCapturing((hipStream_t)stream, &cs));
    ST_CHECK_ARG(cs == hipStreamCaptureStatusNone,
                 "audio: the first FFT call on a device uploads its twiddle tables and may not be captured; call once before capturing");
    int rc;
    if ((rc = upload_table<512>(HIP_SYMBOL(g_tw512))) != 0) return rc;
    if ((rc = upload_table<1024>(HIP_SYMBOL(g_tw1024))) != 0) return rc;
    if ((rc = upload_table<2048>(HIP_SYMBOL(g_tw2048))) != 0) return rc;
    if ((rc = upload_table<4096>(HIP_SYMBOL(g_tw4096))) != 0) return rc;
    g_tw_done[dev] = true;
    return 0;
}

// ------------------------------------------------------------------ complex helpers
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 cmul_negi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)
__device__ __forceinline__ float2 cmul_i(float2 a) { return make_float2(-a.y, a.x); }      // a * i

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

// In-place forward (e^{-}) M-point complex FFT of buf (LDS), natural order in and out: Stockham autosort, each butterfly's inputs
// read into registers before a barrier, outputs written after it.  tw: the N = 2M table.  Ends with a barrier.
template <int M>
__device__ __forceinline__ void fft_lds(float2* buf, const float2* __restrict__ tw) {
    constexpr int LOG2M = ilog2(M);
    const int tid = threadIdx.x;
    int Ns = 1;
    if constexpr (LOG2M & 1) {              // radix-2 first stage (Ns = 1: no twiddle)
        constexpr int NB = M / 2, PER = (NB + GL_THREADS - 1) / GL_THREADS;
        float2 v0[PER], v1[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int j = tid + p * GL_THREADS;
            if (j < NB) { v0[p] = buf[j]; v1[p] = buf[j + NB]; }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int j = tid + p * GL_THREADS;
            if (j < NB) { buf[2 * j] = cadd(v0[p], v1[p]); buf[2 * j + 1] = csub(v0[p], v1[p]); }
        }
        __syncthreads();
        Ns = 2;
    }
    constexpr int NB = M / 4, PER = (NB + GL_THREADS - 1) / GL_THREADS;
#pragma unroll
    for (int stage = 0; stage < LOG2M / 2; ++stage) {
        float2 v[PER][4];
        int jj[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int j = tid + p * GL_THREADS;
            jj[p] = j;
            if (j < NB) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[p][r] = buf[j + r * NB];
            }
        }
        __syncthreads();
        const int tstep = (2 * M) / (Ns * 4);          // table index step per (j % Ns) * r, in N units
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int j = jj[p];
            if (j < NB) {
                const int jm = j & (Ns - 1);
                if (Ns > 1) {
#pragma unroll
                    for (int r = 1; r < 4; ++r) v[p][r] = cmul(v[p][r], tw[jm * r * tstep]);
                }
                const float2 a0 = cadd(v[p][0], v[p][2]), a1 = csub(v[p][0], v[p][2]);
                const float2 a2 = cadd(v[p][1], v[p][3]), a3 = cmul_negi(csub(v[p][1], v[p][3]));
                const int o = (j - jm) * 4 + jm;
                buf[o] = cadd(a0, a2);
                buf[o + Ns] = cadd(a1, a3);
                buf[o + 2 * Ns] = csub(a0, a2);
                buf[o + 3 * Ns] = csub(a1, a3);
            }
        }
        __syncthreads();
        Ns *= 4;
    }
}

// Real split after the forward FFT of z[m] = x[2m] + i x[2m+1]: the one-sided spectrum X[k], X[M-k] of x from Z[k], Z[M-k]
// (k in [0, M/2]; k = 0 gives X[0] and X[M]).
__device__ __forceinline__ void real_split(float2 zk, float2 zc, float2 w, float2& xk, float2& xc) {
    const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
    const float2 o = make_float2(0.5f * (zk.y + zc.y), -0.5f * (zk.x - zc.x));
    const float2 wo = cmul(w, o);
    xk = cadd(e, wo);
    xc = cconj(csub(e, wo));
}

// Inverse of real_split for a C2R transform: Z'[k], Z'[M-k] from Y[k], Y[M-k] (k = 0: Y[0] and Y[M]); the caller zeroes the
// imaginary parts of Y[0] and Y[M] (irfft ignores them).  The inverse M-point FFT of Z' is x[2m] + i x[2m+1] times M.
__device__ __forceinline__ void real_merge(float2 yk, float2 yc, float2 w, float2& zk, float2& zc) {
    const float2 e = make_float2(0.5f * (yk.x + yc.x), 0.5f * (yk.y - yc.y));
    const float2 o = cmul(make_float2(0.5f * (yk.x - yc.x), 0.5f * (yk.y + yc.y)), cconj(w));
    zk = cadd(e, cmul_i(o));
    zc = cadd(cconj(e), cmul_i(cconj(o)));
}

// x index of frame t's sample n (0 <= n < N) with center=True, pad_mode='reflect' (ref: src/audio.py:234-246); L > N/2.
__device__ __forceinline__ int reflect_index(int i, int L) { return i < 0 ? -i : (i >= L ? 2 * (L - 1) - i : i); }

// Overlap-add of the windowed frames at x index i (ref: lib/istft.py conv_transpose1d + window_envelop), without the
// envelope: frames (T, win) of one utterance, frame t' covering padded positions [t' hop + left, t' hop + left + win).
__device__ __forceinline__ float ola_at(const float* __restrict__ fr, int i, int T, int hop, int win, int half, int left) {
    const int s = i + half - left;                 // >= 0 since half >= left
    const int hi = min(T - 1, s / hop);
    const int lo = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
    float acc = 0.0f;
    for (int tp = lo; tp <= hi; ++tp) acc += fr[(size_t)tp * win + (s - tp * hop)];
    return acc;
}

// Ragged batches (st_griffin_lim_batch): utterance b has nfr[b] of the T stored frames, clamped into [tmin, T] with tmin the
// fewest frames check_dims takes (hop (tmin - 1) > n_fft / 2), so whatever nfr holds, every index stays inside the storage of
// the utterance's T frames.  Storage strides stay those of T; reflect padding, overlap-add and envelope use the utterance's own.
__device__ __forceinline__ int ragged_frames(const int* __restrict__ nfr, int b, int tmin, int T) { return min(max(nfr[b], tmin), T); }

// C2R of the frame's spectrum (already merged + conjugated into buf) -> window -> frames_out.  buf holds conj(Z').
template <int N>
__device__ __forceinline__ void inverse_to_frame(float2* buf, const float2* __restrict__ tw, const float* __restrict__ wnd,
                                                 float* __restrict__ out, int win) {
    constexpr int M = N / 2;
    fft_lds<M>(buf, tw);
    const float* xr = reinterpret_cast<const float*>(buf);
    const int left = (N - win) / 2;
    const float scale = 1.0f / (float)M;          // exact (power of two)
    for (int n2 = threadIdx.x; n2 < win; n2 += GL_THREADS) {
        const int n = n2 + left;
        const float v = (n & 1) ? -xr[n] : xr[n];    // x = conj(FFT(conj(Z'))) / M
        out[n2] = v * scale * wnd[n2];
    }
}

// ------------------------------------------------------------------ setup: window and inverse envelope (double)
// wnd[n] = hann_window(win, periodic)[n] (ref: src/audio.py:35); inv_env[i] = 1 / sum_t' wpad(i + N/2 - t' hop)^2 for the
// trimmed iSTFT output i in [0, L) (ref: lib/istft.py window_envelop, trimmed by n_fft//2).
__device__ __forceinline__ float inv_envelope_at(int idx, int N, int T, int hop, int win) {
    const int half = N / 2, left = (N - win) / 2;
    const int s = idx + half - left;
    const int hi = min(T - 1, s / hop);
    const int lo = s - win + 1 <= 0 ? 0 : (s - win + hop) / hop;
    double env = 0.0;
    for (int tp = lo; tp <= hi; ++tp) {
        const double w = 0.5 - 0.5 * cospi(2.0 * (double)(s - tp * hop) / (double)win);
        env += w * w;
    }
    return (float)(1.0 / env);
}

__global__ void gl_setup_kernel(float* __restrict__ wnd, float* __restrict__ inv_env, int N, int T, int hop, int win, int L) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < win) wnd[idx] = (float)(0.5 - 0.5 * cospi(2.0 * (double)idx / (double)win));
    if (inv_env && idx < L) inv_env[idx] = inv_envelope_at(idx, N, T, hop, win);
}

// The ragged form: one envelope per utterance (its own frame count: the right edge differs), env_stride floats apart.  Grid (., B).
__global__ void gl_setup_ragged_kernel(float* __restrict__ wnd, float* __restrict__ inv_env, size_t env_stride, int N, int T, int hop,
                                       int win, const int* __restrict__ nfr, int tmin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (b == 0 && idx < win) wnd[idx] = (float)(0.5 - 0.5 * cospi(2.0 * (double)idx / (double)win));
    const int Tb = ragged_frames(nfr, b, tmin, T);
    if (idx < hop * (Tb - 1)) inv_env[b * env_stride + idx] = inv_envelope_at(idx, N, Tb, hop, win);
}

// ------------------------------------------------------------------ first iSTFT
// SRC_FEAT: Y = amp * e^{i phase} with amp from the (normalised) decoder output read through strides (the (B, T, F) -> (B, F, T)
// transpose of src/audio.py:401 and the denormalisation of :186-188, :281-288 fused here; amp is also written to amp_out as
// (B, T, F) for the iterations).  SRC_AMP: feat is that (B, T, F) magnitude already (mel_to_linear_kernel wrote it): read, not
// written again.  SRC_SPEC: Y is a complex spectrum (B, T, F, 2).  Grid (T, B).  RAGGED: frames t >= nfr[b] leave at once.
enum { SRC_SPEC = 0, SRC_FEAT = 1, SRC_AMP = 2 };

template <int N, int SRC, bool RAGGED>
__global__ __launch_bounds__(GL_THREADS) void gl_first_istft_kernel(const float* __restrict__ feat, long sb, long st, long sf,
                                                                  int normalized, float power, const float* __restrict__ phases,
                                                                  const float2* __restrict__ spec, float* __restrict__ amp_out,
                                                                  const float* __restrict__ wnd, float* __restrict__ frames, int T,
                                                                  int win, const int* __restrict__ nfr, int tmin) {
    constexpr int M = N / 2, F = M + 1;
    __shared__ float2 buf[M];
    const float2* tw = tw_table<N>();
    const int t = blockIdx.x, b = blockIdx.y;
    if constexpr (RAGGED) {
        if (t >= ragged_frames(nfr, b, tmin, T)) return;
    }
    const size_t frame = (size_t)b * T + t;
    auto load_y = [&](int k) -> float2 {
        if constexpr (SRC != SRC_SPEC) {
            float a = feat[b * sb + t * st + k * sf];
            if constexpr (SRC == SRC_FEAT) {
                if (normalized) {
                    a = MIN_LEVEL_DB + fminf(fmaxf(a, 0.0f), 1.0f) * -MIN_LEVEL_DB;     // _denormalize  (:287-288)
                    a = powf(10.0f, 0.05f * (a + REF_LEVEL_DB));                        // _db_to_amp(x + REF_LEVEL_DB)  (:187, :284)
                    if (power != 1.0f) a = powf(a, power);                               // ** power  (:188)
                }
                a = fabsf(a);                                                            // magnitude = specgram.abs()  (:217)
                amp_out[frame * F + k] = a;
            }
            const float ph = phases[((size_t)b * F + k) * T + t];
            return make_float2(a * cosf(ph), a * sinf(ph));                             // _to_complex  (:264-268)
        } else {
            return spec[frame * F + k];
        }
    };
    for (int k = threadIdx.x; k <= M / 2; k += GL_THREADS) {
        float2 yk = load_y(k), yc = load_y(M - k);
        if (k == 0) { yk.y = 0.0f; yc.y = 0.0f; }
        float2 zk, zc;
        real_merge(yk, yc, tw[k], zk, zc);
        buf[k] = cconj(zk);
        if (k != 0 && k != M / 2) buf[M - k] = cconj(zc);
    }
    __syncthreads();
    inverse_to_frame<N>(buf, tw, wnd, frames + frame * win, win);
}

// ------------------------------------------------------------------ one Griffin-Lim iteration (ref: src/audio.py:219-225)
// x = istft(Y_prev) gathered from the previous frames (overlap-add / envelope, reflect-padded), STFT frame t of x, phase
// projection Y = amp * X / |X| (angle(0) = 0: amp + 0i), then this frame of the next istft.  Grid (T, B).  RAGGED: utterance b
// has Tb = nfr[b] frames and Lb = hop (Tb - 1) samples (padding, overlap-add and envelope are its own); frames t >= Tb leave at once.
template <int N, bool RAGGED>
__global__ __launch_bounds__(GL_THREADS) void gl_iter_kernel(const float* __restrict__ frames_in, float* __restrict__ frames_out,
                                                           const float* __restrict__ amp, const float* __restrict__ wnd,
                                                           const float* __restrict__ inv_env, int T, int hop, int win, int L,
                                                           const int* __restrict__ nfr, int tmin, size_t env_stride) {
    constexpr int M = N / 2, F = M + 1, HALF = N / 2;
    __shared__ float2 buf[M];
    float* xr = reinterpret_cast<float*>(buf);
    const float2* tw = tw_table<N>();
    const int t = blockIdx.x, b = blockIdx.y;
    int Tb = T, Lb = L;
    if constexpr (RAGGED) {
        Tb = ragged_frames(nfr, b, tmin, T);
        if (t >= Tb) return;
        Lb = hop * (Tb - 1);
        inv_env += b * env_stride;
    }
    const int left = (N - win) / 2;
    const float* fr = frames_in + (size_t)b * T * win;
    for (int n = threadIdx.x; n < N; n += GL_THREADS) {
        const int nn = n - left;
        float v = 0.0f;
        if (nn >= 0 && nn < win) {
            const int i = reflect_index(t * hop + n - HALF, Lb);
            v = ola_at(fr, i, Tb, hop, win, HALF, left) * inv_env[i] * wnd[nn];
        }
        xr[n] = v;
    }
    __syncthreads();
    fft_lds<M>(buf, tw);
    const float* a = amp + ((size_t)b * T + t) * F;
    for (int k = threadIdx.x; k <= M / 2; k += GL_THREADS) {
        const int c = M - k;
        float2 xk, xc;
        real_split(buf[k], buf[c & (M - 1)], tw[k], xk, xc);
        const float ak = a[k], ac = a[c];
        const float rk = sqrtf(xk.x * xk.x + xk.y * xk.y), rc = sqrtf(xc.x * xc.x + xc.y * xc.y);
        float2 yk = rk > 0.0f ? make_float2(xk.x * (ak / rk), xk.y * (ak / rk)) : make_float2(ak, 0.0f);
        float2 yc = rc > 0.0f ? make_float2(xc.x * (ac / rc), xc.y * (ac / rc)) : make_float2(ac, 0.0f);
        if (k == 0) { yk.y = 0.0f; yc.y = 0.0f; }
        float2 zk, zc;
        real_merge(yk, yc, tw[k], zk, zc);
        buf[k] = cconj(zk);
        if (k != 0 && k != M / 2) buf[c] = cconj(zc);
    }
    __syncthreads();
    inverse_to_frame<N>(buf, tw, wnd, frames_out + ((size_t)b * T + t) * win, win);
}

// ------------------------------------------------------------------ standalone STFT (ref: src/audio.py:234-246)
// x (B, L) -> spec (B, T, F, 2), T = 1 + L / hop.  Grid (T, B).
template <int N>
__global__ __launch_bounds__(GL_THREADS) void stft_kernel(const float* __restrict__ x, float2* __restrict__ spec, int T, int hop,
                                                        int win, int L) {
    constexpr int M = N / 2, F = M + 1, HALF = N / 2;
    __shared__ float2 buf[M];
    float* xr = reinterpret_cast<float*>(buf);
    const float2* tw = tw_table<N>();
    const int t = blockIdx.x, b = blockIdx.y;
    const int left = (N - win) / 2;
    const float* xb = x + (size_t)b * L;
    for (int n = threadIdx.x; n < N; n += GL_THREADS) {
        const int nn = n - left;
        float v = 0.0f;
        if (nn >= 0 && nn < win) {
            const float w = (float)(0.5 - 0.5 * cospi(2.0 * (double)nn / (double)win));
            v = xb[reflect_index(t * hop + n - HALF, L)] * w;
        }
        xr[n] = v;
    }
    __syncthreads();
    fft_lds<M>(buf, tw);
    float2* out = spec + ((size_t)b * T + t) * F;
    for (int k = threadIdx.x; k <= M / 2; k += GL_THREADS) {
        float2 xk, xc;
        real_split(buf[k], buf[(M - k) & (M - 1)], tw[k], xk, xc);
        out[k] = xk;
        if (k != M / 2) out[M - k] = xc;
    }
}

// ------------------------------------------------------------------ final overlap-add (+ inverse pre-emphasis, clip)
// One workgroup per utterance.  x[i] = OLA(frames)[i] * inv_env[i] (ref: lib/istft.py); post & 1: y[n] = x[n] + 0.97 y[n-1]
// (scipy.signal.lfilter([1], [1, -0.97]), src/audio.py:274-276) as a blocked scan -- 16 samples per thread, an inclusive scan of
// the 1024 chunk ends, the carry of one 16384-sample tile into the next; post & 2: clip to [-1, 1] (:192).
__device__ __forceinline__ int ola_slot(int j) { return (j >> 4) * (OLA_CHUNK + 1) + (j & (OLA_CHUNK - 1)); }   // padded: no bank conflicts

// RAGGED: row b holds Lb = hop (nfr[b] - 1) samples of its own overlap-add, scan and clip, and zeros from there to L.
template <bool RAGGED>
__global__ __launch_bounds__(OLA_THREADS) void gl_ola_post_kernel(const float* __restrict__ frames, const float* __restrict__ inv_env,
                                                                 float* __restrict__ out, int N, int T, int hop, int win, int L, int post,
                                                                 const int* __restrict__ nfr, int tmin, size_t env_stride) {
    __shared__ float xs[OLA_THREADS * (OLA_CHUNK + 1)];
    __shared__ float scan[2][OLA_THREADS];
    __shared__ float carry;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int half = N / 2, left = (N - win) / 2;
    const float* fr = frames + (size_t)b * T * win;
    float* ob = out + (size_t)b * L;
    if constexpr (RAGGED) {
        T = ragged_frames(nfr, b, tmin, T);
        for (int i = hop * (T - 1) + tid; i < L; i += OLA_THREADS) ob[i] = 0.0f;
        L = hop * (T - 1);
        inv_env += b * env_stride;
    }
    const float m16 = powf(INV_PREEMPH, (float)OLA_CHUNK);
    if (tid == 0) carry = 0.0f;
    for (int base = 0; base < L; base += OLA_TILE) {
#pragma unroll 4
        for (int q = 0; q < OLA_CHUNK; ++q) {
            const int j = q * OLA_THREADS + tid, i = base + j;
            xs[ola_slot(j)] = i < L ? ola_at(fr, i, T, hop, win, half, left) * inv_env[i] : 0.0f;
        }
        __syncthreads();
        if (post & 1) {
            float y = 0.0f;
            float* mine = xs + tid * (OLA_CHUNK + 1);
#pragma unroll
            for (int q = 0; q < OLA_CHUNK; ++q) y = fmaf(INV_PREEMPH, y, mine[q]);
            // inclusive scan of the chunk ends: V_j = v_j + m16 V_{j-1}
            int cur = 0;
            scan[cur][tid] = y;
            __syncthreads();
            float mult = m16;
            for (int off = 1; off < OLA_THREADS; off <<= 1) {
                const float v = scan[cur][tid] + (tid >= off ? mult * scan[cur][tid - off] : 0.0f);
                scan[cur ^ 1][tid] = v;
                cur ^= 1;
                mult *= mult;
                __syncthreads();
            }
            const float cin = carry;
            // y just before this chunk: the scan of the chunks before it plus the tile's carry decayed over 16 * tid samples
            float yp = tid == 0 ? cin : scan[cur][tid - 1] + powf(m16, (float)tid) * cin;
#pragma unroll
            for (int q = 0; q < OLA_CHUNK; ++q) {
                yp = fmaf(INV_PREEMPH, yp, mine[q]);
                mine[q] = yp;
            }
            __syncthreads();                                   // every thread has read `carry`
            if (tid == OLA_THREADS - 1) carry = yp;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < OLA_CHUNK; ++q) {
            const int j = q * OLA_THREADS + tid, i = base + j;
            if (i < L) {
                float v = xs[ola_slot(j)];
                if (post & 2) v = fminf(fmaxf(v, -1.0f), 1.0f);
                ob[i] = v;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ mel -> linear amplitude (ref: src/audio.py:194-205)
// lin[b, t, k] = sum_m basis[m, k] a[b, t, m], basis (n_mels, F) = pinverse(filterbank)^T, a = _db_to_amp(_denormalize(mel) +
// REF_LEVEL_DB) (normalized) or mel itself.  One workgroup: MEL_TILE frames x 256 bins; the tile's a values are staged in LDS
// once, a thread keeps one accumulator per frame for its bin, so a basis element read once (coalesced along k) serves every
// frame of the tile.  Each accumulator runs over ascending m with fmaf from 0: a row's result depends on neither the tile, the
// batch nor its position in them.  Grid (ceil(F / 256), ceil(T / MEL_TILE), B).  nfr (or null): frames t >= nfr[b] are neither
// read nor written.
constexpr int MEL_TILE = 16;
constexpr int MEL_MAX = 256;

__global__ __launch_bounds__(GL_THREADS) void mel_to_linear_kernel(const float* __restrict__ mel, long sb, long st, long sm,
                                                                  const float* __restrict__ basis, float* __restrict__ lin, int T,
                                                                  int n_mels, int F, int normalized, int take_abs,
                                                                  const int* __restrict__ nfr, int tmin) {
    __shared__ __attribute__((aligned(16))) float a_s[MEL_MAX * MEL_TILE];      // [m][frame of the tile]
    const int k = blockIdx.x * GL_THREADS + threadIdx.x, t0 = blockIdx.y * MEL_TILE, b = blockIdx.z;
    const int nt = min(MEL_TILE, (nfr ? ragged_frames(nfr, b, tmin, T) : T) - t0);
    if (nt <= 0) return;                                     // (the whole workgroup: before the barrier)
    for (int idx = threadIdx.x; idx < MEL_TILE * n_mels; idx += GL_THREADS) {
        const int f = idx / n_mels, m = idx - f * n_mels;
        float a = 0.0f;
        if (f < nt) {
            a = mel[b * sb + (t0 + f) * st + m * sm];
            if (normalized) {
                a = MIN_LEVEL_DB + fminf(fmaxf(a, 0.0f), 1.0f) * -MIN_LEVEL_DB;         // the expressions of gl_first_istft_kernel
                a = powf(10.0f, 0.05f * (a + REF_LEVEL_DB));
            }
        }
        a_s[m * MEL_TILE + f] = a;
    }
    __syncthreads();
    if (k >= F) return;
    float acc[MEL_TILE];
#pragma unroll
    for (int f = 0; f < MEL_TILE; ++f) acc[f] = 0.0f;
    for (int m = 0; m < n_mels; ++m) {
        const float w = basis[(size_t)m * F + k];
        const float4* av = reinterpret_cast<const float4*>(a_s + m * MEL_TILE);
#pragma unroll
        for (int q = 0; q < MEL_TILE / 4; ++q) {
            const float4 v = av[q];
            acc[4 * q] = fmaf(w, v.x, acc[4 * q]);
            acc[4 * q + 1] = fmaf(w, v.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(w, v.z, acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(w, v.w, acc[4 * q + 3]);
        }
    }
    float* o = lin + ((size_t)b * T + t0) * F + k;
#pragma unroll
    for (int f = 0; f < MEL_TILE; ++f)
        if (f < nt) o[(size_t)f * F] = take_abs ? fabsf(acc[f]) : acc[f];
}

// ------------------------------------------------------------------ feature extraction (ref: src/audio.py:156-177, 329-395, 409-437)
// Waveforms -> normalised mel (+ linear) spectrograms, the clean framing and the augmented one (noise at an SNR, time-stretched
// win / hop) in one launch of one workgroup per (frame, utterance, framing).  The per-utterance metadata travels by value.
constexpr int FEAT_MAX_B = 64;
constexpr float AMP_FLOOR = 1e-5f;                           // _amp_to_db's minimum (:278)

struct FeatMeta {
    long off[FEAT_MAX_B];      // first sample of utterance b in the packed buffer
    int len[FEAT_MAX_B];       // its length L_b
    int awin[FEAT_MAX_B];      // augmented framing: win, hop of the stretched rate (:366-373)
    int ahop[FEAT_MAX_B];
    float snr[FEAT_MAX_B];     // dB; NaN: no noise for this utterance (:356-359)
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter (i lo, i hi, utterance, 0), key = the seed.
__device__ __forceinline__ uint4 philox4x32(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// standard normal for (seed, utterance b, sample i): Box-Muller on two 24-bit uniforms, u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ float feat_normal(unsigned long long seed, int b, long i) {
    const uint4 r = philox4x32(make_uint4((unsigned)i, (unsigned)(i >> 32), (unsigned)b, 0u),
                               make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const float u1 = (float)((r.x >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__global__ void feat_noise_kernel(float* __restrict__ out, long n, int b, unsigned long long seed) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = feat_normal(seed, b, i);
}

// The power sums of snr_coeff (:434-437): sum x^2 and sum n^2 of utterance b in POW_PARTS fixed slices, one workgroup each,
// fixed-order double sums into part[(b * POW_PARTS + p) * 2 + {0, 1}]; the frame kernel adds the slices in order (feat_coeff).
// No atomics: deterministic.  The generator is keyed on utt0 + b, the utterance's position in the whole batch (meta and `part`
// are relative to this call's first utterance).
constexpr int POW_THREADS = 256;
constexpr int POW_PARTS = 64;
__global__ __launch_bounds__(POW_THREADS) void feat_power_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                                 unsigned long long seed, int utt0, FeatMeta meta, double* __restrict__ part) {
    __shared__ double sx[POW_THREADS], sn[POW_THREADS];
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long off = meta.off[b];
    const int L = meta.len[b];
    const int chunk = (L + POW_PARTS - 1) / POW_PARTS;
    const int i0 = p * chunk, i1 = min(L, i0 + chunk);
    double ax = 0.0, an = 0.0;
    if (!isnan(meta.snr[b])) {
        for (int i = i0 + tid; i < i1; i += POW_THREADS) {
            const double v = x[off + i];
            const double n = noise ? (double)noise[off + i] : (double)feat_normal(seed, utt0 + b, i);
            ax += v * v;
            an += n * n;
        }
    }
    sx[tid] = ax;
    sn[tid] = an;
    __syncthreads();
    for (int s = POW_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sx[tid] += sx[tid + s];
            sn[tid] += sn[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[((size_t)b * POW_PARTS + p) * 2] = sx[0];
        part[((size_t)b * POW_PARTS + p) * 2 + 1] = sn[0];
    }
}

// coeff = sqrt(sum x^2 / sum n^2 * 10^(-snr / 10)); 0 without noise
__device__ __forceinline__ float feat_coeff(const double* __restrict__ part, int b, float snr) {
    if (isnan(snr)) return 0.0f;
    double ax = 0.0, an = 0.0;
    for (int p = 0; p < POW_PARTS; ++p) {
        ax += part[((size_t)b * POW_PARTS + p) * 2];
        an += part[((size_t)b * POW_PARTS + p) * 2 + 1];
    }
    return an > 0.0 ? (float)sqrt(ax / an * pow(10.0, -0.1 * (double)snr)) : 0.0f;
}

// clamp((20 log10(max(a, 1e-5)) - REF_LEVEL_DB - MIN_LEVEL_DB) / -MIN_LEVEL_DB, 0, 1)    (_amp_to_db, _normalize: :278-285)
__device__ __forceinline__ float feat_norm_db(float a) {
    const float db = 20.0f * log10f(fmaxf(a, AMP_FLOOR)) - REF_LEVEL_DB;
    return fminf(fmaxf((db - MIN_LEVEL_DB) / -MIN_LEVEL_DB, 0.0f), 1.0f);
}

// The three steps a feature frame shares (features_kernel, mfcc_frame_kernel).  frame_load: frame t (centre, reflect padding at L)
// of the pre-emphasised signal y[i] = s[i] - c s[i-1], s = sample(i), under the periodic Hann window of `win` centred in N -> xr[N].
template <int N, class Sample>
__device__ __forceinline__ void frame_load(float* xr, Sample sample, float c, int t, int win, int hop, int L) {
    const int left = (N - win) / 2;
    for (int n = threadIdx.x; n < N; n += GL_THREADS) {
        const int nn = n - left;
        float v = 0.0f;
        if (nn >= 0 && nn < win) {
            const float w = (float)(0.5 - 0.5 * cospi(2.0 * (double)nn / (double)win));
            const int i = reflect_index(t * hop + n - N / 2, L);
            const float y = i == 0 ? sample(0) : fmaf(-c, sample(i - 1), sample(i));     // _preemphasis (:228-232)
            v = y * w;
        }
        xr[n] = v;
    }
    __syncthreads();
}

// |X[k]|, k <= N / 2, of the real frame in buf -> mag.  Ends with a barrier.
template <int N>
__device__ __forceinline__ void frame_magnitudes(float2* buf, const float2* __restrict__ tw, float* mag) {
    constexpr int M = N / 2;
    fft_lds<M>(buf, tw);
    for (int k = threadIdx.x; k <= M / 2; k += GL_THREADS) {
        float2 xk, xc;
        real_split(buf[k], buf[(M - k) & (M - 1)], tw[k], xk, xc);
        mag[k] = sqrtf(xk.x * xk.x + xk.y * xk.y);
        if (k != M / 2) mag[M - k] = sqrtf(xc.x * xc.x + xc.y * xc.y);
    }
    __syncthreads();
}

// normalised mel m of the magnitudes mag[F]: the band's fmaf chain in ascending bin order
__device__ __forceinline__ float band_mel(const float* mag, int F, int m, const int* __restrict__ fb_start, const int* __restrict__ fb_cnt,
                                          const int* __restrict__ fb_off, const float* __restrict__ fb_w) {
    const int k0 = min(max(fb_start[m], 0), F), cnt = min(fb_cnt[m], F - k0);           // (a malformed band reads nothing outside mag)
    const float* w = fb_w + fb_off[m];
    float a = 0.0f;
    for (int j = 0; j < cnt; ++j) a = fmaf(mag[k0 + j], w[j], a);
    return feat_norm_db(a);
}

// Grid (max(T_pad, Ta_pad), B, 1 or 2).  z = 0: the clean framing (win, hop) -> mel (B, T_pad, n_mels) and linear (B, T_pad, F)
// when non-null; z = 1: the augmented framing (meta.awin / ahop, noise times coeff[b]) -> aug (B, Ta_pad, n_mels).  Frame t of
// utterance b is the torch.stft frame (centre, reflect padding at L_b) of y[i] = s[i] - c s[i-1], s = x + coeff n; frames
// t >= 1 + L_b / hop are written as 0 (SPEC_PAD_VALUE).  Mel m sums mag[fb_start[m] + j] * fb_w[fb_off[m] + j], j < fb_cnt[m].
template <int N>
__global__ __launch_bounds__(GL_THREADS) void features_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                            unsigned long long seed, int utt0, const double* __restrict__ part, FeatMeta meta,
                                                            float c, int win, int hop, const int* __restrict__ fb_start,
                                                            const int* __restrict__ fb_cnt, const int* __restrict__ fb_off,
                                                            const float* __restrict__ fb_w, int n_mels, float* __restrict__ mel,
                                                            float* __restrict__ linear, float* __restrict__ aug, int T_pad, int Ta_pad) {
    constexpr int M = N / 2, F = M + 1;
    __shared__ float2 buf[M];
    __shared__ float mag[F];
    float* xr = reinterpret_cast<float*>(buf);
    const float2* tw = tw_table<N>();
    const int t = blockIdx.x, b = blockIdx.y;
    const bool is_aug = blockIdx.z == 1;
    const int Tp = is_aug ? Ta_pad : T_pad;
    if (t >= Tp) return;
    const int L = meta.len[b];
    if (is_aug) {
        win = meta.awin[b];
        hop = meta.ahop[b];
    }
    float* mrow = (is_aug ? aug : mel) + ((size_t)b * Tp + t) * n_mels;
    float* lrow = is_aug || !linear ? nullptr : linear + ((size_t)b * Tp + t) * F;
    if (t >= 1 + L / hop) {                                  // padding frame
        for (int m = threadIdx.x; m < n_mels; m += GL_THREADS) mrow[m] = 0.0f;
        if (lrow)
            for (int k = threadIdx.x; k < F; k += GL_THREADS) lrow[k] = 0.0f;
        return;
    }
    const float* xb = x + meta.off[b];
    const float* nb = noise ? noise + meta.off[b] : nullptr;
    __shared__ float cn_s;
    if (threadIdx.x == 0) cn_s = is_aug && part ? feat_coeff(part, b, meta.snr[b]) : 0.0f;
    __syncthreads();
    const float cn = cn_s;
    auto sample = [&](int i) -> float {                      // x + coeff n (add_noise, :411-416)
        float v = xb[i];
        if (cn != 0.0f) v = fmaf(cn, nb ? nb[i] : feat_normal(seed, utt0 + b, i), v);
        return v;
    };
    frame_load<N>(xr, sample, c, t, win, hop, L);
    frame_magnitudes<N>(buf, tw, mag);
    if (lrow)
        for (int k = threadIdx.x; k < F; k += GL_THREADS) lrow[k] = feat_norm_db(mag[k]);
    for (int m = threadIdx.x; m < n_mels; m += GL_THREADS) mrow[m] = band_mel(mag, F, m, fb_start, fb_cnt, fb_off, fb_w);
}

template <int N>
void launch_features(const float* x, const float* noise, unsigned long long seed, int utt0, const double* part, const FeatMeta& meta, float c,
                     int win, int hop, const int* fs, const int* fc, const int* fo, const float* fw, int n_mels, float* mel,
                     float* linear, float* aug, int B, int T_pad, int Ta_pad, hipStream_t s) {
    const dim3 grid(max(T_pad, aug ? Ta_pad : 0), B, aug ? 2 : 1);
    hipLaunchKernelGGL((features_kernel<N>), grid, dim3(GL_THREADS), 0, s, x, noise, seed, utt0, part, meta, c, win, hop, fs, fc, fo, fw,
                       n_mels, mel, linear, aug, T_pad, Ta_pad);
}

// ------------------------------------------------------------------ MFCC (ref: src/audio.py:119-154)
// 39 = 3 * n_mfcc columns per frame: the first n_mfcc cepstra of the NORMALISED mel (librosa.feature.mfcc(S=mel): the orthonormal
// DCT-II over the mel axis, tabulated by the host as dct (n_mfcc, n_mels)), then their first and second Savitzky-Golay derivatives
// over 9 frames (librosa.feature.delta, order 1 and 2).  Two launches: the frame kernel (the FFT, mel and cepstra of one frame per
// workgroup, the frame loop of features_kernel without noise) and the delta kernel over (B, T, n_mfcc), which reads the cepstra
// columns the first wrote and writes the two derivative columns.
struct MfccMeta {
    long off[FEAT_MAX_B];      // first sample of utterance b in the packed buffer
    int len[FEAT_MAX_B];       // its length L_b
};

constexpr int DELTA_HALF = 4;                                // the 9-frame window of librosa.feature.delta
// savgol_coeffs(9, polyorder = deriv = 1) = j / 60 and (9, 2, 2) = (28, 7, -8, -17, -20, -17, -8, 7, 28) / 462, in ascending frame order
__constant__ float DELTA_W1[2 * DELTA_HALF + 1] = {(float)(-4.0 / 60), (float)(-3.0 / 60), (float)(-2.0 / 60), (float)(-1.0 / 60), 0.0f,
                                                   (float)(1.0 / 60),  (float)(2.0 / 60),  (float)(3.0 / 60),  (float)(4.0 / 60)};
__constant__ float DELTA_W2[2 * DELTA_HALF + 1] = {(float)(28.0 / 462),  (float)(7.0 / 462),   (float)(-8.0 / 462),
                                                   (float)(-17.0 / 462), (float)(-20.0 / 462), (float)(-17.0 / 462),
                                                   (float)(-8.0 / 462),  (float)(7.0 / 462),   (float)(28.0 / 462)};

// Grid (T_pad, B).  Frame t of utterance b as in features_kernel (z = 0) at the MFCC framing (win, hop); the normalised mel row
// stays in LDS (and goes to mel_out (B, T_pad, n_mels) when non-null); out[b, t, k] = sum_m dct[k, m] mel[m], k < n_mfcc, one fmaf
// chain over ascending m.  Frames t >= 1 + L_b / hop: all 3 n_mfcc columns (and the mel row) written as 0.
template <int N>
__global__ __launch_bounds__(GL_THREADS) void mfcc_frame_kernel(const float* __restrict__ x, MfccMeta meta, float c, int win, int hop,
                                                              const int* __restrict__ fb_start, const int* __restrict__ fb_cnt,
                                                              const int* __restrict__ fb_off, const float* __restrict__ fb_w, int n_mels,
                                                              const float* __restrict__ dct, int n_mfcc, float* __restrict__ out,
                                                              float* __restrict__ mel_out, int T_pad) {
    constexpr int M = N / 2, F = M + 1;
    __shared__ float2 buf[M];
    __shared__ float mag[F];
    __shared__ float mels[MEL_MAX];
    float* xr = reinterpret_cast<float*>(buf);
    const float2* tw = tw_table<N>();
    const int t = blockIdx.x, b = blockIdx.y;
    const int L = meta.len[b];
    float* orow = out + ((size_t)b * T_pad + t) * (3 * n_mfcc);
    float* mrow = mel_out ? mel_out + ((size_t)b * T_pad + t) * n_mels : nullptr;
    if (t >= 1 + L / hop) {                                  // padding frame
        for (int k = threadIdx.x; k < 3 * n_mfcc; k += GL_THREADS) orow[k] = 0.0f;
        if (mrow)
            for (int m = threadIdx.x; m < n_mels; m += GL_THREADS) mrow[m] = 0.0f;
        return;
    }
    const float* xb = x + meta.off[b];
    frame_load<N>(xr, [&](int i) -> float { return xb[i]; }, c, t, win, hop, L);
    frame_magnitudes<N>(buf, tw, mag);
    for (int m = threadIdx.x; m < n_mels; m += GL_THREADS) {
        const float v = band_mel(mag, F, m, fb_start, fb_cnt, fb_off, fb_w);
        mels[m] = v;
        if (mrow) mrow[m] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_mfcc; k += GL_THREADS) {
        const float* d = dct + (size_t)k * n_mels;
        float a = 0.0f;
        for (int m = 0; m < n_mels; ++m) a = fmaf(d[m], mels[m], a);
        orow[k] = a;
    }
}

// Grid (ceil(T_pad n_mfcc / 256), B), after mfcc_frame_kernel on the same stream.  delta[t] = sum_j W1[j] c[tc + j - 4] and
// delta2[t] = sum_j W2[j] c[tc + j - 4] with tc = min(max(t, 4), T_b - 5): scipy's savgol_filter(mode='interp') fits the edge
// polynomial of degree = deriv order to the outermost window, whose derivative of that order is the constant the centred window
// gives.  T_b >= 9 (the entry point refuses less).  Reads columns [0, n_mfcc), writes [n_mfcc, 3 n_mfcc) of frames t < T_b.
__global__ __launch_bounds__(256) void mfcc_delta_kernel(float* __restrict__ out, MfccMeta meta, int hop, int n_mfcc, int T_pad) {
    const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int t = idx / n_mfcc, k = idx - t * n_mfcc;
    const int Tb = min(1 + meta.len[b] / hop, T_pad);
    if (t >= Tb || Tb < 2 * DELTA_HALF + 1) return;
    const int W = 3 * n_mfcc;
    const int tc = min(max(t, DELTA_HALF), Tb - 1 - DELTA_HALF);
    const float* cp = out + ((size_t)b * T_pad + tc - DELTA_HALF) * W + k;
    float d1 = 0.0f, d2 = 0.0f;
#pragma unroll
    for (int j = 0; j <= 2 * DELTA_HALF; ++j) {
        const float v = cp[(size_t)j * W];
        d1 = fmaf(DELTA_W1[j], v, d1);
        d2 = fmaf(DELTA_W2[j], v, d2);
    }
    float* orow = out + ((size_t)b * T_pad + t) * W;
    orow[n_mfcc + k] = d1;
    orow[2 * n_mfcc + k] = d2;
}

template <int N>
void launch_mfcc_frames(const float* x, const MfccMeta& meta, float c, int win, int hop, const int* fs, const int* fc, const int* fo,
                        const float* fw, int n_mels, const float* dct, int n_mfcc, float* out, float* mel_out, int B, int T_pad, hipStream_t s) {
    hipLaunchKernelGGL((mfcc_frame_kernel<N>), dim3(T_pad, B), dim3(GL_THREADS), 0, s, x, meta, c, win, hop, fs, fc, fo, fw, n_mels, dct,
                       n_mfcc, out, mel_out, T_pad);
}

// ------------------------------------------------------------------ phone segments (ref: src/audio.py:94-117)
// out (S, max_len, D) contiguous: row i < seg_len[s] of segment s = feat[seg_utt[s], seg_start[s] + i, :], every other row 0.
// One thread per four consecutive floats of the flat output (one 16-byte store; the last thread stores the 1 .. 3 left over one by
// one), whatever D is: a quad may straddle rows.  The utterance and frame indices are clamped into feat.
__global__ __launch_bounds__(256) void segment_gather_kernel(const float* __restrict__ feat, long sb, long st, int B, int T_pad, int D,
                                                            const int* __restrict__ seg_utt, const int* __restrict__ seg_start,
                                                            const int* __restrict__ seg_len, long total, int max_len,
                                                            float* __restrict__ out) {
    const long e0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= total) return;
    long row = e0 / D;
    int d = (int)(e0 - row * D);
    const float* src = nullptr;                              // the feat row of output row `row`; null: a padding row
    auto open_row = [&](long r) {
        const int s = (int)(r / max_len), i = (int)(r - (long)s * max_len);
        src = nullptr;
        if (i < seg_len[s]) {
            const int u = min(max(seg_utt[s], 0), B - 1);
            const long tt = min(max((long)seg_start[s] + i, 0L), (long)T_pad - 1);
            src = feat + u * sb + tt * st;
        }
    };
    open_row(row);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n = (int)min(4L, total - e0);
    for (int r = 0; r < n; ++r) {
        v[r] = src ? src[d] : 0.0f;
        if (++d == D && r + 1 < n) {
            d = 0;
            open_row(++row);
        }
    }
    if (n == 4) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int r = 0; r < n; ++r) out[e0 + r] = v[r];
    }
}

// ------------------------------------------------------------------ host side
struct GlDims {
    int N, hop, win, T, L;
};

size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }
constexpr size_t WND_FLOATS = 4096;

// Supported: n_fft a power of two in [512, 4096] and 0 < 2 hop <= win <= n_fft (every output sample then has a frame whose window
// is non-zero there: the envelope never vanishes).  `who`: the entry point, for the message.
int check_framing(const char* who, int n_fft, int hop, int win) {
    ST_CHECK_ARG(n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096,
                 "%s: n_fft %d not supported (512, 1024, 2048, 4096)", who, n_fft);
    ST_CHECK_ARG(hop > 0 && win <= n_fft && 2 * hop <= win,
                 "%s: need 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)", who, hop, win, n_fft);
    return 0;
}

// The STFT family: a supported framing, at least two frames, and a signal of L > n_fft / 2 samples (reflect padding, as torch requires).
int check_dims(const char* what, int B, int n_fft, int hop, int win, int T, long L) {
    const int rc = check_framing(what, n_fft, hop, win);
    if (rc) return rc;
    ST_CHECK_ARG(B > 0 && B <= 65535 && T >= 2 && (long)T * B * 4096 < (1L << 40), "%s: bad batch %d / frames %d", what, B, T);
    ST_CHECK_ARG(L > n_fft / 2 && L < (1L << 30),
                 "%s: reflect padding needs more than n_fft / 2 = %d samples (T %d frames, hop %d: %ld)", what, n_fft / 2, T, hop, L);
    return 0;
}

// The first iSTFT from `src`.  SRC_SPEC: feat is the complex spectrum (B, T, F, 2) and nothing else is read.  SRC_FEAT: feat through
// its strides, the magnitude also written to amp.  SRC_AMP: the magnitude is in amp already (B, T, F).  frames (null: T for every
// utterance) picks the ragged kernels; the uniform ones take no tmin.
template <int N>
void launch_first(int src, const float* feat, long sb, long st, long sf, int normalized, float power, const float* phases, float* amp,
                  const float* wnd, float* fr, int B, int T, int win, const int* frames, int tmin, hipStream_t s) {
    constexpr long F = N / 2 + 1;
    const float2* spec = src == SRC_SPEC ? (const float2*)feat : nullptr;
    if (src == SRC_SPEC) feat = nullptr;
    if (src == SRC_AMP) feat = amp, amp = nullptr, sb = T * F, st = F, sf = 1, normalized = 0, power = 1.0f;
    auto* kernel = src == SRC_SPEC   ? gl_first_istft_kernel<N, SRC_SPEC, false>
                   : src == SRC_FEAT ? (frames ? gl_first_istft_kernel<N, SRC_FEAT, true> : gl_first_istft_kernel<N, SRC_FEAT, false>)
                                     : (frames ? gl_first_istft_kernel<N, SRC_AMP, true> : gl_first_istft_kernel<N, SRC_AMP, false>);
    hipLaunchKernelGGL(kernel, dim3(T, B), dim3(GL_THREADS), 0, s, feat, sb, st, sf, normalized, power, phases, spec, amp, wnd, fr, T, win,
                       frames, frames ? tmin : 0);
}

template <int N>
void launch_iter(const float* fin, float* fout, const float* amp, const float* wnd, const float* inv_env, int B, int T, int hop, int win,
                 int L, const int* frames, int tmin, size_t env_stride, hipStream_t s) {
    auto* kernel = frames ? gl_iter_kernel<N, true> : gl_iter_kernel<N, false>;
    hipLaunchKernelGGL(kernel, dim3(T, B), dim3(GL_THREADS), 0, s, fin, fout, amp, wnd, inv_env, T, hop, win, L, frames,
                       frames ? tmin : 0, frames ? env_stride : (size_t)0);
}

void launch_mel_to_linear(const float* mel, long sb, long st, long sm, const float* basis, float* lin, int B, int T, int n_mels, int F,
                          int normalized, int take_abs, const int* nfr, int tmin, hipStream_t s) {
    const dim3 grid((F + GL_THREADS - 1) / GL_THREADS, (T + MEL_TILE - 1) / MEL_TILE, B);
    hipLaunchKernelGGL(mel_to_linear_kernel, grid, dim3(GL_THREADS), 0, s, mel, sb, st, sm, basis, lin, T, n_mels, F, normalized,
                       take_abs, nfr, tmin);
}

#define ST_AUDIO_DISPATCH(n_fft, F, ...) \
    switch (n_fft) {                     \
        case 512: F<512>(__VA_ARGS__); break;   \
        case 1024: F<1024>(__VA_ARGS__); break; \
        case 2048: F<2048>(__VA_ARGS__); break; \
        default: F<4096>(__VA_ARGS__); break;   \
    }

template <int N>
void launch_stft(const float* x, float* spec, int B, int T, int hop, int win, int L, hipStream_t s) {
    hipLaunchKernelGGL((stft_kernel<N>), dim3(T, B), dim3(GL_THREADS), 0, s, x, (float2*)spec, T, hop, win, L);
}

// The per-utterance part of a packed waveform batch (st_wave_batch), shared by the extractors: the batch bound, reflect padding at
// every utterance's own length, at least min_frames frames (0: no bound) and [off, off + len) inside the buffer.  Copies off / len
// into the kernel-argument arrays (the caller's zero-filled Meta) and gives the longest frame count.  fr has passed check_framing.
int wave_batch_fill(const char* who, const st_wave_batch* w, const st_framing* fr, int min_frames, long* off_out, int* len_out, int* tmax) {
    ST_CHECK_ARG(w->B > 0 && w->B <= FEAT_MAX_B, "%s: batch %d outside [1, %d]", who, w->B, FEAT_MAX_B);
    *tmax = 0;
    for (int b = 0; b < w->B; ++b) {
        const long off = w->off[b];
        const int len = w->len[b], frames = 1 + len / fr->hop;
        ST_CHECK_ARG(len > fr->n_fft / 2, "%s: utterance %d has %d samples: reflect padding needs more than n_fft / 2 = %d", who, b, len,
                     fr->n_fft / 2);
        ST_CHECK_ARG(frames >= min_frames, "%s: utterance %d has %d frames: the %d-frame derivatives need at least %d", who, b, frames,
                     min_frames, min_frames);
        ST_CHECK_ARG(off >= 0 && off + len <= w->n_samples, "%s: utterance %d [%ld, +%d) outside the %ld samples", who, b, off, len,
                     w->n_samples);
        off_out[b] = off;
        len_out[b] = len;
        *tmax = max(*tmax, frames);
    }
    return 0;
}

// Every instantiation of the STFT family's templated kernels, named once, in the order the code object has always held them: the
// compiler emits an instantiation where it is first named, so this list, not the shape of the launch wrappers, fixes the layout of
// the device code (it stays byte-identical when the host side is rearranged).  The wrappers pick among exactly these.
template <class... K> void name_kernels(K...) {}
void kernel_order() {
    name_kernels(
        stft_kernel<512>, stft_kernel<1024>, stft_kernel<2048>, stft_kernel<4096>,
        gl_first_istft_kernel<512, SRC_FEAT, false>, gl_first_istft_kernel<512, SRC_SPEC, false>,
        gl_first_istft_kernel<1024, SRC_FEAT, false>, gl_first_istft_kernel<1024, SRC_SPEC, false>,
        gl_first_istft_kernel<2048, SRC_FEAT, false>, gl_first_istft_kernel<2048, SRC_SPEC, false>,
        gl_first_istft_kernel<4096, SRC_FEAT, false>, gl_first_istft_kernel<4096, SRC_SPEC, false>,
        gl_ola_post_kernel<false>, gl_iter_kernel<512, false>, gl_iter_kernel<1024, false>, gl_iter_kernel<2048, false>, gl_iter_kernel<4096, false>,
        gl_first_istft_kernel<512, SRC_AMP, true>, gl_first_istft_kernel<512, SRC_FEAT, true>,
        gl_first_istft_kernel<1024, SRC_AMP, true>, gl_first_istft_kernel<1024, SRC_FEAT, true>,
        gl_first_istft_kernel<2048, SRC_AMP, true>, gl_first_istft_kernel<2048, SRC_FEAT, true>,
        gl_first_istft_kernel<4096, SRC_AMP, true>, gl_first_istft_kernel<4096, SRC_FEAT, true>,
        gl_iter_kernel<512, true>, gl_iter_kernel<1024, true>, gl_iter_kernel<2048, true>, gl_iter_kernel<4096, true>, gl_ola_post_kernel<true>,
        gl_first_istft_kernel<512, SRC_AMP, false>, gl_first_istft_kernel<1024, SRC_AMP, false>,
        gl_first_istft_kernel<2048, SRC_AMP, false>, gl_first_istft_kernel<4096, SRC_AMP, false>);
}

bool no_stft_dims(int B, int T, int n_fft, int hop, int win) { return B <= 0 || T <= 1 || hop <= 0 || win <= 0 || n_fft <= 0; }

}  // namespace

extern "C" size_t st_istft_workspace_floats(int B, int T, int n_fft, int hop, int win) {
    if (no_stft_dims(B, T, n_fft, hop, win)) return 0;
    return WND_FLOATS + round64((size_t)hop * (T - 1)) + round64((size_t)B * T * win);
}

extern "C" int st_stft_fwd(const float* x, float* spec, int B, int L, int n_fft, int hop, int win, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(x && spec && hop > 0 && L > 0, "st_stft_fwd: bad arguments");
    const int T = 1 + L / hop;
    int rc = check_dims("st_stft_fwd", B, n_fft, hop, win, T, L);
    if (rc) return rc;
    if ((rc = ensure_twiddles(stream)) != 0) return rc;
    ST_AUDIO_DISPATCH(n_fft, launch_stft, x, spec, B, T, hop, win, L, (hipStream_t)stream);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_istft(const float* spec, float* x, int B, int T, int n_fft, int hop, int win, float* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(spec && x && ws, "st_istft: null pointer");
    int rc = check_dims("st_istft", B, n_fft, hop, win, T, (long)hop * (T - 1));
    if (rc) return rc;
    if ((rc = ensure_twiddles(stream)) != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int L = hop * (T - 1);
    float* wnd = ws;
    float* inv_env = wnd + WND_FLOATS;
    float* frames = inv_env + round64(L);
    hipLaunchKernelGGL(gl_setup_kernel, dim3((max(L, win) + 255) / 256), dim3(256), 0, s, wnd, inv_env, n_fft, T, hop, win, L);
    ST_AUDIO_DISPATCH(n_fft, launch_first, SRC_SPEC, spec, 0, 0, 0, 0, 1.0f, nullptr, nullptr, wnd, frames, B, T, win, nullptr, 0, s);
    hipLaunchKernelGGL(gl_ola_post_kernel<false>, dim3(B), dim3(OLA_THREADS), 0, s, frames, inv_env, x, n_fft, T, hop, win, L, 0,
                       (const int*)nullptr, 0, (size_t)0);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_mel_to_linear(const float* mel, long sb, long st, long sm, const float* basis, float* lin, int B, int T, int n_mels, int F,
                                int normalized, int take_abs, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(mel && basis && lin, "st_mel_to_linear: null pointer");
    ST_CHECK_ARG(n_mels >= 1 && n_mels <= MEL_MAX, "st_mel_to_linear: %d mels outside [1, %d]", n_mels, MEL_MAX);
    ST_CHECK_ARG(F == 257 || F == 513 || F == 1025 || F == 2049, "st_mel_to_linear: %d bins is not n_fft / 2 + 1 of a supported n_fft", F);
    ST_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && (T + MEL_TILE - 1) / MEL_TILE <= 65535 && (long)T * B * 4096 < (1L << 40),
                 "st_mel_to_linear: bad batch %d / frames %d", B, T);
    launch_mel_to_linear(mel, sb, st, sm, basis, lin, B, T, n_mels, F, normalized != 0, take_abs != 0, nullptr, 0, (hipStream_t)stream);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t st_gl_batch_workspace_floats(int B, int T, int n_fft, int hop, int win) {
    if (no_stft_dims(B, T, n_fft, hop, win)) return 0;
    return WND_FLOATS + (size_t)B * round64((size_t)hop * (T - 1)) + round64((size_t)B * T * (n_fft / 2 + 1)) +
           2 * round64((size_t)B * T * win);
}

extern "C" int st_griffin_lim_batch(const st_gl_job* job, const st_framing* fr, float* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(job && fr && job->feat && job->phases && job->wav && ws, "st_griffin_lim_batch: null pointer");
    const st_gl_job& j = *job;
    const int B = j.B, T = j.T, n_fft = fr->n_fft, hop = fr->hop, win = fr->win, *frames = j.frames;
    ST_CHECK_ARG(j.n_iter >= 0 && (j.post & ~3) == 0 && j.power > 0.0f, "st_griffin_lim_batch: bad n_iter %d / post %d / power", j.n_iter,
                 j.post);
    int rc = check_dims("st_griffin_lim_batch", B, n_fft, hop, win, T, (long)hop * (T - 1));
    if (rc) return rc;
    const int L = hop * (T - 1);
    const int F = n_fft / 2 + 1;
    if (j.basis) {
        ST_CHECK_ARG(j.n_in >= 1 && j.n_in <= MEL_MAX, "st_griffin_lim_batch: %d mels outside [1, %d]", j.n_in, MEL_MAX);
        ST_CHECK_ARG(j.power == 1.0f, "st_griffin_lim_batch: mel input is an amplitude (isAmp): power must be 1");
        ST_CHECK_ARG((T + MEL_TILE - 1) / MEL_TILE <= 65535, "st_griffin_lim_batch: too many frames %d", T);
    } else {
        ST_CHECK_ARG(j.n_in == F, "st_griffin_lim_batch: %d bins, expected n_fft / 2 + 1 = %d", j.n_in, F);
    }
    if ((rc = ensure_twiddles(stream)) != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int tmin = n_fft / 2 / hop + 2;                     // the fewest frames check_dims takes (T itself passed it)
    const size_t env_stride = round64(L);
    float* wnd = ws;
    float* inv_env = wnd + WND_FLOATS;
    float* amp = inv_env + (size_t)B * env_stride;
    float* frm[2] = {amp + round64((size_t)B * T * F), nullptr};
    frm[1] = frm[0] + round64((size_t)B * T * win);
    if (frames)
        hipLaunchKernelGGL(gl_setup_ragged_kernel, dim3((max(L, win) + 255) / 256, B), dim3(256), 0, s, wnd, inv_env, env_stride, n_fft, T,
                           hop, win, frames, tmin);
    else
        hipLaunchKernelGGL(gl_setup_kernel, dim3((max(L, win) + 255) / 256), dim3(256), 0, s, wnd, inv_env, n_fft, T, hop, win, L);
    if (j.basis) launch_mel_to_linear(j.feat, j.sb, j.st, j.sf, j.basis, amp, B, T, j.n_in, F, j.normalized != 0, 1, frames, tmin, s);
    ST_AUDIO_DISPATCH(n_fft, launch_first, j.basis ? SRC_AMP : SRC_FEAT, j.feat, j.sb, j.st, j.sf, j.normalized, j.power, j.phases, amp, wnd,
                      frm[0], B, T, win, frames, tmin, s);
    for (int it = 0; it < j.n_iter; ++it)
        ST_AUDIO_DISPATCH(n_fft, launch_iter, frm[it & 1], frm[(it + 1) & 1], amp, wnd, inv_env, B, T, hop, win, L, frames, tmin, env_stride, s);
    if (frames)
        hipLaunchKernelGGL(gl_ola_post_kernel<true>, dim3(B), dim3(OLA_THREADS), 0, s, frm[j.n_iter & 1], inv_env, j.wav, n_fft, T, hop, win,
                           L, j.post, frames, tmin, env_stride);
    else
        hipLaunchKernelGGL(gl_ola_post_kernel<false>, dim3(B), dim3(OLA_THREADS), 0, s, frm[j.n_iter & 1], inv_env, j.wav, n_fft, T, hop, win,
                           L, j.post, (const int*)nullptr, 0, (size_t)0);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t st_features_workspace_floats(int B) { return B > 0 ? round64((size_t)B * POW_PARTS * 4) : 0; }

extern "C" int st_feature_noise(float* out, long n, int utt, unsigned long long seed, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(out && n > 0 && utt >= 0, "st_feature_noise: bad arguments");
    hipLaunchKernelGGL(feat_noise_kernel, dim3((unsigned)min((n + 255) / 256, 4096L)), dim3(256), 0, (hipStream_t)stream, out, n, utt, seed);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_audio_features(const st_wave_batch* w, const st_framing* fr, float preemph, const st_mel_bank* fb, const st_feat_aug* aug,
                                 float* mel, float* linear, int T_pad, float* ws, void* stream) {
    (void)hipGetLastError();
    const char* who = "st_audio_features";
    ST_CHECK_ARG(w && fr && fb && w->x && w->off && w->len && fb->start && fb->cnt && fb->off && fb->w && mel && ws, "%s: null pointer", who);
    static const st_feat_aug none = {};
    const st_feat_aug& a = aug ? *aug : none;
    ST_CHECK_ARG(!a.out || (a.win && a.hop), "%s: the augmented framing needs aug_win / aug_hop", who);
    ST_CHECK_ARG(a.utt0 >= 0 && a.utt0 <= INT_MAX - FEAT_MAX_B, "%s: first utterance index %d", who, a.utt0);
    int rc = check_framing(who, fr->n_fft, fr->hop, fr->win);
    if (rc) return rc;
    ST_CHECK_ARG(fb->n_mels > 0 && fb->n_mels <= fr->n_fft / 2 + 1, "%s: %d mels for n_fft %d", who, fb->n_mels, fr->n_fft);
    FeatMeta meta = {};                                       // (entries beyond B stay zero)
    int tmax = 0, tamax = 0;
    if ((rc = wave_batch_fill(who, w, fr, 0, meta.off, meta.len, &tmax)) != 0) return rc;
    for (int b = 0; b < w->B; ++b) {
        meta.awin[b] = fr->win;
        meta.ahop[b] = fr->hop;
        meta.snr[b] = a.snr_db ? a.snr_db[b] : NAN;
        if (a.out) {
            ST_CHECK_ARG(a.hop[b] > 0 && 2 * a.hop[b] <= a.win[b] && a.win[b] <= fr->n_fft,
                         "%s: utterance %d: augmented framing needs 0 < 2 * hop <= win <= n_fft (hop %d, win %d, n_fft %d)", who, b, a.hop[b],
                         a.win[b], fr->n_fft);
            meta.awin[b] = a.win[b];
            meta.ahop[b] = a.hop[b];
            tamax = max(tamax, 1 + meta.len[b] / a.hop[b]);
        }
    }
    ST_CHECK_ARG(T_pad >= tmax && (!a.out || a.Ta_pad >= tamax), "%s: T_pad %d / Ta_pad %d below the longest framing (%d / %d)", who, T_pad,
                 a.Ta_pad, tmax, tamax);
    if ((rc = ensure_twiddles(stream)) != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool noisy = a.out && a.snr_db;
    double* part = reinterpret_cast<double*>(ws);
    if (noisy) hipLaunchKernelGGL(feat_power_kernel, dim3(POW_PARTS, w->B), dim3(POW_THREADS), 0, s, w->x, a.noise, a.seed, a.utt0, meta, part);
    ST_AUDIO_DISPATCH(fr->n_fft, launch_features, w->x, a.noise, a.seed, a.utt0, noisy ? part : nullptr, meta, preemph, fr->win, fr->hop, fb->start,
                      fb->cnt, fb->off, fb->w, fb->n_mels, mel, linear, a.out, w->B, T_pad, a.Ta_pad, s);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_audio_mfcc(const st_wave_batch* w, const st_framing* fr, float preemph, const st_mel_bank* fb, const float* dct, int n_mfcc,
                             float* out, float* mel_out, int T_pad, void* stream) {
    (void)hipGetLastError();
    const char* who = "st_audio_mfcc";
    ST_CHECK_ARG(w && fr && fb && w->x && w->off && w->len && fb->start && fb->cnt && fb->off && fb->w && dct && out, "%s: null pointer", who);
    int rc = check_framing(who, fr->n_fft, fr->hop, fr->win);
    if (rc) return rc;
    ST_CHECK_ARG(1 <= n_mfcc && n_mfcc <= fb->n_mels && fb->n_mels <= MEL_MAX, "%s: need 1 <= n_mfcc <= n_mels <= %d (n_mfcc %d, n_mels %d)", who,
                 MEL_MAX, n_mfcc, fb->n_mels);
    MfccMeta meta = {};
    int tmax = 0;
    if ((rc = wave_batch_fill(who, w, fr, 2 * DELTA_HALF + 1, meta.off, meta.len, &tmax)) != 0) return rc;
    for (int b = 0; b < w->B; ++b)
        ST_CHECK_ARG(meta.len[b] < (1 << 30), "%s: utterance %d has %d samples: reflect padding needs more than n_fft / 2 = %d", who, b,
                     meta.len[b], fr->n_fft / 2);
    ST_CHECK_ARG(T_pad >= tmax && (long)T_pad * n_mfcc < (1L << 30), "%s: T_pad %d below the longest utterance (%d frames) or too large", who,
                 T_pad, tmax);
    if ((rc = ensure_twiddles(stream)) != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    ST_AUDIO_DISPATCH(fr->n_fft, launch_mfcc_frames, w->x, meta, preemph, fr->win, fr->hop, fb->start, fb->cnt, fb->off, fb->w, fb->n_mels, dct,
                      n_mfcc, out, mel_out, w->B, T_pad, s);
    hipLaunchKernelGGL(mfcc_delta_kernel, dim3((T_pad * n_mfcc + 255) / 256, w->B), dim3(256), 0, s, out, meta, fr->hop, n_mfcc, T_pad);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_segment_gather(const float* feat, long sb, long st, int B, int T_pad, int D, const int* seg_utt, const int* seg_start,
                                 const int* seg_len, int S, int max_len, float* out, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(S >= 0 && max_len >= 0, "st_segment_gather: %d segments of %d rows", S, max_len);
    if (S == 0 || max_len == 0) return 0;
    ST_CHECK_ARG(feat && seg_utt && seg_start && seg_len && out, "st_segment_gather: null pointer");
    ST_CHECK_ARG(B > 0 && T_pad > 0 && D > 0 && st >= D && sb >= 0, "st_segment_gather: bad feat (%d, %d, %d), strides %ld / %ld", B, T_pad, D, sb,
                 st);
    ST_CHECK_ARG(((size_t)out & 15) == 0, "st_segment_gather: out must be 16-byte aligned");
    const long total = (long)S * max_len * D;
    ST_CHECK_ARG((long)S * max_len < (1L << 31) && total < (1L << 38), "st_segment_gather: output (%d, %d, %d) too large", S, max_len, D);
    const long quads = (total + 3) / 4;
    hipLaunchKernelGGL(segment_gather_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feat, sb, st, B, T_pad, D,
                       seg_utt, seg_start, seg_len, total, max_len, out);
    ST_LAUNCH_CHECK();
    return 0;
}
