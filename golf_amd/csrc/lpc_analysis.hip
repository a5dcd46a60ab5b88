// Frame-wise LPC analysis for gfx950: audio -> (gain, a, rc) by the autocorrelation method, and its adjoint.
//
// Definition (include/golf_amd.h; the float64 restatement in tests/lpc_analysis_ref.py is the checker).  Frame f of row b
// starts at sample o_f = origin + f*hop (origin = -floor(W/2) for centred frames, 0 otherwise; x = 0 outside [0, T)):
//   s[k] = x[o_f + k] * window[k]                         k = 0..W-1      (one fp32 product)
//   r[j] = sum_{n=0}^{W-1-j} s[n] s[n+j]                  j = 0..M
//   r[0] <- r[0] (1 + eps_rel) + eps_abs
//   Levinson-Durbin, E_0 = r[0], for i = 1..M:
//       k_i = -(r[i] + sum_{j<i} a_j r[i-j]) / E_{i-1};   a_j <- a_j + k_i a_{i-j} (j < i);   a_i = k_i;   E_i = E_{i-1} (1 - k_i^2)
//   a = a^{(M)},  rc[i-1] = k_i,  gain = sqrt(max(E_M, 0) / sum_k window[k]^2)
// Speech frames reach |k_i| = 0.998: lags summed in fp32 or a recursion run in fp32 miss a 1e-4 parity bar by one to three
// orders of magnitude, so everything after the staged frame is fp64.  A product of two fp32 values is exact in fp64.
//
// Forward: one wave per frame.  The windowed frame sits in the wave's LDS slice, zero padded by M + LAGS taps so that no lag
// needs a bounds check; every lane accumulates its share of LAGS lags at a time in fp64, a butterfly sums them across the
// wave (all lanes end with the same bits).  The recursion keeps coefficient a_{l+1} in lane l: the flip a_{i-j} is a lane
// permutation, the inner product a wave sum, M sequential steps.  The regularised lags go to the caller's workspace as
// fp64: the backward starts from exactly what the forward used.
// Backward, two launches, no atomics:
//   1. one wave per frame: the recursion again from the saved lags with every stage a^{(i)} kept in LDS (triangular,
//      M (M+1) / 2 doubles), then reverse mode through it to g_r (B, F, M+1) in fp64;
//   2. one thread per sample t: over the frames that cover t in ascending order, with k = t - o_f,
//      g_x[t] += window[k] * sum_{j=0}^{M} g_r[f][j] c_j (s_f[k+j] + s_f[k-j]),   c_0 = 1 + eps_rel, c_j = 1 otherwise,
//      the frame's stretch of s_f staged in LDS for the 256 samples of the workgroup.
//
// Source-compensated analysis (golf_lpc_source_filter_f32, forward only; tests/sflpc_ref.py is the checker): iterative adaptive
// inverse filtering restated on lags.  Filtering the windowed frame by a short polynomial c and taking its autocorrelation
// is (r o c)[j] = rho_c[0] r[j] + sum_d rho_c[d] (r[|j-d|] + r[j+d]) with rho_c the autocorrelation of c, so the frame is
// staged and summed once, exactly as above but for M + Q lags, and every later stage (source polynomial, tract, source, ...,
// final tract, gain) is the same wave's recursion on a filtered lag set kept beside r in its LDS slice: rho_c over lanes d,
// (r o c)[j] over lanes j, both as doubles.  No workspace; a frame's bits depend on its samples and the arguments only.
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int LA_MAX_ORDER = 64;
constexpr int LA_MAX_WINDOW = 4096;
constexpr int LA_LAGS = 8;      // lags per pass over the frame
constexpr int LA_TILE = 256;    // samples per workgroup of the gather

__device__ __forceinline__ double la_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// floats of one wave's frame slice: W taps + zero padding for the largest lag of the last pass, kept a multiple of 2 so
// that the doubles of the next slice stay aligned
__host__ __device__ constexpr int la_frame_floats(int W, int M) { return (W + M + LA_LAGS + 1) & ~1; }
static inline int la_fwd_waves(int W) { return W <= 2048 ? 4 : 2; }
static inline size_t la_fwd_lds(int waves, int W, int M) {
    return (size_t)waves * ((M + 1) * sizeof(double) + la_frame_floats(W, M) * sizeof(float));
}
__host__ __device__ constexpr int la_tri(int i) { return i * (i - 1) / 2; }   // first entry of stage i (i entries)
__host__ __device__ constexpr int la_bwd_doubles(int M) { return 2 * (M + 1) + la_tri(M + 1); }
constexpr int LA_BWD_WAVES = 2;

// one Levinson-Durbin step in the lane layout (lane l holds a_{l+1}); returns k_i
__device__ __forceinline__ double la_step(double& a, double& err, const double* r, int i, int lane) {
    const int j = lane + 1;
    const double acc = la_wave_sum(j < i ? a * r[i - j] : 0.0);
    const double k = -(r[i] + acc) / err;
    const double af = __shfl(a, (i - lane - 2) & 63);   // a_{i-j}
    if (j < i) a = a + k * af;
    else if (j == i) a = k;
    err *= 1.0 - k * k;
    return k;
}

__device__ __forceinline__ double la_window_energy(const float* __restrict__ window, int W, int lane) {
    double sw = 0.0;
    for (int k = lane; k < W; k += 64) {
        const double w = (double)window[k];
        sw += w * w;
    }
    return la_wave_sum(sw);
}

// the wave's frame slice: s[k] = x[o + k] * window[k] for k < W (x = 0 outside [0, T)), zeros up to S
__device__ __forceinline__ void la_stage_frame(float* s, int S, const float* __restrict__ xr, const float* __restrict__ window,
                                               int64_t o, int T, int W, int lane) {
    for (int k = lane; k < S; k += 64) {
        const int64_t t = o + k;
        s[k] = (k < W && t >= 0 && t < T) ? xr[t] * window[k] : 0.f;
    }
}

// lags j0 .. j0 + LA_LAGS - 1 of the staged frame, the same bits in every lane
__device__ __forceinline__ void la_lag_pass(double (&v)[LA_LAGS], const float* s, int W, int j0, int lane) {
#pragma unroll
    for (int jj = 0; jj < LA_LAGS; ++jj) v[jj] = 0.0;
    for (int n = lane; n < W; n += 64) {
        const double sn = (double)s[n];
#pragma unroll
        for (int jj = 0; jj < LA_LAGS; ++jj) v[jj] += sn * (double)s[n + j0 + jj];   // zeros past W
    }
#pragma unroll
    for (int jj = 0; jj < LA_LAGS; ++jj) v[jj] = la_wave_sum(v[jj]);
}

// Levinson-Durbin to order n from the lags r: lane l ends with a_{l+1} and k_{l+1} (0 from lane n on); returns E_n
__device__ __forceinline__ double la_levinson(double& a, double& kk, const double* r, int n, int lane) {
    a = 0.0, kk = 0.0;
    double err = r[0];
    for (int i = 1; i <= n; ++i) {
        const double k = la_step(a, err, r, i, lane);
        if (lane + 1 == i) kk = k;
    }
    return err;
}

__global__ void lpc_analysis_fwd_kernel(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ window,
                                        float* __restrict__ gain, float* __restrict__ a_out, float* __restrict__ rc_out,
                                        double* __restrict__ lags, int G, int T, int F, int M, int hop, int W,
                                        int64_t origin, double eps_rel, double eps_abs) {
    extern __shared__ __attribute__((aligned(16))) double la_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int g = blockIdx.x * waves + w;
    if (g >= G) return;   // wave-uniform; nothing below synchronises across waves
    const int S = la_frame_floats(W, M);
    double* r = la_lds + w * (M + 1);
    float* s = (float*)(la_lds + waves * (M + 1)) + (size_t)w * S;
    const int b = g / F, f = g - b * F;

    la_stage_frame(s, S, x + (int64_t)b * x_stride, window, origin + (int64_t)f * hop, T, W, lane);
    const double sw = la_window_energy(window, W, lane);
    wave_lds_fence();

    for (int j0 = 0; j0 <= M; j0 += LA_LAGS) {
        double acc[LA_LAGS];
        la_lag_pass(acc, s, W, j0, lane);
#pragma unroll
        for (int jj = 0; jj < LA_LAGS; ++jj) {
            double v = acc[jj];
            const int j = j0 + jj;
            if (j == 0) v = v * (1.0 + eps_rel) + eps_abs;
            if (lane == 0 && j <= M) {
                r[j] = v;
                lags[(size_t)g * (M + 1) + j] = v;
            }
        }
    }
    wave_lds_fence();

    double a, kk;
    const double err = la_levinson(a, kk, r, M, lane);
    if (lane < M) {
        a_out[(size_t)g * M + lane] = (float)a;
        if (rc_out) rc_out[(size_t)g * M + lane] = (float)kk;
    }
    if (lane == 0) gain[g] = (float)sqrt(fmax(err, 0.0) / sw);
}

// ---- source-compensated analysis (golf_lpc_source_filter_f32): the stages after the lags work on lag sets alone ---------------
constexpr int SF_MAX_SOURCE = 16;
constexpr int SF_MAX_ITER = 8;

__host__ __device__ constexpr int sf_poly(int M, int Q) { return (M > Q ? M : Q) + 1; }   // coefficients of the longer one
// doubles of one wave's slice: r[0..M+Q], then the filtered lags t, the polynomial c and its lags rho, sf_poly each
__host__ __device__ constexpr int sf_doubles(int M, int Q) { return M + Q + 1 + 3 * sf_poly(M, Q); }
static inline size_t sf_lds(int waves, int W, int M, int Q) {
    return (size_t)waves * (sf_doubles(M, Q) * sizeof(double) + la_frame_floats(W, M + Q) * sizeof(float));
}

// c <- 1, a_1 .. a_n from the lane layout
__device__ __forceinline__ void sf_store_poly(double* c, double a, int n, int lane) {
    if (lane == 0) c[0] = 1.0;
    if (lane < n) c[lane + 1] = a;
    wave_lds_fence();
}

// t[0..n] <- the lags of the frame filtered by c (order P, c_0 = 1): rho[d] = sum_p c_p c_{p+d} over lanes d, then
// t[j] = rho[0] r[j] + sum_{d=1}^{P} rho[d] (r[|j-d|] + r[j+d]) over lanes j; r holds lags 0 .. n + P.  An index past lane 63
// (order 64 has 65 coefficients) takes a second round.
__device__ __forceinline__ void sf_filtered_lags(double* t, double* rho, const double* r, const double* c, int P, int n,
                                                 int lane) {
    for (int d = lane; d <= P; d += 64) {
        double acc = 0.0;
        for (int p = 0; p + d <= P; ++p) acc += c[p] * c[p + d];
        rho[d] = acc;
    }
    wave_lds_fence();
    for (int j = lane; j <= n; j += 64) {
        double acc = rho[0] * r[j];
        for (int d = 1; d <= P; ++d) acc += rho[d] * (r[j >= d ? j - d : d - j] + r[j + d]);
        t[j] = acc;
    }
    wave_lds_fence();
}

__global__ void lpc_source_filter_kernel(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ window,
                                         float* __restrict__ gain, float* __restrict__ a_out, float* __restrict__ rc_out,
                                         float* __restrict__ src_out, int G, int T, int F, int M, int Q, int iterations,
                                         int adaptive, double preemphasis, int hop, int W, int64_t origin, double eps_rel,
                                         double eps_abs) {
    extern __shared__ __attribute__((aligned(16))) double la_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int g = blockIdx.x * waves + w;
    if (g >= G) return;   // wave-uniform; nothing below synchronises across waves
    const int J = M + Q, S = la_frame_floats(W, J), NP = sf_poly(M, Q);
    double* r = la_lds + w * sf_doubles(M, Q);
    double* t = r + J + 1;
    double* c = t + NP;
    double* rho = c + NP;
    float* s = (float*)(la_lds + waves * sf_doubles(M, Q)) + (size_t)w * S;
    const int b = g / F, f = g - b * F;

    la_stage_frame(s, S, x + (int64_t)b * x_stride, window, origin + (int64_t)f * hop, T, W, lane);
    const double sw = la_window_energy(window, W, lane);
    wave_lds_fence();

    for (int j0 = 0; j0 <= J; j0 += LA_LAGS) {
        double acc[LA_LAGS];
        la_lag_pass(acc, s, W, j0, lane);
#pragma unroll
        for (int jj = 0; jj < LA_LAGS; ++jj) {
            const int j = j0 + jj;
            if (lane == 0 && j <= J) r[j] = j == 0 ? acc[jj] * (1.0 + eps_rel) + eps_abs : acc[jj];
        }
    }
    wave_lds_fence();

    double a, kk;
    int P = 1;   // the order of the source polynomial in c
    if (adaptive) la_levinson(a, kk, r, 1, lane);
    else a = lane == 0 ? -preemphasis : 0.0;
    sf_store_poly(c, a, P, lane);
    for (int it = 0; it < iterations; ++it) {
        sf_filtered_lags(t, rho, r, c, P, M, lane);
        la_levinson(a, kk, t, M, lane);
        sf_store_poly(c, a, M, lane);             // the tract
        sf_filtered_lags(t, rho, r, c, M, Q, lane);
        la_levinson(a, kk, t, Q, lane);
        sf_store_poly(c, a, P = Q, lane);         // the source
    }
    if (src_out && lane < Q) src_out[(size_t)g * Q + lane] = (float)a;   // zero from lane P on
    sf_filtered_lags(t, rho, r, c, P, M, lane);
    la_levinson(a, kk, t, M, lane);
    if (lane < M) {
        a_out[(size_t)g * M + lane] = (float)a;
        if (rc_out) rc_out[(size_t)g * M + lane] = (float)kk;
    }
    sf_store_poly(c, a, M, lane);
    sf_filtered_lags(t, rho, r, c, M, 0, lane);   // the audio through the tract's inverse alone
    if (lane == 0) gain[g] = (float)sqrt(fmax(t[0], 0.0) / sw);
}

// g_r (G, M+1) from the saved lags and the incoming gradients (each may be null)
__global__ void lpc_analysis_bwd_frames_kernel(const float* __restrict__ g_gain, const float* __restrict__ g_a,
                                               const float* __restrict__ g_rc, const float* __restrict__ window,
                                               const double* __restrict__ lags, double* __restrict__ g_r, int G, int M,
                                               int W) {
    extern __shared__ __attribute__((aligned(16))) double la_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = blockIdx.x * LA_BWD_WAVES + w;
    if (g >= G) return;   // wave-uniform
    double* r = la_lds + (size_t)w * la_bwd_doubles(M);
    double* E = r + (M + 1);
    double* A = E + (M + 1);   // stage i (a^{(i)}_1 .. a^{(i)}_i) at A[la_tri(i)]
    const int j = lane + 1;

    if (lane <= M) r[lane] = lags[(size_t)g * (M + 1) + lane];
    if (lane == 0) r[M] = lags[(size_t)g * (M + 1) + M];   // M = 64: the 65th lag
    const double sw = la_window_energy(window, W, lane);
    wave_lds_fence();
    double a = 0.0, err = r[0];
    if (lane == 0) E[0] = err;
    for (int i = 1; i <= M; ++i) {
        la_step(a, err, r, i, lane);
        if (j <= i) A[la_tri(i) + lane] = a;
        if (lane == 0) E[i] = err;
    }
    wave_lds_fence();

    double abar = (g_a && lane < M) ? (double)g_a[(size_t)g * M + lane] : 0.0;   // adjoint of a^{(i)}_{l+1}
    double rbar = 0.0;                                                            // adjoint of r[l+1]
    const double EM = E[M];
    double Ebar = (g_gain && EM > 0.0) ? (double)g_gain[g] * 0.5 / sqrt(EM * sw) : 0.0;
    for (int i = M; i >= 1; --i) {
        const double k = A[la_tri(i) + i - 1], Ep = E[i - 1];
        const double ap = j < i ? A[la_tri(i - 1) + (i - j) - 1] : 0.0;   // a^{(i-1)}_{i-j}
        const double abar_i = __shfl(abar, i - 1);
        double kbar = (g_rc ? (double)g_rc[(size_t)g * M + i - 1] : 0.0) + abar_i + la_wave_sum(j < i ? abar * ap : 0.0);
        kbar -= 2.0 * k * Ebar * Ep;                                       // E_i = E_{i-1} (1 - k^2)
        const double qbar = -kbar / Ep;                                    // k = -q / E_{i-1}
        Ebar = Ebar * (1.0 - k * k) - kbar * k / Ep;
        const double abar_f = __shfl(abar, (i - lane - 2) & 63);           // adjoint of a^{(i)}_{i-j}
        abar = j < i ? abar + k * abar_f + qbar * r[i - j] : 0.0;
        if (j < i) rbar += qbar * ap;                                      // q = r[i] + sum_j a^{(i-1)}_j r[i-j]
        else if (j == i) rbar += qbar;
    }
    if (lane == 0) g_r[(size_t)g * (M + 1)] = Ebar;                        // E_0 = r[0]
    if (lane < M) g_r[(size_t)g * (M + 1) + j] = rbar;
}

__device__ __forceinline__ int64_t la_floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// g_x (B, T) from g_r: every sample sums over the frames that cover it, ascending in f
__global__ __launch_bounds__(LA_TILE) void lpc_analysis_bwd_gather_kernel(
    const double* __restrict__ g_r, const float* __restrict__ x, int64_t x_stride, const float* __restrict__ window,
    float* __restrict__ g_x, int64_t g_x_stride, int tiles, int T, int F, int M, int hop, int W, int64_t origin, double c0) {
    __shared__ float sl[LA_TILE + 2 * LA_MAX_ORDER];   // s_f[k] for k = t0 - o_f - M .. t0 - o_f + LA_TILE - 1 + M
    __shared__ double gl[LA_MAX_ORDER + 1];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int64_t t0 = (int64_t)tile * LA_TILE, t = t0 + tid;
    const float* xr = x + (int64_t)b * x_stride;
    // frames with o_f <= t0 + LA_TILE - 1 and o_f + W - 1 >= t0
    int64_t f_lo = la_floor_div(t0 - W + 1 - origin + hop - 1, hop), f_hi = la_floor_div(t0 + LA_TILE - 1 - origin, hop);
    if (f_lo < 0) f_lo = 0;
    if (f_hi > F - 1) f_hi = F - 1;
    double acc = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const int64_t o = origin + f * hop;
        __syncthreads();   // the previous frame's reads
        for (int idx = tid; idx < LA_TILE + 2 * M; idx += LA_TILE) {
            const int64_t tt = t0 - M + idx, k = tt - o;
            sl[idx] = (k >= 0 && k < W && tt >= 0 && tt < T) ? xr[tt] * window[k] : 0.f;
        }
        if (tid <= M) gl[tid] = g_r[((size_t)b * F + (size_t)f) * (M + 1) + tid] * (tid == 0 ? c0 : 1.0);
        __syncthreads();
        const int64_t k = t - o;
        if (t < T && k >= 0 && k < W) {
            const int p = tid + M;
            double sum = 0.0;
            for (int j = 0; j <= M; ++j) sum += gl[j] * ((double)sl[p + j] + (double)sl[p - j]);
            acc += (double)window[k] * sum;
        }
    }
    if (t < T) g_x[(int64_t)b * g_x_stride + t] = (float)acc;
}

static int la_check_shape(const char* who, int B, int T, int F, int M, int hop, int W) {
    if (B < 1 || T < 0 || F < 1) return fail(GOLF_EINVAL, "%s: bad size (B=%d T=%d F=%d)", who, B, T, F);
    if (M < 1 || M > LA_MAX_ORDER)
        return fail(GOLF_EUNSUPPORTED, "%s: order M=%d outside 1..%d", who, M, LA_MAX_ORDER);
    if (W <= M) return fail(GOLF_EUNSUPPORTED, "%s: window W=%d must exceed the order M=%d", who, W, M);
    if (W > LA_MAX_WINDOW)
        return fail(GOLF_EUNSUPPORTED, "%s: window W=%d exceeds %d (a frame must fit LDS)", who, W, LA_MAX_WINDOW);
    if (hop < 1) return fail(GOLF_EUNSUPPORTED, "%s: hop=%d must be >= 1", who, hop);
    if ((int64_t)B * F >= ((int64_t)1 << 31))
        return fail(GOLF_EUNSUPPORTED, "%s: B*F = %lld frames, must be < 2^31", who, (long long)B * F);
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" {

size_t golf_lpc_analysis_workspace_bytes(int B, int F, int M) {
    if (B < 1 || F < 1 || M < 1 || M > LA_MAX_ORDER) return 0;
    return align_up((size_t)B * F * (M + 1) * sizeof(double), 256);
}

int golf_lpc_analysis_fwd_f32(const float* x, int64_t x_stride, const float* window, float* gain, float* a, float* rc,
                              void* ws, size_t ws_bytes, int B, int T, int F, int M, int hop, int W, int64_t origin,
                              double eps_rel, double eps_abs, void* stream) {
    if ((!x && T > 0) || !window || !gain || !a || !ws)
        return fail(GOLF_EINVAL, "lpc_analysis_fwd: null pointer (x=%p window=%p gain=%p a=%p ws=%p)", x, window, gain, a, ws);
    if (int e = la_check_shape("lpc_analysis_fwd", B, T, F, M, hop, W)) return e;
    if (x_stride < T) return fail(GOLF_EINVAL, "lpc_analysis_fwd: row stride %lld < T=%d", (long long)x_stride, T);
    if (ws_bytes < golf_lpc_analysis_workspace_bytes(B, F, M) || ((uintptr_t)ws & 255))
        return fail(GOLF_EWORKSPACE, "lpc_analysis_fwd: need %zu bytes aligned to 256, got %zu at %p",
                    golf_lpc_analysis_workspace_bytes(B, F, M), ws_bytes, ws);
    const int G = B * F, waves = la_fwd_waves(W);
    hipLaunchKernelGGL(lpc_analysis_fwd_kernel, dim3((unsigned)ceil_div(G, waves)), dim3(64 * waves),
                       la_fwd_lds(waves, W, M), (hipStream_t)stream, x, x_stride, window, gain, a, rc, (double*)ws, G, T, F,
                       M, hop, W, origin, eps_rel, eps_abs);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_lpc_source_filter_f32(const float* x, int64_t x_stride, const float* window, float* gain, float* a, float* rc,
                               float* source, int B, int T, int F, int M, int Q, int iterations, int adaptive,
                               double preemphasis, int hop, int W, int64_t origin, double eps_rel, double eps_abs,
                               void* stream) {
    const char* who = "lpc_source_filter";
    if (int e = la_check_shape(who, B ? B : 1, T, F, M, hop, W)) return e;   // an empty batch is checked like a row
    if (Q < 1 || Q > SF_MAX_SOURCE)
        return fail(GOLF_EUNSUPPORTED, "%s: source order Q=%d outside 1..%d", who, Q, SF_MAX_SOURCE);
    if (iterations < 0 || iterations > SF_MAX_ITER)
        return fail(GOLF_EUNSUPPORTED, "%s: iterations=%d outside 0..%d", who, iterations, SF_MAX_ITER);
    if (W <= M + Q) return fail(GOLF_EUNSUPPORTED, "%s: window W=%d must exceed M + Q = %d", who, W, M + Q);
    if (!adaptive && !(fabs(preemphasis) < 1.0))   // NaN fails the comparison too
        return fail(GOLF_EINVAL, "%s: preemphasis=%g must be finite with |preemphasis| < 1", who, preemphasis);
    if (B == 0) return GOLF_OK;
    if ((!x && T > 0) || !window || !gain || !a)
        return fail(GOLF_EINVAL, "%s: null pointer (x=%p window=%p gain=%p a=%p)", who, x, window, gain, a);
    if (x_stride < T) return fail(GOLF_EINVAL, "%s: row stride %lld < T=%d", who, (long long)x_stride, T);
    const int G = B * F, waves = la_fwd_waves(W);
    hipLaunchKernelGGL(lpc_source_filter_kernel, dim3((unsigned)ceil_div(G, waves)), dim3(64 * waves),
                       sf_lds(waves, W, M, Q), (hipStream_t)stream, x, x_stride, window, gain, a, rc, source, G, T, F, M, Q,
                       iterations, adaptive, preemphasis, hop, W, origin, eps_rel, eps_abs);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_lpc_analysis_bwd_f32(const float* g_gain, const float* g_a, const float* g_rc, const float* x, int64_t x_stride,
                              const float* window, const void* lags, float* g_x, int64_t g_x_stride, void* ws,
                              size_t ws_bytes, int B, int T, int F, int M, int hop, int W, int64_t origin, double eps_rel,
                              void* stream) {
    if ((!x && T > 0) || !window || !lags || (!g_x && T > 0) || !ws)
        return fail(GOLF_EINVAL, "lpc_analysis_bwd: null pointer (x=%p window=%p lags=%p g_x=%p ws=%p)", x, window, lags,
                    g_x, ws);
    if (int e = la_check_shape("lpc_analysis_bwd", B, T, F, M, hop, W)) return e;
    if (x_stride < T || g_x_stride < T)
        return fail(GOLF_EINVAL, "lpc_analysis_bwd: row stride (%lld, %lld) < T=%d", (long long)x_stride,
                    (long long)g_x_stride, T);
    if (ws_bytes < golf_lpc_analysis_workspace_bytes(B, F, M) || ((uintptr_t)ws & 255))
        return fail(GOLF_EWORKSPACE, "lpc_analysis_bwd: need %zu bytes aligned to 256, got %zu at %p",
                    golf_lpc_analysis_workspace_bytes(B, F, M), ws_bytes, ws);
    const int64_t tiles = ceil_div(T, LA_TILE);
    if ((int64_t)B * tiles >= ((int64_t)1 << 31))
        return fail(GOLF_EUNSUPPORTED, "lpc_analysis_bwd: B*ceil(T/%d) = %lld workgroups, must be < 2^31", LA_TILE,
                    (long long)B * tiles);
    if (T == 0) return GOLF_OK;
    const int G = B * F;
    hipLaunchKernelGGL(lpc_analysis_bwd_frames_kernel, dim3((unsigned)ceil_div(G, LA_BWD_WAVES)), dim3(64 * LA_BWD_WAVES),
                       (size_t)LA_BWD_WAVES * la_bwd_doubles(M) * sizeof(double), (hipStream_t)stream, g_gain, g_a, g_rc,
                       window, (const double*)lags, (double*)ws, G, M, W);
    GOLF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpc_analysis_bwd_gather_kernel, dim3((unsigned)(B * tiles)), dim3(LA_TILE), 0, (hipStream_t)stream,
                       (const double*)ws, x, x_stride, window, g_x, g_x_stride, (int)tiles, T, F, M, hop, W, origin,
                       1.0 + eps_rel);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
