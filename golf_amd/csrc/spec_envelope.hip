// Spectral-envelope analysis for gfx950: (audio, f0) -> the log magnitude envelope and its cepstrum, per frame: a
// pitch-adaptive estimator of the CheapTrick kind.  Definition in include/golf_amd.h; the float64 restatement in
// tests/env_ref.py is the checker.
//
// One launch, one workgroup of four waves per (b, f) frame; no workspace, no atomics, nothing shared between workgroups.  A
// frame lives in LDS from its samples to its outputs:
//   0. Every thread forms the frame's constants in fp64 from the fp32 inputs: fe, the half window hw, r0 = fe n / sr bins and
//      the smoothing half width r = r0 / 3.
//   1. Staging: thread i (strided by 256) loads x[f hop + m], m = i - hw, zero outside [0, T), and keeps (w, w x); the
//      window's argument m fe / (3 sr) is a fraction of a cycle formed in fp64.  sum w, sum w^2 and sum w x are reduced over a
//      fixed tree.  w x - w (sum w x / sum w) goes to index m mod n of a zeroed complex buffer.
//   2. Transform (three times): a radix-2 Stockham FFT of n complex points between two LDS buffers, twiddles exp(-2 pi j k / n)
//      from a table filled once (k / n is exact in fp32).  The second and third inputs are real and even, so the forward
//      transform's real part is what the definition's inverse real DFT and DFT ask for.
//   3. P = |X|^2 / sum w^2; the DC correction reads P and writes a second row, so that no bin reads a corrected neighbour.
//   4. Smoothing: a bin sums its cells directly -- the two edge cells by their covered fraction (fp64 edges), the cells
//      between them whole -- never a difference of running sums.
//   5. log, transform, lifter (sinc and cosine arguments reduced in fp64), ceps out, transform, log_env out.
// Every sum runs in a fixed order: bit-reproducible, and a row does not depend on its batch.  The kernel is a function of
// utterance positions (t = f hop + m in int64), so the block-by-block twin (golf_spectral_envelope_stream_f32) is this kernel
// with the positions of its buffers: samples [x_t0, x_end), f0 frames from f0_first, output column j = frame f_first + j.
#include "common.h"

namespace golf {

constexpr int ENV_THREADS = 256;
constexpr int ENV_MIN_N = 64;
constexpr int ENV_MAX_N = 2048;
constexpr int ENV_GRID_X = 1 << 20;          // frames per grid row

struct EnvArgs {
    const float* x;
    int64_t x_stride;
    const float* f0;
    int64_t f0_stride;
    float* log_env;
    float* ceps;
    int64_t x_t0, x_end;    // the buffer holds samples [x_t0, x_end); a sample outside it reads 0 (the entries say which may)
    int64_t f0_first;       // column 0 of the f0 buffer is frame f0_first
    int64_t f_first;        // column 0 of the outputs is frame f_first
    int G, F, n, log2n, n_ceps, hop;   // F: frames of this launch
    double sample_rate, f0_floor, f0_ceil, unvoiced_f0, q1, voiced_offset;
    float eps;
};

// The n-point forward DFT of a, radix-2 Stockham between a and b; the caller has synchronised a.  Returns where it ended.
__device__ __forceinline__ float2* env_fft(float2* a, float2* b, const float2* tw, int n, int log2n, int tid) {
    const int half = n >> 1;
    for (int s = 0; s < log2n; ++s) {
        const int ns = 1 << s, tstep = half >> s;   // the stage's twiddle exp(-2 pi j k / (2 ns)) = tw[k n / (2 ns)]
        for (int j = tid; j < half; j += ENV_THREADS) {
            const int k = j & (ns - 1);
            const float2 u0 = a[j], v = a[j + half], w = tw[k * tstep];
            const float2 u1 = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            const int j0 = ((j - k) << 1) + k;
            b[j0] = make_float2(u0.x + u1.x, u0.y + u1.y);
            b[j0 + ns] = make_float2(u0.x - u1.x, u0.y - u1.y);
        }
        __syncthreads();
        float2* t = a;
        a = b, b = t;
    }
    return a;
}

// h[0 .. nh] -> its even extension of length n in dst, imaginary parts 0
__device__ __forceinline__ void env_put_even(float2* dst, int k, int nh, float v) {
    dst[k] = make_float2(v, 0.f);
    if (k > 0 && k < nh) dst[2 * nh - k] = make_float2(v, 0.f);
}

__global__ __launch_bounds__(ENV_THREADS) void spec_envelope_kernel(const EnvArgs p) {
    __shared__ float2 buf0[ENV_MAX_N], buf1[ENV_MAX_N];
    __shared__ float2 tw[ENV_MAX_N / 2];
    __shared__ float P[ENV_MAX_N / 2 + 1], Pc[ENV_MAX_N / 2 + 1];
    __shared__ float red[3][ENV_THREADS];
    const int tid = threadIdx.x;
    const int64_t g64 = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (g64 >= p.G) return;
    const int g = (int)g64, b = g / p.F;
    const int64_t f = p.f_first + (g - b * p.F);
    const int n = p.n, nh = n >> 1, log2n = p.log2n;
    const float* xr = p.x + (int64_t)b * p.x_stride;

    // ---- 0. frame constants -------------------------------------------------------------------------------------------------
    const float f0v = p.f0[(int64_t)b * p.f0_stride + (f - p.f0_first)];
    const bool voiced = f0v > 0.f;   // false for a NaN
    const double sr = p.sample_rate;
    const double fe = voiced ? fmin(fmax((double)f0v, p.f0_floor), p.f0_ceil) : p.unvoiced_f0;
    const int hw = (int)floor(1.5 * sr / fe + 0.5);   // <= n/2 - 1: the entry checked it at f0_floor
    const double r0 = fe * (double)n / sr, r = r0 / 3.0;
    const float off = voiced ? (float)p.voiced_offset : 0.f;

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    for (int j = tid; j < n; j += ENV_THREADS) buf0[j] = make_float2(0.f, 0.f);
    for (int j = tid; j < nh; j += ENV_THREADS) {
        float s, c;
        sincospif((float)(2 * j) / (float)n, &s, &c);   // 2 j / n is exact
        tw[j] = make_float2(c, -s);
    }
    const int L = 2 * hw + 1;
    const int64_t t0 = f * p.hop - hw;
    float sw = 0.f, sw2 = 0.f, sxw = 0.f;
    for (int i = tid; i < L; i += ENV_THREADS) {
        const int64_t t = t0 + i;
        const float xv = (t >= p.x_t0 && t < p.x_end) ? xr[t - p.x_t0] : 0.f;
        const double arg = (double)(i - hw) * fe / (3.0 * sr);   // cycles, within about [-1/2, 1/2]
        const float ch = cospif((float)arg);
        const float w = ch * ch;   // 0.5 + 0.5 cos(2 pi arg) = cos^2(pi arg): no cancellation where the window is small
        const float wx = w * xv;
        buf1[i] = make_float2(w, wx);
        sw += w, sw2 = fmaf(w, w, sw2), sxw += wx;
    }
    red[0][tid] = sw, red[1][tid] = sw2, red[2][tid] = sxw;
    __syncthreads();
    for (int s = ENV_THREADS >> 1; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
        }
        __syncthreads();
    }
    const float sum_w = red[0][0], sum_w2 = red[1][0], mean = red[2][0] / sum_w;
    for (int i = tid; i < L; i += ENV_THREADS) {
        const float2 v = buf1[i];
        buf0[(i - hw + n) & (n - 1)] = make_float2(fmaf(-v.x, mean, v.y), 0.f);   // L <= n - 1: no two offsets share an index
    }
    __syncthreads();

    // ---- 2. power spectrum --------------------------------------------------------------------------------------------------
    float2* X = env_fft(buf0, buf1, tw, n, log2n, tid);
    for (int k = tid; k <= nh; k += ENV_THREADS) {
        const float2 v = X[k];
        P[k] = fmaf(v.x, v.x, v.y * v.y) / sum_w2;
    }
    __syncthreads();

    // ---- 3. DC correction ---------------------------------------------------------------------------------------------------
    for (int k = tid; k <= nh; k += ENV_THREADS) {
        float v = P[k];
        if ((double)k < r0) {   // r0 <= n/4 as f0_ceil <= sr/4
            const double u = r0 - (double)k;
            const int i0 = (int)floor(u), i1 = i0 + 1 < nh ? i0 + 1 : nh;
            const float t = (float)(u - (double)i0);
            v += fmaf(t, P[i1], (1.f - t) * P[i0]);
        }
        Pc[k] = v;
    }
    __syncthreads();

    // ---- 4. smoothing over [k - r, k + r] and the log -------------------------------------------------------------------------
    float2* src = X == buf0 ? buf1 : buf0;   // the spectrum has been read: either buffer is free
    float2* dst = X;
    {
        auto cell = [&](int j) {   // the even extensions about 0 and n/2; r + 1/2 < n/2: one reflection
            const int a = j < 0 ? -j : j;
            return Pc[a > nh ? 2 * nh - a : a];
        };
        const float inv = (float)(1.0 / (2.0 * r));
        for (int k = tid; k <= nh; k += ENV_THREADS) {
            const double lo = (double)k - r, hi = (double)k + r;
            const int jl = (int)floor(lo + 0.5), jh = (int)floor(hi + 0.5);
            // cell jl is covered from lo on, cell jh > jl up to hi, the cells between them whole
            float acc = (float)(fmin(hi, (double)jl + 0.5) - lo) * cell(jl);
            for (int j = jl + 1; j < jh; ++j) acc += cell(j);
            if (jh > jl) acc = fmaf((float)(hi - ((double)jh - 0.5)), cell(jh), acc);
            env_put_even(src, k, nh, logf(acc * inv + p.eps));
        }
    }
    __syncthreads();

    // ---- 5. cepstrum, lifter, envelope --------------------------------------------------------------------------------------
    float2* C = env_fft(src, dst, tw, n, log2n, tid);
    src = C == buf0 ? buf1 : buf0;
    dst = C;
    const float inv_n = 1.f / (float)n, q1 = (float)p.q1;
    for (int q = tid; q <= nh; q += ENV_THREADS) {
        float lift = 1.f;
        if (q > 0) {
            const double tq = fe * (double)q / sr;   // cycles of f0 per quefrency: sin(pi tq) from tq mod 2, cos(2 pi tq) from tq mod 1
            const float s = sinpif((float)(tq - 2.0 * floor(0.5 * tq)));
            const float c = cospif((float)(2.0 * (tq - floor(tq))));
            lift = s / (float)(3.14159265358979323846 * tq) * fmaf(2.f * q1, c, 1.f - 2.f * q1);
        }
        const float cl = C[q].x * inv_n * lift;
        if (p.ceps && q < p.n_ceps) p.ceps[(int64_t)g * p.n_ceps + q] = 0.5f * cl + (q == 0 ? off : 0.f);
        env_put_even(src, q, nh, cl);
    }
    if (!p.log_env) return;   // the whole workgroup
    __syncthreads();
    float2* E = env_fft(src, dst, tw, n, log2n, tid);
    for (int k = tid; k <= nh; k += ENV_THREADS) p.log_env[(int64_t)g * (nh + 1) + k] = fmaf(0.5f, E[k].x, off);
}

// the limits both entries share, after their own checks of sizes, pointers and strides; 0 or the code of the refusal
static int env_check_params(const char* who, int n_fft, int n_ceps, int hop, double sample_rate, double f0_floor,
                            double f0_ceil, double unvoiced_f0, double q1, double eps, double voiced_offset) {
    if (n_fft < ENV_MIN_N || n_fft > ENV_MAX_N || (n_fft & (n_fft - 1)))
        return fail(GOLF_EUNSUPPORTED, "%s: n_fft=%d must be a power of two in [%d, %d]", who, n_fft, ENV_MIN_N, ENV_MAX_N);
    const int nb = n_fft / 2 + 1;
    if (hop < 1) return fail(GOLF_EINVAL, "%s: hop=%d must be >= 1", who, hop);
    if (!(sample_rate > 0.0)) return fail(GOLF_EINVAL, "%s: sample_rate=%g must be positive", who, sample_rate);
    if (!(eps > 0.0)) return fail(GOLF_EINVAL, "%s: eps=%g must be positive", who, eps);
    if (n_ceps < 0 || n_ceps > nb) return fail(GOLF_EINVAL, "%s: n_ceps=%d must be 0..%d (n_fft/2 + 1)", who, n_ceps, nb);
    if (!(f0_floor > 0.0)) return fail(GOLF_EINVAL, "%s: f0_floor=%g must be positive", who, f0_floor);
    if (!(f0_floor <= f0_ceil)) return fail(GOLF_EINVAL, "%s: f0_floor=%g must be <= f0_ceil=%g", who, f0_floor, f0_ceil);
    if (!(f0_ceil <= sample_rate / 4.0))
        return fail(GOLF_EINVAL, "%s: f0_ceil=%g must be <= sample_rate/4 = %g", who, f0_ceil, sample_rate / 4.0);
    if (!(unvoiced_f0 >= f0_floor && unvoiced_f0 <= f0_ceil))
        return fail(GOLF_EINVAL, "%s: unvoiced_f0=%g must lie in [f0_floor, f0_ceil] = [%g, %g]", who, unvoiced_f0, f0_floor,
                    f0_ceil);
    if (!(q1 == q1) || !(voiced_offset == voiced_offset))
        return fail(GOLF_EINVAL, "%s: q1=%g and voiced_offset=%g must be numbers", who, q1, voiced_offset);
    const double hw_max = floor(1.5 * sample_rate / f0_floor + 0.5);
    if (!(hw_max <= (double)(n_fft / 2 - 1)))
        return fail(GOLF_EINVAL, "%s: f0_floor=%g: the longest window, 2*%.0f + 1 samples, must fit n_fft=%d (half width <= %d)",
                    who, f0_floor, hw_max, n_fft, n_fft / 2 - 1);
    return GOLF_OK;
}

// the checks both entries share and the launch; `whole`: the one-shot entry, whose buffers are the whole utterance (every
// frame, read as a `last` call reads it) and whose refusals name T and F
static int env_run(const char* who, bool whole, const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                   int64_t f0_stride, int64_t f0_first, int n_f0, float* log_env, float* ceps, int B, int64_t f_first,
                   int n_frames, int last, int n_fft, int n_ceps, int hop, double sample_rate, double f0_floor, double f0_ceil,
                   double unvoiced_f0, double q1, double eps, double voiced_offset, void* stream) {
    const char *nx = whole ? "T" : "n_x", *nf0 = whole ? "F" : "n_f0", *nfr = whole ? "F" : "n_frames";
    if (B < 1 || n_x < 0 || n_f0 < 1 || n_frames < 1)
        return fail(GOLF_EINVAL, "%s: bad size (B=%d %s=%d %s=%d n_frames=%d)", who, B, nx, n_x, nf0, n_f0, n_frames);
    if ((!x && n_x > 0) || !f0) return fail(GOLF_EINVAL, "%s: null pointer (x=%p f0=%p)", who, x, f0);
    if (!log_env && !ceps) return fail(GOLF_EINVAL, "%s: null pointer: log_env and ceps are both NULL", who);
    if (ceps && n_ceps == 0) return fail(GOLF_EINVAL, "%s: n_ceps=0 with a ceps output", who);
    if (x_stride < n_x) return fail(GOLF_EINVAL, "%s: row stride of x %lld < %s=%d", who, (long long)x_stride, nx, n_x);
    if (f0_stride < n_f0) return fail(GOLF_EINVAL, "%s: row stride of f0 %lld < %s=%d", who, (long long)f0_stride, nf0, n_f0);
    if (int rc = env_check_params(who, n_fft, n_ceps, hop, sample_rate, f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset))
        return rc;
    if ((int64_t)B * n_frames >= ((int64_t)1 << 31))
        return fail(GOLF_EINVAL, "%s: B*%s = %lld frames, must be < 2^31", who, nfr, (long long)B * n_frames);
    const int64_t hwmax = (int64_t)floor(1.5 * sample_rate / f0_floor + 0.5);   // <= n_fft/2 - 1: no frame's half window is longer
    if (int rc = frame_position_check(who, x_t0, n_x, f0_first, n_f0, f_first, n_frames, last, hop, hwmax, hwmax + 1, 0, 0))
        return rc;
    EnvArgs a;
    a.x = x, a.x_stride = x_stride, a.f0 = f0, a.f0_stride = f0_stride, a.log_env = log_env, a.ceps = ceps;
    a.x_t0 = x_t0, a.x_end = x_t0 + n_x, a.f0_first = f0_first, a.f_first = f_first;
    a.G = B * n_frames, a.F = n_frames, a.n = n_fft, a.log2n = __builtin_ctz((unsigned)n_fft), a.n_ceps = n_ceps, a.hop = hop;
    a.sample_rate = sample_rate, a.f0_floor = f0_floor, a.f0_ceil = f0_ceil, a.unvoiced_f0 = unvoiced_f0, a.q1 = q1;
    a.voiced_offset = voiced_offset, a.eps = (float)eps;
    const int gx = a.G < ENV_GRID_X ? a.G : ENV_GRID_X;
    hipLaunchKernelGGL(spec_envelope_kernel, dim3((unsigned)gx, (unsigned)ceil_div(a.G, gx)), dim3(ENV_THREADS), 0,
                       (hipStream_t)stream, a);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" int golf_spectral_envelope_f32(const float* x, int64_t x_stride, const float* f0, int64_t f0_stride,
                                          float* log_env, float* ceps, int B, int T, int F, int n_fft, int n_ceps, int hop,
                                          double sample_rate, double f0_floor, double f0_ceil, double unvoiced_f0, double q1,
                                          double eps, double voiced_offset, void* stream) {
    return env_run("spectral_envelope", true, x, x_stride, 0, T, f0, f0_stride, 0, F, log_env, ceps, B, 0, F, 1, n_fft, n_ceps,
                   hop, sample_rate, f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset, stream);
}

extern "C" int golf_spectral_envelope_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                                                 int64_t f0_stride, int64_t f0_first, int n_f0, float* log_env, float* ceps,
                                                 int B, int64_t f_first, int n_frames, int last, int n_fft, int n_ceps, int hop,
                                                 double sample_rate, double f0_floor, double f0_ceil, double unvoiced_f0,
                                                 double q1, double eps, double voiced_offset, void* stream) {
    return env_run("spectral_envelope_stream", false, x, x_stride, x_t0, n_x, f0, f0_stride, f0_first, n_f0, log_env, ceps, B,
                   f_first, n_frames, last, n_fft, n_ceps, hop, sample_rate, f0_floor, f0_ceil, unvoiced_f0, q1, eps,
                   voiced_offset, stream);
}
