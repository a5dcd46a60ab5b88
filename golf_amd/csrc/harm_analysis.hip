// Harmonic-plus-noise analysis for gfx950: (audio, f0) -> harmonic amplitudes and phases and the log magnitudes of the noise
// filter, per frame.  Definition in include/golf_amd.h; the float64 restatement in tests/hna_ref.py is the checker.
//
// One launch, one workgroup of four waves per (b, f) frame; no workspace, no atomics, nothing shared between workgroups.
//   0. Every thread forms the frame's constants in fp64 from the fp32 inputs: the window length L, omega = f0 / sr and the
//      chirp from the neighbouring frames' f0.
//   1. Staging: thread i (strided by 256) loads x[f hop + m], m = i - floor(L/2), zero outside the buffer, and stores the pair
//      (w[i] x, Phi[i]) to LDS: the windowed sample and phi(m) mod 1 formed in fp64 and kept as a Q0.32 fraction of a cycle, so
//      that k phi mod 1 is an exact 32-bit integer product for every harmonic k.
//   2. Projection: a work item is (segment of the window, harmonic); consecutive lanes own consecutive harmonics of one segment,
//      so the LDS reads of the samples are broadcasts and every lane accumulates privately (no cross-lane reduction).  The
//      segments (at most 512 items: two passes of the workgroup) fill the lanes when K < 256.  sin and cos come from v_sin_f32
//      and v_cos_f32, which take revolutions: (float)(k Phi) 2^-32.  The partial sums are added in segment order by thread k.
//   3. Residual: lanes over samples; the phase of harmonic k is a running 32-bit sum of Phi[i]; c_k is a broadcast read.
//      The windowed residual w r replaces w x in LDS.
//   4. Noise: the bins' exponentials have the period N = 2 (n_mag - 1) in m and are even (cos) and odd (sin) about m = 0, so
//      w r is first folded modulo N and then about 0: a bin sums N/2 - 1 (even, odd) pairs whatever L is.  A work item is
//      (segment, bin); the bin's phase advances by its constant Q0.32 step from an exact start.
//   5. Epilogue: S_b = |.|^2 / sum w^2, the box smoothing with reflected ends in fp64, the log.
// Every sum runs in a fixed order: bit-reproducible, and a row does not depend on its batch.  The sums of the window are the
// closed forms sum w = L / 2 and sum w^2 = 3 L / 8 (1 / 2 at L = 2), exact for this Hann window on half-integer offsets.
//
// Two entries launch the kernel.  golf_harmonic_analysis_f32 hands it the whole utterance.  golf_harmonic_analysis_stream_f32
// (analysis_stream.HarmonicNoiseStream) hands it windows of x and f0 with their positions in the utterance and a range of
// frames: the kernel indexes both buffers relative to those positions and asks of each neighbouring f0 frame whether it lies
// in the window, and nothing else differs -- a frame has the same bits from either entry.  The stream entry refuses, before
// the launch, every window from which a frame could read outside its buffers.
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int HNA_THREADS = 256;
constexpr int HNA_MAX_L = 2048;              // window samples
constexpr int HNA_MAX_K = 256;               // harmonics
constexpr int HNA_MAX_NMAG = 513;            // noise bins
constexpr int HNA_ITEMS = 512;               // (segment, harmonic or bin) items when the count allows segments
constexpr int HNA_MAX_SEG = 32;
constexpr int HNA_PART = HNA_MAX_NMAG > HNA_ITEMS ? HNA_MAX_NMAG : HNA_ITEMS;
constexpr int HNA_GRID_X = 1 << 20;          // frames per grid row

struct HnaArgs {
    const float* x;
    int64_t x_stride;
    const float* f0;
    int64_t f0_stride;
    float* amp;
    float* phases;
    float* log_mag;
    // where the buffers sit in the utterance: x holds samples [x_t0, x_end), f0 frames [f0_first, f0_end), and the launch
    // computes frames [f_first, f_first + nf) of every row.  The one-shot entry: 0, T, 0, F, 0, F.
    int64_t x_t0, x_end, f0_first, f0_end, f_first;
    int G, nf, K, n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth;
    double sample_rate, eps;
};

// sin and cos of 2 pi p / 2^32
__device__ __forceinline__ void hna_sincos(unsigned p, float& s, float& c) {
    const float rev = (float)p * 2.3283064365386963e-10f;   // [0, 1] revolutions, rounded to 24 bits
    s = __builtin_amdgcn_sinf(rev);
    c = __builtin_amdgcn_cosf(rev);
}

__device__ __forceinline__ float hna_window(int i, int L) { return 0.5f - 0.5f * cospif((float)(2 * i + 1) / (float)L); }

__global__ __launch_bounds__(HNA_THREADS) void harm_analysis_kernel(const HnaArgs p) {
    __shared__ float2 sp[HNA_MAX_L];      // (w x, later w r; Phi as bits)
    __shared__ float2 part[HNA_PART];     // partial sums of the items
    __shared__ float2 ck[HNA_MAX_K];      // c_k
    __shared__ float S[HNA_MAX_NMAG];
    __shared__ float2 eo[HNA_MAX_NMAG - 1];   // the folded residual: even and odd parts about m = 0
    const int tid = threadIdx.x;
    const int64_t g64 = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (g64 >= p.G) return;
    const int g = (int)g64, b = g / p.nf, K = p.K, n_mag = p.n_mag;
    const int64_t f = p.f_first + (g - b * p.nf);   // the frame's index in the utterance
    const float* xr = p.x + (int64_t)b * p.x_stride;                          // xr[t - x_t0]: sample t, x_t0 <= t < x_end
    const float* fr = p.f0 + (int64_t)b * p.f0_stride + (f - p.f0_first);    // fr[0]: this frame; fr[-1], fr[1]: its neighbours

    // ---- 0. frame constants -------------------------------------------------------------------------------------------------
    const float f0c = fr[0];
    const bool voiced = f0c > 0.f;   // false for a NaN
    const double sr = p.sample_rate;
    double omega = 0.0, chirp = 0.0;
    int L = p.unvoiced_window;
    if (voiced) {
        const double fd = (double)f0c;
        double n_per = ceil((double)p.min_window * fd / sr);
        if (!(n_per >= (double)p.periods)) n_per = (double)p.periods;
        const double v = floor(n_per * sr / fd + 0.5);
        L = v >= 2.0 ? (v <= (double)p.max_window ? (int)v : p.max_window) : 2;   // 2 for a NaN (f0 = +inf)
        omega = fd / sr;
        const float fp = f - 1 >= p.f0_first ? fr[-1] : 0.f, fn = f + 1 < p.f0_end ? fr[1] : 0.f;   // the neighbours that exist
        const double hs = (double)p.hop * sr;
        if (fp > 0.f && fn > 0.f) chirp = ((double)fn - (double)fp) / (2.0 * hs);
        else if (fn > 0.f) chirp = ((double)fn - fd) / hs;
        else if (fp > 0.f) chirp = (fd - (double)fp) / hs;
    }
    const int half = L >> 1;
    const double sum_w = 0.5 * L, sum_w2 = L == 2 ? 0.5 : 0.375 * L;

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    const int64_t t0 = f * p.hop - half;
    for (int i = tid; i < L; i += HNA_THREADS) {
        const int64_t t = t0 + i;
        const float xv = (t >= p.x_t0 && t < p.x_end) ? xr[t - p.x_t0] : 0.f;   // x_t0 <= max(0, t0): below it only t < 0
        unsigned Phi = 0u;
        if (voiced) {
            const double m = (double)(i - half);
            double ph = omega * m + chirp * m * m * 0.5;
            ph -= floor(ph);
            Phi = (unsigned)(unsigned long long)(ph * 4294967296.0 + 0.5);   // 2^32 wraps to 0
        }
        sp[i] = make_float2(hna_window(i, L) * xv, __uint_as_float(Phi));
    }
    __syncthreads();

    if (voiced) {
        // ---- 2. projection --------------------------------------------------------------------------------------------------
        int nseg = HNA_ITEMS / K;
        nseg = nseg > HNA_MAX_SEG ? HNA_MAX_SEG : nseg;   // >= 2 as K <= 256
        const int seglen = (L + nseg - 1) / nseg, items = K * nseg;
        for (int item = tid; item < items; item += HNA_THREADS) {
            const int seg = item / K, k = item - seg * K + 1;
            float ar = 0.f, ai = 0.f;
            if ((double)k * omega < 0.5) {
                const int i0 = seg * seglen, i1 = i0 + seglen < L ? i0 + seglen : L;
#pragma unroll 4
                for (int i = i0; i < i1; ++i) {
                    const float2 v = sp[i];
                    float s, c;
                    hna_sincos((unsigned)k * __float_as_uint(v.y), s, c);
                    ar = fmaf(v.x, c, ar);
                    ai = fmaf(v.x, s, ai);
                }
            }
            part[item] = make_float2(ar, ai);
        }
        __syncthreads();
        const bool live = tid < K && (double)(tid + 1) * omega < 0.5;   // below Nyquist: a prefix of the harmonics
        if (tid < K) {
            float ar = 0.f, ai = 0.f;
            for (int seg = 0; seg < nseg; ++seg) {
                const float2 v = part[seg * K + tid];
                ar += v.x, ai += v.y;
            }
            const float scale = (float)(2.0 / sum_w);
            const float cre = live ? ar * scale : 0.f, cim = live ? -ai * scale : 0.f;   // c_k = scale sum w x exp(-2 pi j k phi)
            ck[tid] = make_float2(cre, cim);
            const float a = sqrtf(fmaf(cre, cre, cim * cim));
            p.amp[(int64_t)g * K + tid] = a;
            if (p.phases) {
                float ph = a > 0.f ? fmaf(atan2f(cim, cre), 0.15915494309189535f, 0.25f) : 0.25f;   // (-1/4, 3/4]
                if (ph < 0.f) ph += 1.f;
                if (ph >= 1.f) ph -= 1.f;
                p.phases[(int64_t)g * K + tid] = ph;
            }
        }
        const int kact = __syncthreads_count(live);
        if (!(n_mag > 0 && p.log_mag)) return;

        // ---- 3. residual ----------------------------------------------------------------------------------------------------
        for (int i = tid; i < L; i += HNA_THREADS) {
            const float2 v = sp[i];
            const unsigned Phi = __float_as_uint(v.y);
            unsigned ph = 0u;
            float model = 0.f;
#pragma unroll 4
            for (int k = 0; k < kact; ++k) {
                ph += Phi;
                const float2 c = ck[k];
                float s, co;
                hna_sincos(ph, s, co);
                model = fmaf(c.x, co, model);    // Re(c_k exp(2 pi j k phi))
                model = fmaf(-c.y, s, model);
            }
            sp[i].x = fmaf(-hna_window(i, L), model, v.x);
        }
        __syncthreads();
    } else {
        if (tid < K) {
            p.amp[(int64_t)g * K + tid] = 0.f;
            if (p.phases) p.phases[(int64_t)g * K + tid] = 0.f;
        }
        if (!(n_mag > 0 && p.log_mag)) return;
    }

    // ---- 4. noise spectrum --------------------------------------------------------------------------------------------------
    {
        // the bins' exponentials have the period N = 2 (n_mag - 1) in m and are even (cos) and odd (sin) about 0: fold w r
        // modulo N, A[j] = sum of w r over m = j mod N, and then about 0, so that a bin sums N/2 - 1 terms whatever L is
        const int nh = n_mag - 1, N = 2 * nh;
        auto fold = [&](int j) {
            float a = 0.f;
            for (int i = (j + half) % N; i < L; i += N) a += sp[i].x;   // m = i - half = j mod N, ascending
            return a;
        };
        for (int j = tid; j < nh; j += HNA_THREADS) {
            const float a = fold(j), b2 = fold(j ? N - j : nh);
            eo[j] = j ? make_float2(a + b2, a - b2) : make_float2(a, b2);   // eo[0]: the two terms without a partner, A[0] and A[N/2]
        }
        __syncthreads();
        int nseg = HNA_ITEMS / n_mag;
        nseg = nseg > HNA_MAX_SEG ? HNA_MAX_SEG : (nseg < 1 ? 1 : nseg);
        const int seglen = (nh - 1 + nseg - 1) / nseg, items = n_mag * nseg;   // terms j = 1 .. nh - 1
        const double rev = 4294967296.0 / (double)N;
        for (int item = tid; item < items; item += HNA_THREADS) {
            const int seg = item / n_mag, bin = item - seg * n_mag;
            const unsigned step = (unsigned)(unsigned long long)rint((double)bin * rev);   // bin / N <= 1/2 of a cycle per sample
            const int j0 = 1 + seg * seglen, j1 = j0 + seglen < nh ? j0 + seglen : nh;
            unsigned ph = step * (unsigned)j0;   // modulo 2^32: the cycle
            float ar = 0.f, ai = 0.f;
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const float2 v = eo[j];
                float s, c;
                hna_sincos(ph, s, c);
                ar = fmaf(v.x, c, ar);
                ai = fmaf(v.y, s, ai);
                ph += step;
            }
            part[item] = make_float2(ar, ai);
        }
        __syncthreads();
        for (int bin = tid; bin < n_mag; bin += HNA_THREADS) {
            float ar = 0.f, ai = 0.f;
            for (int seg = 0; seg < nseg; ++seg) {
                const float2 v = part[seg * n_mag + bin];
                ar += v.x, ai += v.y;
            }
            const float2 lone = eo[0];
            ar += lone.x;
            ar += (bin & 1) ? -lone.y : lone.y;   // exp(-j pi bin) at m = N/2
            S[bin] = (float)(((double)ar * (double)ar + (double)ai * (double)ai) / sum_w2);
        }
        __syncthreads();

        // ---- 5. smoothing and log -------------------------------------------------------------------------------------------
        const int sm = p.smooth, last = n_mag - 1;
        for (int bin = tid; bin < n_mag; bin += HNA_THREADS) {
            double acc = 0.0;
            for (int j = bin - sm; j <= bin + sm; ++j) {
                const int r = j < 0 ? -j : (j > last ? 2 * last - j : j);   // sm <= last: one reflection
                acc += (double)S[r];
            }
            const double mean = acc / (double)(2 * sm + 1);
            p.log_mag[(int64_t)g * n_mag + bin] = 0.5f * logf((float)(mean + p.eps));
        }
    }
}

// the limits both entries share; 0 or the code of the refusal
static int hna_check_params(const char* who, int K, int n_mag, int hop, int periods, int min_window, int max_window,
                            int unvoiced_window, int smooth, double sample_rate, double eps) {
    if (K < 1 || K > HNA_MAX_K) return fail(GOLF_EINVAL, "%s: K=%d harmonics, must be 1..%d", who, K, HNA_MAX_K);
    if (n_mag < 0 || n_mag == 1 || n_mag > HNA_MAX_NMAG)
        return fail(GOLF_EINVAL, "%s: n_mag=%d noise bins, must be 0 (none) or 2..%d", who, n_mag, HNA_MAX_NMAG);
    if (hop < 1) return fail(GOLF_EINVAL, "%s: hop=%d must be >= 1", who, hop);
    if (periods < 2) return fail(GOLF_EINVAL, "%s: periods=%d must be >= 2", who, periods);
    if (max_window < 2 || max_window > HNA_MAX_L)
        return fail(GOLF_EINVAL, "%s: max_window=%d must be 2..%d (a frame must fit LDS)", who, max_window, HNA_MAX_L);
    if (min_window < 1 || min_window > max_window)
        return fail(GOLF_EINVAL, "%s: min_window=%d must be 1..max_window=%d", who, min_window, max_window);
    if (unvoiced_window < 2 || unvoiced_window > HNA_MAX_L)
        return fail(GOLF_EINVAL, "%s: unvoiced_window=%d must be 2..%d (a frame must fit LDS)", who, unvoiced_window,
                    HNA_MAX_L);
    if (smooth < 0 || (n_mag > 0 && smooth >= n_mag))
        return fail(GOLF_EINVAL, "%s: smooth=%d must be 0..n_mag-1 (n_mag=%d)", who, smooth, n_mag);
    if (!(sample_rate > 0.0)) return fail(GOLF_EINVAL, "%s: sample_rate=%g must be positive", who, sample_rate);
    if (!(eps >= 0.0)) return fail(GOLF_EINVAL, "%s: eps=%g must be >= 0", who, eps);
    return GOLF_OK;
}

// the checks both entries share and the launch; `whole`: the one-shot entry, whose buffers are the whole utterance (every
// frame, read as a `last` call reads it) and whose refusals name T and F
static int hna_run(const char* who, bool whole, const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                   int64_t f0_stride, int64_t f0_first, int n_f0, float* amplitudes, float* phases, float* log_mag, int B,
                   int64_t f_first, int n_frames, int last, int K, int n_mag, int hop, int periods, int min_window,
                   int max_window, int unvoiced_window, int smooth, double sample_rate, double eps, void* stream) {
    const char *nx = whole ? "T" : "n_x", *nf0 = whole ? "F" : "n_f0", *nfr = whole ? "F" : "n_frames";
    if (B < 1 || n_x < 0 || n_f0 < 1 || n_frames < 1)
        return fail(GOLF_EINVAL, "%s: bad size (B=%d %s=%d %s=%d n_frames=%d)", who, B, nx, n_x, nf0, n_f0, n_frames);
    if ((!x && n_x > 0) || !f0 || !amplitudes)
        return fail(GOLF_EINVAL, "%s: null pointer (x=%p f0=%p amplitudes=%p)", who, x, f0, amplitudes);
    if (x_stride < n_x) return fail(GOLF_EINVAL, "%s: row stride of x %lld < %s=%d", who, (long long)x_stride, nx, n_x);
    if (f0_stride < n_f0) return fail(GOLF_EINVAL, "%s: row stride of f0 %lld < %s=%d", who, (long long)f0_stride, nf0, n_f0);
    if (int rc = hna_check_params(who, K, n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth, sample_rate,
                                  eps))
        return rc;
    if ((int64_t)B * n_frames >= ((int64_t)1 << 31))
        return fail(GOLF_EINVAL, "%s: B*%s = %lld frames, must be < 2^31", who, nfr, (long long)B * n_frames);
    const int Lmax = max_window > unvoiced_window ? max_window : unvoiced_window;   // no frame's window is longer
    if (int rc = frame_position_check(who, x_t0, n_x, f0_first, n_f0, f_first, n_frames, last, hop, Lmax / 2, Lmax - Lmax / 2,
                                      1, 1))
        return rc;
    HnaArgs a;
    a.x = x, a.x_stride = x_stride, a.f0 = f0, a.f0_stride = f0_stride;
    a.amp = amplitudes, a.phases = phases, a.log_mag = log_mag;
    a.x_t0 = x_t0, a.x_end = x_t0 + n_x, a.f0_first = f0_first, a.f0_end = f0_first + n_f0, a.f_first = f_first;
    a.G = B * n_frames, a.nf = n_frames, a.K = K, a.n_mag = n_mag, a.hop = hop, a.periods = periods;
    a.min_window = min_window, a.max_window = max_window, a.unvoiced_window = unvoiced_window, a.smooth = smooth;
    a.sample_rate = sample_rate, a.eps = eps;
    const int gx = a.G < HNA_GRID_X ? a.G : HNA_GRID_X;
    hipLaunchKernelGGL(harm_analysis_kernel, dim3((unsigned)gx, (unsigned)ceil_div(a.G, gx)), dim3(HNA_THREADS), 0,
                       (hipStream_t)stream, a);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" int golf_harmonic_analysis_f32(const float* x, int64_t x_stride, const float* f0, int64_t f0_stride,
                                          float* amplitudes, float* phases, float* log_mag, int B, int T, int F, int K,
                                          int n_mag, int hop, int periods, int min_window, int max_window,
                                          int unvoiced_window, int smooth, double sample_rate, double eps, void* stream) {
    return hna_run("harmonic_analysis", true, x, x_stride, 0, T, f0, f0_stride, 0, F, amplitudes, phases, log_mag, B, 0, F, 1, K,
                   n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth, sample_rate, eps, stream);
}

extern "C" int golf_harmonic_analysis_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                                                 int64_t f0_stride, int64_t f0_first, int n_f0, float* amplitudes,
                                                 float* phases, float* log_mag, int B, int64_t f_first, int n_frames,
                                                 int last, int K, int n_mag, int hop, int periods, int min_window,
                                                 int max_window, int unvoiced_window, int smooth, double sample_rate,
                                                 double eps, void* stream) {
    return hna_run("harmonic_analysis_stream", false, x, x_stride, x_t0, n_x, f0, f0_stride, f0_first, n_f0, amplitudes, phases,
                   log_mag, B, f_first, n_frames, last, K, n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth,
                   sample_rate, eps, stream);
}
