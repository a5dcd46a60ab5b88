// Glottal-source analysis for gfx950: (a residual's harmonics, f0) -> the table position w, the table phase theta and the fit
// rho, per frame: an exhaustive match of the frame's harmonics against every table row at every phase shift.  Definition in
// include/golf_amd.h; the float64 restatement in tests/glottal_ref.py is the checker.
//
// One launch, one workgroup of four waves per (b, f) frame; no workspace, no atomics, nothing shared between workgroups.
//   0. Every thread forms the frame's constants in fp64 from the fp32 inputs: omega = f0 / sr, the number of live harmonics Hf
//      (the muting rule of harm_analysis.hip, h omega < 0.5) and E2; c_h goes to LDS in fp64 and in fp32.
//   1. The constant right factor, exp(2 pi j i / n_phi) for i = 0 .. n_phi - 1, is a table in LDS; h j mod n_phi indexes it.
//   2. Scores, a tile of 16 rows at a time: D[k,h] = c_h conj(S[k,h]) goes to LDS (harmonic major, so that a wave reads its four
//      rows as one 16-byte broadcast); a lane owns 4 rows x 4 columns (j, j + 64, j + 128, j + 192 of a chunk of 256 columns)
//      and accumulates C[k,j] = sum_h D.re cos + D.im sin with fmaf, h ascending, in registers: 32 FMAs for 6 LDS reads.
//      rho = C inv_k, inv_k = 1 / sqrt(N[k,Hf] E2) formed in fp64 per row; every lane keeps the best (rho, k, j) it has seen.
//      The K x n_phi scores exist in registers only.
//   3. The workgroup reduces its 256 candidates over a fixed tree in LDS; the order is total (larger rho, then smaller k, then
//      smaller j), so the result does not depend on the tree.
//   4. The fp32 winner can be a neighbour of the true one where two cells tie within fp32 rounding (the table's rows are that
//      close), and the refinements are discontinuous across such a flip.  So the 5 x 5 scores around it are formed again in
//      fp64 (c_h unrounded, sincospi of the exact fraction), the winner is taken among the inner 3 x 3, and
//   5. lane 0 does the two refinements in fp64 on those scores and writes the frame's three floats.
// Every sum runs in a fixed order: bit-reproducible, and a row does not depend on its batch.
#include "common.h"

namespace golf {

constexpr int GM_THREADS = 256;
constexpr int GM_MAX_H = 256;                // harmonics
constexpr int GM_MAX_K = 1024;               // table rows
constexpr int GM_MIN_NPHI = 8;
constexpr int GM_MAX_NPHI = 4096;            // phase shifts: the table of step 1 takes 8 n_phi bytes of LDS
constexpr int GM_ROWS = 16;                  // rows per tile: 4 per wave
constexpr int GM_HC = 128;                   // harmonics of a tile held in LDS at a time
constexpr int GM_COLS = 256;                 // columns per chunk: 4 per lane
constexpr int GM_NB = 5;                     // the fp64 neighbourhood of the fp32 winner: GM_NB x GM_NB scores
constexpr int GM_PARTS = 10;                 // lanes per score of it
constexpr int GM_GRID_X = 1 << 20;           // frames per grid row

struct GmArgs {
    const float* amp;
    const float* phases;
    const float* f0;
    int64_t f0_stride;
    const float* S;      // (K, H, 2)
    const float* N;      // (K, H)
    const float* X;      // (K - 1, H)
    float* w;
    float* theta;
    float* rho;
    int G, F, H, K, n_phi;
    double sample_rate;
};

// D = c conj(S) in fp32
__device__ __forceinline__ float2 gm_d(float2 c, float2 s) {
    return make_float2(fmaf(c.x, s.x, c.y * s.y), fmaf(c.y, s.x, -(c.x * s.y)));
}

// larger score first, then the smaller row, then the smaller column; a NaN never wins
__device__ __forceinline__ bool gm_better(float v, int k, int j, float bv, int bk, int bj) {
    return v > bv || (v == bv && (k < bk || (k == bk && j < bj)));
}

__global__ __launch_bounds__(GM_THREADS) void glottal_match_kernel(const GmArgs p) {
    extern __shared__ float2 tw[];                  // n_phi entries: (cos, sin) of 2 pi i / n_phi
    __shared__ float2 cs[GM_MAX_H];                 // c_h
    __shared__ __attribute__((aligned(16))) float dre[GM_HC * GM_ROWS], dim[GM_HC * GM_ROWS];
    __shared__ float inv[GM_ROWS];
    __shared__ float red_v[GM_THREADS];
    __shared__ int red_k[GM_THREADS], red_j[GM_THREADS];
    __shared__ double2 cd[GM_MAX_H];                // c_h before it is rounded
    __shared__ double part64[GM_NB * GM_NB * GM_PARTS], c64[GM_NB * GM_NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g64 = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (g64 >= p.G) return;
    const int g = (int)g64, b = g / p.F, f = g - b * p.F;
    const int H = p.H, K = p.K, n = p.n_phi, mask = n - 1;

    // ---- 0. frame constants -------------------------------------------------------------------------------------------------
    const float f0v = p.f0[(int64_t)b * p.f0_stride + f];
    const bool voiced = f0v > 0.f;   // false for a NaN
    const double omega = voiced ? (double)f0v / p.sample_rate : 0.0;
    const bool live = voiced && tid < H && (double)(tid + 1) * omega < 0.5;   // below Nyquist: a prefix of the harmonics
    if (tid < H) {
        const float a = p.amp[(int64_t)g * H + tid];
        double s, c;
        sincospi(2.0 * ((double)p.phases[(int64_t)g * H + tid] - 0.25), &s, &c);
        const double cr = (double)a * c, ci = (double)a * s;
        cd[tid] = make_double2(cr, ci);
        cs[tid] = make_float2((float)cr, (float)ci);
        red_v[tid] = a;
    }
    const int Hf = __syncthreads_count(live);   // and cs, red_v are visible
    double E2 = 0.0;
    for (int h = 0; h < Hf; ++h) E2 = fma((double)red_v[h], (double)red_v[h], E2);   // every thread, the same order
    if (!(Hf > 0 && E2 > 0.0)) {   // unvoiced, nothing below Nyquist, an all-zero (or NaN) frame: the whole workgroup
        if (tid == 0) {
            if (p.w) p.w[g] = __builtin_nanf("");
            if (p.theta) p.theta[g] = 0.f;
            if (p.rho) p.rho[g] = 0.f;
        }
        return;
    }

    // ---- 1. the right factor ------------------------------------------------------------------------------------------------
    for (int i = tid; i < n; i += GM_THREADS) {
        float s, c;
        sincospif((float)(2 * i) / (float)n, &s, &c);   // 2 i / n is exact
        tw[i] = make_float2(c, s);
    }

    // ---- 2. scores ----------------------------------------------------------------------------------------------------------
    float bv = -__builtin_inff();
    int bk = 0, bj = 0;
    const bool one_chunk = Hf <= GM_HC;   // then a tile's D serves all its column chunks
    for (int k0 = 0; k0 < K; k0 += GM_ROWS) {
        for (int jc = 0; jc < n; jc += GM_COLS) {
            float acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[r][m] = 0.f;
            int jm[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) jm[m] = jc + lane + 64 * m;   // may reach n and beyond when n < 256: masked, not scored
            for (int h0 = 0; h0 < Hf; h0 += GM_HC) {
                const int hc = Hf - h0 < GM_HC ? Hf - h0 : GM_HC;
                if (!(one_chunk && jc > 0)) {
                    __syncthreads();   // the readers of the previous D (and of inv) are done; tw is visible
                    for (int item = tid; item < hc * GM_ROWS; item += GM_THREADS) {
                        const int r = item & (GM_ROWS - 1), hh = item >> 4, k = k0 + r, h = h0 + hh;
                        float2 d = make_float2(0.f, 0.f);
                        if (k < K) {
                            const float2 s = *reinterpret_cast<const float2*>(p.S + 2 * ((int64_t)k * H + h));
                            d = gm_d(cs[h], s);
                        }
                        dre[item] = d.x, dim[item] = d.y;
                    }
                    if (h0 == 0 && tid < GM_ROWS) {
                        const int k = k0 + tid;
                        const double nk = k < K ? (double)p.N[(int64_t)k * H + Hf - 1] : 0.0;
                        inv[tid] = nk > 0.0 ? (float)(1.0 / sqrt(nk * E2)) : 0.f;   // a row without energy scores 0
                    }
                    __syncthreads();
                }
                int idx[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) idx[m] = ((h0 + 1) * jm[m]) & mask;   // h j mod n, h = h0 + 1: exact in 32 bits
                for (int hh = 0; hh < hc; ++hh) {
                    const float4 a4 = *reinterpret_cast<const float4*>(&dre[hh * GM_ROWS + 4 * wave]);
                    const float4 b4 = *reinterpret_cast<const float4*>(&dim[hh * GM_ROWS + 4 * wave]);
                    const float ar[4] = {a4.x, a4.y, a4.z, a4.w}, ai[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float2 t = tw[idx[m]];
                        idx[m] = (idx[m] + jm[m]) & mask;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            acc[r][m] = fmaf(ar[r], t.x, acc[r][m]);
                            acc[r][m] = fmaf(ai[r], t.y, acc[r][m]);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + 4 * wave + r;
                const float ik = inv[4 * wave + r];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float v = acc[r][m] * ik;
                    if (k < K && jm[m] < n && gm_better(v, k, jm[m], bv, bk, bj)) bv = v, bk = k, bj = jm[m];
                }
            }
        }
    }

    // ---- 3. argmax over the workgroup ---------------------------------------------------------------------------------------
    __syncthreads();   // (red_v held the amplitudes until E2 was summed, many barriers ago)
    red_v[tid] = bv, red_k[tid] = bk, red_j[tid] = bj;
    __syncthreads();
    for (int s = GM_THREADS >> 1; s > 0; s >>= 1) {
        if (tid < s && gm_better(red_v[tid + s], red_k[tid + s], red_j[tid + s], red_v[tid], red_k[tid], red_j[tid]))
            red_v[tid] = red_v[tid + s], red_k[tid] = red_k[tid + s], red_j[tid] = red_j[tid + s];
        __syncthreads();
    }
    const int ks = red_k[0], js = red_j[0];

    // ---- 4. the winner again, in fp64 -----------------------------------------------------------------------------------------
    // the 5 x 5 scores around (ks, js): 10 lanes per cell sum a tenth of the harmonics each, then one lane per cell adds the
    // tenths in order.  Rows outside the table stay 0 and are never read.
    if (tid < GM_NB * GM_NB * GM_PARTS) {
        const int cell = tid / GM_PARTS, q = tid - cell * GM_PARTS;
        const int k = ks - 2 + cell / GM_NB, j = (js - 2 + cell % GM_NB) & mask;
        const int per = (Hf + GM_PARTS - 1) / GM_PARTS, hb = q * per, he = hb + per < Hf ? hb + per : Hf;
        double acc = 0.0;
        if (k >= 0 && k < K) {
            for (int h = hb; h < he; ++h) {
                const float2 s = *reinterpret_cast<const float2*>(p.S + 2 * ((int64_t)k * H + h));
                const double2 c = cd[h];
                double sn, cn;
                sincospi(2.0 * (double)(((h + 1) * j) & mask) / (double)n, &sn, &cn);   // an exact fraction of a cycle
                const double dx = c.x * (double)s.x + c.y * (double)s.y, dy = c.y * (double)s.x - c.x * (double)s.y;
                acc += dx * cn + dy * sn;
            }
        }
        part64[tid] = acc;
    }
    __syncthreads();
    if (tid < GM_NB * GM_NB) {
        double acc = 0.0;
        for (int q = 0; q < GM_PARTS; ++q) acc += part64[tid * GM_PARTS + q];
        c64[tid] = acc;
    }
    __syncthreads();
    if (tid != 0) return;
    const int64_t hl = Hf - 1;
    auto row_norm = [&](int k) { return (double)p.N[(int64_t)k * H + hl]; };
    int rf = 2, cf = 2;
    {
        double bvd = -1.0 / 0.0;
        int bkd = 0, bjd = 0;
        for (int r = 1; r <= 3; ++r) {
            const int k = ks - 2 + r;
            if (k < 0 || k >= K) continue;
            const double nk = row_norm(k);
            for (int cc = 1; cc <= 3; ++cc) {
                const int j = (js - 2 + cc) & mask;
                const double v = nk > 0.0 ? c64[r * GM_NB + cc] / sqrt(nk * E2) : 0.0;
                if (v > bvd || (v == bvd && (k < bkd || (k == bkd && j < bjd)))) bvd = v, bkd = k, bjd = j, rf = r, cf = cc;
            }
        }
    }
    const int kf = ks - 2 + rf, jf = (js - 2 + cf) & mask;

    // ---- 5. refinement ------------------------------------------------------------------------------------------------------
    const double ym = c64[rf * GM_NB + cf - 1], y0 = c64[rf * GM_NB + cf], yp = c64[rf * GM_NB + cf + 1];
    const double curv = ym - 2.0 * y0 + yp;   // one row: the parabola's vertex does not depend on its scale
    double d = curv != 0.0 ? 0.5 * (ym - yp) / curv : 0.0;
    d = d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
    double th = ((double)jf + d) / (double)n;
    th -= floor(th);
    float thf = (float)th;
    if (thf >= 1.f) thf = 0.f;
    const double nss = row_norm(kf);
    double best = nss > 0.0 ? y0 / sqrt(nss * E2) : 0.0, wk = (double)kf;
    for (int side = 0; side < 2; ++side) {
        const int ka = kf - 1 + side;   // the pair (ka, ka + 1)
        if (ka < 0 || ka + 1 >= K) continue;
        const double c0 = side ? y0 : c64[(rf - 1) * GM_NB + cf], c1 = side ? c64[(rf + 1) * GM_NB + cf] : y0;
        const double n00 = row_norm(ka), n11 = row_norm(ka + 1), n01 = (double)p.X[(int64_t)ka * H + hl];
        const double u = c1 * n00 - c0 * n01, v = c0 * n11 - c1 * n01;
        double q = u + v != 0.0 ? u / (u + v) : 0.0;
        q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);   // a NaN stays: it then loses every comparison below
        const double nb = (1.0 - q) * (1.0 - q) * n00 + 2.0 * q * (1.0 - q) * n01 + q * q * n11;
        const double sc = nb > 0.0 ? ((1.0 - q) * c0 + q * c1) / sqrt(nb * E2) : 0.0;
        if (sc > best) best = sc, wk = (double)ka + q;
    }
    if (p.w) p.w[g] = (float)(wk / (double)(K - 1));
    if (p.theta) p.theta[g] = thf;
    if (p.rho) p.rho[g] = (float)best;
}

}  // namespace golf

using namespace golf;

extern "C" int golf_glottal_match_f32(const float* amplitudes, const float* phases, const float* f0, int64_t f0_stride,
                                      const float* spectrum, const float* norms, const float* cross, float* w, float* theta,
                                      float* rho, int B, int F, int H, int K, int n_phi, double sample_rate, void* stream) {
    const char* who = "glottal_match";
    if (B < 1 || F < 1) return fail(GOLF_EINVAL, "%s: bad size (B=%d F=%d)", who, B, F);
    if (H < 1 || H > GM_MAX_H) return fail(GOLF_EINVAL, "%s: H=%d harmonics, must be 1..%d", who, H, GM_MAX_H);
    if (K < 2 || K > GM_MAX_K) return fail(GOLF_EINVAL, "%s: K=%d table rows, must be 2..%d", who, K, GM_MAX_K);
    if (n_phi < GM_MIN_NPHI || n_phi > GM_MAX_NPHI || (n_phi & (n_phi - 1)))
        return fail(GOLF_EUNSUPPORTED, "%s: n_phi=%d must be a power of two in [%d, %d]", who, n_phi, GM_MIN_NPHI,
                    GM_MAX_NPHI);
    if (!amplitudes || !phases || !f0)
        return fail(GOLF_EINVAL, "%s: null pointer (amplitudes=%p phases=%p f0=%p)", who, amplitudes, phases, f0);
    if (!spectrum || !norms || !cross)
        return fail(GOLF_EINVAL, "%s: null pointer in the plan (spectrum=%p norms=%p cross=%p)", who, spectrum, norms, cross);
    if (!w && !theta && !rho) return fail(GOLF_EINVAL, "%s: null pointer: w, theta and rho are all NULL", who);
    if (f0_stride < F) return fail(GOLF_EINVAL, "%s: row stride of f0 %lld < F=%d", who, (long long)f0_stride, F);
    if (!(sample_rate > 0.0)) return fail(GOLF_EINVAL, "%s: sample_rate=%g must be positive", who, sample_rate);
    if ((int64_t)B * F >= ((int64_t)1 << 31))
        return fail(GOLF_EINVAL, "%s: B*F = %lld frames, must be < 2^31", who, (long long)B * F);
    GmArgs a;
    a.amp = amplitudes, a.phases = phases, a.f0 = f0, a.f0_stride = f0_stride;
    a.S = spectrum, a.N = norms, a.X = cross, a.w = w, a.theta = theta, a.rho = rho;
    a.G = B * F, a.F = F, a.H = H, a.K = K, a.n_phi = n_phi, a.sample_rate = sample_rate;
    const int gx = a.G < GM_GRID_X ? a.G : GM_GRID_X;
    hipLaunchKernelGGL(glottal_match_kernel, dim3((unsigned)gx, (unsigned)ceil_div(a.G, gx)), dim3(GM_THREADS),
                       (size_t)n_phi * sizeof(float2), (hipStream_t)stream, a);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}
