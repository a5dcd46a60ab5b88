// Mel-cepstral filter design for gfx950: mel cepstra -> complex minimum-phase response rows on bins 0 .. N/2, and its
// adjoint.  The design step of LTVMLSAFilter2 (reference models/filters.py:626-684); definition in include/golf_amd.h:
//   theta_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k),   w_k = 2 pi k / N,   k = 0 .. N/2
//   L_k = sum_{m=0..M} mc[m] (cos(m theta_k) - j sin(m theta_k)),   H_k = exp(Re L_k) (cos(Im L_k) + j sin(Im L_k))
// The warped cepstrum is causal, so Im L is the minimum phase: no Hilbert transform, one real (M+1) x (N/2+1) contraction
// per part.  `basis` holds cos(m theta_k) and sin(m theta_k), evaluated in float64 and rounded once:
//   basis[m * Kp + k] = cos(m theta_k),  basis[(M+1) * Kp + m * Kp + k] = sin(m theta_k),   Kp = N/2 + 64, zero for k > N/2
// (the sine exactly 0 at k = 0 and k = N/2: H is real there, which the Hermitian extension of the frame filter needs).
//
// Forward: one wave owns 16 rows x 64 bins; its 16 mel cepstra sit in LDS ([m][row], read as broadcast float4), every lane
// keeps its bin's 32 accumulators in registers and reads its basis column once per m (L2 resident: 2 (M+1) Kp floats).  The
// store of h is the only pass over row-sized data.  Every output is a sum over m = 0 .. M in that order with fused
// multiply-adds, so a row's bits depend on its mel cepstrum and the basis alone -- not on R or on where the row sits.
// Plain FMAs: at N 1024, M 24 a row is 2 x 25 x 513 FMAs, 513 exp and 513 sincos against 4104 bytes stored (DESIGN.md has
// the measured time: the kernel is not bound by the store).
// Backward: a workgroup of 4 waves owns RB rows (8, or 4 at N 2048: the LDS holds their P / Q rows).  Phase 1 recomputes H
// bin by bin and leaves P + jQ = conj(g_h) H in LDS; phase 2 gives wave w the coefficients m = w, w + 4, ..: each lane sums
// its bins k = lane, lane + 64, .. in ascending order, the lanes combine in a fixed butterfly.  No atomics.
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int ML_MAX_ORDER = 64;
constexpr int ML_ROWS = 16;      // rows per wave of the forward
constexpr int ML_AHEAD = 4;      // coefficients whose basis entries are loaded together
constexpr int ML_BWD_THREADS = 256;

__host__ __device__ constexpr int ml_kp(int N) { return N / 2 + 64; }   // bins 0 .. N/2 padded to whole 64-lane columns
static inline bool ml_n_ok(int N) { return N >= 64 && N <= 2048 && (N & (N - 1)) == 0; }
static inline bool ml_m_ok(int M) { return M >= 0 && M <= ML_MAX_ORDER; }
static inline int ml_bwd_rows(int N) { return N <= 1024 ? 8 : 4; }
static inline size_t ml_bwd_lds(int rows, int N) {
    return ((size_t)(ML_MAX_ORDER + 1) * rows + 2 * (size_t)rows * ml_kp(N)) * sizeof(float);
}

__global__ void ml_basis_kernel(float* __restrict__ basis, int N, int M1, double alpha) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    const int K = N / 2 + 1, Kp = ml_kp(N);
    if (k >= Kp) return;
    float c = 0.f, s = 0.f;
    if (k < K) {
        const double x = 2.0 * (double)k / (double)N;   // w_k / pi
        const double th = M_PI * x + 2.0 * atan2(alpha * sinpi(x), 1.0 - alpha * cospi(x));
        const double a = (double)m * th;                // the product in float64: in fp32 it alone costs 1e-5 at m = 64
        c = (float)cos(a);
        s = (k == 0 || k == K - 1) ? 0.f : (float)sin(a);   // sin(m pi) is 1e-14 in float64, not 0
    }
    basis[(size_t)m * Kp + k] = c;
    basis[(size_t)(M1 + m) * Kp + k] = s;
}

// re[r] + j im[r] = L_k of rows r = 0 .. ROWS-1 from mcs[m * ROWS + r]; cb / sb point at the lane's basis column
template <int ROWS>
__device__ __forceinline__ void ml_log_response(float (&re)[ROWS], float (&im)[ROWS], const float* mcs,
                                                const float* __restrict__ cb, const float* __restrict__ sb, int Kp,
                                                int M1) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) re[r] = im[r] = 0.f;
    // basis entries of ML_AHEAD coefficients at a time, the next group's loads in flight under this group's FMAs (an L2 round
    // trip is several hundred cycles, one coefficient's FMAs a few dozen); the sum still runs over m = 0, 1, .. in order
    float c[ML_AHEAD], s[ML_AHEAD];
#pragma unroll
    for (int u = 0; u < ML_AHEAD; ++u) {
        const int mm = min(u, M1 - 1);
        c[u] = cb[(size_t)mm * Kp], s[u] = sb[(size_t)mm * Kp];
    }
    for (int m0 = 0; m0 < M1; m0 += ML_AHEAD) {
        float cn[ML_AHEAD], sn[ML_AHEAD];
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) {
            const int mm = min(m0 + ML_AHEAD + u, M1 - 1);   // clamped at the end: a redundant reload
            cn[u] = cb[(size_t)mm * Kp], sn[u] = sb[(size_t)mm * Kp];
        }
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) {
            if (m0 + u < M1) {
                const float cm = c[u], ns = -s[u];
                const float4* a4 = reinterpret_cast<const float4*>(mcs + (m0 + u) * ROWS);
#pragma unroll
                for (int q = 0; q < ROWS / 4; ++q) {
                    const float4 a = a4[q];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        re[4 * q + j] = fmaf(f4get(a, j), cm, re[4 * q + j]);
                        im[4 * q + j] = fmaf(f4get(a, j), ns, im[4 * q + j]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) c[u] = cn[u], s[u] = sn[u];
    }
}

// rows [r0, r0 + nrow) of mc (R, M1) -> mcs[m * ROWS + r], zeros for the rows past nrow
template <int ROWS>
__device__ __forceinline__ void ml_stage(float* mcs, const float* __restrict__ mc, int r0, int nrow, int M1, int tid,
                                         int nthr) {
    for (int idx = tid; idx < ROWS * M1; idx += nthr) {
        const int r = idx / M1, m = idx - r * M1;
        mcs[m * ROWS + r] = r < nrow ? mc[(size_t)r0 * M1 + idx] : 0.f;
    }
}

__global__ __launch_bounds__(64) void ml_rows_fwd_kernel(const float* __restrict__ mc, const float* __restrict__ basis,
                                                         float* __restrict__ h, int R, int N, int M1) {
    __shared__ __attribute__((aligned(16))) float mcs[(ML_MAX_ORDER + 1) * ML_ROWS];
    const int lane = threadIdx.x;
    const int K = N / 2 + 1, Kp = ml_kp(N);
    const int r0 = blockIdx.x * ML_ROWS, k = blockIdx.y * 64 + lane;   // k < Kp: the padding columns are zeros
    const int nrow = min(ML_ROWS, R - r0);
    ml_stage<ML_ROWS>(mcs, mc, r0, nrow, M1, lane, 64);
    __syncthreads();
    float re[ML_ROWS], im[ML_ROWS];
    ml_log_response<ML_ROWS>(re, im, mcs, basis + k, basis + (size_t)M1 * Kp + k, Kp, M1);
    if (k >= K) return;
    float2* out = reinterpret_cast<float2*>(h) + (size_t)r0 * K + k;
#pragma unroll
    for (int r = 0; r < ML_ROWS; ++r) {
        if (r < nrow) {
            const float e = expf(re[r]);
            float sn, cs;
            sincosf(im[r], &sn, &cs);
            out[(size_t)r * K] = make_float2(e * cs, e * sn);
        }
    }
}

template <int RB>
__global__ __launch_bounds__(ML_BWD_THREADS) void ml_rows_bwd_kernel(const float* __restrict__ g_h,
                                                                     const float* __restrict__ mc,
                                                                     const float* __restrict__ basis,
                                                                     float* __restrict__ g_mc, int R, int N, int M1) {
    extern __shared__ __attribute__((aligned(16))) float ml_lds[];
    float* mcs = ml_lds;                                                            // [m][RB]
    float2* pq = reinterpret_cast<float2*>(ml_lds + (ML_MAX_ORDER + 1) * RB);       // [RB][Kp], zero past K and past nrow
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int K = N / 2 + 1, Kp = ml_kp(N);
    const int r0 = blockIdx.x * RB;
    const int nrow = min(RB, R - r0);
    const float* cb = basis;
    const float* sb = basis + (size_t)M1 * Kp;
    ml_stage<RB>(mcs, mc, r0, nrow, M1, tid, ML_BWD_THREADS);
    __syncthreads();
    for (int k = tid; k < Kp; k += ML_BWD_THREADS) {
        float re[RB], im[RB];
        if (k < K) ml_log_response<RB>(re, im, mcs, cb + k, sb + k, Kp, M1);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float2 v = make_float2(0.f, 0.f);
            if (k < K && r < nrow) {
                const float2 g = reinterpret_cast<const float2*>(g_h)[(size_t)(r0 + r) * K + k];
                const float e = expf(re[r]);
                float sn, cs;
                sincosf(im[r], &sn, &cs);
                const float hr = e * cs, hi = e * sn;
                v = make_float2(g.x * hr + g.y * hi, g.x * hi - g.y * hr);   // conj(g_h) H
            }
            pq[r * Kp + k] = v;
        }
    }
    __syncthreads();
    for (int m = w; m < M1; m += ML_BWD_THREADS / 64) {
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.f;
        for (int k0 = lane; k0 < Kp; k0 += 64 * ML_AHEAD) {   // ML_AHEAD bins per lane with their loads issued together
            float c[ML_AHEAD], s[ML_AHEAD];
#pragma unroll
            for (int u = 0; u < ML_AHEAD; ++u) {
                const int k = min(k0 + 64 * u, Kp - 1);
                c[u] = cb[(size_t)m * Kp + k], s[u] = sb[(size_t)m * Kp + k];
            }
#pragma unroll
            for (int u = 0; u < ML_AHEAD; ++u) {
                const int k = k0 + 64 * u;
                if (k < Kp) {
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        const float2 v = pq[r * Kp + k];
                        acc[r] = fmaf(v.y, s[u], fmaf(v.x, c[u], acc[r]));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float a = acc[r];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
            if (lane == 0 && r < nrow) g_mc[(size_t)(r0 + r) * M1 + m] = a;
        }
    }
}

// the checks every entry shares; 0 or the code of fail()
static int ml_check(const char* who, int N, int M, size_t basis_bytes, double alpha = 0.0) {
    if (!ml_n_ok(N)) return fail(GOLF_EUNSUPPORTED, "%s: n_fft=%d is not a power of two in [64, 2048]", who, N);
    if (!ml_m_ok(M)) return fail(GOLF_EUNSUPPORTED, "%s: order=%d is outside [0, %d]", who, M, ML_MAX_ORDER);
    if (!(alpha > -1.0 && alpha < 1.0)) return fail(GOLF_EINVAL, "%s: |alpha| must be below 1 (got %g)", who, alpha);
    const size_t need = golf_mlsa_response_basis_bytes(N, M);
    if (basis_bytes < need) return fail(GOLF_EWORKSPACE, "%s: the basis needs %zu bytes, got %zu", who, need, basis_bytes);
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" {

size_t golf_mlsa_response_basis_bytes(int n_fft, int order) {
    if (!ml_n_ok(n_fft) || !ml_m_ok(order)) return 0;
    return 2 * (size_t)(order + 1) * ml_kp(n_fft) * sizeof(float);
}

int golf_mlsa_response_basis_f32(int n_fft, int order, double alpha, void* basis, size_t basis_bytes, void* stream) {
    if (!basis) return fail(GOLF_EINVAL, "mlsa_response_basis: null basis");
    if (const int rc = ml_check("mlsa_response_basis", n_fft, order, basis_bytes, alpha)) return rc;
    const int Kp = ml_kp(n_fft);
    hipLaunchKernelGGL(ml_basis_kernel, dim3((Kp + 255) / 256, order + 1), dim3(256), 0, (hipStream_t)stream, (float*)basis,
                       n_fft, order + 1, alpha);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_mlsa_response_rows_f32(const float* mc, const void* basis, size_t basis_bytes, float* h, int R, int n_fft, int order,
                                void* stream) {
    if (!mc || !basis || !h) return fail(GOLF_EINVAL, "mlsa_response_rows: null pointer (mc=%p basis=%p h=%p)", mc, basis, h);
    if (const int rc = ml_check("mlsa_response_rows", n_fft, order, basis_bytes)) return rc;
    if (R < 0) return fail(GOLF_EINVAL, "mlsa_response_rows: R=%d", R);
    if (R == 0) return GOLF_OK;
    const dim3 grid((R + ML_ROWS - 1) / ML_ROWS, (n_fft / 2 + 1 + 63) / 64);
    hipLaunchKernelGGL(ml_rows_fwd_kernel, grid, dim3(64), 0, (hipStream_t)stream, mc, (const float*)basis, h, R, n_fft,
                       order + 1);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_mlsa_response_rows_bwd_f32(const float* g_h, const float* mc, const void* basis, size_t basis_bytes, float* g_mc, int R,
                                    int n_fft, int order, void* stream) {
    if (!g_h || !mc || !basis || !g_mc)
        return fail(GOLF_EINVAL, "mlsa_response_rows_bwd: null pointer (g_h=%p mc=%p basis=%p g_mc=%p)", g_h, mc, basis, g_mc);
    if (const int rc = ml_check("mlsa_response_rows_bwd", n_fft, order, basis_bytes)) return rc;
    if (R < 0) return fail(GOLF_EINVAL, "mlsa_response_rows_bwd: R=%d", R);
    if (R == 0) return GOLF_OK;
    const int rows = ml_bwd_rows(n_fft);
    const size_t lds = ml_bwd_lds(rows, n_fft);   // at most 38 944 bytes (N 1024, 8 rows): inside the default 64 KiB
    const dim3 grid((R + rows - 1) / rows);
    if (rows == 8)
        hipLaunchKernelGGL(ml_rows_bwd_kernel<8>, grid, dim3(ML_BWD_THREADS), lds, (hipStream_t)stream, g_h, mc,
                           (const float*)basis, g_mc, R, n_fft, order + 1);
    else
        hipLaunchKernelGGL(ml_rows_bwd_kernel<4>, grid, dim3(ML_BWD_THREADS), lds, (hipStream_t)stream, g_h, mc,
                           (const float*)basis, g_mc, R, n_fft, order + 1);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
