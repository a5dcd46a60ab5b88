// Minimum-phase FIR design for gfx950: log magnitudes -> windowed minimum-phase impulse responses, and its adjoint.
//
// Reference: LTVMinimumPhaseFIRFilterPrecise.get_minimum_phase_fir + windowing, models/filters.py:203-221, with
// hilbert() from models/utils.py:557-574:
//   L_sym = even extension of log_mag to N = 2*(n_mag-1) bins,  theta = -Im hilbert(L_sym),
//   h = Re ifft(exp(L_sym + j*theta)) * window
// The FFTs of a real, even sequence are dense real contractions with constant matrices (w_k = 1 for k in {0, N/2}, else 2):
//   theta[k] = sum_j L[j] * S[k][j]                                        k, j = 0..N/2
//       S[k][j] = -(w_j/N) * sum_{0<n<N/2} 2 cos(2 pi j n / N) sin(2 pi k n / N)
//               = -(w_j/N) * (cot((k+j) pi / N) + cot((k-j) pi / N))  for k+j odd, 0 for k+j even and for k in {0, N/2}
//       (sum_{0<n<H} sin(m pi n / H) = cot(m pi / (2H)) for odd m and 0 for even m)
//   h[m] = sum_k (e^L[k] cos theta[k]) * C[k][m] - (e^L[k] sin theta[k]) * Sn[k][m]          m = 0..N-1
//       C[k][m] = (w_k/N) cos(2 pi k m / N),  Sn[k][m] = (w_k/N) sin(2 pi k m / N)
// One workgroup owns 16 or 32 rows (frames) from the log magnitudes to the finished kernel rows: GEMM 1 (theta) runs from
// the rows' log magnitudes in LDS, exp / sincos turn its accumulators into GEMM 2's A operand (again LDS, never global
// memory), GEMM 2 runs over all N columns, the window multiplies in its epilogue.  Both GEMMs are exact-fp32
// v_mfma_f32_16x16x4_f32 (noise_fir.hip gives the reason: bf16 would cost 1e-3), with the B fragments (the constants, L2
// resident) prefetched 8 k-steps ahead in registers.
// The backward recomputes theta and needs the same constants transposed:
//   [g_ec | g_es] = (g_h * window) @ [C^T | -Sn^T];   g_theta = -g_ec * es + g_es * ec;
//   g_L = g_ec * ec + g_es * es + g_theta @ S                                    (ec = e^L cos theta, es = e^L sin theta)
#include "common.h"
#include "device_common.h"

namespace golf {

typedef float mp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int MP_COLS = 128;           // columns per pass of the workgroup: 4 waves x (2 tiles of 16)
constexpr int MP_THREADS = 256;
constexpr int MP_LDS_LIMIT = 160 * 1024;

static inline int mp_pad(int n) { return (int)align_up((size_t)n, MP_COLS); }

// ------------------------------------------------------------------------------------------------------------
// Constants, fp64 evaluation with exact integer argument reduction, rounded once to fp32.  Layout of `basis` (floats),
// Pd = n_mag rounded up to 128, PN = N rounded up to 128, zero in all padding:
//   B1  [j * Pd + k]        = S[k][j]            (Pd x Pd)     theta = L @ B1
//   B1T [k * Pd + j]        = S[k][j]            (Pd x Pd)     g_L += g_theta @ B1T
//   B2  [k * PN + m]        = C[k][m],  B2[(Pd + k) * PN + m] = -Sn[k][m]        (2Pd x PN)   h = [ec | es] @ B2
//   B2T [m * 2Pd + k]       = C[k][m],  B2T[m * 2Pd + Pd + k] = -Sn[k][m]        (PN x 2Pd)   [g_ec | g_es] = g_h @ B2T
// ------------------------------------------------------------------------------------------------------------
__global__ void mp_basis_s_kernel(float* __restrict__ B1, float* __restrict__ B1T, int n_mag, int Pd) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= Pd) return;
    const int N = 2 * (n_mag - 1), H = N >> 1;
    float v = 0.f;
    if (k > 0 && k < H && j < n_mag && ((k + j) & 1)) {
        const double wj = (j == 0 || j == H) ? 1.0 : 2.0;
        const double xp = (double)(k + j) / (double)N, xm = (double)(k - j) / (double)N;   // in (0,1) and (-1/2,1/2), never 0
        v = (float)(-(wj / (double)N) * (cospi(xp) / sinpi(xp) + cospi(xm) / sinpi(xm)));
    }
    B1[(size_t)j * Pd + k] = v;
    B1T[(size_t)k * Pd + j] = v;
}

__global__ void mp_basis_c_kernel(float* __restrict__ B2, float* __restrict__ B2T, int n_mag, int Pd, int PN) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (m >= PN) return;
    const int N = 2 * (n_mag - 1), H = N >> 1;
    float c = 0.f, s = 0.f;
    if (k < n_mag && m < N) {
        const long long r = ((long long)k * m) % N;
        const double wk = (k == 0 || k == H) ? 1.0 : 2.0;
        const double x = 2.0 * (double)r / (double)N;
        c = (float)(wk * cospi(x) / (double)N);
        s = (float)(-wk * sinpi(x) / (double)N);
    }
    B2[(size_t)k * PN + m] = c;
    B2[(size_t)(Pd + k) * PN + m] = s;
    B2T[(size_t)m * 2 * Pd + k] = c;
    B2T[(size_t)m * 2 * Pd + Pd + k] = s;
}

// ------------------------------------------------------------------------------------------------------------
// acc[rt][ct] += As[16*rt .. 16*rt+15][0..K) @ Bm[0..K)[col .. col+31]   (col = first of the wave's 32 columns)
// As: LDS, row stride lda = 2 mod 32 floats (the (row, k) pattern of the A operand hits 32 distinct banks);
// Bm: global, row stride ldb, zero padded; K a multiple of 64.  Operand layout of v_mfma_f32_16x16x4_f32: lane (li, lk) =
// (lane & 15, lane >> 4) supplies A[row li][k lk] and B[k lk][col li] and holds C[rows 4*lk .. 4*lk+3][col li].
// ------------------------------------------------------------------------------------------------------------
template <int RT>
__device__ __forceinline__ void mp_gemm(mp_f32x4 (&acc)[RT][2], const float* As, int lda, const float* __restrict__ Bm,
                                        int ldb, int col, int K, int lane) {
    const int li = lane & 15, lk = lane >> 4;
    const float* bp = Bm + (size_t)lk * ldb + col + li;
    const float* ap = As + li * lda + lk;
    const int ksteps = K >> 2;
    float bq[2][8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        bq[0][i][0] = bp[(size_t)(4 * i) * ldb];
        bq[0][i][1] = bp[(size_t)(4 * i) * ldb + 16];
    }
    for (int s0 = 0; s0 < ksteps; s0 += 16) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            const int sg = s0 + 8 * ph;                 // first k-step of this phase
            const int sn = min(sg + 8, ksteps - 8);     // clamped at the very end: a redundant reload
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bq[ph ^ 1][i][0] = bp[(size_t)(4 * (sn + i)) * ldb];
                bq[ph ^ 1][i][1] = bp[(size_t)(4 * (sn + i)) * ldb + 16];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the 16 prefetch loads ahead of this phase's MFMAs
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = ap[rt * 16 * lda + 4 * (sg + i)];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    acc[rt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bq[ph][i][0], acc[rt][0], 0, 0, 0);
                    acc[rt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bq[ph][i][1], acc[rt][1], 0, 0, 0);
                }
            }
        }
    }
}

template <int RT>
__device__ __forceinline__ void mp_zero(mp_f32x4 (&acc)[RT][2]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = (mp_f32x4){0.f, 0.f, 0.f, 0.f};
}

// rows [g0, g0 + ROWS) x [0, ncol) of a (G, src_stride) matrix -> LDS (row stride ld), times scale[col] if given;
// zeros past G, past nvalid columns
__device__ __forceinline__ void mp_stage(float* dst, int ld, const float* __restrict__ src, int src_stride,
                                         const float* __restrict__ scale, int g0, int G, int rows, int nvalid, int ncol,
                                         int tid) {
    for (int idx = tid; idx < rows * ncol; idx += MP_THREADS) {
        const int r = idx / ncol, k = idx - r * ncol;
        const bool in = g0 + r < G && k < nvalid;
        float v = 0.f;
        if (in) {
            v = src[(size_t)(g0 + r) * src_stride + k];
            if (scale) v *= scale[k];
        }
        dst[r * ld + k] = v;
    }
}

// LDS floats of the two kernels (host and device agree through these)
__host__ __device__ constexpr int mp_ldl(int Pd) { return Pd + 2; }
__host__ __device__ constexpr int mp_lde(int Pd) { return 2 * Pd + 2; }
__host__ __device__ constexpr int mp_ldw(int PN) { return PN + 2; }
static inline size_t mp_fwd_lds(int rows, int Pd) { return (size_t)rows * (mp_ldl(Pd) + mp_lde(Pd)) * sizeof(float); }
static inline size_t mp_bwd_lds(int rows, int Pd, int PN) {
    return (size_t)rows * (mp_ldw(PN) + mp_lde(Pd)) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------------------
// forward: block = 4 waves, 16*RT rows; every pass of 128 columns gives wave w 32 of them (RT x 2 tiles)
// ------------------------------------------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(MP_THREADS) void mp_design_fwd_kernel(const float* __restrict__ log_mag,
                                                                   const float* __restrict__ window,
                                                                   const float* __restrict__ basis,
                                                                   float* __restrict__ kern, int KS, int G, int n_mag,
                                                                   int Pd, int PN) {
    extern __shared__ __attribute__((aligned(16))) float mp_lds[];
    constexpr int ROWS = 16 * RT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int g0 = blockIdx.x * ROWS;
    const int N = 2 * (n_mag - 1);
    const int LDL = mp_ldl(Pd), LDE = mp_lde(Pd);
    float* Ls = mp_lds;                 // log magnitudes (ROWS x Pd); in GEMM 2 the waves' output tiles
    float* Es = mp_lds + ROWS * LDL;    // [e^L cos theta | e^L sin theta] (ROWS x 2Pd)
    const float* B1 = basis;
    const float* B2 = basis + 2 * (size_t)Pd * Pd;

    mp_stage(Ls, LDL, log_mag, n_mag, nullptr, g0, G, ROWS, n_mag, Pd, tid);
    __syncthreads();
    mp_f32x4 acc[RT][2];
    for (int c0 = 0; c0 < Pd; c0 += MP_COLS) {
        mp_zero<RT>(acc);
        mp_gemm<RT>(acc, Ls, LDL, B1, Pd, c0 + w * 32, Pd, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + lk * 4 + r, k = c0 + w * 32 + ct * 16 + li;
                    const float e = expf(Ls[row * LDL + k]);
                    const float th = acc[rt][ct][r];
                    Es[row * LDE + k] = e * cosf(th);
                    Es[row * LDE + Pd + k] = e * sinf(th);
                }
    }
    __syncthreads();   // Es complete; Ls is free from here on
    float* Cw = Ls + w * 32;   // the wave's own 32 columns of a ROWS x 128 tile (row stride LDL >= 130)
    const int cl = lane & 31, rh = lane >> 5;
    for (int c0 = 0; c0 < PN; c0 += MP_COLS) {
        const int m = c0 + w * 32 + cl;
        const float wm = window[min(m, N - 1)];
        mp_zero<RT>(acc);
        mp_gemm<RT>(acc, Es, LDE, B2, PN, c0 + w * 32, 2 * Pd, lane);
        wave_lds_fence();   // the previous pass's reads of Cw
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) Cw[(rt * 16 + lk * 4 + r) * LDL + ct * 16 + li] = acc[rt][ct][r];
        wave_lds_fence();
        // 2 rows x 32 columns per store; taps [N, KS) are the row's zero padding
#pragma unroll 4
        for (int it = 0; it < ROWS / 2; ++it) {
            const int row = 2 * it + rh, g = g0 + row;
            const float v = Cw[row * LDL + cl] * wm;
            if (g < G && m < KS) kern[(size_t)g * KS + m] = m < N ? v : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// backward: g_kern (G, KS) -> g_log_mag (G, n_mag)
// ------------------------------------------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(MP_THREADS) void mp_design_bwd_kernel(const float* __restrict__ g_kern,
                                                                   const float* __restrict__ log_mag,
                                                                   const float* __restrict__ window,
                                                                   const float* __restrict__ basis,
                                                                   float* __restrict__ g_log_mag, int KS, int G,
                                                                   int n_mag, int Pd, int PN) {
    extern __shared__ __attribute__((aligned(16))) float mp_lds[];
    constexpr int ROWS = 16 * RT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int g0 = blockIdx.x * ROWS;
    const int N = 2 * (n_mag - 1);
    const int LDL = mp_ldl(Pd), LDE = mp_lde(Pd), LDW = mp_ldw(PN);
    float* Gw = mp_lds;                 // g_kern * window (ROWS x PN); afterwards the log magnitudes (ROWS x Pd)
    float* Ge = mp_lds + ROWS * LDW;    // [g_ec | g_es] (ROWS x 2Pd); afterwards [g_theta | g_L without the theta path]
    float* Ls = Gw;
    const float* B1 = basis;
    const float* B1T = basis + (size_t)Pd * Pd;
    const float* B2T = basis + 2 * (size_t)Pd * Pd + 2 * (size_t)Pd * PN;

    mp_stage(Gw, LDW, g_kern, KS, window, g0, G, ROWS, N, PN, tid);
    __syncthreads();
    mp_f32x4 acc[RT][2];
    for (int c0 = 0; c0 < 2 * Pd; c0 += MP_COLS) {
        mp_zero<RT>(acc);
        mp_gemm<RT>(acc, Gw, LDW, B2T, 2 * Pd, c0 + w * 32, PN, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Ge[(rt * 16 + lk * 4 + r) * LDE + c0 + w * 32 + ct * 16 + li] = acc[rt][ct][r];
    }
    __syncthreads();   // every wave is done reading Gw
    mp_stage(Ls, LDL, log_mag, n_mag, nullptr, g0, G, ROWS, n_mag, Pd, tid);
    __syncthreads();
    for (int c0 = 0; c0 < Pd; c0 += MP_COLS) {   // theta again; each (row, k) of Ge belongs to one lane
        mp_zero<RT>(acc);
        mp_gemm<RT>(acc, Ls, LDL, B1, Pd, c0 + w * 32, Pd, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + lk * 4 + r, k = c0 + w * 32 + ct * 16 + li;
                    const float e = expf(Ls[row * LDL + k]);
                    const float th = acc[rt][ct][r];
                    const float ec = e * cosf(th), es = e * sinf(th);
                    const float gec = Ge[row * LDE + k], ges = Ge[row * LDE + Pd + k];
                    Ge[row * LDE + k] = ges * ec - gec * es;
                    Ge[row * LDE + Pd + k] = gec * ec + ges * es;
                }
    }
    __syncthreads();
    const int cl = lane & 31, rh = lane >> 5;
    for (int c0 = 0; c0 < Pd; c0 += MP_COLS) {
        mp_zero<RT>(acc);
        mp_gemm<RT>(acc, Ge, LDE, B1T, Pd, c0 + w * 32, Pd, lane);
        float* Cw = Ge + Pd + c0 + w * 32;   // the wave's own 32 columns of the second half: nobody else touches them
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) Cw[(rt * 16 + lk * 4 + r) * LDE + ct * 16 + li] += acc[rt][ct][r];
        wave_lds_fence();
        const int j = c0 + w * 32 + cl;
#pragma unroll 4
        for (int it = 0; it < ROWS / 2; ++it) {
            const int row = 2 * it + rh, g = g0 + row;
            const float v = Cw[row * LDE + cl];
            if (g < G && j < n_mag) g_log_mag[(size_t)g * n_mag + j] = v;
        }
    }
}

// rows per workgroup: 32 if the LDS holds them, else 16, else 0 (n_mag too large)
static int mp_rows(size_t lds16) { return 2 * lds16 <= (size_t)MP_LDS_LIMIT ? 32 : (lds16 <= (size_t)MP_LDS_LIMIT ? 16 : 0); }

template <typename K>
static int mp_raise_lds(K kernel, const char* who) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MP_LDS_LIMIT);
    if (e != hipSuccess)   /* > 64 KB of dynamic LDS per workgroup needs the opt-in */
        return fail((int)e, "%s: cannot raise the dynamic LDS limit: %s", who, hipGetErrorString(e));
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" {

size_t golf_min_phase_fir_basis_bytes(int n_mag) {
    if (n_mag < 2) return 0;
    const size_t Pd = mp_pad(n_mag), PN = mp_pad(2 * (n_mag - 1));
    return (2 * Pd * Pd + 4 * Pd * PN) * sizeof(float);
}

int golf_min_phase_fir_basis_f32(int n_mag, void* basis, size_t basis_bytes, void* stream) {
    if (n_mag < 2 || !basis) return fail(GOLF_EINVAL, "min_phase_fir_basis: n_mag=%d basis=%p", n_mag, basis);
    if (basis_bytes < golf_min_phase_fir_basis_bytes(n_mag))
        return fail(GOLF_EWORKSPACE, "min_phase_fir_basis: need %zu bytes, got %zu", golf_min_phase_fir_basis_bytes(n_mag),
                    basis_bytes);
    const int Pd = mp_pad(n_mag), PN = mp_pad(2 * (n_mag - 1));
    float* B1 = (float*)basis;
    float* B2 = B1 + 2 * (size_t)Pd * Pd;
    hipLaunchKernelGGL(mp_basis_s_kernel, dim3((Pd + 255) / 256, Pd), dim3(256), 0, (hipStream_t)stream, B1,
                       B1 + (size_t)Pd * Pd, n_mag, Pd);
    GOLF_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp_basis_c_kernel, dim3((PN + 255) / 256, Pd), dim3(256), 0, (hipStream_t)stream, B2,
                       B2 + 2 * (size_t)Pd * PN, n_mag, Pd, PN);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_min_phase_fir_kernels_f32(const float* log_mag, const float* window, const void* basis, float* kern, int G,
                                   int n_mag, void* stream) {
    if (!log_mag || !window || !basis || !kern || G < 1 || n_mag < 2)
        return fail(GOLF_EINVAL, "min_phase_fir_kernels: bad argument (G=%d n_mag=%d)", G, n_mag);
    const int Pd = mp_pad(n_mag), PN = mp_pad(2 * (n_mag - 1)), KS = golf_zero_phase_fir_row_stride(n_mag);
    const int rows = mp_rows(mp_fwd_lds(16, Pd));
    if (!rows)
        return fail(GOLF_EUNSUPPORTED, "min_phase_fir_kernels: n_mag=%d needs %zu bytes of LDS per workgroup (limit %d)",
                    n_mag, mp_fwd_lds(16, Pd), MP_LDS_LIMIT);
    const size_t lds = mp_fwd_lds(rows, Pd);
    const dim3 grid((G + rows - 1) / rows);
    if (rows == 32) {
        static const int attr = mp_raise_lds(mp_design_fwd_kernel<2>, "min_phase_fir_kernels");
        if (attr) return attr;
        hipLaunchKernelGGL(mp_design_fwd_kernel<2>, grid, dim3(MP_THREADS), lds, (hipStream_t)stream, log_mag, window,
                           (const float*)basis, kern, KS, G, n_mag, Pd, PN);
    } else {
        static const int attr = mp_raise_lds(mp_design_fwd_kernel<1>, "min_phase_fir_kernels");
        if (attr) return attr;
        hipLaunchKernelGGL(mp_design_fwd_kernel<1>, grid, dim3(MP_THREADS), lds, (hipStream_t)stream, log_mag, window,
                           (const float*)basis, kern, KS, G, n_mag, Pd, PN);
    }
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_min_phase_fir_kernels_bwd_f32(const float* g_kern, const float* log_mag, const float* window, const void* basis,
                                       float* g_log_mag, int G, int n_mag, void* stream) {
    if (!g_kern || !log_mag || !window || !basis || !g_log_mag || G < 1 || n_mag < 2)
        return fail(GOLF_EINVAL, "min_phase_fir_kernels_bwd: bad argument (G=%d n_mag=%d)", G, n_mag);
    const int Pd = mp_pad(n_mag), PN = mp_pad(2 * (n_mag - 1)), KS = golf_zero_phase_fir_row_stride(n_mag);
    const int rows = mp_rows(mp_bwd_lds(16, Pd, PN));
    if (!rows)
        return fail(GOLF_EUNSUPPORTED, "min_phase_fir_kernels_bwd: n_mag=%d needs %zu bytes of LDS per workgroup (limit %d)",
                    n_mag, mp_bwd_lds(16, Pd, PN), MP_LDS_LIMIT);
    const size_t lds = mp_bwd_lds(rows, Pd, PN);
    const dim3 grid((G + rows - 1) / rows);
    if (rows == 32) {
        static const int attr = mp_raise_lds(mp_design_bwd_kernel<2>, "min_phase_fir_kernels_bwd");
        if (attr) return attr;
        hipLaunchKernelGGL(mp_design_bwd_kernel<2>, grid, dim3(MP_THREADS), lds, (hipStream_t)stream, g_kern, log_mag,
                           window, (const float*)basis, g_log_mag, KS, G, n_mag, Pd, PN);
    } else {
        static const int attr = mp_raise_lds(mp_design_bwd_kernel<1>, "min_phase_fir_kernels_bwd");
        if (attr) return attr;
        hipLaunchKernelGGL(mp_design_bwd_kernel<1>, grid, dim3(MP_THREADS), lds, (hipStream_t)stream, g_kern, log_mag,
                           window, (const float*)basis, g_log_mag, KS, G, n_mag, Pd, PN);
    }
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
