// Initial state of the sample-wise LTV all-pole filter on EVERY plan (include/golf_amd.h, "head" entries).  fp32, gfx950 only.
//
// A filter that starts from y[-1-j] = zi[j] is exactly the zero-state filter of an excitation whose first H = min(M, T)
// samples carry a correction:
//     c[t]  = sum_{i=t}^{M-1} A[t,i] zi[i-t]   (t < H; the taps of sample t that still reach in front of t = 0)
//     xh[t] = ex[t] G[t] - c[t]                 (G = up(gain), A = up(a); the core then runs with gain == 1)
// so the chunked scans, the merged pass, the serial and the wave-per-utterance kernels serve zi unchanged, and so do their
// backwards: with q the gradient the core returns for xh (gain == 1: the adjoint recursion itself),
//     g_ex[t] = q[t] G[t]     g_gain = up^T(q ex)     g_a += up^T(-q[t] zi[i-t])  (t < H, i >= t)
//     g_zi[j] = -sum_{t < H, t+j < M} q[t] A[t,t+j]
// The gain is never divided out of the head (it may hold an exact 0), hence the rewritten excitation.
//
// The two elementwise kernels are memory bound: a lane owns 4 consecutive samples, takes them with one 16-byte load and
// store where the row's address allows it (rows may be strided views with any start offset: scalar path otherwise) and does
// ONE integer division, for the frame of its first sample.  The reductions run in a fixed order and use no atomics: the
// gradients are bit-reproducible.
#include "common.h"
#include "device_common.h"

#include <climits>

namespace golf {

namespace {

constexpr int kLaneSamples = 4;
constexpr int kBlock = 256;
constexpr int kBlockSamples = kBlock * kLaneSamples;

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The frame of sample t and the position in it, advanced one sample at a time: f = min(t / hop, F-2), n = t - f*hop
// (F == 1: f = 0 and the interpolation degenerates to z[0]).
struct FramePos {
    int f, n;
    __device__ __forceinline__ FramePos(int t, int F, int hop) : f(0), n(t) {
        if (F >= 2) {
            f = t / hop;
            if (f > F - 2) f = F - 2;
            n = t - f * hop;
        }
    }
    // true when the sample that `n` now points at lies in the next frame
    __device__ __forceinline__ bool crossed(int F, int hop) {
        if (n >= hop && f < F - 2) {
            ++f;
            n -= hop;
            return true;
        }
        return false;
    }
};

// 4 consecutive floats of a row, zeros from `end` on
__device__ __forceinline__ void load4(float (&v)[4], const float* __restrict__ row, int t0, int end) {
    if (t0 + kLaneSamples <= end && aligned16(row + t0)) {
        const float4 q = *reinterpret_cast<const float4*>(row + t0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kLaneSamples; ++j) v[j] = t0 + j < end ? row[t0 + j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ row, int t0, int end, const float (&v)[4]) {
    if (t0 + kLaneSamples <= end && aligned16(row + t0)) {
        *reinterpret_cast<float4*>(row + t0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kLaneSamples; ++j)
            if (t0 + j < end) row[t0 + j] = v[j];
    }
}

// up(gain) at the lane's 4 samples, with the frame and the interpolation weight of each; one division (in FramePos)
__device__ __forceinline__ void gain4(float (&G)[4], int (&fr)[4], float (&w)[4], const float* __restrict__ gb, int t0, int F,
                                      int hop, float inv_hop) {
    FramePos p(t0, F, hop);
    float g0 = gb[p.f], g1 = gb[F >= 2 ? p.f + 1 : p.f];
#pragma unroll
    for (int j = 0; j < kLaneSamples; ++j) {
        if (p.crossed(F, hop)) {
            g0 = g1;
            g1 = gb[p.f + 1];
        }
        fr[j] = p.f;
        w[j] = (float)p.n * inv_hop;
        G[j] = fmaf(w[j], g1 - g0, g0);
        ++p.n;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Forward: xh[t] = ex[t] G[t] - c[t], t in [0, T).  nblk blocks per row; the first of a row also forms c[0 .. H): the lanes
// that own those samples publish their frame and interpolation weight, lane t < H then sums its taps i = t .. M-1 in order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lpc_head_fwd_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                              const float* __restrict__ gain, const float* __restrict__ a,
                                                              const float* __restrict__ zi, float* __restrict__ xh,
                                                              int64_t xh_stride, int T, int F, int M, int hop, int nblk) {
    __shared__ float zs[64], cs[64], wfr[64];
    __shared__ int ffr[64];
    const int b = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x % (unsigned)nblk);
    const int tid = threadIdx.x;
    const int t0 = (blk * kBlock + tid) * kLaneSamples;
    const float* xb = ex + (size_t)b * ex_stride;
    float* ob = xh + (size_t)b * xh_stride;
    const float* gb = gain + (size_t)b * F;
    const float inv_hop = 1.0f / (float)hop;
    const int H = M < T ? M : T;

    float x[4] = {0.f, 0.f, 0.f, 0.f}, G[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
    int fr[4] = {0, 0, 0, 0};
    if (t0 < T) {
        load4(x, xb, t0, T);
        gain4(G, fr, w, gb, t0, F, hop, inv_hop);
    }
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (blk == 0) {   // (block-uniform)
        if (tid < M) zs[tid] = zi[(size_t)b * M + tid];
        if (t0 < H) {   // the lanes 0 .. ceil(H/4)-1 (H <= 64: t0 + j <= 63)
#pragma unroll
            for (int j = 0; j < kLaneSamples; ++j) {
                ffr[t0 + j] = fr[j];
                wfr[t0 + j] = w[j];
            }
        }
        __syncthreads();
        if (tid < H) {
            const int f = ffr[tid];
            const float wt = wfr[tid];
            const float* a0 = a + ((size_t)b * F + f) * M;
            const float* a1 = a + ((size_t)b * F + (F >= 2 ? f + 1 : f)) * M;
            float acc = 0.f;
            for (int i = tid; i < M; ++i) {
                const float lo = a0[i];
                acc = fmaf(fmaf(wt, a1[i] - lo, lo), zs[i - tid], acc);
            }
            cs[tid] = acc;
        }
        __syncthreads();
        if (t0 < H) {
#pragma unroll
            for (int j = 0; j < kLaneSamples; ++j)
                if (t0 + j < H) c[j] = cs[t0 + j];
        }
    }
    if (t0 < T) {
        float o[4];
#pragma unroll
        for (int j = 0; j < kLaneSamples; ++j) o[j] = x[j] * G[j] - c[j];
        store4(ob, t0, T, o);
    }
}

// ------------------------------------------------------------------------------------------
// Backward, launch 1: g_ex[t] = q[t] G[t] for t < T and 0 for T <= t < Tx -- the whole row is written.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lpc_head_gex_kernel(const float* __restrict__ q, int64_t q_stride,
                                                              const float* __restrict__ gain, float* __restrict__ g_ex,
                                                              int64_t g_ex_stride, int Tx, int T, int F, int hop, int nblk) {
    const int b = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x % (unsigned)nblk);
    const int t0 = (blk * kBlock + (int)threadIdx.x) * kLaneSamples;
    if (t0 >= Tx) return;
    float* ob = g_ex + (size_t)b * g_ex_stride;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (t0 < T) {
        float v[4], G[4], w[4];
        int fr[4];
        load4(v, q + (size_t)b * q_stride, t0, T);
        gain4(G, fr, w, gain + (size_t)b * F, t0, F, hop, 1.0f / (float)hop);
#pragma unroll
        for (int j = 0; j < kLaneSamples; ++j) o[j] = t0 + j < T ? v[j] * G[j] : 0.f;
    }
    store4(ob, t0, Tx, o);
}

// ------------------------------------------------------------------------------------------
// Backward, launch 2: single-wave workgroups.
//   blocks [0, n_gain): one per (b, f), GATHER form of up^T: g_gain[b,f] = sum_t w_f(t) q[t] ex[t] over the samples with a
//     weight for frame f -- those of frame f-1 (rising edge) and of frame f (falling edge), fewer than 2 hop, clipped to
//     [0, T) -- lane k taking lo+k, lo+k+64, ... in order, then a fixed shuffle tree.
//   blocks [n_gain, n_gain + B): one per utterance, lane l as tap i = l of g_a_head and as state index j = l of g_zi, the
//     head's samples t = 0 .. H-1 in order.  g_a_head (B, F, M): the head's frames hold up^T(-q[t] zi[i-t]), every other
//     frame is zeroed.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lpc_head_reduce_kernel(const float* __restrict__ q, int64_t q_stride,
                                                             const float* __restrict__ ex, int64_t ex_stride,
                                                             const float* __restrict__ a, const float* __restrict__ zi,
                                                             float* __restrict__ g_gain, float* __restrict__ g_a_head,
                                                             float* __restrict__ g_zi, int n_gain, int T, int F, int M,
                                                             int hop) {
    __shared__ float zs[64];
    const int k = threadIdx.x;
    const float hopf = (float)hop;
    if ((int)blockIdx.x < n_gain) {
        const int f = (int)(blockIdx.x % (unsigned)F), b = (int)(blockIdx.x / (unsigned)F);
        const float* qb = q + (size_t)b * q_stride;
        const float* xb = ex + (size_t)b * ex_stride;
        const HatSpan span(f, F, hop, T);
        float acc = 0.f;
        for (int t = span.lo + k; t < span.hi; t += 64) acc = fmaf(span.weight<float>(t) * qb[t], xb[t], acc);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_down(acc, o);
        if (k == 0) g_gain[(size_t)b * F + f] = acc;
        return;
    }
    const int b = (int)blockIdx.x - n_gain;
    const int H = M < T ? M : T;
    const float* ab = a + (size_t)b * F * M;
    zs[k] = k < M ? zi[(size_t)b * M + k] : 0.f;
    const float qv = k < H ? q[(size_t)b * q_stride + k] : 0.f;
    __syncthreads();
    float* gah = g_a_head ? g_a_head + (size_t)b * F * M : nullptr;
    const float inv_hop = 1.0f / hopf;
    int f = 0, n = 0;          // wave-uniform frame and position of t
    float acc0 = 0.f, acc1 = 0.f, gz = 0.f;   // g_a_head of frames f and f+1, tap k;  g_zi[k]
    for (int t = 0; t < H; ++t) {
        if (n >= hop && f < F - 2) {   // t enters the next frame: frame f is complete
            if (gah && k < M) gah[(size_t)f * M + k] = acc0;
            acc0 = acc1;
            acc1 = 0.f;
            ++f;
            n -= hop;
        }
        const float w = F >= 2 ? (float)n * inv_hop : 0.f;
        const float qt = lane_bcast(qv, t);
        if (k >= t && k < M) {   // tap i = k of sample t reads y[t-1-k] = zi[k-t]
            const float p = -qt * zs[k - t];
            acc0 = fmaf(1.f - w, p, acc0);
            acc1 = fmaf(w, p, acc1);
        }
        if (t + k < M) {         // state j = k is read by tap t+k of sample t
            const float lo = ab[(size_t)f * M + t + k];
            const float hi = ab[(size_t)(F >= 2 ? f + 1 : f) * M + t + k];
            gz = fmaf(-qt, fmaf(w, hi - lo, lo), gz);
        }
        ++n;
    }
    if (gah) {
        int fz = f + 1;   // first frame without a head sample
        if (k < M) {
            gah[(size_t)f * M + k] = acc0;
            if (f + 1 < F) gah[(size_t)(f + 1) * M + k] = acc1;
        }
        if (f + 1 < F) ++fz;
        for (int64_t u = (int64_t)fz * M + k; u < (int64_t)F * M; u += 64) gah[u] = 0.f;
    }
    if (g_zi && k < M) g_zi[(size_t)b * M + k] = gz;
}

static int check_shape(const char* who, int B, int T, int F, int M, int hop) {
    if (B < 1 || T < 1 || F < 1 || M < 1 || hop < 1)
        return fail(GOLF_EINVAL, "%s: B=%d T=%d F=%d M=%d hop=%d must all be >= 1", who, B, T, F, M, hop);
    if (M > 64) return fail(GOLF_EUNSUPPORTED, "%s: M=%d beyond 64", who, M);
    if ((int64_t)T > (int64_t)(F - 1) * hop + 1)
        return fail(GOLF_EINVAL, "%s: T=%d exceeds (F-1)*hop+1=%lld", who, T, (long long)(F - 1) * hop + 1);
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" int golf_ltv_allpole_head_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a,
                                             const float* zi, float* xh, int64_t xh_stride, int B, int T, int F, int M,
                                             int hop, void* stream) {
    const char* who = "ltv_allpole_head_fwd";
    if (int rc = check_shape(who, B, T, F, M, hop)) return rc;
    if (!ex || !gain || !a || !zi || !xh) return fail(GOLF_EINVAL, "%s: null pointer", who);
    if ((B > 1 && (ex_stride < T || xh_stride < T)))
        return fail(GOLF_EINVAL, "%s: row strides %lld / %lld below T=%d", who, (long long)ex_stride, (long long)xh_stride, T);
    const int64_t nblk = ceil_div(T, kBlockSamples);
    if (T > INT_MAX - kBlockSamples || nblk * B > INT_MAX)
        return fail(GOLF_EUNSUPPORTED, "%s: B=%d x T=%d beyond the launch grid", who, B, T);
    hipLaunchKernelGGL(lpc_head_fwd_kernel, dim3((unsigned)(nblk * B)), dim3(kBlock), 0, (hipStream_t)stream, ex, ex_stride,
                       gain, a, zi, xh, xh_stride, T, F, M, hop, (int)nblk);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

extern "C" int golf_ltv_allpole_head_bwd_f32(const float* q, int64_t q_stride, const float* ex, int64_t ex_stride,
                                             const float* gain, const float* a, const float* zi, float* g_ex,
                                             int64_t g_ex_stride, int Tx, float* g_gain, float* g_a_head, float* g_zi,
                                             int B, int T, int F, int M, int hop, void* stream) {
    const char* who = "ltv_allpole_head_bwd";
    if (int rc = check_shape(who, B, T, F, M, hop)) return rc;
    // (the head blocks stage zi for g_a_head and read a for g_zi: a caller that wants one of the two still passes both)
    if (!q || (g_ex && !gain) || (g_gain && !ex) || ((g_zi || g_a_head) && (!a || !zi)))
        return fail(GOLF_EINVAL, "%s: null pointer", who);
    if (B > 1 && (q_stride < T || (g_gain && ex_stride < T)))
        return fail(GOLF_EINVAL, "%s: row strides %lld / %lld below T=%d", who, (long long)q_stride, (long long)ex_stride, T);
    if (g_ex) {
        if (Tx < T || (B > 1 && g_ex_stride < Tx))
            return fail(GOLF_EINVAL, "%s: T=%d exceeds Tx=%d, or g_ex_stride=%lld below it", who, T, Tx,
                        (long long)g_ex_stride);
        const int64_t nblk = ceil_div(Tx, kBlockSamples);
        if (Tx > INT_MAX - kBlockSamples || nblk * B > INT_MAX)
            return fail(GOLF_EUNSUPPORTED, "%s: B=%d x Tx=%d beyond the launch grid", who, B, Tx);
    }
    if ((int64_t)B * F + B > INT_MAX) return fail(GOLF_EUNSUPPORTED, "%s: B*F=%lld beyond 2^31", who, (long long)B * F);
    hipStream_t st = (hipStream_t)stream;
    if (g_ex) {
        const int64_t nblk = ceil_div(Tx, kBlockSamples);
        hipLaunchKernelGGL(lpc_head_gex_kernel, dim3((unsigned)(nblk * B)), dim3(kBlock), 0, st, q, q_stride, gain, g_ex,
                           g_ex_stride, Tx, T, F, hop, (int)nblk);
        GOLF_LAUNCH_CHECK();
    }
    const int n_gain = g_gain ? B * F : 0;
    const int n_head = (g_a_head || g_zi) ? B : 0;
    if (n_gain + n_head > 0) {
        hipLaunchKernelGGL(lpc_head_reduce_kernel, dim3((unsigned)(n_gain + n_head)), dim3(64), 0, st, q, q_stride, ex,
                           ex_stride, a, zi, g_gain, g_a_head, g_zi, n_gain, T, F, M, hop);
        GOLF_LAUNCH_CHECK();
    }
    return GOLF_OK;
}
