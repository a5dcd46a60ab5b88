// f0 analysis for gfx950: audio -> (f0, period, aperiodicity) per frame by YIN (de Cheveigne & Kawahara, JASA 2002, steps
// 1-5).  Definition in include/golf_amd.h; the float64 restatement in tests/f0_ref.py is the checker.
//
// One launch, one workgroup of four waves per frame.
//   1. The S = W + tau_max samples of the frame go to LDS with coalesced loads, eight in flight per thread, zeros outside
//      [0, T) and in the padding behind S that lets the last lag tile read without a bounds check.
//   2. Difference function, fp32.  A lag tile is 64 lanes x YIN_R = 256 consecutive lags: lane l owns lags
//      tau0 + 4 l .. tau0 + 4 l + 3.  The j range [0, W) is cut in blocks of YIN_J = 8 samples and the blocks are dealt to
//      the four waves in contiguous quarters.  Per block a lane reads s[j0 .. j0+8) (the same address in every lane: a
//      broadcast) and its own s[j0 + tau0 + 4 l .. + 12), five ds_read_b128 for 32 (subtract, fused multiply-add) pairs,
//      issued as 16 + 16 packed fp32 operations on two lags at a time.
//      The lane stride is 16 bytes: the 16 lanes of every ds_read_b128 lane group cover 64 distinct banks, no conflict, no
//      padding or swizzle.  The W mod 8 samples left over are taken one at a time by the last wave.
//   3. Each wave writes its 256 partial sums to its LDS row; thread t adds the four rows in wave order into d[tau0 + t].
//      Order of every sum: j ascending inside a wave, waves ascending.  Nothing depends on the batch or on timing.
//   4. Wave 0: running sum of d[1..tau] in fp64, 64 lags at a time (a wave prefix sum in a fixed order and a carry),
//      d'[tau] = d[tau] tau / sum rounded to fp32, in place.
//   5. Wave 0: the search as ballots over 64 lags at a time (first lag below the threshold; then the first lag at which the
//      descent stops), the fallback argmin as a wave reduction on (value, index) that keeps the smaller index on ties.
//      Every loop runs at most tau_max / 64 + 1 times whatever the data, NaN included.
//   6. Lane 0 refines in fp64 from the fp32 d' and stores.  The frame's energy (voicing) is an fp64 sum in a fixed order.
//
// golf_f0_candidates_f32 (the front end of the path search in f0_viterbi.hip) is the same launch with another search: steps
// 1-4 are one device function, yin_dprime, that both kernels inline, and step 6 is one function, yin_refine.  Its wave 0
// picks the K <= 7 local minima of d' with the smallest values in K rounds: a round scans [tau_min, tau_max] 64 lags at a
// time for the smallest (value, lag) pair above the pair of the round before and ends in a wave reduction that keeps the
// smaller lag on ties, so a round is tau_max / 64 + 1 steps whatever the data and a NaN is never picked.  Lane k < n then
// refines pick k and stores it at its rank among the picks' lags (ascending lag); lanes n .. K-1 store the absent slots.
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int YIN_THREADS = 256;
constexpr int YIN_WAVES = YIN_THREADS / 64;
constexpr int YIN_R = 4;                     // consecutive lags per lane
constexpr int YIN_J = 8;                     // samples of j per block
constexpr int YIN_TILE = 64 * YIN_R;         // lags per tile
constexpr int YIN_MAX_S = 16384;             // samples of one frame (W + tau_max): at most 132 KiB of LDS
constexpr size_t YIN_LDS_OPT_IN = 160 * 1024;
constexpr int YIN_STAGE = 8;                 // samples a thread has in flight while staging
constexpr int YIN_GRID_X = 1 << 20;           // frames per grid row

static inline int yin_tiles(int tau_max) { return ceil_div(tau_max + 1, YIN_TILE); }
// floats of the staged frame: the last block of j (< W) against the last lag of the last tile, rounded up to a float4
static inline int yin_frame_floats(int W, int tau_max) { return (W + yin_tiles(tau_max) * YIN_TILE + 3) & ~3; }
static inline size_t yin_lds_bytes(int W, int tau_max) {
    return YIN_WAVES * sizeof(double) +
           sizeof(float) * ((size_t)yin_frame_floats(W, tau_max) + YIN_WAVES * YIN_TILE + tau_max + 1);
}

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double yin_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Steps 1-4 for the frame of this workgroup: on return d' [0, tau_max] is in LDS at *d_out (fp32) and the four partial
// energies of the window at *en_out, both visible to wave 0.  Returns the frame's index for wave 0 and -1 for the waves
// that are done (waves 1-3, and every wave of a workgroup behind the last frame).
__device__ __forceinline__ int yin_dprime(double* yin_lds, const float* __restrict__ x, int64_t x_stride, int G, int T, int F,
                                          int hop, int W, int tau_max, int64_t origin, int s_len, float** d_out,
                                          double** en_out) {
    double* en = yin_lds;                               // YIN_WAVES partial energies
    float* s = (float*)(yin_lds + YIN_WAVES);           // s_len floats, 16-byte aligned
    float* part = s + s_len;                            // YIN_WAVES rows of YIN_TILE partial sums
    float* d = part + YIN_WAVES * YIN_TILE;             // tau_max + 1: d, then d' in place
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar loop bounds
    const int64_t g64 = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;   // 2-D grid: 256 G threads may pass 2^32 in one dimension
    if (g64 >= G) return -1;
    const int g = (int)g64, b = g / F, f = g - b * F;
    const int S = W + tau_max;
    const int64_t o = origin + (int64_t)f * hop;
    const float* xr = x + (int64_t)b * x_stride;
    *d_out = d, *en_out = en;

    double e = 0.0;
    for (int k0 = tid; k0 < s_len; k0 += YIN_STAGE * YIN_THREADS) {   // YIN_STAGE loads in flight, then their stores
        float v[YIN_STAGE];
#pragma unroll
        for (int u = 0; u < YIN_STAGE; ++u) {
            const int k = k0 + u * YIN_THREADS;
            const int64_t t = o + k;
            v[u] = (k < S && t >= 0 && t < T) ? xr[t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < YIN_STAGE; ++u) {
            const int k = k0 + u * YIN_THREADS;
            if (k < s_len) s[k] = v[u];
            if (k < W) e += (double)v[u] * (double)v[u];
        }
    }
    e = yin_wave_sum(e);
    if (lane == 0) en[w] = e;
    __syncthreads();

    const int nblk = W / YIN_J;
    const int jb = (int)((int64_t)nblk * w / YIN_WAVES) * YIN_J, je = (int)((int64_t)nblk * (w + 1) / YIN_WAVES) * YIN_J;
    for (int tau0 = 0; tau0 <= tau_max; tau0 += YIN_TILE) {
        const float* sb = s + tau0 + YIN_R * lane;
        v2f acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};   // lags tau0 + 4 l + (0, 1) and + (2, 3)
        for (int j0 = jb; j0 < je; j0 += YIN_J) {
            float a[YIN_J], q[YIN_J + YIN_R];
#pragma unroll
            for (int k = 0; k < YIN_J; k += 4) {
                const float4 v = *(const float4*)(s + j0 + k);
                a[k] = v.x, a[k + 1] = v.y, a[k + 2] = v.z, a[k + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < YIN_J + YIN_R; k += 4) {
                v4f v = *(const v4f*)(sb + j0 + k);
                asm("" : "+v"(v));     // one ds_read_b128: hipcc otherwise reads the odd pairs below from LDS again
                q[k] = v.x, q[k + 1] = v.y, q[k + 2] = v.z, q[k + 3] = v.w;
            }
            // packed fp32 operands are even-aligned register pairs: (q[k], q[k+1]) is one as loaded for even k and a copy
            // for odd k (a few moves per 32 packed operations; hipcc's second pass over LDS for them made the loop LDS-bound)
            v2f ev[(YIN_J + YIN_R) / 2], od[(YIN_J + YIN_R) / 2 - 1];
#pragma unroll
            for (int m = 0; m < (YIN_J + YIN_R) / 2; ++m) ev[m] = v2f{q[2 * m], q[2 * m + 1]};
#pragma unroll
            for (int m = 0; m < (YIN_J + YIN_R) / 2 - 1; ++m) {
                od[m] = v2f{q[2 * m + 1], q[2 * m + 2]};
                asm("" : "+v"(od[m]));
            }
#pragma unroll
            for (int jj = 0; jj < YIN_J; ++jj) {
                const v2f aa = {a[jj], a[jj]};
                const v2f q01 = (jj & 1) ? od[jj / 2] : ev[jj / 2], q23 = (jj & 1) ? od[jj / 2 + 1] : ev[jj / 2 + 1];
                const v2f t01 = aa - q01, t23 = aa - q23;
                acc01 = __builtin_elementwise_fma(t01, t01, acc01);
                acc23 = __builtin_elementwise_fma(t23, t23, acc23);
            }
        }
        float acc[YIN_R] = {acc01.x, acc01.y, acc23.x, acc23.y};
        if (w == YIN_WAVES - 1)
            for (int j = nblk * YIN_J; j < W; ++j) {
                const float aj = s[j];
#pragma unroll
                for (int r = 0; r < YIN_R; ++r) {
                    const float t = aj - sb[j + r];
                    acc[r] = fmaf(t, t, acc[r]);
                }
            }
        *(float4*)(part + w * YIN_TILE + YIN_R * lane) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        __syncthreads();
        if (tau0 + tid <= tau_max) {
            float v = part[tid];
#pragma unroll
            for (int ww = 1; ww < YIN_WAVES; ++ww) v += part[ww * YIN_TILE + tid];
            d[tau0 + tid] = v;
        }
        __syncthreads();   // the next tile's partial sums; after the last tile, d for wave 0
    }
    if (w != 0) return -1;

    // d -> d' in place, 64 lags at a time
    double carry = 0.0;
    for (int c0 = 0; c0 <= tau_max; c0 += 64) {
        const int tau = c0 + lane;
        const double dv = (tau >= 1 && tau <= tau_max) ? (double)d[tau] : 0.0;
        double run = dv;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double up = __shfl_up(run, off);
            if (lane >= off) run += up;
        }
        run += carry;
        carry = __shfl(run, 63);
        if (tau <= tau_max) d[tau] = (tau >= 1 && run != 0.0) ? (float)(dv * (double)tau / run) : 1.f;
    }
    wave_lds_fence();
    return g;
}

// Step 6 at the integer lag star, in fp64 from the fp32 d'.
__device__ __forceinline__ void yin_refine(const float* d, int star, int tau_max, double& period, double& apv) {
    const double bq = (double)d[star];
    double delta = 0.0;
    apv = bq;
    if (star - 1 >= 1 && star + 1 <= tau_max) {
        const double aq = (double)d[star - 1], cq = (double)d[star + 1];
        const double den = aq - 2.0 * bq + cq;
        if (den > 0.0) {
            delta = fmin(fmax((aq - cq) / (2.0 * den), -1.0), 1.0);
            if (delta != 0.0) apv = bq - (aq - cq) * delta * 0.25;
        }
    }
    period = (double)star + delta;
}

__device__ __forceinline__ double yin_energy(const double* en) {
    double energy = en[0];
#pragma unroll
    for (int ww = 1; ww < YIN_WAVES; ++ww) energy += en[ww];
    return energy;
}

__global__ __launch_bounds__(YIN_THREADS) void f0_yin_kernel(const float* __restrict__ x, int64_t x_stride,
                                                             float* __restrict__ f0_out, float* __restrict__ period_out,
                                                             float* __restrict__ ap_out, int G, int T, int F, int hop, int W,
                                                             int tau_min, int tau_max, int64_t origin, int s_len,
                                                             double sample_rate, double threshold, double floor2) {
    extern __shared__ __attribute__((aligned(16))) double yin_lds[];
    float* d;
    double* en;
    const int g = yin_dprime(yin_lds, x, x_stride, G, T, F, hop, W, tau_max, origin, s_len, &d, &en);
    if (g < 0) return;
    const int lane = threadIdx.x & 63;

    // first lag below the threshold, then down to where the descent stops
    int star = -1;
    bool found = false;
    for (int c0 = tau_min; c0 <= tau_max; c0 += 64) {
        const int tau = c0 + lane;
        const unsigned long long m = __ballot(tau <= tau_max && (double)d[tau] < threshold);
        if (m) {
            star = c0 + __ffsll((long long)m) - 1;
            found = true;
            break;
        }
    }
    if (found) {
        for (int c0 = star; c0 <= tau_max; c0 += 64) {
            const int tau = c0 + lane;
            const unsigned long long m = __ballot(tau <= tau_max && (tau + 1 > tau_max || !(d[tau + 1] < d[tau])));
            if (m) {   // always taken at tau_max at the latest
                star = c0 + __ffsll((long long)m) - 1;
                break;
            }
        }
    } else {
        float bv = INFINITY;
        int bi = 0x7fffffff;
        for (int tau = tau_min + lane; tau <= tau_max; tau += 64) {
            const float v = d[tau];
            if (v < bv || bi == 0x7fffffff) bv = v, bi = tau;   // ascending tau: the first of equal values stays
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        }
        star = bi;
    }

    if (lane == 0) {
        double period, apv;
        yin_refine(d, star, tau_max, period, apv);
        const double energy = yin_energy(en);
        const bool voiced = found && energy / (double)W > floor2;
        if (f0_out) f0_out[g] = voiced ? (float)(sample_rate / period) : 0.f;
        if (period_out) period_out[g] = (float)period;
        if (ap_out) ap_out[g] = (float)apv;
    }
}

constexpr int YIN_MAX_K = 7;                 // candidates per frame

__global__ __launch_bounds__(YIN_THREADS) void f0_candidates_kernel(const float* __restrict__ x, int64_t x_stride,
                                                                    float* __restrict__ period_out,
                                                                    float* __restrict__ ap_out, int G, int T, int F, int hop,
                                                                    int W, int tau_min, int tau_max, int K, int64_t origin,
                                                                    int s_len, double floor2) {
    extern __shared__ __attribute__((aligned(16))) double yin_lds[];
    float* d;
    double* en;
    const int g = yin_dprime(yin_lds, x, x_stride, G, T, F, hop, W, tau_max, origin, s_len, &d, &en);
    if (g < 0) return;
    const int lane = threadIdx.x & 63;

    // K rounds: the smallest (value, lag) among the local minima that lie above the pick of the round before
    int ct[YIN_MAX_K], n = 0;
    float pv = -INFINITY;
    int pt = -1;
    bool more = yin_energy(en) / (double)W > floor2;   // a quiet frame (and one of NaN) has no candidate
#pragma unroll
    for (int r = 0; r < YIN_MAX_K; ++r) {
        ct[r] = 0x7fffffff;
        if (r < K && more) {
            float bv = INFINITY;
            int bi = 0x7fffffff;
            for (int tau = tau_min + lane; tau <= tau_max; tau += 64) {
                const float v = d[tau], left = d[tau - 1], right = tau < tau_max ? d[tau + 1] : INFINITY;
                const bool is_min = v < left && v <= right;               // false on a NaN
                const bool above = v > pv || (v == pv && tau > pt);
                if (is_min && above && (v < bv || bi == 0x7fffffff)) bv = v, bi = tau;   // ascending tau: the first of equals stays
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
            }
            if (bi == 0x7fffffff) {
                more = false;
            } else {
                ct[r] = bi, pv = bv, pt = bi, n = r + 1;
            }
        }
    }

    // lane k < n refines pick k and stores it at the rank of its lag; lanes n .. K-1 store the absent slots
    if (lane < K) {
        int mine = 0x7fffffff, slot = lane;
        float pf = 0.f, af = INFINITY;
#pragma unroll
        for (int r = 0; r < YIN_MAX_K; ++r)
            if (lane == r) mine = ct[r];
        if (lane < n) {
            slot = 0;
#pragma unroll
            for (int r = 0; r < YIN_MAX_K; ++r) slot += ct[r] < mine;
            double period, apv;
            yin_refine(d, mine, tau_max, period, apv);
            pf = (float)period, af = (float)apv;
        }
        period_out[(int64_t)g * K + slot] = pf;
        ap_out[(int64_t)g * K + slot] = af;
    }
}

}  // namespace golf

using namespace golf;

// the refusals that golf_f0_yin_f32 and golf_f0_candidates_f32 share; GOLF_OK if none applies
static int yin_refuse(const char* who, int64_t x_stride, int B, int T, int F, int hop, int W, int tau_min, int tau_max) {
    if (B < 1 || T < 0 || F < 1) return fail(GOLF_EINVAL, "%s: bad size (B=%d T=%d F=%d)", who, B, T, F);
    if (x_stride < T) return fail(GOLF_EINVAL, "%s: row stride %lld < T=%d", who, (long long)x_stride, T);
    if (hop < 1) return fail(GOLF_EUNSUPPORTED, "%s: hop=%d must be >= 1", who, hop);
    if (tau_min < 1) return fail(GOLF_EUNSUPPORTED, "%s: tau_min=%d must be >= 1", who, tau_min);
    if (tau_max <= tau_min) return fail(GOLF_EUNSUPPORTED, "%s: tau_max=%d must exceed tau_min=%d", who, tau_max, tau_min);
    if (W < 1) return fail(GOLF_EUNSUPPORTED, "%s: window W=%d must be >= 1", who, W);
    if ((int64_t)W + tau_max > YIN_MAX_S)
        return fail(GOLF_EUNSUPPORTED, "%s: frame W + tau_max = %lld samples exceeds %d (a frame must fit LDS)", who,
                    (long long)W + tau_max, YIN_MAX_S);
    if ((int64_t)B * F >= ((int64_t)1 << 31))
        return fail(GOLF_EUNSUPPORTED, "%s: B*F = %lld frames, must be < 2^31", who, (long long)B * F);
    return GOLF_OK;
}

extern "C" {

int golf_f0_yin_f32(const float* x, int64_t x_stride, float* f0, float* period, float* ap, int B, int T, int F, int hop,
                    int W, int tau_min, int tau_max, int64_t origin, double sample_rate, double threshold, double rms_floor,
                    void* stream) {
    if ((!x && T > 0) || (!f0 && !period && !ap))
        return fail(GOLF_EINVAL, "f0_yin: null pointer (x=%p f0=%p period=%p ap=%p; at least one output)", x, f0, period, ap);
    if (!(sample_rate > 0.0)) return fail(GOLF_EINVAL, "f0_yin: sample_rate=%g must be positive", sample_rate);
    if (const int rc = yin_refuse("f0_yin", x_stride, B, T, F, hop, W, tau_min, tau_max)) return rc;
    const size_t lds = yin_lds_bytes(W, tau_max);
    if (lds > 64 * 1024) {   /* > 64 KB of dynamic LDS per workgroup needs the opt-in */
        static const hipError_t attr =
            hipFuncSetAttribute((const void*)f0_yin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, YIN_LDS_OPT_IN);
        if (attr != hipSuccess)
            return fail((int)attr, "f0_yin: cannot raise the dynamic LDS limit: %s", hipGetErrorString(attr));
    }
    const int G = B * F, gx = G < YIN_GRID_X ? G : YIN_GRID_X;
    hipLaunchKernelGGL(f0_yin_kernel, dim3((unsigned)gx, (unsigned)ceil_div(G, gx)), dim3(YIN_THREADS), lds,
                       (hipStream_t)stream, x, x_stride, f0, period, ap, G, T, F, hop, W, tau_min, tau_max, origin,
                       yin_frame_floats(W, tau_max), sample_rate,
                       threshold, rms_floor * rms_floor);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int golf_f0_candidates_f32(const float* x, int64_t x_stride, float* cand_period, float* cand_ap, int B, int T, int F, int hop,
                           int W, int tau_min, int tau_max, int K, int64_t origin, double rms_floor, void* stream) {
    if ((!x && T > 0) || !cand_period || !cand_ap)
        return fail(GOLF_EINVAL, "f0_candidates: null pointer (x=%p cand_period=%p cand_ap=%p)", x, cand_period, cand_ap);
    if (const int rc = yin_refuse("f0_candidates", x_stride, B, T, F, hop, W, tau_min, tau_max)) return rc;
    if (K < 1 || K > YIN_MAX_K) return fail(GOLF_EUNSUPPORTED, "f0_candidates: K=%d candidates, must be 1..%d", K, YIN_MAX_K);
    const size_t lds = yin_lds_bytes(W, tau_max);
    if (lds > 64 * 1024) {   /* > 64 KB of dynamic LDS per workgroup needs the opt-in */
        static const hipError_t attr = hipFuncSetAttribute((const void*)f0_candidates_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, YIN_LDS_OPT_IN);
        if (attr != hipSuccess)
            return fail((int)attr, "f0_candidates: cannot raise the dynamic LDS limit: %s", hipGetErrorString(attr));
    }
    const int G = B * F, gx = G < YIN_GRID_X ? G : YIN_GRID_X;
    hipLaunchKernelGGL(f0_candidates_kernel, dim3((unsigned)gx, (unsigned)ceil_div(G, gx)), dim3(YIN_THREADS), lds,
                       (hipStream_t)stream, x, x_stride, cand_period, cand_ap, G, T, F, hop, W, tau_min, tau_max, K, origin,
                       yin_frame_floats(W, tau_max), rms_floor * rms_floor);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
