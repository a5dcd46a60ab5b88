// Sample-wise LTV all-pole filter (include/golf_amd.h, a-1) with the recursion carried in FLOAT64: forward (one-shot and
// carried-state), adjoint, gradients and the gradient of the initial state, for every shape the fp32 filter serves (any
// 1 <= M <= 64, hop >= 1, F >= 1), 64-bit row addressing; gfx950 only.  The exact mode: for the utterances at the edge of
// stability on which NO fp32 recursion reaches 1e-4 of the float64 oracle, for gradcheck, for evaluation renders in double.
//
// The design is that of lpc_any.hip restated in double -- the cost class of an exact mode is one serial recursion per
// utterance.  One WAVE per utterance, one LANE per tap, the recursion in SCATTER (transposed direct) form:
//     y[t]  = ex[t]*G[t] + acc_0                       (lane 0, broadcast by two v_readfirstlane)
//     acc_k = fma(-A[t+1+k, k], y[t], acc_{k+1})       (a wave_shl:1 DPP move of each half + one v_fma_f64)
// Lane k evaluates its coefficient at its OWN time t+1+k and keeps its own frame and position n in it; a frame switch takes
// the row that was prefetched one frame earlier.  A coefficient is fma(n, (a1 - a0)*inv_hop, a0) with n counted from the frame
// start (kept as a double that counts in exact integer steps), and the taps of a sample accumulate in the order i = M-1 .. 0:
// a sample's bits depend neither on where a block of the carried-state form starts nor on where the 64-sample I/O blocks fall.
// EVERYTHING on the chain is double: accumulators, interpolated coefficient, up(gain), the broadcast y, the 64-deep history.
//
// The kernels are templates on the I/O scalar (float or double) of ex, gain, a, gy, y and the gradient outputs: values are
// widened at the load (exact) and rounded ONCE at the store; the arithmetic is the same double code in both instantiations.
// The carried state, the initial state zi, its gradient and the adjoint's g in the workspace are doubles whatever the I/O
// type: a chain of fp32-I/O blocks continues from the UNROUNDED last outputs, which is what keeps it on the one-shot's bits.
#include "common.h"
#include "device_common.h"

#include <climits>

namespace golf {

#define F64_WAVE_SHL1 0x130   /* lane l reads lane l+1 (lane 63: no source) */
#define F64_WAVE_SHR1 0x138   /* lane l reads lane l-1 (lane 0: no source) */

struct Halves {
    int lo, hi;
};
__device__ __forceinline__ Halves halves(double v) { return __builtin_bit_cast(Halves, v); }
__device__ __forceinline__ double whole(int lo, int hi) { return __builtin_bit_cast(double, Halves{lo, hi}); }

// lane l <- lane l+1, lane 63 <- 0
__device__ __forceinline__ double wave_down(double v) {
    const Halves h = halves(v);
    return whole(__builtin_amdgcn_update_dpp(0, h.lo, F64_WAVE_SHL1, 0xF, 0xF, true),
                 __builtin_amdgcn_update_dpp(0, h.hi, F64_WAVE_SHL1, 0xF, 0xF, true));
}
// lane l <- lane l-1, lane 0 <- head's lane 0
__device__ __forceinline__ double wave_push(double hist, double head) {
    const Halves h = halves(hist), o = halves(head);
    return whole(__builtin_amdgcn_update_dpp(o.lo, h.lo, F64_WAVE_SHR1, 0xF, 0xF, false),
                 __builtin_amdgcn_update_dpp(o.hi, h.hi, F64_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ double first_lane(double v) {
    const Halves h = halves(v);
    return whole(__builtin_amdgcn_readfirstlane(h.lo), __builtin_amdgcn_readfirstlane(h.hi));
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    const Halves h = halves(v);
    return whole(__builtin_amdgcn_readlane(h.lo, lane), __builtin_amdgcn_readlane(h.hi, lane));
}

// up(gain)[t] as the forward and the gradient kernel both evaluate it
template <typename IO>
__device__ __forceinline__ double gain_at(const IO* __restrict__ gb, int t, int F, int hop, double inv_hop) {
    if (F < 2) return (double)gb[0];
    int f = t / hop;
    if (f > F - 2) f = F - 2;
    const double g0 = (double)gb[f], g1 = (double)gb[f + 1];
    return fma((double)(t - f * hop), (g1 - g0) * inv_hop, g0);
}

// smallest value over the wave, as a scalar: four DPP butterfly steps inside the rows of 16, then the four rows
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_XOR1, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_XOR2, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ------------------------------------------------------------------------------------------
// Forward.  STATE: y[-1-i] = state[b][i] (doubles); a prologue replays those M values through the update without emitting
// (contributions to times before the block fall off lane 0 unused), which rebuilds the accumulators with the one-shot's
// operation sequence; the last M outputs, unrounded, are written back.
//   The time loop is cut into RUNS in which no lane changes its frame (wave_min of the lanes' distances to their next frame):
// the body of a run is branch-free and the lanes that have reached a frame boundary switch between two runs.
// ------------------------------------------------------------------------------------------
template <typename IO, bool STATE>
__global__ __launch_bounds__(64) void lpc_f64_fwd_kernel(const IO* __restrict__ ex, int64_t ex_stride,
                                                         const IO* __restrict__ gain, const IO* __restrict__ a,
                                                         IO* __restrict__ y, int64_t y_stride, int T, int F, int M, int hop,
                                                         double* __restrict__ state) {
    const int b = blockIdx.x, k = threadIdx.x;
    const IO* xb = ex + (size_t)b * ex_stride;
    IO* yb = y + (size_t)b * y_stride;
    const IO* gb = gain + (size_t)b * F;
    const IO* ab = a + (size_t)b * F * M + (k < M ? k : 0);   // this lane's tap of frame 0
    const double inv_hop = 1.0 / (double)hop;
    const bool tap = k < M;

    // this lane's own time: tau = t + 1 + k, t = the step being computed; the prologue starts at t = -M
    const int tau = (STATE ? -M : 0) + 1 + k;
    int f = 0, n = tau;   // (tau < 0: frame 0 with a negative position -- those contributions are never used)
    if (F >= 2 && tau >= 0) {
        f = tau / hop;
        if (f > F - 2) f = F - 2;
        n = tau - f * hop;
    }
    int left = (tap && f < F - 2) ? hop - n : INT_MAX;   // steps until this lane enters its next frame (never in the last one)
    auto row = [&](int fr) { return tap ? (double)ab[(size_t)(fr < F ? fr : F - 1) * M] : 0.0; };
    double a0 = row(f), a1 = row(f + 1), an = row(f + 2);
    double d = (a1 - a0) * inv_hop;
    double nd = (double)n;   // the position in the frame, counted in doubles: exact, and no conversion on the chain
    double acc = 0.0;
    double hist = 0.0;       // lane l: y[t-1-l], the last 64 outputs

    auto update = [&](double sy) {
        const double sh = wave_down(acc);
        const double cf = fma(nd, d, a0);
        acc = fma(-cf, sy, sh);
        nd += 1.0;
    };
    auto ran = [&](int run) {   // `run` steps done: the lanes that have reached their next frame take the row prefetched a frame ago
        left = left == INT_MAX ? INT_MAX : left - run;
        if (left == 0) {
            ++f;
            nd = 0.0;
            a0 = a1;
            a1 = an;
            d = (a1 - a0) * inv_hop;
            an = row(f + 2);
            left = f < F - 2 ? hop : INT_MAX;
        }
    };

    if constexpr (STATE) {
        hist = tap ? state[(size_t)b * M + k] : 0.0;
        for (int j = M - 1; j >= 0; --j) {   // y[-1-j], oldest first
            update(lane_bcast(hist, j));
            ran(1);
        }
    }

    // 64 samples of ex and what up(gain) needs for them, loaded one block ahead; the arithmetic waits for the block's turn
    double xr, g0, g1, gn;
    auto fetch = [&](int64_t t0) {
        const int64_t t = t0 + k;
        xr = g0 = g1 = gn = 0.0;
        if (t < T) {
            int fg = F >= 2 ? (int)t / hop : 0;
            if (F >= 2 && fg > F - 2) fg = F - 2;
            xr = (double)xb[t];
            g0 = (double)gb[fg];
            g1 = (double)gb[F >= 2 ? fg + 1 : fg];
            gn = (double)((int)t - fg * hop);
        }
    };
    auto step = [&](double& xcur) {
        const double y0 = acc + xcur;   // lane 0: y[t]
        const double sy = first_lane(y0);
        hist = wave_push(hist, y0);
        xcur = wave_down(xcur);
        update(sy);
    };
    fetch(0);
    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        double xcur = xr * fma(gn, (g1 - g0) * inv_hop, g0);   // lane l: ex[t0+l] * up(gain)[t0+l]
        fetch(t0 + 64);
        const int ns = T - t0 < 64 ? (int)(T - t0) : 64;
        for (int s = 0; s < ns;) {
            int run = wave_min_i32(left);
            if (run > ns - s) run = ns - s;
            s += run;
            int r = run;
            for (; r >= 8; r -= 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) step(xcur);
            }
            for (; r > 0; --r) step(xcur);
            ran(run);
        }
        if (k < ns) yb[t0 + ns - 1 - k] = (IO)hist;   // the one rounding of the fp32 instantiation
    }
    if constexpr (STATE) {
        if (tap) state[(size_t)b * M + k] = hist;   // y[T-1-k]; for T < M the old state shifted in behind the block
    }
}

// ------------------------------------------------------------------------------------------
// Adjoint: g[t] = gy[t] - sum_i A[t+1+i, i] g[t+1+i], t = T-1 .. 0, written to g (B, T) dense doubles.  The same runs; every
// lane is in the same frame, so a run ends where the frame of t does.
// ------------------------------------------------------------------------------------------
template <typename IO>
__global__ __launch_bounds__(64) void lpc_f64_adj_kernel(const IO* __restrict__ gy, int64_t gy_stride,
                                                         const IO* __restrict__ a, double* __restrict__ g, int T, int F,
                                                         int M, int hop) {
    const int b = blockIdx.x, k = threadIdx.x;
    const IO* gyb = gy + (size_t)b * gy_stride;
    double* gb = g + (size_t)b * T;
    const IO* ab = a + (size_t)b * F * M + (k < M ? k : 0);
    const double inv_hop = 1.0 / (double)hop;
    const bool tap = k < M;
    int f = 0;
    if (F >= 2) {
        f = (T - 1) / hop;
        if (f > F - 2) f = F - 2;
    }
    int n = T - 1 - f * hop;   // wave-uniform position of t in frame f
    auto row = [&](int fr) { return tap ? (double)ab[(size_t)(fr < 0 ? 0 : (fr < F ? fr : F - 1)) * M] : 0.0; };
    double a0 = row(f), a1 = row(f + 1), ap = row(f - 1);
    double d = (a1 - a0) * inv_hop;
    double nd = (double)n;
    double lam = 0.0, hist = 0.0;

    auto fetch = [&](int thi) {   // lane l: gy[thi - l]
        const int t = thi - k;
        return t >= 0 ? (double)gyb[t] : 0.0;
    };
    auto step = [&](double& gcur) {
        const double g0 = lam + gcur;   // lane 0: g[t]
        const double sg = first_lane(g0);
        hist = wave_push(hist, g0);
        gcur = wave_down(gcur);
        const double sh = wave_down(lam);
        const double cf = fma(nd, d, a0);
        lam = fma(-cf, sg, sh);
        nd -= 1.0;
    };
    double gnext = fetch(T - 1);
    for (int thi = T - 1; thi >= 0; thi -= 64) {
        double gcur = gnext;
        gnext = fetch(thi - 64);
        const int ns = thi + 1 < 64 ? thi + 1 : 64;
        for (int s = 0; s < ns;) {
            int run = f > 0 ? n + 1 : ns;   // samples of frame f that are left (frame 0 runs down to t = 0)
            if (run > ns - s) run = ns - s;
            s += run;
            n -= run;
            for (; run >= 8; run -= 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) step(gcur);
            }
            for (; run > 0; --run) step(gcur);
            if (n < 0 && f > 0) {   // the previous frame's row was prefetched a frame ago
                --f;
                n = hop - 1;
                nd = (double)n;
                a1 = a0;
                a0 = ap;
                d = (a1 - a0) * inv_hop;
                ap = row(f - 1);
            }
        }
        if (k < ns) gb[thi - ns + 1 + k] = hist;   // lane l: g[thi-(ns-1)+l]
    }
}

// ------------------------------------------------------------------------------------------
// Gradients, one workgroup per (utterance, frame):
//   g_ex[t] = g[t]*G[t];  g_gain[f] = sum_t w_f(t) g[t] ex[t];  g_a[f,i] = -sum_t w_f(t) g[t] y[t-1-i]
// with the hat weights of the interpolation's adjoint: frame(t) = min(t/hop, F-2), n = t - frame(t)*hop, weight 1 - n/hop to
// frame(t) and n/hop to frame(t)+1 (so the last sample (F-1)*hop goes wholly to frame F-1); F == 1: weight 1.  y[t] for t < 0
// is the initial state, y[-1-j] = zi[j] (zeros without one).  256 samples at a time are staged in LDS as p = w*g and y (with
// 64 samples of history), all doubles; wave v takes the v-th 64 of them, lane k the tap k.  Every sum runs in a fixed order,
// no atomics.  The workgroup of frame 0 also writes the zeros of g_ex beyond the output length (`tail` of them) and
//   g_zi[j] = -sum_{t < min(T, M-j)} A[t, t+j] g[t]
// with A as the adjoint kernel forms it.  A NULL output pointer skips that gradient's stores.
// ------------------------------------------------------------------------------------------
template <typename IO>
__global__ __launch_bounds__(256) void lpc_f64_grad_kernel(const double* __restrict__ g, const IO* __restrict__ y,
                                                           int64_t y_stride, const IO* __restrict__ ex, int64_t ex_stride,
                                                           const IO* __restrict__ gain, const IO* __restrict__ a,
                                                           const double* __restrict__ zi, IO* __restrict__ g_ex,
                                                           int64_t g_ex_stride, IO* __restrict__ g_gain,
                                                           IO* __restrict__ g_a, double* __restrict__ g_zi, int T, int F,
                                                           int M, int hop, int64_t tail) {
    __shared__ double ps[256], ys[256 + 64], part[4][64], pgain[4];
    const int f = (int)(blockIdx.x % (unsigned)F), b = (int)(blockIdx.x / (unsigned)F);
    const int tid = threadIdx.x, wv = tid >> 6, k = tid & 63;
    const double* gb = g + (size_t)b * T;
    const IO* yb = y + (size_t)b * y_stride;
    const IO* xb = ex + (size_t)b * ex_stride;
    const IO* gnb = gain + (size_t)b * F;
    const double* zb = zi ? zi + (size_t)b * M : nullptr;
    IO* gxb = g_ex ? g_ex + (size_t)b * g_ex_stride : nullptr;
    const double inv_hop = 1.0 / (double)hop, hopd = (double)hop;
    if (f == 0) {
        if (gxb)   // the excitation was longer than the output, its gradient there is zero
            for (int64_t u = tid; u < tail; u += 256) gxb[T + u] = (IO)0;
        if (g_zi && tid < M) {
            const int j = tid, H = T < M - j ? T : M - j;
            const IO* ab = a + (size_t)b * F * M;
            double s = 0.0;
            for (int t = 0; t < H; ++t) {
                int fr = F >= 2 ? t / hop : 0;
                if (F >= 2 && fr > F - 2) fr = F - 2;
                const double c0 = (double)ab[(size_t)fr * M + t + j];
                const double c1 = (double)ab[(size_t)(fr + 1 < F ? fr + 1 : F - 1) * M + t + j];
                s = fma(-fma((double)(t - fr * hop), (c1 - c0) * inv_hop, c0), gb[t], s);
            }
            g_zi[(size_t)b * M + j] = s;
        }
    }
    // samples with a weight for frame f: those of frame f-1 (rising edge) and of frame f (falling edge), clipped to [0, T)
    const int64_t tB = (int64_t)f * hop;           // first sample of frame f
    int64_t lo64 = f >= 1 ? tB - hop : 0;
    int64_t hi64 = f <= F - 2 ? tB + hop : tB;     // exclusive
    if (F < 2 || f >= F - 2) hi64 += 1;            // the last sample (F-1)*hop belongs to frame F-2
    if (hi64 > T) hi64 = T;
    if (lo64 > hi64) lo64 = hi64;
    const int lo = (int)lo64, hi = (int)hi64;
    const bool last = f == F - 1 && F >= 2;        // frame F-1 has a rising edge only
    double acc = 0.0, accg = 0.0;
    for (int64_t c0 = lo; c0 < hi; c0 += 256) {
        const int64_t t = c0 + tid;
        double p = 0.0, e = 0.0;
        if (t < hi) {
            const double gv = gb[t];
            e = (double)xb[t];
            double w = 1.0;
            bool mine = true;                      // g_ex[t] is written by the frame whose falling edge holds t
            if (F >= 2) {
                const bool rising = last || t < tB;
                w = rising ? (double)(t - (tB - hop)) / hopd : (double)(hop - (t - tB)) / hopd;
                mine = !rising;
            }
            if (mine && gxb) gxb[t] = (IO)(gv * gain_at(gnb, (int)t, F, hop, inv_hop));
            p = w * gv;
        }
        ps[tid] = p;
        accg = fma(p, e, accg);
        for (int u = tid; u < 256 + 64; u += 256) {   // ys[u] = y[c0 - 64 + u]
            const int64_t ty = c0 - 64 + u;
            double v = 0.0;
            if (ty >= 0) {
                if (ty < T) v = (double)yb[ty];
            } else if (zb && -1 - ty < M) {
                v = zb[-1 - ty];
            }
            ys[u] = v;
        }
        __syncthreads();
        if (k < M) {
            const double* pw = ps + 64 * wv;
            const double* yk = ys + 64 * wv + 63 - k;   // yk[s] = y[c0 + 64 wv + s - 1 - k]
#pragma unroll 8
            for (int s = 0; s < 64; ++s) acc = fma(pw[s], yk[s], acc);
        }
        __syncthreads();
    }
    // gain: fixed-order tree over the wave, then the four waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) accg += __shfl_down(accg, o);
    part[wv][k] = acc;
    if (k == 0) pgain[wv] = accg;
    __syncthreads();
    if (g_a && tid < M)
        g_a[((size_t)b * F + f) * M + tid] = (IO)(-(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]));
    if (g_gain && tid == 64) g_gain[(size_t)b * F + f] = (IO)(((pgain[0] + pgain[1]) + pgain[2]) + pgain[3]);
}

static size_t f64_ws_bytes(int B, int T) { return align_up((size_t)B * (size_t)T * sizeof(double), 256); }

static int check_f64_args(const char* who, int B, int T, int F, int M, int hop, int io) {
    if (B < 1 || T < 1 || F < 1 || M < 1 || hop < 1) return fail(GOLF_EINVAL, "%s: non-positive size", who);
    if (M > 64) return fail(GOLF_EUNSUPPORTED, "%s: M=%d > 64", who, M);
    if ((int64_t)T > (int64_t)(F - 1) * hop + 1)
        return fail(GOLF_EINVAL, "%s: T=%d exceeds (F-1)*hop+1=%lld", who, T, (long long)(F - 1) * hop + 1);
    if (io != 0 && io != 1) return fail(GOLF_EINVAL, "%s: io=%d is neither 0 (fp32 tensors) nor 1 (fp64 tensors)", who, io);
    return GOLF_OK;
}

template <typename IO>
static int launch_f64_fwd(const void* ex, int64_t ex_stride, const void* gain, const void* a, void* y, int64_t y_stride, int B,
                          int T, int F, int M, int hop, double* state, hipStream_t st) {
    if (state)
        hipLaunchKernelGGL((lpc_f64_fwd_kernel<IO, true>), dim3((unsigned)B), dim3(64), 0, st, (const IO*)ex, ex_stride,
                           (const IO*)gain, (const IO*)a, (IO*)y, y_stride, T, F, M, hop, state);
    else
        hipLaunchKernelGGL((lpc_f64_fwd_kernel<IO, false>), dim3((unsigned)B), dim3(64), 0, st, (const IO*)ex, ex_stride,
                           (const IO*)gain, (const IO*)a, (IO*)y, y_stride, T, F, M, hop, state);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

template <typename IO>
static int launch_f64_bwd(const void* gy, int64_t gy_stride, const void* y, int64_t y_stride, const void* ex,
                          int64_t ex_stride, const void* gain, const void* a, const double* zi, void* g_ex,
                          int64_t g_ex_stride, int64_t tail, void* g_gain, void* g_a, double* g_zi, int B, int T, int F, int M,
                          int hop, double* g, hipStream_t st) {
    hipLaunchKernelGGL(lpc_f64_adj_kernel<IO>, dim3((unsigned)B), dim3(64), 0, st, (const IO*)gy, gy_stride, (const IO*)a, g,
                       T, F, M, hop);
    GOLF_LAUNCH_CHECK();
    if (!g_ex && !g_gain && !g_a && !g_zi) return GOLF_OK;
    hipLaunchKernelGGL(lpc_f64_grad_kernel<IO>, dim3((unsigned)(B * F)), dim3(256), 0, st, (const double*)g, (const IO*)y,
                       y_stride, (const IO*)ex, ex_stride, (const IO*)gain, (const IO*)a, zi, (IO*)g_ex, g_ex_stride,
                       (IO*)g_gain, (IO*)g_a, g_zi, T, F, M, hop, tail);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" size_t golf_ltv_allpole_f64_workspace_bytes(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return f64_ws_bytes(B, T);
}

extern "C" int golf_ltv_allpole_fwd_f64(const void* ex, int64_t ex_stride, const void* gain, const void* a, void* y,
                                        int64_t y_stride, int B, int T, int F, int M, int hop, double* state, int io,
                                        void* stream) {
    const char* who = "ltv_allpole_fwd_f64";
    if (int rc = check_f64_args(who, B, T, F, M, hop, io)) return rc;
    if (!ex || !gain || !a || !y) return fail(GOLF_EINVAL, "%s: null pointer", who);
    if (ex_stride < T || y_stride < T) return fail(GOLF_EINVAL, "%s: row stride < T", who);
    hipStream_t st = (hipStream_t)stream;
    return io ? launch_f64_fwd<double>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st)
              : launch_f64_fwd<float>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
}

extern "C" int golf_ltv_allpole_bwd_f64(const void* gy, int64_t gy_stride, const void* y, int64_t y_stride, const void* ex,
                                        int64_t ex_stride, const void* gain, const void* a, const double* zi, void* g_ex,
                                        int64_t g_ex_stride, int64_t g_ex_width, void* g_gain, void* g_a, double* g_zi, int B,
                                        int T, int F, int M, int hop, void* ws, size_t ws_bytes, int io, void* stream) {
    const char* who = "ltv_allpole_bwd_f64";
    if (int rc = check_f64_args(who, B, T, F, M, hop, io)) return rc;
    if (!gy || !y || !ex || !gain || !a) return fail(GOLF_EINVAL, "%s: null pointer", who);
    if (gy_stride < T || y_stride < T || ex_stride < T) return fail(GOLF_EINVAL, "%s: row stride < T", who);
    if (g_ex && (g_ex_width < T || g_ex_stride < g_ex_width))
        return fail(GOLF_EINVAL, "%s: g_ex width %lld below T=%d, or row stride %lld below the width", who,
                    (long long)g_ex_width, T, (long long)g_ex_stride);
    if ((int64_t)B * F > INT_MAX) return fail(GOLF_EUNSUPPORTED, "%s: B*F=%lld beyond 2^31", who, (long long)B * F);
    if (!ws || ws_bytes < f64_ws_bytes(B, T) || ((uintptr_t)ws & 255))
        return fail(GOLF_EINVAL, "%s: workspace needs %zu bytes, 256-aligned (got %zu)", who, f64_ws_bytes(B, T), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int64_t tail = g_ex ? g_ex_width - (int64_t)T : 0;
    return io ? launch_f64_bwd<double>(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, zi, g_ex, g_ex_stride, tail, g_gain,
                                       g_a, g_zi, B, T, F, M, hop, (double*)ws, st)
              : launch_f64_bwd<float>(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, zi, g_ex, g_ex_stride, tail, g_gain,
                                      g_a, g_zi, B, T, F, M, hop, (double*)ws, st);
}
