// Sample-wise LTV all-pole filter (include/golf_amd.h, a-1) for the shapes WITHOUT a ring plan: any 1 <= M <= 64, any hop >= 1,
// any F >= 1 (lpc_ss_plan.h make_ss_plan returns false: no ring width in {8,16,24,32,40} divides the hop, M > 38, or F == 1).
// fp32, 64-bit row addressing.  Forward (one-shot and carried-state), adjoint and gradients; gfx950 only.
//
// The recursion is serial in time, so the cost of a sample is the dependent chain behind it.  One WAVE per utterance, one LANE
// per tap, and the recursion in SCATTER (transposed direct) form: lane k holds the partial sum destined for time t+k,
//     y[t]  = ex[t]*G[t] + acc_0                       (lane 0, broadcast by v_readfirstlane)
//     acc_k = fma(-A[t+1+k, k], y[t], acc_{k+1})       (one wave_shl:1 DPP move + one FMA)
// -- no cross-lane reduction and no memory on the chain.  Lane k evaluates its coefficient at its OWN time t+1+k, so every lane
// keeps its own frame and its own position n in it (for hop < M the lanes sit several frames apart); a frame switch takes the
// row that was prefetched one frame earlier.  A coefficient is fmaf(n, (a1 - a0)*inv_hop, a0) with n counted from the frame
// start, and the taps of a sample accumulate in the order i = M-1 .. 0: a sample's bits depend neither on where a block of the
// carried-state form starts nor on where the 64-sample I/O blocks fall.  The excitation and the outputs move 64 samples at a
// time (one coalesced load, one coalesced store); inside the loop the next input reaches lane 0 by a wave_shl:1 move and the
// output enters a 64-deep history register by wave_shr:1 -- which at the end IS the carried state (the last M outputs).
//   Lanes >= M run with zero coefficients.  (Their partial sums stay 0 while y is finite; once y overflows, 0*inf poisons them
//   one step earlier than the recursion itself would.)
//
// The adjoint is the same chain in reverse time, g[t] = gy[t] + lam_0, lam_k = fma(-A[t,k], g[t], lam_{k+1}), with every lane at
// the SAME time t (the frame switch is wave-uniform); it writes g to the workspace.  The gradients are then fully parallel:
// one workgroup per (utterance, frame) sums the hat-weighted correlations in a fixed order (no atomics: bit-reproducible).
#include "common.h"
#include "device_common.h"

#include <climits>

namespace golf {

#define DPP_WAVE_SHL1 0x130   /* lane l reads lane l+1 (lane 63: no source) */
#define DPP_WAVE_SHR1 0x138   /* lane l reads lane l-1 (lane 0: no source) */

// lane l <- lane l+1, lane 63 <- 0
__device__ __forceinline__ float wave_down(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), DPP_WAVE_SHL1, 0xF, 0xF, true));
}
// lane l <- lane l-1, lane 0 <- head's lane 0
__device__ __forceinline__ float wave_push(float hist, float head) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, head), __builtin_bit_cast(int, hist),
                                                                 DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ float first_lane(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// up(gain)[t] as the forward and the gradient kernel both evaluate it
__device__ __forceinline__ float gain_at(const float* __restrict__ gb, int t, int F, int hop, float inv_hop) {
    if (F < 2) return gb[0];
    int f = t / hop;
    if (f > F - 2) f = F - 2;
    const float g0 = gb[f], g1 = gb[f + 1];
    return fmaf((float)(t - f * hop), (g1 - g0) * inv_hop, g0);
}

// smallest value over the wave, as a scalar: four DPP butterfly steps inside the rows of 16, then the four rows
__device__ __forceinline__ int wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_XOR1, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_XOR2, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ------------------------------------------------------------------------------------------
// Forward.  STATE: y[-1-i] = state[b][i]; a prologue replays those M values through the update without emitting (contributions
// to times before the block fall off lane 0 unused), which rebuilds the accumulators with the one-shot's operation sequence.
//   The time loop is cut into RUNS in which no lane changes its frame (wave_min of the lanes' distances to their next frame):
// the body of a run is branch-free -- 9 VALU instructions per sample -- and the lanes that have reached a frame boundary switch
// between two runs.  With hop >= M that is one long run and M runs of one sample per hop samples.
// ------------------------------------------------------------------------------------------
template <bool STATE>
__global__ __launch_bounds__(64) void lpc_any_fwd_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                         const float* __restrict__ gain, const float* __restrict__ a,
                                                         float* __restrict__ y, int64_t y_stride, int T, int F, int M, int hop,
                                                         float* __restrict__ state) {
    const int b = blockIdx.x, k = threadIdx.x;
    const float* xb = ex + (size_t)b * ex_stride;
    float* yb = y + (size_t)b * y_stride;
    const float* gb = gain + (size_t)b * F;
    const float* ab = a + (size_t)b * F * M + (k < M ? k : 0);   // this lane's tap of frame 0
    const float inv_hop = 1.0f / (float)hop;
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
    auto row = [&](int fr) { return tap ? ab[(size_t)(fr < F ? fr : F - 1) * M] : 0.f; };
    float a0 = row(f), a1 = row(f + 1), an = row(f + 2);
    float d = (a1 - a0) * inv_hop;
    float acc = 0.f;
    float hist = 0.f;   // lane l: y[t-1-l], the last 64 outputs

    auto update = [&](float sy) {
        const float sh = wave_down(acc);
        const float cf = fmaf((float)n, d, a0);
        acc = fmaf(-cf, sy, sh);
        ++n;
    };
    auto ran = [&](int run) {   // `run` steps done: the lanes that have reached their next frame take the row prefetched a frame ago
        left = left == INT_MAX ? INT_MAX : left - run;
        if (left == 0) {
            ++f;
            n = 0;
            a0 = a1;
            a1 = an;
            d = (a1 - a0) * inv_hop;
            an = row(f + 2);
            left = f < F - 2 ? hop : INT_MAX;
        }
    };

    if constexpr (STATE) {
        hist = tap ? state[(size_t)b * M + k] : 0.f;
        for (int j = M - 1; j >= 0; --j) {   // y[-1-j], oldest first
            update(lane_bcast(hist, j));
            ran(1);
        }
    }

    // 64 samples of ex and what up(gain) needs for them, loaded one block ahead; the arithmetic waits for the block's turn
    float xr, g0, g1, gn;
    auto fetch = [&](int64_t t0) {
        const int64_t t = t0 + k;
        xr = g0 = g1 = gn = 0.f;
        if (t < T) {
            int fg = F >= 2 ? (int)t / hop : 0;
            if (F >= 2 && fg > F - 2) fg = F - 2;
            xr = xb[t];
            g0 = gb[fg];
            g1 = gb[F >= 2 ? fg + 1 : fg];
            gn = (float)((int)t - fg * hop);
        }
    };
    auto step = [&](float& xcur) {
        const float y0 = acc + xcur;   // lane 0: y[t]
        const float sy = first_lane(y0);
        hist = wave_push(hist, y0);
        xcur = wave_down(xcur);
        update(sy);
    };
    fetch(0);
    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        float xcur = xr * fmaf(gn, (g1 - g0) * inv_hop, g0);   // lane l: ex[t0+l] * up(gain)[t0+l]
        fetch(t0 + 64);
        const int ns = T - t0 < 64 ? (int)(T - t0) : 64;
        for (int s = 0; s < ns;) {
            int run = wave_min(left);
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
        if (k < ns) yb[t0 + ns - 1 - k] = hist;
    }
    if constexpr (STATE) {
        if (tap) state[(size_t)b * M + k] = hist;   // y[T-1-k]; for T < M the old state shifted in behind the block
    }
}

// ------------------------------------------------------------------------------------------
// Adjoint: g[t] = gy[t] - sum_i A[t+1+i, i] g[t+1+i], t = T-1 .. 0, written to g (B, T) dense.  The same runs; every lane is in
// the same frame, so a run ends where the frame of t does.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lpc_any_adj_kernel(const float* __restrict__ gy, int64_t gy_stride,
                                                         const float* __restrict__ a, float* __restrict__ g, int T, int F,
                                                         int M, int hop) {
    const int b = blockIdx.x, k = threadIdx.x;
    const float* gyb = gy + (size_t)b * gy_stride;
    float* gb = g + (size_t)b * T;
    const float* ab = a + (size_t)b * F * M + (k < M ? k : 0);
    const float inv_hop = 1.0f / (float)hop;
    const bool tap = k < M;
    int f = 0;
    if (F >= 2) {
        f = (T - 1) / hop;
        if (f > F - 2) f = F - 2;
    }
    int n = T - 1 - f * hop;   // wave-uniform position of t in frame f
    auto row = [&](int fr) { return tap ? ab[(size_t)(fr < 0 ? 0 : (fr < F ? fr : F - 1)) * M] : 0.f; };
    float a0 = row(f), a1 = row(f + 1), ap = row(f - 1);
    float d = (a1 - a0) * inv_hop;
    float lam = 0.f, hist = 0.f;

    auto fetch = [&](int thi) {   // lane l: gy[thi - l]
        const int t = thi - k;
        return t >= 0 ? gyb[t] : 0.f;
    };
    auto step = [&](float& gcur) {
        const float g0 = lam + gcur;   // lane 0: g[t]
        const float sg = first_lane(g0);
        hist = wave_push(hist, g0);
        gcur = wave_down(gcur);
        const float sh = wave_down(lam);
        const float cf = fmaf((float)n, d, a0);
        lam = fmaf(-cf, sg, sh);
        --n;
    };
    float gnext = fetch(T - 1);
    for (int thi = T - 1; thi >= 0; thi -= 64) {
        float gcur = gnext;
        gnext = fetch(thi - 64);
        const int ns = thi + 1 < 64 ? thi + 1 : 64;
        for (int s = 0; s < ns;) {
            int run = f > 0 ? n + 1 : ns;   // samples of frame f that are left (frame 0 runs down to t = 0)
            if (run > ns - s) run = ns - s;
            s += run;
            for (; run >= 8; run -= 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) step(gcur);
            }
            for (; run > 0; --run) step(gcur);
            if (n < 0 && f > 0) {   // the previous frame's row was prefetched a frame ago
                --f;
                n = hop - 1;
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
// frame(t) and n/hop to frame(t)+1 (so the last sample (F-1)*hop goes wholly to frame F-1); F == 1: weight 1.  256 samples
// at a time are staged in LDS as p = w*g, ex and y (with 64 samples of history); wave v takes the v-th 64 of them, lane k the
// tap k.  Every sum runs in a fixed order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpc_any_grad_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                           int64_t y_stride, const float* __restrict__ ex, int64_t ex_stride,
                                                           const float* __restrict__ gain, float* __restrict__ g_ex,
                                                           int64_t g_ex_stride, float* __restrict__ g_gain,
                                                           float* __restrict__ g_a, int T, int F, int M, int hop,
                                                           int64_t tail) {
    __shared__ float ps[256], ys[256 + 64], part[4][64], pgain[4];
    const int f = (int)(blockIdx.x % (unsigned)F), b = (int)(blockIdx.x / (unsigned)F);
    const int tid = threadIdx.x, wv = tid >> 6, k = tid & 63;
    const float* gb = g + (size_t)b * T;
    const float* yb = y + (size_t)b * y_stride;
    const float* xb = ex + (size_t)b * ex_stride;
    const float* gnb = gain + (size_t)b * F;
    float* gxb = g_ex + (size_t)b * g_ex_stride;
    if (f == 0)   // GOLF_SS_ZERO_TAIL: the excitation was longer than the output, its gradient there is zero
        for (int64_t u = tid; u < tail; u += 256) gxb[T + u] = 0.f;
    const float inv_hop = 1.0f / (float)hop, hopf = (float)hop;
    // samples with a weight for frame f: those of frame f-1 (rising edge) and of frame f (falling edge), clipped to [0, T)
    const int64_t tB = (int64_t)f * hop;           // first sample of frame f
    int64_t lo64 = f >= 1 ? tB - hop : 0;
    int64_t hi64 = f <= F - 2 ? tB + hop : tB;     // exclusive
    if (F < 2 || f >= F - 2) hi64 += 1;            // the last sample (F-1)*hop belongs to frame F-2
    if (hi64 > T) hi64 = T;
    if (lo64 > hi64) lo64 = hi64;
    const int lo = (int)lo64, hi = (int)hi64;
    const bool last = f == F - 1 && F >= 2;        // frame F-1 has a rising edge only
    float acc = 0.f, accg = 0.f;
    for (int64_t c0 = lo; c0 < hi; c0 += 256) {
        const int64_t t = c0 + tid;
        float p = 0.f, e = 0.f;
        if (t < hi) {
            const float gv = gb[t];
            e = xb[t];
            float w = 1.f;
            if (F >= 2) {
                const bool rising = last || t < tB;
                w = rising ? (float)(t - (tB - hop)) / hopf : (float)(hop - (t - tB)) / hopf;
                if (!rising) gxb[t] = gv * gain_at(gnb, (int)t, F, hop, inv_hop);
            } else {
                gxb[t] = gv * gain_at(gnb, (int)t, F, hop, inv_hop);
            }
            p = w * gv;
        }
        ps[tid] = p;
        accg = fmaf(p, e, accg);
        for (int u = tid; u < 256 + 64; u += 256) {   // ys[u] = y[c0 - 64 + u]
            const int64_t ty = c0 - 64 + u;
            ys[u] = (ty >= 0 && ty < T) ? yb[ty] : 0.f;
        }
        __syncthreads();
        if (k < M) {
            const float* pw = ps + 64 * wv;
            const float* yk = ys + 64 * wv + 63 - k;   // yk[s] = y[c0 + 64 wv + s - 1 - k]
#pragma unroll 8
            for (int s = 0; s < 64; ++s) acc = fmaf(pw[s], yk[s], acc);
        }
        __syncthreads();
    }
    // gain: fixed-order tree over the wave, then the four waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) accg += __shfl_down(accg, o);
    part[wv][k] = acc;
    if (k == 0) pgain[wv] = accg;
    __syncthreads();
    if (tid < M) g_a[((size_t)b * F + f) * M + tid] = -(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
    if (tid == 64) g_gain[(size_t)b * F + f] = ((pgain[0] + pgain[1]) + pgain[2]) + pgain[3];
}

// ------------------------------------------------------------------------------------------
// launchers (declared in common.h; called from lpc_ss.hip's entry points where make_ss_plan has no plan)
// ------------------------------------------------------------------------------------------
size_t any_ws_bytes(int B, int T) { return align_up((size_t)B * (size_t)T * sizeof(float), 256); }

int launch_any_fwd(const float* ex, int64_t ex_stride, const float* gain, const float* a, float* y, int64_t y_stride, int B,
                   int T, int F, int M, int hop, float* state, hipStream_t st) {
    if (state)
        hipLaunchKernelGGL(lpc_any_fwd_kernel<true>, dim3((unsigned)B), dim3(64), 0, st, ex, ex_stride, gain, a, y, y_stride,
                           T, F, M, hop, state);
    else
        hipLaunchKernelGGL(lpc_any_fwd_kernel<false>, dim3((unsigned)B), dim3(64), 0, st, ex, ex_stride, gain, a, y, y_stride,
                           T, F, M, hop, state);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int launch_any_bwd(const float* gy, int64_t gy_stride, const float* y, int64_t y_stride, const float* ex, int64_t ex_stride,
                   const float* gain, const float* a, float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T,
                   int F, int M, int hop, char* ws, int64_t tail, hipStream_t st) {
    if ((int64_t)B * F > INT_MAX) return fail(GOLF_EUNSUPPORTED, "ltv_allpole_bwd: B*F=%lld beyond 2^31", (long long)B * F);
    float* g = (float*)ws;
    hipLaunchKernelGGL(lpc_any_adj_kernel, dim3((unsigned)B), dim3(64), 0, st, gy, gy_stride, a, g, T, F, M, hop);
    GOLF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpc_any_grad_kernel, dim3((unsigned)(B * F)), dim3(256), 0, st, (const float*)g, y, y_stride, ex,
                       ex_stride, gain, g_ex, g_ex_stride, g_gain, g_a, T, F, M, hop, tail);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf
