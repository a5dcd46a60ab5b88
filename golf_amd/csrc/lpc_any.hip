// Sample-wise LTV all-pole filter (include/golf_amd.h, a-1), one WAVE per utterance: any 1 <= M <= 64, any hop >= 1, any F >= 1,
// 64-bit row addressing; gfx950 only.  Forward (one-shot and carried-state), adjoint and gradients, as templates on the compute
// scalar C and the I/O scalar IO, instantiated three times:
//   (float, float)    the fp32 chain of the shapes WITHOUT a ring plan (lpc_ss_plan.h make_ss_plan returns false: no ring width
//                     in {8,16,24,32,40} divides the hop, M > 38, or F == 1), called from lpc_ss.hip's entry points;
//   (double, float)   the recursion in FLOAT64 on fp32 tensors (mode="fp64"), and
//   (double, double)  on double tensors, for every shape: golf_ltv_allpole_{fwd,bwd}_f64 below.  The exact mode: for the
//                     utterances at the edge of stability on which NO fp32 recursion reaches 1e-4 of the float64 oracle, for
//                     gradcheck, for evaluation renders in double -- its cost class is one serial recursion per utterance.
//
// The recursion is serial in time, so the cost of a sample is the dependent chain behind it.  One LANE per tap, and the
// recursion in SCATTER (transposed direct) form: lane k holds the partial sum destined for time t+k,
//     y[t]  = ex[t]*G[t] + acc_0                       (lane 0, broadcast by v_readfirstlane)
//     acc_k = fma(-A[t+1+k, k], y[t], acc_{k+1})       (one wave_shl:1 DPP move + one FMA; in double, a move of each half)
// -- no cross-lane reduction and no memory on the chain.  Lane k evaluates its coefficient at its OWN time t+1+k, so every lane
// keeps its own frame and its own position n in it (for hop < M the lanes sit several frames apart); a frame switch takes the
// row that was prefetched one frame earlier.  A coefficient is fma(n, (a1 - a0)*inv_hop, a0) with n counted from the frame
// start, and the taps of a sample accumulate in the order i = M-1 .. 0: a sample's bits depend neither on where a block of the
// carried-state form starts nor on where the 64-sample I/O blocks fall.  The excitation and the outputs move 64 samples at a
// time (one coalesced load, one coalesced store); inside the loop the next input reaches lane 0 by a wave_shl:1 move and the
// output enters a 64-deep history register by wave_shr:1 -- which at the end IS the carried state (the last M outputs).
//   Lanes >= M run with zero coefficients.  (Their partial sums stay 0 while y is finite; once y overflows, 0*inf poisons them
//   one step earlier than the recursion itself would.)
//
// EVERYTHING on the chain is of type C: accumulators, interpolated coefficient, up(gain), the broadcast y, the history.  Values
// of type IO are widened at the load (exact) and rounded ONCE at the store.  The carried state, the initial state zi, its
// gradient and the adjoint's g in the workspace are of type C whatever the I/O type: a chain of fp32-I/O blocks in double
// continues from the UNROUNDED last outputs, which is what keeps it on the one-shot's bits.
//
// The adjoint is the same chain in reverse time, g[t] = gy[t] + lam_0, lam_k = fma(-A[t,k], g[t], lam_{k+1}), with every lane at
// the SAME time t (the frame switch is wave-uniform); it writes g to the workspace.  The gradients are then fully parallel:
// one workgroup per (utterance, frame) sums the hat-weighted correlations in a fixed order (no atomics: bit-reproducible).
#include "common.h"
#include "device_common.h"

#include <climits>

namespace golf {

struct Halves {
    int lo, hi;
};
__device__ __forceinline__ Halves halves(double v) { return __builtin_bit_cast(Halves, v); }
__device__ __forceinline__ double whole(int lo, int hi) { return __builtin_bit_cast(double, Halves{lo, hi}); }

// lane l <- lane l+1, lane 63 <- 0
__device__ __forceinline__ int wave_down(int v) { return __builtin_amdgcn_update_dpp(0, v, DPP_WAVE_SHL1, 0xF, 0xF, true); }
__device__ __forceinline__ float wave_down(float v) { return __builtin_bit_cast(float, wave_down(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ double wave_down(double v) { return whole(wave_down(halves(v).lo), wave_down(halves(v).hi)); }
// lane l <- lane l-1, lane 0 <- head's lane 0
__device__ __forceinline__ int wave_push(int hist, int head) {
    return __builtin_amdgcn_update_dpp(head, hist, DPP_WAVE_SHR1, 0xF, 0xF, false);
}
__device__ __forceinline__ float wave_push(float hist, float head) {
    return __builtin_bit_cast(float, wave_push(__builtin_bit_cast(int, hist), __builtin_bit_cast(int, head)));
}
__device__ __forceinline__ double wave_push(double hist, double head) {
    return whole(wave_push(halves(hist).lo, halves(head).lo), wave_push(halves(hist).hi, halves(head).hi));
}
__device__ __forceinline__ float first_lane(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double first_lane(double v) {
    return whole(__builtin_amdgcn_readfirstlane(halves(v).lo), __builtin_amdgcn_readfirstlane(halves(v).hi));
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    return whole(__builtin_amdgcn_readlane(halves(v).lo, lane), __builtin_amdgcn_readlane(halves(v).hi, lane));
}

// The position n of a sample in its frame, as the coefficient's fma takes it -- the one place where the two compute types differ
// on purpose.  fp32 keeps the int and converts it at every step (a float counter stops being exact at 2^24).  double counts in
// doubles (exact integer steps, no conversion on the chain) beside an int that moves once per run, for the adjoint's run length.
template <typename C>
struct TapPos;
template <>
struct TapPos<float> {
    int n;
    __device__ __forceinline__ explicit TapPos(int n0) : n(n0) {}
    __device__ __forceinline__ float value() const { return (float)n; }
    __device__ __forceinline__ int index() const { return n; }
    __device__ __forceinline__ void step(int s) { n += s; }   // one sample
    __device__ __forceinline__ void ran(int) {}                // a run: the int has moved with the steps
    __device__ __forceinline__ void set(int v) { n = v; }
};
template <>
struct TapPos<double> {
    int i;
    double n;
    __device__ __forceinline__ explicit TapPos(int n0) : i(n0), n((double)n0) {}
    __device__ __forceinline__ double value() const { return n; }
    __device__ __forceinline__ int index() const { return i; }
    __device__ __forceinline__ void step(int s) { n += (double)s; }
    __device__ __forceinline__ void ran(int s) { i += s; }
    __device__ __forceinline__ void set(int v) { i = v, n = (double)v; }
};

// up(gain)[t] as the forward and the gradient kernel both evaluate it
template <typename C, typename IO>
__device__ __forceinline__ C gain_at(const IO* __restrict__ gb, int t, int F, int hop, C inv_hop) {
    if (F < 2) return (C)gb[0];
    int f = t / hop;
    if (f > F - 2) f = F - 2;
    const C g0 = (C)gb[f], g1 = (C)gb[f + 1];
    return fma((C)(t - f * hop), (g1 - g0) * inv_hop, g0);
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
// to times before the block fall off lane 0 unused), which rebuilds the accumulators with the one-shot's operation sequence;
// the last M outputs, unrounded, are written back.
//   The time loop is cut into RUNS in which no lane changes its frame (wave_min of the lanes' distances to their next frame):
// the body of a run is branch-free -- 9 VALU instructions per sample in fp32 -- and the lanes that have reached a frame
// boundary switch between two runs.  With hop >= M that is one long run and M runs of one sample per hop samples.
// ------------------------------------------------------------------------------------------
template <typename C, typename IO, bool STATE>
__global__ __launch_bounds__(64) void lpc_any_fwd_kernel(const IO* __restrict__ ex, int64_t ex_stride,
                                                         const IO* __restrict__ gain, const IO* __restrict__ a,
                                                         IO* __restrict__ y, int64_t y_stride, int T, int F, int M, int hop,
                                                         C* __restrict__ state) {
    const int b = blockIdx.x, k = threadIdx.x;
    const IO* xb = ex + (size_t)b * ex_stride;
    IO* yb = y + (size_t)b * y_stride;
    const IO* gb = gain + (size_t)b * F;
    const IO* ab = a + (size_t)b * F * M + (k < M ? k : 0);   // this lane's tap of frame 0
    const C inv_hop = C(1) / (C)hop;
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
    auto row = [&](int fr) { return tap ? (C)ab[(size_t)(fr < F ? fr : F - 1) * M] : C(0); };
    C a0 = row(f), a1 = row(f + 1), an = row(f + 2);
    C d = (a1 - a0) * inv_hop;
    TapPos<C> pos(n);
    C acc = 0;
    C hist = 0;   // lane l: y[t-1-l], the last 64 outputs

    auto update = [&](C sy) {
        const C sh = wave_down(acc);
        const C cf = fma(pos.value(), d, a0);
        acc = fma(-cf, sy, sh);
        pos.step(1);
    };
    auto ran = [&](int run) {   // `run` steps done: the lanes that have reached their next frame take the row prefetched a frame ago
        left = left == INT_MAX ? INT_MAX : left - run;
        if (left == 0) {
            ++f;
            pos.set(0);
            a0 = a1;
            a1 = an;
            d = (a1 - a0) * inv_hop;
            an = row(f + 2);
            left = f < F - 2 ? hop : INT_MAX;
        }
    };

    if constexpr (STATE) {
        hist = tap ? state[(size_t)b * M + k] : C(0);
        for (int j = M - 1; j >= 0; --j) {   // y[-1-j], oldest first
            update(lane_bcast(hist, j));
            ran(1);
        }
    }

    // 64 samples of ex and what up(gain) needs for them, loaded one block ahead; the arithmetic waits for the block's turn
    C xr, g0, g1, gn;
    auto fetch = [&](int64_t t0) {
        const int64_t t = t0 + k;
        xr = g0 = g1 = gn = 0;
        if (t < T) {
            int fg = F >= 2 ? (int)t / hop : 0;
            if (F >= 2 && fg > F - 2) fg = F - 2;
            xr = (C)xb[t];
            g0 = (C)gb[fg];
            g1 = (C)gb[F >= 2 ? fg + 1 : fg];
            gn = (C)((int)t - fg * hop);
        }
    };
    auto step = [&](C& xcur) {
        const C y0 = acc + xcur;   // lane 0: y[t]
        const C sy = first_lane(y0);
        hist = wave_push(hist, y0);
        xcur = wave_down(xcur);
        update(sy);
    };
    fetch(0);
    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        C xcur = xr * fma(gn, (g1 - g0) * inv_hop, g0);   // lane l: ex[t0+l] * up(gain)[t0+l]
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
        if (k < ns) yb[t0 + ns - 1 - k] = (IO)hist;   // the one rounding of (double, float)
    }
    if constexpr (STATE) {
        if (tap) state[(size_t)b * M + k] = hist;   // y[T-1-k]; for T < M the old state shifted in behind the block
    }
}

// ------------------------------------------------------------------------------------------
// Adjoint: g[t] = gy[t] - sum_i A[t+1+i, i] g[t+1+i], t = T-1 .. 0, written to g (B, T) dense.  The same runs; every lane is in
// the same frame, so a run ends where the frame of t does.
// ------------------------------------------------------------------------------------------
template <typename C, typename IO>
__global__ __launch_bounds__(64) void lpc_any_adj_kernel(const IO* __restrict__ gy, int64_t gy_stride,
                                                         const IO* __restrict__ a, C* __restrict__ g, int T, int F, int M,
                                                         int hop) {
    const int b = blockIdx.x, k = threadIdx.x;
    const IO* gyb = gy + (size_t)b * gy_stride;
    C* gb = g + (size_t)b * T;
    const IO* ab = a + (size_t)b * F * M + (k < M ? k : 0);
    const C inv_hop = C(1) / (C)hop;
    const bool tap = k < M;
    int f = 0;
    if (F >= 2) {
        f = (T - 1) / hop;
        if (f > F - 2) f = F - 2;
    }
    TapPos<C> pos(T - 1 - f * hop);   // wave-uniform position of t in frame f
    auto row = [&](int fr) { return tap ? (C)ab[(size_t)(fr < 0 ? 0 : (fr < F ? fr : F - 1)) * M] : C(0); };
    C a0 = row(f), a1 = row(f + 1), ap = row(f - 1);
    C d = (a1 - a0) * inv_hop;
    C lam = 0, hist = 0;

    auto fetch = [&](int thi) {   // lane l: gy[thi - l]
        const int t = thi - k;
        return t >= 0 ? (C)gyb[t] : C(0);
    };
    auto step = [&](C& gcur) {
        const C g0 = lam + gcur;   // lane 0: g[t]
        const C sg = first_lane(g0);
        hist = wave_push(hist, g0);
        gcur = wave_down(gcur);
        const C sh = wave_down(lam);
        const C cf = fma(pos.value(), d, a0);
        lam = fma(-cf, sg, sh);
        pos.step(-1);
    };
    C gnext = fetch(T - 1);
    for (int thi = T - 1; thi >= 0; thi -= 64) {
        C gcur = gnext;
        gnext = fetch(thi - 64);
        const int ns = thi + 1 < 64 ? thi + 1 : 64;
        for (int s = 0; s < ns;) {
            int run = f > 0 ? pos.index() + 1 : ns;   // samples of frame f that are left (frame 0 runs down to t = 0)
            if (run > ns - s) run = ns - s;
            s += run;
            pos.ran(-run);
            for (; run >= 8; run -= 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) step(gcur);
            }
            for (; run > 0; --run) step(gcur);
            if (pos.index() < 0 && f > 0) {   // the previous frame's row was prefetched a frame ago
                --f;
                pos.set(hop - 1);
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
// with the hat weights of the interpolation's adjoint (device_common.h: HatSpan).  256 samples at a time are staged in LDS as
// p = w*g and y (with 64 samples of history), of type C; wave v takes the v-th 64 of them, lane k the tap k.  Every sum runs in
// a fixed order, no atomics.  The workgroup of frame 0 also writes the zeros of g_ex beyond the output length (`tail` of them:
// the excitation was longer than the output).
//   ZI (the float64 entries): y[t] for t < 0 is the initial state, y[-1-j] = zi[j] (zeros for a null zi); the workgroup of
// frame 0 also writes g_zi[j] = -sum_{t < min(T, M-j)} A[t, t+j] g[t] with A as the adjoint kernel forms it; and a NULL output
// pointer skips that gradient's stores.  Without ZI, zi and g_zi are not read and every output is written.
// ------------------------------------------------------------------------------------------
template <typename C, typename IO, bool ZI>
__global__ __launch_bounds__(256) void lpc_any_grad_kernel(const C* __restrict__ g, const IO* __restrict__ y, int64_t y_stride,
                                                           const IO* __restrict__ ex, int64_t ex_stride,
                                                           const IO* __restrict__ gain, const IO* __restrict__ a,
                                                           const C* __restrict__ zi, IO* __restrict__ g_ex,
                                                           int64_t g_ex_stride, IO* __restrict__ g_gain, IO* __restrict__ g_a,
                                                           C* __restrict__ g_zi, int T, int F, int M, int hop, int64_t tail) {
    __shared__ C ps[256], ys[256 + 64], part[4][64], pgain[4];
    const int f = (int)(blockIdx.x % (unsigned)F), b = (int)(blockIdx.x / (unsigned)F);
    const int tid = threadIdx.x, wv = tid >> 6, k = tid & 63;
    const C* gb = g + (size_t)b * T;
    const IO* yb = y + (size_t)b * y_stride;
    const IO* xb = ex + (size_t)b * ex_stride;
    const IO* gnb = gain + (size_t)b * F;
    const C* zb = ZI && zi ? zi + (size_t)b * M : nullptr;
    IO* gxb = !ZI || g_ex ? g_ex + (size_t)b * g_ex_stride : nullptr;
    const C inv_hop = C(1) / (C)hop;
    if (f == 0) {
        if (!ZI || gxb)
            for (int64_t u = tid; u < tail; u += 256) gxb[T + u] = (IO)0;
        if constexpr (ZI) {
            if (g_zi && tid < M) {
                const int j = tid, H = T < M - j ? T : M - j;
                const IO* ab = a + (size_t)b * F * M;
                C s = 0;
                for (int t = 0; t < H; ++t) {
                    int fr = F >= 2 ? t / hop : 0;
                    if (F >= 2 && fr > F - 2) fr = F - 2;
                    const C c0 = (C)ab[(size_t)fr * M + t + j];
                    const C c1 = (C)ab[(size_t)(fr + 1 < F ? fr + 1 : F - 1) * M + t + j];
                    s = fma(-fma((C)(t - fr * hop), (c1 - c0) * inv_hop, c0), gb[t], s);
                }
                g_zi[(size_t)b * M + j] = s;
            }
        }
    }
    const HatSpan span(f, F, hop, T);
    C acc = 0, accg = 0;
    for (int64_t c0 = span.lo; c0 < span.hi; c0 += 256) {
        const int64_t t = c0 + tid;
        C p = 0, e = 0;
        if (t < span.hi) {
            const C gv = gb[t];
            e = (C)xb[t];
            if (!span.rising(t) && (!ZI || gxb))   // g_ex[t] is written by the frame whose falling edge holds t
                gxb[t] = (IO)(gv * gain_at(gnb, (int)t, F, hop, inv_hop));
            p = span.weight<C>(t) * gv;
        }
        ps[tid] = p;
        accg = fma(p, e, accg);
        for (int u = tid; u < 256 + 64; u += 256) {   // ys[u] = y[c0 - 64 + u]
            const int64_t ty = c0 - 64 + u;
            C v = 0;
            if (ty >= 0) {
                if (ty < T) v = (C)yb[ty];
            } else if (zb && -1 - ty < M) {
                v = zb[-1 - ty];
            }
            ys[u] = v;
        }
        __syncthreads();
        if (k < M) {
            const C* pw = ps + 64 * wv;
            const C* yk = ys + 64 * wv + 63 - k;   // yk[s] = y[c0 + 64 wv + s - 1 - k]
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
    if ((!ZI || g_a) && tid < M)
        g_a[((size_t)b * F + f) * M + tid] = (IO)(-(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]));
    if ((!ZI || g_gain) && tid == 64) g_gain[(size_t)b * F + f] = (IO)(((pgain[0] + pgain[1]) + pgain[2]) + pgain[3]);
}

// ------------------------------------------------------------------------------------------
// launchers.  The backward's workspace is the adjoint's g (B, T) of type C.
// ------------------------------------------------------------------------------------------
template <typename C>
static size_t wave_ws_bytes(int B, int T) {
    return align_up((size_t)B * (size_t)T * sizeof(C), 256);
}

template <typename C, typename IO>
static int launch_wave_fwd(const void* ex, int64_t ex_stride, const void* gain, const void* a, void* y, int64_t y_stride, int B,
                           int T, int F, int M, int hop, C* state, hipStream_t st) {
    auto* kernel = state ? lpc_any_fwd_kernel<C, IO, true> : lpc_any_fwd_kernel<C, IO, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, st, (const IO*)ex, ex_stride, (const IO*)gain, (const IO*)a,
                       (IO*)y, y_stride, T, F, M, hop, state);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

template <typename C, typename IO, bool ZI>
static int launch_wave_bwd(const void* gy, int64_t gy_stride, const void* y, int64_t y_stride, const void* ex,
                           int64_t ex_stride, const void* gain, const void* a, const C* zi, void* g_ex, int64_t g_ex_stride,
                           int64_t tail, void* g_gain, void* g_a, C* g_zi, int B, int T, int F, int M, int hop, C* g,
                           hipStream_t st) {
    hipLaunchKernelGGL((lpc_any_adj_kernel<C, IO>), dim3((unsigned)B), dim3(64), 0, st, (const IO*)gy, gy_stride, (const IO*)a,
                       g, T, F, M, hop);
    GOLF_LAUNCH_CHECK();
    if (!g_ex && !g_gain && !g_a && !g_zi) return GOLF_OK;
    hipLaunchKernelGGL((lpc_any_grad_kernel<C, IO, ZI>), dim3((unsigned)(B * F)), dim3(256), 0, st, (const C*)g, (const IO*)y,
                       y_stride, (const IO*)ex, ex_stride, (const IO*)gain, (const IO*)a, zi, (IO*)g_ex, g_ex_stride,
                       (IO*)g_gain, (IO*)g_a, g_zi, T, F, M, hop, tail);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

// the fp32 chain (declared in common.h; called from lpc_ss.hip's entry points where make_ss_plan has no plan)
size_t any_ws_bytes(int B, int T) { return wave_ws_bytes<float>(B, T); }

int launch_any_fwd(const float* ex, int64_t ex_stride, const float* gain, const float* a, float* y, int64_t y_stride, int B,
                   int T, int F, int M, int hop, float* state, hipStream_t st) {
    return launch_wave_fwd<float, float>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
}

int launch_any_bwd(const float* gy, int64_t gy_stride, const float* y, int64_t y_stride, const float* ex, int64_t ex_stride,
                   const float* gain, const float* a, float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T,
                   int F, int M, int hop, char* ws, int64_t tail, hipStream_t st) {
    if ((int64_t)B * F > INT_MAX) return fail(GOLF_EUNSUPPORTED, "ltv_allpole_bwd: B*F=%lld beyond 2^31", (long long)B * F);
    return launch_wave_bwd<float, float, false>(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, nullptr, g_ex, g_ex_stride,
                                                tail, g_gain, g_a, nullptr, B, T, F, M, hop, (float*)ws, st);
}

static int check_f64_args(const char* who, int B, int T, int F, int M, int hop, int io) {
    if (B < 1 || T < 1 || F < 1 || M < 1 || hop < 1) return fail(GOLF_EINVAL, "%s: non-positive size", who);
    if (M > 64) return fail(GOLF_EUNSUPPORTED, "%s: M=%d > 64", who, M);
    if ((int64_t)T > (int64_t)(F - 1) * hop + 1)
        return fail(GOLF_EINVAL, "%s: T=%d exceeds (F-1)*hop+1=%lld", who, T, (long long)(F - 1) * hop + 1);
    if (io != 0 && io != 1) return fail(GOLF_EINVAL, "%s: io=%d is neither 0 (fp32 tensors) nor 1 (fp64 tensors)", who, io);
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" size_t golf_ltv_allpole_f64_workspace_bytes(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return wave_ws_bytes<double>(B, T);
}

extern "C" int golf_ltv_allpole_fwd_f64(const void* ex, int64_t ex_stride, const void* gain, const void* a, void* y,
                                        int64_t y_stride, int B, int T, int F, int M, int hop, double* state, int io,
                                        void* stream) {
    const char* who = "ltv_allpole_fwd_f64";
    if (int rc = check_f64_args(who, B, T, F, M, hop, io)) return rc;
    if (!ex || !gain || !a || !y) return fail(GOLF_EINVAL, "%s: null pointer", who);
    if (ex_stride < T || y_stride < T) return fail(GOLF_EINVAL, "%s: row stride < T", who);
    hipStream_t st = (hipStream_t)stream;
    return io ? launch_wave_fwd<double, double>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st)
              : launch_wave_fwd<double, float>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
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
    const size_t need = wave_ws_bytes<double>(B, T);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255))
        return fail(GOLF_EINVAL, "%s: workspace needs %zu bytes, 256-aligned (got %zu)", who, need, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int64_t tail = g_ex ? g_ex_width - (int64_t)T : 0;
    return io ? launch_wave_bwd<double, double, true>(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, zi, g_ex, g_ex_stride,
                                                      tail, g_gain, g_a, g_zi, B, T, F, M, hop, (double*)ws, st)
              : launch_wave_bwd<double, float, true>(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, zi, g_ex, g_ex_stride,
                                                     tail, g_gain, g_a, g_zi, B, T, F, M, hop, (double*)ws, st);
}
