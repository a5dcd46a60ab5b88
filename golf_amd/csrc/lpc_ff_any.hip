// Frame-wise LTI all-pole filter (include/golf_amd.h, a-4) for the shapes WITHOUT a ring: any 1 <= M <= 64, any hop >= 1, any
// window length W >= 2*hop (lpc_ff.hip needs a ring width in {8,16,24,32,40} with M <= width - 2 and width <= hop, and its
// adjoint a window that is a multiple of that width).  fp32, 64-bit row addressing; gfx950 only.
//
// Frames kernel: one WAVE per (utterance, frame), one LANE per tap, the recursion in SCATTER (transposed direct) form as in
// lpc_any.hip -- lane k holds the partial sum destined for the frame position p + k, p the position being computed:
//     y[p]  = acc_0                                   (v_readfirstlane)
//     acc_k = fma(-a[k], y[p], acc_{k+1})             (one wave_shl:1 DPP move + one FMA)
// A frame's coefficients are constant and its state starts at zero, so there is no frame switch, no per-lane time and no run
// splitting; and because lane k IS position p + k, the 64 inputs of a block are added to the 64 partial sums in ONE
// instruction when the block starts (x[p] then rides down to lane 0 with the sum it belongs to; lanes >= M hold zero
// coefficients and only pass it on, exactly).  The output enters lane s of a block register by v_writelane.  That leaves
// four VALU instructions per sample (lpc_any.hip: nine), none of them on memory; input and output move 64 samples at a time,
// coalesced, the next block's loads in flight under the current block's recursion.
//   REV = false  forward:  input ex * up(gain) at t = f*hop - W/2 + k (0 outside [0, Tx)), k ascending, output y_f[k]
//   REV = true   adjoint:  input window[k] * g_q[f*hop - W/2 + k], k DEscending, no gain, output u_f[k]
// Both write the unwindowed frame into the (B, nfr, W) layout that ff_ola_kernel / ff_bwd_ola_kernel read.
//
// Gradient kernel: g_a[b,f,i] = -sum_k u_f[k] * y_f[k-1-i], one workgroup per (utterance, coefficient frame), the rows staged
// 256 positions at a time (LDS use independent of W), every sum in a fixed order: no atomics, bit-reproducible.
#include "common.h"
#include "device_common.h"

#include <climits>

namespace golf {

// v_writelane_b32: lane `lane` (wave-uniform) of `old` takes the wave-uniform `value`.  (The intrinsic has no clang builtin.)
__device__ int wave_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

template <bool REV>
__global__ __launch_bounds__(64) void ff_any_frames_kernel(const float* __restrict__ x, int64_t x_stride,
                                                           const float* __restrict__ gain, const float* __restrict__ a,
                                                           const float* __restrict__ window, float* __restrict__ wf, int Tx,
                                                           int F, int M, int hop, int W, int nfr) {
    const int q = blockIdx.x;                 // (b, f)
    const int b = q / nfr, f = q - b * nfr;
    const int k = threadIdx.x;
    const float* xb = x + (size_t)b * x_stride;
    const float* gb = gain + (size_t)b * F;
    float* out = wf + (size_t)q * W;
    const float ncf = k < M ? -a[((size_t)b * F + f) * M + k] : 0.f;
    const float inv_hop = 1.0f / (float)hop;
    const int t00 = f * hop - W / 2;          // global sample of frame position 0

    // the 64 inputs of a block and what up(gain) (forward) or the window (adjoint) needs for them, loaded one block ahead;
    // the arithmetic waits for the block's turn.  Lane l of block k0 is recursion step k0 + l.
    float xr, c0, c1, cn;
    auto fetch = [&](int k0) {
        const int s = k0 + k;
        const int p = REV ? W - 1 - s : s;    // frame position of that step
        const int t = t00 + p;
        xr = c0 = c1 = cn = 0.f;
        if (s < W && t >= 0 && t < Tx) {
            xr = xb[t];
            if (REV) {
                c0 = window[p];
            } else {
                int fg = t / hop;
                if (fg > F - 2) fg = F - 2;
                c0 = gb[fg];
                c1 = gb[fg + 1];
                cn = (float)(t - fg * hop);
            }
        }
    };

    float acc = 0.f;   // lane l: the partial sum of frame position (current step) + l
    float blk = 0.f;   // lane s: the output of step k0 + s
    auto step = [&](int s) {
        const int sy = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc));
        blk = __builtin_bit_cast(float, wave_writelane(sy, s, __builtin_bit_cast(int, blk)));
        const float sh = __builtin_bit_cast(
            float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), DPP_WAVE_SHL1, 0xF, 0xF, true));
        acc = fmaf(ncf, __builtin_bit_cast(float, sy), sh);
    };

    fetch(0);
    for (int k0 = 0; k0 < W; k0 += 64) {
        acc += REV ? xr * c0 : xr * fmaf(cn, (c1 - c0) * inv_hop, c0);
        fetch(k0 + 64);
        const int ns = W - k0 < 64 ? W - k0 : 64;
        int s = 0;
        for (; s + 8 <= ns; s += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) step(s + u);
        }
        for (; s < ns; ++s) step(s);
        if (k < ns) out[REV ? W - 1 - k0 - k : k0 + k] = blk;
    }
}

// g_a[b,f,i] = -sum_k u_f[k] * y_f[k-1-i] for ALL F coefficient frames (zeros for f >= nfr).  256 positions at a time are
// staged in LDS: u, and y with 64 positions of history in front; wave v takes the v-th 64 of them, lane i the tap i.
__global__ __launch_bounds__(256) void ff_any_grad_a_kernel(const float* __restrict__ uf, const float* __restrict__ yf,
                                                            float* __restrict__ g_a, int F, int M, int W, int nfr) {
    __shared__ __attribute__((aligned(16))) float us[256];
    __shared__ float ys[256 + 64], part[4][64];
    const int f = (int)(blockIdx.x % (unsigned)F), b = (int)(blockIdx.x / (unsigned)F);
    const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), i = tid & 63;
    float* o = g_a + ((size_t)b * F + f) * M;
    if (f >= nfr) {   // block-uniform
        if (tid < M) o[tid] = 0.f;
        return;
    }
    const size_t base = ((size_t)b * nfr + f) * W;
    const float* ub = uf + base;
    const float* yb = yf + base;
    float acc = 0.f;
    for (int c0 = 0; c0 < W; c0 += 256) {
        const int kk = c0 + tid;
        us[tid] = kk < W ? ub[kk] : 0.f;
        for (int u = tid; u < 256 + 64; u += 256) {   // ys[u] = y_f[c0 - 64 + u]
            const int ky = c0 - 64 + u;
            ys[u] = (ky >= 0 && ky < W) ? yb[ky] : 0.f;
        }
        __syncthreads();
        if (i < M && c0 + 64 * wv < W) {
            const float* pw = us + 64 * wv;
            const float* yk = ys + 64 * wv + 63 - i;   // yk[s] = y_f[c0 + 64 wv + s - 1 - i]
#pragma unroll 8
            for (int s = 0; s < 64; ++s) acc = fmaf(pw[s], yk[s], acc);
        }
        __syncthreads();
    }
    part[wv][i] = acc;
    __syncthreads();
    if (tid < M) o[tid] = -(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
}

// ------------------------------------------------------------------------------------------
// launchers (declared in common.h; called from lpc_ff.hip's entry points where the ring chain does not serve the shape)
// ------------------------------------------------------------------------------------------
int launch_ff_any_frames(bool rev, const float* x, int64_t x_stride, const float* gain, const float* a, const float* window,
                         float* wf, int B, int Tx, int F, int M, int hop, int W, int nfr, hipStream_t st) {
    const unsigned nq = (unsigned)((int64_t)B * nfr);
    if (rev)
        hipLaunchKernelGGL(ff_any_frames_kernel<true>, dim3(nq), dim3(64), 0, st, x, x_stride, gain, a, window, wf, Tx, F, M,
                           hop, W, nfr);
    else
        hipLaunchKernelGGL(ff_any_frames_kernel<false>, dim3(nq), dim3(64), 0, st, x, x_stride, gain, a, window, wf, Tx, F, M,
                           hop, W, nfr);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

int launch_ff_any_grad_a(const float* uf, const float* yf, float* g_a, int B, int F, int M, int W, int nfr, hipStream_t st) {
    hipLaunchKernelGGL(ff_any_grad_a_kernel, dim3((unsigned)((int64_t)B * F)), dim3(256), 0, st, uf, yf, g_a, F, M, W, nfr);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf
