// Shared host-side helpers for libgolf_hip.so (gfx950 only; no other backend exists).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "golf_amd.h"
#include "lpc_ss_plan.h"   // SsPlan, make_ss_plan, ceil_div, align_up: HIP-free, shared with the host tests
#include "stream_plan.h"   // RingPlan, ring_plan, frame_position_check: HIP-free, shared with the host tests

namespace golf {

char* err_buf();
int fail(int code, const char* fmt, ...);

// Every launch goes through this: returns the hipError_t (>0) of a failed launch.
#define GOLF_LAUNCH_CHECK()                                                              \
    do {                                                                                 \
        hipError_t e__ = hipGetLastError();                                              \
        if (e__ != hipSuccess) {                                                         \
            snprintf(golf::err_buf(), 512, "%s:%d launch failed: %s", __FILE__, __LINE__, \
                     hipGetErrorString(e__));                                            \
            return (int)e__;                                                             \
        }                                                                                \
    } while (0)

// ---- sample-wise filter for the shapes without a plan (lpc_any.hip): any 1 <= M <= 64, hop >= 1, F >= 1 ---------------------
size_t any_ws_bytes(int B, int T);   // the backward's workspace: g (B, T)
// state == nullptr: y[<0] = 0; else state (B, M) in and out (golf_ltv_allpole_fwd_state_f32)
int launch_any_fwd(const float* ex, int64_t ex_stride, const float* gain, const float* a, float* y, int64_t y_stride, int B,
                   int T, int F, int M, int hop, float* state, hipStream_t st);
// tail: g_ex[b][T .. T + tail) is zeroed (GOLF_SS_ZERO_TAIL)
int launch_any_bwd(const float* gy, int64_t gy_stride, const float* y, int64_t y_stride, const float* ex, int64_t ex_stride,
                   const float* gain, const float* a, float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T,
                   int F, int M, int hop, char* ws, int64_t tail, hipStream_t st);

// ---- frame-wise filter for the shapes the ring chain does not serve (lpc_ff_any.hip): any 1 <= M <= 64, hop >= 1, W >= 1 ----
// rev == false: x = ex (B rows of Tx, stride x_stride), wf <- y_f;  rev == true: x = g_q (Tx = Ty), wf <- u_f.  wf (B, nfr, W)
int launch_ff_any_frames(bool rev, const float* x, int64_t x_stride, const float* gain, const float* a, const float* window,
                         float* wf, int B, int Tx, int F, int M, int hop, int W, int nfr, hipStream_t st);
// g_a (B, F, M) fully written (zeros for the frames >= nfr) from u_f and y_f (B, nfr, W)
int launch_ff_any_grad_a(const float* uf, const float* yf, float* g_a, int B, int F, int M, int W, int nfr, hipStream_t st);

}  // namespace golf
