// The f0 path recursion for gfx950, once: what f0_viterbi.hip (one launch per utterance) and f0_viterbi_stream.hip (its
// fixed-lag twin, carried from call to call) both run, so that C[f, .] has the same bits in both whatever the cuts.  Each
// kernel keeps its own control flow, its backpointer storage and its backtrace; the leaves below are shared.
//
// One wave per utterance.  With K <= PATH_MAX_K candidates there are at most 8 states (0 = unvoiced, k + 1 = slot k), and the
// 64 lanes are the 8 x 8 (to, from) pairs: lane = 8 to + from.  Everything is float64.
//   1. path_prepare: a block of PATH_FB frames is prepared by all lanes: lane l takes (frame, state) pairs 64 at a time and
//      writes log2 of the period, the local cost and the presence flag to LDS; then, a frame at a time, lane (to, from) writes
//      the transition cost t(from, to) of that frame, +inf where either end is absent.  No difference of infinities is formed:
//      the logs are subtracted only where both slots are present.  Nothing here depends on the path so far.
//   2. path_step, the walk: per frame the kernel reads t and the local cost from LDS (addresses known ahead, so the reads of
//      later frames are in flight while the chain waits); the step is one add, the min over `from` as three exchanges inside
//      the group of 8 lanes (DPP quad permutes and the half-row mirror: no LDS), one add of the local cost, and one
//      ds_bpermute that hands lane (to, from) the new cost of state `from` for the next frame.  The backpointer is the lowest
//      `from` whose cost equals the min (a ballot and a bit scan, so the smaller `from` wins a tie); it is not on the chain,
//      and the kernel stores it beside the chain, a byte per (frame, state).
#pragma once
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int PATH_MAX_K = 7;
constexpr int PATH_FB = 32;   // frames prepared per block

// what both entry points refuse, with the caller's name in front
static inline int path_refuse(const char* who, int K, double sample_rate, double lag_ref) {
    if (!(sample_rate > 0.0) || !(lag_ref > 0.0))
        return fail(GOLF_EINVAL, "%s: sample_rate=%g and lag_ref=%g must be positive", who, sample_rate, lag_ref);
    if (K < 1 || K > PATH_MAX_K) return fail(GOLF_EUNSUPPORTED, "%s: K=%d candidates, must be 1..%d", who, K, PATH_MAX_K);
    return GOLF_OK;
}

template <int CTRL>
__device__ __forceinline__ double path_dppd(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
constexpr int PATH_DPP_HALF_MIRROR = 0x141;   // row_half_mirror: lane i of a group of 8 reads lane 7 - i

// min over the 8 lanes of a group; every lane of the group ends with it
__device__ __forceinline__ double path_min8(double v) {
    v = fmin(v, path_dppd<DPP_XOR1>(v));
    v = fmin(v, path_dppd<DPP_XOR2>(v));
    return fmin(v, path_dppd<PATH_DPP_HALF_MIRROR>(v));
}
// the lowest lane of this lane's group of 8 whose value equals the group's min: the smaller index wins a tie.  A ballot and
// a bit scan beside the dependent chain, not on it.
__device__ __forceinline__ int path_argmin8(double v, double vmin, int to) {
    const unsigned long long m = __ballot(v == vmin);
    return (__ffs((int)((m >> (to << 3)) & 0xff)) - 1) & 7;
}

// a prepared block in LDS: each kernel declares one
struct PathBlock {
    double t[PATH_FB * 64];          // t(from, to) of the block's frames
    double lp[(PATH_FB + 1) * 8];    // log2 period; row 0 is the frame before the block
    double loc[PATH_FB * 8];         // local cost, +inf for an absent state
    int pr[(PATH_FB + 1) * 8];       // 1 = present
};

// Prepares the block's `nb` frames from their candidates (cp, ca: K a frame, the block's first frame first).  `roll`: the last
// frame of a full block before this one becomes row 0 (otherwise the caller has filled row 0, or `first`); `first`: the block
// begins the utterance, so its frame 0 has no predecessor and no transition costs.  Fenced on both sides.
__device__ __forceinline__ void path_prepare(PathBlock& blk, const float* __restrict__ cp, const float* __restrict__ ca, int nb,
                                             int K, bool roll, bool first, double log2_ref, double u_cost, double lag_cost,
                                             double jump_cost, double switch_cost) {
    const int lane = threadIdx.x, to = lane >> 3, from = lane & 7;
    if (roll && lane < 8) {
        blk.lp[lane] = blk.lp[PATH_FB * 8 + lane];
        blk.pr[lane] = blk.pr[PATH_FB * 8 + lane];
    }
    wave_lds_fence();
    for (int e = lane; e < nb * 8; e += 64) {
        const int fr = e >> 3, s = e & 7;
        double lp = 0.0, loc = u_cost;
        int pr = 1;
        if (s > 0) {
            pr = 0, loc = INFINITY;
            if (s <= K) {
                const int at = fr * K + (s - 1);
                const float p = cp[at], a = ca[at];
                if (p > 0.f && a < INFINITY) {   // a < inf is false for NaN and for +inf
                    pr = 1;
                    lp = log2((double)p);
                    loc = fmax((double)a, 0.0) + lag_cost * (lp - log2_ref);
                }
            }
        }
        blk.lp[(fr + 1) * 8 + s] = lp, blk.loc[fr * 8 + s] = loc, blk.pr[(fr + 1) * 8 + s] = pr;
    }
    wave_lds_fence();
#pragma unroll 4
    for (int fr = (first ? 1 : 0); fr < nb; ++fr) {
        double t = INFINITY;
        if (blk.pr[(fr + 1) * 8 + to] && blk.pr[fr * 8 + from]) {
            if (to == 0 || from == 0)
                t = (to == 0 && from == 0) ? 0.0 : switch_cost;
            else
                t = jump_cost * fabs(blk.lp[(fr + 1) * 8 + to] - blk.lp[fr * 8 + from]);
        }
        blk.t[fr * 64 + lane] = t;
    }
    wave_lds_fence();
}

// One frame of the walk in lane (to, from): c_from holds C[f - 1, from] and leaves with C[f, from]; t and l are the frame's
// t(from, to) and local cost of `to`.  Returns the backpointer of `to`, the same in the 8 lanes of its group.
__device__ __forceinline__ int path_step(double& c_from, double t, double l, int to, int from) {
    const double v = c_from + t;
    const double vmin = path_min8(v);
    const double c_to = vmin + l;
    const int i = path_argmin8(v, vmin, to);
    c_from = __shfl(c_to, from << 3);
    return i;
}

}  // namespace golf
