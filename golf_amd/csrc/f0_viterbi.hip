// f0 path search for gfx950: per-frame candidate periods -> the minimum-cost path through them (and the unvoiced state) over
// an utterance, in the manner of Praat's path finder (Boersma 1993).  Definition in include/golf_amd.h; the float64
// restatement in tests/f0_track_ref.py is the checker.  The candidates come from golf_f0_candidates_f32 (f0_yin.hip).
//
// One launch, one wave per utterance.  With K <= 7 candidates there are at most 8 states (0 = unvoiced, k + 1 = slot k), and
// the 64 lanes are the 8 x 8 (to, from) pairs: lane = 8 to + from.  Everything is float64.
//   1. A block of VIT_FB frames is prepared by all lanes: lane l takes (frame, state) pairs 64 at a time and writes log2 of
//      the period, the local cost and the presence flag to LDS; then, a frame at a time, lane (to, from) writes the
//      transition cost t(from, to) of that frame, +inf where either end is absent.  No difference of infinities is formed:
//      the logs are subtracted only where both slots are present.  Nothing here depends on the path so far.
//   2. The walk: per frame one LDS read of t and one of the local cost (addresses known ahead, so the reads of later frames
//      are in flight while the chain waits), one add, the min over `from` as three exchanges inside the group of 8 lanes
//      (DPP quad permutes and the half-row mirror: no LDS), one add of the local cost, and one ds_bpermute that hands lane (to, from) the new cost of state `from`
//      for the next frame.  The backpointer is the lowest `from` whose cost equals the min (a ballot and a bit scan, so the
//      smaller `from` wins a tie); it is not on the chain and goes to LDS beside it, a byte per (frame, state).
//   3. The backpointers of VIT_CH frames fit LDS.  A longer utterance spills every full chunk to the caller's workspace
//      (coalesced) and the backtrace loads the chunks again, last first; F <= VIT_CH needs no workspace.
//   4. End state: the min over the 8 final costs, the smaller state on ties.  The backtrace takes 64 frames at a time: lane l
//      reads the 8 backpointers of its frame (one ds_read_b64), and the walk is a scalar chain of v_readlane, shift and mask
//      with no memory access on it; lane l keeps the state of its frame and stores state and f0 = sample_rate / period of
//      the chosen slot, coalesced.
// No atomics, one fixed order: bit-reproducible, and a row does not depend on its batch.
#include "common.h"
#include "device_common.h"

namespace golf {

constexpr int VIT_MAX_K = 7;
constexpr int VIT_FB = 32;        // frames prepared per block
constexpr int VIT_CH = 4096;      // frames whose backpointers LDS holds (a multiple of VIT_FB)
static_assert(VIT_CH % VIT_FB == 0, "a chunk is whole blocks");

static inline size_t vit_ws_bytes(int B, int F) { return F > VIT_CH ? (size_t)B * (size_t)F * 8 : 0; }

template <int CTRL>
__device__ __forceinline__ double dppd(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
constexpr int VIT_DPP_HALF_MIRROR = 0x141;   // row_half_mirror: lane i of a group of 8 reads lane 7 - i

// min over the 8 lanes of a group; every lane of the group ends with it
__device__ __forceinline__ double vit_min8(double v) {
    v = fmin(v, dppd<DPP_XOR1>(v));
    v = fmin(v, dppd<DPP_XOR2>(v));
    return fmin(v, dppd<VIT_DPP_HALF_MIRROR>(v));
}
// the lowest lane of this lane's group of 8 whose value equals the group's min: the smaller index wins a tie.  A ballot and
// a bit scan beside the dependent chain, not on it.
__device__ __forceinline__ int vit_argmin8(double v, double vmin, int to) {
    const unsigned long long m = __ballot(v == vmin);
    return (__ffs((int)((m >> (to << 3)) & 0xff)) - 1) & 7;
}

__global__ __launch_bounds__(64) void f0_viterbi_kernel(const float* __restrict__ cand_period, const float* __restrict__ cand_ap,
                                                        float* __restrict__ f0_out, int* __restrict__ state_out,
                                                        unsigned* __restrict__ ws, int F, int K, double sample_rate,
                                                        double log2_ref, double u_cost, double lag_cost, double jump_cost,
                                                        double switch_cost) {
    __shared__ double tS[VIT_FB * 64];              // t(from, to) of the block's frames
    __shared__ double lpS[(VIT_FB + 1) * 8];        // log2 period; row 0 is the frame before the block
    __shared__ double locS[VIT_FB * 8];             // local cost, +inf for an absent state
    __shared__ int prS[(VIT_FB + 1) * 8];           // 1 = present
    __shared__ __attribute__((aligned(8))) unsigned char bpS[VIT_CH * 8];   // backpointers of the chunk

    const int lane = threadIdx.x, to = lane >> 3, from = lane & 7;
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * F;
    const float* cp = cand_period + row * K;
    const float* ca = cand_ap + row * K;
    const bool spill = F > VIT_CH;
    unsigned* wsr = spill ? ws + row * 2 : nullptr;   // 8 bytes a frame

    double c_from = 0.0;   // C[f - 1, from]
    for (int fb = 0; fb < F; fb += VIT_FB) {
        const int nf = min(VIT_FB, F - fb);
        if (fb > 0 && lane < 8) {   // the last frame of the block before becomes row 0
            lpS[lane] = lpS[VIT_FB * 8 + lane];
            prS[lane] = prS[VIT_FB * 8 + lane];
        }
        wave_lds_fence();
        for (int e = lane; e < nf * 8; e += 64) {
            const int fr = e >> 3, s = e & 7;
            double lp = 0.0, loc = u_cost;
            int pr = 1;
            if (s > 0) {
                pr = 0, loc = INFINITY;
                if (s <= K) {
                    const int64_t at = (int64_t)(fb + fr) * K + (s - 1);
                    const float p = cp[at], a = ca[at];
                    if (p > 0.f && a < INFINITY) {   // a < inf is false for NaN and for +inf
                        pr = 1;
                        lp = log2((double)p);
                        loc = fmax((double)a, 0.0) + lag_cost * (lp - log2_ref);
                    }
                }
            }
            lpS[(fr + 1) * 8 + s] = lp, locS[fr * 8 + s] = loc, prS[(fr + 1) * 8 + s] = pr;
        }
        wave_lds_fence();
#pragma unroll 4
        for (int fr = (fb == 0 ? 1 : 0); fr < nf; ++fr) {
            double t = INFINITY;
            if (prS[(fr + 1) * 8 + to] && prS[fr * 8 + from]) {
                if (to == 0 || from == 0)
                    t = (to == 0 && from == 0) ? 0.0 : switch_cost;
                else
                    t = jump_cost * fabs(lpS[(fr + 1) * 8 + to] - lpS[fr * 8 + from]);
            }
            tS[fr * 64 + lane] = t;
        }
        wave_lds_fence();

        int fr = 0;
        if (fb == 0) {   // C[0, s] = local cost
            c_from = locS[from];
            fr = 1;
        }
        double t_next = tS[min(fr, nf - 1) * 64 + lane], l_next = locS[min(fr, nf - 1) * 8 + to];
        for (; fr < nf; ++fr) {
            const double t = t_next, l = l_next;
            const int nx = min(fr + 1, nf - 1);   // the next frame's costs are on their way while this one reduces
            t_next = tS[nx * 64 + lane], l_next = locS[nx * 8 + to];
            const double v = c_from + t;
            const double vmin = vit_min8(v);
            const double c_to = vmin + l;
            const int i = vit_argmin8(v, vmin, to);
            if (from == 0) bpS[((fb + fr) & (VIT_CH - 1)) * 8 + to] = (unsigned char)i;
            c_from = __shfl(c_to, from << 3);
        }
        if (spill && ((fb + nf) % VIT_CH == 0 || fb + nf == F)) {   // the chunk that ends here goes to the workspace
            wave_lds_fence();
            const int c0 = (fb + nf - 1) / VIT_CH * VIT_CH, words = (fb + nf - c0) * 2;
            const unsigned* src = (const unsigned*)bpS;
            for (int k = lane; k < words; k += 64) wsr[(int64_t)c0 * 2 + k] = src[k];
        }
    }
    if (spill) __threadfence();   // the wave reads its own spill below

    // end state: lanes 0 .. 7 hold C[F - 1, from]
    int s = __builtin_amdgcn_readfirstlane(vit_argmin8(c_from, vit_min8(c_from), to));

    for (int c0 = (F - 1) / VIT_CH * VIT_CH; c0 >= 0; c0 -= VIT_CH) {
        const int nc = min(VIT_CH, F - c0);
        if (spill) {
            unsigned* dst = (unsigned*)bpS;
            for (int k = lane; k < nc * 2; k += 64) dst[k] = wsr[(int64_t)c0 * 2 + k];
        }
        wave_lds_fence();
        // 64 frames at a time, last first: lane l holds the 8 backpointers of frame g0 + l in a register pair, and the walk is
        // a scalar chain of (read lane k, shift by 8 s, mask) with no memory on it; lane k keeps the state of its frame
        for (int g0 = (nc - 1) / 64 * 64; g0 >= 0; g0 -= 64) {
            const int fc = g0 + lane;
            const uint2 w = fc < nc ? ((const uint2*)bpS)[fc] : make_uint2(0u, 0u);
            const int top = nc - 1 - g0;   // the group's last frame, wave-uniform
            int st = 0;
#pragma unroll
            for (int k = 63; k >= 0; --k) {
                if (k <= top) {
                    if (lane == k) st = s;
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)w.x, k);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)w.y, k);
                    s = (int)((s < 4 ? lo : hi) >> ((s & 3) << 3)) & 7;   // frame 0's bytes are not a path: s is not used after it
                }
            }
            if (fc < nc) {
                if (st > K) st = 0;   // never on finite costs: an absent state costs +inf and state 0 does not
                if (state_out) state_out[row + c0 + fc] = st;
                if (f0_out)
                    f0_out[row + c0 + fc] = st > 0 ? (float)(sample_rate / (double)cp[(int64_t)(c0 + fc) * K + (st - 1)]) : 0.f;
            }
        }
        wave_lds_fence();   // the next chunk overwrites bpS
    }
}

}  // namespace golf

using namespace golf;

extern "C" {

size_t golf_f0_viterbi_workspace_bytes(int B, int F, int K) {
    if (B < 1 || F < 1 || K < 1 || K > VIT_MAX_K) return 0;
    return vit_ws_bytes(B, F);
}

int golf_f0_viterbi_f32(const float* cand_period, const float* cand_ap, float* f0, int* state, void* ws, size_t ws_bytes,
                        int B, int F, int K, double sample_rate, double lag_ref, double unvoiced_cost, double lag_cost,
                        double jump_cost, double switch_cost, void* stream) {
    if (!cand_period || !cand_ap || (!f0 && !state))
        return fail(GOLF_EINVAL, "f0_viterbi: null pointer (cand_period=%p cand_ap=%p f0=%p state=%p; at least one output)",
                    cand_period, cand_ap, f0, state);
    if (B < 1 || F < 1) return fail(GOLF_EINVAL, "f0_viterbi: bad size (B=%d F=%d)", B, F);
    if (!(sample_rate > 0.0) || !(lag_ref > 0.0))
        return fail(GOLF_EINVAL, "f0_viterbi: sample_rate=%g and lag_ref=%g must be positive", sample_rate, lag_ref);
    if (K < 1 || K > VIT_MAX_K) return fail(GOLF_EUNSUPPORTED, "f0_viterbi: K=%d candidates, must be 1..%d", K, VIT_MAX_K);
    if ((int64_t)B * F >= ((int64_t)1 << 31))
        return fail(GOLF_EUNSUPPORTED, "f0_viterbi: B*F = %lld frames, must be < 2^31", (long long)B * F);
    const size_t need = vit_ws_bytes(B, F);
    if (need && (!ws || ws_bytes < need))
        return fail(GOLF_EINVAL, "f0_viterbi: workspace %p of %zu bytes, need %zu (golf_f0_viterbi_workspace_bytes)", ws,
                    ws_bytes, need);
    hipLaunchKernelGGL(f0_viterbi_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cand_period, cand_ap, f0, state,
                       (unsigned*)ws, F, K, sample_rate, log2(lag_ref), unvoiced_cost, lag_cost, jump_cost, switch_cost);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
