// f0 path search for gfx950: per-frame candidate periods -> the minimum-cost path through them (and the unvoiced state) over
// an utterance, in the manner of Praat's path finder (Boersma 1993).  Definition in include/golf_amd.h; the float64
// restatement in tests/f0_track_ref.py is the checker.  The candidates come from golf_f0_candidates_f32 (f0_yin.hip).
//
// One launch, one wave per utterance; the lane layout, the block preparation and the walk step are f0_path.h's, shared with
// the streaming kernel.  What is this kernel's own:
//   1. The backpointers of VIT_CH frames fit LDS.  A longer utterance spills every full chunk to the caller's workspace
//      (coalesced) and the backtrace loads the chunks again, last first; F <= VIT_CH needs no workspace.
//   2. End state: the min over the 8 final costs, the smaller state on ties.  The backtrace takes 64 frames at a time: lane l
//      reads the 8 backpointers of its frame (one ds_read_b64), and the walk is a scalar chain of v_readlane, shift and mask
//      with no memory access on it; lane l keeps the state of its frame and stores state and f0 = sample_rate / period of
//      the chosen slot, coalesced.
// No atomics, one fixed order: bit-reproducible, and a row does not depend on its batch.
#include "f0_path.h"

namespace golf {

constexpr int VIT_CH = 4096;      // frames whose backpointers LDS holds (a multiple of PATH_FB)
static_assert(VIT_CH % PATH_FB == 0, "a chunk is whole blocks");

static inline size_t vit_ws_bytes(int B, int F) { return F > VIT_CH ? (size_t)B * (size_t)F * 8 : 0; }

__global__ __launch_bounds__(64) void f0_viterbi_kernel(const float* __restrict__ cand_period, const float* __restrict__ cand_ap,
                                                        float* __restrict__ f0_out, int* __restrict__ state_out,
                                                        unsigned* __restrict__ ws, int F, int K, double sample_rate,
                                                        double log2_ref, double u_cost, double lag_cost, double jump_cost,
                                                        double switch_cost) {
    __shared__ PathBlock blk;
    __shared__ __attribute__((aligned(8))) unsigned char bpS[VIT_CH * 8];   // backpointers of the chunk

    const int lane = threadIdx.x, to = lane >> 3, from = lane & 7;
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * F;
    const float* cp = cand_period + row * K;
    const float* ca = cand_ap + row * K;
    const bool spill = F > VIT_CH;
    unsigned* wsr = spill ? ws + row * 2 : nullptr;   // 8 bytes a frame

    double c_from = 0.0;   // C[f - 1, from]
    for (int fb = 0; fb < F; fb += PATH_FB) {
        const int nf = min(PATH_FB, F - fb);
        path_prepare(blk, cp + (int64_t)fb * K, ca + (int64_t)fb * K, nf, K, fb > 0, fb == 0, log2_ref, u_cost, lag_cost,
                     jump_cost, switch_cost);

        int fr = 0;
        if (fb == 0) {   // C[0, s] = local cost
            c_from = blk.loc[from];
            fr = 1;
        }
        double t_next = blk.t[min(fr, nf - 1) * 64 + lane], l_next = blk.loc[min(fr, nf - 1) * 8 + to];
        for (; fr < nf; ++fr) {
            const double t = t_next, l = l_next;
            const int nx = min(fr + 1, nf - 1);   // the next frame's costs are on their way while this one reduces
            t_next = blk.t[nx * 64 + lane], l_next = blk.loc[nx * 8 + to];
            const int i = path_step(c_from, t, l, to, from);
            if (from == 0) bpS[((fb + fr) & (VIT_CH - 1)) * 8 + to] = (unsigned char)i;
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
    int s = __builtin_amdgcn_readfirstlane(path_argmin8(c_from, path_min8(c_from), to));

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
    if (B < 1 || F < 1 || K < 1 || K > PATH_MAX_K) return 0;
    return vit_ws_bytes(B, F);
}

int golf_f0_viterbi_f32(const float* cand_period, const float* cand_ap, float* f0, int* state, void* ws, size_t ws_bytes,
                        int B, int F, int K, double sample_rate, double lag_ref, double unvoiced_cost, double lag_cost,
                        double jump_cost, double switch_cost, void* stream) {
    if (!cand_period || !cand_ap || (!f0 && !state))
        return fail(GOLF_EINVAL, "f0_viterbi: null pointer (cand_period=%p cand_ap=%p f0=%p state=%p; at least one output)",
                    cand_period, cand_ap, f0, state);
    if (B < 1 || F < 1) return fail(GOLF_EINVAL, "f0_viterbi: bad size (B=%d F=%d)", B, F);
    if (const int rc = path_refuse("f0_viterbi", K, sample_rate, lag_ref)) return rc;
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
