// Streaming f0 path search for gfx950: the recursion of f0_viterbi.hip with its costs carried from call to call, and every
// frame decided a fixed number of frames late.  Definition in include/golf_amd.h; the float64 restatement in
// tests/f0_stream_ref.py is the checker.
//
// One launch, one wave per row; the lane layout, the block preparation and the walk step are f0_path.h's, shared with the
// one-shot kernel.  What is this kernel's own:
//   1. The forward walk runs the shared step block by block, so C[f, .] has the one-shot's bits whatever the cuts.
//      C[f_done - 1, .], the logs and the presence flags of frame f_done - 1 come from the carry and those of the call's
//      last frame go back to it.  Beside the chain, not on it: the backpointers (a byte per (frame, state)) and
//      e(f) = argmin_s C[f, s] (a byte per frame) go to two LDS rings indexed by the frame number.
//   2. After every chunk of VS_CH frames the frames that became final are decided, 64 at a time, a lane each: lane g starts
//      from e(h), h = min(g + lag, the last frame consumed), and follows the backpointers from h down to g + 1: at most
//      `lag` LDS reads, whatever the data holds (the state is masked to 3 bits before it indexes).  The rings hold
//      VS_RING = 2048 frames >= lag + VS_CH, so no frame that is still needed is overwritten.
//   3. f0 of a decided frame is sample_rate / period of its slot: the period is read from this call's candidates or, for a
//      frame of an earlier call, from the carry, which keeps the candidate periods of the last `lag` frames.
// Carry of one row (golf_f0_viterbi_stream_state_bytes = B (192 + 40 lag)):
//      [0, 64)     C[n - 1, 0..7]            float64         n = frames consumed so far
//      [64, 128)   log2 period[n - 1, 0..7]  float64
//      [128, 160)  present[n - 1, 0..7]      int32           (160 .. 191 unused)
//      [192, 192 + 8 lag)                    backpointers of frame f at slot f mod lag, 8 bytes a frame
//      [192 + 8 lag, 192 + 40 lag)           candidate periods of frame f at slot f mod lag, 8 floats a frame
// A call with f_done == 0 reads none of it.  No atomics, one fixed order: bit-reproducible, and a row does not depend on its
// batch or on how the frames were cut into calls.
#include "f0_path.h"

namespace golf {

constexpr int VS_MAX_LAG = 1024;
constexpr int VS_CH = 1024;        // frames walked between two rounds of decisions (a multiple of PATH_FB)
constexpr int VS_RING = 2048;      // frames the LDS rings hold (a power of two)
constexpr int VS_HEAD = 192;       // bytes of a row's carry before its two rings
static_assert(VS_CH % PATH_FB == 0, "a chunk is whole blocks");
static_assert((VS_RING & (VS_RING - 1)) == 0 && VS_RING >= VS_MAX_LAG + VS_CH, "the rings hold the lag and a chunk");

static inline size_t vs_row_bytes(int lag) { return (size_t)VS_HEAD + (size_t)40 * (size_t)lag; }
static inline bool vs_sizes_ok(int B, int K, int lag) {
    return B >= 1 && K >= 1 && K <= PATH_MAX_K && lag >= 0 && lag <= VS_MAX_LAG;
}

__global__ __launch_bounds__(64) void f0_viterbi_stream_kernel(const float* __restrict__ cand_period,
                                                               const float* __restrict__ cand_ap, float* __restrict__ f0_out,
                                                               int* __restrict__ state_out, int64_t out_stride,
                                                               char* __restrict__ carry, int64_t row_bytes, int nf, int K, int L,
                                                               int f_done, int flush, double sample_rate, double log2_ref,
                                                               double u_cost, double lag_cost, double jump_cost,
                                                               double switch_cost) {
    __shared__ PathBlock blk;
    __shared__ __attribute__((aligned(8))) unsigned char bpS[VS_RING * 8];   // backpointers of frame f at f mod VS_RING
    __shared__ unsigned char eS[VS_RING];           // e(f) at f mod VS_RING

    const int lane = threadIdx.x, to = lane >> 3, from = lane & 7;
    const int b = blockIdx.x;
    const int n = f_done + nf;                      // frames consumed after this call (< 2^31: the host checked)
    const int Lr = max(L, 1);                       // ring indices are reduced modulo this; with L == 0 no ring slot is touched
    const float* cp = cand_period + (int64_t)b * nf * K;
    const float* ca = cand_ap + (int64_t)b * nf * K;
    char* cr = carry + (int64_t)b * row_bytes;
    double* cC = (double*)cr;
    double* cLp = (double*)(cr + 64);
    int* cPr = (int*)(cr + 128);
    uint2* cBp = (uint2*)(cr + VS_HEAD);
    float* cPer = (float*)(cr + VS_HEAD + (int64_t)8 * L);

    int dec = max(f_done - L, 0);                   // frames decided before this call
    const int out0 = dec;                           // the frame of column 0
    double c_from = 0.0;                            // C[f - 1, from]
    if (f_done > 0) {
        c_from = cC[from];
        if (lane < 8) {
            blk.lp[lane] = cLp[lane];
            blk.pr[lane] = cPr[lane] != 0;
        }
        for (int g = dec + lane; g < f_done; g += 64) ((uint2*)bpS)[g & (VS_RING - 1)] = cBp[g % Lr];
        const int e = path_argmin8(c_from, path_min8(c_from), to);   // e(f_done - 1): a flush without frames ends there
        if (lane == 0) eS[(f_done - 1) & (VS_RING - 1)] = (unsigned char)e;
    }

    int last_nb = 0;                                // frames of the call's last block
    for (int n0 = f_done;;) {
        const int n1 = n - n0 > VS_CH ? n0 + VS_CH : n;   // the chunk is frames [n0, n1)
        for (int fb = n0; fb < n1; fb += PATH_FB) {
            const int nb = min(PATH_FB, n1 - fb);
            last_nb = nb;
            // row 0 of the call's first block came from the carry; every block but the call's last is full
            path_prepare(blk, cp + (int64_t)(fb - f_done) * K, ca + (int64_t)(fb - f_done) * K, nb, K, fb > f_done, fb == 0,
                         log2_ref, u_cost, lag_cost, jump_cost, switch_cost);

            int fr = 0;
            if (fb == 0) {   // C[0, s] = local cost; frame 0 has no predecessor: its backpointers are never followed
                c_from = blk.loc[from];
                const int e = path_argmin8(c_from, path_min8(c_from), to);
                if (lane < 8) bpS[lane] = 0;
                if (lane == 0) eS[0] = (unsigned char)e;
                fr = 1;
            }
            double t_next = blk.t[min(fr, nb - 1) * 64 + lane], l_next = blk.loc[min(fr, nb - 1) * 8 + to];
            for (; fr < nb; ++fr) {
                const double t = t_next, l = l_next;
                const int nx = min(fr + 1, nb - 1);   // the next frame's costs are on their way while this one reduces
                t_next = blk.t[nx * 64 + lane], l_next = blk.loc[nx * 8 + to];
                const int i = path_step(c_from, t, l, to, from);
                const int slot = (fb + fr) & (VS_RING - 1);
                if (from == 0) bpS[slot * 8 + to] = (unsigned char)i;
                const int e = path_argmin8(c_from, path_min8(c_from), to);   // beside the chain: nothing below waits for it
                if (lane == 0) eS[slot] = (unsigned char)e;
            }
        }
        wave_lds_fence();

        // the frames that are final now: [dec, hi), seen from h = min(g + L, n1 - 1)
        const int hi = (n1 == n && flush) ? n : max(n1 - L, 0);
        const int top = n1 - 1;
        for (int g0 = dec; g0 < hi; g0 += 64) {
            const int g = g0 + lane;
            if (g < hi) {
                const int h = top - g > L ? g + L : top;
                int s = eS[h & (VS_RING - 1)] & 7;
                for (int k = h; k > g; --k) s = bpS[(k & (VS_RING - 1)) * 8 + s] & 7;   // h - g <= L steps
                if (s > K) s = 0;   // never on finite costs: an absent state costs +inf and state 0 does not
                const int64_t at = (int64_t)b * out_stride + (g - out0);
                if (state_out) state_out[at] = s;
                if (f0_out) {
                    float v = 0.f;
                    if (s > 0) {
                        const float p = g >= f_done ? cp[(int64_t)(g - f_done) * K + (s - 1)] : cPer[(g % Lr) * 8 + (s - 1)];
                        v = (float)(sample_rate / (double)p);
                    }
                    f0_out[at] = v;
                }
            }
        }
        dec = max(dec, hi);
        if (n1 >= n) break;
        n0 = n1;
        wave_lds_fence();   // the next chunk overwrites ring slots the lanes have just read
    }

    if (nf > 0) {   // what the next call needs; every read of the carry above has been consumed by a store before these
        __threadfence();
        if (lane < 8) {   // lanes 0 .. 7 hold C[n - 1, from]
            cC[lane] = c_from;
            cLp[lane] = blk.lp[last_nb * 8 + lane];
            cPr[lane] = blk.pr[last_nb * 8 + lane];
        }
        const int lo = max(n - L, f_done);   // n - L does not overflow: n >= 0, L <= 1024
        for (int g = lo + lane; g < n; g += 64) cBp[g % Lr] = ((const uint2*)bpS)[g & (VS_RING - 1)];
        for (int e = lane; e < (n - lo) * 8; e += 64) {
            const int g = lo + (e >> 3), k = e & 7;
            cPer[(g % Lr) * 8 + k] = k < K ? cp[(int64_t)(g - f_done) * K + k] : 0.f;
        }
    }
}

}  // namespace golf

using namespace golf;

extern "C" {

size_t golf_f0_viterbi_stream_state_bytes(int B, int K, int lag) {
    if (!vs_sizes_ok(B, K, lag)) return 0;
    return (size_t)B * vs_row_bytes(lag);
}

int golf_f0_viterbi_stream_f32(const float* cand_period, const float* cand_ap, float* f0, int* state, int64_t out_stride,
                               void* carry, size_t carry_bytes, int B, int nf, int K, int lag, int64_t f_done, int flush,
                               double sample_rate, double lag_ref, double unvoiced_cost, double lag_cost, double jump_cost,
                               double switch_cost, void* stream) {
    if (B < 1 || nf < 0 || f_done < 0)
        return fail(GOLF_EINVAL, "f0_viterbi_stream: bad size (B=%d nf=%d f_done=%lld)", B, nf, (long long)f_done);
    if (nf > 0 && (!cand_period || !cand_ap))
        return fail(GOLF_EINVAL, "f0_viterbi_stream: null pointer (cand_period=%p cand_ap=%p)", cand_period, cand_ap);
    if (nf == 0 && !flush) return fail(GOLF_EINVAL, "f0_viterbi_stream: nf=0 frames without flush: nothing to do");
    if (nf == 0 && f_done == 0) return fail(GOLF_EINVAL, "f0_viterbi_stream: flush of an utterance of no frames (nf=0 f_done=0)");
    if (const int rc = path_refuse("f0_viterbi_stream", K, sample_rate, lag_ref)) return rc;
    if (lag < 0 || lag > VS_MAX_LAG) return fail(GOLF_EUNSUPPORTED, "f0_viterbi_stream: lag=%d frames, must be 0..%d", lag, VS_MAX_LAG);
    if (f_done + nf >= ((int64_t)1 << 31) || (int64_t)B * nf >= ((int64_t)1 << 31))
        return fail(GOLF_EUNSUPPORTED, "f0_viterbi_stream: f_done + nf = %lld and B*nf = %lld frames, must be < 2^31",
                    (long long)(f_done + nf), (long long)B * nf);
    const size_t need = (size_t)B * vs_row_bytes(lag);
    if (!carry || carry_bytes < need || ((uintptr_t)carry & 7))
        return fail(GOLF_EINVAL, "f0_viterbi_stream: carry %p of %zu bytes, need %zu, 8-byte aligned "
                    "(golf_f0_viterbi_stream_state_bytes)", carry, carry_bytes, need);
    const int64_t n = f_done + nf;
    const int64_t before = f_done > lag ? f_done - lag : 0;
    const int64_t after = flush ? n : (n > lag ? n - lag : 0);
    const int64_t n_out = after - before;
    if (n_out > 0 && !f0 && !state)
        return fail(GOLF_EINVAL, "f0_viterbi_stream: null pointer (f0=%p state=%p; at least one output)", f0, state);
    if (out_stride < n_out)
        return fail(GOLF_EINVAL, "f0_viterbi_stream: out_stride=%lld < %lld frames written", (long long)out_stride, (long long)n_out);
    if (nf == 0 && n_out == 0) return GOLF_OK;   // a flush at lag 0: every frame was decided when it came
    hipLaunchKernelGGL(f0_viterbi_stream_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cand_period, cand_ap, f0,
                       state, out_stride, (char*)carry, (int64_t)vs_row_bytes(lag), nf, K, lag, (int)f_done, flush ? 1 : 0,
                       sample_rate, log2(lag_ref), unvoiced_cost, lag_cost, jump_cost, switch_cost);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // extern "C"
