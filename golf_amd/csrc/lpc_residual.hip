// The fused residual for gfx950: (audio, gain, a) -> e = (the inverse all-pole filter of the audio) / up(gain), the decoder's
// excitation estimate that the glottal-source analysis reads.  Definition in include/golf_amd.h; the float64 restatement in
// tests/residual_ref.py is the checker.
//
// One launch, one workgroup of RES_TILE threads per (row, tile of RES_TILE samples), one output sample per thread.  The tile's
// samples and the M samples before them are staged in LDS once (a thread's taps are the RES_TILE + M window shifted by its
// lane: consecutive lanes read consecutive words, no bank conflict); the coefficient rows of the sample's two frames are read
// from global memory through the caches, where a wave's lanes share them whenever hop >= 64 -- they are not staged, so that
// hop 1, where a tile touches RES_TILE + 1 frames of M coefficients, costs no LDS.  Every output is a function of utterance
// positions alone (t, and f = t / hop, in int64): no workspace, no atomics, a fixed order of the M fused multiply-adds --
// bit-reproducible, a row does not depend on its batch, and the block-by-block twin is this kernel at another position.
// The numerator has golf_ltv_inverse_f32's bits (the same expressions in the same order); the quotient is one correctly
// rounded fp32 division (hipcc's default; nothing on the command line relaxes it).
#include "common.h"

namespace golf {

constexpr int RES_TILE = 256;
constexpr int RES_MAX_M = 64;
constexpr int RES_GRID_X = 1 << 20;   // workgroups per grid row

struct ResArgs {
    const float* x;
    int64_t x_stride, x_t0, x_end;   // the buffer holds samples [x_t0, x_end)
    const float* gain;
    const float* a;
    int64_t fr_first;                // the buffers hold frames [fr_first, fr_first + n_fr)
    float* e;
    int64_t e_stride, t_first;       // column j of e is sample t_first + j
    int64_t F;                       // the frames of the utterance when it ends with these buffers, else 2^62: no clamp
    int n_fr, n_out, tiles, G, M, hop;
};

__global__ __launch_bounds__(RES_TILE) void ltv_residual_kernel(const ResArgs p) {
    __shared__ float xs[RES_TILE + RES_MAX_M];
    const int64_t g64 = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (g64 >= p.G) return;
    const int g = (int)g64, b = g / p.tiles, tile = g - b * p.tiles;
    const int tid = threadIdx.x, M = p.M;
    const int j0 = tile * RES_TILE;   // < n_out
    const int n = p.n_out - j0 < RES_TILE ? p.n_out - j0 : RES_TILE;
    const int64_t t0 = p.t_first + j0;
    const float* xr = p.x + (int64_t)b * p.x_stride;
    for (int j = tid; j < n + M; j += RES_TILE) {
        const int64_t s = t0 - M + j;   // a sample below 0 reads 0 and is never multiplied; the entry checked the rest
        xs[j] = (s >= p.x_t0 && s < p.x_end) ? xr[s - p.x_t0] : 0.f;
    }
    __syncthreads();
    if (tid >= n) return;

    const int64_t t = t0 + tid;
    int64_t f = p.F >= 2 ? t / p.hop : 0;
    if (p.F >= 2 && f > p.F - 2) f = p.F - 2;
    const float w = (float)(t - f * p.hop) / (float)p.hop;
    const int64_t r0 = (int64_t)b * p.n_fr + (f - p.fr_first), r1 = p.F >= 2 ? r0 + 1 : r0;
    const float* pa0 = p.a + r0 * M;
    const float* pa1 = p.a + r1 * M;
    const float* xt = xs + M + tid;
    float acc = xt[0];
    const int taps = t < (int64_t)M ? (int)t : M;   // t - 1 - i >= 0
    for (int i = 0; i < taps; ++i) {
        const float cf = fmaf(w, pa1[i] - pa0[i], pa0[i]);
        acc = fmaf(cf, xt[-1 - i], acc);
    }
    const float g0 = p.gain[r0], g1 = p.gain[r1];
    p.e[(int64_t)b * p.e_stride + j0 + tid] = __fdiv_rn(acc, fmaf(w, g1 - g0, g0));
}

// the checks both entries share and the launch; every position has been brought to the stream's form
static int residual_run(const char* who, const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* gain,
                        const float* a, int64_t fr_first, int n_fr, float* e, int64_t e_stride, int B, int64_t t_first,
                        int n_out, int last, int M, int hop, void* stream) {
    const int64_t far = (int64_t)1 << 62;   // positions stay below it, so that no sum or product here or in the kernel wraps
    if (B < 1 || n_x < 1 || n_fr < 1 || n_out < 1)
        return fail(GOLF_EINVAL, "%s: bad size (B=%d n_x=%d n_fr=%d n_out=%d)", who, B, n_x, n_fr, n_out);
    if (!x || !gain || !a || !e)
        return fail(GOLF_EINVAL, "%s: null pointer (x=%p gain=%p a=%p e=%p)", who, x, gain, a, e);
    if (M < 1 || M > RES_MAX_M) return fail(GOLF_EINVAL, "%s: M=%d must be 1..%d", who, M, RES_MAX_M);
    if (hop < 1) return fail(GOLF_EINVAL, "%s: hop=%d must be >= 1", who, hop);
    if (x_stride < n_x) return fail(GOLF_EINVAL, "%s: row stride of x %lld < n_x=%d", who, (long long)x_stride, n_x);
    if (e_stride < n_out) return fail(GOLF_EINVAL, "%s: row stride of e %lld < n_out=%d", who, (long long)e_stride, n_out);
    if (x_t0 < 0 || x_t0 > far) return fail(GOLF_EINVAL, "%s: x_t0=%lld must be 0..2^62", who, (long long)x_t0);
    if (t_first < 0 || t_first > far) return fail(GOLF_EINVAL, "%s: t_first=%lld must be 0..2^62", who, (long long)t_first);
    if (fr_first < 0 || fr_first > far / hop - n_fr)
        return fail(GOLF_EINVAL, "%s: fr_first=%lld must be >= 0 with (fr_first + n_fr) hop <= 2^62", who, (long long)fr_first);
    const int tiles = ceil_div(n_out, RES_TILE);
    if ((int64_t)B * tiles >= ((int64_t)1 << 31))
        return fail(GOLF_EINVAL, "%s: B * ceil(n_out / %d) = %lld workgroups, must be < 2^31", who, RES_TILE,
                    (long long)B * tiles);
    const int64_t t_end = t_first + n_out, x_end = x_t0 + n_x, fr_end = fr_first + n_fr;
    const int64_t lo = t_first - M > 0 ? t_first - M : 0;
    if (x_t0 > lo)
        return fail(GOLF_EINVAL, "%s: x_t0=%lld lies above sample %lld, the first tap of sample t_first=%lld", who,
                    (long long)x_t0, (long long)lo, (long long)t_first);
    if (x_end < t_end)
        return fail(GOLF_EINVAL, "%s: n_x=%d: x ends at sample %lld, before the last computed sample %lld", who, n_x,
                    (long long)x_end, (long long)(t_end - 1));
    int64_t f_lo = t_first / hop;   // the frame of the first sample
    if (last) {
        if (t_end > (fr_end - 1) * hop + 1)
            return fail(GOLF_EINVAL, "%s: n_out=%d: the samples end at %lld, beyond (F - 1) hop + 1 = %lld of the F=%lld "
                        "frames the utterance ends with (last is set)", who, n_out, (long long)t_end,
                        (long long)((fr_end - 1) * hop + 1), (long long)fr_end);
        if (f_lo > fr_end - 2) f_lo = fr_end - 2 > 0 ? fr_end - 2 : 0;
    } else if ((t_end - 1) / hop + 1 >= fr_end) {
        return fail(GOLF_EINVAL, "%s: n_fr=%d: the frames end at %lld, without frame %lld after the last sample %lld, and "
                    "last is not set", who, n_fr, (long long)fr_end, (long long)((t_end - 1) / hop + 1), (long long)(t_end - 1));
    }
    if (fr_first > f_lo)
        return fail(GOLF_EINVAL, "%s: fr_first=%lld lies above frame %lld of the first sample t_first=%lld", who,
                    (long long)fr_first, (long long)f_lo, (long long)t_first);
    ResArgs p;
    p.x = x, p.x_stride = x_stride, p.x_t0 = x_t0, p.x_end = x_end, p.gain = gain, p.a = a, p.fr_first = fr_first;
    p.e = e, p.e_stride = e_stride, p.t_first = t_first, p.F = last ? fr_end : far;
    p.n_fr = n_fr, p.n_out = n_out, p.tiles = tiles, p.G = B * tiles, p.M = M, p.hop = hop;
    const int gx = p.G < RES_GRID_X ? p.G : RES_GRID_X;
    hipLaunchKernelGGL(ltv_residual_kernel, dim3((unsigned)gx, (unsigned)ceil_div(p.G, gx)), dim3(RES_TILE), 0,
                       (hipStream_t)stream, p);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" int golf_ltv_residual_f32(const float* x, int64_t x_stride, const float* gain, const float* a, float* e,
                                     int64_t e_stride, int B, int T, int F, int M, int hop, void* stream) {
    const char* who = "ltv_residual";
    if (B < 1 || T < 1 || F < 1) return fail(GOLF_EINVAL, "%s: bad size (B=%d T=%d F=%d)", who, B, T, F);
    if (hop < 1) return fail(GOLF_EINVAL, "%s: hop=%d must be >= 1", who, hop);
    if (x_stride < T) return fail(GOLF_EINVAL, "%s: row stride of x %lld < T=%d", who, (long long)x_stride, T);
    const int64_t cap = (int64_t)(F - 1) * hop + 1;   // T' = min(T, (F - 1) hop + 1)
    const int n_out = cap < T ? (int)cap : T;
    return residual_run(who, x, x_stride, 0, T, gain, a, 0, F, e, e_stride, B, 0, n_out, 1, M, hop, stream);
}

extern "C" int golf_ltv_residual_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* gain,
                                            const float* a, int64_t fr_first, int n_fr, float* e, int64_t e_stride, int B,
                                            int64_t t_first, int n_out, int last, int M, int hop, void* stream) {
    return residual_run("ltv_residual_stream", x, x_stride, x_t0, n_x, gain, a, fr_first, n_fr, e, e_stride, B, t_first, n_out,
                        last, M, hop, stream);
}
