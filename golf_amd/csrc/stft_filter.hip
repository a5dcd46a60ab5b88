// STFT-domain frame filter, block by block: the arithmetic of LTVCepFilter (NHV) and DiffWorldSPFilter (WORLD) --
// torch.stft(center, reflect) -> multiply by a per-frame response -> torch.istft -- one frame at a time, with the frames an
// unfinished output sample can still need carried between calls.
//
//   frame f   covers input samples [f*hop - n/2, f*hop + n/2); an index i < 0 reads x[-i], and once the utterance has ended
//             (x_end = T) an index i >= T reads x[2(T-1) - i]
//   u_f     = Re IFFT(FFT(w * frame_f) * H_f),  H_f given on bins 0 .. n/2 and extended by Hermitian symmetry
//   y[m]    = sum_f w[k] u_f[k] / sum_f w[k]^2,  k = m + n/2 - f*hop, over the frames 0 <= f < frames that cover m
//
// Two launches over the ring and workspace layout of stream_plan.h (RingPlan), as golf_lti_frames_ola_stream_f32 (lpc_ff.hip):
//   frames   the new frames into ws[b][S + f - f0], plus (extra blocks) the carried frames [f0 - S, f0) ring -> ws[b][0 .. S)
//   OLA      the output samples from ws alone, frames in ascending f with fmaf (the synthesis window is applied here, so a
//            frame is rounded once), plus (extra blocks) the last min(S, nf) new frames ws -> ring
// Neither launch reads what the same launch writes.  A frame is transformed by one group of n/4 lanes from its own samples
// and its own response row, so its bits -- and with the fixed summation order every output sample -- do not depend on how
// the input is split into calls.
//
// The transform: a Stockham radix-4 FFT in LDS (one radix-2 stage last when log2 n is odd), n/4 lanes per frame, one
// butterfly per lane and stage, so n = 1024 runs 5 stages instead of radix-2's 10 and every stage costs two barriers.  Frames
// of n <= 128 share a 64-lane block (4 or 2 frames per wave); n >= 256 takes one block of n/4 lanes per frame.  LDS holds the
// frame as separate re / im arrays (b32 accesses bank on (a/4) % 32 over 32-lane groups): a stage reads elements
// j + r*n/4 -- consecutive lanes, consecutive banks -- and writes base(j) + r*Ns.  Unpadded, the writes of the stages with
// Ns = 1 and Ns = 4 would land on 8 banks (4-way); element i is therefore stored at i + 4*(i >> 5), which makes the Ns = 4
// stage conflict-free, and the Ns = 1 stage writes its four consecutive elements as one 16-byte store.  Ns = 16 stays 2-way,
// Ns >= 64 is conflict-free.  n = 1024: 2 * 1152 floats for the frame + 2 * 1024 for the twiddles = 17 KB per block.
// Twiddles: exp(-2 pi i t / n) for t < n, formed once per block with sincospif (its argument 2t/n is exact) and kept in LDS;
// no fast-math sine or cosine.
#include <algorithm>
#include <climits>

#include "common.h"
#include "device_common.h"

namespace golf {

struct StftArgs {
    const float* x;      // window of the input: samples x0 .. x0+nx-1, row stride x_stride
    int64_t x_stride;
    int xl;              // -x0: window index below which a sample is reflected about global sample 0
    int xe;              // x_end - x0: window index from which a sample is reflected about x_end - 1 (INT_MAX/2 while open)
    int xb;              // window index of frame f0's position 0: f0*hop - n/2 - x0
    const float* h;      // response rows h0 .. h0+nh-1: (B, nh, n/2+1) real or (B, nh, n/2+1, 2) interleaved complex
    int nh, hr, h_kind;  // hr = f0 - h0
    const float* window;
    int nf, S, hop, n, lg, fpb;   // lg = log2 n; fpb: frames per block
    const float* carry;
    int ncin, cin_slot;  // carried frames copied into ws[b][S - ncin ..): ring slots cin_slot, cin_slot + 1, .. (mod S)
    float* ws;           // (B, S + nf, n)
};

__device__ __forceinline__ int stft_pad(int i) { return i + ((i >> 5) << 2); }

// One radix-4 stage (sub-transforms of length Ns = 1 << ls done) of the lane's frame, in place: read, barrier, write, barrier.
template <bool INV>
__device__ __forceinline__ void stft_radix4(float* re, float* im, const float* twc, const float* tws, int j, int q, int ls,
                                            int lg) {
    const int Ns = 1 << ls;
    const int k = j & (Ns - 1);
    const int t1 = k << (lg - ls - 2);
    float vr[4], vi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = stft_pad(j + r * q);
        vr[r] = re[i];
        vi[r] = im[i];
    }
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float c = twc[r * t1], s = INV ? -tws[r * t1] : tws[r * t1];
        const float a = vr[r], b = vi[r];
        vr[r] = fmaf(a, c, -b * s);
        vi[r] = fmaf(a, s, b * c);
    }
    const float a0r = vr[0] + vr[2], a0i = vi[0] + vi[2], a1r = vr[0] - vr[2], a1i = vi[0] - vi[2];
    const float a2r = vr[1] + vr[3], a2i = vi[1] + vi[3], a3r = vr[1] - vr[3], a3i = vi[1] - vi[3];
    // forward: bin 1 = a1 - i a3, bin 3 = a1 + i a3; the inverse swaps them
    const float rr = INV ? -a3i : a3i, ri = INV ? a3r : -a3r;
    float orr[4] = {a0r + a2r, a1r + rr, a0r - a2r, a1r - rr};
    float oi[4] = {a0i + a2i, a1i + ri, a0i - a2i, a1i - ri};
    __syncthreads();
    const int base = ((j >> ls) << (ls + 2)) + k;
    if (ls == 0) {   // four consecutive elements (stft_pad keeps groups of 4 together, 16-byte aligned)
        const int i = stft_pad(base);
        *reinterpret_cast<float4*>(re + i) = make_float4(orr[0], orr[1], orr[2], orr[3]);
        *reinterpret_cast<float4*>(im + i) = make_float4(oi[0], oi[1], oi[2], oi[3]);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = stft_pad(base + r * Ns);
            re[i] = orr[r];
            im[i] = oi[r];
        }
    }
    __syncthreads();
}

// The last stage when log2 n is odd: radix 2 over Ns = n/2; a lane takes the butterflies j and j + n/4.
template <bool INV>
__device__ __forceinline__ void stft_radix2_last(float* re, float* im, const float* twc, const float* tws, int j, int q) {
    float ar[2], ai[2], br[2], bi[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int k = j + u * q;
        const int i0 = stft_pad(k), i1 = stft_pad(k + 2 * q);
        const float c = twc[k], s = INV ? -tws[k] : tws[k];
        const float a = re[i1], b = im[i1];
        ar[u] = re[i0];
        ai[u] = im[i0];
        br[u] = fmaf(a, c, -b * s);
        bi[u] = fmaf(a, s, b * c);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int k = j + u * q;
        const int i0 = stft_pad(k), i1 = stft_pad(k + 2 * q);
        re[i0] = ar[u] + br[u];
        im[i0] = ai[u] + bi[u];
        re[i1] = ar[u] - br[u];
        im[i1] = ai[u] - bi[u];
    }
    __syncthreads();
}

template <bool INV>
__device__ __forceinline__ void stft_fft(float* re, float* im, const float* twc, const float* tws, int j, int q, int lg) {
    int ls = 0;
    for (; ls + 2 <= lg; ls += 2) stft_radix4<INV>(re, im, twc, tws, j, q, ls, lg);
    if (ls < lg) stft_radix2_last<INV>(re, im, twc, tws, j, q);
}

// grid (ceil(nf / fpb) + ncin, B), fpb * n/4 threads, dynamic LDS = 2 n (twiddles) + fpb * 2 * (n + n/8) floats.
__global__ __launch_bounds__(512) void stft_frames_kernel(StftArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = p.n, q = n >> 2, lg = p.lg;
    const int b = blockIdx.y;
    const int nblk = (p.nf + p.fpb - 1) / p.fpb;
    if ((int)blockIdx.x >= nblk) {
        ring_to_ws(p.carry, p.ws, b, blockIdx.x - nblk, p.S, n, p.S + p.nf, p.ncin, p.cin_slot, threadIdx.x, blockDim.x);
        return;
    }
    const int P = n + (n >> 3);
    float* twc = lds;
    float* tws = lds + n;
    const int g = threadIdx.x >> (lg - 2), j = threadIdx.x & (q - 1);
    float* re = lds + 2 * n + (size_t)g * 2 * P;
    float* im = re + P;
    const int fl = blockIdx.x * p.fpb + g;   // frame f0 + fl
    const bool mine = fl < p.nf;
    const int flc = mine ? fl : p.nf - 1;    // (a group past the last frame repeats it and writes nothing)
    {
        const float step = -2.0f / (float)n;   // exact: n is a power of two
        for (int t = threadIdx.x; t < n; t += blockDim.x) {
            float s, c;
            sincospif((float)t * step, &s, &c);
            twc[t] = c;
            tws[t] = s;
        }
    }
    {
        const float* xrow = p.x + (size_t)b * p.x_stride;
        const int sb = p.xb + flc * p.hop;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            int r = sb + k;
            if (r < p.xl) r = 2 * p.xl - r;
            if (r >= p.xe) r = 2 * (p.xe - 1) - r;
            re[stft_pad(k)] = xrow[r] * p.window[k];
            im[stft_pad(k)] = 0.f;
        }
    }
    __syncthreads();
    stft_fft<false>(re, im, twc, tws, j, q, lg);
    {
        // bins j + u*n/4 are the ones this lane reads in the inverse's first stage: no barrier in between
        const int nb = (n >> 1) + 1;
        const float* hrow = p.h + ((size_t)b * p.nh + p.hr + flc) * nb * (p.h_kind ? 2 : 1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            const int kk = k <= (n >> 1) ? k : n - k;
            float hre, him = 0.f;
            if (p.h_kind) {
                const float2 hv = *reinterpret_cast<const float2*>(hrow + 2 * kk);
                hre = hv.x;
                him = k <= (n >> 1) ? hv.y : -hv.y;
            } else {
                hre = hrow[kk];
            }
            const int i = stft_pad(k);
            const float a = re[i], c = im[i];
            re[i] = fmaf(a, hre, -c * him);
            im[i] = fmaf(a, him, c * hre);
        }
    }
    stft_fft<true>(re, im, twc, tws, j, q, lg);
    if (mine) {
        float* orow = p.ws + ((size_t)b * (p.S + p.nf) + p.S + fl) * n;
        const float inv_n = 1.0f / (float)n;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            orow[k] = re[stft_pad(k)] * inv_n;
        }
    }
}

// Output samples n0 + i, i < ny, from the frames at ws slot f - (f0 - S); extra blocks copy the last ncout new frames into the
// carried ring.  m = mb + i: the sample's position relative to ws slot 0 (sample + n/2 - (f0 - S)*hop); slots [fmin, fmax]
// hold frames that exist.
__global__ __launch_bounds__(256) void stft_ola_kernel(const float* __restrict__ ws, const float* __restrict__ window,
                                                       float* __restrict__ y, int64_t y_stride, float* __restrict__ carry,
                                                       int ny, int mb, int fmin, int fmax, int nslot, int hop, int n, int S,
                                                       int ncout, int cout_slot) {
    const int b = blockIdx.y;
    const int nob = (ny + 255) / 256;
    if ((int)blockIdx.x >= nob) {
        ws_to_ring(ws, carry, b, blockIdx.x - nob, S, n, nslot, ncout, cout_slot, threadIdx.x, 256);
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ny) return;
    const int m = mb + i;
    int fhi = m / hop;
    if (fhi > fmax) fhi = fmax;
    int flo = m - n + 1 <= 0 ? 0 : (m - n + hop) / hop;
    if (flo < fmin) flo = fmin;
    const float* wf = ws + (size_t)b * nslot * n;
    float acc = 0.f, norm = 0.f;
    for (int f = flo; f <= fhi; ++f) {
        const int k = m - f * hop;
        const float wk = window[k];
        acc = fmaf(wk, wf[(size_t)f * n + k], acc);
        norm = fmaf(wk, wk, norm);
    }
    y[(size_t)b * y_stride + i] = acc / norm;
}

// ---- backward of the whole utterance (x_end = T, frames_end = frames, a zero carry) -------------------------------------------
// With q = gy / norm:  gu_f[k] = w[k] q[f*hop - n/2 + k]  (0 outside [0, Ty)),  GU_f = FFT(gu_f),  V_f = FFT(v_f) recomputed;
//   g_h_f[kk] = c[kk] conj(V_f[kk]) GU_f[kk] / n  on bins 0 .. n/2  (c = 1 at 0 and n/2, else 2: a bin and its mirror);
//   gv_f      = Re IFFT(conj(Hext_f) GU_f);   G[p] = sum_f w[k] gv_f[k]  on the padded positions p = f*hop - n/2 + k;
//   g_x[r]    = G[r] + G[-r] (1 <= r <= n/2) + G[2(T-1) - r] (where that position is >= T): the transpose of the reflect pad.
// Two launches again: the frames (gv_f -> ws, g_h rows in place), then a gather of g_x from ws alone in a fixed order.
// v_f and gu_f are transformed one after the other, not packed as v + i gu into one complex transform: the split of a packed
// spectrum rounds GU_f relative to |V_f| + |GU_f|, and a loss gradient is routinely orders of magnitude smaller than the
// signal.  V_f's bins wait in registers meanwhile -- a lane needs exactly the bins it owns -- so the LDS is the forward's.
struct StftBwdArgs {
    const float* gy;     // (B, Ty)
    int64_t gy_stride;
    const float* x;      // (B, T)
    int64_t x_stride;
    const float* h;      // (B, F, n/2+1) real or (B, F, n/2+1, 2)
    int h_kind;
    const float* window;
    float* g_h;          // as h, or null: V_f and the response gradient are skipped
    float* ws;           // (B, frames, n): gv_f; null: no g_x wanted, the inverse transform is skipped
    int T, Ty, F, frames, hop, n, lg, fpb;
};

// grid (ceil(frames / fpb) + (g_h ? F - frames : 0), B): the extra blocks zero the response rows no frame uses.
__global__ __launch_bounds__(512) void stft_bwd_frames_kernel(StftBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = p.n, q = n >> 2, lg = p.lg, half = n >> 1;
    const int b = blockIdx.y;
    const int nb = half + 1, hw = p.h_kind ? 2 : 1;
    const int nblk = (p.frames + p.fpb - 1) / p.fpb;
    if ((int)blockIdx.x >= nblk) {
        float* dst = p.g_h + ((size_t)b * p.F + p.frames + (blockIdx.x - nblk)) * nb * hw;
        for (int k = threadIdx.x; k < nb * hw; k += blockDim.x) dst[k] = 0.f;
        return;
    }
    const int P = n + (n >> 3);
    float* twc = lds;
    float* tws = lds + n;
    const int g = threadIdx.x >> (lg - 2), j = threadIdx.x & (q - 1);
    float* re = lds + 2 * n + (size_t)g * 2 * P;
    float* im = re + P;
    const int f = blockIdx.x * p.fpb + g;
    const bool mine = f < p.frames;
    const int fc = mine ? f : p.frames - 1;    // (a group past the last frame repeats it and writes nothing)
    {
        const float step = -2.0f / (float)n;
        for (int t = threadIdx.x; t < n; t += blockDim.x) {
            float s, c;
            sincospif((float)t * step, &s, &c);
            twc[t] = c;
            tws[t] = s;
        }
    }
    const int sb = fc * p.hop - half;
    float vr[3] = {0.f, 0.f, 0.f}, vi[3] = {0.f, 0.f, 0.f};   // V_f at bins j, j + n/4, j + n/2 (the last is used by j = 0 only)
    if (p.g_h) {
        const float* xrow = p.x + (size_t)b * p.x_stride;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            int r = sb + k;
            if (r < 0) r = -r;
            if (r >= p.T) r = 2 * (p.T - 1) - r;
            re[stft_pad(k)] = xrow[r] * p.window[k];
            im[stft_pad(k)] = 0.f;
        }
        __syncthreads();
        stft_fft<false>(re, im, twc, tws, j, q, lg);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            vr[u] = re[stft_pad(j + u * q)];
            vi[u] = im[stft_pad(j + u * q)];
        }
    }
    {
        // the elements this lane has just read are the ones it overwrites: no barrier in between
        const float* gyrow = p.gy + (size_t)b * p.gy_stride;
        const int fmax = p.frames - 1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            const int m = sb + k;          // output sample; m + n/2 is its position relative to frame 0's start
            float v = 0.f;
            if (m >= 0 && m < p.Ty) {
                const int mp = m + half;
                int fhi = mp / p.hop;
                if (fhi > fmax) fhi = fmax;
                const int flo = mp - n + 1 <= 0 ? 0 : (mp - n + p.hop) / p.hop;
                float norm = 0.f;          // the forward's normaliser, in the forward's order
                for (int ff = flo; ff <= fhi; ++ff) {
                    const float wk = p.window[mp - ff * p.hop];
                    norm = fmaf(wk, wk, norm);
                }
                v = p.window[k] * (gyrow[m] / norm);
            }
            re[stft_pad(k)] = v;
            im[stft_pad(k)] = 0.f;
        }
    }
    __syncthreads();
    stft_fft<false>(re, im, twc, tws, j, q, lg);
    const float inv_n = 1.0f / (float)n;
    if (p.g_h && mine) {
        float* grow = p.g_h + ((size_t)b * p.F + f) * nb * hw;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int k = j + u * q;
            if (k > half) continue;
            const float gr = re[stft_pad(k)], gi = im[stft_pad(k)];
            const float c = (k == 0 || k == half) ? inv_n : 2.0f * inv_n;
            const float hr = fmaf(vr[u], gr, vi[u] * gi) * c;    // conj(V) GU
            if (p.h_kind)
                *reinterpret_cast<float2*>(grow + 2 * k) = make_float2(hr, fmaf(vr[u], gi, -vi[u] * gr) * c);
            else
                grow[k] = hr;
        }
    }
    if (!p.ws) return;   // (uniform over the block)
    {
        // bins j + u*n/4 are the ones this lane reads in the inverse's first stage: no barrier in between
        const float* hrow = p.h + ((size_t)b * p.F + fc) * nb * hw;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            const int kk = k <= half ? k : n - k;
            float hre, him = 0.f;              // conj(Hext[k])
            if (p.h_kind) {
                const float2 hv = *reinterpret_cast<const float2*>(hrow + 2 * kk);
                hre = hv.x;
                him = k <= half ? -hv.y : hv.y;
            } else {
                hre = hrow[kk];
            }
            const int i = stft_pad(k);
            const float a = re[i], c = im[i];
            re[i] = fmaf(a, hre, -c * him);
            im[i] = fmaf(a, him, c * hre);
        }
    }
    stft_fft<true>(re, im, twc, tws, j, q, lg);
    if (mine) {
        float* orow = p.ws + ((size_t)b * p.frames + f) * n;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * q;
            orow[k] = re[stft_pad(k)] * inv_n;
        }
    }
}

// G at padded position p (mp = p + n/2 >= 0): the frames that cover it, in ascending f with fmaf; 0 where none does.
__device__ __forceinline__ float stft_bwd_G(const float* __restrict__ wf, const float* __restrict__ window, int mp, int frames,
                                            int hop, int n) {
    int fhi = mp / hop;
    if (fhi > frames - 1) fhi = frames - 1;
    const int flo = mp - n + 1 <= 0 ? 0 : (mp - n + hop) / hop;
    float acc = 0.f;
    for (int f = flo; f <= fhi; ++f) {
        const int k = mp - f * hop;
        acc = fmaf(window[k], wf[(size_t)f * n + k], acc);
    }
    return acc;
}

// g_x (B, T) from the frames in ws: the position itself, its mirror about sample 0, its mirror about sample T-1.
__global__ __launch_bounds__(256) void stft_bwd_gather_kernel(const float* __restrict__ ws, const float* __restrict__ window,
                                                              float* __restrict__ g_x, int64_t g_x_stride, int T, int frames,
                                                              int hop, int n) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= T) return;
    const int half = n >> 1;
    const float* wf = ws + (size_t)b * frames * n;
    float acc = stft_bwd_G(wf, window, r + half, frames, hop, n);
    if (r >= 1 && r <= half) acc += stft_bwd_G(wf, window, half - r, frames, hop, n);
    const int p2 = 2 * (T - 1) - r;
    if (p2 >= T) acc += stft_bwd_G(wf, window, p2 + half, frames, hop, n);
    g_x[(size_t)b * g_x_stride + r] = acc;
}

// rows (gridDim.y) of `cols` zeros
__global__ __launch_bounds__(256) void stft_bwd_zero_kernel(float* __restrict__ dst, int64_t stride, int64_t cols) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cols) dst[(size_t)blockIdx.y * stride + i] = 0.f;
}

static int stft_log2(int n) {   // log2 n for a power of two in [64, 2048], else 0
    for (int lg = 6; lg <= 11; ++lg)
        if (n == (1 << lg)) return lg;
    return 0;
}

// The one-shot geometry the backward takes (what the forward takes with the end markers set), else an error code.
static int stft_bwd_geometry(int B, int T, int F, int n_fft, int hop, bool report) {
    auto no = [&](int code, const char* msg) { return report ? fail(code, "stft_filter_frames_bwd: %s", msg) : code; };
    if (B < 1 || T < 1 || F < 1 || hop < 1 || n_fft < 1) return no(GOLF_EINVAL, "bad size");
    if (!stft_log2(n_fft)) return no(GOLF_EUNSUPPORTED, "n_fft is not a power of two in [64, 2048]");
    if (n_fft < 2 * hop) return no(GOLF_EINVAL, "n_fft < 2*hop");
    if (T <= n_fft / 2) return no(GOLF_EINVAL, "T samples cannot be reflect-padded by n_fft/2");
    const int64_t frames = std::min<int64_t>(1 + T / hop, F);
    if (frames * n_fft >= (1ll << 29) || T >= (1 << 29) || (int64_t)F * (n_fft / 2 + 1) >= (1ll << 29))
        return no(GOLF_EUNSUPPORTED, "call too large");
    return GOLF_OK;
}

}  // namespace golf

using namespace golf;

extern "C" size_t golf_stft_filter_stream_state_bytes(int B, int n_fft, int hop) {
    if (B < 1 || hop < 1 || !stft_log2(n_fft) || n_fft < 2 * hop) return 0;
    return ring_state_bytes(B, n_fft, hop);
}

extern "C" int golf_stft_filter_frames_stream_f32(const float* x, int64_t x_stride, int64_t x0, int nx, int64_t x_end,
                                                  const float* h, int64_t h0, int nh, int h_kind, int64_t frames_end,
                                                  const float* window, int64_t f0, int nf, float* y, int64_t y_stride,
                                                  int64_t n0, int ny, int B, int n_fft, int hop, float* carry, void* ws,
                                                  size_t ws_bytes, void* stream) {
    if (B < 1 || hop < 1 || n_fft < 1 || nf < 0 || ny < 0 || nx < 0 || nh < 0 || x0 < 0 || h0 < 0 || f0 < 0 || n0 < 0 ||
        (h_kind != 0 && h_kind != 1))
        return fail(GOLF_EINVAL, "stft_filter_stream: bad size, kind or negative start");
    const int lg = stft_log2(n_fft);
    if (!lg) return fail(GOLF_EUNSUPPORTED, "stft_filter_stream: n_fft %d is not a power of two in [64, 2048]", n_fft);
    if (n_fft < 2 * hop) return fail(GOLF_EINVAL, "stft_filter_stream: n_fft %d < 2*hop %d", n_fft, 2 * hop);
    if (!window || !carry || (nf > 0 && (!x || !h)) || ((nf > 0 || ny > 0) && !ws) || (ny > 0 && !y))
        return fail(GOLF_EINVAL, "stft_filter_stream: null pointer");
    if ((x_end < 0) != (frames_end < 0))
        return fail(GOLF_EINVAL, "stft_filter_stream: x_end and frames_end are both open (< 0) or both set");
    const bool fin = x_end >= 0;
    const int64_t W = n_fft, pad = n_fft / 2, H = hop;
    const int S = ring_S(n_fft, hop);
    int64_t nfr = kRingOpen, Ty = kRingOpen;
    if (fin) {
        if (x_end <= pad) return fail(GOLF_EINVAL, "stft_filter_stream: x_end %lld cannot be reflect-padded by n_fft/2 = %lld",
                                      (long long)x_end, (long long)pad);
        if (frames_end < 1 || frames_end > 1 + x_end / H)
            return fail(GOLF_EINVAL, "stft_filter_stream: frames_end %lld outside [1, 1 + x_end/hop = %lld]",
                        (long long)frames_end, (long long)(1 + x_end / H));
        nfr = frames_end;
        Ty = (nfr - 1) * H;
        if (int rc = ring_check_end("stft_filter_stream", f0, nf, n0, ny, nfr, Ty)) return rc;
    }
    if ((nf > 0 && nx > 0 && x_stride < nx) || (ny > 0 && y_stride < ny))
        return fail(GOLF_EINVAL, "stft_filter_stream: row stride too small");
    if ((int64_t)(S + nf) * W >= (1ll << 29) || nx >= (1 << 29) || (int64_t)(S + nf + 1) * H >= (1ll << 29) ||
        (int64_t)nh * (pad + 1) >= (1ll << 29))
        return fail(GOLF_EUNSUPPORTED, "stft_filter_stream: call too large (%d frames, %d samples)", nf, nx);
    // frames [f0, f0+nf): their response rows and the samples they read, reflections included
    if (nf > 0) {
        if (f0 < h0 || f0 + nf > h0 + nh)
            return fail(GOLF_EINVAL, "stft_filter_stream: the response window does not cover the frames");
        const int64_t s0 = f0 * H - pad, e1 = (f0 + nf - 1) * H + pad;   // first frame's start, last frame's end (exclusive)
        int64_t lo = std::max<int64_t>(0, s0), hi = e1 - 1;
        if (s0 < 0) hi = std::max(hi, -s0);                              // x[-i]
        if (fin && e1 > x_end) {                                         // x[2(T-1) - i], i up to e1 - 1
            lo = std::min(lo, 2 * (x_end - 1) - (e1 - 1));
            hi = std::min(hi, x_end - 1);
            if (s0 < 0) hi = std::max(hi, std::min(-s0, x_end - 1));
        }
        if (x0 > lo || x0 + nx <= hi)
            return fail(GOLF_EINVAL, "stft_filter_stream: the input window does not cover samples [%lld, %lld]",
                        (long long)lo, (long long)hi);
    }
    RingPlan r;
    if (int rc = ring_plan("stft_filter_stream", n_fft, hop, f0, nf, n0, ny, nfr, Ty, B, ws, ws_bytes, &r)) return rc;
    if (nf == 0 && ny == 0) return GOLF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int lim = 1 << 30;
    StftArgs p;
    p.x = x;
    p.x_stride = x_stride;
    p.xl = (int)std::max<int64_t>(-x0, -lim);
    p.xe = fin ? (int)std::min<int64_t>(x_end - x0, lim) : lim;
    p.xb = (int)std::max<int64_t>(std::min<int64_t>(f0 * H - pad - x0, lim), -lim);
    p.h = h;
    p.nh = nh;
    p.hr = (int)(nf > 0 ? f0 - h0 : 0);
    p.h_kind = h_kind;
    p.window = window;
    p.nf = nf;
    p.S = S;
    p.hop = hop;
    p.n = n_fft;
    p.lg = lg;
    p.fpb = n_fft >= 256 ? 1 : 256 / n_fft;   // 64-lane blocks at least
    p.carry = carry;
    p.ncin = r.ncin, p.cin_slot = r.cin_slot;
    p.ws = (float*)ws;
    if (nf > 0 || p.ncin > 0) {
        const int threads = p.fpb * (n_fft / 4);
        const size_t ldsb = sizeof(float) * (2 * (size_t)n_fft + (size_t)p.fpb * 2 * (n_fft + n_fft / 8));
        hipLaunchKernelGGL(stft_frames_kernel, dim3((unsigned)(ceil_div(nf, p.fpb) + p.ncin), B), dim3(threads), ldsb, st, p);
        GOLF_LAUNCH_CHECK();
    }
    if (ny > 0 || r.ncout > 0) {
        hipLaunchKernelGGL(stft_ola_kernel, dim3((unsigned)(ceil_div(ny, 256) + r.ncout), B), dim3(256), 0, st,
                           (const float*)ws, window, y, y_stride, carry, ny, r.mb, r.fmin, r.fmax, r.nslot, hop, n_fft, S,
                           r.ncout, r.cout_slot);
        GOLF_LAUNCH_CHECK();
    }
    return GOLF_OK;
}

extern "C" size_t golf_stft_filter_frames_bwd_workspace_bytes(int B, int T, int F, int n_fft, int hop) {
    if (stft_bwd_geometry(B, T, F, n_fft, hop, false) != GOLF_OK) return 0;
    return align_up(sizeof(float) * (size_t)B * std::min(1 + T / hop, F) * n_fft, 256);
}

extern "C" int golf_stft_filter_frames_bwd_f32(const float* gy, int64_t gy_stride, const float* x, int64_t x_stride,
                                               const float* h, int h_kind, const float* window, float* g_x,
                                               int64_t g_x_stride, float* g_h, int B, int T, int F, int n_fft, int hop,
                                               void* ws, size_t ws_bytes, void* stream) {
    if (h_kind != 0 && h_kind != 1) return fail(GOLF_EINVAL, "stft_filter_frames_bwd: bad kind %d", h_kind);
    const int rc = stft_bwd_geometry(B, T, F, n_fft, hop, true);
    if (rc != GOLF_OK) return rc;
    const int frames = std::min(1 + T / hop, F), Ty = hop * (frames - 1);
    if (!x || !h || !window || (Ty > 0 && !gy) || (!g_x && !g_h))
        return fail(GOLF_EINVAL, "stft_filter_frames_bwd: null pointer (one of g_x, g_h may be null)");
    if (x_stride < T || gy_stride < Ty || (g_x && g_x_stride < T))
        return fail(GOLF_EINVAL, "stft_filter_frames_bwd: row stride too small");
    const size_t need = golf_stft_filter_frames_bwd_workspace_bytes(B, T, F, n_fft, hop);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255))
        return fail(GOLF_EWORKSPACE, "stft_filter_frames_bwd: workspace needs %zu bytes, 256-aligned (got %zu)", need, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int64_t hcols = (int64_t)F * (n_fft / 2 + 1) * (h_kind ? 2 : 1);
    if (Ty == 0) {   // a single frame reaches no output sample
        if (g_x) {
            hipLaunchKernelGGL(stft_bwd_zero_kernel, dim3((unsigned)ceil_div(T, 256), B), dim3(256), 0, st, g_x, g_x_stride,
                               (int64_t)T);
            GOLF_LAUNCH_CHECK();
        }
        if (g_h) {
            hipLaunchKernelGGL(stft_bwd_zero_kernel, dim3((unsigned)ceil_div(hcols, 256), B), dim3(256), 0, st, g_h, hcols, hcols);
            GOLF_LAUNCH_CHECK();
        }
        return GOLF_OK;
    }
    StftBwdArgs p;
    p.gy = gy;
    p.gy_stride = gy_stride;
    p.x = x;
    p.x_stride = x_stride;
    p.h = h;
    p.h_kind = h_kind;
    p.window = window;
    p.g_h = g_h;
    p.ws = g_x ? (float*)ws : nullptr;
    p.T = T;
    p.Ty = Ty;
    p.F = F;
    p.frames = frames;
    p.hop = hop;
    p.n = n_fft;
    p.lg = stft_log2(n_fft);
    p.fpb = n_fft >= 256 ? 1 : 256 / n_fft;
    const int threads = p.fpb * (n_fft / 4);
    const size_t ldsb = sizeof(float) * (2 * (size_t)n_fft + (size_t)p.fpb * 2 * (n_fft + n_fft / 8));
    hipLaunchKernelGGL(stft_bwd_frames_kernel, dim3((unsigned)(ceil_div(frames, p.fpb) + (g_h ? F - frames : 0)), B),
                       dim3(threads), ldsb, st, p);
    GOLF_LAUNCH_CHECK();
    if (g_x) {
        hipLaunchKernelGGL(stft_bwd_gather_kernel, dim3((unsigned)ceil_div(T, 256), B), dim3(256), 0, st, (const float*)ws,
                           window, g_x, g_x_stride, T, frames, hop, n_fft);
        GOLF_LAUNCH_CHECK();
    }
    return GOLF_OK;
}
