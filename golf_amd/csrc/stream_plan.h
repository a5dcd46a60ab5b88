// Host-side plan of the block-by-block entries: whether a call's position allows a launch, and where its frames sit in the
// carried ring and the workspace.  No HIP here, so it is tested on a CPU (tests/test_stream_plan_host.py); the entries in
// lpc_ff.hip, stft_filter.hip, harm_analysis.hip and spec_envelope.hip execute it and decide none of it themselves.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "golf_amd.h"

namespace golf {

int fail(int code, const char* fmt, ...);

// ---- carried-frame overlap-add (golf_lti_frames_ola_stream_f32, golf_stft_filter_frames_stream_f32) -----------------------
// Frame f covers the output positions [f*hop - W/2, f*hop - W/2 + W).  A call filters frames [f0, f0+nf) into ws[b][S + f - f0]
// and writes the samples [n0, n0+ny); the last S = ceil(W/hop) - 1 filtered frames are carried in a (B, S, W) ring, slot f % S.
inline int ring_S(int W, int hop) { return (W + hop - 1) / hop - 1; }
inline size_t ring_state_bytes(int B, int W, int hop) { return sizeof(float) * (size_t)B * ring_S(W, hop) * W; }
constexpr int64_t kRingOpen = INT64_MAX;   // nfr and Ty while the utterance has not ended

struct RingPlan {
    int ncin, cin_slot;     // carried frames [f0 - ncin, f0): ring slots cin_slot, cin_slot + 1, .. (mod S) -> ws[b][S - ncin ..)
    int ncout, cout_slot;   // the last ncout new frames: ws[b][nslot - ncout ..) -> ring slots cout_slot, cout_slot + 1, .. (mod S)
    int nslot;              // S + nf workspace slots; slot s holds frame f0 - S + s
    int mb;                 // output sample n0 + i lies at position mb + i relative to the start of ws slot 0
    int fmin, fmax;         // the slots that hold frames that exist
};

// Once the utterance has ended with nfr frames and Ty output samples, a call stays within them.
inline int ring_check_end(const char* who, int64_t f0, int nf, int64_t n0, int ny, int64_t nfr, int64_t Ty) {
    if (f0 + nf > nfr) return fail(GOLF_EINVAL, "%s: frames past the last one (%lld)", who, (long long)nfr);
    if (n0 + ny > Ty) return fail(GOLF_EINVAL, "%s: samples past the end (%lld)", who, (long long)Ty);
    return GOLF_OK;
}

// The order of the calls: every frame the samples [n0, n0+ny) need is filtered by now and the ring still holds the earliest
// one, and no frame leaves the ring before the samples it reaches are written.  Then the workspace, then the plan.
inline int ring_plan(const char* who, int W, int hop, int64_t f0, int nf, int64_t n0, int ny, int64_t nfr, int64_t Ty, int B,
                     const void* ws, size_t ws_bytes, RingPlan* p) {
    const int64_t pad = W / 2, H = hop;
    const int S = ring_S(W, hop);
    auto flo = [&](int64_t n) { const int64_t d = n + pad - W + 1; return d <= 0 ? (int64_t)0 : (d + H - 1) / H; };
    const int64_t fdone = f0 + nf;
    if (ny > 0) {
        const int64_t fhi = std::min((n0 + ny - 1 + pad) / H, nfr - 1);
        if (fhi >= fdone) return fail(GOLF_EINVAL, "%s: sample %lld needs frame %lld, not filtered yet", who,
                                      (long long)(n0 + ny - 1), (long long)fhi);
        if (flo(n0) < f0 - S) return fail(GOLF_EINVAL, "%s: sample %lld needs frame %lld; the carry holds frames from %lld", who,
                                          (long long)n0, (long long)flo(n0), (long long)(f0 - S));
    }
    if (nf > 0 && n0 > std::max<int64_t>(0, f0 * H - pad))
        return fail(GOLF_EINVAL, "%s: samples before %lld were written without frame %lld", who, (long long)n0, (long long)f0);
    if (n0 + ny != Ty && flo(n0 + ny) < fdone - S)
        return fail(GOLF_EINVAL, "%s: write the samples up to %lld before filtering frame %lld (the carry holds %d frames)", who,
                    (long long)((fdone - S) * H - pad + W - 1), (long long)(fdone - 1), S);
    const size_t need = sizeof(float) * (size_t)B * (S + nf) * W;
    if ((nf > 0 || ny > 0) && (ws_bytes < need || ((uintptr_t)ws & 255)))
        return fail(GOLF_EWORKSPACE, "%s: workspace needs %zu bytes, 256-aligned (got %zu)", who, need, ws_bytes);
    const int64_t fbase = f0 - S;   // the frame of ws slot 0
    p->ncin = ny > 0 ? (int)std::min<int64_t>(S, f0) : 0;
    p->cin_slot = p->ncin ? (int)((f0 - p->ncin) % S) : 0;
    p->ncout = (int)std::min<int64_t>(S, nf);
    p->cout_slot = p->ncout ? (int)((fdone - p->ncout) % S) : 0;
    p->nslot = S + nf;
    p->mb = (int)(n0 + pad - fbase * H);
    p->fmin = (int)std::max<int64_t>(0, -fbase);
    p->fmax = (int)(std::min(fdone, nfr) - 1 - fbase);
    return GOLF_OK;
}

// ---- frame position of an analysis stream (golf_harmonic_analysis_stream_f32, golf_spectral_envelope_stream_f32) ----------
// Frames f_first .. f_first + n_frames - 1, of which frame f may read the samples [f*hop - back, f*hop + ahead) and the f0
// frames f - f_back .. f + f_ahead, from x (n_x samples from x_t0 on) and f0 (n_f0 frames from f0_first on); only a `last` call
// reads beyond the buffers.  Positions stay below 2^62: no sum or product here or in a kernel wraps.  (In Python:
// functional._check_frame_position.)
inline int frame_position_check(const char* who, int64_t x_t0, int n_x, int64_t f0_first, int n_f0, int64_t f_first,
                                int n_frames, int last, int hop, int64_t back, int64_t ahead, int f_back, int f_ahead) {
    const int64_t far = (int64_t)1 << 62;
    if (x_t0 < 0 || x_t0 > far) return fail(GOLF_EINVAL, "%s: x_t0=%lld must be 0..2^62", who, (long long)x_t0);
    if (f0_first < 0 || f0_first > far) return fail(GOLF_EINVAL, "%s: f0_first=%lld must be 0..2^62", who, (long long)f0_first);
    if (f_first < 0 || f_first > far / hop - n_frames)
        return fail(GOLF_EINVAL, "%s: f_first=%lld must be >= 0 with (f_first + n_frames) hop <= 2^62", who, (long long)f_first);
    const int64_t lo = std::max<int64_t>(f_first * hop - back, 0), f_lo = std::max<int64_t>(f_first - f_back, 0);
    const int64_t f_end = f_first + n_frames, x_end = x_t0 + n_x, f0_end = f0_first + n_f0;
    if (x_t0 > lo)
        return fail(GOLF_EINVAL, "%s: x_t0=%lld lies above sample %lld, where the window of frame f_first=%lld may start", who,
                    (long long)x_t0, (long long)lo, (long long)f_first);
    if (f0_first > f_lo)
        return fail(GOLF_EINVAL, "%s: f0_first=%lld lies above frame %lld, the first that frame f_first=%lld reads", who,
                    (long long)f0_first, (long long)f_lo, (long long)f_first);
    if (f_end > f0_end)
        return fail(GOLF_EINVAL, "%s: n_f0=%d: f0 ends at frame %lld, before the last computed frame %lld", who, n_f0,
                    (long long)f0_end, (long long)(f_end - 1));
    if (!last && (f_end - 1) * hop + ahead > x_end)
        return fail(GOLF_EINVAL, "%s: n_x=%d: x ends at sample %lld, before the window of frame %lld may end (%lld) and "
                    "last is not set", who, n_x, (long long)x_end, (long long)(f_end - 1),
                    (long long)((f_end - 1) * hop + ahead));
    if (!last && f_end + f_ahead > f0_end)   // (f_ahead = 0: the check before the last one has made it)
        return fail(GOLF_EINVAL, "%s: n_f0=%d: f0 ends at frame %lld, without the neighbour after frame %lld, and last is "
                    "not set", who, n_f0, (long long)f0_end, (long long)(f_end - 1));
    return GOLF_OK;
}

}  // namespace golf
