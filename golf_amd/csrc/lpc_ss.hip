// Sample-wise time-varying all-pole (LPC) synthesis filter for gfx950 — GOLF-ss end filter.
//
// Replaces LTVMinimumPhaseFilterPrecise.forward (reference models/filters.py:99-113), i.e.
// AudioTensor gain broadcast + a.reduce_hop_length() (models/utils.py:171-191,538-544) +
// torchlpc.sample_wise_lpc (models/filters.py:112), and its autograd backward.
//
// Algorithm (MI355X-first; nothing like the reference's serial 22-thread numba kernel):
//   The recursion y[t] = x[t] - sum_i A[t,i] y[t-1-i] is linear in the state
//   s_t = (y[t-1..t-M]).  Time is cut into chunks of L samples.  Per chunk c:
//     P1f/P1h  M homogeneous trajectories (unit initial states, no input) -> Phi_c (MxM)
//              [fp32 for inference, fp64 for training; stored fp32]
//     P1z      one zero-state trajectory with the real input              -> z_c   (M)  [fp32]
//   so that s_{c+1} = Phi_c s_c + z_c.  Then
//     first pass   chunk-boundary states S1 from the maps (two-level scan: group composites on the f64 matrix pipe +
//                  per-group scans; or one wave per utterance, flat)
//     refinement   every chunk re-runs its L-step recursion from S1_c -> its true end state E_c; the DEFECTS
//                  d_c = E_c - S1_{c+1} are scanned on their own (delta_{c+1} = Phi_c delta_c + d_c) and the final
//                  states are S1 + delta: one Parareal sweep in delta form.  The maps then act on a correction that is
//                  ~1e-4 of the state, so their fp32 rounding (and the fp32 trajectories' error) is second order and the
//                  result is the sequential fp32 recursion's -- the reference's arithmetic -- up to its own rounding.
//     final pass   every chunk runs from S1_c + delta_c -> y
//   B*NC*(M+1) independent in-lane recursions instead of B serial ones: at B=32, T=47761
//   that is 146k lanes x 240 steps instead of 32 lanes x 47761 steps.
//   Conditioning tiers (lpc_fixup_kernel; numerics measured in tools/numlab): the sweep contracts as long
//   as the maps are accurate relative to their size.  Chunks whose fp32 map has entries beyond ~30 are recomputed from
//   fp64 trajectories (in place, rounded to fp32); utterances with entries beyond ~256 take their boundary states from
//   an fp64 scan over maps kept as doubles.  Both ride in launches that exist anyway.
//   Frame-rate coefficients (B,F,M) are interpolated on the fly (a_f + n*d_f, one FMA per tap);
//   the (B,T,M) tensor the reference materialises (134 MB at B=32) never exists.
//   Each lane keeps its M-sample history in a statically indexed rotating register window
//   (time loop unrolled by W, W | hop), so there are no moves and no LDS traffic in the loop.
//
// Backward: the adjoint of the recursion in transposed form
//     g[t] = gy[t] + lam[0];   lam[k] <- lam[k+1] - A[t,k] g[t]
//   (same-time coefficients: no tap-shifted A[t+1+i,i]) has chunk transition Phi_c^T, so the
//   forward's Phi is reused: B1 local adjoint per chunk, B2 boundary scan with Phi^T, B3 per-chunk
//   reverse recursion that also accumulates d/d gain and d/d a at frame rate (hat weights),
//   B4 tiny segment->frame reduction.  No (B,T,M) gradient tensor either.
#include "common.h"
#include "device_common.h"
#include "lpc_p1f.h"
#include <cstdlib>
#include <type_traits>

namespace golf {

// Conditioning tiers of the time-chunked algorithm (numerics: tools/numlab/lab2.py).
// The delta-form refinement sweep makes every error of the coarse propagator second order, PROVIDED the sweep contracts:
// the chunk maps have to be accurate relative to their size.  fp32 homogeneous trajectories lose ~1e-5 x (largest entry),
// so -- measured against the sequential fp32 recursion, the reference's arithmetic, over the benchmark recipe and much
// harsher coefficient tracks --
//   tier 1  largest |entry| of a chunk's fp32 map <= G1 (30): fp32 map + one sweep = sequential fp32 (1.8 % of the
//           recipe's utterances have a chunk beyond 30, 0.13 % one beyond 256);
//   tier 2  an utterance with a chunk beyond G1 (or 160 chunks beyond G2: hot_count): lpc_fixup_kernel recomputes the maps of
//           its chunks beyond G2 (8; round 5: 10) from
//           fp64 trajectories, rounds them to fp32 IN PLACE, and everything downstream is unchanged: equal to sequential
//           fp32 up to entries of ~400.  (Why the second threshold: inside a long stretch of 15..30 the fp32 maps' errors
//           are amplified by the hot neighbours -- over 2048 utterances of the recipe "chunks beyond 30 only" left one at
//           3.5 x the sequential error, "beyond 10 where some chunk is beyond 30" none above 1.2 x.)
//   tier 3  an utterance with an entry beyond G3 (256), a non-finite one, groups of maps whose product could overflow
//           fp32, or -- round 6, hot_all_16ths -- a tier-2 utterance EVERY chunk of which is hot: all its maps are recomputed and kept as DOUBLES, its boundary states are scanned in fp64 (flat path: one
//           wave, riding in the first scan launch; two-level path: fp64 group composites + fold in the refinement launch's
//           extra rows, the groups' own maps in the final pass's prologue -- precise_group_job), and its chunks run from
//           those states without a sweep: at or below the sequential recursion's error for entries up to 7e4 (beyond that
//           both are garbage).
// Cost: one light launch (lpc_fixup_kernel: every wave reads its utterance's per-chunk maxima and returns unless it owns a
// hot chunk); a hot chunk costs its wave one fp64 pass over the chunk (~25 us), a tier-3 utterance additionally a 199-step
// fp64 scan (~45 us) beside the 15 us pre-pass.  No sequential fallback exists any more (round 2: 2.6 ms).
static float phi_guard() {
    static const float v = [] { const char* e = getenv("GOLF_SS_PHI_GUARD"); return e ? (float)atof(e) : 30.f; }();
    return v;   // <= 0: no chunk is ever hot (dev knob)
}
static float phi_guard2() {
    // 10 (round 5; rounds 3 - 4 shipped 16): tools/fuzz_tiers.py, seed 31, found two utterances of harsher-than-recipe tracks
    // (largest entries 44 and 34, 77 % and 20 % of their chunks beyond 16) at 19 x and 6 x the sequential recursion's error with
    // the fp32 maps of their chunks in 10..16 left alone; at 12 the second is still 5 x off, at 10 / 8 / 4 both are within 2 x.
    // Costs a batch with hot utterances ~5 us alone (54 % more of the recipe's hot chunks are recomputed), a cold one nothing.
    // Round 6: 8.  The three rows of the round-5 soak that sat at 1.01 - 1.09 x the suite's bound with their chunks beyond 10
    // recomputed (tools/fuzz_tiers.py seeds 31 / 909 / 808: tier-2 utterances, largest entries 32 - 134, 75 - 160 hot chunks) come out
    // at 0.3 - 0.6 x with the chunks in 8..10 recomputed as well; the recipe's batches pay ~1.3 us in the mean of 32 (a hot batch ~3).
    static const float v = [] { const char* e = getenv("GOLF_SS_PHI_GUARD2"); return e ? (float)atof(e) : 8.f; }();
    return v;   // chunks of an utterance that has a chunk beyond G1 are hot from G2 on
}
static float group_log2_guard() {
    // Sum over a group's 16 chunks of log2(max(|map entries|, 1)) beyond which the utterance is tier 3.  Until round 4 this
    // was 120: a guard against fp32 overflow of the composites only.  tools/fuzz_tiers.py found what it has to guard as well:
    // an utterance just under G3 (largest entry 203) whose maps stay large over a whole group came out of the two-level path
    // at 5 % error where the sequential recursion has 0.26 % and the flat scan 0.9 % -- the products cancel from ~2^115 down,
    // and neither an fp32 composite nor the fp64 chain behind it survives that.  104 sends it to tier 3 (error 2e-4) and moves
    // 4 of the recipe's 2 048 utterances with it (tier 3: 2 -> 6; at 112: 2, at 96: 8, at 80: 21).
    // Round 5: 96.  Another soak seed (tools/fuzz_tiers.py 120 101, case 114) has an utterance whose groups stay just under 104:
    // 4.7 x the sequential recursion's error through the two-level path (2.5e-3 against 5.2e-4), 0.8 x through the flat scan; with
    // the guard at 96 it is tier 3 and at 0.23 of the bound.  Two more of the recipe's 2 048 utterances go with it.
    static const float v = [] { const char* e = getenv("GOLF_SS_GROUP_LOG2"); return e ? (float)atof(e) : 96.f; }();
    return v;
}
static int hot_all_16ths() {
    // An utterance with a chunk beyond G1 at least this many sixteenths of whose chunks are beyond G2 is tier 3 (0: never).
    // Round 6: 16 -- hot from its first chunk to its last.  Every one of its maps is recomputed from fp64 trajectories anyway, so
    // what tier 3 adds is the fp64 boundary scan, and that is the one thing that takes such a row BELOW the sequential recursion's
    // error instead of to another realisation of it: tools/fuzz_tiers.py 120 606 case 90 (31 of 31 chunks hot, largest entry 44;
    // gradient of the gain at 3.9 x the serial kernels' error with every map accurate, one sweep, either scan).  The numerics lab
    // shows the same tail for accurate maps (tools/numlab/fail_rows.py: "flat all64 d1" 1.05 on another row): for rows whose
    // sequential error is already 3 - 20 x the 1e-4 target, "one more realisation of the rounding noise" is what a sweep converges to.
    static const int v = [] { const char* e = getenv("GOLF_SS_HOT_ALL_16THS"); return e ? atoi(e) : 16; }();
    return v;
}
static int hot_count() {
    // An utterance with at least this many chunks beyond G2 is treated like one with a chunk beyond G1 (0: never).
    // Round 6: 160.  tools/fuzz_tiers.py 120 31 case 11 row 12: no map beyond 24.9 -- tier 1 -- but 146 of 178 beyond 10 and a
    // sequential fp32 error of 1.7e-3; with fp32 maps ONE sweep does not contract there (lab: 1.1e-2 after one sweep, 1.5e-3 after
    // two, 9e-4 with accurate maps; device: 5.3e-3 / 8.1e-3 by scan).  What decides is the conditioning of the whole recursion, which
    // no per-chunk maximum shows (730 tier-1 rows of harsher-than-recipe tracks in the lab, tools/numlab/tier1_study.py: none above
    // 0.8 x the bound, whatever their counts); a long run of medium maps is the cheapest witness that catches the known case:
    // one more of the recipe's 1 024 utterances is hot for it.
    static const int v = [] { const char* e = getenv("GOLF_SS_HOT_COUNT"); return e ? atoi(e) : 160; }();
    return v;
}
static float phi_guard3() {
    static const float v = [] { const char* e = getenv("GOLF_SS_PHI_GUARD3"); return e ? (float)atof(e) : 256.f; }();
    return v;   // <= 0: no utterance is ever tier 3 (dev knob)
}
// rows of 16 utterances are addressed through one 32-bit buffer descriptor (serial kernels)
static bool serial_strides_ok(int64_t s0, int64_t s1) { return s0 < (1 << 24) && s1 < (1 << 24); }
constexpr unsigned kTierHot = 2u, kTierPrecise = 3u;
// Which boundary scan the forward ran is recorded behind the tier words ([2B]); the backward's first kernel compares it with
// its own and raises [2B + 1], which golf_ltv_allpole_status_u32 reports: a C caller that hands the backward other scan
// flags than the forward (or a workspace some other forward filled) would otherwise read composites nobody wrote.
constexpr unsigned kScanTwoLevel = 0x2C0DE001u, kScanFlat = 0x2C0DE002u;
__device__ __forceinline__ void record_scan_kind(const unsigned* tier, int B, unsigned kind) {
    if (tier) { unsigned* w = const_cast<unsigned*>(tier); w[2 * B] = kind; w[2 * B + 1] = 0u; }
}
__device__ __forceinline__ void check_scan_kind(const unsigned* tier, int B, unsigned kind) {
    if (tier && tier[2 * B] != kind) const_cast<unsigned*>(tier)[2 * B + 1] = 1u;
}
// tier words: tier[2 b] = 0 / 2 / 3, tier[2 b + 1] = number of hot chunks (wave-uniform reads: b is)
__device__ __forceinline__ bool tier3(const unsigned* __restrict__ tier, int b) {
    return tier != nullptr && __builtin_amdgcn_readfirstlane((int)tier[2 * b]) == (int)kTierPrecise;
}

// ------------------------------------------------------------------------------------------
// Tap-parallel in-register recursion (fp32): a QUAD of 4 lanes runs one chunk, 16 chunks per wave.
//   Lane r of the quad owns taps [r*TPL, (r+1)*TPL) and a TPL-deep rotating window holding the history delayed
//   by r*TPL samples: w[k] ~ y[t-1-(r*TPL+k)].  Per sample: TPL coefficient FMAs + TPL dot FMAs, a 2-stage DPP
//   butterfly (v_add_f32 with quad_perm operands) for the tap sum, and a 1-lane DPP shift that hands each lane the
//   sample leaving its left neighbour's window (a 4-stage systolic delay line).  ~18 instructions per sample
//   instead of ~62 for the one-lane-per-chunk version: a lone wave issues roughly one instruction per 4-5 cycles
//   whatever it is, so instruction count IS the latency of these kernels.
// ------------------------------------------------------------------------------------------
//   MODE 0 (P1z): zero initial state, chunks c < NCQ=NP, final state -> out[(b*NCQ+c)*W + i]
//   MODE 1 (P3) : initial state S[(b*NCS+c)*64 + i], writes y[b][t]
//   MODE 2      : initial state S[(b*NCS+c)*64 + i], chunks c < NCQ=NP, final state -> out (refinement sweep)
//   MODE 3      : as MODE 2 but the defect alone, start states and defects in LDS (two-level scan, LS = true)
// The body is a device function of ONE wave (its LDS tiles are passed in, its only synchronisation is the wave-level
// LDS fence) so that it can also run as one of the four independent waves of lpc_p1fz_kernel's workgroups.
template <int W, int NT, int MODE, bool LS = false>
__device__ __forceinline__ void fwdq_body(const float* __restrict__ ex, int64_t ex_stride,
                                          const float* __restrict__ gain, const float* __restrict__ a,
                                          const float* __restrict__ S, float* __restrict__ out, int64_t y_stride, int T,
                                          int F, int M, int hop, int L, int NCQ, int NCS,
                                          const float* __restrict__ zin, float* __restrict__ xt,
                                          float* __restrict__ yt, int b, int cg, int lane,
                                          const float* lst = nullptr, float* ldl = nullptr,
                                          unsigned* __restrict__ nonfinite = nullptr) {
    // lst (two-level scan): the chunk start states of this wave's 16 chunks (+ the next one) in LDS, row stride 32,
    // instead of the scanned states S in HBM; ldl: the defects of MODE 3 are also left in LDS ([16][32])
    constexpr int TPL = quad_tpl(W, NT);
    constexpr bool WY = MODE == 1;   // the pass that writes y
    static_assert(MODE >= 0 && MODE <= 3 && (MODE != 3 || LS), "MODE 3 exists only with LDS-resident start states");
    constexpr int R = 16;
    using TL = Tile<W, R>;
    const int lq = lane / W, lr = lane % W;
    const int row = lane >> 2, r = lane & 3;
    const int c0 = cg * R;
    const int c = c0 + row;
    const bool mine = c < NCQ;
    const BufRow xrow(ex + (size_t)b * ex_stride, T);
    const BufRow yrow(WY ? out + (size_t)b * y_stride : nullptr, WY ? T : 0);
    float w[TPL];
    if (MODE >= 1 && mine) {   // MODE 1, 2, 3 start from the scanned state
        if constexpr (LS) {   // (LDS and HBM pointers are kept in separate code paths: no pointer selects)
#pragma unroll
            for (int k = 0; k < TPL; ++k) w[TPL - 1 - k] = lst[row * 32 + r * TPL + k];
        } else {
            const float* sp = S + ((size_t)b * NCS + c) * 64 + r * TPL;
#pragma unroll
            for (int k = 0; k < TPL; ++k) w[TPL - 1 - k] = sp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < TPL; ++k) w[k] = 0.f;
    }
    float a0[TPL], dd[TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) { a0[k] = 0.f; dd[k] = 0.f; }
    float g0 = 0.f, dg = 0.f;
    const float inv_hop = 1.0f / (float)hop;
    int fcur = -1;
    const int nblk = L / W;
    float nx[TL::ITS];
    bool bad = false;   // a non-finite output sample went to y (status word of the boundary, include/golf_amd.h)
    TL::fetch(nx, xrow, c0 * L, L, lq, lr);
    for (int blk = 0; blk < nblk; ++blk) {
        const int tw = c0 * L + blk * W;  // block start of the wave's first chunk
        if (tw >= T) break;               // wave-uniform: nothing left for any lane
        TL::scatter(xt, nx, lq, lr);
        wave_lds_fence();
        float xin[W];
        TL::rows_load(xin, xt, row);
        TL::fetch(nx, xrow, tw + W, L, lq, lr);  // prefetch next block (past the end: hardware returns 0)
        const int t0 = c * L + blk * W;
        const bool act = mine && t0 < T;
        float keep[W / 4];
#pragma unroll
        for (int j = 0; j < W / 4; ++j) keep[j] = 0.f;
        if (act) {
            int f = t0 / hop;
            if (f > F - 2) f = F - 2;
            if (f != fcur) {
                fcur = f;
                const float* pa0 = a + ((size_t)b * F + f) * M;
                const float* pa1 = pa0 + M;
#pragma unroll
                for (int k = 0; k < TPL; ++k) {
                    const int i = r * TPL + k;
                    const float v0 = i < M ? pa0[i] : 0.f;
                    const float v1 = i < M ? pa1[i] : 0.f;
                    a0[k] = v0;
                    dd[k] = (v1 - v0) * inv_hop;
                }
                g0 = gain[(size_t)b * F + f];
                dg = (gain[(size_t)b * F + f + 1] - g0) * inv_hop;
            }
            const float n0 = (float)(t0 - f * hop);
#pragma unroll
            for (int s = 0; s < W; ++s) {
                const float n = n0 + (float)s;
                const float x = xin[s] * fmaf(n, dg, g0);
                float cf[TPL];
#pragma unroll
                for (int k = 0; k < TPL; ++k) cf[k] = fmaf(n, dd[k], a0[k]);  // all coefficients first (latency)
                float pa = 0.f, pb = 0.f;
#pragma unroll
                for (int k = TPL - 1; k >= 1; --k) {
                    const int slot = (s - 1 - k + 4 * TPL) % TPL;
                    if (k & 1) pa = fmaf(cf[k], w[slot], pa);
                    else       pb = fmaf(cf[k], w[slot], pb);
                }
                float part = fmaf(cf[0], w[(s - 1 + TPL) % TPL], pa + pb);  // newest sample last: shortest chain
                part += dppf<DPP_XOR1>(part);
                part += dppf<DPP_XOR2>(part);
                const float y = x - part;
                const float oldest = w[s % TPL];
                const float inc = dppf<DPP_SHR1>(oldest);
                w[s % TPL] = r == 0 ? y : inc;
                if (WY) keep[s >> 2] = ((s & 3) == r) ? y : keep[s >> 2];
            }
        }
        if (WY) {
#pragma unroll
            for (int j = 0; j < W / 4; ++j) yt[row * TL::LD + 4 * j + r] = keep[j];
            wave_lds_fence();
            float o[TL::ITS];
            TL::gather(o, yt, lq, lr);
            TL::store(o, yrow, tw, L, lq, lr);
#pragma unroll
            for (int it = 0; it < TL::ITS; ++it) bad = bad || !(fabsf(o[it]) <= 3.4028235e38f);
        }
        wave_lds_fence();
    }
    if (WY && nonfinite && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicOr(nonfinite, 1u);
    if (!WY && mine) {
        float* zp = out + ((size_t)b * NCQ + c) * W;
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            const int i = r * TPL + k;
            if (i < W) {
                float v = i < M ? w[TPL - 1 - k] : 0.f;
                // MODE 2 / 3 (refinement sweep): the chunk was re-run from the first-pass state S1_c, v = its true end
                // state E_c; what leaves is the DEFECT E_c - S1_{c+1}.  The second scan propagates only the correction
                // (delta_{c+1} = Phi_c delta_c + d_c) and the final states are S1 + delta: one Parareal iteration in
                // delta form -- the maps' rounding acts on a quantity that is already ~1e-4 of the state, so the result
                // is second order in every error of the coarse propagator (tools/numlab: rescanning z + d from scratch
                // instead leaves the first-order rounding of Phi s in the states, 3-10 x a sequential recursion's error).
                if (MODE == 2) v -= S[((size_t)b * NCS + c + 1) * 64 + i];
                if constexpr (MODE == 3) {
                    v -= lst[(row + 1) * 32 + i];
                    ldl[row * 32 + i] = v;
                    if (!out) continue;   // wave-uniform (merged chunk pass: the defects stay in LDS)
                }
                if constexpr (MODE == 0) {   // zero-state pass inside the pre-pass launch: z also stays in LDS for the group scan
                    if (ldl) ldl[row * 32 + i] = v;
                }
                zp[i] = v;
            }
        }
    }
}

template <int W, int NT, int MODE>
__global__ __launch_bounds__(64) void lpc_fwdq_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                      const float* __restrict__ gain, const float* __restrict__ a,
                                                      const float* __restrict__ S, float* __restrict__ out,
                                                      int64_t y_stride, int T, int F, int M, int hop, int L, int NCQ,
                                                      int NCS, const float* __restrict__ zin,
                                                      const unsigned* __restrict__ tier = nullptr) {
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[MODE == 1 ? TL::SIZE : 1];
    if (MODE == 2 && tier3(tier, blockIdx.y)) return;   // tier-3 utterances take no refinement sweep (see phi_guard)
    fwdq_body<W, NT, MODE>(ex, ex_stride, gain, a, S, out, y_stride, T, F, M, hop, L, NCQ, NCS, zin, xt, yt,
                           blockIdx.y, blockIdx.x, threadIdx.x);
}

// ------------------------------------------------------------------------------------------
// Batch-parallel SERIAL variant (large batches; the north_star's "serial sample recursion in-lane, batch x channel
// across wavefronts"): a quad of 4 lanes runs ONE WHOLE utterance from t = 0 to T, 16 utterances per wave, B/16 waves.
// Same tap-parallel systolic inner loop as fwdq_body; what differs is the data movement: the wave's 16 rows belong to
// 16 utterances (row stride = the tensor's row stride, one buffer descriptor over the 16 rows, out-of-range elements
// get offset -1 = out of bounds -> the hardware returns 0 / drops the store), and the frame parameters of frame f+2 are
// loaded while frame f is being processed (a lone wave would otherwise stall ~1 us on dependent loads at each of the
// 200 frame boundaries).  No transition matrices, no scan, no redundant arithmetic: 1x the reference's FMA count.
// ------------------------------------------------------------------------------------------
// Round 5: LPU lanes per utterance, 4 or 8.  A lone wave issues one instruction per ~7 cycles whatever it is, so a wave's time per
// sample is its instruction count: 6 + 6 FMAs + 2 butterfly adds + 5 with a quad, 3 + 3 + 3 + 5 with eight lanes (the third
// butterfly step is row_half_mirror; the history shifts by row_shr:1, lane 0 of each group being overwritten anyway).  Eight
// lanes halve the utterances per wave, which costs nothing while there are fewer waves than SIMDs (B < 8192): the serial
// filter's ~3.0 ms per batch becomes ~2.1.
// (one wave = `unit`: utterances (64 / LPU) unit .. + 64 / LPU - 1)
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {   // row-level DPP move (row_shr / row_half_mirror): every lane has a source or reads 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// STATE (golf_ltv_allpole_fwd_state_f32): y[<0] comes from state (B, M), state[b][i] = y[b][-1-i], loaded into the ring before the
// time loop; after it the block's last M outputs (read back from y) replace it.  The time loop itself is the same either way.
template <int W, int NT, int LPU, bool STATE = false>
__device__ __forceinline__ void serial_fwd_unit(int unit, float* __restrict__ xt, float* __restrict__ yt,
                                                const float* __restrict__ ex, int64_t ex_stride,
                                                const float* __restrict__ gain, const float* __restrict__ a,
                                                float* __restrict__ y, int64_t y_stride, int B, int T, int F, int M,
                                                int hop, float* state = nullptr) {
    static_assert(LPU == 4 || LPU == 8, "a quad or half a DPP row per utterance");
    constexpr int ROWS = 64 / LPU;
    constexpr int TPL = LPU == 4 ? quad_tpl(W, NT) : (NT + LPU - 1) / LPU;
    static_assert(W % LPU == 0 && W % TPL == 0, "the unrolled block is whole turns of the history ring and of the output slots");
    using TL = Tile<W, ROWS>;
    const int lane = threadIdx.x & 63;
    const int lq = lane / W, lr = lane % W;
    const int row = lane / LPU, r = lane % LPU;
    const int b0 = unit * ROWS;
    if (b0 >= B) return;   // wave-uniform
    const int nrow = B - b0 < ROWS ? B - b0 : ROWS;
    const int b = b0 + (row < nrow ? row : nrow - 1);  // idle groups shadow the last utterance; their stores are masked
    const int xs = (int)ex_stride, ys = (int)y_stride;
    const BufRow xblk(ex + (size_t)b0 * ex_stride, nrow * xs);
    const BufRow yblk(y + (size_t)b0 * y_stride, nrow * ys);
    auto fetch = [&](float (&v)[TL::ITS], int t0) {
#pragma unroll
        for (int it = 0; it < TL::ITS; ++it) {
            int rw, col;
            TL::rowcol(it, lq, lr, rw, col);
            const int t = t0 + col;
            v[it] = xblk.ld((t < T && rw < nrow) ? rw * xs + t : -1);
        }
    };
    auto load_row = [&](float (&dst)[TPL], int f) {
        const float* pa = a + ((size_t)b * F + f) * M;
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            const int i = r * TPL + k;
            dst[k] = pa[i < M ? i : 0];
            if (i >= M) dst[k] = 0.f;
        }
    };
    const float inv_hop = 1.0f / (float)hop;
    float w[TPL], a0[TPL], a1[TPL], an[TPL], dd[TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) w[k] = 0.f;
    if constexpr (STATE) {   // tap i = r*TPL + k reads slot (s-1-k) mod TPL of lane r: at s = 0 that holds y[-1-i]
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            const int i = r * TPL + k;
            w[TPL - 1 - k] = i < M ? state[(size_t)b * M + i] : 0.f;
        }
    }
    int f = 0, n0 = 0;
    load_row(a0, 0);
    load_row(a1, 1);
    load_row(an, F > 2 ? 2 : F - 1);
    const float* gb = gain + (size_t)b * F;
    float g0 = gb[0], g1 = gb[1], gn = gb[F > 2 ? 2 : F - 1];
    float dg = (g1 - g0) * inv_hop;
#pragma unroll
    for (int k = 0; k < TPL; ++k) dd[k] = (a1[k] - a0[k]) * inv_hop;
    float nx[TL::ITS];
    fetch(nx, 0);
    for (int t0 = 0; t0 < T; t0 += W) {
        TL::scatter(xt, nx, lq, lr);
        wave_lds_fence();
        float xin[W];
        TL::rows_load(xin, xt, row);
        fetch(nx, t0 + W);
        if (n0 == hop && f < F - 2) {   // frame boundary (wave-uniform): rotate the parameter rows, prefetch frame f+2
            ++f;
            n0 = 0;
#pragma unroll
            for (int k = 0; k < TPL; ++k) { a0[k] = a1[k]; a1[k] = an[k]; dd[k] = (a1[k] - a0[k]) * inv_hop; }
            g0 = g1; g1 = gn; dg = (g1 - g0) * inv_hop;
            const int fn = f + 2 < F ? f + 2 : F - 1;
            load_row(an, fn);
            gn = gb[fn];
        }
        float keep[W / LPU];
#pragma unroll
        for (int j = 0; j < W / LPU; ++j) keep[j] = 0.f;
        const float nb = (float)n0;
#pragma unroll
        for (int s = 0; s < W; ++s) {
            const float n = nb + (float)s;
            const float x = xin[s] * fmaf(n, dg, g0);
            float cf[TPL];
#pragma unroll
            for (int k = 0; k < TPL; ++k) cf[k] = fmaf(n, dd[k], a0[k]);
            float pa = 0.f, pb = 0.f;
#pragma unroll
            for (int k = TPL - 1; k >= 1; --k) {
                const int slot = (s - 1 - k + 4 * TPL) % TPL;
                if (k & 1) pa = fmaf(cf[k], w[slot], pa);
                else       pb = fmaf(cf[k], w[slot], pb);
            }
            float part = fmaf(cf[0], w[(s - 1 + TPL) % TPL], pa + pb);
            part += dppf<DPP_XOR1>(part);
            part += dppf<DPP_XOR2>(part);
            if (LPU == 8) part += dpp_row<0x141>(part);          // row_half_mirror: lane i <-> 7 - i, the other quad's sum
            const float yv = x - part;
            const float oldest = w[s % TPL];
            const float inc = LPU == 4 ? dppf<DPP_SHR1>(oldest) : dpp_row<0x111>(oldest);   // row_shr:1
            w[s % TPL] = r == 0 ? yv : inc;
            keep[s / LPU] = ((s % LPU) == r) ? yv : keep[s / LPU];
        }
        n0 += W;
#pragma unroll
        for (int j = 0; j < W / LPU; ++j) yt[row * TL::LD + LPU * j + r] = keep[j];
        wave_lds_fence();
        float o[TL::ITS];
        TL::gather(o, yt, lq, lr);
#pragma unroll
        for (int it = 0; it < TL::ITS; ++it) {
            int rw, col;
            TL::rowcol(it, lq, lr, rw, col);
            const int t = t0 + col;
            yblk.st((t < T && rw < nrow) ? rw * ys + t : -1, o[it]);
        }
        wave_lds_fence();
    }
    if constexpr (STATE) {
        // the ring ran on past T inside the last W-block, so the new state is read back from y: y[T-1-i], or for T < M the
        // old state shifted in.  Every read of the row is issued before its first write (one wave owns the row).
        __threadfence();
        constexpr int NS = (NT + LPU - 1) / LPU;
        float v[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = r + j * LPU;
            v[j] = i < M ? (i < T ? y[(size_t)b * y_stride + (T - 1 - i)] : state[(size_t)b * M + (i - T)]) : 0.f;
        }
        if (row < nrow) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int i = r + j * LPU;
                if (i < M) state[(size_t)b * M + i] = v[j];
            }
        }
    }
}

template <int W, int NT, int LPU>
__global__ __launch_bounds__(256) void lpc_serial_fwd_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                            const float* __restrict__ gain,
                                                            const float* __restrict__ a, float* __restrict__ y,
                                                            int64_t y_stride, int B, int T, int F, int M, int hop) {
    using TL = Tile<W, 64 / LPU>;
    // workgroups of 4 INDEPENDENT waves (one per SIMD of a CU; they never synchronise): single-wave workgroups are
    // placed unevenly by the dispatcher once there are about as many waves as SIMDs (measured on the transition kernel)
    __shared__ float xt_all[4][TL::SIZE];
    __shared__ float yt_all[4][TL::SIZE];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    serial_fwd_unit<W, NT, LPU>(blockIdx.x * 4 + wv, xt_all[wv], yt_all[wv], ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop);
}

template <int W, int NT, int LPU>
__global__ __launch_bounds__(256) void lpc_serial_fwd_state_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                                  const float* __restrict__ gain,
                                                                  const float* __restrict__ a, float* __restrict__ y,
                                                                  int64_t y_stride, int B, int T, int F, int M, int hop,
                                                                  float* state) {
    using TL = Tile<W, 64 / LPU>;
    __shared__ float xt_all[4][TL::SIZE];
    __shared__ float yt_all[4][TL::SIZE];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    serial_fwd_unit<W, NT, LPU, true>(blockIdx.x * 4 + wv, xt_all[wv], yt_all[wv], ex, ex_stride, gain, a, y, y_stride, B, T, F,
                                      M, hop, state);
}

// Final pass of the flat-scan path: every chunk runs from its boundary state S_c (first pass + correction, or the fp64
// scan of a tier-3 utterance) and writes y.
template <int W, int NT>
__global__ __launch_bounds__(64) void lpc_fwdq_final_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                            const float* __restrict__ gain,
                                                            const float* __restrict__ a, const float* __restrict__ S,
                                                            float* __restrict__ y, int64_t y_stride, int T, int F, int M,
                                                            int hop, int L, int NC, unsigned* __restrict__ nonfinite) {
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[TL::SIZE];
    fwdq_body<W, NT, 1>(ex, ex_stride, gain, a, S, y, y_stride, T, F, M, hop, L, NC, NC, nullptr, xt, yt, blockIdx.y,
                        blockIdx.x, threadIdx.x, nullptr, nullptr, nonfinite);
}

// Serial adjoint (backward of the above): the transposed-form recursion of lpc_adjq_kernel run over the whole utterance
// in reverse time, lam(T) = 0, writes g[b][t] = dL/dy_total; the parallel gradient kernels (lpc_grad_corr / _reduce)
// follow unchanged.  Parameter rows are prefetched one frame ahead in the direction of travel (frame f-1).
template <int W, int NT>
__global__ __launch_bounds__(256) void lpc_serial_adj_kernel(const float* __restrict__ gy, int64_t gy_stride,
                                                            const float* __restrict__ a, float* __restrict__ g,
                                                            int64_t g_stride, int B, int T, int F, int M, int hop) {
    constexpr int TPL = quad_tpl(W, NT);
    using TL = Tile<W, 16>;
    // workgroups of 4 INDEPENDENT waves (one per SIMD of a CU; they never synchronise): single-wave workgroups are
    // placed unevenly by the dispatcher once there are about as many waves as SIMDs (measured on the transition kernel)
    __shared__ float xt_all[4][TL::SIZE];
    __shared__ float yt_all[4][TL::SIZE];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xt = xt_all[wv];
    float* yt = yt_all[wv];
    const int lane = threadIdx.x & 63;
    const int lq = lane / W, lr = lane % W;
    const int row = lane >> 2, r = lane & 3;
    const int b0 = (blockIdx.x * 4 + wv) * 16;
    if (b0 >= B) return;   // wave-uniform
    const int nrow = B - b0 < 16 ? B - b0 : 16;
    const int b = b0 + (row < nrow ? row : nrow - 1);
    const int xs = (int)gy_stride, ys = (int)g_stride;
    const BufRow xblk(gy + (size_t)b0 * gy_stride, nrow * xs);
    const BufRow yblk(g + (size_t)b0 * g_stride, nrow * ys);
    auto fetch = [&](float (&v)[TL::ITS], int t0) {
#pragma unroll
        for (int it = 0; it < TL::ITS; ++it) {
            int rw, col;
            TL::rowcol(it, lq, lr, rw, col);
            const int t = t0 + col;
            v[it] = xblk.ld((t0 >= 0 && t < T && rw < nrow) ? rw * xs + t : -1);
        }
    };
    auto load_row = [&](float (&dst)[TPL], int f) {
        const float* pa = a + ((size_t)b * F + f) * M;
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            const int i = r * TPL + k;
            dst[k] = pa[i < M ? i : 0];
            if (i >= M) dst[k] = 0.f;
        }
    };
    const float inv_hop = 1.0f / (float)hop;
    float p[TPL], a0[TPL], a1[TPL], an[TPL], dd[TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) p[k] = 0.f;
    int t0 = ((T - 1) / W) * W;
    int f = t0 / hop;
    if (f > F - 2) f = F - 2;
    int n0 = t0 - f * hop;
    load_row(a0, f);
    load_row(a1, f + 1);
    load_row(an, f > 0 ? f - 1 : 0);
#pragma unroll
    for (int k = 0; k < TPL; ++k) dd[k] = (a1[k] - a0[k]) * inv_hop;
    float nx[TL::ITS];
    fetch(nx, t0);
    for (; t0 >= 0; t0 -= W) {
        TL::scatter(xt, nx, lq, lr);
        wave_lds_fence();
        float gin[W];
        TL::rows_load(gin, xt, row);
        fetch(nx, t0 - W);
        if (n0 < 0) {   // crossed into frame f-1 (wave-uniform)
            --f;
            n0 += hop;
#pragma unroll
            for (int k = 0; k < TPL; ++k) { a1[k] = a0[k]; a0[k] = an[k]; dd[k] = (a1[k] - a0[k]) * inv_hop; }
            load_row(an, f > 0 ? f - 1 : 0);
        }
        float keep[W / 4];
#pragma unroll
        for (int j = 0; j < W / 4; ++j) keep[j] = 0.f;
        const float nb = (float)n0;
#pragma unroll
        for (int s = W - 1; s >= 0; --s) {
            const int st = W - 1 - s;
            const float n = nb + (float)s;
            const float head = p[st % TPL];
            const float gv = dppf<DPP_BC0>(gin[s] + head);
            float inc = dppf<DPP_SHL1>(head);
            inc = r == 3 ? 0.f : inc;
#pragma unroll
            for (int k = 0; k < TPL - 1; ++k) {
                const float cf = fmaf(n, dd[k], a0[k]);
                p[(k + st + 1) % TPL] = fmaf(-cf, gv, p[(k + st + 1) % TPL]);
            }
            const float cfl = fmaf(n, dd[TPL - 1], a0[TPL - 1]);
            p[st % TPL] = fmaf(-cfl, gv, inc);
            keep[s >> 2] = ((s & 3) == r) ? gv : keep[s >> 2];
        }
        n0 -= W;
#pragma unroll
        for (int j = 0; j < W / 4; ++j) yt[row * TL::LD + 4 * j + r] = keep[j];
        wave_lds_fence();
        float o[TL::ITS];
        TL::gather(o, yt, lq, lr);
#pragma unroll
        for (int it = 0; it < TL::ITS; ++it) {
            int rw, col;
            TL::rowcol(it, lq, lr, rw, col);
            const int t = t0 + col;
            yblk.st((t < T && rw < nrow) ? rw * ys + t : -1, o[it]);
        }
        wave_lds_fence();
    }
}

// ------------------------------------------------------------------------------------------
// P1h: homogeneous trajectories in fp64 -> transition matrix of chunk q = b*NP + c, stored twice:
//   Phi [q][j][i] (row j contiguous: adjoint scan reads rows)   = d s_end[i] / d s_start[j]
//   PhiT[q][i][j] (row i contiguous: forward scan reads rows)
//   lane = flat chunk q;  `pair` selects trajectories (2*pair, 2*pair+1)
// ------------------------------------------------------------------------------------------
// trajectories per lane: KT = 3 (launch_transitions).  B=32: 22 trajectories / KT groups x 100 chunk blocks =
// 2200 / 1100 / 800 waves of relative length 0.67 / 1 / 1.33 on 1024 SIMDs for KT = 1 / 2 / 3: only KT=3 fits one wave
// per SIMD.

template <int W, int NT, int KT, typename R>
__device__ __forceinline__ void p1_hom_body(int qblk, int grp, const float* __restrict__ a, float* __restrict__ Phi,
                                            float* __restrict__ PhiT, int F, int M, int hop, int L, int NP, int nq) {
    const int q = qblk * 64 + (threadIdx.x & 63);
    if (q >= nq) return;
    const int jb = KT * grp;  // trajectories jb .. jb+KT-1
    if (jb >= M) {            // padding rows/columns: exact zeros
#pragma unroll
        for (int r = 0; r < KT; ++r) {
            const int j = jb + r;
            if (j < NT) {
                float* o = Phi + ((size_t)q * NT + j) * W;
#pragma unroll
                for (int i = 0; i < W; ++i) o[i] = 0.f;
            }
        }
        return;
    }
    const int b = q / NP, c = q - b * NP;
    R h[KT][W];
#pragma unroll
    for (int r = 0; r < KT; ++r)
#pragma unroll
        for (int k = 0; k < W; ++k) h[r][k] = (W - 1 - k == jb + r && jb + r < M) ? (R)1 : (R)0;
    R a0[NT], dd[NT];
    const R inv_hop = (R)1 / (R)hop;
    int fcur = -1;
    const int nblk = L / W;
    for (int blk = 0; blk < nblk; ++blk) {
        const int t0 = c * L + blk * W;
        const int f = t0 / hop;  // <= F-2: chunks with a transition matrix end before (F-1)*hop
        if (f != fcur) {
            fcur = f;
            // (unconditional loads from a clamped index, the select after the conversion: see fixup_wave)
            const float* pa0 = a + ((size_t)b * F + f) * M;
            const float* pa1 = pa0 + M;
            float u0[NT], u1[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int ic = i < M ? i : M - 1;
                u0[i] = pa0[ic];
                u1[i] = pa1[ic];
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const R w0 = (R)u0[i], w1 = (R)u1[i];
                const R v0 = i < M ? w0 : (R)0, v1 = i < M ? w1 : (R)0;
                a0[i] = v0;
                dd[i] = (v1 - v0) * inv_hop;
            }
        }
        const R n0 = (R)(t0 - f * hop);
#pragma unroll
        for (int s = 0; s < W; ++s) {
            const R n = n0 + (R)s;
            R ra[KT], rb[KT];
#pragma unroll
            for (int r = 0; r < KT; ++r) { ra[r] = (R)0; rb[r] = (R)0; }
            // The interpolated coefficient is produced PD taps before it is consumed: hipcc otherwise places each
            // `cf = __builtin_elementwise_fma(n,dd,a0)` right in front of its uses and every tap eats the fp64 FMA latency (measured:
            // 11.6 cycles per FMA instead of 4.8).  sched_barrier pins the order written here.
            constexpr int PD = 2;
            R cfq[PD];
#pragma unroll
            for (int j = 0; j < PD; ++j) cfq[j] = __builtin_elementwise_fma(n, dd[NT - 1 - j], a0[NT - 1 - j]);
#pragma unroll
            for (int i = NT - 1; i >= 1; --i) {
                const R cf = cfq[(NT - 1 - i) % PD];
                if (i - PD >= 0) cfq[(NT - 1 - i) % PD] = __builtin_elementwise_fma(n, dd[i - PD], a0[i - PD]);
                const int slot = (s - 1 - i + 2 * W) % W;
#pragma unroll
                for (int r = 0; r < KT; ++r) {
                    if (i & 1) ra[r] = __builtin_elementwise_fma(cf, h[r][slot], ra[r]);
                    else       rb[r] = __builtin_elementwise_fma(cf, h[r][slot], rb[r]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            const R cf0 = cfq[(NT - 1) % PD];
            const int sp = (s - 1 + W) % W;
#pragma unroll
            for (int r = 0; r < KT; ++r) h[r][s] = __builtin_elementwise_fma(-cf0, h[r][sp], -(ra[r] + rb[r]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int r = 0; r < KT; ++r) {
        const int j = jb + r;
        if (j < NT) {
            float* o = Phi + ((size_t)q * NT + j) * W;
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = (i < M && j < M) ? (float)h[r][W - 1 - i] : 0.f;
        }
    }
}

// (p1f_body -- the fp32 transition-map trajectories, four per lane as two float2 rings -- lives in lpc_p1f.h since round 6)
// (Round 4 built the same trajectories with TWO per lane -- one float2 ring, 11 lanes per chunk and no padding trajectories, 114
// VGPRs, 1 116 waves -- and measured it: alone in its launch 43.8 us against 37.7 (279 workgroups on 256 CUs: the doubled CUs
// are the tail, and 1 100 lane-sets can never be <= 1 024 waves), four batches in flight 71.3 against 69.2 us/step.  Removed;
// commit 37966e3 has it.)
// Register allocation of the transition kernel, measured with 4 batches in flight (tools/ab2.sh r14_ab / r15_ab): 172 VGPRs (what
// hipcc takes: two such waves fit a SIMD) 69.1 - 69.4 us/step; capped at 168 (three fit) 71.1 - 71.5 -- transition waves of
// different batches stacked three deep are worse than queued; padded to 264 (one per SIMD) 68.9 - 69.1: no gain.  Left alone.
template <int W, int NT, int NR = 2>
__global__ __launch_bounds__(64 * P1F_WPB) void lpc_p1f_kernel(const float* __restrict__ a, float* __restrict__ PhiT,
                                                               int F, int M, int hop, int L, int NP, int nq,
                                                               float* __restrict__ pmax, unsigned* __restrict__ fixcnt,
                                                               int B, float* __restrict__ Phi) {
    __shared__ __attribute__((aligned(16))) float tile_all[P1fGeom<W, NT, NR>::TILE_FLOATS];
    p1f_body<W, NT, NR>(a, PhiT, F, M, hop, L, NP, nq, tile_all, blockIdx.x, pmax, fixcnt, B, Phi);
}

// ------------------------------------------------------------------------------------------
// Tried and NOT adopted (round 3, verdict r2 #4; the kernel is in git history: commit f49862c, `p1m_body`): the fp32 maps on
// the MATRIX pipe -- v_mfma_f32_4x4x1_16b_f32 = 16 independent 4x4 outer products per instruction; a quad of lanes owns 4
// trajectories of a chunk and advances them 4 samples per block step: D[r][j] = sum_h cf_{h+r-1}[n+r] y_j[n-h] in NT
// instructions (A = the lane's coefficient for row r = lane & 3: 4 x fewer interpolations; B = the lane's own history ring),
// then the 4 x 4 triangular part in 6 VALU FMAs; the zero-state response rode in the chunk's spare 23rd trajectory (no P1z
// waves).  On paper 44 matrix-pipe cycles per sample per 64 trajectories against ~88 VALU-issue cycles.  MEASURED
// (tools/ubench/mfma_4x4x1_probe.hip): the 2-pass instruction sustains one issue per ~11.4 cycles, not 8, and VALU
// instructions of OTHER waves on the SIMD do not issue beside it -- 22 MFMAs + 38 VALU instructions per block step cost
// 400-420 SIMD cycles at 1..4 waves per SIMD (250 for the MFMAs alone), the SUM, against 375 for p1f_body's same work.  The
// kernel: 64.8 us (p1fz: 40.2), step 159 us alone / 87.9 pipelined (136 / 74.4); parity identical (every lpc_ss test passed).
// Also tried and NOT adopted: the zero-state response in the spare trajectory of p1f_body itself (M = 22 of 24: the .x half
// of group 5's hB ring; u = ex * gain staged per wave in the copy-out tile, one v_sub_f32 per sample) -- the 416 P1z waves
// and a tenth of the step's VALU instructions gone, parity green -- but the kernel took 46.9 us instead of 39.9 (staging
// prologue + 24 more live registers in waves that are the critical path; the P1z waves had been running on CUs the
// transition waves leave idle), the step 141.7 us alone instead of 134.6 and 74.2 us pipelined either way: the pipelined
// rate is NOT bound by the amount of VALU work (a finding that redirects the search: DESIGN.md 4.1).
// ------------------------------------------------------------------------------------------
// `upw` zero-state units (16 chunks of one utterance each) per wave, one after the other: the host picks upw so that the
// fused grid has no more workgroups than the device has CUs -- an extra workgroup would share the SIMDs of a CU whose
// transition waves are issue-bound.
template <int W, int NT>
__device__ __forceinline__ void p1z_units(const float* __restrict__ ex, int64_t ex_stride,
                                          const float* __restrict__ gain, const float* __restrict__ a,
                                          float* __restrict__ z, int T, int F, int M, int hop, int L, int NP, int ncg,
                                          int B, int upw, int zblk, float (*xt)[Tile<W, 16>::SIZE]) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    light_wave_priority();
    for (int u = 0; u < upw; ++u) {
        const int unit = (zblk * 4 + wv) * upw + u;
        if (unit >= ncg * B) return;  // wave-uniform; the waves of a workgroup never synchronise with each other
        fwdq_body<W, NT, 0>(ex, ex_stride, gain, a, nullptr, z, 0, T, F, M, hop, L, NP, NP, nullptr, xt[wv], nullptr,
                            unit / ncg, unit - (unit / ncg) * ncg, threadIdx.x & 63);
        wave_lds_fence();
    }
}

// Horizontal fusion of the two kernels that open the inference forward and do not depend on each other: the fp32
// transition matrices (needs only `a`; 637 issue-bound waves, one per SIMD of 160 CUs) and the zero-state pass P1z
// (416 light waves).  Workgroups [0, nblk_f) run p1f_body, the rest run four P1z units as four independent waves, so
// P1z uses the CUs the transition kernel leaves idle instead of a launch of its own after it.  (Forking P1z onto a
// second stream instead costs more in event record/wait than it hides: DESIGN.md.)
template <int W, int NT>
__global__ __launch_bounds__(64 * P1F_WPB) void lpc_p1fz_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                                const float* __restrict__ gain,
                                                                const float* __restrict__ a, float* __restrict__ z,
                                                                float* __restrict__ PhiT, int T, int F, int M, int hop,
                                                                int L, int NP, int nq, int nblk_f, int ncg, int B,
                                                                int upw, float* __restrict__ pmax,
                                                                unsigned* __restrict__ fixcnt, float* __restrict__ Phi) {
    using TL = Tile<W, 16>;
    __shared__ __attribute__((aligned(16))) float tile_all[P1fGeom<W, NT>::TILE_FLOATS];
    __shared__ float xt[P1F_WPB][TL::SIZE];
    if ((int)blockIdx.x < nblk_f) {
        p1f_body<W, NT>(a, PhiT, F, M, hop, L, NP, nq, tile_all, blockIdx.x, pmax, fixcnt, B, Phi);
    } else {
        p1z_units<W, NT>(ex, ex_stride, gain, a, z, T, F, M, hop, L, NP, ncg, B, upw, (int)blockIdx.x - nblk_f, xt);
    }
}

// The same fusion for the training path: fp64 transition trajectories (800 waves) beside the zero-state pass.
template <int W, int NT, int KT>
__global__ __launch_bounds__(256) void lpc_p1hz_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                       const float* __restrict__ gain, const float* __restrict__ a,
                                                       float* __restrict__ z, float* __restrict__ Phi,
                                                       float* __restrict__ PhiT, int T, int F, int M, int hop, int L,
                                                       int NP, int nq, int nblk_h, int ncg, int B, int upw) {
    using TL = Tile<W, 16>;
    __shared__ float xt[4][TL::SIZE];
    if ((int)blockIdx.x < nblk_h) {
        constexpr int NG = (NT + KT - 1) / KT;
        const int nqb = (nq + 63) / 64;
        const int unit = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int qblk = unit / NG, grp = unit - qblk * NG;
        if (qblk >= nqb) return;
        p1_hom_body<W, NT, KT, double>(qblk, grp, a, Phi, PhiT, F, M, hop, L, NP, nq);
    } else {
        p1z_units<W, NT>(ex, ex_stride, gain, a, z, T, F, M, hop, L, NP, ncg, B, upw, (int)blockIdx.x - nblk_h, xt);
    }
}

// Phi[q][j][i] -> PhiT[q][i][j] (training path: the fp64 kernel writes Phi with float4 stores; transposing here costs
// 27 MB of coalesced traffic instead of ~3 M scattered 4-byte stores inside the trajectory kernel: -28 us there).
template <int W, int NT>
__global__ __launch_bounds__(256) void lpc_transpose_kernel(const float* __restrict__ Phi, float* __restrict__ PhiT,
                                                            int nq, float* __restrict__ pmax,
                                                            unsigned* __restrict__ fixcnt, int B) {
    __shared__ float t[4][NT * (W + 1)];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (fixcnt && blockIdx.x == 0)   // counters of the fix-up that follows in the next launch (see fixup_wave)
        for (int e = threadIdx.x; e < 5 * B + 1; e += 256) fixcnt[e] = 0u;
    const int q = blockIdx.x * 4 + wv;
    if (q >= nq) return;
    const float* src = Phi + (size_t)q * NT * W;
    float* dst = PhiT + (size_t)q * NT * W;
    float* tt = t[wv];
    unsigned mx = 0u;   // largest |entry| as a bit pattern (NaN ranks above inf): the conditioning guard, see kPhiGuard
    for (int e = lane; e < NT * W; e += 64) {  // e = j*W + i
        const int j = e / W, i = e - j * W;
        const float v = src[e];
        tt[j * (W + 1) + i] = v;
        mx = max(mx, __float_as_uint(fabsf(v)));
    }
    if (pmax) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
        if (lane == 0) pmax[q] = __uint_as_float(mx);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < NT * W; e += 64) {  // e = i*W + j
        const int i = e / W, j = e - i * W;
        dst[e] = (j < NT) ? tt[j * (W + 1) + i] : 0.f;
    }
}

// (A variant that interpolates the coefficients once per chunk into an LDS tile and runs 3 trajectories per lane
// against it — 23 instead of 33 fp64 FMAs per trajectory-step — was measured SLOWER (84.7 vs 77.6 us): a lone wave
// already sustains one fp64 FMA per ~5.2 cycles (tools/ubench/fma_issue.hip), and the LDS reads, waits and
// producer bookkeeping cost more issue slots than the FMAs they saved.  See DESIGN.md.)
template <int W, int NT, int KT, typename R>
__global__ __launch_bounds__(256) void lpc_p1h_kernel(const float* __restrict__ a, float* __restrict__ Phi,
                                                      float* __restrict__ PhiT, int F, int M, int hop, int L, int NP,
                                                      int nq) {
    constexpr int NG = (NT + KT - 1) / KT;  // trajectory groups per chunk
    // Workgroups of 4 independent waves, unit = (block of 64 chunks, trajectory group).  Every wave is FMA-issue
    // bound, so two waves on one SIMD take twice as long: what matters is that the number of waves stays below the
    // 1024 SIMDs AND that they are spread one per SIMD, which a 4-wave workgroup per CU guarantees and single-wave
    // workgroups did not (see lpc_p1f_kernel).  The groups of one chunk block sit in the same / neighbouring
    // workgroups and share the coefficient rows of `a` in cache.
    const int nqb = (nq + 63) / 64;
    const int unit = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qblk = unit / NG, grp = unit - qblk * NG;
    if (qblk >= nqb) return;
    p1_hom_body<W, NT, KT, R>(qblk, grp, a, Phi, PhiT, F, M, hop, L, NP, nq);
}

// ------------------------------------------------------------------------------------------
// Conditioning tiers (see phi_guard): the fix-up of hot chunk maps.
//   Decision: every wave that needs it derives its utterance's tier from the per-chunk maxima the transition kernel left
//   (a few loads + wave reductions; all waves arrive at the same answer, nothing is communicated).
//   Work: unit = (chunk c, trajectory j), one QUAD of lanes per unit, 16 units per wave -- the tap-parallel systolic
//   recursion of fwdq_body in fp64 (lane r owns taps [r TPL, (r+1) TPL) and a TPL-deep window; per step TPL coefficient +
//   TPL dot FMAs, a 2-stage DPP butterfly, a 1-lane DPP shift): ~13 us per chunk instead of ~25 us with one lane per
//   trajectory.  A unit's quad ends with column j of the chunk's map: overwrites it in the fp32 map (rounded once) and,
//   for a tier-3 utterance, stores row j of the map kept as doubles.
//   Units are enumerated densely over ALL chunks (u = c NT + j) and dealt round-robin to the utterance's fix-up waves; a
//   wave skips a pass none of whose 16 units is hot, so a cluster of hot chunks spreads over consecutive waves.
//   `accurate` (training path: the maps already come from fp64 trajectories): only tier 3 is acted on.
// ------------------------------------------------------------------------------------------
struct UttTier { bool t2, t3; unsigned nhot; };

__device__ __forceinline__ UttTier utterance_tier(const float* __restrict__ pm, int NP, int lane, float g1, float g2,
                                                  float g3, int accurate, float glog, int hot16, int hotn) {
    unsigned umax = 0u;
    unsigned n = 0u;       // chunks beyond G2 (counted in the same pass over the maxima: every wave that derives a tier pays for it)
    bool ovf = false;
    for (int c0 = 0; c0 < NP; c0 += 64) {
        const int c = c0 + lane;
        const float v = c < NP ? fabsf(pm[c]) : 0.f;
        n += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(c < NP && !(v <= g2)));
        umax = max(umax, __float_as_uint(v));   // bit patterns: a NaN ranks above +inf and cannot hide
        // the product of a composite group's 16 maps must stay far from the fp32 range (sum of log2 of the maxima over the
        // group: c0 is a multiple of 64, so 16-lane rows are the groups of lpc_group_prepass_kernel)
        float lg = __log2f(fmaxf(v, 1.f));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) lg += __shfl_xor(lg, off);
        ovf = ovf || lg > glog;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) umax = max(umax, (unsigned)__shfl_xor((int)umax, off));
    UttTier d;
    d.t3 = g3 > 0.f && (!(__uint_as_float(umax) <= g3) || __builtin_amdgcn_ballot_w64(ovf) != 0ull);
    bool beyond_g1 = g1 > 0.f && !(__uint_as_float(umax) <= g1);   // some chunk beyond G1: chunks beyond G2 are hot
    d.nhot = 0u;
    // (round 6) ... or a long run of them: an utterance none of whose maps passes G1 but most of which pass G2 (see hot_count)
    if (!d.t3 && g1 > 0.f) beyond_g1 = beyond_g1 || (hotn > 0 && n >= (unsigned)hotn);
    d.t2 = !accurate && beyond_g1;
    if (!d.t3 && beyond_g1) {
        // (round 6) hot from end to end: with (nearly) every map recomputed anyway, the fp64 boundary scan is what is left of
        // tier 3's cost, and it is the only thing that takes such a row below the sequential recursion's error (see hot_all_16ths)
        if (g3 > 0.f && hot16 > 0 && n * 16u >= (unsigned)NP * (unsigned)hot16) d.t3 = true;
        else if (d.t2) d.nhot = n;
    }
    if (d.t3) d.nhot = (unsigned)NP;
    return d;
}

// 64-bit DPP = two 32-bit DPP moves (v_add_f64 takes no DPP operand).  bound_ctrl: no `old` value has to be materialised.
template <int CTRL>
__device__ __forceinline__ double dppd(double v) {
    const long long x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
struct FixArgs {
    const float* a;      // (B, F, M) coefficients
    float* PhiT;         // fp32 maps [b][c][i][j]
    float* Phi;          // the same maps as [b][c][j][i] (training with fp32 trajectories: the backward's orientation), or null
    double* Phi64;       // maps as doubles [b][c][j][i] (tier 3 only)
    const float* pmax;   // largest |entry| per chunk, from the transition kernel
    unsigned* tier;      // [b][2]: tier, hot chunks
    unsigned* status;    // [0] non-finite output of the forward (reset by its first boundary-scan kernel)
    unsigned* fixcnt;    // [b]: fix-up units completed, [B + b]: units claimed, [2 B]: a wait for the fix-up ran out (all zeroed by
                         // the transition kernel, i.e. once per set of maps: a handle reused for several forwards keeps reporting it)
    int F, M, hop, L, NP, B;
    float g1, g2, g3, glog;
    int hot16, hotn;     // hot_all_16ths(), hot_count()
    int accurate;
};

// One wave of utterance b's fix-up.  Units (hot chunk, trajectory) are CLAIMED 16 at a time from a per-utterance counter, so
// any number of waves can share the work in any order: the workgroups that lead the grid guarantee that it gets done
// (they are resident or finished before any wave that waits for them starts), the ones that trail the grid only make it
// faster when there is room for them.  `hotlist`: the wave's own LDS scratch for the compact list of hot chunks.
constexpr int kHotListMax = 512;    // chunks per utterance the compact list holds (ushort); longer utterances enumerate all chunks
                                    // (4 lists x 1 KB + the composites' 8 KB = 12 KB: the pre-pass fits a CU beside two oscillator workgroups)
// Stores of the fix-up go THROUGH to memory (agent-scope stores): their readers are waves of the same launch on any XCD, and the
// alternative -- an agent-scope release fence per fix-up wave -- writes back the whole L2 of the XCD each time (round 5).
// (Same box, alternating, one of the four slots holding a hot utterance: 68.8 - 69.2 -> 68.5 - 69.0 us/step.)
template <typename T> __device__ __forceinline__ void st_through(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int W, int NT>
__device__ __forceinline__ void fixup_wave(const FixArgs& fa, int b, bool writes_tier, unsigned short* __restrict__ hotlist) {
    constexpr int TPL = quad_tpl(W, NT);
    const int lane = threadIdx.x & 63;
    const int row = lane >> 2, r = lane & 3;
    const int NP = fa.NP, M = fa.M, F = fa.F, hop = fa.hop, L = fa.L;
    const float* pm = fa.pmax + (size_t)b * NP;
    const UttTier d = utterance_tier(pm, NP, lane, fa.g1, fa.g2, fa.g3, fa.accurate, fa.glog, fa.hot16, fa.hotn);
    if (writes_tier && lane == 0) {
        fa.tier[2 * b] = d.t3 ? kTierPrecise : (d.t2 ? kTierHot : 0u);
        fa.tier[2 * b + 1] = d.nhot;
    }
    if (d.nhot == 0u) return;   // wave-uniform: the common case ends here
    const bool listed = NP <= kHotListMax;
    if (listed) {   // compact list of the hot chunks (every wave builds its own: a few ballots)
        int base = 0;
        for (int c0 = 0; c0 < NP; c0 += 64) {
            const int c = c0 + lane;
            const bool h = c < NP && (d.t3 || !(fabsf(pm[c < NP ? c : 0]) <= fa.g2));
            const unsigned long long m = __builtin_amdgcn_ballot_w64(h);
            const int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (h) hotlist[base + pre] = (unsigned short)c;
            base += __builtin_popcountll(m);
        }
        wave_lds_fence();
    }
    const int total = (listed ? (int)d.nhot : NP) * NT;   // units: (listed chunk, trajectory)
    unsigned done = 0u;
    for (;;) {
        int k0 = 0;
        if (lane == 0) k0 = (int)atomicAdd(fa.fixcnt + fa.B + b, 16u);   // claim counters follow the B done counters
        k0 = __builtin_amdgcn_readfirstlane(k0);
        if (k0 >= total) break;
        const int k = k0 + row;
        const bool live = k < total;
        done += (unsigned)((total - k0 < 16) ? total - k0 : 16);
        const int h = live ? k / NT : 0, j = live ? k - h * NT : 0;
        const int c = listed ? (int)hotlist[h] : h;
        const bool hot = live && (listed || d.t3 || !(fabsf(pm[c]) <= fa.g2));
        if (!hot) continue;   // whole quads
        const size_t q = (size_t)b * NP + c;
        double* o64 = fa.Phi64 + (q * NT + j) * W;
        if (d.t3)
            for (int i = 4 * TPL + r; i < W; i += 4) st_through(o64 + i, 0.0);
        if (j >= M) {   // padding trajectory: the fp32 map already holds zeros there; the doubles need them
            if (d.t3) {
#pragma unroll
                for (int kk = 0; kk < TPL; ++kk) st_through(o64 + r * TPL + kk, 0.0);
            }
            continue;
        }
        double w[TPL], a0[TPL], dd[TPL];
#pragma unroll
        for (int kk = 0; kk < TPL; ++kk) w[TPL - 1 - kk] = (r * TPL + kk == j) ? 1.0 : 0.0;
        const double inv_hop = 1.0 / (double)hop;
        int fcur = -1;
        const int nblk = L / W;
        for (int blk = 0; blk < nblk; ++blk) {
            const int t0 = c * L + blk * W;
            const int f = t0 / hop;  // <= F-2: chunks with a transition matrix end before (F-1)*hop
            if (f != fcur) {
                fcur = f;
                // Unconditional loads from a clamped index, the select AFTER the conversion: written as
                // `i < M ? (double)pa0[i] : 0.0` these were 12 conditional loads each waited for -- twelve serial round trips
                // per hot chunk (found in round 3's last session, ISA of the pre-pass).  (No buffer descriptors here: the
                // lanes of a wave work on different chunks, a descriptor has to be wave-uniform.)
                const float* pa0 = fa.a + ((size_t)b * F + f) * M;
                const float* pa1 = pa0 + M;
                float u0[TPL], u1[TPL];
#pragma unroll
                for (int kk = 0; kk < TPL; ++kk) {
                    const int i = r * TPL + kk, ic = i < M ? i : M - 1;
                    u0[kk] = pa0[ic];
                    u1[kk] = pa1[ic];
                }
#pragma unroll
                for (int kk = 0; kk < TPL; ++kk) {
                    const bool in = r * TPL + kk < M;
                    const double w0 = (double)u0[kk], w1 = (double)u1[kk];
                    const double v0 = in ? w0 : 0.0, v1 = in ? w1 : 0.0;
                    a0[kk] = -v0;                       // NEGATED coefficients: the tap sum is the new sample itself
                    dd[kk] = (v0 - v1) * inv_hop;
                }
            }
            const double n0 = (double)(t0 - f * hop);
#pragma unroll
            for (int s = 0; s < W; ++s) {
                const double n = n0 + (double)s;
                double cf[TPL];
#pragma unroll
                for (int kk = 0; kk < TPL; ++kk) cf[kk] = __builtin_elementwise_fma(n, dd[kk], a0[kk]);
                double pa = 0.0, pb = 0.0;
#pragma unroll
                for (int kk = TPL - 1; kk >= 1; --kk) {
                    const int slot = (s - 1 - kk + 4 * TPL) % TPL;
                    if (kk & 1) pa = __builtin_elementwise_fma(cf[kk], w[slot], pa);
                    else        pb = __builtin_elementwise_fma(cf[kk], w[slot], pb);
                }
                double part = __builtin_elementwise_fma(cf[0], w[(s - 1 + TPL) % TPL], pa + pb);
                part += dppd<DPP_XOR1>(part);
                part += dppd<DPP_XOR2>(part);       // = y[t] (homogeneous: no input), in every lane of the quad
                const double inc = dppd<DPP_SHR1>(w[s % TPL]);
                w[s % TPL] = r == 0 ? part : inc;   // lane 0 takes y, the others their left neighbour's oldest
                // (a DPP bank mask cannot do this select: banks are lanes 4i..4i+3 of a row, not lane % 4)
            }
        }
        // this lane holds entries i = r TPL + kk of column j: d s_end[i] / d s_start[j]
        if (!fa.accurate) {
            float* o = fa.PhiT + q * NT * W + j;
#pragma unroll
            for (int kk = 0; kk < TPL; ++kk) {
                const int i = r * TPL + kk;
                if (i < NT) st_through(o + (size_t)i * W, i < M ? (float)w[TPL - 1 - kk] : 0.f);
            }
            if (fa.Phi) {
                float* o2 = fa.Phi + (q * NT + j) * W;
#pragma unroll
                for (int kk = 0; kk < TPL; ++kk) {
                    const int i = r * TPL + kk;
                    if (i < W) st_through(o2 + i, i < M ? (float)w[TPL - 1 - kk] : 0.f);
                }
            }
        }
        if (d.t3) {
#pragma unroll
            for (int kk = 0; kk < TPL; ++kk) {
                const int i = r * TPL + kk;
                st_through(o64 + i, i < M ? w[TPL - 1 - kk] : 0.0);
            }
        }
    }
    if (!done) return;                                        // wave-uniform: nothing stored, nothing to report
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (ordering for the compiler) ...
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // ... vmcnt(0): the stores above are acknowledged
    if (lane == 0 && done) atomicAdd(fa.fixcnt + b, done);
}

// Waves of the SAME launch that read an utterance's maps after its fix-up (the composite and zero-state workgroups of
// lpc_group_prepass_kernel): wait until all units have reported.  A waiter first runs fixup_wave itself (the claim loop), so
// when it gets here every unit is finished or claimed by a wave that is resident and computing: forward progress does not
// depend on the order in which workgroups were dispatched.  The spin is bounded all the same (a hang is never acceptable);
// running out is reported in fixcnt[2 B] -> bit 1 of status word 2, which the Python binding raises on.
__device__ __forceinline__ void wait_for_fixup(const FixArgs& fa, int b, unsigned nhot, int NT) {
    const unsigned expected = (fa.NP <= kHotListMax ? nhot : (unsigned)fa.NP) * (unsigned)NT;
    unsigned it = 0u;
    while (__hip_atomic_load(fa.fixcnt + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expected) {
        __builtin_amdgcn_s_sleep(8);
        if (++it > (1u << 16)) {
            if ((threadIdx.x & 63) == 0) atomicOr(fa.fixcnt + 2 * fa.B, 1u);
            break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// The fix-up as a launch of its own (flat-scan path, transitions prepared without the two-level scan):
// grid (KF, B), 4 independent waves per workgroup.
template <int W, int NT>
__global__ __launch_bounds__(256) void lpc_fixup_kernel(FixArgs fa) {
    __shared__ unsigned short hotlist[4][kHotListMax];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    fixup_wave<W, NT>(fa, blockIdx.y, blockIdx.x == 0 && wv == 0, hotlist[wv]);
}

__device__ __forceinline__ double lane_bcast_d(double v, int lane) {
    const long long x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), lane);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}

// Tier-3 boundary states: s_{c+1} = Phi_c s_c + z_c in fp64 over the maps kept as doubles ([c][j][i]: lane i takes
// element i of every row j, so the wave's accesses are contiguous), one wave per utterance; states leave rounded to fp32
// into rows of `sstride` floats (32: S1 of the two-level path, 64: S of the flat one).
template <int W, int NT>
__device__ __forceinline__ void precise_fwd_scan_w1(const double* __restrict__ P64, const float* __restrict__ zb,
                                                    float* __restrict__ Sb, int sstride, int NP, int lane) {
    const bool act = lane < NT;
    const int ii = act ? lane : 0;
    constexpr int D = 4;
    double buf[D][NT];
    float zc[D];
    auto fetch = [&](int u, int c) {
        const int cl = c < NP ? c : NP - 1;
        const double* mp = P64 + (size_t)cl * NT * W + ii;
#pragma unroll
        for (int j = 0; j < NT; ++j) buf[u][j] = mp[(size_t)j * W];
        zc[u] = zb[(size_t)cl * W + ii];
    };
    double s = 0.0;
    if (NP > 0) {
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, u);
        for (int c0 = 0; c0 < NP; c0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int c = c0 + u;
                if (c < NP) {   // wave-uniform
                    if (lane < sstride) Sb[(size_t)c * sstride + lane] = (float)s;
                    double acc0 = (double)zc[u], acc1 = 0.0;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const double sj = lane_bcast_d(s, j);
                        if (j & 1) acc1 = __builtin_elementwise_fma(buf[u][j], sj, acc1);
                        else       acc0 = __builtin_elementwise_fma(buf[u][j], sj, acc0);
                    }
                    s = act ? acc0 + acc1 : 0.0;
                    fetch(u, c + D);
                }
            }
        }
    }
    if (lane < sstride) Sb[(size_t)(NP > 0 ? NP : 0) * sstride + lane] = (float)s;
}

// Tier-3 adjoint boundary states (backward): lam_start(c) = Phi_c^T lam_end(c) + zadj_c in fp64; lane j reads row j of
// the doubles (contiguous).  Mirrors lpc_adj_scan_kernel: lamEnd[c][:] = adjoint state at the END of chunk c.
template <int W, int NT>
__device__ __forceinline__ void precise_adj_scan_w1(const double* __restrict__ P64, const float* __restrict__ zb,
                                                    float* __restrict__ Lb, int lstride, int NP, int lane) {
    const bool act = lane < NT;
    const int jj = act ? lane : 0;
    if (lane < lstride) Lb[(size_t)NP * lstride + lane] = 0.f;
    double lam = act ? (double)zb[(size_t)NP * W + jj] : 0.0;
    constexpr int D = 4;
    double buf[D][NT];
    float zc[D];
    auto fetch = [&](int u, int c) {
        const int cl = c > 0 ? c : 0;
        const double* mp = P64 + ((size_t)cl * NT + jj) * W;
#pragma unroll
        for (int i = 0; i < NT; ++i) buf[u][i] = mp[i];
        zc[u] = zb[(size_t)cl * W + jj];
    };
    if (NP <= 0) return;
#pragma unroll
    for (int u = 0; u < D; ++u) fetch(u, NP - 1 - u);
    for (int u0 = 0; u0 < NP; u0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int c = NP - 1 - (u0 + u);
            if (c >= 0) {   // wave-uniform
                if (lane < lstride) Lb[(size_t)c * lstride + lane] = (float)lam;
                double acc0 = (double)zc[u], acc1 = 0.0;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const double li = lane_bcast_d(lam, i);
                    if (i & 1) acc1 = __builtin_elementwise_fma(buf[u][i], li, acc1);
                    else       acc0 = __builtin_elementwise_fma(buf[u][i], li, acc0);
                }
                lam = act ? acc0 + acc1 : 0.0;
                fetch(u, c - D);
            }
        }
    }
}

// The same scans with the matvec split over the two halves of the wave (round 4; orders up to 32).  Lane (i, h = lane / 32)
// owns row i and the columns of half h: half as many doubles to fetch per step (a ring twice as deep in the same registers),
// half as long a dependent FMA chain, and the state reaches a lane by ds_bpermute (per-lane source: readlane's scalar
// result cannot differ between the halves) -- ~36 instead of ~70 issued instructions per step, and the fetch latency that
// bounded the one-lane-per-row version (400 ns per step: 80 us for the 199 steps of a 2 s utterance) is covered.
__device__ __forceinline__ double lane_perm_d(double v, int src_lane) {
    const long long x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)(x >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}
template <int W, int NT>
__device__ __forceinline__ void precise_fwd_scan(const double* __restrict__ P64, const float* __restrict__ zb,
                                                 float* __restrict__ Sb, int sstride, int NP, int lane) {
    if constexpr (NT > 32) {
        precise_fwd_scan_w1<W, NT>(P64, zb, Sb, sstride, NP, lane);
    } else {
        constexpr int NH = (NT + 1) / 2;          // columns per half
        const int h = lane >> 5, i = lane & 31;
        const bool act = i < NT;
        const int ii = act ? i : 0, j0 = h * NH;
        constexpr int D = 4;   // (a deeper ring raises the register count of the whole refinement kernel these waves ride in)
        double buf[D][NH];
        float zc[D];
        auto fetch = [&](int u, int c) {
            const int cl = c < NP ? c : NP - 1;
            const double* mp = P64 + (size_t)cl * NT * W + ii;
#pragma unroll
            for (int k = 0; k < NH; ++k) {   // raw loads from a clamped row: the mask of a padding column (odd orders) is applied
                const int j = j0 + k;        // to the STATE value at use -- a select here makes hipcc wait for every load at once
                buf[u][k] = mp[(size_t)(j < NT ? j : NT - 1) * W];
            }
            zc[u] = zb[(size_t)cl * W + ii];
        };
        double s = 0.0;                            // component i, the same value in both halves
        if (NP > 0) {
#pragma unroll
            for (int u = 0; u < D; ++u) fetch(u, u);
            for (int c0 = 0; c0 < NP; c0 += D) {
#pragma unroll
                for (int u = 0; u < D; ++u) {
                    const int c = c0 + u;
                    if (c < NP) {   // wave-uniform
                        if (lane < sstride) Sb[(size_t)c * sstride + lane] = h == 0 ? (float)s : 0.f;
                        // all permutes of a step in flight at once, ONE wait: left to itself hipcc reuses one register pair
                        // for the permuted value and waits for every ds_bpermute before the FMA that consumes it -- twelve
                        // LDS round trips per step, 1.3 us (measured: a tier-3 batch 243 -> 413 us with that schedule)
                        double sj[NH];
#pragma unroll
                        for (int k = 0; k < NH; ++k) {
                            const double v = lane_perm_d(s, j0 + k < NT ? j0 + k : 0);
                            sj[k] = (2 * NH == NT || j0 + k < NT) ? v : 0.0;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                        for (int k = 0; k < NH; ++k) {
                            if (k & 1) acc1 = __builtin_elementwise_fma(buf[u][k], sj[k], acc1);
                            else       acc0 = __builtin_elementwise_fma(buf[u][k], sj[k], acc0);
                        }
                        const double part = acc0 + acc1;
                        const double tot = part + lane_perm_d(part, lane ^ 32);   // commutative: both halves get the same bits
                        s = act ? tot + (double)zc[u] : 0.0;
                        fetch(u, c + D);
                    }
                }
            }
        }
        if (lane < sstride) Sb[(size_t)(NP > 0 ? NP : 0) * sstride + lane] = h == 0 ? (float)s : 0.f;
    }
}
template <int W, int NT>
__device__ __forceinline__ void precise_adj_scan(const double* __restrict__ P64, const float* __restrict__ zb,
                                                 float* __restrict__ Lb, int lstride, int NP, int lane) {
    if constexpr (NT > 32) {
        precise_adj_scan_w1<W, NT>(P64, zb, Lb, lstride, NP, lane);
    } else {
        constexpr int NH = (NT + 1) / 2;          // rows i of the map per half (lam'_j = sum_i Phi[i][j] lam_i)
        const int h = lane >> 5, j = lane & 31;
        const bool act = j < NT;
        const int jj = act ? j : 0, i0 = h * NH;
        if (lane < lstride) Lb[(size_t)NP * lstride + lane] = 0.f;
        double lam = act ? (double)zb[(size_t)NP * W + jj] : 0.0;
        constexpr int D = 4;   // (a deeper ring raises the register count of the whole refinement kernel these waves ride in)
        double buf[D][NH];
        float zc[D];
        auto fetch = [&](int u, int c) {
            const int cl = c > 0 ? c : 0;
            const double* mp = P64 + ((size_t)cl * NT + jj) * W;
#pragma unroll
            for (int k = 0; k < NH; ++k) {   // (raw loads; padding masked at use: see precise_fwd_scan)
                const int i = i0 + k;
                buf[u][k] = mp[i < NT ? i : NT - 1];
            }
            zc[u] = zb[(size_t)cl * W + jj];
        };
        if (NP <= 0) return;
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, NP - 1 - u);
        for (int u0 = 0; u0 < NP; u0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int c = NP - 1 - (u0 + u);
                if (c >= 0) {   // wave-uniform
                    if (lane < lstride) Lb[(size_t)c * lstride + lane] = h == 0 ? (float)lam : 0.f;
                    double li[NH];   // (all permutes of the step in flight at once: see precise_fwd_scan)
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        const double v = lane_perm_d(lam, i0 + k < NT ? i0 + k : 0);
                        li[k] = (2 * NH == NT || i0 + k < NT) ? v : 0.0;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        if (k & 1) acc1 = __builtin_elementwise_fma(buf[u][k], li[k], acc1);
                        else       acc0 = __builtin_elementwise_fma(buf[u][k], li[k], acc0);
                    }
                    const double part = acc0 + acc1;
                    const double tot = part + lane_perm_d(part, lane ^ 32);
                    lam = act ? tot + (double)zc[u] : 0.0;
                    fetch(u, c - D);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Two-level boundary scan (round 2; the default for long utterances with M <= 24; GOLF_SS_FLAT_SCAN selects the flat one).  The flat scan below is 199 dependent 22 x 22
// matvecs on ONE wave per utterance: 31 us, twice per inference step (38 % of the single-stream step).  The chunk maps
// of an utterance are cut into groups of 16 -- the 16 chunks one wave of the chunk kernels (lpc_fwdq*) owns:
//   lpc_group_composite_kernel  M_g = Phi_{c0+15} ... Phi_{c0} for every group, once per step: a chain of 16 exact-fp32
//       32x32 MFMA products per wave whose running product stays in the accumulator registers: for
//       v_mfma_f32_32x32x2_f32 the D layout (register v, lane l -> row 8(v/4) + 4(l/32) + v%4, column l%32) IS the B
//       layout of K-step v if the contraction index is enumerated as k = 8(v/4) + 4(l/32) + v%4, so D feeds back as B
//       with no data movement; the A fragments for that enumeration are three float4 loads of the lane's row of Phi_c.
//   lpc_group_zscan_kernel      v_g = the group's zero-state response to its inputs z (16 steps), one wave per group,
//       spread over the chip (a first version ran the 16 groups of an utterance as 16 waves of ONE workgroup: a scan
//       step occupies its SIMD's issue port for ~360 cycles -- the 22 v_readlane_b32 -- so four waves on a SIMD simply
//       queue; 31.5 us per scan, no gain).
//   lpc_fwdq2_kernel            the chunk kernels with a prologue: the wave folds the (M_g, v_g) of the groups before
//       its own (<= 12 steps) and then scans its own 16 chunk maps (16 steps), leaving its 17 chunk start states in LDS
//       -- no boundary-state array in HBM, no device-wide dependency besides kernel order.  The refinement pass ends
//       with an epilogue that scans the group's 16 defects (-> v'_g), so the second scan needs no launch of its own:
//       the final pass folds (M_g, v_g + v'_g) and scans with inputs z + defect.
//   16 + <= 12 + 16 dependent steps on the critical path of each pass instead of 199 per scan.
//   lpc_fwdq2m_kernel           (round 5) both chunk passes in ONE launch for a batch that runs alone: the waves of an utterance
//       hand their defect responses to each other through flag words (a wave waits only for workgroups dispatched before it)
//       and keep their 16 maps in LDS between the three stages that need them.
// ------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int W> constexpr int kMapRow = W + 4;   // row stride of a group's maps kept in LDS (lpc_fwdq2m_kernel), in words
// prefetch depths of the two-level prologues (maps fetched ahead of the matvec that uses them): chunk maps / composites
// (measured round 4: 8 + 8 and 6 + 8 deep were slower -- the prologue's matvec steps are issue-bound, not fetch-bound)
constexpr int kPrefetchMaps = 6, kPrefetchComposites = 4;

// s' = rows . s + add with the state broadcast by v_readlane (lane i = component i, `rw` = row i of the matrix)
template <int W, int NT>
__device__ __forceinline__ float matvec_step(const float4* rw, float s, float add, bool act) {
    // Four partial sums (columns j mod 4), written as two packed accumulators over the (x, y) / (z, w) halves of the row's
    // float4s: the pairs are the registers the loads filled, so each v_pk_fma_f32 takes them as they are.  (Left to hipcc, a
    // scalar four-accumulator form is SLP-packed too, but across the accumulators -- columns (3, 5), (7, 9) ... -- and every pair costs two
    // v_mov to assemble: ~70 instructions per step instead of ~38 for the same 22 FMAs, on the critical path of every scan.)
    typedef float pk2 __attribute__((ext_vector_type(2)));
    static_assert(NT % 2 == 0, "column pairs");
    pk2 accA = {add, 0.f}, accB = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NT / 2; ++k) {
        const float4& q = rw[k / 2];
        const pk2 pj = (k & 1) ? pk2{q.z, q.w} : pk2{q.x, q.y};
        const pk2 sj = {lane_bcast(s, 2 * k), lane_bcast(s, 2 * k + 1)};
        if (k & 1) accB = __builtin_elementwise_fma(pj, sj, accB);
        else       accA = __builtin_elementwise_fma(pj, sj, accA);
    }
    return act ? (accA.x + accA.y) + (accB.x + accB.y) : 0.f;
}

// Composite map of a group, M_g = Phi_{c1-1} ... Phi_{c0}, accumulated in DOUBLE precision on the matrix pipe.
// Why not fp32 (round 2 first built this as an exact-fp32 MFMA product chain, 4.8 us): the entries of a companion-form
// transition matrix cancel heavily in products (consecutive samples are almost collinear states), so an fp32 chain of 16
// products comes out with ~1e-4 relative error for benign filters and ~1e-2 when poles sit at radius 0.9999 (first
// reflection coefficient ~0.98: ordinary voiced speech).  The flat scan never forms products -- it applies Phi_c to actual
// states, at rounding level -- and a refinement sweep cannot repair a coarse propagator whose error times the
// dynamics' error growth is of order one: boundary-state error 1.3 (!) instead of 6e-3 on such an utterance, 8e-8 on
// both for a benign one (numpy emulation; tests/test_gpu_lpc_ss.py::test_ill_conditioned_rows).  With the products
// accumulated in fp64 and rounded ONCE to fp32 the two-level scan is as accurate as the flat one (3.7e-3 vs 5.9e-3).
// (A VALU version -- v_fma_f64, maps staged in LDS as doubles, columns split over 2 / 4 / 8 waves -- took 20.6 / 19.2 /
// 28.6 us for the pre-pass: ~240 dependent-issue instructions per product per wave.)
// v_mfma_f64_16x16x4_f64: the state space is padded to NTL x 16 (NTL = 1 or 2 tiles).  The columns of M_g are
// independent, so a wave owns ONE column tile jt and both row tiles: per product NTL x NTL x 4 MFMAs, no exchange with
// any other wave.  The running product never leaves the accumulators.  D: lane (kq = l / 16, n = l % 16), register v ->
// tile position p = kq + 4 v (probed on the hardware, tools/ubench/mfma_f64_layout.hip; the f32 16x16x4 instruction has
// 4 kq + v).  Used as the B operand of K-step s = v, lane kq contributes position kq + 4 s -- so the tile's 16 positions
// may hold the state components in any fixed order rho, as long as the A operand of step s is column rho(kq + 4 s) of row
// rho(m).  rho(kq + 4 s) = 8 (s / 2) + 2 kq + s % 2: steps 0, 1 cover components 0..7 of the tile and steps 2, 3
// components 8..15 -- for the second K tile of a 22-component state (components 16..21) steps 2 and 3 meet only padding
// and are skipped (12 MFMAs per product instead of 16), and the A operand is two contiguous float2 of the lane's row.
// The permutation costs nothing: it is address arithmetic on the A rows, the identity start and the final store.
typedef double f64x4 __attribute__((ext_vector_type(4)));
template <int W, int NT>
struct CompGeom {
    static constexpr int NTL = NT > 16 ? 2 : 1;   // 16-wide tiles of the (padded) state space = waves per group
    static constexpr int KW = NTL;
};
// One product step P <- Phi . P on the matrix pipe; A fragments fr[it][kt] as fetched by comp_fetch / read from LDS.
template <int NT, int NTL, typename AV>
__device__ __forceinline__ void comp_product(const AV (&fr)[NTL][NTL], f64x4 (&P)[NTL]) {
    // one accumulator per (row tile, K tile): NTL x NTL independent chains of 4 MFMAs (a dependent f64 MFMA waits for its
    // predecessor: two chains of 8 measured ~190 cycles per instruction, four chains of 4 ~130)
    const f64x4 zero4 = {0.0, 0.0, 0.0, 0.0};
    f64x4 Dn[NTL][NTL];
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
        for (int it = 0; it < NTL; ++it)
#pragma unroll
            for (int kt = 0; kt < NTL; ++kt) {
                if (sidx == 0) Dn[it][kt] = zero4;
                if (16 * kt + 8 * (sidx / 2) + sidx % 2 < NT)   // step s meets columns 16 kt + 8 (s / 2) + 2 kq + s % 2
                    Dn[it][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fr[it][kt][sidx], P[kt][sidx], Dn[it][kt],
                                                                      0, 0, 0);
            }
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        P[it] = Dn[it][0];
#pragma unroll
        for (int kt = 1; kt < NTL; ++kt) P[it] += Dn[it][kt];
    }
}

// The workgroup of one group: wave (jt, h) multiplies the maps of HALF the chain (h = 0: c0 .. cmid-1, h = 1: cmid ..
// c1-1) for column tile jt -- 8 dependent products instead of 16, an f64 MFMA being ~130 cycles from one wave --; the
// h = 1 waves leave their product P_B in LDS (doubles, padded 32 x 32), and after one workgroup barrier the h = 0 waves,
// which still hold P_A[:, jt] in their accumulators, finish with M[:, jt] = P_B . P_A[:, jt].
typedef float f32x4v __attribute__((ext_vector_type(4)));
template <int W, int NT>
__device__ __forceinline__ void group_composite_wg(const float* __restrict__ PhiT, float* __restrict__ MT, int NP, int NG,
                                                   int b, int g, double* __restrict__ pb_lds /* [32][32] */,
                                                   float* __restrict__ MTt = nullptr) {
    static_assert(NT <= 32 && W % 4 == 0, "two 16-wide tiles");
    constexpr int NTL = CompGeom<W, NT>::NTL;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jt = wv & 1, h = wv >> 1;
    const int m = lane & 15, kq = lane >> 4;
    const int n = 16 * jt + m;                                        // this lane's column
    const int rm = 8 * (m >> 3) + 2 * (m & 3) + ((m >> 2) & 1);       // rho(m), m = kq' + 4 s'
    const int rq = 2 * kq;                                            // rho(kq + 4 v) = 8 (v / 2) + rq + v % 2
    const int c0 = g * kGroup, c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
    const int cmid = c0 + kGroup / 2 < c1 ? c0 + kGroup / 2 : c1;
    const int ca = h ? cmid : c0, cb = h ? c1 : cmid;                 // this wave's part of the chain
    const bool live = jt < NTL;                                       // orders <= 16 have one column tile
    f64x4 P[NTL];                                                     // P[kt][v] = P(row 16 kt + rho(kq + 4 v), column n)
#pragma unroll
    for (int kt = 0; kt < NTL; ++kt)
#pragma unroll
        for (int v = 0; v < 4; ++v) P[kt][v] = (16 * kt + 8 * (v / 2) + rq + v % 2 == n && n < NT) ? 1.0 : 0.0;
    if (live) {
        const float* base = PhiT + (size_t)b * NP * NT * W;
        // A fragments: row 16 it + rho(m), columns 16 kt + 2 kq + {0, 1} and 16 kt + 8 + 2 kq + {0, 1} of map c (zero
        // outside the NT x W array)
        constexpr int D = 2;                                          // maps fetched ahead (deeper rings measured slower)
        f32x4v fr[D][NTL][NTL];
        auto fetch = [&](int u, int c) {
            const float* mp = base + (size_t)(c < cb ? c : (cb > ca ? cb - 1 : ca)) * NT * W;
#pragma unroll
            for (int it = 0; it < NTL; ++it)
#pragma unroll
                for (int kt = 0; kt < NTL; ++kt) {
                    const int row = 16 * it + rm, col = 16 * kt + rq;
                    const float* rp = mp + (size_t)(row < NT ? row : 0) * W;
                    const bool ok = row < NT && cb > ca;
                    // (columns >= NT are padding: zero by construction, and not trusted -- NT and col are even)
                    const float2 lo = (ok && col < NT) ? *reinterpret_cast<const float2*>(rp + col) : make_float2(0.f, 0.f);
                    const float2 hi = (ok && col + 8 < NT) ? *reinterpret_cast<const float2*>(rp + col + 8)
                                                           : make_float2(0.f, 0.f);
                    fr[u][it][kt] = f32x4v{lo.x, lo.y, hi.x, hi.y};
                }
        };
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, ca + u);
#pragma unroll
        for (int k = 0; k < kGroup / 2; ++k) {
            const int u = k % D;
            if (ca + k < cb) {   // wave-uniform
                comp_product<NT, NTL>(fr[u], P);
                if (k + D < kGroup / 2) fetch(u, ca + k + D);
            }
        }
        if (h == 1) {   // P_B[rho-position basis -> original row i][column n] for the final product's A operand
#pragma unroll
            for (int it = 0; it < NTL; ++it)
#pragma unroll
                for (int v = 0; v < 4; ++v) pb_lds[(16 * it + 8 * (v / 2) + rq + v % 2) * 32 + n] = P[it][v];
        }
    }
    __syncthreads();
    if (h == 1 || !live) return;
    {   // M[:, jt] = P_B . P_A[:, jt]: A fragments of P_B from LDS (row 16 it + rho(m), the same columns as above)
        f64x4 fa[NTL][NTL];
#pragma unroll
        for (int it = 0; it < NTL; ++it)
#pragma unroll
            for (int kt = 0; kt < NTL; ++kt) {
                const double* rp = pb_lds + (16 * it + rm) * 32 + 16 * kt + rq;
                const double2 lo = *reinterpret_cast<const double2*>(rp), hi = *reinterpret_cast<const double2*>(rp + 8);
                fa[it][kt] = f64x4{lo.x, lo.y, hi.x, hi.y};
            }
        comp_product<NT, NTL>(fa, P);
    }
    // M_g[i][n] rounded once to fp32; columns NT .. W-1 of the rows (never read) are written as zeros
    float* mt = MT + ((size_t)b * NG + g) * NT * W;
#pragma unroll
    for (int it = 0; it < NTL; ++it)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = 16 * it + 8 * (v / 2) + rq + v % 2;   // rho(kq + 4 v)
            if (i < NT && n < W) mt[(size_t)i * W + n] = n < NT ? (float)P[it][v] : 0.f;
            // training: the transposed copy, for the backward's two-level adjoint scan (rows of M_g^T are what its lanes read)
            if (MTt && i < W && n < NT) MTt[(((size_t)b * NG + g) * NT + n) * W + i] = i < NT ? (float)P[it][v] : 0.f;
        }
}

// ------------------------------------------------------------------------------------------
// Tier 3 on the two-level path (round 4): the boundary states of an utterance whose maps are kept as doubles used to come
// from ONE wave's fp64 scan over all its chunks (199 dependent steps, ~45 us, riding in the refinement launch, which then
// lasted that long).  Now in two levels like the fp32 path: per group an fp64 composite (the same v_mfma_f64 product chain
// as group_composite_wg, one wave, both column tiles, the operands read as doubles) and the group's zero-state response;
// the wave that completes an utterance's last group folds them into the group start states G (NG steps); the final pass
// scans each group's own 16 maps from G in its prologue (what its fp32 prologue costs anyway).  16 + NG + 16 dependent
// steps instead of NP.
// precise_scan_range: s <- Phi_c s + z_c over n maps stored [c][j][i] as doubles, the split-half layout of precise_fwd_scan;
// z of type ZT in rows of zstride; the states before every map and after the last go to Sb (rows of sstride, type ST) when
// Sb is not null; returns the final state (component lane % 32, the same value in both halves).
template <int W, int NT, typename ZT, typename ST>
__device__ __forceinline__ double precise_scan_range(const double* __restrict__ P64, const ZT* __restrict__ zb, int zstride,
                                                     ST* __restrict__ Sb, int sstride, int n, int lane,
                                                     const double* __restrict__ s0) {
    static_assert(NT <= 32, "split-half layout");
    constexpr int NH = (NT + 1) / 2;          // columns per half
    const int h = lane >> 5, i = lane & 31;
    const bool act = i < NT;
    const int ii = act ? i : 0, j0 = h * NH;
    constexpr int D = 4;
    double buf[D][NH];
    ZT zc[D];
    auto fetch = [&](int u, int c) {
        const int cl = c < n ? c : n - 1;
        const double* mp = P64 + (size_t)cl * NT * W + ii;
#pragma unroll
        for (int k = 0; k < NH; ++k) {   // raw loads from a clamped row; padding columns are masked on the state value
            const int j = j0 + k;
            buf[u][k] = mp[(size_t)(j < NT ? j : NT - 1) * W];
        }
        zc[u] = zb[(size_t)cl * zstride + ii];
    };
    double s = 0.0;
    if (s0) { const double v = s0[ii]; s = act ? v : 0.0; }
    if (n > 0) {
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, u);
        for (int c0 = 0; c0 < n; c0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int c = c0 + u;
                if (c < n) {   // wave-uniform
                    if (Sb && lane < sstride) Sb[(size_t)c * sstride + lane] = h == 0 ? (ST)s : (ST)0;
                    double sj[NH];   // all permutes of a step in flight at once (see precise_fwd_scan)
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        const double v = lane_perm_d(s, j0 + k < NT ? j0 + k : 0);
                        sj[k] = (2 * NH == NT || j0 + k < NT) ? v : 0.0;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        if (k & 1) acc1 = __builtin_elementwise_fma(buf[u][k], sj[k], acc1);
                        else       acc0 = __builtin_elementwise_fma(buf[u][k], sj[k], acc0);
                    }
                    const double part = acc0 + acc1;
                    const double tot = part + lane_perm_d(part, lane ^ 32);
                    s = act ? tot + (double)zc[u] : 0.0;
                    fetch(u, c + D);
                }
            }
        }
    }
    if (Sb && lane < sstride) Sb[(size_t)(n > 0 ? n : 0) * sstride + lane] = h == 0 ? (ST)s : (ST)0;
    return s;
}

// M = Phi_{c1-1} ... Phi_{c0} of maps kept as doubles ([c][j][i]), one wave, written in the same [j][i] layout (so that the
// fold over the groups is a precise_scan_range over the composites).
template <int W, int NT>
__device__ __forceinline__ float precise_group_composite(const double* __restrict__ P64b, int c0, int c1,
                                                         double* __restrict__ M64, int lane) {
    static_assert(NT <= 32 && W % 4 == 0, "two 16-wide tiles");
    constexpr int NTL = CompGeom<W, NT>::NTL;
    const int m = lane & 15, kq = lane >> 4;
    const int rm = 8 * (m >> 3) + 2 * (m & 3) + ((m >> 2) & 1);       // rho(m), see group_composite_wg
    const int rq = 2 * kq;
    // one column tile after the other (the chain is walked NTL times): the refinement kernel these waves ride in must not
    // need more registers for this rare path than for its own work
    double pmx = 0.0;   // largest |entry| of any partial product (NaN-propagating: fmax would drop one, the comparison keeps it out of "small")
#pragma unroll 1
    for (int jt = 0; jt < NTL; ++jt) {
        f64x4 P[NTL];                                                 // P[kt][v] = P(row 16 kt + rho(kq + 4 v), column 16 jt + m)
#pragma unroll
        for (int kt = 0; kt < NTL; ++kt)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                P[kt][v] = (16 * kt + 8 * (v / 2) + rq + v % 2 == 16 * jt + m && 16 * jt + m < NT) ? 1.0 : 0.0;
        constexpr int D = 2;
        f64x4 fr[D][NTL][NTL];
        auto fetch = [&](int u, int c) {   // A fragments: row 16 it + rho(m), columns 16 kt + rq + {0, 1, 8, 9}; clamped loads, masks after
            const double* mp = P64b + (size_t)(c < c1 ? c : c1 - 1) * NT * W;
#pragma unroll
            for (int it = 0; it < NTL; ++it)
#pragma unroll
                for (int kt = 0; kt < NTL; ++kt) {
                    const int row = 16 * it + rm, col = 16 * kt + rq;
                    const int rc = row < NT ? row : 0;
                    double v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cc = col + (e & 1) + 8 * (e >> 1);
                        v[e] = mp[(size_t)(cc < NT ? cc : NT - 1) * W + rc];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cc = col + (e & 1) + 8 * (e >> 1);
                        fr[u][it][kt][e] = (row < NT && cc < NT) ? v[e] : 0.0;
                    }
                }
        };
        if (c1 > c0) {
#pragma unroll
            for (int u = 0; u < D; ++u) fetch(u, c0 + u);
            for (int cb = c0; cb < c1; cb += D) {
#pragma unroll
                for (int u = 0; u < D; ++u) {
                    if (cb + u < c1) {   // wave-uniform
                        comp_product<NT, NTL>(fr[u], P);
#pragma unroll
                        for (int kt = 0; kt < NTL; ++kt)
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const double av = __builtin_fabs(P[kt][v]);
                                pmx = (av <= pmx) ? pmx : av;   // a NaN entry becomes the maximum
                            }
                        fetch(u, cb + u + D);
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NTL; ++it)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * it + 8 * (v / 2) + rq + v % 2, nn = 16 * jt + m;
                if (i < W && nn < NT) M64[(size_t)nn * W + i] = i < NT ? P[it][v] : 0.0;
            }
    }
    float fm = (float)pmx;   // (overflows to inf beyond fp32: also "too large")
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(fm, off);
        fm = (o <= fm) ? fm : o;
    }
    return fm;
}

// The adjoint of precise_scan_range: lam <- Phi_c^T lam + z_c over the n maps of a range, from the top map down (the split-half
// layout of precise_adj_scan: lane (j, h) owns component j and half the rows i; maps [c][j][i] give lane j its row contiguous
// in i).  Row r + 1 of Sb receives the state above map r, row 0 the state below map 0 (when Sb is not null); s0 = the state
// above the top map (null: zero).  Returns the final state.
template <int W, int NT, typename ZT, typename ST, typename S0T>
__device__ __forceinline__ double precise_adj_range(const double* __restrict__ P64, const ZT* __restrict__ zb, int zstride,
                                                    ST* __restrict__ Sb, int sstride, int n, int lane,
                                                    const S0T* __restrict__ s0) {
    static_assert(NT <= 32, "split-half layout");
    constexpr int NH = (NT + 1) / 2;
    const int h = lane >> 5, j = lane & 31;
    const bool act = j < NT;
    const int jj = act ? j : 0, i0 = h * NH;
    constexpr int D = 4;
    double buf[D][NH];
    ZT zc[D];
    auto fetch = [&](int u, int c) {
        const int cl = c > 0 ? c : 0;
        const double* mp = P64 + ((size_t)cl * NT + jj) * W;
#pragma unroll
        for (int k = 0; k < NH; ++k) {   // raw loads; padding rows are masked on the state value
            const int i = i0 + k;
            buf[u][k] = mp[i < NT ? i : NT - 1];
        }
        zc[u] = zb[(size_t)cl * zstride + jj];
    };
    double lam = 0.0;
    if (s0) { const double v = (double)s0[jj]; lam = act ? v : 0.0; }
    if (n > 0) {
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, n - 1 - u);
        for (int u0 = 0; u0 < n; u0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int c = n - 1 - (u0 + u);
                if (c >= 0) {   // wave-uniform
                    if (Sb && lane < sstride) Sb[(size_t)(c + 1) * sstride + lane] = h == 0 ? (ST)lam : (ST)0;
                    double li[NH];   // all permutes of a step in flight at once (see precise_fwd_scan)
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        const double v = lane_perm_d(lam, i0 + k < NT ? i0 + k : 0);
                        li[k] = (2 * NH == NT || i0 + k < NT) ? v : 0.0;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        if (k & 1) acc1 = __builtin_elementwise_fma(buf[u][k], li[k], acc1);
                        else       acc0 = __builtin_elementwise_fma(buf[u][k], li[k], acc0);
                    }
                    const double part = acc0 + acc1;
                    const double tot = part + lane_perm_d(part, lane ^ 32);
                    lam = act ? tot + (double)zc[u] : 0.0;
                    fetch(u, c - D);
                }
            }
        }
    }
    if (Sb && lane < sstride) Sb[lane] = h == 0 ? (ST)lam : (ST)0;
    return lam;
}

// The backward's counterpart of precise_group_job (refinement launch of the adjoint, extra rows): the group's adjoint response
// to its zadj from a zero state; the wave that completes the utterance folds the groups from the top down with the TRANSPOSED
// composites -- M64 as the forward's precise_group_job left it in the workspace ([g][j][i] is exactly the layout the adjoint
// reads) -- into GA[g] = L(c0_g - 1), GA[NG] = L(NP - 1) = zadj[NP].  The final pass scans each group's own maps from GA[g + 1].
template <int W, int NT>
__device__ __forceinline__ void precise_adj_group_job(const double* __restrict__ Phi64, const float* __restrict__ zadj,
                                                      const double* __restrict__ M64, double* __restrict__ W64,
                                                      double* __restrict__ GA64, unsigned* __restrict__ arrived, int b,
                                                      int g, int NP, int NC, int NG, int lane) {
    const double* P64b = Phi64 + (size_t)b * NP * NT * W;
    const int c0 = g * kGroup, c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
    const double w = precise_adj_range<W, NT, float, float, float>(P64b + (size_t)c0 * NT * W, zadj + ((size_t)b * NC + c0) * W,
                                                                   W, (float*)nullptr, 0, c1 - c0, lane, (const float*)nullptr);
    if (lane < 32) W64[((size_t)b * NG + g) * 32 + lane] = w;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    unsigned old = 0u;
    if (lane == 0) old = atomicAdd(arrived + b, 1u);
    old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
    if (old + 1u != (unsigned)NG) return;   // wave-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (lane == 0) arrived[b] = 0u;
    precise_adj_range<W, NT, double, double, float>(M64 + (size_t)b * NG * NT * W, W64 + (size_t)b * NG * 32, 32,
                                                    GA64 + (size_t)b * (NG + 1) * 32, 32, NG, lane,
                                                    zadj + ((size_t)b * NC + NP) * W);
}

// One (utterance, group) job of a tier-3 utterance in the refinement launch's extra rows (see lpc_fwdq2_kernel).
// Guard of the fp64 composites (found by tools/fuzz_tiers.py: an utterance whose 16-chunk products pass through entries of 1e10+
// before cancelling came out at 19 x the sequential recursion's error through the fold, 3.5 x through the flat scan, which only
// ever applies maps to states): when any partial product of any group exceeds kCompositeGuard, the wave that completes the
// utterance runs the flat fp64 scan instead of the fold and marks the utterance (word B + b of `arrived`' = 1) for the final
// pass -- and for the backward, whose adjoint then takes the flat scan too.
constexpr float kCompositeGuard = 1.0e6f;
template <int W, int NT>
__device__ __forceinline__ void precise_group_job(const double* __restrict__ Phi64, const float* __restrict__ z,
                                                  double* __restrict__ M64, double* __restrict__ V64,
                                                  double* __restrict__ G64, unsigned* __restrict__ arrived, int b, int g,
                                                  int NP, int NG, int lane, int B, float* __restrict__ S1, int part,
                                                  unsigned* __restrict__ ready = nullptr) {
    // part 0: the group's composite, part 1: its zero-state response -- two waves per group (round 5: one wave did both, 16 + 13 us
    // of dependent fp64 steps in a row, and the batch of a tier-3 utterance waited for it)
    // ready (merged chunk pass): word b is set once the utterance's group start states (or flat-scan states) are in memory --
    // the utterance's chunk waves of the SAME launch wait for it
    const double* P64b = Phi64 + (size_t)b * NP * NT * W;
    const int c0 = g * kGroup, c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
    if (part == 0) {   // wave-uniform
        double* m64 = M64 + ((size_t)b * NG + g) * NT * W;
        const float pmx = precise_group_composite<W, NT>(P64b, c0, c1, m64, lane);
        if (lane == 0) atomicMax(arrived + B + b, pmx == pmx ? __float_as_uint(pmx) : 0x7fc00000u);   // non-negative floats order as their bits
    } else {
        const double v = precise_scan_range<W, NT, float, float>(P64b + (size_t)c0 * NT * W, z + ((size_t)b * NP + c0) * W, W,
                                                                  (float*)nullptr, 0, c1 - c0, lane, (const double*)nullptr);
        if (lane < 32) V64[((size_t)b * NG + g) * 32 + lane] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    unsigned old = 0u;
    if (lane == 0) old = atomicAdd(arrived + b, 1u);
    old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
    if (old + 1u != 2u * (unsigned)NG) return;   // wave-uniform
    // this wave completed the utterance: every composite and response is visible after the acquire
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const unsigned mxbits = __hip_atomic_load(arrived + B + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool flat = !(__uint_as_float(mxbits) <= kCompositeGuard);   // wave-uniform; NaN -> flat
    if (lane == 0) {   // ready for the next forward on this workspace (all NG arrivals are in)
        arrived[b] = 0u;
        arrived[B + b] = 0u;
        arrived[2 * B + b] = flat ? 1u : 0u;
    }
    if (flat)
        precise_fwd_scan<W, NT>(P64b, z + (size_t)b * NP * W, S1 + (size_t)b * (NP + 1) * 32, 32, NP, lane);
    else
        precise_scan_range<W, NT, double, double>(M64 + (size_t)b * NG * NT * W, V64 + (size_t)b * NG * 32, 32,
                                                   G64 + (size_t)b * (NG + 1) * 32, 32, NG, lane, (const double*)nullptr);
    if (ready) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) __hip_atomic_store(ready + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Group-local scan from a zero state: v = zero-state response of the group's chunk maps to the inputs x ([b][NP][W]).
template <int W, int NT>
__device__ __forceinline__ void group_zscan_body(const float* __restrict__ PhiT, const float* __restrict__ x,
                                                 float* __restrict__ V, int NP, int NG, int b, int g, int i) {
    const bool act = i < NT;
    const int ii = act ? i : 0;
    const int c0 = g * kGroup, c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
    const float4* rows = reinterpret_cast<const float4*>(PhiT + ((size_t)b * NP * NT + ii) * W);
    const size_t cstride4 = (size_t)NT * W / 4;
    const float* xb = x + (size_t)b * NP * W + ii;
    // a ring of D maps ahead.  Registers decide how many of the launch's workgroups are resident at once: the 416
    // composite + 104 scan workgroups of a B = 32 launch need 3 waves per SIMD (<= 168 VGPRs), or the last scan
    // workgroups only start when the first composites retire.
    constexpr int D = 4;
    float4 buf[D][W / 4];
    float xc[D];
    auto fetch = [&](int u, int c) {
        const int cl = c < c1 ? c : c1 - 1;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) buf[u][k] = rows[(size_t)cl * cstride4 + k];
        xc[u] = xb[(size_t)cl * W];
    };
#pragma unroll
    for (int u = 0; u < D; ++u) fetch(u, c0 + u);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
        const int u = k % D;
        if (c0 + k < c1) s = matvec_step<W, NT>(buf[u], s, xc[u], act);   // wave-uniform
        if (k + D < kGroup) fetch(u, c0 + k + D);
    }
    if (i < 32) V[((size_t)b * NG + g) * 32 + i] = s;
}

// Group-local scan from a zero state with the inputs in LDS (x[k][32], k = chunk of the group): v = the response of the
// group's chunk maps -> V[b][g].  Epilogue of the refinement pass (inputs = its defects) and of the zero-state units that
// run inside the pre-pass launch (inputs = their z).
template <int W, int NT, int D = 4, bool FROMLDS = false, bool WT = false>
__device__ __forceinline__ void group_scan_lds(const float* __restrict__ PhiT, const float* __restrict__ xl,
                                               float* __restrict__ Vout, int b, int g, int NP, int NG, int lane,
                                               const float* mapl = nullptr) {
    // FROMLDS: the group's maps were left in LDS by the prologue (group_prologue MAPIO 1): row ii of map k at mapl[(k * NT + ii) * kMapRow]
    const bool act = lane < NT;
    const int ii = act ? lane : 0;
    const int c0 = g * kGroup;
    const size_t cstride4 = (size_t)NT * W / 4;
    const float4* rows = reinterpret_cast<const float4*>(PhiT + ((size_t)b * NP * NT + ii) * W);
    const float4* lrows = reinterpret_cast<const float4*>(mapl) + ii * (kMapRow<W> / 4);
    auto row4 = [&](int cl, int k) -> float4 {
        if constexpr (FROMLDS) return lrows[(cl - c0) * (NT * kMapRow<W> / 4) + k];
        else                   return rows[(size_t)cl * cstride4 + k];
    };
    const int c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
    float4 pb[D][W / 4];   // D maps ahead
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int cl = c0 + u < c1 ? c0 + u : c1 - 1;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) pb[u][k] = row4(cl, k);
    }
    float s = 0.f;
    for (int cb = c0; cb < c1; cb += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            if (cb + u < c1) {   // wave-uniform
                s = matvec_step<W, NT>(pb[u], s, xl[(cb + u - c0) * 32 + ii], act);
                const int cn = cb + u + D < c1 ? cb + u + D : c1 - 1;
#pragma unroll
                for (int k = 0; k < W / 4; ++k) pb[u][k] = row4(cn, k);
            }
        }
    }
    if constexpr (WT) {   // written THROUGH to memory (agent-scope store): read by other waves of the same launch
        if (lane < 32) __hip_atomic_store(Vout + ((size_t)b * NG + g) * 32 + lane, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if (lane < 32) Vout[((size_t)b * NG + g) * 32 + lane] = s;
    }
}

// Both pre-passes of the two-level scan AND the fix-up of hot chunk maps in ONE launch (they depend only on the transition
// kernel's outputs) -- and, round 4, the zero-state pass itself (`parts` bit 2): the wave that scans group g's zero-state
// responses first COMPUTES them (fwdq_body MODE 0 on the group's 16 chunks; z stays in its LDS tile, a copy goes to HBM for the
// refinement pass) and then scans them through the group's maps.  The transition kernel is then a launch of its own that
// needs only the coefficients -- the form in which it can run beside the oscillator's launches (ltv_allpole_prepare(maps_only=True)).
// Workgroup ranges, in grid order (`parts` bit 0: fix-up + composites, bit 1: zero-state scans, bit 2: ... preceded by the
// zero-state pass):
//   B*KF1               leading fix-up workgroups (fixup_wave; 4 independent waves each): every wave derives its utterance's
//                       tier and returns at once unless the utterance has hot chunks.  A head start for hot utterances, not a
//                       guarantee the launch depends on (waiters help, see wait_for_fixup);
//   ceil(NG*B / 4)      the groups' zero-state responses (one wave per group, four independent waves per workgroup);
//   NG*B                group composites (4 waves cooperating on one group);
//   B*KF2               trailing fix-up workgroups: the same waves again, claiming units from the same counters -- they make
//                       a hot utterance's fix-up ~one 13 us pass, and cost a cold batch nothing (they start after everything
//                       else has been dispatched and return after one load).
// A composite / zero-state wave looks at its OWN group's 16 chunk maxima first: nothing beyond G2 there (the common case)
// -> its maps are final, go ahead.  Otherwise it derives the utterance's tier like the fix-up waves do: tier 2 helps with the
// fix-up and then waits until the utterance's units have all reported (wait_for_fixup), tier 3 steps aside (its states
// come from the fp64 scan wave in the refinement launch).  So a batch without hot chunks pays neither a launch nor a wait
// for the conditioning machinery (as a launch of its own the fix-up cost 4 us of latency and 6 us/step of the pipelined
// rate; with all its workgroups leading this grid, 7 us), and a hot one pays about one fix-up pass inside this launch.
struct ZPassArgs {            // the zero-state pass of `parts` bit 2 (fwdq_body MODE 0)
    const float* ex; int64_t ex_stride; const float* gain; int T;
    // merged chunk pass (lpc_fwdq2m_kernel) next in the stream: its flag words and the non-finite status word start at zero
    unsigned* gflag; int ngflag; unsigned* nonfinite;
};
template <int W, int NT>
struct PrepassLds {           // one workgroup is a fix-up, a zero-state or a composite workgroup: the regions overlap
    using TL = Tile<W, 16>;
    static constexpr int HOT = 4 * kHotListMax * 2;                                   // bytes: the fix-up waves' lists
    static constexpr int COMP = 32 * 32 * 8;                                          // the composites' P_B (doubles)
    static constexpr int ZP = 4 * (TL::SIZE + kGroup * 32) * 4;                       // per wave: input tile + z[16][32]
    static constexpr int BYTES = HOT + (COMP > ZP ? COMP : ZP);
};
template <int W, int NT>
__global__ __launch_bounds__(256) void lpc_group_prepass_kernel(const float* __restrict__ PhiT,
                                                                float* __restrict__ z, float* __restrict__ MT,
                                                                float* __restrict__ V, int NP, int NG, int B,
                                                                int parts, FixArgs fa, int KF1, int KF2,
                                                                float* __restrict__ MTt, ZPassArgs zp) {
    using PL = PrepassLds<W, NT>;
    using TL = Tile<W, 16>;
    __shared__ __attribute__((aligned(32))) unsigned char lds_raw[PL::BYTES];
    unsigned short (*hot_lds)[kHotListMax] = reinterpret_cast<unsigned short (*)[kHotListMax]>(lds_raw);
    double* pb_lds = reinterpret_cast<double*>(lds_raw + PL::HOT);
    light_wave_priority();
    if (zp.gflag && blockIdx.x == 0) {
        for (int i = threadIdx.x; i < zp.ngflag; i += 256) zp.gflag[i] = 0u;
        if (threadIdx.x == 0 && zp.nonfinite) zp.nonfinite[0] = 0u;
    }
    const bool fix = fa.pmax != nullptr && (parts & 1);   // (fa.pmax == nullptr: no fix-up at all; no host path passes that)
    const int nu = NG * B;
    const int nf1 = fix ? B * KF1 : 0, nz = (parts & 2) ? (nu + 3) / 4 : 0, nc = (parts & 1) ? nu : 0;
    int blk = (int)blockIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk < nf1) {
        fixup_wave<W, NT>(fa, blk / KF1, blk % KF1 == 0 && wv == 0, hot_lds[wv]);
        return;
    }
    blk -= nf1;
    if (blk >= nz + nc) {   // trailing fix-up workgroups
        blk -= nz + nc;
        if (fix) fixup_wave<W, NT>(fa, blk / KF2, false, hot_lds[wv]);
        return;
    }
    const bool comp = blk >= nz;
    int b, g;
    float* zl = nullptr;
    if (comp) {
        blk -= nz;
        // the fold of group g runs over the groups BEFORE it: the last composite is needed only when the final partial
        // chunk opens a group of its own (NP a multiple of 16) -- and by the backward's adjoint fold, which runs over the
        // groups ABOVE (training: MTt given)
        if (blk % NG == NG - 1 && NP % kGroup != 0 && !MTt) return;
        b = blk / NG; g = blk % NG;
    } else {
        const int u2 = blk * 4 + wv;
        if (u2 >= nu) return;
        b = u2 / NG; g = u2 % NG;
        if (parts & 4) {   // the zero-state pass of this group's 16 chunks: needs the excitation, not the maps
            float* xt = reinterpret_cast<float*>(lds_raw + PL::HOT) + wv * (TL::SIZE + kGroup * 32);
            zl = xt + TL::SIZE;
            fwdq_body<W, NT, 0>(zp.ex, zp.ex_stride, zp.gain, fa.a, nullptr, z, 0, zp.T, fa.F, fa.M, fa.hop, fa.L, NP, NP,
                                nullptr, xt, nullptr, b, g, lane, nullptr, zl);
            wave_lds_fence();
        }
    }
    if (fa.pmax) {
        const int c = g * kGroup + (lane & 15);
        const float v = c < NP ? fabsf(fa.pmax[(size_t)b * NP + c]) : 0.f;
        if (__builtin_amdgcn_ballot_w64(!(v <= fa.g2)) != 0ull) {   // a chunk of this group may have been recomputed
            const UttTier d = utterance_tier(fa.pmax + (size_t)b * NP, NP, lane, fa.g1, fa.g2, fa.g3, fa.accurate, fa.glog, fa.hot16, fa.hotn);
            if (d.t3) {
                // a tier-3 utterance needs none of this wave's products (its states come from the fp64 scan), but ALL its
                // 199 x 22 map units recomputed as doubles -- 4.3 passes of the 64 fix-up waves an utterance owns.  The
                // utterance's 13 x 5 composite / z-scan waves have nothing else to do: they take units too (round 4:
                // the fix-up of a tier-3 utterance ~2 passes instead of ~4.3)
                if (fix) fixup_wave<W, NT>(fa, b, false, hot_lds[wv]);
                return;
            }
            if (d.nhot > 0u && !fa.accurate) {
                // Help before waiting: the units are claimed from a counter, so this wave takes whatever nobody has claimed
                // yet.  When it returns every unit is done or in the hands of a RESIDENT wave (claiming is what a wave does
                // right before computing), so the wait below ends whatever order the workgroups were dispatched in -- the
                // leading fix-up workgroups are a head start, not a progress guarantee the launch depends on.
                fixup_wave<W, NT>(fa, b, false, hot_lds[wv]);
                wait_for_fixup(fa, b, d.nhot, NT);
            }
        }
    }
    if (comp)    group_composite_wg<W, NT>(PhiT, MT, NP, NG, b, g, pb_lds, MTt);
    else if (zl) group_scan_lds<W, NT>(PhiT, zl, V, b, g, NP, NG, lane);
    else         group_zscan_body<W, NT>(PhiT, z, V, NP, NG, b, g, lane);
}

#ifdef FWDQ2_TIMING   // dev build (tools/fwdq2_phases.py): s_memtime stamps of the chunk-pass waves' phases, lane 0
__device__ unsigned long long g_fq_stamps[2 * 64 * 64 * 8];
#define FQ_STAMP(p, i) do { if ((p) && threadIdx.x == 0) (p)[i] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int golf_debug_fwdq2_stamps(unsigned long long* host_out, int n) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fq_stamps), sizeof(unsigned long long) * (size_t)n, 0, hipMemcpyDeviceToHost);
}
#else
#define FQ_STAMP(p, i) do { } while (0)
#endif

// Prologue of the two-level chunk kernels: start states of the wave's chunks c0 .. c0+16 -> st[17][32] (LDS).
//   t = fold of (M_g', v_g') over the groups before g, then the wave's own chunk maps with inputs x
//   (first pass: v = zero-state group responses, x = z; correction pass: v = the groups' responses to the defects, x = defects).
//   SAMEK (merged chunk pass, lpc_fwdq2m_kernel): the group responses V ([g'][32], this utterance's) and the inputs x of the own
//   maps ([k][32]) are in LDS; `pre` runs between the first map fetches and the fold.
struct NoWait { __device__ __forceinline__ void operator()() const {} };
//   MAPIO 1: the own maps' rows are also left in LDS (mapl[k][NT][W + 4], the lane's row where the lane will look for it: with the
//   4 words of padding sixteen lanes' 16-byte accesses fall on 64 different banks for every ring width) for the
//   stages that need them again; MAPIO 2: they are taken from there (no global fetch: a CU pulls ~11 B/cycle, so four waves
//   re-streaming 34 KB each cost ~5 us per stage however deep the prefetch).
template <int W, int NT, bool THIN = false, bool SAMEK = false, typename PRE = NoWait, int MAPIO = 0>
__device__ __forceinline__ void group_prologue(const float* __restrict__ PhiT, const float* __restrict__ MT,
                                               const float* V, const float* x,
                                               float* __restrict__ st, int b, int g, int NP, int NG, int lane,
                                               unsigned long long* fqs = nullptr, PRE pre = PRE(), float* mapl = nullptr) {
    const bool act = lane < NT;
    const int ii = act ? lane : 0;
    const size_t cstride4 = (size_t)NT * W / 4;
    float t = 0.f;
    // the wave's own chunk maps: first fetches issued before the fold below, so they are in flight during it
    // THIN (GOLF_SS_THROUGHPUT): 4 + 2 maps ahead instead of 6 + 4 -- 196 / 246 VGPRs instead of 290 / 269, so that two chunk-pass
    // waves (or one and a transition wave) share a SIMD's registers; costs a lone batch ~1.3 us per pass (tools/ab2.sh ab_regs)
    constexpr int DC = MAPIO == 2 ? 2 : THIN ? 4 : kPrefetchMaps;
    float4* mapl4 = reinterpret_cast<float4*>(mapl) + ii * (kMapRow<W> / 4);   // the lane's row of map k at + k * NT * kMapRow / 4
    const float4* rows = reinterpret_cast<const float4*>(PhiT + ((size_t)b * NP * NT + ii) * W);
    const float* xb = SAMEK ? x : x + (size_t)b * NP * W + ii;
    const int c0 = g * kGroup;
    float4 pb[DC][W / 4];
    float xx[DC];
    auto fetchc = [&](int u, int c) {
        const int cl = c < NP ? c : NP - 1;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
            if constexpr (MAPIO == 2) pb[u][k] = mapl4[(cl >= c0 ? cl - c0 : 0) * (NT * kMapRow<W> / 4) + k];
            else                      pb[u][k] = rows[(size_t)cl * cstride4 + k];
        }
        if constexpr (SAMEK) xx[u] = x[(cl >= c0 ? cl - c0 : 0) * 32 + ii];
        else                 xx[u] = xb[(size_t)cl * W];
    };
#pragma unroll
    for (int u = 0; u < DC; ++u) fetchc(u, c0 + u);
    pre();   // (SAMEK: the wait for the groups before this one, behind the map fetches just issued; leaves their responses in V)
    {   // (a) the groups before this one
        constexpr int D = THIN ? 2 : kPrefetchComposites;
        const float4* mrows = reinterpret_cast<const float4*>(MT + ((size_t)b * NG * NT + ii) * W);
        const float* vb = SAMEK ? V + ii : V + (size_t)b * NG * 32 + ii;
        float4 mb[D][W / 4];
        float vv[D];
        auto fetch = [&](int u, int gg) {
            const int gl = gg < NG ? gg : NG - 1;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) mb[u][k] = mrows[(size_t)gl * cstride4 + k];
            vv[u] = vb[(size_t)gl * 32];
        };
        const int ng = g < NG ? g : NG;
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, u);
        for (int gb = 0; gb < ng; gb += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                if (gb + u < ng) {   // wave-uniform
                    t = matvec_step<W, NT>(mb[u], t, vv[u], act);
                    fetch(u, gb + u + D);
                }
            }
        }
    }
    FQ_STAMP(fqs, 1);
    {   // (b) the wave's own chunk maps (kGroup = 16 is not a multiple of DC: the slot index runs modulo DC)
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const int u = k % DC;
            const int c = c0 + k;
            if (lane < 32) st[k * 32 + lane] = t;
            if (c < NP) t = matvec_step<W, NT>(pb[u], t, xx[u], act);   // wave-uniform
            if constexpr (MAPIO == 1) {
#pragma unroll
                for (int q = 0; q < W / 4; ++q) mapl4[k * (NT * kMapRow<W> / 4) + q] = pb[u][q];
            }
            if (k + DC < kGroup) fetchc(u, c + DC);
        }
        if (lane < 32) st[kGroup * 32 + lane] = t;
    }
    wave_lds_fence();
}

// The chunk kernels of the two-level path.
//   MODE 3, refinement pass: start states S1 from the prologue (fold of the groups before + scan of the own chunk maps, inputs
//     z), kept in HBM for the final pass; every chunk re-runs from S1_c and leaves its defect d_c = E_c - S1_{c+1}; epilogue:
//     the group's response to its own defects -> V2[b][g].
//   MODE 1, final pass: the SAME prologue run on the defects (composites folded with V2, chunk maps with inputs d) gives the
//     correction delta_c; chunks run from S1_c + delta_c and write y.  (Delta form: see fwdq_body.)
//   Tier-3 utterances (see phi_guard) skip the refinement pass: the waves of rows blockIdx.y >= B of ITS grid share the
//     (tier-3 utterance, group) jobs of the fp64 two-level scan -- composite, group response, and for the wave that
//     completes an utterance the fold into the group start states G64 (this launch has the registers and lasts 26 us
//     anyway); the final pass scans each group's own maps from G64 in its prologue.
#ifndef GOLF_FWDQ2_WAVES
#define GOLF_FWDQ2_WAVES 1   // waves per SIMD the chunk kernels' register allocation must allow (build parameter: A/B of residency)
#endif
template <int W, int NT, int MODE, bool THIN = false>
__global__ __launch_bounds__(64, GOLF_FWDQ2_WAVES) void lpc_fwdq2_kernel(const float* __restrict__ ex, int64_t ex_stride,
                                                       const float* __restrict__ gain, const float* __restrict__ a,
                                                       float* __restrict__ out, int64_t y_stride, int T, int F, int M,
                                                       int hop, int L, int NCQ, const float* __restrict__ PhiT,
                                                       const float* __restrict__ MT, const float* __restrict__ V,
                                                       float* __restrict__ V2out, const float* __restrict__ x, int NP,
                                                       int NG, float* __restrict__ S1,
                                                       const unsigned* __restrict__ tier,
                                                       unsigned* __restrict__ nonfinite, int B,
                                                       const double* __restrict__ Phi64, double* __restrict__ M64,
                                                       double* __restrict__ V64, double* __restrict__ G64,
                                                       unsigned* __restrict__ arrived, const float* __restrict__ zq) {
    static_assert(MODE == 1 || MODE == 3, "final pass or refinement pass");
    light_wave_priority();
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[MODE == 1 ? TL::SIZE : 1];
    __shared__ float st[(kGroup + 1) * 32];
    __shared__ float dl[MODE == 3 ? kGroup * 32 : 1];
    if constexpr (MODE == 3) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            record_scan_kind(tier, B, kScanTwoLevel);
            if (nonfinite) nonfinite[0] = 0u;   // per forward: the final pass (next launch) ORs 1 in when a non-finite sample leaves
        }
        if ((int)blockIdx.y >= B) {
            // fp64 boundary states of tier-3 utterances, two levels (precise_group_job; x = the zero-state responses z): the
            // extra rows' waves share the (utterance, group) jobs -- one utterance's groups land on different waves
            const int w = ((int)blockIdx.y - B) * (int)gridDim.x + (int)blockIdx.x;
            const int nw = ((int)gridDim.y - B) * (int)gridDim.x;
            for (int job = w; job < 2 * B * NG; job += nw) {
                const int bp = job / (2 * NG), r = job - bp * 2 * NG;
                if (tier3(tier, bp))   // wave-uniform
                    precise_group_job<W, NT>(Phi64, x, M64, V64, G64, arrived, bp, r >> 1, NP, NG, threadIdx.x, B, S1, r & 1);
            }
            return;
        }
    }
    const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
    const int c0 = g * kGroup;
    const bool precise = tier3(tier, b);   // wave-uniform
    float* s1b = S1 + (size_t)b * (NP + 1) * 32;
#ifdef FWDQ2_TIMING
    unsigned long long* fqs = (b < 64 && g < 64) ? g_fq_stamps + ((size_t)((MODE == 3 ? 0 : 1) * 64 + b) * 64 + g) * 8 : nullptr;
#else
    unsigned long long* fqs = nullptr;
#endif
    FQ_STAMP(fqs, 0);
    if constexpr (MODE == 3) {
        if (precise) return;
        // (the successor-fold operands below are fetched HERE, ahead of the prologue they do not depend on: a round trip
        //  off the critical path)
        const bool fold_next = c0 + kGroup <= NP;   // wave-uniform; the composite of this group exists (lpc_group_prepass_kernel)
        float4 mb[W / 4];
        float vv = 0.f;
        {
            const int ii = lane < NT ? lane : 0;
            const int gc = fold_next ? g : 0;
            const float4* mrow = reinterpret_cast<const float4*>(MT + (((size_t)b * NG + gc) * NT + ii) * W);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) mb[k] = mrow[k];
            vv = V[((size_t)b * NG + gc) * 32 + ii];
        }
        group_prologue<W, NT, THIN>(PhiT, MT, V, x, st, b, g, NP, NG, lane, fqs);
        FQ_STAMP(fqs, 2);
        // The state the NEXT group starts from is its own fold, M_g S1_{c0} + v_g -- not this wave's scan result st[16]
        // (the two differ by the composite's rounding).  The defect of the group's last chunk has to be taken against the
        // state its successor really runs from, or that difference would never be corrected: recompute the successor's
        // fold step here (same operands, same instruction sequence: bit-identical) and put it in st[16].
        if (fold_next) {
            const bool act = lane < NT;
            const float t0 = lane < 32 ? st[lane] : 0.f;
            const float t1 = matvec_step<W, NT>(mb, t0, vv, act);
            if (lane < 32) st[kGroup * 32 + lane] = t1;
            wave_lds_fence();
        }
        // S1 -> HBM: the own chunks' start states, and S1_{NP} when no later group of this grid owns it
        for (int e = lane; e < kGroup * 32; e += 64)
            if (c0 + e / 32 <= NP) s1b[(size_t)c0 * 32 + e] = st[e];
        if (c0 + kGroup == NP && lane < 32) s1b[(size_t)NP * 32 + lane] = st[kGroup * 32 + lane];
        for (int e = lane; e < kGroup * 32; e += 64) dl[e] = 0.f;
        wave_lds_fence();
    } else {
        if (precise && arrived[2 * B + b] != 0u) {   // tier 3, composites beyond the guard: S1 from the flat fp64 scan
            for (int e = lane; e < (kGroup + 1) * 32; e += 64)
                st[e] = c0 + e / 32 <= NP ? s1b[(size_t)c0 * 32 + e] : 0.f;
        } else if (precise) {
            // tier 3: the group's start state from the fold of the fp64 composites (refinement launch), then the own chunk
            // maps as doubles with the zero-state responses -- the states the fp64 recursion over the whole utterance gives
            for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] = 0.f;
            wave_lds_fence();
            const int c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
            const int n = c1 > c0 ? c1 - c0 : 0;
            const int cs = c0 < NP ? c0 : (NP > 0 ? NP - 1 : 0);
            precise_scan_range<W, NT, float, float>(Phi64 + ((size_t)b * NP + cs) * NT * W, zq + ((size_t)b * NP + cs) * W, W, st,
                                                    32, n, lane, G64 + ((size_t)b * (NG + 1) + g) * 32);
        } else {
            // the first-pass states S1 of the group (written by the refinement pass): all loads issued BEFORE the prologue and
            // added after it.  (As a loop `st[e] += cond ? s1b[..] : 0` this was 9 conditional loads each waited for -- nine
            // serial round trips in front of the recursion; found in round 3 via the same pattern in the frame kernel.)
            constexpr int NE = ((kGroup + 1) * 32 + 63) / 64;
            float s1v[NE];
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = lane + 64 * u;
                const bool ok = e < (kGroup + 1) * 32 && c0 + e / 32 <= NP;
                const float v = s1b[(size_t)c0 * 32 + (ok ? e : 0)];
                s1v[u] = ok ? v : 0.f;
            }
            group_prologue<W, NT, THIN>(PhiT, MT, V, x, st, b, g, NP, NG, lane, fqs);   // delta_c (V = defect responses, x = defects)
            FQ_STAMP(fqs, 2);
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = lane + 64 * u;
                if (e < (kGroup + 1) * 32) st[e] += s1v[u];
            }
        }
        wave_lds_fence();
    }
    FQ_STAMP(fqs, 3);
    fwdq_body<W, NT, MODE, true>(ex, ex_stride, gain, a, nullptr, out, y_stride, T, F, M, hop, L, NCQ, 0, nullptr, xt, yt,
                                 b, g, lane, st, dl, nonfinite);
    FQ_STAMP(fqs, 4);
    if (MODE == 3) {   // epilogue: the group's response to its own defects, for the final pass's fold
        wave_lds_fence();
        group_scan_lds<W, NT>(PhiT, dl, V2out, b, g, NP, NG, lane);
    }
    FQ_STAMP(fqs, 5);
}

// Round 5: refinement pass AND final pass in ONE launch (the third read of the 13.5 MB of chunk maps, the second
// read of the excitation, the S1 / defect round trips through HBM and a launch).  A wave keeps its 16 chunks for both sweeps:
//   phase A = MODE 3 above (first-pass states S1 -> LDS, re-run of the chunks, defects -> LDS, the group's response to them ->
//             Vd[b][g], then ONE release + flag word (b, g));
//   wait      for the flag words of the groups BEFORE g of the same utterance.  Those waves have lower workgroup ids (grid x = group,
//             y = utterance).  Workgroups are dealt round-robin to the 8 XCDs and each XCD dispatches ITS share in id order, so
//             "lower id = dispatched first" holds per XCD, not across the chip.  What makes the wait safe is that the
//             host only takes this kernel when the WHOLE grid is resident at once (one wave per SIMD: grid <= 4 x CUs, launch_fwd)
//             -- then every wave of the launch gets a slot without any other finishing.  Other kernels on the chip can delay
//             that (several of these launches in flight from eager callers on several streams can fill an XCD with each
//             other's waiters; a caller with batches in flight sets GOLF_SS_THROUGHPUT and never gets this kernel), so the
//             spin is bounded, and running out is LOUD: status word 2 bit 1, the non-finite bit, and NaN in the y of the
//             chunks whose start states would have come from unstaged responses;
//   phase B = MODE 1 above: the same prologue on the defects (Vd read past the caches, the own defects from LDS; the maps and the
//             excitation tile come from this XCD's L2, where phase A left them), S1 + delta, chunks -> y.
// Tier-3 utterances: their fp64 jobs ride in the FIRST rows of the grid (dispatched before every wave that waits for them); the
// wave that completes an utterance sets its `ready` word, which the utterance's chunk waves wait for before phase B.
// The flag words are zeroed by the pre-pass launch of the same forward (as is the non-finite status word: here the pass that
// raises it and the pass that used to clear it are one launch).
template <int W, int NT>
__global__ __launch_bounds__(64, GOLF_FWDQ2_WAVES) void lpc_fwdq2m_kernel(
    const float* __restrict__ ex, int64_t ex_stride, const float* __restrict__ gain, const float* __restrict__ a,
    float* __restrict__ y, int64_t y_stride, int T, int F, int M, int hop, int L, int NC, const float* __restrict__ PhiT,
    const float* __restrict__ MT, const float* __restrict__ Vz, float* Vd, const float* __restrict__ z, int NP, int NG,
    float* __restrict__ S1, const unsigned* __restrict__ tier, unsigned* __restrict__ nonfinite, int B,
    const double* __restrict__ Phi64, double* __restrict__ M64, double* __restrict__ V64, double* __restrict__ G64,
    unsigned* __restrict__ arrived, unsigned* gflag, unsigned* __restrict__ timeout_word) {
    light_wave_priority();
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[TL::SIZE];
    __shared__ float st[(kGroup + 1) * 32];
    __shared__ float dl[kGroup * 32];
    __shared__ float s1l[(kGroup + 1) * 32];
    __shared__ float vdl[kMergedMaxGroups * 32];
    // the group's maps, fetched ONCE and kept for the two stages that need them again (where they fit: not the 40-wide ring)
    constexpr bool LM = kGroup * NT * kMapRow<W> * 4 <= 48 * 1024;
    constexpr bool THIN = false;
    __shared__ __attribute__((aligned(16))) float mapl[LM ? kGroup * NT * kMapRow<W> : 4];
    const int lane = threadIdx.x;
    const int nextra = (int)gridDim.y - B;
    unsigned* ready = gflag + (size_t)B * NG;
    if ((int)blockIdx.y < nextra) {   // fp64 boundary states of tier-3 utterances (see lpc_fwdq2_kernel), FIRST in dispatch order
        if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) record_scan_kind(tier, B, kScanTwoLevel);
        const int w = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
        const int nw = nextra * (int)gridDim.x;
        for (int job = w; job < 2 * B * NG; job += nw) {
            const int bp = job / (2 * NG), r = job - bp * 2 * NG;
            if (tier3(tier, bp))   // wave-uniform
                precise_group_job<W, NT>(Phi64, z, M64, V64, G64, arrived, bp, r >> 1, NP, NG, lane, B, S1, r & 1, ready);
        }
        return;
    }
    const int b = (int)blockIdx.y - nextra, g = blockIdx.x;
    const int c0 = g * kGroup;
    const bool precise = tier3(tier, b);   // wave-uniform
    float* s1b = S1 + (size_t)b * (NP + 1) * 32;
    unsigned* fl = gflag + (size_t)b * NG;
    bool lost = false;   // wave-uniform: a bounded wait ran out -- nothing this wave computes from here on can be trusted
    auto timed_out = [&]() { lost = true; if (lane == 0) { atomicOr(timeout_word, 1u); if (nonfinite) atomicOr(nonfinite, 1u); } };
#ifdef FWDQ2_TIMING
    unsigned long long* fqs = (b < 64 && g < 64) ? g_fq_stamps + ((size_t)b * 64 + g) * 8 : nullptr;
#define FQM_STAMP(i) do { if (fqs && lane == 0) fqs[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FQM_STAMP(i) do { } while (0)
#endif
    FQM_STAMP(0);
    if (!precise) {
        // ---- phase A: first-pass states, chunks re-run from them, defects (see MODE 3 of lpc_fwdq2_kernel)
        const bool fold_next = c0 + kGroup <= NP;   // wave-uniform
        float4 mb[W / 4];
        float vv = 0.f;
        {
            const int ii = lane < NT ? lane : 0;
            const int gc = fold_next ? g : 0;
            const float4* mrow = reinterpret_cast<const float4*>(MT + (((size_t)b * NG + gc) * NT + ii) * W);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) mb[k] = mrow[k];
            vv = Vz[((size_t)b * NG + gc) * 32 + ii];
        }
        group_prologue<W, NT, THIN, false, NoWait, LM ? 1 : 0>(PhiT, MT, Vz, z, st, b, g, NP, NG, lane, nullptr, NoWait(), mapl);
        FQM_STAMP(1);
        if (fold_next) {
            const bool act = lane < NT;
            const float t0 = lane < 32 ? st[lane] : 0.f;
            const float t1 = matvec_step<W, NT>(mb, t0, vv, act);
            if (lane < 32) st[kGroup * 32 + lane] = t1;
            wave_lds_fence();
        }
        for (int e = lane; e < (kGroup + 1) * 32; e += 64) s1l[e] = st[e];
        for (int e = lane; e < kGroup * 32; e += 64) dl[e] = 0.f;
        wave_lds_fence();
        if (g < NG) {   // (the final partial chunk in a group of its own, NP a multiple of 16, has no map and no defect)
            fwdq_body<W, NT, 3, true>(ex, ex_stride, gain, a, nullptr, nullptr, (int64_t)0, T, F, M, hop, L, NP, 0, nullptr, xt,
                                      nullptr, b, g, lane, st, dl, nullptr);
            wave_lds_fence();
            FQM_STAMP(2);
            group_scan_lds<W, NT, LM ? 2 : 4, LM, true>(PhiT, dl, Vd, b, g, NP, NG, lane, mapl);
            FQM_STAMP(3);
            // (no agent-scope release: that is a write-back of this XCD's whole L2 -- with other batches' kernels on the chip,
            //  of THEIR output; the 32 words went through to memory, the flag follows once they are acknowledged)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
            if (lane == 0) __hip_atomic_store(fl + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        FQM_STAMP(4);
        // ---- phase B: the correction from the same prologue run on the defects, S1 + delta.  Between its first map fetches and
        // its fold: the wait for the groups before this one, then their responses Vd -> LDS in ONE batch of agent-scope loads
        // (each XCD has its own L2; as loads of the fold they sat in the in-order return queue in front of every map)
        const int npred = g < NG ? g : NG;
        auto wait_and_stage = [&]() {
            for (unsigned it = 0u;; ++it) {
                bool ok = true;
                for (int l = lane; l < npred; l += 64)
                    ok = ok && __hip_atomic_load(fl + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                if (__builtin_amdgcn_ballot_w64(!ok) == 0ull) break;
                __builtin_amdgcn_s_sleep(2);
                if (it > (1u << 17)) { timed_out(); break; }
            }
            FQM_STAMP(5);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // (ordering only)
            const float* vsrc = Vd + (size_t)b * NG * 32;
            float tmp[kMergedMaxGroups / 2];
#pragma unroll
            for (int u = 0; u < kMergedMaxGroups / 2; ++u) {
                const int e = lane + 64 * u;
                tmp[u] = e < npred * 32 ? __hip_atomic_load(vsrc + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kMergedMaxGroups / 2; ++u) vdl[lane + 64 * u] = tmp[u];
            wave_lds_fence();
        };
        group_prologue<W, NT, THIN, true, decltype(wait_and_stage), LM ? 2 : 0>(PhiT, MT, vdl, dl, st, b, g, NP, NG, lane, nullptr,
                                                                               wait_and_stage, mapl);
        for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] += s1l[e];
    } else {
        for (unsigned it = 0u; __hip_atomic_load(ready + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u; ++it) {
            __builtin_amdgcn_s_sleep(8);
            if (it > (1u << 16)) { timed_out(); break; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (__hip_atomic_load(arrived + 2 * B + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {   // S1 from the flat fp64 scan
            for (int e = lane; e < (kGroup + 1) * 32; e += 64)
                st[e] = c0 + e / 32 <= NP ? s1b[(size_t)c0 * 32 + e] : 0.f;
        } else {
            for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] = 0.f;
            wave_lds_fence();
            const int c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
            const int n = c1 > c0 ? c1 - c0 : 0;
            const int cs = c0 < NP ? c0 : (NP > 0 ? NP - 1 : 0);
            precise_scan_range<W, NT, float, float>(Phi64 + ((size_t)b * NP + cs) * NT * W, z + ((size_t)b * NP + cs) * W, W, st,
                                                    32, n, lane, G64 + ((size_t)b * (NG + 1) + g) * 32);
        }
    }
    if (lost)   // never hand out audio computed from start states that did not arrive
        for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] = __builtin_nanf("");
    wave_lds_fence();
    FQM_STAMP(6);
    fwdq_body<W, NT, 1, true>(ex, ex_stride, gain, a, nullptr, y, y_stride, T, F, M, hop, L, NC, 0, nullptr, xt, yt, b, g, lane,
                              st, dl, nonfinite);
    FQM_STAMP(7);
#undef FQM_STAMP
}

// ------------------------------------------------------------------------------------------
// P2: chunk-boundary scan, one wave per utterance, lane i = state component.
//   S[b][c][:] = state at the start of chunk c;  s_{c+1} = Phi_c s_c + z_c.
//   The step is a 22x22 matvec with s broadcast by v_readlane; what bounds it is the latency of
//   fetching Phi_c, so rows are read as float4 (7 loads per chunk: vmcnt only counts 63) and kept
//   D chunks ahead in registers.
//   ACC = false: first pass, S = states from the zero-state responses z.  Blocks [B, 2B) of that launch hold one wave per
//     utterance that returns unless the utterance is tier 3 (see phi_guard): then it writes S from the fp64 scan, and the
//     regular wave of that utterance steps aside (in both passes).
//   ACC = true: correction pass of the delta-form refinement sweep, S += scan of the defects.
// ------------------------------------------------------------------------------------------
template <int W, int NT, int D, bool ACC>
__global__ __launch_bounds__(64) void lpc_p2_scan_kernel(const float* __restrict__ PhiT, const float* __restrict__ z,
                                                         float* __restrict__ S, int NC, int NP, int B,
                                                         const unsigned* __restrict__ tier,
                                                         const double* __restrict__ Phi64,
                                                         unsigned* __restrict__ nonfinite = nullptr) {
    const int i = threadIdx.x;
    if (!ACC && blockIdx.x == 0 && i == 0) {
        record_scan_kind(tier, B, kScanFlat);
        if (nonfinite) nonfinite[0] = 0u;   // per forward (see lpc_fwdq2_kernel)
    }
    if ((int)blockIdx.x >= B) {
        const int bp = (int)blockIdx.x - B;
        if (tier3(tier, bp))
            precise_fwd_scan<W, NT>(Phi64 + (size_t)bp * NP * NT * W, z + (size_t)bp * NP * W, S + (size_t)bp * NC * 64, 64,
                                    NP, i);
        return;
    }
    const int b = blockIdx.x;
    if (tier3(tier, b)) return;
    const bool act = i < NT;
    const int ii = act ? i : 0;
    float* Sb = S + (size_t)b * NC * 64 + i;  // rows padded to 64 floats: every lane stores, no predication
    if (NP <= 0) { if (!ACC) Sb[0] = 0.f; return; }
    const float4* rows = reinterpret_cast<const float4*>(PhiT + ((size_t)b * NP * NT + ii) * W);
    const size_t cstride4 = (size_t)NT * W / 4;
    const float* zb = z + (size_t)b * NP * W + ii;
    float4 buf[D][W / 4];
    float zc[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int cl = u < NP ? u : NP - 1;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) buf[u][k] = rows[(size_t)cl * cstride4 + k];
        zc[u] = zb[(size_t)cl * W];
    }
    float s = 0.f;
#define GOLF_P2_STEP(u)                                                              \
    {                                                                                \
        float acc0 = zc[u], acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;                      \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) {                             \
            const float pj = f4get(buf[u][j / 4], j % 4);                            \
            const float sj = lane_bcast(s, j);                                       \
            if ((j & 3) == 0) acc0 = fmaf(pj, sj, acc0);                             \
            else if ((j & 3) == 1) acc1 = fmaf(pj, sj, acc1);                        \
            else if ((j & 3) == 2) acc2 = fmaf(pj, sj, acc2);                        \
            else acc3 = fmaf(pj, sj, acc3);                                          \
        }                                                                            \
        s = act ? (acc0 + acc1) + (acc2 + acc3) : 0.f;                               \
    }
    int c0 = 0;
    for (; c0 + D <= NP; c0 += D) {  // steady state: straight-line, loads stay D chunks ahead
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int c = c0 + u;
            if (ACC) Sb[(size_t)c * 64] += s; else Sb[(size_t)c * 64] = s;
            GOLF_P2_STEP(u)
            const int cn = c + D < NP ? c + D : NP - 1;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) buf[u][k] = rows[(size_t)cn * cstride4 + k];
            zc[u] = zb[(size_t)cn * W];
        }
    }
#pragma unroll
    for (int u = 0; u < D; ++u) {  // remainder (< D chunks), operands already in registers
        const int c = c0 + u;
        if (c < NP) {
            if (ACC) Sb[(size_t)c * 64] += s; else Sb[(size_t)c * 64] = s;
            GOLF_P2_STEP(u)
        }
    }
#undef GOLF_P2_STEP
    if (ACC) Sb[(size_t)NP * 64] += s; else Sb[(size_t)NP * 64] = s;
}

// ------------------------------------------------------------------------------------------
// Backward: transposed-form adjoint recursion, tap-parallel like the forward:
//     g[t] = gy[t] + lam[0];   lam[k] <- lam[k+1] - A[t,k] g[t]
//   lane r of a quad holds lam[r*TPL .. r*TPL+TPL-1] in a ring p[(k + step) % TPL]; per sample lane 0 forms g and
//   broadcasts it (DPP), every lane pulls lam[(r+1)*TPL] from its right neighbour (DPP shift) and does TPL FMAs.
//   L(c) := the adjoint state at the END of chunk c (= at the start of chunk c+1); L(NP) = 0; lam_start(c) = L(c-1).
//   MODE 0 (B1): lam_end = 0, lam at chunk start -> zadj[(b*NC+c)*W + k]
//   MODE 1 (B3): lam_end = L(c), writes g[b][t] (the adjoint signal dL/dy_total)
//   MODE 2     : refinement sweep of the flat scan: lam_end = L1(c) from HBM, out = the DEFECT lam_start(c) - L1(c-1)
//   MODE 3     : the same with the states in LDS (two-level scan, LS = true): lst[k+1] = L1(c0+k), lst[0] = L1(c0-1)
//   Where the states come from: lamEnd[(b*NC+c)*64 + k] (HBM; LS = false) or lst[(row+1)*32 + k] (LDS; LS = true).
//   A device function of ONE wave, like fwdq_body.
// ------------------------------------------------------------------------------------------
template <int W, int NT, int MODE, bool LS = false>
__device__ __forceinline__ void adjq_body(const float* __restrict__ gy, int64_t gy_stride, const float* __restrict__ a,
                                          const float* __restrict__ lamEnd, float* __restrict__ out, int64_t g_stride,
                                          int T, int F, int M, int hop, int L, int NC, int NCQ,
                                          float* __restrict__ xt, float* __restrict__ yt, int b, int cg, int lane,
                                          const float* lst = nullptr, float* ldl = nullptr) {
    constexpr int TPL = quad_tpl(W, NT);
    constexpr int R = 16;
    using TL = Tile<W, R>;
    static_assert(MODE >= 0 && MODE <= 3 && (MODE != 3 || LS), "MODE 3 exists only with LDS-resident states");
    const int lq = lane / W, lr = lane % W;
    const int row = lane >> 2, r = lane & 3;
    const int c0 = cg * R;
    const int c = c0 + row;
    const bool mine = c < NCQ;
    const BufRow gyrow(gy + (size_t)b * gy_stride, T);
    const BufRow grow(MODE == 1 ? out + (size_t)b * g_stride : nullptr, MODE == 1 ? T : 0);
    float p[TPL];
    if (MODE >= 1 && mine) {
        if constexpr (LS) {
#pragma unroll
            for (int k = 0; k < TPL; ++k) p[k] = lst[(row + 1) * 32 + r * TPL + k];
        } else {
            const float* lp = lamEnd + ((size_t)b * NC + c) * 64 + r * TPL;
#pragma unroll
            for (int k = 0; k < TPL; ++k) p[k] = lp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < TPL; ++k) p[k] = 0.f;
    }
    float a0[TPL], dd[TPL];
#pragma unroll
    for (int k = 0; k < TPL; ++k) { a0[k] = 0.f; dd[k] = 0.f; }
    const float inv_hop = 1.0f / (float)hop;
    int fcur = -1;
    const int nblk = L / W;
    int blk = nblk - 1;
    while (blk > 0 && c0 * L + blk * W >= T) --blk;  // wave-uniform: first block that still has samples
    float nx[TL::ITS];
    TL::fetch(nx, gyrow, c0 * L + blk * W, L, lq, lr);
    for (; blk >= 0; --blk) {
        const int tw = c0 * L + blk * W;
        TL::scatter(xt, nx, lq, lr);
        wave_lds_fence();
        float gin[W];
        TL::rows_load(gin, xt, row);
        TL::fetch(nx, gyrow, tw - W, L, lq, lr);  // prefetch the earlier block (before 0: hardware returns 0)
        const int t0 = c * L + blk * W;
        const bool act = mine && t0 < T;
        float keep[W / 4];
#pragma unroll
        for (int j = 0; j < W / 4; ++j) keep[j] = 0.f;
        if (act) {
            int f = t0 / hop;
            if (f > F - 2) f = F - 2;
            if (f != fcur) {
                fcur = f;
                const float* pa0 = a + ((size_t)b * F + f) * M;
                const float* pa1 = pa0 + M;
#pragma unroll
                for (int k = 0; k < TPL; ++k) {
                    const int i = r * TPL + k;
                    const float v0 = i < M ? pa0[i] : 0.f;
                    const float v1 = i < M ? pa1[i] : 0.f;
                    a0[k] = v0;
                    dd[k] = (v1 - v0) * inv_hop;
                }
            }
            const float n0 = (float)(t0 - f * hop);
#pragma unroll
            for (int s = W - 1; s >= 0; --s) {
                const int st = W - 1 - s;  // steps done in this block; ring index base (W % TPL == 0)
                const float n = n0 + (float)s;
                const float head = p[st % TPL];                 // this lane's lam[r*TPL]
                const float g = dppf<DPP_BC0>(gin[s] + head);    // lane 0: gy + lam[0]
                float inc = dppf<DPP_SHL1>(head);                // right neighbour's lam[(r+1)*TPL]
                inc = r == 3 ? 0.f : inc;                        // lam[4*TPL] = 0
#pragma unroll
                for (int k = 0; k < TPL - 1; ++k) {
                    const float cf = fmaf(n, dd[k], a0[k]);
                    p[(k + st + 1) % TPL] = fmaf(-cf, g, p[(k + st + 1) % TPL]);
                }
                const float cfl = fmaf(n, dd[TPL - 1], a0[TPL - 1]);
                p[st % TPL] = fmaf(-cfl, g, inc);
                if (MODE == 1) keep[s >> 2] = ((s & 3) == r) ? g : keep[s >> 2];
            }
        }
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < W / 4; ++j) yt[row * TL::LD + 4 * j + r] = keep[j];
            wave_lds_fence();
            float o[TL::ITS];
            TL::gather(o, yt, lq, lr);
            TL::store(o, grow, tw, L, lq, lr);
        }
        wave_lds_fence();
    }
    if (MODE != 1 && mine) {
        float* zp = out + ((size_t)b * NC + c) * W;
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
            const int i = r * TPL + k;
            if (i < W) {
                float v = i < NT ? p[k] : 0.f;
                // refinement sweep (see fwdq_body): the defect of this chunk's start state against the state the chunk
                // below really starts from; chunk 0 has no chunk below (its defect feeds nothing)
                if (MODE == 2) v = c >= 1 ? v - lamEnd[((size_t)b * NC + c - 1) * 64 + i] : 0.f;
                if constexpr (MODE == 3) v = c >= 1 ? v - lst[row * 32 + i] : 0.f;
                if (MODE != 2 && ldl) ldl[row * 32 + i] = v;   // (the two-level kernels' epilogue scans these)
                zp[i] = v;
            }
        }
    }
}

template <int W, int NT, int MODE>
__global__ __launch_bounds__(64) void lpc_adjq_kernel(const float* __restrict__ gy, int64_t gy_stride,
                                                      const float* __restrict__ a, const float* __restrict__ lamEnd,
                                                      float* __restrict__ out, int64_t g_stride, int T, int F, int M,
                                                      int hop, int L, int NC, const unsigned* __restrict__ tier = nullptr) {
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[MODE == 1 ? TL::SIZE : 1];
    if (MODE == 0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) check_scan_kind(tier, (int)gridDim.y, kScanFlat);
    if (MODE == 2 && tier3(tier, blockIdx.y)) return;   // tier-3 utterances take no refinement sweep
    adjq_body<W, NT, MODE>(gy, gy_stride, a, lamEnd, out, g_stride, T, F, M, hop, L, NC, NC, xt, yt, blockIdx.y, blockIdx.x,
                           threadIdx.x);
}

// ------------------------------------------------------------------------------------------
// Two-level ADJOINT boundary scan (round 3): the mirror of lpc_fwdq2_kernel for the backward.
//   L(c-1) = Phi_c^T L(c) + zadj_c runs from the top chunk down.  Groups are the forward's (chunks 16 g .. 16 g + 15), so
//   the forward's composites serve transposed: through group g, L(16 g - 1) = M_g^T L(16 g + 15) + w_g.
//   lpc_adjq2_kernel<0>  local adjoints zadj_c of the wave's 16 chunks (B1) + epilogue: the group's response w_g to its own
//                        zadj (16-step scan from zero with Phi_c^T) -> Wz[b][g]
//   lpc_adjq2_kernel<3>  refinement: prologue = fold of (M_g'^T, w_g') over the groups ABOVE (top state L(NP-1) = zadj_NP),
//                        then the own chunks' scan -> L1 (kept in HBM); chunks re-run from L1(c), defects
//                        d_c = lam_start(c) - L1(c-1) (the bottom chunk's against the state the group below really starts
//                        from: one more fold step, bit-identical to that group's own); epilogue: response to the defects -> Wd
//   lpc_adjq2_kernel<1>  final: the same prologue on (Wd, defects, top state 0) = the correction delta; chunks run from
//                        L1 + delta and write g.
//   Tier-3 utterances: the fp64 scan wave (precise_adj_scan) rides in the refinement launch's extra rows and writes L1.
//   st layout (LDS, 17 rows of 32): st[k+1] = L(c0+k), st[0] = L(c0-1).
// ------------------------------------------------------------------------------------------
template <int W, int NT>
__device__ __forceinline__ void adj_group_prologue(const float* __restrict__ Phi, const float* __restrict__ MTt,
                                                   const float* __restrict__ Wv, const float* __restrict__ x, int NC,
                                                   bool with_top, float* __restrict__ st, int b, int g, int NP, int NG,
                                                   int lane) {
    const bool act = lane < NT;
    const int ii = act ? lane : 0;
    const size_t cstride4 = (size_t)NT * W / 4;
    const int c0 = g * kGroup;
    const int gt = NG - 1;                                   // top group with chunk maps
    const int ct = c0 + kGroup - 1 < NP - 1 ? c0 + kGroup - 1 : NP - 1;   // top chunk map of this group (if any)
    // the wave's own chunk maps (rows of Phi: lane j holds row j = column j of Phi^T), first fetches before the fold
    constexpr int DC = kPrefetchMaps;
    const float4* rows = reinterpret_cast<const float4*>(Phi + ((size_t)b * NP * NT + ii) * W);
    const float* xb = x + (size_t)b * NC * W + ii;
    float4 pb[DC][W / 4];
    float xx[DC];
    auto fetchc = [&](int u, int c) {
        const int cl = c < 0 ? 0 : (c < NP ? c : NP - 1);
#pragma unroll
        for (int k = 0; k < W / 4; ++k) pb[u][k] = rows[(size_t)cl * cstride4 + k];
        xx[u] = xb[(size_t)cl * W];
    };
#pragma unroll
    for (int u = 0; u < DC; ++u) fetchc(u, ct - u);
    // state entering the top group: L(NP-1) = zadj_NP (first pass) or 0 (correction pass)
    float t = (with_top && act) ? x[((size_t)b * NC + NP) * W + ii] : 0.f;
    if (g < gt) {   // (a) the groups above this one, from the top down
        constexpr int D = kPrefetchComposites;
        const float4* mrows = reinterpret_cast<const float4*>(MTt + ((size_t)b * NG * NT + ii) * W);
        const float* vb = Wv + (size_t)b * NG * 32 + ii;
        float4 mb[D][W / 4];
        float vv[D];
        auto fetch = [&](int u, int gg) {
            const int gl = gg > g ? gg : g + 1;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) mb[u][k] = mrows[(size_t)gl * cstride4 + k];
            vv[u] = vb[(size_t)gl * 32];
        };
#pragma unroll
        for (int u = 0; u < D; ++u) fetch(u, gt - u);
        for (int gb = gt; gb > g; gb -= D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                if (gb - u > g) {   // wave-uniform
                    t = matvec_step<W, NT>(mb[u], t, vv[u], act);
                    fetch(u, gb - u - D);
                }
            }
        }
    }
    // (b) the own chunks, top down: st[k+1] = L(c0+k); rows above the top chunk map hold L = 0 except ... the top state
    for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] = 0.f;
    wave_lds_fence();
    if (c0 <= NP - 1) {
#pragma unroll
        for (int k = 0; k < kGroup; ++k) {
            const int u = k % DC;
            const int c = ct - k;
            if (c >= c0) {   // wave-uniform
                if (lane < 32) st[(c - c0 + 1) * 32 + lane] = t;
                t = matvec_step<W, NT>(pb[u], t, xx[u], act);
                if (k + DC < kGroup) fetchc(u, c - DC);
            }
        }
        if (lane < 32) st[lane] = t;   // L(c0-1) by the own scan (replaced by the fold value of the group below in MODE 3)
    }
    wave_lds_fence();
}

template <int W, int NT, int MODE>
__global__ __launch_bounds__(64) void lpc_adjq2_kernel(const float* __restrict__ gy, int64_t gy_stride,
                                                       const float* __restrict__ a, float* __restrict__ out,
                                                       int64_t g_stride, int T, int F, int M, int hop, int L, int NC,
                                                       const float* __restrict__ Phi, const float* __restrict__ MTt,
                                                       const float* __restrict__ Wv, float* __restrict__ Wout,
                                                       const float* __restrict__ x, int NP, int NG,
                                                       float* __restrict__ L1, const unsigned* __restrict__ tier, int B,
                                                       const double* __restrict__ Phi64, const double* __restrict__ M64,
                                                       double* __restrict__ W64, double* __restrict__ GA64,
                                                       unsigned* __restrict__ arrived, const float* __restrict__ zq) {
    static_assert(MODE == 0 || MODE == 1 || MODE == 3, "local adjoints, final pass or refinement pass");
    using TL = Tile<W, 16>;
    __shared__ float xt[TL::SIZE];
    __shared__ float yt[MODE == 1 ? TL::SIZE : 1];
    __shared__ float st[(kGroup + 1) * 32];
    __shared__ float dl[kGroup * 32];
    if constexpr (MODE == 0) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) check_scan_kind(tier, B, kScanTwoLevel);
    }
    if constexpr (MODE == 3) {
        if ((int)blockIdx.y >= B) {   // fp64 adjoint boundary states of tier-3 utterances, two levels (x = zadj): see lpc_fwdq2_kernel
            const int w = ((int)blockIdx.y - B) * (int)gridDim.x + (int)blockIdx.x;
            const int nw = ((int)gridDim.y - B) * (int)gridDim.x;
            for (int job = w; job < B * NG; job += nw) {
                const int bp = job / NG, gj = job - bp * NG;
                if (!tier3(tier, bp)) continue;   // wave-uniform
                if (arrived[2 * B + bp] != 0u) {   // the forward found this utterance's composites beyond the guard: flat adjoint scan
                    if (gj == 0)
                        precise_adj_scan<W, NT>(Phi64 + (size_t)bp * NP * NT * W, x + (size_t)bp * NC * W,
                                                L1 + (size_t)bp * (NC + 1) * 32 + 32, 32, NP, threadIdx.x);
                } else {
                    precise_adj_group_job<W, NT>(Phi64, x, M64, W64, GA64, arrived, bp, gj, NP, NC, NG, threadIdx.x);
                }
            }
            return;
        }
    }
    const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
    const int c0 = g * kGroup;
    const bool precise = tier3(tier, b);   // wave-uniform
    float* l1b = L1 + (size_t)b * (NC + 1) * 32;   // row c+1 = L1(c), c = -1 .. NP
    const bool act = lane < NT;
    const int ii = act ? lane : 0;
    if constexpr (MODE == 0) {
        for (int e = lane; e < kGroup * 32; e += 64) dl[e] = 0.f;
        wave_lds_fence();
        adjq_body<W, NT, 0>(gy, gy_stride, a, nullptr, out, 0, T, F, M, hop, L, NC, NC, xt, yt, b, g, lane, nullptr, dl);
        if (g >= NG || precise) return;   // a group without chunk maps (it holds only the final partial chunk)
    } else if constexpr (MODE == 3) {
        if (precise) return;
        float4 mb[W / 4];   // (operands of the fold step below, fetched ahead of the prologue: see lpc_fwdq2_kernel)
        float vv;
        {
            const float4* mrow = reinterpret_cast<const float4*>(MTt + (((size_t)b * NG + g) * NT + ii) * W);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) mb[k] = mrow[k];
            vv = Wv[((size_t)b * NG + g) * 32 + ii];
        }
        adj_group_prologue<W, NT>(Phi, MTt, Wv, x, NC, true, st, b, g, NP, NG, lane);
        if (g >= 1) {   // the state the group BELOW really starts from: its fold step M_g^T L1(c0+15) + w_g, recomputed here
            const int ktop = (c0 + kGroup - 1 < NP - 1 ? kGroup - 1 : NP - 1 - c0);   // row of the group's top chunk map
            const float tin = lane < 32 ? st[(ktop + 1) * 32 + lane] : 0.f;
            const float t1 = matvec_step<W, NT>(mb, tin, vv, act);
            if (lane < 32) st[lane] = t1;
            wave_lds_fence();
        }
        for (int e = lane; e < kGroup * 32; e += 64)   // L1 -> HBM: rows c0+k+1 of this group (c0+k <= NP)
            if (c0 + e / 32 <= NP) l1b[(size_t)(c0 + 1) * 32 + e] = st[32 + e];
        for (int e = lane; e < kGroup * 32; e += 64) dl[e] = 0.f;
        wave_lds_fence();
        adjq_body<W, NT, 3, true>(gy, gy_stride, a, nullptr, out, 0, T, F, M, hop, L, NC, NP, xt, yt, b, g, lane, st, dl);
    } else {
        if (precise && arrived[2 * B + b] != 0u) {   // rows 0 .. NP of L1 hold L(-1) .. L(NP-1) from the flat fp64 scan; L(NP) = 0
            for (int e = lane; e < (kGroup + 1) * 32; e += 64)
                st[e] = c0 + e / 32 <= NP ? l1b[(size_t)c0 * 32 + e] : 0.f;
        } else if (precise) {
            // tier 3: st[k] = L(c0 + k - 1) from the fold of the transposed fp64 composites (refinement launch) and the group's
            // own maps as doubles with zadj; L(NP) = 0
            for (int e = lane; e < (kGroup + 1) * 32; e += 64) st[e] = 0.f;
            wave_lds_fence();
            const int c1 = c0 + kGroup < NP ? c0 + kGroup : NP;
            const int n = c1 > c0 ? c1 - c0 : 0;
            const int cs = c0 < NP ? c0 : (NP > 0 ? NP - 1 : 0);
            const int gt = g + 1 < NG ? g + 1 : NG;
            precise_adj_range<W, NT, float, float, double>(Phi64 + ((size_t)b * NP + cs) * NT * W, zq + ((size_t)b * NC + cs) * W,
                                                           W, st, 32, n, lane, GA64 + ((size_t)b * (NG + 1) + gt) * 32);
        } else {
            constexpr int NE = ((kGroup + 1) * 32 + 63) / 64;   // (loads ahead of the prologue: see lpc_fwdq2_kernel)
            float l1v[NE];
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = lane + 64 * u;
                const bool ok = e < (kGroup + 1) * 32 && c0 + e / 32 <= NP;
                const float v = l1b[(size_t)c0 * 32 + (ok ? e : 0)];
                l1v[u] = ok ? v : 0.f;
            }
            adj_group_prologue<W, NT>(Phi, MTt, Wv, x, NC, false, st, b, g, NP, NG, lane);   // delta (Wv = Wd, x = defects)
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = lane + 64 * u;
                if (e < (kGroup + 1) * 32) st[e] += l1v[u];
            }
        }
        wave_lds_fence();
        adjq_body<W, NT, 1, true>(gy, gy_stride, a, nullptr, out, g_stride, T, F, M, hop, L, NC, NC, xt, yt, b, g, lane, st,
                                  nullptr);
        return;
    }
    // epilogue (MODE 0 / 3): the group's response to its own inputs (zadj_c / defects d_c), scanned from zero, top down
    {
        wave_lds_fence();
        const size_t cstride4 = (size_t)NT * W / 4;
        const float4* rows = reinterpret_cast<const float4*>(Phi + ((size_t)b * NP * NT + ii) * W);
        const int ct = c0 + kGroup - 1 < NP - 1 ? c0 + kGroup - 1 : NP - 1;
        constexpr int D = 4;
        float4 pbuf[D][W / 4];
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int cl = ct - u > c0 ? ct - u : c0;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) pbuf[u][k] = rows[(size_t)cl * cstride4 + k];
        }
        float s = 0.f;
        for (int cb = ct; cb >= c0; cb -= D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int c = cb - u;
                if (c >= c0) {   // wave-uniform
                    const float xi = dl[(c - c0) * 32 + ii];   // zadj_c (MODE 0) / defect d_c (MODE 3), left in LDS by the body
                    s = matvec_step<W, NT>(pbuf[u], s, xi, act);
                    const int cn = c - D > c0 ? c - D : c0;
#pragma unroll
                    for (int k = 0; k < W / 4; ++k) pbuf[u][k] = rows[(size_t)cn * cstride4 + k];
                }
            }
        }
        if (lane < 32) Wout[((size_t)b * NG + g) * 32 + lane] = s;
    }
}

// B2: lamEnd[b][c][:] = adjoint state at the END of chunk c; lam_start(c) = Phi_c^T lam_end(c) + zadj_c.
//   lane j reads row j of Phi (float4 x W/4), D chunks ahead.
//   Blocks [B, 2B): one wave per utterance that returns unless the utterance is tier 3 (see phi_guard): then the scan runs
//   in fp64 over the maps kept as doubles, and the regular wave of that utterance steps aside.
//   ACC: correction pass of the delta-form refinement sweep -- zadj holds the defects, lamEnd += their scan (the top state,
//   L(NP-1), is exact and gets no correction).
template <int W, int NT, int D, bool ACC>
__global__ __launch_bounds__(64) void lpc_adj_scan_kernel(const float* __restrict__ Phi, const float* __restrict__ zadj,
                                                          float* __restrict__ lamEnd, int NC, int NP, int B,
                                                          const unsigned* __restrict__ tier,
                                                          const double* __restrict__ Phi64) {
    const int j = threadIdx.x;
    if ((int)blockIdx.x >= B) {
        const int bp = (int)blockIdx.x - B;
        if (!ACC && tier3(tier, bp))
            precise_adj_scan<W, NT>(Phi64 + (size_t)bp * NP * NT * W, zadj + (size_t)bp * NC * W,
                                    lamEnd + (size_t)bp * NC * 64, 64, NP, j);
        return;
    }
    const int b = blockIdx.x;
    if (tier3(tier, b)) return;
    const bool act = j < NT;
    const int jj = act ? j : 0;
    float* Lb = lamEnd + (size_t)b * NC * 64 + j;  // rows padded to 64 floats
    const float* zb = zadj + (size_t)b * NC * W + jj;
    // last chunk (c = NP) has no transition matrix and lam_end = 0
    if (!ACC) Lb[(size_t)NP * 64] = 0.f;
    float lam = (act && !ACC) ? zb[(size_t)NP * W] : 0.f;
    if (NP <= 0) return;
    const float4* rows = reinterpret_cast<const float4*>(Phi + ((size_t)b * NP * NT + jj) * W);
    const size_t cstride4 = (size_t)NT * W / 4;
    float4 buf[D][W / 4];
    float zc[D];
    // slot u <-> chunk NP-1-(u0+u), descending
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int cl = NP - 1 - u > 0 ? NP - 1 - u : 0;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) buf[u][k] = rows[(size_t)cl * cstride4 + k];
        zc[u] = zb[(size_t)cl * W];
    }
#define GOLF_B2_STEP(u)                                                              \
    {                                                                                \
        float acc0 = zc[u], acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;                      \
        _Pragma("unroll") for (int i = 0; i < NT; ++i) {                             \
            const float pj = f4get(buf[u][i / 4], i % 4);                            \
            const float li = lane_bcast(lam, i);                                     \
            if ((i & 3) == 0) acc0 = fmaf(pj, li, acc0);                             \
            else if ((i & 3) == 1) acc1 = fmaf(pj, li, acc1);                        \
            else if ((i & 3) == 2) acc2 = fmaf(pj, li, acc2);                        \
            else acc3 = fmaf(pj, li, acc3);                                          \
        }                                                                            \
        lam = act ? (acc0 + acc1) + (acc2 + acc3) : 0.f;                             \
    }
    int u0 = 0;
    for (; u0 + D <= NP; u0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int c = NP - 1 - (u0 + u);
            if (ACC) Lb[(size_t)c * 64] += lam; else Lb[(size_t)c * 64] = lam;
            GOLF_B2_STEP(u)
            const int cn = c - D > 0 ? c - D : 0;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) buf[u][k] = rows[(size_t)cn * cstride4 + k];
            zc[u] = zb[(size_t)cn * W];
        }
    }
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int c = NP - 1 - (u0 + u);
        if (c >= 0) {
            if (ACC) Lb[(size_t)c * 64] += lam; else Lb[(size_t)c * 64] = lam;
            GOLF_B2_STEP(u)
        }
    }
#undef GOLF_B2_STEP
}

// B3b: parallel part of the backward.  One WAVE per gradient segment (4 segments per workgroup), lane k = tap
//   (lane NT = the gain term):
//   g_ex[t] = g[t]*G[t];  per-segment hat-weighted correlations
//   V0[k] = sum_t -g[t] y[t-1-k],  V1[k] = sum_t -n g[t] y[t-1-k]   (n = t - f*hop)
//   U0    = sum_t  g[t] ex[t],     U1    = sum_t  n g[t] ex[t]
// (the reference forms a (B,T,M) gradient tensor and back-propagates through F.interpolate).
__global__ __launch_bounds__(256) void lpc_grad_corr_kernel(const float* __restrict__ g, int64_t g_stride,
                                                            const float* __restrict__ y, int64_t y_stride,
                                                            const float* __restrict__ ex, int64_t ex_stride,
                                                            const float* __restrict__ gain, float* __restrict__ g_ex,
                                                            int64_t g_ex_stride, float* __restrict__ pa,
                                                            float* __restrict__ pg, int T, int F, int NT, int W,
                                                            int hop, int seg, int NSEG, int tail) {
    // per wave: (g, n g) pairs, ex and y (with 64 samples of history) of the segment.  One loop serves every lane: tap
    // lanes correlate the pairs with y[t-1-k], the gain lane with ex[t] -- two packed FMAs per two samples and lane
    // (first version: scalar FMAs, the n-weights formed in the loop and a second, divergent loop for the gain lane:
    // 24 instructions per four samples where this has 8; 17.6 us -> see DESIGN.md)
    __shared__ __attribute__((aligned(16))) f32x2 gp_[4][256 + 4];
    __shared__ float es_[4][256 + 4], ys_[4][256 + 64 + 4];
    const int wv = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int sg = blockIdx.x * 4 + wv, b = blockIdx.y;
    if (sg >= NSEG) return;  // whole wave
    if (sg == NSEG - 1)      // GOLF_SS_ZERO_TAIL: the excitation was longer than the output, its gradient there is zero
        for (int u = k; u < tail; u += 64) g_ex[(size_t)b * g_ex_stride + T + u] = 0.f;
    f32x2* gp = gp_[wv];
    float* es = es_[wv];
    float* ys = ys_[wv];
    const int ts = sg * seg;
    const int len = (ts + seg <= T ? seg : T - ts);  // 1..256
    int f = ts / hop;
    if (f > F - 2) f = F - 2;
    const int nbase = ts - f * hop;
    const float g0 = gain[(size_t)b * F + f];
    const float dg = (gain[(size_t)b * F + f + 1] - g0) / (float)hop;
    const float* gb = g + (size_t)b * g_stride;
    const float* yb = y + (size_t)b * y_stride;
    const float* eb = ex + (size_t)b * ex_stride;
    {   // every load of the staging issued before the first use (as loops with the loads under `if (u < len)` these were
        // 4 + 5 serial round trips per wave)
        float gv[4], ev[4], yv[5];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = k + 64 * q;
            const int uc = u < len ? u : 0;
            gv[q] = gb[ts + uc];
            ev[q] = eb[ts + uc];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int t = ts - 64 + k + 64 * q;
            yv[q] = yb[(t >= 0 && t < T) ? t : 0];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = k + 64 * q;
            const float n = (float)(nbase + u);
            const float g = u < len ? gv[q] : 0.f;
            if (u < len) g_ex[(size_t)b * g_ex_stride + ts + u] = g * fmaf(n, dg, g0);
            gp[u] = f32x2{g, g * n};   // zero beyond the segment
            es[u] = u < len ? ev[q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) {  // ys[u] = y[ts - 64 + u]
            const int u = k + 64 * q, t = ts - 64 + u;
            ys[u] = (t >= 0 && t < T) ? yv[q] : 0.f;
        }
    }
    __builtin_amdgcn_s_waitcnt(0);  // single wave owns its LDS rows
    __builtin_amdgcn_wave_barrier();
    const int len4 = (len + 3) & ~3;
    // Lanes kk = 0..NT-1 own one tap each, lane NT the gain: with NT + 1 <= 32 the two halves of the wave take the
    // two halves of the segment (first version: 23 of 64 lanes busy for the whole segment, 27 us).
    const bool split = NT + 1 <= 32;
    const int half = split ? k >> 5 : 0, kk = split ? k & 31 : k;
    const int tmid = split ? ((len4 / 4 + 1) / 2) * 4 : len4;
    const int tb = half ? tmid : 0, te = half ? len4 : tmid;
    f32x2 acc[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
    if (kk <= NT) {
        const float* yk = kk < NT ? ys + 63 - kk : es;  // yk[t] = y[ts + t - 1 - kk]  /  ex[ts + t]
        for (int t = tb; t < te; t += 4) {
            const f32x4v p01 = *reinterpret_cast<const f32x4v*>(gp + t), p23 = *reinterpret_cast<const f32x4v*>(gp + t + 2);
            const float y0 = yk[t], y1 = yk[t + 1], y2 = yk[t + 2], y3 = yk[t + 3];
            acc[0] = __builtin_elementwise_fma(f32x2{p01[0], p01[1]}, f32x2{y0, y0}, acc[0]);
            acc[1] = __builtin_elementwise_fma(f32x2{p01[2], p01[3]}, f32x2{y1, y1}, acc[1]);
            acc[2] = __builtin_elementwise_fma(f32x2{p23[0], p23[1]}, f32x2{y2, y2}, acc[2]);
            acc[3] = __builtin_elementwise_fma(f32x2{p23[2], p23[3]}, f32x2{y3, y3}, acc[3]);
        }
    }
    const f32x2 accs = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    float v0 = accs.x, v1 = accs.y;
    if (split) {
        v0 += __shfl_down(v0, 32);
        v1 += __shfl_down(v1, 32);
    }
    if (half == 0) {
        if (kk < NT) {
            float* pp = pa + ((size_t)b * NSEG + sg) * 2 * W;
            pp[kk] = -v0;
            pp[W + kk] = -v1;
        } else if (kk == NT) {
            pg[((size_t)b * NSEG + sg) * 2 + 0] = v0;
            pg[((size_t)b * NSEG + sg) * 2 + 1] = v1;
        }
    }
}

__global__ void lpc_grad_reduce_kernel(const float* __restrict__ pa, const float* __restrict__ pg,
                                       float* __restrict__ g_a, float* __restrict__ g_gain, int B, int F, int M,
                                       int W, int hop, int seg, int NSEG) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = M + 1;
    if (idx >= B * F * per) return;
    const int k = idx % per;
    const int f = (idx / per) % F;
    const int b = idx / (per * F);
    const int R = hop / seg;
    const float inv_hop = 1.0f / (float)hop;
    float acc = 0.f;
    // segments whose frame is f contribute V0 - V1/hop; segments whose frame is f-1 contribute V1/hop
    const int lo = (f - 1) * R < 0 ? 0 : (f - 1) * R;
    const int hi = (f + 2) * R < NSEG ? (f + 2) * R : NSEG;
    for (int sg = lo; sg < hi; ++sg) {
        int fs = sg / R;
        if (fs > F - 2) fs = F - 2;
        float v0, v1;
        if (k < M) {
            const float* pp = pa + ((size_t)b * NSEG + sg) * 2 * W;
            v0 = pp[k];
            v1 = pp[W + k];
        } else {
            v0 = pg[((size_t)b * NSEG + sg) * 2 + 0];
            v1 = pg[((size_t)b * NSEG + sg) * 2 + 1];
        }
        if (fs == f) acc += v0 - v1 * inv_hop;
        if (fs == f - 1) acc += v1 * inv_hop;
    }
    if (k < M) g_a[((size_t)b * F + f) * M + k] = acc;
    else g_gain[(size_t)b * F + f] = acc;
}

// a-5 inverse filter: fully parallel FIR with interpolated coefficients.
__global__ void lpc_inverse_kernel(const float* __restrict__ y, int64_t y_stride, const float* __restrict__ a,
                                   float* __restrict__ e, int64_t e_stride, int B, int T, int F, int M, int hop) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * T) return;
    const int b = (int)(idx / T), t = (int)(idx - (int64_t)b * T);
    int f = F >= 2 ? t / hop : 0;
    if (F >= 2 && f > F - 2) f = F - 2;
    const float w = (float)(t - f * hop) / (float)hop;
    const float* pa0 = a + ((size_t)b * F + f) * M;
    const float* pa1 = F >= 2 ? pa0 + M : pa0;
    const float* yb = y + (size_t)b * y_stride;
    float acc = yb[t];
    for (int i = 0; i < M; ++i) {
        if (t - 1 - i < 0) break;
        const float cf = fmaf(w, pa1[i] - pa0[i], pa0[i]);
        acc = fmaf(cf, yb[t - 1 - i], acc);
    }
    e[(size_t)b * e_stride + t] = acc;
}

// Backward of the analysis filter e[t] = y[t] + sum_i A[t,i] y[t-1-i]  (A = up(a)):
//   g_y[t]   = g_e[t] + sum_i A[t+1+i, i] g_e[t+1+i]
//   g_a[f,i] = sum_t hat_f(t) g_e[t] y[t-1-i]      (hat_f = the interpolation weights of frame f: up^T)
__global__ void lpc_inverse_bwd_y_kernel(const float* __restrict__ ge, int64_t ge_stride, const float* __restrict__ a,
                                         float* __restrict__ gy, int64_t gy_stride, int B, int T, int F, int M,
                                         int hop) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * T) return;
    const int b = (int)(idx / T), t = (int)(idx - (int64_t)b * T);
    const float* gb = ge + (size_t)b * ge_stride;
    float acc = gb[t];
    for (int i = 0; i < M; ++i) {
        const int u = t + 1 + i;
        if (u >= T) break;
        int f = F >= 2 ? u / hop : 0;
        if (F >= 2 && f > F - 2) f = F - 2;
        const float w = (float)(u - f * hop) / (float)hop;
        const float* pa0 = a + ((size_t)b * F + f) * M;
        const float* pa1 = F >= 2 ? pa0 + M : pa0;
        acc = fmaf(fmaf(w, pa1[i] - pa0[i], pa0[i]), gb[u], acc);
    }
    gy[(size_t)b * gy_stride + t] = acc;
}

// one wave per (b, f): lanes stride over the (at most 2*hop+1) samples whose interpolation touches frame f
__global__ __launch_bounds__(64) void lpc_inverse_bwd_a_kernel(const float* __restrict__ ge, int64_t ge_stride,
                                                               const float* __restrict__ y, int64_t y_stride,
                                                               float* __restrict__ g_a, int T, int F, int M, int hop) {
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float* gb = ge + (size_t)b * ge_stride;
    const float* yb = y + (size_t)b * y_stride;
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
    // samples t with segment index s(t) = min(t / hop, F-2): weight (1-w) on frame s, w on frame s+1
    int t_lo = (f - 1) * hop, t_hi = (f + 1) * hop;  // [t_lo, t_hi)
    if (f == F - 1) t_hi = T;                        // the clamped tail belongs to segment F-2
    if (t_lo < 0) t_lo = 0;
    if (t_hi > T) t_hi = T;
    const float inv_hop = 1.0f / (float)hop;
    for (int t = t_lo + lane; t < t_hi; t += 64) {
        int sgm = F >= 2 ? t / hop : 0;
        if (F >= 2 && sgm > F - 2) sgm = F - 2;
        const float w = F >= 2 ? (float)(t - sgm * hop) * inv_hop : 0.f;
        const float wt = sgm == f ? 1.0f - w : (sgm == f - 1 ? w : 0.f);
        const float gv = gb[t] * wt;
        for (int i = 0; i < M; ++i) {
            if (t - 1 - i < 0) break;
            acc[i] = fmaf(gv, yb[t - 1 - i], acc[i]);
        }
    }
    for (int i = 0; i < M; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) g_a[((size_t)b * F + f) * M + i] = v;
    }
}

// Conditioning / health status of the forward that last used a workspace (golf_ltv_allpole_status_u32): one workgroup.
__global__ __launch_bounds__(256) void lpc_status_kernel(const unsigned* __restrict__ tier,
                                                         const unsigned* __restrict__ status,
                                                         const unsigned* __restrict__ fixcnt,
                                                         const float* __restrict__ pmax, int B, int NP,
                                                         unsigned* __restrict__ out) {
    __shared__ unsigned sh[3][256];
    unsigned nh = 0u, n3 = 0u, mx = 0u;
    for (int b = threadIdx.x; b < B; b += 256) {
        nh += tier[2 * b + 1] > 0u ? 1u : 0u;
        n3 += tier[2 * b] == kTierPrecise ? 1u : 0u;
    }
    for (int64_t q = threadIdx.x; q < (int64_t)B * NP; q += 256) mx = max(mx, __float_as_uint(fabsf(pmax[q])));
    sh[0][threadIdx.x] = nh; sh[1][threadIdx.x] = n3; sh[2][threadIdx.x] = mx;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
            sh[2][threadIdx.x] = max(sh[2][threadIdx.x], sh[2][threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = sh[0][0]; out[1] = sh[1][0]; out[3] = sh[2][0];
        // bit 0: a non-finite sample left the filter, bit 1: a wait for the fix-up timed out, bit 2: a backward ran on this
        // workspace with another boundary scan than the forward that filled it
        out[2] = (status[0] ? 1u : 0u) | (fixcnt[2 * B] ? 2u : 0u) | (tier[2 * B + 1] ? 4u : 0u);
    }
}
__global__ void lpc_status_zero_kernel(unsigned* __restrict__ out) { if (threadIdx.x < 4) out[threadIdx.x] = 0u; }

// ------------------------------------------------------------------------------------------
// host-side dispatch
// ------------------------------------------------------------------------------------------
// CU count of the CURRENT device (cached per device id: a process may drive several GPUs)
static int device_cu_count() {
    constexpr int kMaxDev = 16;
    static int cache[kMaxDev] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
    if (cache[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

// Conditioning tiers (see phi_guard): the arguments of the fix-up.  Maps that come from fp64 trajectories already (not
// `fast`: the training path) are `accurate`, only tier-3 utterances get their doubles.
static FixArgs fix_args(const SsPlan& p, const SsChain& c, const float* a, int B, int F, int M, int hop, char* ws) {
    FixArgs fa;
    fa.a = a;
    fa.PhiT = (float*)(ws + p.off_phiT);
    fa.Phi = (c.training && c.fast) ? (float*)(ws + p.off_phi) : nullptr;
    fa.Phi64 = (double*)(ws + p.off_phi64);
    fa.pmax = (const float*)(ws + p.off_pmax);
    fa.tier = (unsigned*)(ws + p.off_tier);
    fa.status = (unsigned*)(ws + p.off_status);
    fa.fixcnt = (unsigned*)(ws + p.off_fixcnt);
    fa.F = F; fa.M = M; fa.hop = hop; fa.L = p.L; fa.NP = p.NP;
    fa.B = B;
    fa.g1 = phi_guard(); fa.g2 = phi_guard2(); fa.g3 = phi_guard3(); fa.glog = group_log2_guard();
    fa.hot16 = hot_all_16ths();
    fa.hotn = hot_count();
    fa.accurate = c.fast ? 0 : 1;
    return fa;
}

// ... as a launch of its own (flat-scan path)
template <int W, int NT>
static int launch_fixup(const SsPlan& p, const SsChain& c, const float* a, int B, int F, int M, int hop, char* ws,
                        hipStream_t st) {
    hipLaunchKernelGGL((lpc_fixup_kernel<W, NT>), dim3((unsigned)(c.k1 + c.k2), B), dim3(256), 0, st,
                       fix_args(p, c, a, B, F, M, hop, ws));
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

// Transitions prepared ahead of the excitation: what the forward's boundary scan derives from the matrices alone -- the
// fix-up of hot chunk maps and, with the two-level scan, the group composites (one launch).
template <int W, int NT>
static int launch_composites(const SsPlan& p, const SsChain& c, const float* a, int B, int F, int M, int hop, char* ws,
                             hipStream_t st) {
    if constexpr (NT <= 24) {
        if (c.two_level) {
            hipLaunchKernelGGL((lpc_group_prepass_kernel<W, NT>), dim3((unsigned)(c.nf + c.nu)), dim3(256), 0, st,
                               (const float*)(ws + p.off_phiT), (float*)nullptr, (float*)(ws + p.off_mt),
                               (float*)nullptr, p.NP, p.NG, B, 1, fix_args(p, c, a, B, F, M, hop, ws), c.k1, c.k2,
                               c.training ? (float*)(ws + p.off_mtT) : (float*)nullptr, ZPassArgs{nullptr, 0, nullptr, 0});
            GOLF_LAUNCH_CHECK();
            return GOLF_OK;
        }
    }
    return launch_fixup<W, NT>(p, c, a, B, F, M, hop, ws, st);
}

// The fp32 transition matrices alone (+ their per-chunk maxima): needs only the coefficients.
template <int W, int NT>
static int launch_maps(const SsPlan& p, const float* a, int B, int F, int M, int hop, char* ws, bool training, hipStream_t st) {
    float* Phi = (float*)(ws + p.off_phi);
    float* PhiT = (float*)(ws + p.off_phiT);
    const int nq = B * p.NP;
    hipLaunchKernelGGL((lpc_p1f_kernel<W, NT, 2>), dim3((unsigned)ceil_div(nq, P1fGeom<W, NT, 2>::CPW * P1F_WPB)),
                       dim3(64 * P1F_WPB), 0, st, a, PhiT, F, M, hop, p.L, p.NP, nq, (float*)(ws + p.off_pmax),
                       (unsigned*)(ws + p.off_fixcnt), B, training ? Phi : (float*)nullptr);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

template <int W, int NT>
static int launch_transitions(const SsPlan& p, const SsChain& c, bool composites, const float* a, int B, int F, int M,
                              int hop, char* ws, hipStream_t st) {
    if (p.NP <= 0) return GOLF_OK;
    if (c.fast) {  // fp32 trajectories as float2 pairs (the forward then runs one refinement sweep)
        if (int rc = launch_maps<W, NT>(p, a, B, F, M, hop, ws, c.training, st)) return rc;
        if (!composites) return GOLF_OK;   // the forward runs the fix-up and the composites itself
        return launch_composites<W, NT>(p, c, a, B, F, M, hop, ws, st);
    }
    float* Phi = (float*)(ws + p.off_phi);
    float* PhiT = (float*)(ws + p.off_phiT);
    const int nq = B * p.NP;
    constexpr int NG = (NT + 2) / 3;
    hipLaunchKernelGGL((lpc_p1h_kernel<W, NT, 3, double>), dim3((unsigned)ceil_div(ceil_div(nq, 64) * NG, 4)),
                       dim3(256), 0, st, a, Phi, PhiT, F, M, hop, p.L, p.NP, nq);
    GOLF_LAUNCH_CHECK();
    hipLaunchKernelGGL((lpc_transpose_kernel<W, NT>), dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st,
                       (const float*)Phi, PhiT, nq, (float*)(ws + p.off_pmax), (unsigned*)(ws + p.off_fixcnt), B);
    GOLF_LAUNCH_CHECK();
    return composites ? launch_composites<W, NT>(p, c, a, B, F, M, hop, ws, st) : GOLF_OK;
}

// Fork/join helper: `side` runs P1h (needs only `a`) while `st` runs P1z (needs the excitation).
// Events come from a small per-thread ring that is never destroyed (destroying an event another stream still
// waits on proved racy); an event is reused only 64 fork/joins later, long after its wait has been consumed.
struct ForkJoin {
    static hipEvent_t next_event() {
        // events belong to the device that was current when they were created: one ring per (thread, device)
        constexpr int kMaxDev = 16;
        static thread_local hipEvent_t ring[kMaxDev][64] = {};
        static thread_local unsigned head[kMaxDev] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
        hipEvent_t& e = ring[dev][head[dev]++ & 63];
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        return e;
    }
    int record_and_wait(hipStream_t from, hipStream_t to) {
        hipEvent_t ev = next_event();
        if (!ev) return 1;
        if (hipEventRecord(ev, from) != hipSuccess) return 1;
        if (hipStreamWaitEvent(to, ev, 0) != hipSuccess) return 1;
        return 0;
    }
};

// ss_chain's decisions in launch order
template <int W, int NT>
static int launch_fwd(const SsPlan& p, const SsChain& c, int n_cu, const float* ex, int64_t ex_stride, const float* gain,
                      const float* a, float* y, int64_t y_stride, int B, int T, int F, int M, int hop, char* ws,
                      hipStream_t side, hipStream_t st) {
    float* PhiT = (float*)(ws + p.off_phiT);
    float* z = (float*)(ws + p.off_z);
    float* S = (float*)(ws + p.off_S);
    const unsigned* tier = p.NP > 0 ? (const unsigned*)(ws + p.off_tier) : nullptr;
    unsigned* nonfinite = (unsigned*)(ws + p.off_status);
    const double* Phi64 = (const double*)(ws + p.off_phi64);
    constexpr int D = 8;
    ForkJoin fork, join;
    switch (c.maps) {
        case SsMaps::Own:   // the matrices alone; fix-up, composites and the zero-state pass follow in the pre-pass launch
            if (int rc = launch_maps<W, NT>(p, a, B, F, M, hop, ws, c.training, st)) return rc;
            break;
        case SsMaps::WithZeroState: {   // transitions + zero-state pass in one launch
            constexpr int KT = 3;
            const int nq = B * p.NP, ncg = (int)ceil_div(p.NP, 16);
            const int64_t nunit = (int64_t)ncg * B;
            const int nblk = c.fast ? (int)ceil_div(nq, P1fGeom<W, NT>::CPW * P1F_WPB) : (int)ceil_div(ceil_div(nq, 64) * ((NT + KT - 1) / KT), 4);
            const int upw = ss_upw(nblk, nunit, n_cu), nblk_z = (int)ceil_div(nunit, 4 * upw);
            if (c.fast) {
                hipLaunchKernelGGL((lpc_p1fz_kernel<W, NT>), dim3((unsigned)(nblk + nblk_z)), dim3(64 * P1F_WPB),
                                   0, st, ex, ex_stride, gain, a, z, PhiT, T, F, M, hop, p.L, p.NP, nq, nblk, ncg,
                                   B, upw, (float*)(ws + p.off_pmax), (unsigned*)(ws + p.off_fixcnt),
                                   c.training ? (float*)(ws + p.off_phi) : (float*)nullptr);
                GOLF_LAUNCH_CHECK();
            } else {
                float* Phi = (float*)(ws + p.off_phi);
                hipLaunchKernelGGL((lpc_p1hz_kernel<W, NT, KT>), dim3((unsigned)(nblk + nblk_z)), dim3(256), 0, st,
                                   ex, ex_stride, gain, a, z, Phi, PhiT, T, F, M, hop, p.L, p.NP, nq, nblk, ncg, B,
                                   upw);
                GOLF_LAUNCH_CHECK();
                hipLaunchKernelGGL((lpc_transpose_kernel<W, NT>), dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st,
                                   (const float*)Phi, PhiT, nq, (float*)(ws + p.off_pmax),
                                   (unsigned*)(ws + p.off_fixcnt), B);
                GOLF_LAUNCH_CHECK();
            }
            break;
        }
        case SsMaps::ViaTransitions:   // with the fix-up and the composites, beside the zero-state pass
            if (c.fork && fork.record_and_wait(st, side)) return fail((int)hipErrorUnknown, "ltv_allpole_fwd: stream fork failed");
            if (int rc = launch_transitions<W, NT>(p, c, true, a, B, F, M, hop, ws, c.fork ? side : st)) return rc;
            break;
        default: break;   // None, Have
    }
    if (c.zero_state == SsZeroState::Own) {
        // the zero-state pass as a launch of its own (prepared transitions, side stream, SPLIT_P1)
        hipLaunchKernelGGL((lpc_fwdq_kernel<W, NT, 0>), dim3((unsigned)ceil_div(p.NP, 16), B), dim3(64), 0, st, ex,
                           ex_stride, gain, a, (const float*)nullptr, z, (int64_t)0, T, F, M, hop, p.L, p.NP, p.NP,
                           (const float*)nullptr, (const unsigned*)nullptr);
        GOLF_LAUNCH_CHECK();
    }
    if (c.join && join.record_and_wait(side, st)) return fail((int)hipErrorUnknown, "ltv_allpole_fwd: stream join failed");
    if constexpr (NT <= 24) {
        if (c.two_level) {   // two-level boundary scan (see the kernels above)
            float* MT = (float*)(ws + p.off_mt);
            float* Vz = (float*)(ws + p.off_gv);                    // [b][NG][32] zero-state group responses
            float* Vd = Vz + (size_t)B * p.NG * 32;                   // ... and the groups' responses to the defects
            float* dfc = (float*)(ws + p.off_z2);                     // defects E_c - S1_{c+1} of the refinement pass
            float* S1 = (float*)(ws + p.off_S1);                      // first-pass chunk start states
            double* M64 = (double*)(ws + p.off_m64);                  // tier 3: fp64 group composites, responses, start states
            double* V64 = (double*)(ws + p.off_v64);
            double* G64 = (double*)(ws + p.off_g64);
            unsigned* arrived = (unsigned*)(ws + p.off_fixcnt) + 2 * (size_t)B + 1;
            const int gxf = (int)ceil_div(p.NC, kGroup);
            unsigned* gflag = (unsigned*)(ws + p.off_gflag);
            // transitions prepared ahead (HAVE_TRANSITIONS) or forked onto the side stream: their composites came with them
            const int count = (c.owed == SsOwed::Prepass ? c.nf + c.nu : 0) + c.nz;   // in workgroups
            hipLaunchKernelGGL((lpc_group_prepass_kernel<W, NT>), dim3((unsigned)count), dim3(256), 0, st,
                               (const float*)PhiT, z, MT, Vz, p.NP, p.NG, B, c.parts, fix_args(p, c, a, B, F, M, hop, ws),
                               c.k1, c.k2, c.training ? (float*)(ws + p.off_mtT) : (float*)nullptr,
                               ZPassArgs{ex, ex_stride, gain, T, c.merged ? gflag : (unsigned*)nullptr, B * (p.NG + 1), nonfinite});
            GOLF_LAUNCH_CHECK();
            // refinement pass (both precisions of the maps: the sweep is what makes the states the sequential recursion's)
            const int gx3 = (int)ceil_div(p.NP, kGroup);
            if (c.merged) {   // refinement + final pass in one launch (lpc_fwdq2m_kernel)
                hipLaunchKernelGGL((lpc_fwdq2m_kernel<W, NT>), dim3((unsigned)gxf, B + (int)ceil_div(B, gxf)), dim3(64), 0, st, ex,
                                   ex_stride, gain, a, y, y_stride, T, F, M, hop, p.L, p.NC, (const float*)PhiT, (const float*)MT,
                                   (const float*)Vz, Vd, (const float*)z, p.NP, p.NG, S1, tier, nonfinite, B, Phi64, M64, V64, G64,
                                   arrived, gflag, (unsigned*)(ws + p.off_fixcnt) + 2 * (size_t)B);
                GOLF_LAUNCH_CHECK();
                return GOLF_OK;
            }
#define GOLF_FWDQ2_LAUNCH(THINV)                                                                                              \
            hipLaunchKernelGGL((lpc_fwdq2_kernel<W, NT, 3, THINV>), dim3((unsigned)gx3, B + (int)ceil_div(B, gx3)), dim3(64), 0,  \
                               st, ex, ex_stride, gain, a, dfc, (int64_t)0, T, F, M, hop, p.L, p.NP, (const float*)PhiT,        \
                               (const float*)MT, (const float*)Vz, Vd, (const float*)z, p.NP, p.NG, S1, tier, nonfinite, B,  \
                               Phi64, M64, V64, G64, arrived, (const float*)z);                                                \
            GOLF_LAUNCH_CHECK();                                                                                               \
            hipLaunchKernelGGL((lpc_fwdq2_kernel<W, NT, 1, THINV>), dim3((unsigned)gxf, B), dim3(64), 0, st, ex, ex_stride,    \
                               gain, a, y, y_stride, T, F, M, hop, p.L, p.NC, (const float*)PhiT, (const float*)MT,            \
                               (const float*)Vd, (float*)nullptr, (const float*)dfc, p.NP, p.NG, S1, tier, nonfinite, B,       \
                               Phi64, M64, V64, G64, arrived, (const float*)z);
            if (c.thin) { GOLF_FWDQ2_LAUNCH(true) } else { GOLF_FWDQ2_LAUNCH(false) }
#undef GOLF_FWDQ2_LAUNCH
            GOLF_LAUNCH_CHECK();
            return GOLF_OK;
        }
    }
    if (c.owed == SsOwed::Fixup)   // (otherwise launch_transitions / the caller's transitions call ran it)
        if (int rc = launch_fixup<W, NT>(p, c, a, B, F, M, hop, ws, st)) return rc;
    hipLaunchKernelGGL((lpc_p2_scan_kernel<W, NT, D, false>), dim3(2 * B), dim3(64), 0, st, (const float*)PhiT,
                       (const float*)z, S, p.NC, p.NP, B, tier, Phi64, nonfinite);
    GOLF_LAUNCH_CHECK();
    if (p.NP > 0) {  // one refinement sweep in delta form (see fwdq_body, MODE 2): defects, their scan added to S
        float* dfc = (float*)(ws + p.off_z2);
        hipLaunchKernelGGL((lpc_fwdq_kernel<W, NT, 2>), dim3((unsigned)ceil_div(p.NP, 16), B), dim3(64), 0, st, ex,
                           ex_stride, gain, a, (const float*)S, dfc, (int64_t)0, T, F, M, hop, p.L, p.NP, p.NC,
                           (const float*)nullptr, tier);
        GOLF_LAUNCH_CHECK();
        hipLaunchKernelGGL((lpc_p2_scan_kernel<W, NT, D, true>), dim3(B), dim3(64), 0, st, (const float*)PhiT,
                           (const float*)dfc, S, p.NC, p.NP, B, tier, Phi64);
        GOLF_LAUNCH_CHECK();
    }
    const int gxf = (int)ceil_div(p.NC, 16);
    hipLaunchKernelGGL((lpc_fwdq_final_kernel<W, NT>), dim3((unsigned)gxf, B), dim3(64), 0, st, ex, ex_stride, gain, a,
                       (const float*)S, y, y_stride, T, F, M, hop, p.L, p.NC, p.NP > 0 ? nonfinite : (unsigned*)nullptr);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

// The end of both backwards: g -> g_ex and the hat-weighted correlations per segment, then the segment -> frame reduction.
static int launch_grad_tail(const SsPlan& p, const float* y, int64_t y_stride, const float* ex, int64_t ex_stride,
                            const float* gain, float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T,
                            int F, int M, int hop, char* ws, int tail, hipStream_t st) {
    const float* gbuf = (const float*)(ws + p.off_g);
    float* pa = (float*)(ws + p.off_pa);
    float* pg = (float*)(ws + p.off_pg);
    hipLaunchKernelGGL(lpc_grad_corr_kernel, dim3((unsigned)ceil_div(p.NSEG, 4), B), dim3(256), 0, st, gbuf, (int64_t)T, y,
                       y_stride, ex, ex_stride, gain, g_ex, g_ex_stride, pa, pg, T, F, p.NT, p.W, hop, p.seg, p.NSEG, tail);
    GOLF_LAUNCH_CHECK();
    const int64_t n4 = (int64_t)B * F * (M + 1);
    hipLaunchKernelGGL(lpc_grad_reduce_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, st, (const float*)pa,
                       (const float*)pg, g_a, g_gain, B, F, M, p.W, hop, p.seg, p.NSEG);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

template <int W, int NT>
static int launch_bwd(const SsPlan& p, bool two_level, const float* gy, int64_t gy_stride, const float* y, int64_t y_stride,
                      const float* ex, int64_t ex_stride, const float* gain, const float* a, float* g_ex,
                      int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T, int F, int M, int hop, char* ws,
                      int tail, hipStream_t st) {
    const float* Phi = (const float*)(ws + p.off_phi);
    float* zadj = (float*)(ws + p.off_zadj);
    float* lam = (float*)(ws + p.off_lam);
    float* gbuf = (float*)(ws + p.off_g);
    float* dadj = (float*)(ws + p.off_dadj);
    const unsigned* tier = p.NP > 0 ? (const unsigned*)(ws + p.off_tier) : nullptr;   // as the forward left them
    const double* Phi64 = (const double*)(ws + p.off_phi64);
    constexpr int D = 8;
    const dim3 gq((unsigned)ceil_div(p.NC, 16), B);
    if constexpr (NT <= 24) {
        if (two_level) {   // two-level adjoint scan + refinement sweep (see lpc_adjq2_kernel)
            const float* MTt = (const float*)(ws + p.off_mtT);   // written by the (training) forward's pre-pass
            float* Wz = (float*)(ws + p.off_wadj);
            float* Wd = Wz + (size_t)B * p.NG * 32;
            float* L1 = (float*)(ws + p.off_L1);
            // tier 3: the forward's fp64 composites (read transposed), and its response / start-state regions reused for the adjoint
            const double* M64 = (const double*)(ws + p.off_m64);
            double* W64 = (double*)(ws + p.off_v64);
            double* GA64 = (double*)(ws + p.off_g64);
            unsigned* arrived = (unsigned*)(ws + p.off_fixcnt) + 2 * (size_t)B + 1;
            hipLaunchKernelGGL((lpc_adjq2_kernel<W, NT, 0>), gq, dim3(64), 0, st, gy, gy_stride, a, zadj, (int64_t)0, T, F, M,
                               hop, p.L, p.NC, Phi, MTt, (const float*)nullptr, Wz, (const float*)nullptr, p.NP, p.NG, L1,
                               tier, B, Phi64, M64, W64, GA64, arrived, (const float*)zadj);
            GOLF_LAUNCH_CHECK();
            const int gx3 = (int)ceil_div(p.NP, kGroup);
            hipLaunchKernelGGL((lpc_adjq2_kernel<W, NT, 3>), dim3((unsigned)gx3, B + (int)ceil_div(B, gx3)), dim3(64), 0, st,
                               gy, gy_stride, a, dadj, (int64_t)0, T, F, M, hop, p.L, p.NC, Phi, MTt, (const float*)Wz, Wd,
                               (const float*)zadj, p.NP, p.NG, L1, tier, B, Phi64, M64, W64, GA64, arrived, (const float*)zadj);
            GOLF_LAUNCH_CHECK();
            hipLaunchKernelGGL((lpc_adjq2_kernel<W, NT, 1>), gq, dim3(64), 0, st, gy, gy_stride, a, gbuf, (int64_t)T, T, F, M,
                               hop, p.L, p.NC, Phi, MTt, (const float*)Wd, (float*)nullptr, (const float*)dadj, p.NP, p.NG,
                               L1, tier, B, Phi64, M64, W64, GA64, arrived, (const float*)zadj);
            GOLF_LAUNCH_CHECK();
            return launch_grad_tail(p, y, y_stride, ex, ex_stride, gain, g_ex, g_ex_stride, g_gain, g_a, B, T, F, M, hop, ws, tail, st);
        }
    }
    // flat adjoint scan, with the same refinement sweep in delta form
    hipLaunchKernelGGL((lpc_adjq_kernel<W, NT, 0>), gq, dim3(64), 0, st, gy, gy_stride, a, (const float*)nullptr,
                       zadj, (int64_t)0, T, F, M, hop, p.L, p.NC, tier);
    GOLF_LAUNCH_CHECK();
    hipLaunchKernelGGL((lpc_adj_scan_kernel<W, NT, D, false>), dim3(2 * B), dim3(64), 0, st, Phi, (const float*)zadj, lam,
                       p.NC, p.NP, B, tier, Phi64);
    GOLF_LAUNCH_CHECK();
    if (p.NP > 0) {
        hipLaunchKernelGGL((lpc_adjq_kernel<W, NT, 2>), gq, dim3(64), 0, st, gy, gy_stride, a, (const float*)lam, dadj,
                           (int64_t)0, T, F, M, hop, p.L, p.NC, tier);
        GOLF_LAUNCH_CHECK();
        hipLaunchKernelGGL((lpc_adj_scan_kernel<W, NT, D, true>), dim3(B), dim3(64), 0, st, Phi, (const float*)dadj, lam,
                           p.NC, p.NP, B, tier, Phi64);
        GOLF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((lpc_adjq_kernel<W, NT, 1>), gq, dim3(64), 0, st, gy, gy_stride, a, (const float*)lam, gbuf,
                       (int64_t)T, T, F, M, hop, p.L, p.NC, (const unsigned*)nullptr);
    GOLF_LAUNCH_CHECK();
    return launch_grad_tail(p, y, y_stride, ex, ex_stride, gain, g_ex, g_ex_stride, g_gain, g_a, B, T, F, M, hop, ws, tail, st);
}

// The serial forward, 8 or 4 lanes per utterance; STATE (golf_ltv_allpole_fwd_state_f32): from and into a carried state.
// Eight lanes per utterance while that leaves at most one wave per SIMD (the wave's time per sample falls from ~19 to ~14
// instructions): measured 2673 -> 2381 us at B = 2048, 2785 -> 2481 at 8192; at 16 384 (two waves per SIMD) the quad wins,
// 3071 vs 3351 -- there the chip is busy either way and the quad does the least total work
template <int W, int NT, int LPU, bool STATE>
static int serial_fwd_lanes(const float* ex, int64_t ex_stride, const float* gain, const float* a, float* y, int64_t y_stride,
                             int B, int T, int F, int M, int hop, float* state, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(B, 256 / LPU));
    if constexpr (STATE) {
        hipLaunchKernelGGL((lpc_serial_fwd_state_kernel<W, NT, LPU>), grid, dim3(256), 0, st, ex, ex_stride, gain, a, y,
                           y_stride, B, T, F, M, hop, state);
    } else {
        hipLaunchKernelGGL((lpc_serial_fwd_kernel<W, NT, LPU>), grid, dim3(256), 0, st, ex, ex_stride, gain, a, y, y_stride,
                           B, T, F, M, hop);
    }
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}
template <int W, int NT, bool STATE>
static int launch_serial_fwd(std::bool_constant<STATE>, const SsPlan& p, const float* ex, int64_t ex_stride, const float* gain, const float* a,
                             float* y, int64_t y_stride, int B, int T, int F, int M, int hop, float* state, hipStream_t st) {
    constexpr bool can8 = W % 8 == 0 && W % ((NT + 7) / 8) == 0;
    if constexpr (can8) {
        if ((int64_t)B * 8 <= (int64_t)64 * 1024)
            return serial_fwd_lanes<W, NT, 8, STATE>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
    }
    return serial_fwd_lanes<W, NT, 4, STATE>(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
}

template <int W, int NT>
static int launch_serial_bwd(const SsPlan& p, const float* gy, int64_t gy_stride, const float* y, int64_t y_stride,
                             const float* ex, int64_t ex_stride, const float* gain, const float* a, float* g_ex,
                             int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T, int F, int M, int hop,
                             char* ws, int tail, hipStream_t st) {
    hipLaunchKernelGGL((lpc_serial_adj_kernel<W, NT>), dim3((unsigned)ceil_div(B, 64)), dim3(256), 0, st, gy, gy_stride,
                       a, (float*)(ws + p.off_g), (int64_t)T, B, T, F, M, hop);
    GOLF_LAUNCH_CHECK();
    return launch_grad_tail(p, y, y_stride, ex, ex_stride, gain, g_ex, g_ex_stride, g_gain, g_a, B, T, F, M, hop, ws, tail, st);
}

// One case per (W, NT) instantiation of lpc_ss_plan.h's table.
#define GOLF_SS_CASE(w, nt, FN, ...) case (w) * 100 + (nt): return FN<w, nt>(__VA_ARGS__);
#define GOLF_SS_DISPATCH(FN, ...)                                \
    switch (p.W * 100 + p.NT) {                                  \
        GOLF_SS_INSTANCES(GOLF_SS_CASE, FN, __VA_ARGS__)         \
        default: break;                                          \
    }

static int ss_mode(int flags) {
    return (flags & GOLF_SS_SERIAL) ? GOLF_SS_SERIAL : ((flags & GOLF_SS_CHUNKED) ? GOLF_SS_CHUNKED : 0);
}
static bool plan_fast(int B, int T, int F, int M, int hop, SsPlan* p, int flags = 0) {
    return make_ss_plan(B, T, F, M, hop, p, ss_mode(flags));
}

}  // namespace golf

using namespace golf;

static int check_ws(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255))
        return fail(GOLF_EWORKSPACE, "%s: workspace needs %zu bytes, 256-aligned (got %zu)", who, need, ws_bytes);
    return GOLF_OK;
}

static int check_ss_args(int B, int T, int F, int M, int hop) {
    if (B < 1 || T < 1 || F < 1 || M < 1 || hop < 1) return fail(GOLF_EINVAL, "ltv_allpole: non-positive size");
    if (M > 64) return fail(GOLF_EUNSUPPORTED, "ltv_allpole: M=%d > 64", M);
    if ((int64_t)T > (int64_t)(F - 1) * hop + 1)
        return fail(GOLF_EINVAL, "ltv_allpole: T=%d exceeds (F-1)*hop+1=%lld", T, (long long)(F - 1) * hop + 1);
    return GOLF_OK;
}

extern "C" size_t golf_ltv_allpole_workspace_bytes_ex(int B, int T, int F, int M, int hop, int flags) {
    SsPlan p;
    if (B < 1 || T < 1 || F < 1 || M < 1 || hop < 1) return 0;
    if (!plan_fast(B, T, F, M, hop, &p, flags)) return any_ws_bytes(B, T);   // no ring plan: the adjoint's g (lpc_any.hip)
    return p.total;
}

// Default path selection.  Below the serial threshold the chunked layout is returned, which also covers a forced
// GOLF_SS_SERIAL call (its buffers are a subset); at or above it only the (much smaller) serial layout.
extern "C" size_t golf_ltv_allpole_workspace_bytes(int B, int T, int F, int M, int hop) {
    return golf_ltv_allpole_workspace_bytes_ex(B, T, F, M, hop, 0);
}

extern "C" int golf_ltv_allpole_transitions_f32(const float* a, int B, int T, int F, int M, int hop, void* ws,
                                                size_t ws_bytes, int flags, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!a) return fail(GOLF_EINVAL, "ltv_allpole_transitions: null pointer");
    SsPlan p;
    if (!plan_fast(B, T, F, M, hop, &p, flags)) return GOLF_OK;  // no ring plan (lpc_any.hip): no transition matrices
    if (p.serial) return GOLF_OK;                                 // nor has the batch-parallel serial path
    if (int rc = check_ws("ltv_allpole_transitions", ws, ws_bytes, p.total)) return rc;
    const SsChain t = ss_transitions(p, B, flags, device_cu_count());
    GOLF_SS_DISPATCH(launch_transitions, p, t, t.owed != SsOwed::None, a, B, F, M, hop, (char*)ws, (hipStream_t)stream)
    return fail(GOLF_EUNSUPPORTED, "ltv_allpole_transitions: no kernel for W=%d NT=%d", p.W, p.NT);
}

extern "C" int golf_ltv_allpole_status_u32(const void* ws, size_t ws_bytes, int B, int T, int F, int M, int hop, int flags,
                                           uint32_t* out, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!out) return fail(GOLF_EINVAL, "ltv_allpole_status: null pointer");
    hipStream_t st = (hipStream_t)stream;
    SsPlan p;
    // the serial and the wave-per-utterance algorithms have no transition matrices: nothing is recomputed, all four words are 0
    if (!plan_fast(B, T, F, M, hop, &p, flags) || !ss_has_maps(p)) {
        hipLaunchKernelGGL(lpc_status_zero_kernel, dim3(1), dim3(64), 0, st, (unsigned*)out);
        GOLF_LAUNCH_CHECK();
        return GOLF_OK;
    }
    if (int rc = check_ws("ltv_allpole_status", ws, ws_bytes, p.total)) return rc;
    const char* w = (const char*)ws;
    hipLaunchKernelGGL(lpc_status_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)(w + p.off_tier),
                       (const unsigned*)(w + p.off_status), (const unsigned*)(w + p.off_fixcnt),
                       (const float*)(w + p.off_pmax), B, p.NP, (unsigned*)out);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

extern "C" int golf_ltv_allpole_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a,
                                        float* y, int64_t y_stride, int B, int T, int F, int M, int hop, void* ws,
                                        size_t ws_bytes, int flags, void* side_stream, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!ex || !gain || !a || !y) return fail(GOLF_EINVAL, "ltv_allpole_fwd: null pointer");
    if (ex_stride < T || y_stride < T) return fail(GOLF_EINVAL, "ltv_allpole_fwd: row stride < T");
    hipStream_t st = (hipStream_t)stream;
    SsPlan p;
    if (!plan_fast(B, T, F, M, hop, &p, flags))   // no ring plan for (M, hop, F): one wave per utterance, no workspace
        return launch_any_fwd(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, nullptr, st);
    if (p.serial && !serial_strides_ok(ex_stride, y_stride)) {
        if (flags & GOLF_SS_SERIAL) return fail(GOLF_EUNSUPPORTED, "ltv_allpole_fwd: serial path needs row strides < 2^24");
        plan_fast(B, T, F, M, hop, &p, GOLF_SS_CHUNKED);
    }
    if (int rc = check_ws("ltv_allpole_fwd", ws, ws_bytes, p.total)) return rc;
    if (p.serial) {
        GOLF_SS_DISPATCH(launch_serial_fwd, std::false_type{}, p, ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, nullptr, st)
        return fail(GOLF_EUNSUPPORTED, "ltv_allpole_fwd: no kernel for W=%d NT=%d", p.W, p.NT);
    }
    hipStream_t side = (hipStream_t)side_stream;
    if (side == st) side = nullptr;
    const int n_cu = device_cu_count();
    const SsChain c = ss_chain(p, B, flags, side != nullptr, n_cu);
    GOLF_SS_DISPATCH(launch_fwd, p, c, n_cu, ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, (char*)ws, side, st)
    return fail(GOLF_EUNSUPPORTED, "ltv_allpole_fwd: no kernel for W=%d NT=%d", p.W, p.NT);
}

extern "C" int golf_ltv_allpole_fwd_state_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a, float* y,
                                              int64_t y_stride, int B, int T, int F, int M, int hop, float* state,
                                              void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!ex || !gain || !a || !y || !state) return fail(GOLF_EINVAL, "ltv_allpole_fwd_state: null pointer");
    if (ex_stride < T || y_stride < T) return fail(GOLF_EINVAL, "ltv_allpole_fwd_state: row stride < T");
    hipStream_t st = (hipStream_t)stream;
    SsPlan p;
    if (!make_ss_plan(B, T, F, M, hop, &p, GOLF_SS_SERIAL))
        return launch_any_fwd(ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st);
    if (!serial_strides_ok(ex_stride, y_stride))
        return fail(GOLF_EUNSUPPORTED, "ltv_allpole_fwd_state: serial path needs row strides < 2^24");
    GOLF_SS_DISPATCH(launch_serial_fwd, std::true_type{}, p, ex, ex_stride, gain, a, y, y_stride, B, T, F, M, hop, state, st)
    return fail(GOLF_EUNSUPPORTED, "ltv_allpole_fwd_state: no kernel for W=%d NT=%d", p.W, p.NT);
}

extern "C" int golf_ltv_allpole_bwd_f32(const float* gy, int64_t gy_stride, const float* y, int64_t y_stride,
                                        const float* ex, int64_t ex_stride, const float* gain, const float* a,
                                        float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a, int B, int T,
                                        int F, int M, int hop, void* ws, size_t ws_bytes, int flags, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!gy || !y || !ex || !gain || !a || !g_ex || !g_gain || !g_a)
        return fail(GOLF_EINVAL, "ltv_allpole_bwd: null pointer");
    if (gy_stride < T || y_stride < T || ex_stride < T || g_ex_stride < T)
        return fail(GOLF_EINVAL, "ltv_allpole_bwd: row stride < T");
    SsPlan p;
    hipStream_t st = (hipStream_t)stream;
    if (!plan_fast(B, T, F, M, hop, &p, flags)) {   // no ring plan: adjoint by one wave per utterance, g in the workspace
        if (int rc = check_ws("ltv_allpole_bwd", ws, ws_bytes, any_ws_bytes(B, T))) return rc;
        return launch_any_bwd(gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, g_ex, g_ex_stride, g_gain, g_a, B, T, F, M,
                              hop, (char*)ws, (flags & GOLF_SS_ZERO_TAIL) ? g_ex_stride - (int64_t)T : 0, st);
    }
    if (int rc = check_ws("ltv_allpole_bwd", ws, ws_bytes, p.total)) return rc;
    const int64_t tail64 = (flags & GOLF_SS_ZERO_TAIL) ? g_ex_stride - (int64_t)T : 0;
    if (tail64 > 0x7fffffff) return fail(GOLF_EINVAL, "ltv_allpole_bwd: GOLF_SS_ZERO_TAIL with a row stride beyond 2^31");
    const int tail = (int)tail64;
    if (p.serial && !serial_strides_ok(gy_stride, gy_stride))
        return fail(GOLF_EUNSUPPORTED, "ltv_allpole_bwd: serial path needs row strides < 2^24");
    if (p.serial) {
        GOLF_SS_DISPATCH(launch_serial_bwd, p, gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, g_ex, g_ex_stride,
                         g_gain, g_a, B, T, F, M, hop, (char*)ws, tail, st)
        return fail(GOLF_EUNSUPPORTED, "ltv_allpole_bwd: no kernel for W=%d NT=%d", p.W, p.NT);
    }
    const bool two_level = ss_two_level(p, B, flags, device_cu_count());   // the forward's boundary scan: it left the composites
    GOLF_SS_DISPATCH(launch_bwd, p, two_level, gy, gy_stride, y, y_stride, ex, ex_stride, gain, a, g_ex, g_ex_stride, g_gain, g_a,
                     B, T, F, M, hop, (char*)ws, tail, st)
    return fail(GOLF_EUNSUPPORTED, "ltv_allpole_bwd: no kernel for W=%d NT=%d", p.W, p.NT);
}

extern "C" int golf_ltv_inverse_f32(const float* y, int64_t y_stride, const float* a, float* e, int64_t e_stride,
                                    int B, int T, int F, int M, int hop, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!y || !a || !e) return fail(GOLF_EINVAL, "ltv_inverse: null pointer");
    if (y_stride < T || e_stride < T) return fail(GOLF_EINVAL, "ltv_inverse: row stride < T");
    const int64_t n = (int64_t)B * T;
    hipLaunchKernelGGL(lpc_inverse_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, y,
                       y_stride, a, e, e_stride, B, T, F, M, hop);
    GOLF_LAUNCH_CHECK();
    return GOLF_OK;
}

extern "C" int golf_ltv_inverse_bwd_f32(const float* g_e, int64_t g_e_stride, const float* y, int64_t y_stride,
                                        const float* a, float* g_y, int64_t g_y_stride, float* g_a, int B, int T,
                                        int F, int M, int hop, void* stream) {
    if (int rc = check_ss_args(B, T, F, M, hop)) return rc;
    if (!g_e || !y || !a) return fail(GOLF_EINVAL, "ltv_inverse_bwd: null pointer");
    if (g_e_stride < T || y_stride < T || (g_y && g_y_stride < T))
        return fail(GOLF_EINVAL, "ltv_inverse_bwd: row stride < T");
    hipStream_t st = (hipStream_t)stream;
    if (g_y) {
        const int64_t n = (int64_t)B * T;
        hipLaunchKernelGGL(lpc_inverse_bwd_y_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, g_e,
                           g_e_stride, a, g_y, g_y_stride, B, T, F, M, hop);
        GOLF_LAUNCH_CHECK();
    }
    if (g_a) {
        hipLaunchKernelGGL(lpc_inverse_bwd_a_kernel, dim3((unsigned)F, B), dim3(64), 0, st, g_e, g_e_stride, y,
                           y_stride, g_a, T, F, M, hop);
        GOLF_LAUNCH_CHECK();
    }
    return GOLF_OK;
}
