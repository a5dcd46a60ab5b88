// Host-side plan of the sample-wise all-pole filter: the workspace layout and which launches a call runs.  No HIP here, so
// the policy is tested on a CPU (tests/test_ss_plan_host.py); the launchers in lpc_ss.hip execute it and decide nothing.
#pragma once
#include <cstddef>
#include <cstdint>

#include "golf_amd.h"

namespace golf {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- chunk plan shared by forward and backward of the sample-wise filter -------------------
struct SsPlan {
    int W;      // ring/unroll width: W >= M+1, hop % W == 0  (0 => no ring plan: lpc_any.hip)
    int NT;     // taps computed (>= M, zero padded)
    int L;      // chunk length: L % W == 0 and (L % hop == 0 || hop % L == 0)
    int NC;     // chunks per utterance = ceil(T/L)
    int NP;     // chunks that own a transition matrix = NC-1
    int seg;    // gradient segment length = min(L, hop)
    int NSEG;   // ceil(T/seg)
    bool serial;  // batch-parallel serial kernels (large batches): no transition matrices / boundary states in ws
    // workspace offsets (bytes)
    int NG, GS; // two-level boundary scan: NG groups of GS chunk maps (NG == 0: flat scan)
    size_t off_phi, off_phiT, off_z, off_E, off_z2, off_S, off_zadj, off_lam, off_g, off_pa, off_pg, off_mt, off_gv, off_pmax, total;
    // conditioning tiers (see lpc_fixup_kernel): per-utterance tier words, first-pass chunk start states of the two-level
    // scan (the delta-form refinement adds its correction to exactly these), the status words, and -- touched only for the
    // rare tier-3 utterances -- the transition matrices as doubles
    size_t off_tier, off_S1, off_status, off_phi64, off_fixcnt;
    size_t off_m64, off_v64, off_g64;   // tier 3 on the two-level path: fp64 group composites, group responses, group start states
    size_t off_mtT, off_L1, off_wadj, off_dadj;   // backward: two-level adjoint scan
    size_t off_gflag;   // merged chunk pass (lpc_fwdq2m_kernel): [B][NG] "defect response published" + [B] "fp64 states ready" words
};

// (W, NT) kernel instantiations: NT taps computed (zero padded above M), ring width W >= NT+1
// (the adjoint ring needs one free slot), W | hop.  The plan's table and the launchers' dispatch both come from this list.
#define GOLF_SS_TABLE(X, ...)                                                                                          \
    X(8, 2, __VA_ARGS__) X(8, 4, __VA_ARGS__) X(8, 6, __VA_ARGS__) X(16, 8, __VA_ARGS__) X(16, 12, __VA_ARGS__)        \
    X(16, 14, __VA_ARGS__) X(24, 8, __VA_ARGS__) X(24, 12, __VA_ARGS__) X(24, 16, __VA_ARGS__) X(24, 20, __VA_ARGS__)  \
    X(24, 22, __VA_ARGS__) X(32, 16, __VA_ARGS__) X(32, 22, __VA_ARGS__) X(32, 26, __VA_ARGS__) X(32, 30, __VA_ARGS__) \
    X(40, 22, __VA_ARGS__) X(40, 26, __VA_ARGS__) X(40, 32, __VA_ARGS__) X(40, 38, __VA_ARGS__)
#ifdef GOLF_SS_ONLY_24_22   // dev builds (tools/build_variant.sh): only the benchmark's instantiation, a 10x shorter compile
#define GOLF_SS_INSTANCES(X, ...) X(24, 22, __VA_ARGS__)
#else
#define GOLF_SS_INSTANCES(X, ...) GOLF_SS_TABLE(X, __VA_ARGS__)
#endif
struct WNT { int W, NT; };
#define GOLF_SS_ROW(w, nt, ...) {w, nt},
constexpr WNT kTable[] = {GOLF_SS_TABLE(GOLF_SS_ROW, ~)};
#undef GOLF_SS_ROW

// Batch size from which the batch-parallel serial kernels replace the chunked scan (build parameter).
// Chunking buys parallelism in time at the price of (M+2)-fold arithmetic; once the batch alone fills the chip's wave
// slots that price stops paying.  Measured crossover on MI355X (M=22, T=47761): DESIGN.md §4.1.
#ifndef GOLF_SS_SERIAL_MIN_BATCH
#define GOLF_SS_SERIAL_MIN_BATCH 2048
#endif

constexpr int kGroup = 16;   // chunk maps per group = chunks per wave of the chunk kernels
constexpr int kMergedMaxGroups = 32;   // (the waiting wave stages the earlier groups' responses in LDS: 128 bytes each)

inline bool make_ss_plan(int B, int T, int F, int M, int hop, SsPlan* p, int mode = 0) {
    p->W = 0;
    p->NT = 0;
    // mode: 0 = by batch size, GOLF_SS_SERIAL / GOLF_SS_CHUNKED force one; rows of 16 utterances must fit a 2 GB
    // buffer descriptor
    p->serial = mode == GOLF_SS_SERIAL || (mode != GOLF_SS_CHUNKED && B >= GOLF_SS_SERIAL_MIN_BATCH);
    if (F >= 2) {
        for (const WNT& e : kTable) {
            if (e.NT < M || hop % e.W != 0) continue;
            if (p->W == 0 || e.NT < p->NT || (e.NT == p->NT && e.W < p->W)) { p->W = e.W; p->NT = e.NT; }
        }
    }
    if (p->W == 0) { p->total = 256; return false; }
    const int W = p->W;
    int L;
    const int target = 240;
    if (hop >= target) {
        L = W;
        for (int cand = W; cand <= 256 && cand <= hop; cand += W)
            if (hop % cand == 0) L = cand;
    } else {
        L = hop * (target / hop);
    }
    // (Shorter chunks were tried in round 4 with an env override here: L = 120 at hop 240 halves the chunk recursion -- flat-scan
    //  chunk passes 13 / 10 us instead of ~20 -- but the two-level passes stay at 26 / 21 us because their prologues grow with the
    //  group count (25 groups: 24 fold steps), the pre-pass goes 16 -> 30 us and the maps double: one batch alone 143 vs 129 us,
    //  four in flight 87.9 vs 69.3.)
    p->L = L;
    p->NC = (int)ceil_div(T, L);
    p->NP = p->NC - 1;
    p->seg = L < hop ? L : hop;
    p->NSEG = (int)ceil_div(T, p->seg);
    size_t o = 0;
    if (p->serial) {   // batch-parallel serial path: no transition matrices, no boundary states
        p->off_phi = p->off_phiT = p->off_z = p->off_E = p->off_z2 = p->off_S = p->off_zadj = p->off_lam = 0;
        p->NG = p->GS = 0;
        p->off_mt = p->off_gv = p->off_pmax = 0;
        p->off_tier = p->off_S1 = p->off_status = p->off_phi64 = p->off_fixcnt = 0;
        p->off_m64 = p->off_v64 = p->off_g64 = 0;
        p->off_mtT = p->off_L1 = p->off_wadj = p->off_dadj = 0;
        p->off_gflag = 0;
        p->off_g = o;    o = align_up(o + sizeof(float) * (size_t)B * T, 256);
        p->off_pa = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NSEG * 2 * W, 256);
        p->off_pg = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NSEG * 2, 256);
        p->total = o;
        return true;
    }
    p->off_phi = o;  o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1) * p->NT * W, 256);
    p->off_phiT = o; o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1) * p->NT * W, 256);
    p->off_z = o;    o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1) * W, 256);
    p->off_E = o;    o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1) * W, 256);
    p->off_z2 = o;   o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1) * W, 256);
    p->off_S = o;    o = align_up(o + sizeof(float) * (size_t)B * p->NC * 64, 256);
    p->off_zadj = o; o = align_up(o + sizeof(float) * (size_t)B * p->NC * W, 256);
    p->off_lam = o;  o = align_up(o + sizeof(float) * (size_t)B * p->NC * 64, 256);
    p->off_g = o;    o = align_up(o + sizeof(float) * (size_t)B * T, 256);
    p->off_pa = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NSEG * 2 * W, 256);
    p->off_pg = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NSEG * 2, 256);
    p->off_pmax = o; o = align_up(o + sizeof(float) * (size_t)B * (p->NP > 0 ? p->NP : 1), 256);   // max |Phi_c| per chunk
    p->off_tier = o; o = align_up(o + sizeof(unsigned) * ((size_t)B * 2 + 2), 256);   // conditioning tier + hot-chunk count per utterance; [2B] scan kind of the forward, [2B+1] backward mismatch
    p->off_status = o; o = align_up(o + sizeof(unsigned) * 8, 256);              // status words (non-finite output flag)
    p->off_fixcnt = o; o = align_up(o + sizeof(unsigned) * ((size_t)B * 5 + 1), 256);   // fix-up units completed / claimed per utterance; [2B]: a wait for the fix-up ran out; [2B+1 .. 3B]: groups of a tier-3 utterance that have their fp64 composite; [3B+1 .. 4B]: largest partial product of those composites; [4B+1 .. 5B]: 1 = that utterance's fp64 states come from the flat scan
    // two-level boundary scan (lpc_group_prepass_kernel + lpc_fwdq2_kernel): worth it from ~48 chunk maps on, and the
    // chunk kernels' prologue keeps rows of up to 24 state components in its prefetch rings
    p->NG = 0;
    p->GS = 0;
    p->off_mt = p->off_gv = o;
    if (p->NP >= 48 && p->NT <= 24) {
        p->GS = 16;                                  // = the 16 chunks a wave of the chunk kernels owns
        p->NG = (int)ceil_div(p->NP, p->GS);
        p->off_mt = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NG * p->NT * W, 256);
        p->off_gv = o; o = align_up(o + sizeof(float) * (size_t)B * p->NG * 32 * 2, 256);   // group responses (z, defects)
    }
    p->off_S1 = o;   o = align_up(o + sizeof(float) * (size_t)B * p->NC * 32, 256);   // first-pass chunk start states (two-level)
    // backward, two-level adjoint scan: transposed composites, first-pass adjoint states L1 (rows -1 .. NP), group responses
    // (zadj, defects), defects
    p->off_mtT = o;  o = align_up(o + sizeof(float) * (size_t)B * (p->NG > 0 ? p->NG : 1) * p->NT * W, 256);
    p->off_L1 = o;   o = align_up(o + sizeof(float) * (size_t)B * (p->NC + 1) * 32, 256);
    p->off_wadj = o; o = align_up(o + sizeof(float) * (size_t)B * (p->NG > 0 ? p->NG : 1) * 32 * 2, 256);
    p->off_dadj = o; o = align_up(o + sizeof(float) * (size_t)B * p->NC * W, 256);
    // transition matrices as doubles, [b][c][j][i] (trajectory-major), written and read only for tier-3 utterances: the
    // allocation is never touched otherwise (27 MB at B = 32 x 2 s)
    p->off_phi64 = o; o = align_up(o + sizeof(double) * (size_t)B * (p->NP > 0 ? p->NP : 1) * p->NT * W, 256);
    // ... and, on the two-level path, their group composites / group responses / group start states as doubles
    p->off_m64 = o;  o = align_up(o + sizeof(double) * (size_t)B * (p->NG > 0 ? p->NG : 1) * p->NT * W, 256);
    p->off_v64 = o;  o = align_up(o + sizeof(double) * (size_t)B * (p->NG > 0 ? p->NG : 1) * 32, 256);
    p->off_g64 = o;  o = align_up(o + sizeof(double) * (size_t)B * (p->NG + 1) * 32, 256);
    p->off_gflag = o; o = align_up(o + sizeof(unsigned) * (size_t)B * (p->NG + 1), 256);   // zeroed by every forward's pre-pass launch
    p->total = o;
    return true;
}

// The serial and the wave-per-utterance algorithms, and an utterance of one chunk, have no transition matrices.
inline bool ss_has_maps(const SsPlan& p) { return p.W > 0 && !p.serial && p.NP > 0; }

// The two-level boundary scan buys latency with (utterance x group) waves whose prologues hold a SIMD's registers
// (one wave per SIMD).  Measured with 4 batches in flight / one batch alone, two-level vs flat, us per step:
//   B = 32: 71.9 vs 71.6 / 140 vs 166;  B = 48: 101 vs 94 / 192 vs 214;  B = 64: 132 vs 117 / 212 vs 229;
//   (with the earlier fp32 composites) B = 96: 204 vs 166 / 300 vs 286;  B = 256: 537 vs 437 / 629 vs 515
// so it is taken while B x NG stays below half the SIMD count (B <= 39 at 2 s), where it costs the pipelined rate nothing.
// (Build parameter GOLF_SS_TWO_LEVEL_WAVES: a fixed cap on B x NG instead; 0 = 2 x the CU count.)
// Depends on the plan, B, GOLF_SS_FLAT_SCAN and the CU count alone: the backward reads the composites this choice left.
#ifndef GOLF_SS_TWO_LEVEL_WAVES
#define GOLF_SS_TWO_LEVEL_WAVES 0
#endif
inline bool ss_two_level(const SsPlan& p, int B, int flags, int n_cu) {
    const int64_t cap = GOLF_SS_TWO_LEVEL_WAVES > 0 ? (int64_t)GOLF_SS_TWO_LEVEL_WAVES : (int64_t)2 * n_cu;
    return p.NG > 0 && !(flags & GOLF_SS_FLAT_SCAN) && (int64_t)B * p.NG <= cap;
}

// golf_ltv_allpole_fwd_f32 (ss_chain): maps, zero-state pass, join, then pre-pass + chunk passes (two_level) or fix-up + flat
// scans + final pass.  golf_ltv_allpole_transitions_f32 (ss_transitions): the maps (fp32, or lpc_p1h + transpose), then `owed`.
enum class SsMaps {
    None,             // the plan has none (one chunk)
    Have,             // already in the workspace (GOLF_SS_HAVE_TRANSITIONS)
    Own,              // a launch of their own (lpc_p1f): fix-up, composites and the zero-state pass follow in the pre-pass launch
    WithZeroState,    // one launch with the zero-state pass (lpc_p1fz, or lpc_p1hz + transpose)
    ViaTransitions,   // launch_transitions with its composites: on the side stream, or on the main one (GOLF_SS_SPLIT_P1)
};
enum class SsZeroState { None, WithMaps, InPrepass, Own };   // Own: lpc_fwdq MODE 0 (prepared transitions, side stream, SPLIT_P1)
enum class SsOwed { None, Prepass, Fixup };   // fix-up (+ composites) run by this call: in the pre-pass launch / launch_fixup
struct SsChain {
    bool fast;          // fp32 maps (GOLF_SS_FAST_TRANSITIONS); otherwise from fp64 trajectories: accurate already
    bool training;      // the backward follows: keep what it needs
    bool two_level;     // two-level boundary scan (group composites, lpc_group_prepass_kernel); otherwise flat
    int k1, k2;         // fix-up workgroups per utterance that lead / trail the grid (fixup_kf)
    int nf, nu, nz;     // two-level: fix-up, composite and response workgroups of the pre-pass launch
    SsMaps maps; SsZeroState zero_state;   // who produces the maps; where the zero-state pass runs
    SsOwed owed;        // None: launch_transitions or the caller's transitions call ran them (transitions call: MAPS_ONLY)
    bool fork, join;    // the maps go to the side stream; the main stream waits for it before the boundary scan
    bool merged;        // both chunk passes as one launch (lpc_fwdq2m_kernel); otherwise a pair of lpc_fwdq2 launches,
    bool thin;          // ... in their THIN form
    int parts;          // of lpc_group_prepass_kernel: 2 zero-state group responses | 1 fix-up + composites | 4 zero-state pass
};

// fix-up workgroups (4 waves of 16 units) per utterance: KF1 lead the grid (the guarantee), KF2 trail it (the speed);
// together at most one pass over all units of an utterance.  Build parameters GOLF_SS_FIXUP_KF1 (> 0) / GOLF_SS_FIXUP_KF2 (>= 0)
// fix either count; the defaults take the rules below.
#ifndef GOLF_SS_FIXUP_KF1
#define GOLF_SS_FIXUP_KF1 0
#endif
#ifndef GOLF_SS_FIXUP_KF2
#define GOLF_SS_FIXUP_KF2 -1
#endif
inline void fixup_kf(const SsPlan& p, bool lone_batch, SsChain* s) {
    const int64_t all = ceil_div((int64_t)p.NP * p.NT, 64);   // workgroups that cover every unit in one pass
    // Round 6 (G2 = 8: a hot utterance of the recipe now has 50 - 150 hot chunks, not 5 - 20): a caller WITHOUT batches in flight
    // (no GOLF_SS_THROUGHPUT, two-level path) gets (10, 38) -- trailing workgroups cost a lone batch nothing, leading ones cost its
    // cold utterances.  One batch alone over 32 recipe seeds, mean / cold / hot / tier 3, us: (6, 10) 140.4 / 123.2 / 147.6 / 170.3;
    // (10, 22) 137.3 / 122.4 / 142.9 / 164.1; (10, 38) 136.2 / 121.8 / 142.2 / 161.1; (8, 48) 136.8; (10, 59) 137.3; (6, 63) 137.8;
    // (16, 32) 139.0 / 128.8 / ..; (32, 0) 140.1 / 131.1.  With four batches in flight the same settings LOSE (headline 68.7 ->
    // 70.2 - 72.6 us/step): there every idle workgroup is dispatch cost, and (6, 10) stays.
    int k1 = GOLF_SS_FIXUP_KF1 > 0 ? GOLF_SS_FIXUP_KF1 : (lone_batch ? 10 : 6);
    if (k1 > all) k1 = (int)(all < 1 ? 1 : all);
    // Every fix-up workgroup that finds nothing to do is dispatch cost, and with several batches in flight that is what
    // counts.  Measured, (KF1, KF2) -> us/step pipelined: B = 256, launch of its own (18 hot utterances + one tier 3 in the
    // four slots; kernel alone in brackets): (6, 10) 452 [77], (6, 26) 461 [52], (6, 42) 470 [61], (6, 90) 483 [67];
    // B = 32, merged into the pre-pass (headline / driver's 20 steps / recipe_stream): (6, 10) 74.3 / 82.9 / 77.9,
    // (6, 26) 74.9 / 83.5 / 78.4, (6, 42) 75.8 / 86.4 / 80.9.  16 workgroups = 1024 units per pass: one pass for up to 46 hot
    // chunks of an utterance (typical: 5 - 20); a tier-3 utterance (all 199) takes five.
    int64_t k2 = GOLF_SS_FIXUP_KF2 >= 0 ? GOLF_SS_FIXUP_KF2 : (lone_batch ? 38 : 10);
    if (k1 + k2 > all) k2 = all - k1 > 0 ? all - k1 : 0;
    s->k1 = k1; s->k2 = (int)k2;
}

inline SsChain ss_transitions(const SsPlan& p, int B, int flags, int n_cu) {
    SsChain c{};
    c.fast = (flags & GOLF_SS_FAST_TRANSITIONS) != 0;
    c.training = !c.fast || (flags & GOLF_SS_TRAINING);
    c.two_level = ss_two_level(p, B, flags, n_cu);
    fixup_kf(p, c.two_level && !(flags & GOLF_SS_THROUGHPUT), &c);   // the lone-batch rule holds on the two-level path only
    if (c.two_level) { c.nf = B * (c.k1 + c.k2); c.nu = p.NG * B; c.nz = (int)ceil_div(c.nu, 4); }
    const bool maps_only = flags & GOLF_SS_MAPS_ONLY;   // the forward (HAVE | MAPS_ONLY) then runs them
    c.owed = !ss_has_maps(p) || maps_only ? SsOwed::None : c.two_level ? SsOwed::Prepass : SsOwed::Fixup;
    return c;
}

inline SsChain ss_chain(const SsPlan& p, int B, int flags, bool side_stream, int n_cu) {
    SsChain c = ss_transitions(p, B, flags, n_cu);   // the same scan, fix-up and pre-pass figures; who runs what follows
    const bool have = flags & GOLF_SS_HAVE_TRANSITIONS, throughput = flags & GOLF_SS_THROUGHPUT;
    const bool one_stream = !side_stream && !(flags & GOLF_SS_SPLIT_P1);
    const bool maps_only = have && (flags & GOLF_SS_MAPS_ONLY);   // the caller's transitions call left the matrices only
    // Round 4: the zero-state pass inside the pre-pass launch (lpc_group_prepass_kernel `parts` bit 2) -- the transition
    // kernel then needs only the coefficients and is a launch of its own (or part of the oscillator's: MAPS_ONLY).
    const bool zin = c.two_level && c.fast && one_stream && (maps_only || throughput);
    bool owed = false;
    if (ss_has_maps(p)) {
        if (have) { c.maps = SsMaps::Have; owed = maps_only; }
        else if (zin) { c.maps = SsMaps::Own; owed = true; }
        else if (one_stream) { c.maps = SsMaps::WithZeroState; owed = true; }
        else { c.maps = SsMaps::ViaTransitions; c.fork = side_stream; }
        c.zero_state = zin ? SsZeroState::InPrepass : c.maps == SsMaps::WithZeroState ? SsZeroState::WithMaps : SsZeroState::Own;
        c.join = side_stream;
    }
    c.owed = !owed ? SsOwed::None : c.two_level ? SsOwed::Prepass : SsOwed::Fixup;
    if (c.two_level) {
        const int64_t gxf = ceil_div(p.NC, kGroup);
        // One batch alone (latency chain): the two chunk passes as ONE launch.  With batches in flight (GOLF_SS_THROUGHPUT) the
        // pair of thin launches stays: measured 68.4 vs 70.5 us/step -- a wave that lives through both sweeps holds its registers
        // for 44 us, waiting included.
        // ... and only while its whole grid is resident at once (296 VGPRs: one wave per SIMD), which is what its waits rely on
        // (see the kernel's comment).  ss_two_level's own cap (B x NG <= 2 x CUs) keeps today's shapes far below that.
        c.merged = !throughput && p.NG <= kMergedMaxGroups && gxf * (B + ceil_div(B, gxf)) <= (int64_t)4 * n_cu;
        c.thin = throughput;
        c.parts = (owed ? 3 : 2) | (zin ? 4 : 0);
    }
    return c;
}

// Units of the zero-state pass per wave in the launch it shares with the maps' `nblk` workgroups: one workgroup per CU if 4 allow it.
inline int ss_upw(int64_t nblk, int64_t nunit, int n_cu) {
    int upw = 1;
    while (upw < 4 && nblk + ceil_div(nunit, 4 * upw) > n_cu) ++upw;
    return upw;
}

}  // namespace golf
